"""Test-side reference of the full-sum CTC score over a token graph (csrc/ctc_graph_score.hip): an fp64 numpy restatement of the
recurrences of include/rvb.h (rvb_ctc_score_graph), vectorised over nodes and arcs per frame with flat candidate arrays.

States: B_start, and per node j T_j and B_j.  Frame 0: a(B_start) = lp[0][blank], a(T_j) = lp[0][tok_j] where -1 is a predecessor, the
rest -inf.  Frame t: a(B_start) stays; a(B_j) = lse(a'(B_j), a'(T_j)) + lp[t][blank]; a(T_j) = lse(a'(T_j), per predecessor p a'(B_p)
(a'(B_start) for -1) and a'(T_p) if tok_p != tok_j) + lp[t][tok_j].  loglik = lse over the finals of a(B_f), a(T_f) at the last frame.
beta is the mirror image over the successors and includes the emission of its own frame; gamma_t(T_j) = a + beta - lp - loglik.
Per node from g = exp(gamma(T_j)): occupancy, mean_frame, peak_post, peak_frame (first maximum), `second` (the largest posterior at any
other frame) and visit = sum_t [g_t - exp(a_{t-1}(T_j) + beta_t(T_j) - loglik)], the mass that ENTERS T_j at frame t.
No normalisation is needed in fp64 at the sizes the tests use.  Only the T rows of alpha are kept ([T, N] fp64); the backward sweep
reduces on the fly."""
import numpy as np


def _lse_seg(cand, off, seg):
    """log-sum-exp of the segments of cand that start at off (none empty); seg: the segment of each entry.  -inf where all are"""
    m = np.maximum.reduceat(cand, off)
    mm = np.where(np.isneginf(m), 0.0, m)
    with np.errstate(divide="ignore"):
        return mm + np.log(np.add.reduceat(np.exp(cand - mm[seg]), off))


class Plan:
    """the flat candidate lists of one graph.  Forward vector X = [B_start, T_0.., B_0.., -inf]; backward Y = [T_0.., B_0.., -inf]."""

    def __init__(self, tokens, preds, finals, blank=0):
        tok = np.asarray(tokens, np.int64)
        N = len(tok)
        assert N >= 1 and not np.any(tok == blank) and not np.any(tok < 0)
        self.N, self.tok, self.blank = N, tok, blank
        self.fin = np.asarray(finals, bool)
        assert self.fin.any()
        succ = [[] for _ in range(N)]
        self.from_start = np.zeros(N, bool)
        idx, off = [], []
        for j, ps in enumerate(preds):
            assert len(ps) >= 1 and len(set(ps)) == len(ps) and all(-1 <= p < j for p in ps)
            off.append(len(idx))
            idx.append(1 + j)                                    # stay
            for p in ps:
                if p < 0:
                    idx.append(0)
                    self.from_start[j] = True
                else:
                    idx.append(1 + N + p)
                    if tok[p] != tok[j]:
                        idx.append(1 + p)
                    succ[p].append(j)
        self.f_idx, self.f_off = np.array(idx, np.int64), np.array(off, np.int64)
        self.f_seg = np.repeat(np.arange(N), np.diff(np.append(self.f_off, len(idx))))
        self.succ = succ
        ti, to, bi, bo = [], [], [], []
        for j in range(N):
            to.append(len(ti))
            ti += [j, N + j] + [s for s in succ[j] if tok[s] != tok[j]]
            bo.append(len(bi))
            bi += [N + j] + succ[j]
        self.t_idx, self.t_off = np.array(ti, np.int64), np.array(to, np.int64)
        self.t_seg = np.repeat(np.arange(N), np.diff(np.append(self.t_off, len(ti))))
        self.b_idx, self.b_off = np.array(bi, np.int64), np.array(bo, np.int64)
        self.b_seg = np.repeat(np.arange(N), np.diff(np.append(self.b_off, len(bi))))

    def first(self, lp):
        X = np.full(2 * self.N + 2, -np.inf)
        X[0] = lp[0, self.blank]
        X[1:1 + self.N][self.from_start] = lp[0, self.tok][self.from_start]
        return X

    def step(self, X, row):
        N = self.N
        Tn = _lse_seg(X[self.f_idx], self.f_off, self.f_seg) + row[self.tok]
        Tp, Bp = X[1:1 + N], X[1 + N:1 + 2 * N]
        m = np.maximum(Tp, Bp)
        mm = np.where(np.isneginf(m), 0.0, m)
        with np.errstate(divide="ignore"):
            Bn = mm + np.log(np.exp(Tp - mm) + np.exp(Bp - mm)) + row[self.blank]
        Xn = np.empty_like(X)
        Xn[0] = X[0] + row[self.blank]
        Xn[1:1 + N], Xn[1 + N:1 + 2 * N], Xn[-1] = Tn, Bn, -np.inf
        return Xn

    def end(self, X):
        N = self.N
        c = np.concatenate((X[1:1 + N][self.fin], X[1 + N:1 + 2 * N][self.fin]))
        m = c.max()
        if np.isneginf(m):
            raise ValueError("infeasible: no path with a finite score")
        return float(m + np.log(np.exp(c - m).sum()))


def loglik(lp, tokens, preds, finals, blank=0):
    """fp64 log-likelihood only, O(N) memory"""
    lp = np.asarray(lp, np.float64)
    pl = Plan(tokens, preds, finals, blank)
    X = pl.first(lp)
    for t in range(1, lp.shape[0]):
        X = pl.step(X, lp[t])
    return pl.end(X)


def score(lp, tokens, preds, finals, blank=0):
    """-> (loglik, dict of per-node visit, occupancy, mean_frame (-1 where the occupancy is 0), peak_post, peak_frame, second)"""
    lp = np.asarray(lp, np.float64)
    T = lp.shape[0]
    pl = Plan(tokens, preds, finals, blank)
    N = pl.N
    aT = np.empty((T, N))
    X = pl.first(lp)
    aT[0] = X[1:1 + N]
    for t in range(1, T):
        X = pl.step(X, lp[t])
        aT[t] = X[1:1 + N]
    ll = pl.end(X)

    occ, tsum, visit = np.zeros(N), np.zeros(N), np.zeros(N)
    peak, second, pf = np.full(N, -1.0), np.full(N, -1.0), np.zeros(N, np.int64)
    Y = np.full(2 * N + 1, -np.inf)
    for t in range(T - 1, -1, -1):
        e = lp[t, pl.tok]
        if t == T - 1:
            uT = np.where(pl.fin, 0.0, -np.inf)
            uB = uT.copy()
        else:
            uT = _lse_seg(Y[pl.t_idx], pl.t_off, pl.t_seg)
            uB = _lse_seg(Y[pl.b_idx], pl.b_off, pl.b_seg)
        Y[:N], Y[N:2 * N] = uT + e, uB + lp[t, blank]
        g = np.exp(aT[t] + uT - ll)                              # gamma = alpha + beta - lp - loglik, beta - lp = u
        stay = np.exp(aT[t - 1] + Y[:N] - ll) if t > 0 else 0.0
        occ += g
        tsum += g * t
        visit += g - stay
        new = g >= peak                                          # frames descend: >= keeps the first frame of a tie
        second = np.where(new, peak, np.maximum(second, g))
        pf = np.where(new, t, pf)
        peak = np.where(new, g, peak)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(occ > 0, tsum / occ, -1.0)
    return ll, {"visit": visit, "occupancy": occ, "mean_frame": mean, "peak_post": peak, "peak_frame": pf,
                "second": np.maximum(second, 0.0)}


def flat(graphs):
    """[(tokens, preds, finals)] -> (node_tokens, n_nodes, pred_off, preds, is_final) as rvb_ctc_score_graph reads them (each array
    with one spare element, so none is empty)"""
    tok = np.concatenate([np.asarray(g[0], np.int32) for g in graphs] + [np.zeros(1, np.int32)]).astype(np.int32)
    nn = np.array([len(g[0]) for g in graphs], np.int32)
    off = np.concatenate([np.concatenate([[0], np.cumsum([len(p) for p in g[1]])]) for g in graphs]).astype(np.int32)
    prd = np.array([p for g in graphs for ps in g[1] for p in ps] + [0], np.int32)
    fin = np.concatenate([np.asarray(g[2], np.uint8) for g in graphs] + [np.zeros(1, np.uint8)]).astype(np.uint8)
    return tok, nn, off, prd, fin
