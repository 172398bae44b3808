"""Test-side reference of the WINDOWED full-sum CTC score over a token graph (csrc/ctc_graph_fb_window.hip): an fp64 numpy band
restatement on top of tests/graph_score_ref.py's Plan (the flat candidate lists of the graph), independent of the kernel.

Band semantics (include/rvb.h, rvb_ctc_score_graph_long_*).  lo_of[t] is the window of frame t, never decreasing, lo_of[0] = 0:
  * node j is alive at t iff lo_of[t] <= j < min(lo_of[t] + W, N); B_start is alive iff lo_of[t] == 0;
  * a transition into T_j at t from predecessor p counts iff j is alive at t and p >= lo_of[t] (p = -1: iff lo_of[t] == 0);
  * stay transitions of an alive node always count; a node that was not alive before holds -inf;
  * loglik is the lse over the final nodes alive at the last frame; the posteriors are those of that sum.
Here: before frame t is computed everything below lo_of[t] is SET to -inf in the row of frame t - 1 (the candidates are masked by
lo_of: lo never decreases, so nothing below it is read again), and after it everything that is not alive at t.  The backward sweep
is the mirror image: the successors' row of frame t + 1 holds -inf outside its window, and a node below lo_of[t + 1] gets -inf at
frame t whatever its successors hold.
The policy (tables, next_window) is tests/graph_align_window_ref.py's; `live` restates the set the device reports its best node over."""
import numpy as np

import graph_align_window_ref as GW
import graph_score_ref as R

DEFAULT_W = 4096
MAX_W = 4096


def check_window(window_nodes):
    if window_nodes != 0 and (window_nodes < 256 or window_nodes > MAX_W or window_nodes % 256):
        raise ValueError("window_nodes must be 0 or a multiple of 256 in [256, 4096]")


def effective_window(N, window_nodes):
    return min(window_nodes or DEFAULT_W, GW.pad64(N))


def _mask_below(X, N, lo):
    """row of the frame before: what a window at lo no longer reads"""
    if lo > 0:
        X[0] = -np.inf
        X[1:1 + min(lo, N)] = -np.inf
        X[1 + N:1 + N + min(lo, N)] = -np.inf


def _mask_dead(X, N, lo, W):
    """row of a frame: what is not alive in the window at lo"""
    _mask_below(X, N, lo)
    hi = min(lo + W, N)
    X[1 + hi:1 + N] = -np.inf
    X[1 + N + hi:1 + 2 * N] = -np.inf


class Band:
    """the forward lattice of one graph, advanced frame by frame with the window given for each frame; X is the row of the last frame
    ([B_start, T_0.., B_0.., -inf], fp64)"""

    def __init__(self, lp, pl, W):
        self.lp, self.pl, self.W, self.t, self.lo, self.X = lp, pl, W, 0, 0, None

    def frame(self, lo):
        pl, N, t = self.pl, self.pl.N, self.t
        assert lo >= self.lo and (t > 0 or lo == 0)
        if t == 0:
            X = pl.first(self.lp)
        else:
            X = self.X.copy()
            _mask_below(X, N, lo)
            X = pl.step(X, self.lp[t])
        _mask_dead(X, N, lo, self.W)
        self.X, self.lo, self.t = X, lo, t + 1
        return X


def score(lp, tokens, preds, finals, W, lo_of, blank=0, keep=False, rows_at=()):
    """-> (loglik, dict of per-node visit, occupancy, mean_frame (-1 where the occupancy is 0), peak_post, peak_frame, second); with
    keep also "alpha" ([T, N]: the rows of T_j) and "post_sum" ([T]: the posteriors of a frame summed over ALL its states); "rows": the
    whole alpha row of each frame of rows_at.  ValueError when no path inside the windows has a finite score."""
    lp = np.asarray(lp, np.float64)
    lo_of = np.asarray(lo_of, np.int64)
    T = lp.shape[0]
    pl = R.Plan(tokens, preds, finals, blank)
    N = pl.N
    assert lo_of[0] == 0 and np.all(np.diff(lo_of) >= 0)
    band = Band(lp, pl, W)
    aT, aB, a0 = np.empty((T, N)), (np.empty((T, N)) if keep else None), np.empty(T)
    rows = {}
    for t in range(T):
        X = band.frame(int(lo_of[t]))
        aT[t], a0[t] = X[1:1 + N], X[0]
        if keep:
            aB[t] = X[1 + N:1 + 2 * N]
        if t in rows_at:
            rows[t] = X.copy()
    ll = pl.end(band.X)

    occ, tsum, visit = np.zeros(N), np.zeros(N), np.zeros(N)
    peak, second, pf = np.full(N, -1.0), np.full(N, -1.0), np.zeros(N, np.int64)
    post_sum = np.zeros(T)
    nodes = np.arange(N)
    Y = np.full(2 * N + 1, -np.inf)
    ystart = -np.inf                                             # beta of B_start
    for t in range(T - 1, -1, -1):
        lo = int(lo_of[t])
        alive = (nodes >= lo) & (nodes < lo + W)
        e = lp[t, pl.tok]
        if t == T - 1:
            uT = np.where(pl.fin & alive, 0.0, -np.inf)
            uB = uT.copy()
            ustart = -np.inf
        else:
            lon = int(lo_of[t + 1])
            uT = R._lse_seg(Y[pl.t_idx], pl.t_off, pl.t_seg)
            uB = R._lse_seg(Y[pl.b_idx], pl.b_off, pl.b_seg)
            cut = ~alive | (nodes < lon)                         # not alive here, or below the window of the frame after
            uT[cut] = -np.inf
            uB[cut] = -np.inf
            if lon == 0:
                c = np.concatenate(([ystart], Y[:N][pl.from_start]))
                m = c.max()
                ustart = m + np.log(np.exp(c - m).sum()) if m > -np.inf else -np.inf
            else:
                ustart = -np.inf
        Y[:N], Y[N:2 * N] = uT + e, uB + lp[t, blank]
        ystart = ustart + lp[t, blank] if lo == 0 else -np.inf
        g = np.exp(aT[t] + uT - ll)                              # gamma = alpha + beta - lp - loglik, beta - lp = u
        stay = np.exp(aT[t - 1] + Y[:N] - ll) if t > 0 else 0.0
        if keep:
            post_sum[t] = g.sum() + np.exp(aB[t] + uB - ll).sum() + np.exp(a0[t] + ustart - ll)
        occ += g
        tsum += g * t
        visit += g - stay
        new = g >= peak                                          # frames descend: >= keeps the first frame of a tie
        second = np.where(new, peak, np.maximum(second, g))
        pf = np.where(new, t, pf)
        peak = np.where(new, g, peak)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(occ > 0, tsum / occ, -1.0)
    out = {"visit": visit, "occupancy": occ, "mean_frame": mean, "peak_post": peak, "peak_frame": pf, "second": np.maximum(second, 0.0)}
    if keep:
        out["alpha"], out["post_sum"] = aT, post_sum
    out["rows"] = rows
    return ll, out


def drive(lp, tokens, preds, finals, window_nodes=0, slab_rows=1 << 30, blank=0):
    """the driver on the restatement's own rows: slabs of slab_rows frames, each cut into launches by the policy, which is fed the node
    of the first maximum of the launch's last row over the live states -> (lo_of [T], best per launch)"""
    check_window(window_nodes)
    lp = np.asarray(lp, np.float64)
    N, T = len(tokens), len(lp)
    W = effective_window(N, window_nodes)
    tab = GW.tables(tokens, preds, finals)
    rem = frames_to_end(tokens, preds, finals)
    band = Band(lp, R.Plan(tokens, preds, finals, blank), W)
    lo_of, best = np.zeros(T, np.int32), []
    lo, b = 0, -1
    for s0 in range(0, T, slab_rows):
        s1 = min(T, s0 + slab_rows)
        f0 = s0
        while f0 < s1:
            lo, f1 = GW.next_window(tab, N, T, W, f0, s1, lo, b)
            assert f0 < f1 <= s1
            for t in range(f0, f1):
                band.frame(lo)
            lo_of[f0:f1] = lo
            vals, node = live_row(band.X, rem, N, W, lo, T - f1)
            b = int(node[int(np.argmax(vals))]) if len(vals) and vals.max() > -np.inf else -1
            best.append(b)
            f0 = f1
    return lo_of, best


def frames_to_end(tokens, preds, finals):
    """-> (remT [N], remB [N], rem_start): the fewest frames from T_j, from B_j, from B_start to a final end (FAR: never)"""
    N = len(tokens)
    remT, remB = np.full(N, GW.FAR, np.int64), np.full(N, GW.FAR, np.int64)
    rem_start = GW.FAR
    for j in range(N - 1, -1, -1):
        if finals[j]:
            remT[j] = remB[j] = 0
        if remT[j] >= GW.FAR:
            continue
        for p in preds[j]:
            if p < 0:
                rem_start = min(rem_start, remT[j] + 1)
            else:
                remT[p] = min(remT[p], remT[j] + (1 if tokens[p] != tokens[j] else 2))
                remB[p] = min(remB[p], remT[j] + 1)
    return remT, remB, rem_start


def live_row(row, rem, N, W, lo, left):
    """the states of a band row the normaliser (and the reported best node) run over, in the order B_start, T_lo, B_lo, T_lo+1, ...
    -> (values, node of each); a state counts while its frames to the end are within the `left` frames left"""
    remT, remB, rem_start = rem
    hi = min(lo + W, N)
    vals, node = [], []
    if lo == 0 and rem_start <= left:
        vals.append(row[0]); node.append(0)
    for j in range(lo, hi):
        if remT[j] <= left:
            vals.append(row[1 + j]); node.append(j)
        if remB[j] <= left:
            vals.append(row[1 + N + j]); node.append(j)
    return np.array(vals), np.array(node, np.int64)


def replay_policy(tokens, preds, finals, T, W, slab_rows, best):
    """the launches the policy cuts when it is fed the best nodes `best` (one per launch, as the device reported them)
    -> (lo_of [T], [(f0, f1, lo)] per launch)"""
    N = len(tokens)
    tab = GW.tables(tokens, preds, finals)
    lo_of = np.zeros(T, np.int32)
    lo, b, k, cuts = 0, -1, 0, []
    for s0 in range(0, T, slab_rows):
        s1 = min(T, s0 + slab_rows)
        f0 = s0
        while f0 < s1:
            lo, f1 = GW.next_window(tab, N, T, W, f0, s1, lo, b)
            assert f0 < f1 <= s1
            lo_of[f0:f1] = lo
            cuts.append((f0, f1, lo))
            b = int(best[k]) if k < len(best) else -1
            k += 1
            f0 = f1
    return lo_of, cuts


def brute_force(lp, tokens, preds, finals, W, lo_of, blank=0):
    """every state path made of counted transitions, enumerated -> (loglik, visit [N]).  For graphs and lattices of a few states."""
    lp = np.asarray(lp, np.float64)
    T, N = lp.shape[0], len(tokens)
    START = -1

    def alive(t, j):
        return lo_of[t] <= j < min(lo_of[t] + W, N)

    total = 0.0
    through = np.zeros(N)

    def walk(t, state, logp, seen):
        nonlocal total
        kind, j = state
        if t == T - 1:
            if kind != "S" and finals[j]:
                p = np.exp(logp)
                total += p
                for n in seen:
                    through[n] += p
            return
        lo = lo_of[t + 1]
        nxt = []
        if kind == "S":
            if lo == 0:
                nxt.append((("S", START), blank))
                nxt += [(("T", k), tokens[k]) for k in range(N) if -1 in preds[k] and alive(t + 1, k)]
        else:
            if alive(t + 1, j) and j >= lo:
                if kind == "T":
                    nxt.append((("T", j), tokens[j]))
                nxt.append((("B", j), blank))
                for k in range(j + 1, N):
                    if j in preds[k] and alive(t + 1, k) and (kind == "B" or tokens[k] != tokens[j]):
                        nxt.append((("T", k), tokens[k]))
        for st, col in nxt:
            walk(t + 1, st, logp + lp[t + 1, col], seen | {st[1]} if st[0] == "T" else seen)

    walk(0, ("S", START), lp[0, blank], frozenset())
    for k in range(N):
        if -1 in preds[k] and alive(0, k):
            walk(0, ("T", k), lp[0, tokens[k]], frozenset({k}))
    if total <= 0:
        raise ValueError("infeasible")
    return float(np.log(total)), through / total


# ------------------------------------------------------------------------------------------------ the cases the tests share
MOVING = [("npt1", 256, 112, 21), ("npt2", 2048, 575, 22), ("npt4", 4096, 1100, 23)]   # (tag, W, L, seed): groups graphs of 4 L nodes
MOVING_SLAB = 500
V_MOVING = 12


def moving_case(L, seed):
    """graph_align_window_ref.peaked_case("groups") over T = 1.25 L frames, a little above the shortest reading (L frames): a window
    smaller than the graph has to move -> (lp, (tokens, preds, finals))"""
    lp, tokens, preds, finals, _ = GW.peaked_case("groups", seed, L, V_MOVING, T=int(1.25 * L))
    return lp, (tokens, preds, finals)


def peaky_case():
    """the first moving case with its logits scaled by 6 (the log-probs times 6, normalised again in fp32)"""
    lp, graph = moving_case(112, 31)
    x = lp.astype(np.float32) * np.float32(6.0)
    m = x.max(1, keepdims=True)
    lp6 = (x - m - np.log(np.exp(x - m).sum(1, keepdims=True, dtype=np.float32))).astype(np.float32)
    return np.ascontiguousarray(lp6), graph
