"""Reference of the CTC phrase search (rvb_ctc_find, csrc/ctc_find.hip): the recurrence written cell by cell in fp32 numpy, the
suppression rule, and an exhaustive enumeration of every path that the recurrence is validated against.  No code is shared with
the product.

A phrase y[0..L-1] is the lattice z = [y0, b, y1, b, ..., y(L-1)] (S = 2L - 1 states, no leading or trailing blank).
d[t][s] = lp[t][z[s]] - w[t] with w[t] the row maximum;  h[t][0] = max(h[t-1][0], 0) + d[t][0];
h[t][s] = max(h[t-1][s], h[t-1][s-1] (, h[t-1][s-2] if z[s] is a token, s >= 2, z[s] != z[s-2])) + d[t][s];
the first maximum in the order stay, one below (state 0: the fresh start), two below; every state carries the start frame of its
chosen path; frame t is an arrival if state S - 1 was not entered by "stay"."""
import itertools

import numpy as np

F = np.float32
NEG = F(-np.inf)


def lattice(y, blank):
    z = []
    for k, tok in enumerate(y):
        if k:
            z.append(blank)
        z.append(int(tok))
    return z


def candidates(lp, w, y, blank, threshold):
    """-> (list of (end, start, fp32 score) in frame order: every arrival with score >= threshold)"""
    lp = np.asarray(lp, F)
    T = lp.shape[0]
    z = lattice(y, blank)
    S = len(z)
    h = [NEG] * S
    st = [0] * S
    out = []
    thr = F(threshold)
    for t in range(T):
        nh, ns = [NEG] * S, [0] * S
        for s in range(S):
            d = F(lp[t, z[s]]) - F(w[t])
            best, start, code = h[s], st[s], 0
            if s == 0:
                c1, s1 = F(0.0), t
            else:
                c1, s1 = h[s - 1], st[s - 1]
            if c1 > best:
                best, start, code = c1, s1, 1
            if s >= 2 and s % 2 == 0 and z[s] != z[s - 2] and h[s - 2] > best:
                best, start, code = h[s - 2], st[s - 2], 2
            nh[s] = F(best + d)
            ns[s] = start
            if s == S - 1 and code != 0 and nh[s] >= thr:
                out.append((t, start, nh[s]))
        h, st = nh, ns
    return out


def suppress(cands, max_hits):
    """cands: (end, start, score) -> the hits (start, end, score) in order of end"""
    order = sorted(cands, key=lambda c: (-float(c[2]), c[0], c[1]))
    kept = []
    for end, start, score in order:
        if len(kept) >= max_hits:
            break
        if all(end < s or e < start for e, s, _ in kept):
            kept.append((end, start, score))
    return [(s, e, v) for e, s, v in sorted(kept, key=lambda c: c[0])]


def find(lp, w, y, blank, threshold, max_candidates, max_hits):
    """what the device pipeline returns for one pair: (count, kept raw candidates, hits)"""
    c = candidates(lp, w, y, blank, threshold)
    kept = c[:max_candidates]
    return len(c), kept, suppress(kept, max_hits)


# ---------------------------------------------------------------------------------------------------------- brute force
def _paths_into(z, t, s):
    """every path that is in state s at frame t, as the list of (frame, state) from its first frame on; states only move up by 0, 1
    or (where the lattice allows) 2, and a path begins in state 0"""
    def skip_ok(k):
        return k >= 2 and k % 2 == 0 and z[k] != z[k - 2]

    def rec(t, s):
        # codes backwards: 0 stay, 1 from one below / fresh start, 2 from two below
        if s == 0:
            yield [(t, 0)], (1,)                                # a fresh start at t
        if t == 0:
            return
        for tail, codes in rec(t - 1, s):
            yield tail + [(t, s)], (0,) + codes
        if s >= 1:
            for tail, codes in rec(t - 1, s - 1):
                yield tail + [(t, s)], (1,) + codes
        if skip_ok(s):
            for tail, codes in rec(t - 1, s - 2):
                yield tail + [(t, s)], (2,) + codes
    return rec(t, s)


def brute_force(lp, w, y, blank, stats=None):
    """Exhaustive: per frame t the best score of any path in state S - 1 at t, the path the tie order picks among the best (the
    smallest code sequence read backwards from t), and from it the arrival set.  Sums are fp64 over inputs on a grid where they are
    exact.  -> list of (end, start, score) for the arrivals; stats["ties"] counts the frames whose best score several paths reach"""
    lp = np.asarray(lp, np.float64)
    z = lattice(y, blank)
    S = len(z)
    out = []
    for t in range(lp.shape[0]):
        best, scores = None, []
        for path, codes in _paths_into(z, t, S - 1):
            score = sum(lp[f, z[s]] - float(w[f]) for f, s in path)
            scores.append(score)
            key = (-score, codes)
            if best is None or key < best[0]:
                best = (key, path, codes, score)
        if best is None:
            continue
        if stats is not None and scores.count(best[3]) > 1:
            stats["ties"] = stats.get("ties", 0) + 1
        _, path, codes, score = best
        if codes[0] != 0:
            out.append((t, path[0][0], score))
    return out


def all_phrases(V, blank, max_len):
    toks = [v for v in range(V) if v != blank]
    for L in range(1, max_len + 1):
        yield from itertools.product(toks, repeat=L)
