"""Test-side reference of CTC forced alignment: an independent numpy statement of the recurrence, in fp32, vectorised over the states.

Extended sequence z = [b, y0, b, y1, ..., y(L-1), b], S = 2L + 1 states.  alpha[0][0] = lp[0][z0], alpha[0][1] = lp[0][z1], the rest
-inf.  For t >= 1 the predecessors of s are s, s-1 and, when z[s] is not blank, s >= 2 and z[s] != z[s-2], also s-2;
alpha[t][s] = max(pred) + lp[t][z[s]] in fp32; the back-pointer is the FIRST maximum in the order s, s-1, s-2.  The path ends in the
better of S-1 and S-2 (S-1 on a tie).  Also here: an fp64 path scorer, the fp64 Viterbi optimum, the collapse check and the seeded
input constructions the goldens (tests/golden/force_align.json) and the GPU tests regenerate their inputs from."""
import numpy as np

KINDS = ("random", "quant", "repeat", "neginf", "min_t", "min_t_quant")


def extend(y, blank):
    z = np.full(2 * len(y) + 1, blank, np.int64)
    z[1::2] = y
    return z


def min_frames(y):
    y = np.asarray(y)
    return len(y) + int(np.sum(y[1:] == y[:-1]))


def check_request(T, V, y, blank):
    y = np.asarray(y)
    if y.size == 0:
        raise ValueError("empty transcript")
    if np.any(y < 0) or np.any(y >= V) or np.any(y == blank):
        raise ValueError("token id outside [0, V) or equal to the blank")
    if T < min_frames(y):
        raise ValueError("infeasible: fewer frames than tokens + adjacent repeats")


def force_align(lp, y, blank=0):
    """-> (labels [T], fp32 score).  lp fp32 [T, V]."""
    lp = np.asarray(lp)
    assert lp.dtype == np.float32 and lp.ndim == 2
    T, V = lp.shape
    y = np.asarray(y, np.int64)
    check_request(T, V, y, blank)
    z = extend(y, blank)
    S = len(z)
    skip = np.zeros(S, bool)
    skip[2:] = (z[2:] != blank) & (z[2:] != z[:-2])
    ninf = np.float32(-np.inf)
    alpha = np.full(S, ninf, np.float32)
    alpha[0], alpha[1] = lp[0, z[0]], lp[0, z[1]]
    S4 = (S + 3) // 4
    bp = np.zeros((T, S4), np.uint8)                    # 2 bits per state
    c1, c2, codes = np.empty(S, np.float32), np.empty(S, np.float32), np.zeros(S4 * 4, np.uint8)
    for t in range(1, T):
        c1[0] = ninf; c1[1:] = alpha[:-1]
        c2[:2] = ninf; c2[2:] = alpha[:-2]
        best = alpha.copy()
        m1 = c1 > best
        best[m1] = c1[m1]
        m2 = skip & (c2 > best)
        best[m2] = c2[m2]
        codes[:S] = m1
        codes[:S][m2] = 2
        q = codes.reshape(-1, 4)
        bp[t] = q[:, 0] | (q[:, 1] << 2) | (q[:, 2] << 4) | (q[:, 3] << 6)
        alpha = best + lp[t, z]                          # float32 + float32
        assert alpha.dtype == np.float32
    s = S - 2 if alpha[S - 2] > alpha[S - 1] else S - 1
    score = alpha[s]
    if not score > ninf:
        raise ValueError("infeasible: no path with a finite score")
    states = np.empty(T, np.int64)
    for t in range(T - 1, 0, -1):
        states[t] = s
        s -= (int(bp[t, s >> 2]) >> ((s & 3) * 2)) & 3
    states[0] = s
    return z[states], np.float32(score)


def collapse(labels, blank=0):
    labels = np.asarray(labels)
    keep = np.ones(len(labels), bool)
    keep[1:] = labels[1:] != labels[:-1]
    out = labels[keep]
    return out[out != blank]


def path_score64(lp, labels):
    return float(np.sum(np.asarray(lp, np.float64)[np.arange(len(labels)), np.asarray(labels)]))


def optimum64(lp, y, blank=0):
    """fp64 Viterbi optimum of the same lattice (score only)."""
    lp = np.asarray(lp, np.float64)
    z = extend(np.asarray(y, np.int64), blank)
    S = len(z)
    skip = np.zeros(S, bool)
    skip[2:] = (z[2:] != blank) & (z[2:] != z[:-2])
    alpha = np.full(S, -np.inf)
    alpha[0], alpha[1] = lp[0, z[0]], lp[0, z[1]]
    for t in range(1, lp.shape[0]):
        best = alpha.copy()
        best[1:] = np.maximum(best[1:], alpha[:-1])
        c2 = np.where(skip[2:], alpha[:-2], -np.inf)
        best[2:] = np.maximum(best[2:], c2)
        alpha = best + lp[t, z]
    return float(max(alpha[S - 1], alpha[S - 2]))


def planted_path(rng, y, T, blank):
    """a random valid frame labelling of y over T frames (T >= min_frames(y))"""
    L = len(y)
    dur = np.zeros(2 * L + 1, np.int64)
    dur[1::2] = 1
    for i in range(1, L):
        if y[i] == y[i - 1]:
            dur[2 * i] = 1
    extra = T - int(dur.sum())
    assert extra >= 0
    if extra:
        dur += rng.multinomial(extra, np.full(2 * L + 1, 1.0 / (2 * L + 1)))
    return np.repeat(extend(y, blank), dur)


def make_case(seed, T, V, L, kind, blank=0):
    """-> (lp fp32 [T, V], y int32 [L], T).  Log-softmax of N(0, 1) logits with +4 on a planted valid path (so the optimum stays near a real
    alignment).  kinds: random; quant = log-probs rounded to multiples of 0.25 (sums exact in fp32: ties are plentiful); repeat =
    adjacent tokens repeated with probability 0.4; neginf = a tenth of the off-path entries -inf; min_t / min_t_quant = repeats and
    T exactly the minimum feasible (the T passed in is ignored)."""
    assert kind in KINDS
    rng = np.random.default_rng([seed, KINDS.index(kind)])
    y = rng.integers(1, V, L).astype(np.int32)
    if kind in ("repeat", "min_t", "min_t_quant"):
        for i in range(1, L):
            if rng.random() < 0.4:
                y[i] = y[i - 1]
    if kind in ("min_t", "min_t_quant"):
        T = min_frames(y)
    path = planted_path(rng, y, T, blank)
    logits = rng.standard_normal((T, V)).astype(np.float32)
    logits[np.arange(T), path] += np.float32(4.0)
    m = logits.max(1, keepdims=True)
    lp = (logits - m - np.log(np.exp(logits - m).sum(1, keepdims=True, dtype=np.float32))).astype(np.float32)
    if kind in ("quant", "min_t_quant"):
        lp = (np.round(lp * 4) / 4).astype(np.float32)
    if kind == "neginf":
        hole = rng.random((T, V)) < 0.1
        hole[np.arange(T), path] = False
        lp[hole] = -np.inf
    return np.ascontiguousarray(lp), y, int(T)
