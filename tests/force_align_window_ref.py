"""Test-side reference of the WINDOWED CTC Viterbi (csrc/ctc_viterbi_window.hip): a numpy restatement, independent of the kernel.

The recurrence is tests/force_align_ref.py's: fp32 adds, predecessors in the order s, s-1, s-2, the first maximum wins, the path ends
in the better of S-1 and S-2 (S-1 on a tie).  What is added:
  * only the window [lo, lo + W) of the S states is alive at a frame: a predecessor below lo is -inf, nothing above lo + W - 1 is written;
  * the frames arrive in slabs of `slab_rows`, each slab is cut into launches of W / 4 - 16 frames (segments()), and lo changes only between
    launches: next_lo() below, fed with the FIRST maximum (lowest state on a tie) of the window after the launch before, -1 if all -inf;
  * W = min(requested or 32768, S rounded up to 32);
  * the back-trace reports the path's smallest distance to a window edge, min(st - lo[t], lo[t] + W - 1 - st) over the frames, where
    the lower edge counts only if lo[t] != 0 and the upper only if lo[t] + W < S_pad (else it is the lattice's own edge); W if no
    frame counts.
A wildcard (id -2, only with w given) emits w[t] + bias (one fp32 add) and is a label of its own: two adjacent ones allow no skip."""
import numpy as np

import force_align_ref as R

WILDCARD = -2
DEFAULT_W = 32768


def pad32(n):
    return (n + 31) // 32 * 32


def round_down32(v):
    return v // 32 * 32                       # Python floors: also right below zero


def next_lo(S, T, W, f0, f1, lo_prev, best_prev):
    """The window policy, four steps in this order, then never back."""
    S_pad = pad32(S)
    if f0 <= 0:
        return 0
    lo = round_down32(best_prev - W // 2) if best_prev >= 0 else lo_prev     # 1. centre on the best state
    lo = max(lo, lo_prev)                                                    # 2. never below lo_prev
    lo = min(lo, round_down32(2 * f0 + 1))                                   # 3. not above the highest state frame f0 can reach ...
    lo = min(lo, S_pad - W)                                                  #    ... nor past the end of the lattice
    need = S - 2 - 2 * (T - f1)                                              # 4. the end stays reachable from the window at f1 - 1
    if lo + W - 1 < need:
        lo = pad32(need - W + 1)
    return max(lo, lo_prev)


def segments(T, W, slab_rows):
    """the launches: every slab's frames in pieces of W / 4 - 16 frames (2 states a frame: W / 2 - 32, the room that rounding lo down
    to a multiple of 32 leaves above a best state at the centre); a window below 160 states never moves and is cut at W / 4"""
    seg = W // 4 - 16 if W // 4 > 32 else max(W // 4, 1)
    out = []
    for s0 in range(0, T, slab_rows):
        s1 = min(T, s0 + slab_rows)
        for g0 in range(s0, s1, seg):
            out.append((g0, min(g0 + seg, s1)))
    return out


def effective_window(L, window_states):
    return min(window_states or DEFAULT_W, pad32(2 * L + 1))


def check_window(window_states):
    if window_states != 0 and (window_states < 256 or window_states > 32768 or window_states % 256):
        raise ValueError("window_states must be 0 or a multiple of 256 in [256, 32768]")


def force_align_window(lp, y, window_states=0, slab_rows=8192, blank=0, w=None, bias=0.0):
    """-> (labels [T], fp32 score, lo [T] int32, min_margin).  lp fp32 [T, V]; y may hold WILDCARD when w (fp32 [T]) is given.
    Raises ValueError("infeasible ...") when no path inside the windows has a finite score."""
    lp = np.asarray(lp)
    assert lp.dtype == np.float32 and lp.ndim == 2
    T, V = lp.shape
    y = np.asarray(y, np.int64)
    check_window(window_states)
    wild_tok = (y == WILDCARD) if w is not None else np.zeros(len(y), bool)
    R.check_request(T, V, np.where(wild_tok, 1 if blank != 1 else 2, y), blank)       # a wildcard is no vocabulary id: checked as one
    if T < R.min_frames(y):
        raise ValueError("infeasible: fewer frames than tokens + adjacent repeats")
    L = len(y)
    S, S_pad = 2 * L + 1, pad32(2 * L + 1)
    W = effective_window(L, window_states)
    z = np.full(S_pad, blank, np.int64)                       # the label of every state; past S - 1: blank, never alive
    z[1:S:2] = y
    skip = np.zeros(S_pad, bool)
    skip[2:S] = (z[2:S] != blank) & (z[2:S] != z[:S - 2])
    wild = np.zeros(S_pad, bool)
    wild[1:S:2] = wild_tok
    col = np.where(wild, blank, z)
    ninf = np.float32(-np.inf)
    ew = None if w is None else (np.asarray(w, np.float32) + np.float32(bias)).astype(np.float32)

    def emit(t, a, b):
        e = lp[t, col[a:b]]
        if ew is not None:
            e = np.where(wild[a:b], ew[t], e)
        return e.astype(np.float32)

    alpha = np.full(S_pad, ninf, np.float32)
    bp = np.zeros((T, W // 4), np.uint8)                       # 2 bits per cell, window-relative
    lo_of = np.zeros(T, np.int32)
    alpha[0:2] = emit(0, 0, 2)
    lo, best = 0, -1
    c1, c2, bestv = (np.empty(W, np.float32) for _ in range(3))
    m1, m2, codes = np.empty(W, bool), np.empty(W, bool), np.zeros(W, np.uint8)
    for f0, f1 in segments(T, W, slab_rows):
        lo = next_lo(S, T, W, f0, f1, lo, best)
        assert lo % 32 == 0 and 0 <= lo <= S_pad - W
        hi = lo + W
        live = min(hi, S) - lo                                # states of the window that exist
        nsk = ~skip[lo:hi]
        a = alpha[lo:hi]                                      # a view: the window's states of the whole lattice
        for t in range(max(f0, 1), f1):
            # the first maximum in the order s, s-1, s-2: a later candidate wins only if it is strictly greater, and then max() is it
            c1[0] = ninf; c1[1:] = a[:-1]                     # below the window: -inf
            c2[:2] = ninf; c2[2:] = a[:-2]
            c2[nsk] = ninf
            np.greater(c1, a, out=m1)
            np.maximum(a, c1, out=bestv)
            np.greater(c2, bestv, out=m2)
            np.maximum(bestv, c2, out=bestv)
            np.copyto(codes, m1, casting="unsafe")
            codes[m2] = 2
            q = codes.reshape(-1, 4)
            bp[t] = q[:, 0] | (q[:, 1] << 2) | (q[:, 2] << 4) | (q[:, 3] << 6)
            new = bestv + emit(t, lo, hi)
            assert new.dtype == np.float32
            new[live:] = ninf
            a[:] = new
            lo_of[t] = lo
        win = alpha[lo:lo + live]
        k = int(np.argmax(win)) if live > 0 else 0            # the first maximum
        best = lo + k if live > 0 and win[k] > ninf else -1
    s = S - 2 if alpha[S - 2] > alpha[S - 1] else S - 1
    score = alpha[s]
    if not score > ninf:
        raise ValueError("infeasible: no path inside the window with a finite score")
    states = np.empty(T, np.int64)
    margin = W
    for t in range(T - 1, -1, -1):
        states[t] = s
        idx = s - int(lo_of[t])
        assert 0 <= idx < W
        if lo_of[t] != 0:
            margin = min(margin, idx)
        if lo_of[t] + W < S_pad:
            margin = min(margin, W - 1 - idx)
        if t:
            s -= (int(bp[t, idx >> 2]) >> ((idx & 3) * 2)) & 3
    zl = np.where(wild, WILDCARD, z)
    return zl[states], np.float32(score), lo_of, int(margin)


DECOY_W = 256


def decoy_case(seed, T=700, V=12, L=300, early=128, slow=20, blank=0, boost=4.0):
    """A lattice whose early frames fit a LATER part of the transcript as well as the part that was spoken.  The true path is planted
    over all T frames with +4, as in make_case, and spends the first `early` frames on its first `slow` tokens.  On top, frame t of the
    first `early` frames gets +boost on token t: a second labelling that walks the transcript at a token per frame (no adjacent
    repeats, so every step is a legal skip) and after `early` frames (launches of 48, with lo = 0 until then) stands at state 2 early - 1, far
    more than DECOY_W / 2 states above the true path.  Where the runaway is the better PARTIAL path at that frame (a matter of the
    noise: the seeds are searched), the policy centres the window on it and drops the true path; the exact Viterbi keeps the true
    path, because the runaway then has to wait, on labels the frames do not carry, until the speech catches up.  -> (lp, y)"""
    rng = np.random.default_rng([seed, 4242])
    y = rng.integers(1, V, L).astype(np.int32)
    for i in range(1, L):
        while y[i] == y[i - 1]:
            y[i] = rng.integers(1, V)
    head = R.planted_path(rng, y[:slow], early, blank)
    tail = R.planted_path(rng, y[slow:], T - early, blank)
    path = np.concatenate([head, tail])
    assert R.collapse(path, blank).tolist() == y.tolist()
    logits = rng.standard_normal((T, V)).astype(np.float32)
    logits[np.arange(T), path] += np.float32(4.0)
    fast = y[:early]                                           # one token per frame: states 1, 3, 5, ...
    logits[np.arange(early), fast] += np.float32(boost)
    m = logits.max(1, keepdims=True)
    lp = (logits - m - np.log(np.exp(logits - m).sum(1, keepdims=True, dtype=np.float32))).astype(np.float32)
    return np.ascontiguousarray(lp), y
