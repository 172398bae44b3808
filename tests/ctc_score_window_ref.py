"""Test-side reference of the WINDOWED full-sum CTC score (csrc/ctc_fb_window.hip): an fp64 numpy band forward-backward, independent
of the kernel.  The recursions are tests/ctc_score_ref.py's; what is added is the band.

Band semantics.  lo_of[t] is the window of the launch that computes frame t (non-decreasing, a multiple of 32), W its width.
  * cell (t, s) is alive iff lo_of[t] <= s < min(lo_of[t] + W, S);
  * a transition (t-1, s') -> (t, s) counts iff both cells are alive and s' >= lo_of[t];
  * the full sum runs over the paths made of counted transitions.
So alpha[t] reads no predecessor below lo_of[t], and beta[t][s] is -inf for s < lo_of[t + 1] (no counted transition leaves the
cell).  gamma = alpha + beta - lp - loglik; over the alive states of a frame exp(gamma) sums to 1."""
import numpy as np

import ctc_score_ref as R
import force_align_ref as A
from ctc_score_ref import make_lattice                     # noqa: F401  (the inputs of the tests)
from force_align_window_ref import effective_window, next_lo, pad32, segments


def lo_per_frame(T, W, slab_rows, los):
    """the launches' windows (one per segment of segments()) -> lo_of [T]"""
    segs = segments(T, W, slab_rows)
    assert len(segs) == len(los)
    lo_of = np.zeros(T, np.int64)
    for (f0, f1), lo in zip(segs, los):
        lo_of[f0:f1] = lo
    return lo_of


def check_band(lo_of, S, W):
    lo_of = np.asarray(lo_of, np.int64)
    assert lo_of[0] == 0 and (np.diff(lo_of) >= 0).all() and (lo_of % 32 == 0).all() and lo_of.max() <= pad32(S) - W


def band_alpha_beta(lp, y, lo_of, W, blank=0):
    """-> (alpha [T, S], beta [T, S], loglik), fp64; -inf in every dead cell"""
    lp = np.asarray(lp, np.float64)
    T, V = lp.shape
    y = np.asarray(y, np.int64)
    A.check_request(T, V, y, blank)
    z = A.extend(y, blank)
    S = len(z)
    check_band(lo_of, S, W)
    skip = R._skip(z, blank)
    up2 = np.concatenate((skip[2:], np.zeros(2, bool)))
    ninf = -np.inf
    alpha = np.full((T, S), ninf)
    alpha[0, 0], alpha[0, 1] = lp[0, z[0]], lp[0, z[1]]
    P = np.full(S + 2, ninf)
    for t in range(1, T):
        lo = int(lo_of[t])
        hi = min(lo + W, S)
        P[2:] = alpha[t - 1]                               # P[s + 2] = alpha[t - 1][s]; dead cells hold -inf
        x0 = P[lo + 2:hi + 2]
        x1 = P[lo + 1:hi + 1].copy()
        x2 = np.where(skip[lo:hi], P[lo:hi], ninf)
        x1[:1] = ninf                                      # s' = lo - 1 lies below the window of frame t
        x2[:2] = ninf                                      # s' = lo - 2, lo - 1
        alpha[t, lo:hi] = R._lse(x0, x1, x2) + lp[t, z[lo:hi]]
    ll = float(R._lse(alpha[-1, S - 1], alpha[-1, S - 2]))
    beta = np.full((T, S), ninf)
    lo = int(lo_of[T - 1])
    for s in (S - 1, S - 2):
        if lo <= s < lo + W:
            beta[T - 1, s] = lp[T - 1, z[s]]
    N = np.full(S + 2, ninf)
    for t in range(T - 2, -1, -1):
        lo = int(lo_of[t])
        hi = min(lo + W, S)
        N[:S] = beta[t + 1]
        row = R._lse(N[lo:hi], N[lo + 1:hi + 1], np.where(up2[lo:hi], N[lo + 2:hi + 2], ninf)) + lp[t, z[lo:hi]]
        row[:max(0, int(lo_of[t + 1]) - lo)] = ninf        # the cut at a move: nothing leaves a state below the next window
        beta[t, lo:hi] = row
    return alpha, beta, ll


def band_gamma(lp, y, lo_of, W, blank=0, keep_alpha_at=()):
    """-> (gamma [T, S] fp64 log-posteriors, loglik, {t: alpha[t] copy for t in keep_alpha_at})"""
    lp64 = np.asarray(lp, np.float64)
    z = A.extend(np.asarray(y, np.int64), blank)
    alpha, beta, ll = band_alpha_beta(lp64, y, lo_of, W, blank)
    kept = {int(t): alpha[int(t)].copy() for t in keep_alpha_at}
    g = alpha
    g += beta
    del beta
    e = lp64[:, z]
    with np.errstate(invalid="ignore"):
        g -= np.where(np.isneginf(e), 0.0, e)
        g -= ll
    g[np.isnan(g)] = -np.inf
    return g, ll, kept


def score(lp, y, lo_of, W, blank=0, keep_alpha_at=()):
    """-> (loglik, per-token dict as ctc_score_ref.score returns it, kept alpha rows)"""
    g, ll, kept = band_gamma(lp, y, lo_of, W, blank, keep_alpha_at)
    return ll, R.reduce_tokens(g), kept


def live_from(S, T, t):
    """the lowest state of frame t that can still reach the end"""
    return max(0, S - 2 * (T - t))


def path_states(labels, blank=0):
    """the state of every frame of a valid frame labelling (planted_path)"""
    st = np.zeros(len(labels), np.int64)
    s = 0 if labels[0] == blank else 1
    st[0] = s
    for t in range(1, len(labels)):
        if labels[t] != labels[t - 1]:
            s += 1 if (labels[t] == blank or labels[t - 1] == blank) else 2
        st[t] = s
    return st


def planted_lattice(seed, T, V, L, through=None, blank=0, boost=4.0):
    """Seeded (lp fp32 [T, V], y int32 [L], states [T]): the log-softmax of N(0, 1) logits with +boost on a planted path (force_align_ref's
    planted_path).  through = (frame, state): the path sits at that ODD state at that frame (its token ends its run there)."""
    rng = np.random.default_rng([seed, T, V, L, 77])
    y = rng.integers(1, V, L).astype(np.int32)
    for i in range(1, L):
        while y[i] == y[i - 1]:
            y[i] = rng.integers(1, V)
    if through is None:
        path = A.planted_path(rng, y, T, blank)
    else:
        g, s = through
        assert s % 2 == 1
        k = (s + 1) // 2                                   # tokens y[:k] over the frames [0, g]
        head = A.planted_path(rng, y[:k], g + 1, blank)
        n = len(head)
        while head[n - 1] == blank:                        # the trailing blanks go to the last token's run
            n -= 1
        head[n:] = y[k - 1]
        tail = A.planted_path(rng, y[k:], T - g - 1, blank)
        path = np.concatenate([head, tail])
    assert A.collapse(path, blank).tolist() == y.tolist()
    logits = rng.standard_normal((T, V)).astype(np.float32)
    logits[np.arange(T), path] += np.float32(boost)
    m = logits.max(1, keepdims=True)
    lp = (logits - m - np.log(np.exp(logits - m).sum(1, keepdims=True, dtype=np.float32))).astype(np.float32)
    st = path_states(path, blank)
    if through is not None:
        assert st[through[0]] == through[1]
    return np.ascontiguousarray(lp), y, st


def centred_schedule(T, W, S, slab_rows, states, floor_from=None):
    """a window per launch that follows a known path: centred on the path's state at the launch's first frame, never back, inside
    the lattice.  floor_from = (launch index, lo): from that launch on the window is at least lo (a forced jump)."""
    los, lo = [], 0
    for i, (f0, f1) in enumerate(segments(T, W, slab_rows)):
        want = 0 if f0 == 0 else (int(states[f0]) - W // 2) // 32 * 32
        if floor_from is not None and i >= floor_from[0]:
            want = max(want, floor_from[1])
        lo = min(max(lo, want, 0), pad32(S) - W)
        los.append(lo)
    return los


def policy_schedule(lp, y, W, slab_rows, blank=0):
    """the windows the policy (next_lo) picks when it is fed with this reference's own best state: the first maximum of alpha over
    the window states that can still reach the end, after each launch -> (los per launch, best per launch)"""
    lp = np.asarray(lp, np.float64)
    T = lp.shape[0]
    z = A.extend(np.asarray(y, np.int64), blank)
    S = len(z)
    skip = R._skip(z, blank)
    ninf = -np.inf
    a = np.full(S, ninf)
    a[0], a[1] = lp[0, z[0]], lp[0, z[1]]
    P = np.full(S + 2, ninf)
    los, bests, lo, best = [], [], 0, -1
    for f0, f1 in segments(T, W, slab_rows):
        lo = next_lo(S, T, W, f0, f1, lo, best)
        hi = min(lo + W, S)
        for t in range(max(f0, 1), f1):
            P[2:] = a
            x1 = P[lo + 1:hi + 1].copy()
            x2 = np.where(skip[lo:hi], P[lo:hi], ninf)
            x1[:1] = ninf
            x2[:2] = ninf
            row = R._lse(P[lo + 2:hi + 2], x1, x2) + lp[t, z[lo:hi]]
            a[:] = ninf
            a[lo:hi] = row
        b0 = max(lo, live_from(S, T, f1 - 1))
        best = -1
        if b0 < hi and a[b0:hi].max() > ninf:
            best = b0 + int(np.argmax(a[b0:hi]))
        los.append(lo)
        bests.append(best)
    return los, bests


# ---- the inputs of tests/test_ctc_score_window_gpu.py that are compared with this reference under the 2 % cap on skipped peak frames
V = 32
CUT_G0, CUT_LO = 336, 288                                  # the forced jump: launch 7 of 48 frames each, to state 32 * 9


def moving_case(L, T):
    return make_lattice(700 + L, T, V, L)


def cut_case():
    """-> (lp, y, unforced schedule, forced schedule): the planted path sits at state CUT_LO - 1 at frame CUT_G0 - 1"""
    L, T, W = 300, 700, 256
    lp, y, st = planted_lattice(900, T, V, L, through=(CUT_G0 - 1, CUT_LO - 1), boost=2.5)   # +4 saturates: too many tied peak frames
    S = 2 * L + 1
    free = centred_schedule(T, W, S, T, st)
    forced = centred_schedule(T, W, S, T, st, floor_from=(CUT_G0 // 48, CUT_LO))
    return lp, y, free, forced


MOVING = [(300, 700, 256, (700, 100, 47)), (2300, 2500, 4352, (2500,)), (8400, 8600, 16640, (8600,))]
