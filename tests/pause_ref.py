"""Chunks cut at pauses: a restatement of the definition in include/rvb.h (rvb_pause_chunks), in fp64 and in fp32, the rounding bound
between the two, and the replay check that the GPU tests apply to the kernel's own cuts.

Per recording, over its own n fbank frames f = 0 .. n-1:
  e[f]  = the sum of the 80 log-mel values of frame f
  s[c]  = the sum of e[clamp(c + j, 0, n - 1)] for j = -h .. h-1, for a cut position c in 0 .. n (between frames c-1 and c)
  start_0 = 0; while n - start_k > chunk_size: lo = start_k + chunk_size - search, hi = min(start_k + chunk_size, n - 7),
  start_{k+1} = the LAST c in [lo, hi] with the minimum s; a NaN s is never chosen; all NaN: hi.  The final piece runs to n.

The bound.  The kernel forms e as ONE fp32 sum of 80 terms and s as ONE fp32 sum of 2h values of e, in some order.  A floating-point sum
of m terms in any order has error at most (m - 1) u sum|terms| to first order in u = 2^-24 (Higham, Accuracy and Stability of Numerical
Algorithms, 2nd ed., eq. 4.4).  Level one: |e32[f] - e[f]| <= 79 u sum_bins |x[f]|.  Level two sums the 2h computed e32:
|s32 - sum e32| <= (2h - 1) u sum |e32| <= (2h - 1) u sum_{window} |x| (first order), and sum e32 differs from s by at most the level-one
errors added up, 79 u sum_{window} |x|.  Together
    |s32[c] - s64[c]| <= delta[c] = (79 + 2h - 1) * 2^-24 * sum over the window's 2h * 80 values of |x|
which is about 0.14 at h = 10 for log-mel magnitudes around 15 (98 * 6e-8 * 24 000); speech and a pause differ by thousands.
A kernel that picks c has s32[c] <= s32[m] for every candidate m, so s64[c] <= s64[m] + delta[c] + delta[m]: the replay check."""
import numpy as np

U = 2.0 ** -24


def loudness(feats, dtype=np.float64):
    """e [n] from feats [n, 80]"""
    feats = np.asarray(feats)
    return feats.astype(dtype).sum(axis=1, dtype=dtype) if len(feats) else np.zeros(0, dtype)


def _window_index(n, h):
    """[n + 1, 2h]: the frames clamp(c + j, 0, n - 1), j = -h .. h-1, behind every cut position c = 0 .. n"""
    return np.clip(np.arange(n + 1)[:, None] + np.arange(-h, h)[None, :], 0, n - 1)


def smoothed(e, h):
    """s [n + 1] in e's own dtype"""
    n = len(e)
    with np.errstate(invalid="ignore"):
        return e[_window_index(n, h)].sum(axis=1, dtype=e.dtype)


def delta(feats, h):
    """the bound on |s32 - s64| per cut position, [n + 1] (module docstring)"""
    a = np.abs(np.asarray(feats, np.float64)).sum(axis=1)
    return (79 + 2 * h - 1) * U * a[_window_index(len(a), h)].sum(axis=1)


def check_params(chunk_size, search, h):
    assert 1 <= h <= 64 and chunk_size >= 7 and 7 <= search <= chunk_size - 7, (chunk_size, search, h)


def pick(s, lo, hi):
    """the last position in [lo, hi] with the minimum of s; NaN is never chosen; all NaN: hi"""
    win = s[lo:hi + 1]
    ok = ~np.isnan(win)
    if not ok.any():
        return hi
    m = win[ok].min()
    return lo + int(np.flatnonzero(ok & (win == m))[-1])


def cuts_from_s(s, n, chunk_size, search):
    starts = [0] if n > 0 else []
    while n > 0 and n - starts[-1] > chunk_size:
        lo = starts[-1] + chunk_size - search
        hi = min(starts[-1] + chunk_size, n - 7)
        assert lo <= hi
        starts.append(pick(s, lo, hi))
    return starts


def cuts(feats, chunk_size, search, h, dtype=np.float64):
    """the piece starts of one recording's features [n, 80]; dtype float64 = the definition, float32 = its fp32 restatement"""
    check_params(chunk_size, search, h)
    n = len(feats)
    if n <= chunk_size:
        return [0] if n else []
    return cuts_from_s(smoothed(loudness(feats, dtype), h), n, chunk_size, search)


def lens_of(starts, n):
    return [b - a for a, b in zip(starts, list(starts[1:]) + [n])]


def check_tiling(starts, n, chunk_size):
    """pieces tile [0, n) exactly once and in order; 7 <= lens <= chunk_size except for a recording's only piece"""
    starts = [int(x) for x in starts]
    if n == 0:
        assert starts == []
        return
    assert starts[0] == 0 and all(b > a for a, b in zip(starts, starts[1:])) and starts[-1] < n
    ln = lens_of(starts, n)
    assert sum(ln) == n and max(ln) <= chunk_size
    if len(ln) > 1:
        assert min(ln) >= 7
    else:
        assert n <= chunk_size


def replay_check(feats, starts, chunk_size, search, h):
    """Validity of cuts somebody else made (the kernel's), from their own previous start: every cut lies in [lo, hi] and its fp64 s is
    within delta[c] + delta[m] of the window's fp64 minimum s[m].  Every cut is checked; the first that fails raises."""
    check_params(chunk_size, search, h)
    n = len(feats)
    starts = [int(x) for x in starts]
    check_tiling(starts, n, chunk_size)
    if n <= chunk_size:
        assert starts == ([0] if n else [])
        return
    s = smoothed(loudness(feats, np.float64), h)
    d = delta(feats, h)
    for k in range(1, len(starts)):
        prev, c = starts[k - 1], starts[k]
        assert n - prev > chunk_size, "piece %d: a cut where the rest fits one chunk" % k
        lo, hi = prev + chunk_size - search, min(prev + chunk_size, n - 7)
        assert lo <= c <= hi, "cut %d at %d outside [%d, %d]" % (k, c, lo, hi)
        m = pick(s, lo, hi)
        if np.isnan(s[m]):
            assert c == hi, "cut %d: every candidate is NaN, the cut must be hi" % k
            continue
        assert not np.isnan(s[c]), "cut %d at %d has a NaN s" % (k, c)
        assert s[c] <= s[m] + d[c] + d[m], "cut %d at %d: s %.6f above the minimum %.6f at %d by more than %.3g" % (
            k, c, s[c], s[m], m, d[c] + d[m])
    assert n - starts[-1] <= chunk_size, "the last piece exceeds chunk_size"


FLOOR = np.float32(-15.942385)         # log of the fbank's epsilon: every bin of a frame of digital silence


def burst_audio(seconds=30.0, seed=0):
    """int16 PCM: noise bursts of 0.3 - 0.5 s separated by 0.3 - 0.4 s of zeros"""
    rng = np.random.default_rng(seed)
    out = np.zeros(int(seconds * 16000), np.int16)
    t = int(rng.uniform(0.0, 0.2) * 16000)
    while t < len(out):
        nb = int(rng.uniform(0.3, 0.5) * 16000)
        seg = out[t:t + nb]
        seg[:] = (rng.standard_normal(len(seg)) * 3000.0).astype(np.int16)
        t += nb + int(rng.uniform(0.3, 0.4) * 16000)
    return out
