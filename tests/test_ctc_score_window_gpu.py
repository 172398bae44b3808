"""The windowed CTC forward-backward kernels (csrc/ctc_fb_window.hip) through the lab hook rvb_test_ctc_score_window: bit for bit
against rvb_test_ctc_score where the window never moves, and against the fp64 band reference (tests/ctc_score_window_ref.py) on the
windows the device itself chose (or was forced to) where it does.

Bounds.  loglik: |got - ref| <= 1e-5 * T, the condition derived in tests/test_ctc_score_gpu.py.  Posteriors, occupancies and mean
frames are measured against the band reference; the asserted tolerances are 4 x the largest error recorded on the MI355X over the
cases of this file (docs/tuning-log.md), capped by the conditions of test_ctc_score_gpu.py (1e-3 absolute for peak_post, 1e-3
relative for occupancy, mean_frame relative to max(mean_frame, 1)).  peak_frame must equal the reference's wherever its two
largest posteriors of the token differ by more than the posterior tolerance; at most 2 % of the tokens may be skipped for that
(tests/test_ctc_score_window_ref.py holds the reference's own near-ties inside that cap)."""
import numpy as np
import pytest

import ctc_score_ref as R
import ctc_score_window_ref as WR
from reverb_amd import _lib
from reverb_amd._lib import dptr, fptr, iptr

pytestmark = pytest.mark.gpu
V = WR.V
LL_PER_FRAME = 1e-5
TOL_POST = 9.1e-4        # absolute, peak_post: 4 x the recorded 2.27e-4 (the peaky case)
TOL_OCC = 1e-3           # relative, occupancy: recorded 4.34e-4 (the peaky case), 4 x that is above the cap
TOL_MEAN = 1.7e-4        # relative to max(mean_frame, 1): 4 x the recorded 4.25e-5 (the peaky case)
REPEATS = (2, 8, 16)     # y[i] == y[i - 1] at token pairs that straddle a thread boundary, SPT = 4 / 16 / 32


def tlib():
    return _lib.load_test()


def window_score(lp, y, window=0, slab=None, lo_force=None, post=True, expect_ok=True):
    T, L = lp.shape[0], len(y)
    y = np.ascontiguousarray(y, np.int32)
    W = WR.effective_window(L, window)
    n = len(WR.segments(T, W, slab or T))
    ll = np.full(1, np.nan, np.float64)
    occ, mean, peak = (np.full(L, np.nan, np.float32) for _ in range(3))
    pf = np.full(L, -1, np.int32)
    lo, best = np.full(T, -5, np.int32), np.full(n, -5, np.int32)
    f = None if lo_force is None else np.ascontiguousarray(lo_force, np.int32)
    assert f is None or len(f) == n
    rc = tlib().rvb_test_ctc_score_window(fptr(lp), T, lp.shape[1], iptr(y), L, 0, slab or T, window, None if f is None else iptr(f),
                                          dptr(ll), fptr(occ) if post else None, fptr(mean) if post else None,
                                          fptr(peak) if post else None, iptr(pf) if post else None, iptr(lo), iptr(best))
    if not expect_ok:
        return rc, tlib().rvb_last_error().decode(), (ll, occ, lo)
    assert rc == 0, tlib().rvb_last_error().decode()
    return (float(ll[0]), occ, mean, peak, pf), lo, best


def plain_score(lp, y, slab=None, post=True):
    T, L = lp.shape[0], len(y)
    y = np.ascontiguousarray(y, np.int32)
    ll = np.zeros(1, np.float64)
    occ, mean, peak = (np.full(L, np.nan, np.float32) for _ in range(3))
    pf = np.full(L, -1, np.int32)
    rc = tlib().rvb_test_ctc_score(fptr(lp), T, lp.shape[1], iptr(y), L, 0, slab or T, dptr(ll), fptr(occ), fptr(mean), fptr(peak), iptr(pf))
    assert rc == 0, tlib().rvb_last_error().decode()
    return float(ll[0]), occ, mean, peak, pf


def check_against_band(tag, lp, y, got, lo_of, W, frames=True, keep=()):
    ll, occ, mean, peak, pf = got
    T = lp.shape[0]
    ref_ll, ref, kept = WR.score(lp, y, lo_of, W, keep_alpha_at=keep)
    e_ll = abs(ll - ref_ll)
    e_post = float(np.abs(peak - ref["peak_post"]).max())
    e_occ = float((np.abs(occ - ref["occupancy"]) / ref["occupancy"]).max())
    e_mean = float((np.abs(mean - ref["mean_frame"]) / np.maximum(ref["mean_frame"], 1.0)).max())
    clear = ref["peak_post"] - ref["second"] > TOL_POST
    print("%s: T %d L %d W %d loglik %.9g err %.3g (%.3g per frame) peak_post %.3g occupancy %.3g mean_frame %.3g peak_frame skipped %d of %d"
          % (tag, T, len(y), W, ll, e_ll, e_ll / T, e_post, e_occ, e_mean, int((~clear).sum()), len(y)))
    assert not np.isnan(ll) and not any(np.isnan(a).any() for a in (occ, mean, peak))
    assert e_ll <= LL_PER_FRAME * T
    assert e_post <= TOL_POST and e_occ <= TOL_OCC and e_mean <= TOL_MEAN
    if frames:
        assert (~clear).sum() <= 0.02 * len(y)
    assert np.array_equal(pf[clear], ref["peak_frame"][clear])
    assert float(occ.sum()) <= T * (1 + TOL_OCC)
    return ref_ll, kept


@pytest.mark.parametrize("L,T,slabs", [(20, 64, (64, 63, 7, 1)), (2100, 2200, (2200, 1000, 2199)), (8200, 8300, (8300, 8299))])
def test_a_still_window_gives_the_plain_kernels_bits(L, T, slabs):
    """window_states = 0 on a lattice below the default window: W = S_pad, the window never moves, one case per states-per-thread.
    What this pins beyond the carried state: the compiler contracts `occ += p * inv` and `ts += g * t` into fused multiply-adds for
    SOME tokens of a thread, and which ones depends on how the thread's bounds are written; the windowed backward kernel writes them
    in the plain kernel's form for that reason (a predicate on the thread gave occupancies that differed in the last bit)."""
    lp, y = R.make_lattice(300 + L, T, V, L, 1.0, [i for i in REPEATS if i < L])
    base = plain_score(lp, y)
    for s in slabs:
        got, lo, best = window_score(lp, y, 0, s)
        assert (lo == 0).all()
        assert got[0] == base[0], "loglik differs from rvb_test_ctc_score's with slab_rows = %d" % s
        for a, b, name in zip(got[1:], base[1:], ("occupancy", "mean_frame", "peak_post", "peak_frame")):
            assert np.array_equal(a, b), "%s differs from rvb_test_ctc_score's with slab_rows = %d" % (name, s)
        fwd, _, _ = window_score(lp, y, 0, s, post=False)
        assert fwd[0] == base[0], "the forward-only call disagrees on loglik"


def check_moving(tag, lp, y, W, slab):
    T, S = lp.shape[0], 2 * len(y) + 1
    got, lo_of, best = window_score(lp, y, W, slab)
    segs = WR.segments(T, W, slab)
    lo_prev, best_prev = 0, -1
    for (f0, f1), b in zip(segs, best):                                      # the policy, fed with the device's own best states
        want = WR.next_lo(S, T, W, f0, f1, lo_prev, best_prev)
        assert (lo_of[f0:f1] == want).all(), "launch [%d, %d): window %d, the policy says %d" % (f0, f1, lo_of[f0], want)
        lo_prev, best_prev = want, int(b)
    assert lo_of[-1] > 0, "the window moved"
    _, kept = check_against_band(tag, lp, y, got, lo_of, W, keep=[f1 - 1 for _, f1 in segs])
    for (f0, f1), b in zip(segs, best):                                      # the reported best state is a maximum of the reference's row
        lo = int(lo_of[f0])
        row = kept[f1 - 1][max(lo, WR.live_from(S, T, f1 - 1)):min(lo + W, S)]
        if row.size == 0 or not row.max() > -np.inf:
            assert b == -1
        else:
            assert max(lo, WR.live_from(S, T, f1 - 1)) <= b < min(lo + W, S)
            assert kept[f1 - 1][b] >= row.max() - 1e-4, "launch [%d, %d): best %d is %.3g below the row maximum" % (
                f0, f1, b, row.max() - kept[f1 - 1][b])


@pytest.mark.parametrize("slab", WR.MOVING[0][3])
def test_moving_window_4_states_per_thread(slab):
    L, T, W, _ = WR.MOVING[0]
    lp, y = WR.moving_case(L, T)
    check_moving("move4/%d" % slab, lp, y, W, slab)


@pytest.mark.parametrize("L,T,W,slabs", WR.MOVING[1:])
def test_moving_window_16_and_32_states_per_thread(L, T, W, slabs):
    """L = 8400: the window can move only 192 states, the smallest lattice that moves a window of 32 states per thread"""
    lp, y = WR.moving_case(L, T)
    check_moving("move%d" % (16 if W <= 16384 else 32), lp, y, W, slabs[0])


def test_the_cut_at_a_move():
    """a forced jump of the window at a launch boundary, through the planted path: the call succeeds, the results are the band
    reference's, and the cut carried mass (more than 1 nat of it)"""
    lp, y, free, forced = WR.cut_case()
    T, W = lp.shape[0], 256
    got, lo_of, _ = window_score(lp, y, W, T, lo_force=forced)
    assert np.array_equal(lo_of, WR.lo_per_frame(T, W, T, forced))
    assert lo_of[WR.CUT_G0 - 1] < WR.CUT_LO == lo_of[WR.CUT_G0]
    ref_ll, _ = check_against_band("cut", lp, y, got, lo_of, W)
    free_ll = WR.score(lp, y, WR.lo_per_frame(T, W, T, free), W)[0]
    print("cut: unforced %.6f forced %.6f" % (free_ll, ref_ll))
    assert free_ll - ref_ll > 1.0


def test_peaky_inputs_give_no_nan():
    """logits x 6 under a moving window; compared without the cap on skipped peak frames, as test_ctc_score_gpu.py does"""
    lp, y = R.make_lattice(500, 4096, V, 300, 6.0, [150])
    got, lo_of, _ = window_score(lp, y, 256, 4096)
    assert np.isfinite(got[0]) and lo_of[-1] > 0
    check_against_band("peaky", lp, y, got, lo_of, 256, frames=False)


def test_an_infeasible_band_is_refused_after_the_pass():
    """T = L: one path, 2 t + 1 at frame t; the forced window jumps far above it"""
    lp, y = R.make_lattice(600, 300, V, 300)
    n = len(WR.segments(300, 256, 300))
    rc, msg, (ll, occ, lo) = window_score(lp, y, 256, 300, lo_force=[0] + [352] * (n - 1), expect_ok=False)
    assert rc == -1 and "infeasible: no path inside the window of 256 states emits the transcript over 300 frames" in msg
    assert np.isnan(ll[0]) and np.isnan(occ).all() and (lo == -5).all(), "outputs untouched"
    got, _, _ = window_score(lp, y, 256, 300)                                # the policy's own windows keep the path
    assert np.abs(got[3] - 1.0).max() <= 1e-5
