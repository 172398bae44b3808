"""The CTC forward-backward kernels (csrc/ctc_forward_backward.hip) through the lab hooks rvb_test_ctc_score / _batch, against the fp64
restatement (tests/ctc_score_ref.py) on the same fp32 log-prob bits.

Bounds.  loglik: |got - ref| <= 1e-5 * T nats, a condition: after normalisation the cells that matter have magnitude <= ~32, three
fp32 roundings per frame are 3 * 2^-24 * 32 = 6e-6, the ceiling is about twice that.  Posteriors and occupancies: 4 x the largest
error recorded on the MI355X over all cases of this file (docs/tuning-log.md), capped by the condition of 1e-3; the frame-weighted
mean is compared relative to max(mean_frame, 1).  peak_frame must equal the restatement's wherever its two largest posteriors of
the token differ by more than the posterior tolerance; at most 2 % of the tokens may be skipped for that."""
import numpy as np
import pytest

import ctc_score_ref as R
import force_align_ref as A
from reverb_amd import _lib
from reverb_amd._lib import dptr, fptr, iptr

pytestmark = pytest.mark.gpu
V = 32
LL_PER_FRAME = 1e-5
TOL_POST = 1e-3          # absolute, peak_post: recorded 4.43e-4, 4 x that is above the cap
TOL_OCC = 1e-3           # relative, occupancy: recorded 7.81e-4, 4 x that is above the cap
TOL_MEAN = 1.6e-4        # relative to max(mean_frame, 1): 4 x the recorded 3.84e-5
REPEATS = (2, 8, 16)     # y[i] == y[i - 1] at the token pairs (SPT / 2 - 1, SPT / 2) that straddle a thread boundary, SPT = 4 / 16 / 32


def tlib():
    return _lib.load_test()


def score(lp, y, slab=None, post=True, blank=0):
    T, L = lp.shape[0], len(y)
    y = np.ascontiguousarray(y, np.int32)
    ll = np.zeros(1, np.float64)
    occ, mean, peak = (np.full(L, np.nan, np.float32) for _ in range(3))
    pf = np.full(L, -1, np.int32)
    rc = tlib().rvb_test_ctc_score(fptr(lp), T, lp.shape[1], iptr(y), L, blank, slab or T, dptr(ll), fptr(occ) if post else None,
                                   fptr(mean) if post else None, fptr(peak) if post else None, iptr(pf) if post else None)
    assert rc == 0, tlib().rvb_last_error().decode()
    return (float(ll[0]), occ, mean, peak, pf) if post else float(ll[0])


def viterbi(lp, y):
    lab = np.zeros(lp.shape[0], np.int32)
    sc = np.zeros(1, np.float32)
    y = np.ascontiguousarray(y, np.int32)
    assert tlib().rvb_test_ctc_viterbi(fptr(lp), lp.shape[0], lp.shape[1], iptr(y), len(y), 0, lp.shape[0], iptr(lab), fptr(sc)) == 0
    return float(sc[0])


def check_against_ref(tag, lp, y, got, frames=True):
    ll, occ, mean, peak, pf = got
    T = lp.shape[0]
    ref_ll, ref = R.score(lp, y)
    e_ll = abs(ll - ref_ll)
    e_post = float(np.abs(peak - ref["peak_post"]).max())
    e_occ = float((np.abs(occ - ref["occupancy"]) / ref["occupancy"]).max())
    e_mean = float((np.abs(mean - ref["mean_frame"]) / np.maximum(ref["mean_frame"], 1.0)).max())
    clear = ref["peak_post"] - ref["second"] > TOL_POST
    print("%s: T %d L %d loglik %.9g err %.3g (%.3g per frame) peak_post %.3g occupancy %.3g mean_frame %.3g peak_frame skipped %d of %d"
          % (tag, T, len(y), ll, e_ll, e_ll / T, e_post, e_occ, e_mean, int((~clear).sum()), len(y)))
    assert not np.isnan(ll) and not any(np.isnan(a).any() for a in (occ, mean, peak))
    assert e_ll <= LL_PER_FRAME * T
    assert e_post <= TOL_POST and e_occ <= TOL_OCC and e_mean <= TOL_MEAN
    if frames:
        assert (~clear).sum() <= 0.02 * len(y)
    assert np.array_equal(pf[clear], ref["peak_frame"][clear])


@pytest.mark.parametrize("L", [1, 2047, 2048, 8191, 8192])
def test_instantiation_edges(L):
    """S = 3, 4095 / 4097 (4 -> 16 states per thread), 16383 / 16385 (16 -> 32), with repeats across a thread boundary"""
    rep = [i for i in REPEATS if i < L]
    T = L + len(rep) + 8
    lp, y = R.make_lattice(100 + L, T, V, L, 1.0, rep)
    assert A.min_frames(y) == L + len(rep)
    got = score(lp, y)
    fwd = score(lp, y, post=False)
    assert fwd == got[0], "the forward-only call and the call with posteriors disagree on loglik"
    check_against_ref("edge", lp, y, got)


@pytest.mark.parametrize("L", [1, 300, 2100, 8200])
def test_tightest_lattice_has_one_path(L):
    rep = [i for i in REPEATS if i < L]
    T = L + len(rep)
    lp, y = R.make_lattice(200 + L, T, V, L, 1.0, rep)
    ll, occ, mean, peak, pf = score(lp, y)
    vit = viterbi(lp, y)
    print("tight: T %d loglik %.9g viterbi %.9g diff %.3g" % (T, ll, vit, abs(ll - vit)))
    assert abs(ll - vit) <= LL_PER_FRAME * T
    assert np.abs(peak - 1.0).max() <= 1e-5 and np.abs(occ - 1.0).max() <= 1e-5
    frames = np.arange(L) + np.cumsum(np.isin(np.arange(L), rep))          # the only path: one frame per token, a blank before a repeat
    assert np.array_equal(pf, frames) and np.abs(mean - frames).max() <= 1e-5 * max(T, 1)


@pytest.mark.parametrize("L,T,slabs", [(20, 64, (1, 7, 64, 63)), (2100, 2200, (2200, 1000, 2199)), (8200, 8300, (8300, 8299))])
def test_results_do_not_depend_on_the_slabs(L, T, slabs):
    """slab_rows = T - 1 puts a forward boundary before frame T - 1 and a backward boundary above frame 1 (the backward slabs end at
    the last row)"""
    lp, y = R.make_lattice(300 + L, T, V, L, 1.0, [i for i in REPEATS if i < L])
    base = score(lp, y, slabs[0])
    if L == 20:
        check_against_ref("slab", lp, y, base)
    for s in slabs[1:]:
        got = score(lp, y, s)
        assert got[0] == base[0], "loglik changes with slab_rows = %d" % s
        for a, b in zip(got[1:], base[1:]):
            assert np.array_equal(a, b), "per-token results change with slab_rows = %d" % s
        assert score(lp, y, s, post=False) == base[0]


def test_batch_equals_one_by_one():
    # all three on the 4-states instance, alone or together: the order in which a row's posteriors are summed for its normaliser
    # follows the states per thread, so only launches of the same instance agree bit for bit
    shapes = [(5, 40), (300, 700), (2000, 2100)]
    cases = [R.make_lattice(400 + L, T, V, L, 1.0, [i for i in REPEATS if i < L]) for L, T in shapes]
    lp = np.ascontiguousarray(np.concatenate([c[0] for c in cases]))
    y = np.ascontiguousarray(np.concatenate([c[1] for c in cases]), np.int32)
    Ts = np.array([T for _, T in shapes], np.int32)
    Ls = np.array([L for L, _ in shapes], np.int32)
    for slab in (int(Ts.sum()), 1000):
        ll = np.zeros(3, np.float64)
        occ, mean, peak = (np.zeros(len(y), np.float32) for _ in range(3))
        pf = np.zeros(len(y), np.int32)
        rc = tlib().rvb_test_ctc_score_batch(fptr(lp), iptr(Ts), V, iptr(y), iptr(Ls), 3, 0, slab, dptr(ll), fptr(occ), fptr(mean), fptr(peak),
                                             iptr(pf))
        assert rc == 0, tlib().rvb_last_error().decode()
        t0 = 0
        for i, (clp, cy) in enumerate(cases):
            n = len(cy)
            one = score(clp, cy)
            assert one[0] == ll[i]
            for a, b in zip(one[1:], (occ, mean, peak, pf)):
                assert np.array_equal(a, b[t0:t0 + n])
            t0 += n


def test_peaky_inputs_give_no_nan():
    """logits scaled by 6: some states have all predecessors at -inf (underflow of the normalised alpha) for hundreds of frames.
    A token here holds a posterior of 1 - 1e-9 over several frames, so most peak frames are ties of the restatement itself (217 of
    300 tokens): the frames are compared where they are not, without the 2 % cap the other cases keep."""
    lp, y = R.make_lattice(500, 4096, V, 300, 6.0, [150])
    got = score(lp, y)
    assert np.isfinite(got[0])
    check_against_ref("peaky", lp, y, got, frames=False)


def test_refusals(monkeypatch):
    lp, y = R.make_lattice(600, 40, V, 10)
    ll = np.zeros(1, np.float64)
    occ = np.zeros(10, np.float32)
    lib = tlib()
    hole = lp.copy()
    hole[5, :] = -np.inf                                                     # no path with a finite score
    assert lib.rvb_test_ctc_score(fptr(hole), 40, V, iptr(y), 10, 0, 40, dptr(ll), None, None, None, None) != 0
    assert "infeasible: no path of 40 frames emits the transcript with a finite score" in lib.rvb_last_error().decode()
    monkeypatch.setenv("RVB_CTC_SCORE_FAKE_NOMEM_ABOVE", "5000")
    rc = lib.rvb_test_ctc_score(fptr(lp), 40, V, iptr(y), 10, 0, 40, dptr(ll), fptr(occ), None, None, None)
    msg = lib.rvb_last_error().decode()
    assert rc == -4 and "do not fit" in msg                                  # RVB_E_NOMEM
    assert str(40 * 32 * 4) + " bytes of alpha rows" in msg                  # 21 states padded to 32, 4 bytes per frame and state
    assert lib.rvb_test_ctc_score(fptr(lp), 40, V, iptr(y), 10, 0, 40, dptr(ll), None, None, None, None) == 0, "forward-only needs no rows"
    monkeypatch.delenv("RVB_CTC_SCORE_FAKE_NOMEM_ABOVE")
    assert lib.rvb_test_ctc_score(fptr(lp), 40, V, iptr(y), 10, 0, 40, dptr(ll), fptr(occ), None, None, None) == 0
