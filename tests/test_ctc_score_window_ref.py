"""The band reference of the windowed full-sum score (tests/ctc_score_window_ref.py) against the whole-lattice reference and its own
invariants, and the refusals of the lab hook rvb_test_ctc_score_window that come before any device work.  No GPU."""
import os
import re

import numpy as np
import pytest

import ctc_score_ref as R
import ctc_score_window_ref as WR
from reverb_amd import _lib
from reverb_amd._lib import dptr, fptr, iptr

V = WR.V
HERE = os.path.dirname(os.path.abspath(__file__))


def tlib():
    return _lib.load_test()


def test_a_still_window_is_the_whole_lattice():
    for L, T in ((1, 3), (20, 64), (300, 340)):
        lp, y = R.make_lattice(11 + L, T, V, L, 1.0, [2] if L > 2 else [])
        ll, ref = R.score(lp, y)
        W = WR.effective_window(L, 0)
        assert W >= 2 * L + 1
        bll, band, _ = WR.score(lp, y, np.zeros(T, np.int64), W)
        assert abs(bll - ll) <= 1e-12 * max(1.0, abs(ll))
        for k in ("occupancy", "mean_frame", "peak_post", "second"):
            assert np.abs(band[k] - ref[k]).max() <= 1e-9
        assert np.array_equal(band["peak_frame"], ref["peak_frame"])


def test_posteriors_of_a_frame_sum_to_one_across_a_cut():
    lp, y, free, forced = WR.cut_case()
    T, W = lp.shape[0], 256
    lo_of = WR.lo_per_frame(T, W, T, forced)
    assert lo_of[WR.CUT_G0 - 1] < WR.CUT_LO == lo_of[WR.CUT_G0], "the forced schedule jumps at the launch boundary"
    g, ll, _ = WR.band_gamma(lp, y, lo_of, W)
    S = g.shape[1]
    for t in range(T):
        alive = np.zeros(S, bool)
        alive[lo_of[t]:min(lo_of[t] + W, S)] = True
        assert np.isneginf(g[t, ~alive]).all()
        assert abs(np.exp(g[t, alive]).sum() - 1.0) <= 1e-9
    free_ll = WR.score(lp, y, WR.lo_per_frame(T, W, T, free), W)[0]
    assert free_ll - ll > 1.0, "the cut carries mass: %.3f nats" % (free_ll - ll)
    assert R.loglik(lp, y) >= free_ll >= ll


def near_ties(ref):
    return int((ref["peak_post"] - ref["second"] <= 1e-3).sum())


@pytest.mark.parametrize("L,T,W,slabs", WR.MOVING)
def test_the_moving_inputs_stay_within_the_skip_cap(L, T, W, slabs):
    """the GPU file skips the peak frame of a token whose two largest posteriors are within its tolerance (<= 1e-3), 2 % of the tokens
    at the most: the reference's own near-ties stay inside that, on the windows the policy picks from the reference's best states"""
    lp, y = WR.moving_case(L, T)
    for slab in slabs:
        los, _ = WR.policy_schedule(lp, y, W, slab)
        assert los[-1] > 0, "the window moves"
        ref = WR.score(lp, y, WR.lo_per_frame(T, W, slab, los), W)[1]
        n = near_ties(ref)
        print("L %d T %d W %d slab %d: %d near-ties of %d, windows %s" % (L, T, W, slab, n, L, sorted(set(los))))
        assert n <= 0.02 * L


def test_the_cut_input_stays_within_the_skip_cap():
    lp, y, free, forced = WR.cut_case()
    T = lp.shape[0]
    for los in (free, forced):
        assert near_ties(WR.score(lp, y, WR.lo_per_frame(T, 256, T, los), 256)[1]) <= 0.02 * len(y)


def call(lp, y, window=0, slab=None, lo_force=None, post=True, blank=0):
    T, L = lp.shape[0], len(y)
    y = np.ascontiguousarray(y, np.int32)
    ll = np.full(1, 123.0, np.float64)
    occ = np.full(max(L, 1), 7.0, np.float32)
    lo = np.full(T, -5, np.int32)
    f = None if lo_force is None else np.ascontiguousarray(lo_force, np.int32)
    rc = tlib().rvb_test_ctc_score_window(fptr(lp), T, lp.shape[1], iptr(y if L else np.zeros(1, np.int32)), L, blank, slab or T, window,
                                          None if f is None else iptr(f), dptr(ll), fptr(occ) if post else None, None, None, None,
                                          iptr(lo), None)
    assert ll[0] == 123.0 and (occ == 7.0).all() and (lo == -5).all(), "a refusal leaves the outputs untouched"
    return rc, tlib().rvb_last_error().decode()


def test_refusals_come_before_device_work(monkeypatch):
    lp, y = R.make_lattice(21, 700, V, 300)
    for w in (100, 255, 32768 + 256, -256):
        rc, msg = call(lp, y, window=w)
        assert rc == -1 and "window_states %d must be 0" % w in msg
    rc, msg = call(lp, y[:0])
    assert rc == -1 and "empty transcript" in msg
    bad = y.copy()
    bad[7] = 0
    rc, msg = call(lp, bad)
    assert rc == -1 and "token 7 is the blank id 0" in msg
    bad[7] = -2                                                              # RVB_CTC_WILDCARD: no wildcards in a full sum
    rc, msg = call(lp, bad)
    assert rc == -1 and "token id -2 outside [0, 32)" in msg
    n = len(WR.segments(700, 256, 700))                                      # S_pad - W = 608 - 256 = 352
    ok = [0] * n
    for i, v in ((3, 48), (3, 384), (0, 32)):
        f = list(ok)
        f[i:] = [v] * (n - i)
        rc, msg = call(lp, y, window=256, lo_force=f)
        assert rc == -1 and "lo_force[%d] = %d must be a multiple of 32 in [0, 352]" % (i, v) in msg
    f = list(ok)
    f[3], f[4] = 64, 32
    rc, msg = call(lp, y, window=256, lo_force=f)
    assert rc == -1 and "lo_force[4] = 32" in msg and "not below the entry before it" in msg
    monkeypatch.setenv("RVB_CTC_SCORE_FAKE_NOMEM_ABOVE", "5000")
    rc, msg = call(lp, y, window=256)
    assert rc == -4 and "do not fit" in msg and str(700 * 256 * 4) + " bytes of alpha rows" in msg      # RVB_E_NOMEM, T * W * 4


def test_the_long_score_calls_are_exported_and_declared():
    header = open(os.path.join(HERE, "..", "include", "rvb.h")).read()
    lib = _lib.load()
    for name in ("begin", "feed", "loglik", "feed_back", "finish", "end"):
        sym = "rvb_ctc_score_long_" + name
        assert re.search(r"^int %s\(rvb_engine\*" % sym, header, re.M), sym + " is not declared in rvb.h"
        assert getattr(lib, sym) is not None
    for scope in ("ctc_fb_window_forward", "ctc_fb_window_backward"):
        assert '"%s"' % scope in header
