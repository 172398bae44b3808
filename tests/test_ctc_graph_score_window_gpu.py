"""The windowed full-sum kernels over token graphs (csrc/ctc_graph_fb_window.hip) through the lab hook rvb_test_ctc_score_graph_window:
bit for bit against rvb_test_ctc_score_graph where the window holds the graph, and against the fp64 band restatement
(tests/graph_score_window_ref.py) on the device's own windows where it moves.

Bounds.  loglik: |got - ref| <= 1e-5 * T nats, the condition tests/test_ctc_score_gpu.py derives, not widened.  The per-node outputs
are measured against the fp64 band restatement, never against the kernel, on the nodes and in the relative forms
tests/test_ctc_graph_score_gpu.py defines (peak_post absolute; occupancy relative and mean_frame relative to max(mean_frame, 1), both
on the nodes of reference visit >= 1e-3; visit absolute): 4 x the largest error recorded on the MI355X over all cases of this file
(docs/tuning-log.md), capped by the standing conditions 1e-3 (peak_post, occupancy, mean_frame) and 1e-2 (visit).  peak_frame must
equal the restatement's wherever its two largest posteriors of the node differ by more than the posterior tolerance; among the nodes
with reference visit >= 0.5 at most 5 % may be skipped for that (tests/test_graph_score_window_ref.py shows that the restatement alone
stays inside that cap on the moving and the cut cases; the peaky case, where it ties on 14 of 81 nodes, asserts the frames that are
clear and no NaN).

Recorded on the MI355X, largest over all cases below (the forced cut gives visit, peak_post and occupancy, the policy's windows on
the same graph mean_frame, the moving window of 2048 nodes loglik): loglik 1.05e-8 T; visit 1.78e-5; peak_post 1.47e-5; occupancy
1.79e-5; mean_frame 1.12e-6."""
import numpy as np
import pytest

import ctc_score_ref as C
import graph_align_ref as G
import graph_align_window_ref as GW
import graph_score_ref as R
import graph_score_window_ref as WS
from reverb_amd import _lib
from reverb_amd._lib import dptr, fptr, iptr, u8ptr

pytestmark = pytest.mark.gpu
V = 32
LL_PER_FRAME = 1e-5
TOL_POST = 5.9e-5        # absolute, peak_post: 4 x the recorded 1.47e-5 (docs/tuning-log.md), below the cap of 1e-3
TOL_OCC = 7.2e-5         # relative, occupancy on nodes of visit >= 1e-3: 4 x the recorded 1.79e-5
TOL_MEAN = 4.5e-6        # relative to max(mean_frame, 1), same nodes: 4 x the recorded 1.12e-6
TOL_VISIT = 7.2e-5       # absolute: 4 x the recorded 1.78e-5, below the condition of 1e-2
REPEATS = (2, 8, 16)


def tlib():
    return _lib.load_test()


def pack(graph):
    tok = np.ascontiguousarray(graph[0], np.int32)
    off = np.ascontiguousarray(np.concatenate([[0], np.cumsum([len(p) for p in graph[1]])]).astype(np.int32))
    prd = np.array([p for ps in graph[1] for p in ps], np.int32)
    return tok, off, prd, np.ascontiguousarray(graph[2], np.uint8)


def window_score(lp, graph, window=0, slab=None, lo_force=None, post=True, expect=0):
    """-> (loglik, visit, occupancy, mean_frame, peak_post, peak_frame, lo_of [T], best per launch); with post=False the per-node
    arrays are None.  expect != 0: the refusal's code is asserted, the outputs must be untouched, -> the message"""
    lp = np.ascontiguousarray(lp, np.float32)
    T, N = lp.shape[0], len(graph[0])
    tok, off, prd, fin = pack(graph)
    ll = np.full(1, 123.0, np.float64)
    vis, occ, mean, peak = (np.full(N, -7.0, np.float32) for _ in range(4))
    pf, lo, best, launches = np.full(N, -7, np.int32), np.full(T, -7, np.int32), np.full(T, -7, np.int32), np.full(1, -7, np.int32)
    force = None if lo_force is None else np.ascontiguousarray(lo_force, np.int32)
    outs = [fptr(a) if post else None for a in (vis, occ, mean, peak)] + [iptr(pf) if post else None]
    rc = tlib().rvb_test_ctc_score_graph_window(fptr(lp), T, lp.shape[1], iptr(tok), N, iptr(off), iptr(prd), u8ptr(fin), 0, slab or T, window,
                                                iptr(force), dptr(ll), *outs, iptr(lo), iptr(best), iptr(launches))
    msg = tlib().rvb_last_error().decode()
    if expect:
        assert rc == expect, (rc, msg)
        assert ll[0] == 123.0 and all(np.all(a == -7) for a in (vis, occ, mean, peak, pf, lo, best, launches)), "a refusal wrote an output"
        return msg
    assert rc == 0, msg
    n = int(launches[0])
    if not post:
        return float(ll[0]), None, None, None, None, None, lo, best[:n]
    return float(ll[0]), vis, occ, mean, peak, pf, lo, best[:n]


def plain_score(lp, graph, post=True):
    lp = np.ascontiguousarray(lp, np.float32)
    tok, nn, off, prd, fin = R.flat([graph])
    N = len(graph[0])
    Ts = np.array([len(lp)], np.int32)
    ll = np.full(1, np.nan, np.float64)
    vis, occ, mean, peak = (np.full(N, np.nan, np.float32) for _ in range(4))
    pf = np.full(N, -1, np.int32)
    outs = [fptr(a) if post else None for a in (vis, occ, mean, peak)] + [iptr(pf) if post else None]
    rc = tlib().rvb_test_ctc_score_graph(fptr(lp), iptr(Ts), 1, lp.shape[1], iptr(tok), iptr(nn), iptr(off), iptr(prd), u8ptr(fin), 0, len(lp),
                                         dptr(ll), *outs)
    assert rc == 0, tlib().rvb_last_error().decode()
    return float(ll[0]), vis, occ, mean, peak, pf


def still_graph(L, seed):
    """a random multi-arc graph around a reading with repeated labels (also across an arc: the builders draw alternatives from the
    same small vocabulary)"""
    rng = np.random.default_rng([seed, L])
    _, y = C.make_lattice(seed, 1, V, L, 1.0, [i for i in REPEATS if i < L])
    y = [int(t) for t in y]
    return G.build(G.around(rng, y, V) if seed % 2 else G.groups(rng, y, V, n_alt=3))


_STILL = {}


def still_case(L, seed):
    if (L, seed) not in _STILL:
        g = still_graph(L, seed)
        lp = C.make_lattice(seed, len(g[0]) + 8, V, 1)[0]
        _STILL[(L, seed)] = (lp, g, plain_score(lp, g))
    return _STILL[(L, seed)]


# (L, seed, nodes per thread): graphs of about 60, 1500 and 3000 nodes, one per instantiation
STILL = [(20, 901, 1), (500, 902, 2), (1000, 904, 4)]


@pytest.mark.parametrize("L,seed,npt", STILL)
@pytest.mark.parametrize("cut", ["T", "T-1", "7", "1"])
def test_a_window_that_holds_the_graph_is_the_plain_kernel_bit_for_bit(L, seed, npt, cut):
    lp, g, want = still_case(L, seed)
    T, N = len(lp), len(g[0])
    W = GW.pad64(N)
    assert N <= 4096 and (1 if W <= 1024 else 2 if W <= 2048 else 4) == npt, (N, W)
    slab = {"T": T, "T-1": T - 1, "7": 7, "1": 1}[cut]
    got = window_score(lp, g, 0, slab)
    assert not got[6].any()                                          # the window never moved
    assert got[0] == want[0], "loglik differs from rvb_test_ctc_score_graph's with slab_rows = %d" % slab
    for k, name in enumerate(("visit", "occupancy", "mean_frame", "peak_post", "peak_frame"), 1):
        assert np.array_equal(got[k], want[k]), "%s differs from rvb_test_ctc_score_graph's with slab_rows = %d" % (name, slab)
    fwd = window_score(lp, g, 0, slab, post=False)
    assert fwd[0] == want[0] and plain_score(lp, g, post=False)[0] == want[0]


def errors(tag, lp, graph, got, ref_ll, ref):
    ll, vis, occ, mean, peak, pf = got[:6]
    T, N = lp.shape[0], len(graph[0])
    seen = ref["visit"] >= 1e-3
    e_ll = abs(ll - ref_ll)
    e_vis = float(np.abs(vis - ref["visit"]).max())
    e_post = float(np.abs(peak - ref["peak_post"]).max())
    e_occ = float((np.abs(occ - ref["occupancy"])[seen] / ref["occupancy"][seen]).max())
    e_mean = float((np.abs(mean - ref["mean_frame"])[seen] / np.maximum(ref["mean_frame"][seen], 1.0)).max())
    sure = ref["visit"] >= 0.5
    clear = ref["peak_post"] - ref["second"] > TOL_POST
    print("%s: T %d N %d loglik %.9g err %.3g (%.3g per frame) visit %.3g peak_post %.3g occupancy %.3g mean_frame %.3g "
          "peak_frame skipped %d of %d" % (tag, T, N, ll, e_ll, e_ll / T, e_vis, e_post, e_occ, e_mean, int((sure & ~clear).sum()), int(sure.sum())))
    return e_ll, e_vis, e_post, e_occ, e_mean, sure, clear


def check_against_band(tag, lp, graph, W, got, frames=True, rows_at=()):
    lo_of = got[6]
    ref_ll, ref = WS.score(lp, *graph, W, lo_of, rows_at=rows_at)
    e_ll, e_vis, e_post, e_occ, e_mean, sure, clear = errors(tag, lp, graph, got, ref_ll, ref)
    assert not np.isnan(got[0]) and not any(np.isnan(a).any() for a in got[1:5])
    assert e_ll <= LL_PER_FRAME * len(lp)
    assert e_vis <= TOL_VISIT
    assert e_post <= TOL_POST and e_occ <= TOL_OCC and e_mean <= TOL_MEAN
    if frames:
        assert (sure & ~clear).sum() <= 0.05 * sure.sum()
    assert np.array_equal(got[5][sure & clear], ref["peak_frame"][sure & clear])
    return ref_ll, ref


@pytest.mark.parametrize("tag,W,L,seed", WS.MOVING)
def test_a_moving_window_follows_the_policy_and_scores_as_the_band_restatement(tag, W, L, seed):
    lp, g = WS.moving_case(L, seed)
    T, N = len(lp), len(g[0])
    got = window_score(lp, g, W, WS.MOVING_SLAB)
    lo_of, best = got[6], got[7]
    want_lo, cuts = WS.replay_policy(*g, T, W, WS.MOVING_SLAB, best)         # the policy, replayed from the device's own best nodes
    assert len(cuts) == len(best) and np.array_equal(lo_of, want_lo)
    assert lo_of[-1] > 0 and np.all(np.diff(lo_of) >= 0) and np.all(lo_of % 64 == 0)
    _, ref = check_against_band("moving " + tag, lp, g, W, got, rows_at={f1 - 1 for _, f1, _ in cuts})
    # the node each launch reported: within 1e-4 of the maximum of the restatement's row of the launch's last frame over the same states
    rem = WS.frames_to_end(*g)
    for (f0, f1, lo), b in zip(cuts, best):
        vals, node = WS.live_row(ref["rows"][f1 - 1], rem, N, W, lo, T - f1)
        assert b >= 0 and vals[node == b].max() >= vals.max() - 1e-4, (tag, f1, int(b))
    fwd = window_score(lp, g, W, WS.MOVING_SLAB, post=False)
    assert fwd[0] == got[0] and np.array_equal(fwd[6], lo_of)


def test_a_forced_cut_through_mass_scores_as_the_band_restatement():
    lp, g, force, lo_of = GW.cut_case()
    got = window_score(lp, g, GW.CUT_W, GW.CUT_SLAB, lo_force=force)
    assert np.array_equal(got[6], lo_of)
    ref_ll, _ = check_against_band("cut", lp, g, GW.CUT_W, got)
    free = window_score(lp, g, 1024, GW.CUT_SLAB, post=False)       # 949 nodes: this window holds the graph
    print("cut: forced band %.6f, free %.6f" % (got[0], free[0]))
    assert free[0] - got[0] > 1.0 and abs(free[0] - R.loglik(lp, *g)) <= LL_PER_FRAME * len(lp)


def test_peaky_inputs_give_no_nan():
    lp, g = WS.peaky_case()
    got = window_score(lp, g, 256, WS.MOVING_SLAB)
    assert np.isfinite(got[0]) and got[6][-1] > 0
    check_against_band("peaky", lp, g, 256, got, frames=False)


def test_an_infeasible_forced_band_is_refused_after_the_pass_with_the_outputs_untouched():
    lp, g, _, _ = GW.cut_case()
    # the jump to 448 comes at frame 300, before any path can have reached the overlap of the two windows
    msg = window_score(lp, g, GW.CUT_W, 300, lo_force=[0, GW.CUT_LO, GW.CUT_LO, GW.CUT_LO], expect=-1)
    assert "infeasible: no path inside the window of 512 nodes ends in a final node after 1200 frames" in msg
    with pytest.raises(ValueError, match="infeasible"):
        WS.score(lp, *g, GW.CUT_W, np.where(np.arange(len(lp)) < 300, 0, GW.CUT_LO))
    got = window_score(lp, g, GW.CUT_W, 300)                         # the policy's own windows succeed
    assert got[6][-1] > 0
    check_against_band("policy on the cut graph", lp, g, GW.CUT_W, got)
