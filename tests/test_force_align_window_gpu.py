"""The windowed CTC Viterbi kernels (csrc/ctc_viterbi_window.hip) through the lab hook rvb_test_ctc_viterbi_window against the numpy
restatement tests/force_align_window_ref.py: labels, the window of every frame and the margin EQUAL, the score bit-identical.  The
only arithmetic is one fp32 add per cell on the same lp bits, and the window policy is integer arithmetic on a first-maximum state, so
there is no tolerance anywhere in this file."""
import functools

import numpy as np
import pytest

import force_align_ref as R
import force_align_window_ref as WR
from reverb_amd import _lib
from test_force_align_window_ref import DECOY_SEED

pytestmark = pytest.mark.gpu


def window(lib, lp, y, W, slab, w=None, bias=0.0, blank=0):
    T, V = lp.shape
    labels, lo = np.full(T, -7, np.int32), np.full(T, -7, np.int32)
    score, margin = np.zeros(1, np.float32), np.full(1, -7, np.int32)
    _lib.check(lib.rvb_test_ctc_viterbi_window(_lib.fptr(lp), T, V, None if w is None else _lib.fptr(w), bias,
                                               _lib.iptr(np.ascontiguousarray(y, np.int32)), len(y), blank, slab, W, _lib.iptr(labels),
                                               _lib.fptr(score), _lib.iptr(lo), _lib.iptr(margin)), "rvb_test_ctc_viterbi_window")
    return labels, score[0], lo, int(margin[0])


def exact(lib, lp, y, slab=8192, blank=0):
    T, V = lp.shape
    labels, score = np.full(T, -7, np.int32), np.zeros(1, np.float32)
    _lib.check(lib.rvb_test_ctc_viterbi(_lib.fptr(lp), T, V, _lib.iptr(np.ascontiguousarray(y, np.int32)), len(y), blank, slab,
                                        _lib.iptr(labels), _lib.fptr(score)), "rvb_test_ctc_viterbi")
    return labels, score[0]


def same(got, want):
    (gl, gs, glo, gm), (wl, ws, wlo, wm) = got, want
    bad = np.nonzero(glo != wlo)[0]
    assert bad.size == 0, "windows differ at %d frames, first %s: %s / %s" % (bad.size, bad[:5], glo[bad[:5]], wlo[bad[:5]])
    bad = np.nonzero(gl != wl)[0]
    assert bad.size == 0, "labels differ at %d frames, first %s" % (bad.size, bad[:5])
    assert np.float32(gs).tobytes() == np.float32(ws).tobytes(), (gs, ws)
    assert gm == wm, (gm, wm)


@functools.lru_cache(maxsize=None)
def case(seed, T, V, L, kind):
    return R.make_case(seed, T, V, L, kind)


@functools.lru_cache(maxsize=None)
def ref(seed, T, V, L, kind, W, slab):
    lp, y, _ = case(seed, T, V, L, kind)
    return WR.force_align_window(lp, y, W, slab)


def holds_the_end(lo, L, W):
    S = 2 * L + 1
    assert S % 32 != 0 and lo[-1] > 0 and lo[-1] <= S - 1 < lo[-1] + W


@pytest.mark.parametrize("kind", ["random", "quant"])
@pytest.mark.parametrize("slab", [97, 600])
def test_many_shifts_and_a_slab_edge_inside_a_launch(lib, kind, slab):
    """W = 256, S = 1001, T = 600: launches of 48 frames, cut again wherever a slab of 97 rows ends."""
    want = ref(11, 600, 16, 500, kind, 256, slab)
    lp, y, _ = case(11, 600, 16, 500, kind)
    same(window(lib, lp, y, 256, slab), want)
    holds_the_end(want[2], 500, 256)
    assert len(set(want[2].tolist())) > 10


# one case per instantiation at its edge: 4 states per thread with all 1024 threads, the narrowest window of 16, of 32, the widest of 32
EDGES = [(4096, 5000, 6500), (4352, 5000, 6500), (16640, 9000, 11000), (32768, 20000, 24000)]


@pytest.mark.parametrize("W,L,T", EDGES)
def test_every_instantiation_at_its_edge(lib, W, L, T):
    """the last: 20 000 tokens, above the one-workgroup aligner's cap of 16 383; its back-pointers take T W / 4 = 196 MB"""
    want = ref(7, T, 32, L, "random", W, 8192)
    lp, y, _ = case(7, T, 32, L, "random")
    same(window(lib, lp, y, W, 8192), want)
    holds_the_end(want[2], L, W)
    assert R.collapse(want[0]).tolist() == y.tolist()


@pytest.mark.parametrize("kind", ["random", "quant", "repeat"])
def test_a_window_that_holds_the_lattice_is_the_exact_kernel(lib, kind):
    lp, y, _ = case(21, 2000, 32, 700, kind)
    want = exact(lib, lp, y, 64)
    for W, slab in ((0, 64), (2048, 8192)):                     # S = 1401: both windows are reduced to 1408 states
        labels, score, lo, margin = window(lib, lp, y, W, slab)
        assert np.array_equal(labels, want[0]) and np.float32(score).tobytes() == np.float32(want[1]).tobytes()
        assert not lo.any() and margin == 1408


def test_a_wildcard_run_that_straddles_a_window_shift(lib):
    lp, y, _ = case(5, 1500, 16, 640, "random")
    w = np.ascontiguousarray(lp.max(1))
    yw = np.concatenate([y[:300], [WR.WILDCARD], y[330:]]).astype(np.int32)
    want = WR.force_align_window(lp, yw, 256, 97, w=w, bias=-0.5)
    run = np.nonzero(want[0] == WR.WILDCARD)[0]
    starts = [f0 for f0, _ in WR.segments(1500, 256, 97)]
    # the path sits on the wildcard across several launches, each of which rebuilds the wildcard bits from its own lo != 0
    assert run.size > 60 and sum(run[0] < f0 <= run[-1] for f0 in starts) >= 2 and want[2][run[0]] > 0
    same(window(lib, lp, yw, 256, 97, w=w, bias=-0.5), want)


def test_the_wild_form_without_a_wildcard_gives_the_same_bits(lib):
    lp, y, _ = case(11, 600, 16, 500, "quant")
    w = np.ascontiguousarray(lp.max(1))
    same(window(lib, lp, y, 256, 97, w=w, bias=-0.25), ref(11, 600, 16, 500, "quant", 256, 97))
    lp, y, _ = case(7, 6500, 32, 5000, "random")
    w = np.ascontiguousarray(lp.max(1))
    for W in (4096, 4352):
        same(window(lib, lp, y, W, 8192, w=w), ref(7, 6500, 32, 5000, "random", W, 8192))


def test_the_decoy(lib):
    """the window follows a runaway partial path and drops the true one: the call still succeeds, reports margin 0 and a score below
    the exact kernel's"""
    lp, y = WR.decoy_case(DECOY_SEED)
    want = WR.force_align_window(lp, y, WR.DECOY_W, 8192)
    got = window(lib, lp, y, WR.DECOY_W, 8192)
    same(got, want)
    assert got[3] == 0 and float(got[1]) < float(exact(lib, lp, y)[1]) - 100.0


def test_neginf_and_minimum_length(lib):
    for kind, T, L, W in (("neginf", 4000, 700, 256), ("min_t", 0, 3000, 1024), ("min_t_quant", 0, 5000, 512)):
        lp, y, T = R.make_case(5, T, 24, L, kind)
        for slab in (8192, 64):
            same(window(lib, lp, y, W, slab), WR.force_align_window(lp, y, W, slab))


def test_a_path_that_does_not_exist_inside_the_window_is_refused(lib):
    lp, y, _ = R.make_case(1, 700, 8, 300, "random")
    lp[377, :] = -np.inf
    T = lp.shape[0]
    labels, lo = np.full(T, -7, np.int32), np.full(T, -7, np.int32)
    score, margin = np.zeros(1, np.float32), np.full(1, -7, np.int32)
    rc = lib.rvb_test_ctc_viterbi_window(_lib.fptr(lp), T, 8, None, 0.0, _lib.iptr(y), len(y), 0, 64, 256, _lib.iptr(labels),
                                         _lib.fptr(score), _lib.iptr(lo), _lib.iptr(margin))
    assert rc == -1 and b"infeasible: no path inside the window" in lib.rvb_last_error() and np.all(labels == -7) and np.all(lo == -7)
