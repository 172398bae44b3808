"""CTC Viterbi kernels (csrc/ctc_viterbi.hip) through the lab hook rvb_test_ctc_viterbi: labels IDENTICAL to the reference's goldens and,
where the reference's Python loop is too slow, to the numpy restatement of the same recurrence (tests/force_align_ref.py); scores
bit-equal.  The only arithmetic is an fp32 add per cell, so there is no tolerance anywhere in this file."""
import json
import os

import numpy as np
import pytest

import force_align_ref as R
from conftest import ROOT
from reverb_amd import _lib

pytestmark = pytest.mark.gpu
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "force_align.json")))
SLABS = (8192, 64, 1)


def viterbi(lib, lp, y, slab, blank=0):
    T, V = lp.shape
    labels = np.full(T, -7, np.int32)
    score = np.zeros(1, np.float32)
    _lib.check(lib.rvb_test_ctc_viterbi(_lib.fptr(lp), T, V, _lib.iptr(np.ascontiguousarray(y, np.int32)), len(y), blank, slab,
                                        _lib.iptr(labels), _lib.fptr(score)), "rvb_test_ctc_viterbi")
    return labels, score[0]


def same(got, want):
    (gl, gs), (wl, ws) = got, want
    bad = np.nonzero(gl != wl)[0]
    assert bad.size == 0, "labels differ at %d frames, first %s" % (bad.size, bad[:5])
    assert np.float32(gs).tobytes() == np.float32(ws).tobytes(), (gs, ws)


@pytest.mark.parametrize("slab", SLABS)
@pytest.mark.parametrize("case", GOLDEN["cases"], ids=lambda c: "%s-%d" % (c["kind"], c["seed"]))
def test_reference_goldens(lib, case, slab):
    lp, y, T = R.make_case(case["seed"], case["T"], case["V"], case["L"], case["kind"])
    labels, score = viterbi(lib, lp, y, slab)
    assert labels.tolist() == case["labels"]
    assert np.float32(score).tobytes() == R.force_align(lp, y)[1].tobytes()


# T x L of the issue (infeasible pairs left out: T >= L + repeats), random and quantised-tie inputs, every slab size
SHAPES = [(1, 1), (7, 1), (7, 2), (512, 1), (512, 2), (512, 199), (8192 + 3, 2), (8192 + 3, 199), (8192 + 3, 3000),
          (2 * 8192 + 5, 1), (2 * 8192 + 5, 199), (2 * 8192 + 5, 3000)]


# the "repeat" construction needs up to 2 L frames
SHAPE_KINDS = [(T, L, k) for T, L in SHAPES for k in ("random", "quant", "repeat") if k != "repeat" or T >= 2 * L]


@pytest.mark.parametrize("T,L,kind", SHAPE_KINDS)
def test_identical_to_the_restatement(lib, T, L, kind):
    lp, y, _ = R.make_case(100 + T % 97 + L, T, 48, L, kind)
    want = R.force_align(lp, y)
    for slab in SLABS:
        same(viterbi(lib, lp, y, slab), want)


# states per thread 4: S <= 4096; 16: S <= 16384; 32: S <= 32767 (the cap) -- each at its smallest and largest S
@pytest.mark.parametrize("L", [1, 2047, 2048, 8191, 8192, 16383])
@pytest.mark.parametrize("kind", ["random", "quant"])
def test_every_instantiation_at_its_edges(lib, L, kind):
    T = max(int(L * 1.25), 4)
    lp, y, _ = R.make_case(7 + L, T, 32, L, kind)
    want = R.force_align(lp, y)
    same(viterbi(lib, lp, y, 8192), want)
    same(viterbi(lib, lp, y, 1000), want)


def test_the_benched_hour_fits_one_lattice(lib):
    """T = 90 112 frames, 13 935 tokens (S = 27 871): the size requirement.  V = 64 keeps the host matrix at 23 MB."""
    lp, y, _ = R.make_case(2024, 90112, 64, 13935, "quant")
    want = R.force_align(lp, y)
    same(viterbi(lib, lp, y, 8192), want)
    assert R.collapse(want[0]).tolist() == y.tolist()


def test_neginf_and_minimum_length(lib):
    for kind, T, L in (("neginf", 4000, 700), ("min_t", 0, 3000), ("min_t_quant", 0, 5000)):
        lp, y, T = R.make_case(5, T, 24, L, kind)
        want = R.force_align(lp, y)
        for slab in (8192, 64):
            same(viterbi(lib, lp, y, slab), want)


def test_a_path_that_does_not_exist_is_refused(lib):
    lp, y, _ = R.make_case(1, 200, 8, 20, "random")
    lp[77, :] = -np.inf
    labels = np.full(200, -7, np.int32); score = np.zeros(1, np.float32)
    rc = lib.rvb_test_ctc_viterbi(_lib.fptr(lp), 200, 8, _lib.iptr(y), 20, 0, 64, _lib.iptr(labels), _lib.fptr(score))
    assert rc == -1 and b"infeasible" in lib.rvb_last_error() and np.all(labels == -7)
