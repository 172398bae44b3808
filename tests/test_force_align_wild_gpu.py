"""CTC Viterbi kernels with wildcards (the WILD instantiations of csrc/ctc_viterbi.hip) through the lab hook rvb_test_ctc_viterbi_wild.

Truth, by definition: append the column w + bias (one fp32 addition) to the [T, V] log-probs, give the wildcard the id V, and run the
numpy restatement tests/force_align_ref.py::force_align, which is pinned to the reference's goldens, on that [T, V + 1] matrix.  w is
the row maximum of lp, so in the quantised kind a wildcard ties with the model's own best label on every frame and the kernel's tie
rule (first maximum in the order s, s-1, s-2) decides.  Labels are compared identically and scores bit for bit: the only arithmetic
is fp32 addition, so there is no tolerance anywhere in this file."""
import numpy as np
import pytest

import force_align_ref as R
from reverb_amd import _lib

pytestmark = pytest.mark.gpu
W = -2                     # RVB_CTC_WILDCARD
BIASES = (0.0, -0.75)


def wild_hook(lib, lp, w, bias, y, slab, blank=0):
    T, V = lp.shape
    labels = np.full(T, -7, np.int32)
    score = np.full(1, 123.0, np.float32)
    rc = lib.rvb_test_ctc_viterbi_wild(_lib.fptr(lp), T, V, _lib.fptr(w), bias, _lib.iptr(np.ascontiguousarray(y, np.int32)), len(y), blank,
                                       slab, _lib.iptr(labels), _lib.fptr(score))
    return rc, labels, score[0]


def viterbi_wild(lib, lp, w, bias, y, slab):
    rc, labels, score = wild_hook(lib, lp, w, bias, y, slab)
    _lib.check(rc, "rvb_test_ctc_viterbi_wild")
    return labels, score


def truth(lp, w, bias, y):
    """force_align on [lp | w + bias] with the wildcard as label V; its labels with V written back as the sentinel"""
    V = lp.shape[1]
    ext = np.ascontiguousarray(np.concatenate([lp, (w + np.float32(bias)).astype(np.float32)[:, None]], axis=1))
    assert ext.dtype == np.float32
    ye = np.where(np.asarray(y) == W, V, y)
    labels, score = R.force_align(ext, ye)
    return np.where(labels == V, W, labels).astype(np.int32), score


def same(got, want):
    (gl, gs), (wl, ws) = got, want
    bad = np.nonzero(gl != wl)[0]
    assert bad.size == 0, "labels differ at %d frames, first %s" % (bad.size, bad[:5])
    assert np.float32(gs).tobytes() == np.float32(ws).tobytes(), (gs, ws)


def place(y, where):
    """the transcript with wildcards at a named placement"""
    y = np.array(y, np.int32)
    L = len(y)
    at = {"first": [0], "last": [L - 1], "middle": [L // 2], "fifth": list(range(0, L, 5)), "pair": [L // 2 - 1, L // 2] if L >= 2 else [0],
          "all": list(range(L))}[where]
    y[at] = W
    return y


PLACEMENTS = ("first", "last", "middle", "fifth", "pair", "all")
SMALL = [(1, 1), (7, 2)]
LARGE = [(512, 199), (8192 + 3, 3000)]
# with one token every placement is the wildcard alone
CASES = [(T, L, k, p) for T, L in SMALL + LARGE for k in ("random", "quant") for p in (PLACEMENTS if L > 1 else ("all",))]


@pytest.mark.parametrize("T,L,kind,where", CASES)
def test_identical_to_the_restatement_with_a_wildcard_column(lib, T, L, kind, where):
    lp, y, _ = R.make_case(300 + T % 97 + L, T, 48, L, kind)
    y = place(y, where)
    w = lp.max(axis=1)
    for bias in BIASES:
        want = truth(lp, w, bias, y)
        assert R.collapse(np.where(want[0] == W, 48, want[0])).tolist() == np.where(y == W, 48, y).tolist()
        for slab in ((8192, 64, 1) if (T, L) in SMALL else (8192, 1000)):
            same(viterbi_wild(lib, lp, w, bias, y, slab), want)


# states per thread 4: S <= 4096 (2 tokens per thread); 16: S <= 16384 (8); 32: S <= 32767 (16) -- each at its smallest and largest
# S, once, with wildcards at the first and last token and at a token that is the first of its thread in every instantiation (its
# predecessor two states below lives in the left neighbour) and the one before it (the last of that neighbour: an adjacent pair
# across a thread boundary, which must not skip)
@pytest.mark.parametrize("L", [2047, 2048, 8191, 8192, 16383])
def test_every_wild_instantiation_at_its_edges(lib, L):
    T = int(L * 1.25)
    lp, y, _ = R.make_case(11 + L, T, 32, L, "quant")
    edge = (L // 2) // 16 * 16
    y = np.array(y, np.int32)
    y[[0, L - 1, edge - 1, edge]] = W
    w = lp.max(axis=1)
    want = truth(lp, w, 0.0, y)
    same(viterbi_wild(lib, lp, w, 0.0, y, 8192), want)
    same(viterbi_wild(lib, lp, w, 0.0, y, 1000), want)


@pytest.mark.parametrize("T,L,kind", [(7, 2, "quant"), (512, 199, "random"), (512, 199, "quant"), (8192 + 3, 3000, "quant")])
def test_without_a_wildcard_the_plain_kernel_answers(lib, T, L, kind):
    lp, y, _ = R.make_case(300 + T % 97 + L, T, 48, L, kind)
    labels = np.full(T, -7, np.int32)
    score = np.zeros(1, np.float32)
    _lib.check(lib.rvb_test_ctc_viterbi(_lib.fptr(lp), T, 48, _lib.iptr(y), L, 0, 1000, _lib.iptr(labels), _lib.fptr(score)),
               "rvb_test_ctc_viterbi")
    for bias in BIASES:
        same(viterbi_wild(lib, lp, lp.max(axis=1), bias, y, 1000), (labels, score[0]))


def test_refusals_by_name_leave_the_outputs_untouched(lib):
    lp, y, _ = R.make_case(1, 20, 8, 5, "random")
    y = place(y, "middle")
    w = lp.max(axis=1)
    for bias, word in ((0.5, b"bias"), (float("nan"), b"bias"), (float("-inf"), b"bias")):
        rc, labels, score = wild_hook(lib, lp, w, bias, y, 64)
        assert rc == -1 and word in lib.rvb_last_error() and np.all(labels == -7) and score == 123.0
    # an adjacent pair of wildcards is a repeated label: L tokens + 1 repeat need L + 1 frames
    pair = np.array([1, W, W, 2, 3], np.int32)
    rc, labels, score = wild_hook(lib, lp[:5], w[:5], 0.0, pair, 64)
    assert rc == -1 and b"infeasible" in lib.rvb_last_error() and b"1 adjacent repeats" in lib.rvb_last_error()
    assert np.all(labels == -7) and score == 123.0
    rc, labels, score = wild_hook(lib, lp[:6], w[:6], 0.0, pair, 64)
    assert rc == 0 and R.collapse(labels).tolist() == pair.tolist()
    # the plain hook still takes the sentinel for an id outside the vocabulary
    out = np.full(20, -7, np.int32); sc = np.zeros(1, np.float32)
    assert lib.rvb_test_ctc_viterbi(_lib.fptr(lp), 20, 8, _lib.iptr(y), 5, 0, 64, _lib.iptr(out), _lib.fptr(sc)) == -1
    assert b"outside" in lib.rvb_last_error() and np.all(out == -7)
