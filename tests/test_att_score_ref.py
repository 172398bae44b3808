"""tests/att_score_ref.py (the fp64 restatement the GPU tests compare the engine with) against tests/golden/att_score.json: the losses
and accuracies the unmodified reference's LabelSmoothingLoss and th_accuracy return on the same seeded logits
(scripts/gen_golden_att_score.py).  Smoothing 0 and 0.1, both normalisations, V = 5 and 48, a padded batch of 2 (ignore_id rows) and
a tie for the arg-max.  The closed form the engine's host code composes must agree with the dense sum to 1e-12 relative."""
import json
import os

import numpy as np
import pytest

import att_score_ref as R
from conftest import ROOT
from reverb_amd import _lib

GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "att_score.json")))
CASES = GOLDEN["cases"]


def test_golden_covers_the_cases():
    assert GOLDEN["ignore_id"] == R.IGNORE_ID
    assert {c["smoothing"] for c in CASES} == {0.0, 0.1} and {c["normalize_length"] for c in CASES} == {False, True}
    assert {c["V"] for c in CASES} == {5, 48}
    assert any(len(c["lens"]) == 2 and c["lens"][0] != c["lens"][1] for c in CASES) and any(c["tie"] for c in CASES)
    assert set(CASES[0]) == {"seed", "lens", "V", "scale", "tie", "smoothing", "normalize_length", "loss", "accuracy"}


@pytest.mark.parametrize("case", CASES, ids=lambda c: "s%d-V%d-lsm%g-%s%s" % (c["seed"], c["V"], c["smoothing"],
                                                                                "len" if c["normalize_length"] else "batch",
                                                                                "-tie" if c["tie"] else ""))
def test_restatement_matches_the_reference(case):
    x, t = R.make_case(case["seed"], case["lens"], case["V"], case["scale"], case["tie"])
    want = float(case["loss"])
    dense = R.loss(x, t, case["smoothing"], case["normalize_length"])
    closed = R.loss(x, t, case["smoothing"], case["normalize_length"], closed=True)
    assert abs(dense - want) <= 1e-12 * abs(want)
    assert abs(closed - dense) <= 1e-12 * abs(dense)
    correct, n = R.accuracy(x, t)
    assert n == sum(case["lens"])
    assert float(np.float32(correct) / np.float32(n)) == float(case["accuracy"])      # th_accuracy divides in float32


def test_the_tie_goes_to_the_lowest_index_and_counts_as_wrong():
    x, t = R.make_case(5, [5], 5, 2.0, True)
    row = x[0, 0]
    top = np.flatnonzero(row == row.max())
    assert len(top) == 2 and t[0, 0] == top[1] and R.row_stats(x[0])[2][0] == top[0]
    correct, n = R.accuracy(x, t)
    x2 = x.copy()
    x2[0, 0, top[0]] -= 1.0                       # without the duplicate the target is the maximum
    assert R.accuracy(x2, t) == (correct + 1, n)


def test_zero_smoothing_is_the_cross_entropy():
    x, t = R.make_case(2, [12], 48)
    lp = R.log_softmax(x[0])
    assert abs(R.loss(x, t, 0.0, False) + lp[np.arange(12), t[0]].sum()) <= 1e-12 * 30
    assert np.all(R.kl_dense(x[0], t[0], 0.1) >= 0.0)                                  # a KL divergence


def test_entry_points_are_declared_bound_and_kept_out_of_the_product():
    import re
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "reverb_amd", "csrc", "test_api.h")).read(), flags=re.S)
    m = re.search(r"\brvb_test_row_xent\s*\(([^)]*)\)", text)
    assert m and len(m.group(1).split(",")) == 10 == len(_lib.TEST_SIGNATURES["rvb_test_row_xent"][1])
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rvb.h")).read(), flags=re.S)
    m = re.search(r"\brvb_attention_score\s*\(([^)]*)\)", text)
    assert m and len(m.group(1).split(",")) == 14 == len(_lib.SIGNATURES["rvb_attention_score"][1])
    product, tlib = _lib.load(), _lib.load_test()
    assert hasattr(product, "rvb_attention_score") and hasattr(tlib, "rvb_test_row_xent") and not hasattr(product, "rvb_test_row_xent")


def test_row_xent_hook_checks_its_arguments_before_any_device_work():
    """ptr that does not ascend from 0, a target outside [0, V) and ld < V are refused (E_ARG = -1) before the hook looks for a device,
    so this holds with and without a GPU: the kernel never sees an index it could read out of bounds with."""
    lib = _lib.load_test()
    x = np.zeros((2, 8), np.float32)
    logp, lse, sx, top = np.zeros(4, np.float32), np.zeros(2, np.float32), np.zeros(2, np.float64), np.zeros(2, np.int32)

    def call(V, ld, ptr, tgt):
        p, t = np.array(ptr, np.int32), np.array(tgt, np.int32)
        return lib.rvb_test_row_xent(_lib.fptr(x), 2, V, ld, _lib.iptr(p), _lib.iptr(t), _lib.fptr(logp), _lib.fptr(lse), _lib.dptr(sx),
                                     _lib.iptr(top))
    assert call(8, 8, [0, 1, 2], [0, 8]) == -1 and b"target outside" in lib.rvb_last_error()
    assert call(8, 8, [0, 1, 2], [-1, 0]) == -1
    assert call(8, 8, [0, 2, 1], [0, 0]) == -1 and b"ptr decreases" in lib.rvb_last_error()
    assert call(8, 8, [1, 1, 2], [0, 0]) == -1
    assert call(8, 7, [0, 1, 2], [0, 0]) == -1
    assert call(0, 8, [0, 1, 2], [0, 0]) == -1
