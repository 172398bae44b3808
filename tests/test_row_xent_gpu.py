"""row_xent (csrc/softmax_topk.hip) through the lab hook rvb_test_row_xent: per (row, target) pair the log-prob, per row lse, the sum of
the logits and the arg-max, against fp64 and against the sibling kernel behind rvb_test_lse_gather_multi.

Shapes, one failure mode each: V = 48 (less than one batch of loads: most lanes hold nothing), 1003 (V % 4 != 0: the scalar path
alone), 1024 (exactly one batch), 10001 in rows of 10004 (the engine's padded stride: vectors, then a one-element tail).  R = 9 rows
(not a multiple of the 4 rows of a block) with 1, 3, 0, 70, 2, 1, 1, 5, 2 targets: a row nobody asks still writes its statistics, one
has more targets than lanes.  Row 1 has its maximum planted at index 0, row 4 at V - 1 (in the tail where there is one), row 6 twice
(the lower index wins, as torch.argmax on the CPU), row 7 is scaled by 20.

Bounds.  logp: 3e-6 against fp64 log_softmax on the N(0, 2) rows, the bound tests/test_kernels_gpu.py applies to the sibling; and the
SAME BITS as the sibling where ld = V (this hook of the sibling has no stride; tests/test_rowlse_kernels_gpu.py holds the two to the
same bits at (10001, 10004) through the strided one).  sum_x: V max|x| 2^-23.  The loss of a pair is
    kl = const - (c - u) logp_t - u sum_x + u V lse,      c = 1 - smoothing, u = smoothing / (V - 1)
so its error is at most |c - u| 3e-6 <= 3e-6 from the target term, plus u V 3e-6 = smoothing V / (V - 1) 3e-6 from V lse (lse is held
to the bound of logp, whose error it is), plus u times the error of sum_x, u V max|x| 2^-23 = smoothing V / (V - 1) max|x| 2^-23 < 1.2e-7
for max|x| < 10: 3.5e-6 in all at smoothing 0.1, asserted at 5e-6.
The row scaled by 20: every fp32 quantity of the row (x_t, lse, logp = x_t - lse) is rounded relative to its magnitude, and the
3e-6 above is 1.57 units in the last place of values in [16, 32), the highest binade lse and |logp| of the N(0, 2) rows reach
(lse <= ln V + 2.2 < 11.5, |logp| <= lse + max|x| < 21 at V = 10001; a unit there is 2^-19 = 1.9e-6; the test checks they stay
below 32).  With M = max(|lse|, max |logp|) of the scaled row, a unit in the last place is at most M 2^-23, so the same 1.57 units
are 3e-6 M / 16: logp, lse and the loss of that row are held to their bounds times max(1, M / 16).
Measured on an MI355X (V = 48 / 1003 / 1024 / 10001): logp 5.7e-7 / 1.05e-6 / 9.3e-7 / 1.54e-6, lse 3.6e-7 / 5.7e-7 / 4.6e-7 / 5.8e-7,
loss 5.2e-7 / 1.0e-6 / 8.9e-7 / 1.44e-6 on the N(0, 2) rows; the scaled row at most 0.26 of its logp bound, 0.11 of its lse bound,
0.15 of its loss bound; sum_x at most 0.036 of its bound; logp bit-identical to the sibling on the three shapes with ld = V."""
import numpy as np
import pytest

import att_score_ref as R
from reverb_amd import _lib
from reverb_amd._lib import dptr, fptr, iptr

pytestmark = pytest.mark.gpu
COUNTS = [1, 3, 0, 70, 2, 1, 1, 5, 2]
SMOOTHING = 0.1
SCALED = 7


def _case(V, ld):
    rng = np.random.default_rng(800 + V)
    nrow = len(COUNTS)
    x = (rng.standard_normal((nrow, V)) * 2).astype(np.float32)
    x[1, 0] = x[1].max() + 1.0
    x[4, V - 1] = x[4].max() + 1.0
    x[6, V // 3] = x[6, V - 2] = x[6].max() + 1.0
    x[SCALED] *= 20.0
    ptr = np.concatenate([[0], np.cumsum(COUNTS)]).astype(np.int32)
    tgt = rng.integers(0, V, int(ptr[-1])).astype(np.int32)
    tgt[ptr[1]] = 0; tgt[ptr[4]] = V - 1; tgt[ptr[6]] = V - 2       # the planted maxima are asked for, the losing duplicate too
    padded = np.full((nrow, ld), 1e30, np.float32)                  # the pad columns must not be read: they would win every maximum
    padded[:, :V] = x
    return x, padded, ptr, tgt


@pytest.mark.parametrize("V,ld", [(48, 48), (1003, 1003), (1024, 1024), (10001, 10004)])
def test_row_xent_against_fp64_and_the_sibling(lib, V, ld):
    x, padded, ptr, tgt = _case(V, ld)
    nrow, P = len(COUNTS), int(ptr[-1])
    logp = np.full(P, np.nan, np.float32); lse = np.full(nrow, np.nan, np.float32)
    sum_x = np.full(nrow, np.nan, np.float64); top1 = np.full(nrow, -1, np.int32)
    _lib.check(lib.rvb_test_row_xent(fptr(padded), nrow, V, ld, iptr(ptr), iptr(tgt), fptr(logp), fptr(lse), dptr(sum_x), iptr(top1)),
               "rvb_test_row_xent")
    row_of = np.repeat(np.arange(nrow), COUNTS)
    x64 = x.astype(np.float64)
    ref_lp = R.log_softmax(x64)[row_of, tgt]
    ref_lse, ref_sum, ref_top = R.row_stats(x64)
    if ld == V:
        sib = np.full(P, np.nan, np.float32)
        _lib.check(lib.rvb_test_lse_gather_multi(fptr(x), nrow, V, iptr(ptr), iptr(tgt), P, fptr(sib)), "rvb_test_lse_gather_multi")
        assert np.array_equal(logp.view(np.uint32), sib.view(np.uint32)), "logp differs in bits from lse_gather_multi"
    assert np.array_equal(top1, ref_top), (top1, ref_top)
    assert top1[1] == 0 and top1[4] == V - 1 and top1[6] == V // 3
    # per-row scale of the fp32 bounds: 1 on the N(0, 2) rows, M / 16 on the scaled row (docstring)
    M = np.abs(ref_lse).copy()
    np.maximum.at(M, row_of, np.abs(ref_lp))
    scale = np.ones(nrow)
    scale[SCALED] = max(1.0, M[SCALED] / 16.0)
    assert np.all(M[np.arange(nrow) != SCALED] < 32.0), "the N(0, 2) rows must lie where the 3e-6 bound was derived"
    e_lp, e_lse = np.abs(logp - ref_lp) / scale[row_of], np.abs(lse - ref_lse) / scale
    e_sum = np.abs(sum_x - ref_sum) / (V * np.abs(x64).max(axis=1) * 2.0 ** -23)
    got_kl = R.compose(logp.astype(np.float64), lse.astype(np.float64)[row_of], sum_x[row_of], V, SMOOTHING)
    ref_kl = R.kl_dense(x64[row_of], tgt, SMOOTHING)
    e_kl = np.abs(got_kl - ref_kl) / scale[row_of]
    plain = row_of != SCALED
    print("V %d ld %d: logp %.3g lse %.3g loss %.3g (N(0,2) rows)  scaled row / its bound: logp %.3g lse %.3g loss %.3g  sum_x / bound %.3g"
          % (V, ld, e_lp[plain].max(), np.delete(e_lse, SCALED).max(), e_kl[plain].max(), e_lp[~plain].max() / 3e-6,
             e_lse[SCALED] / 3e-6, e_kl[~plain].max() / 5e-6, e_sum.max()))
    assert e_lp.max() <= 3e-6 and e_lse.max() <= 3e-6
    assert e_sum.max() <= 1.0
    assert e_kl.max() <= 5e-6
    # smoothing 0: the loss is -logp, whatever the other two statistics are
    assert np.array_equal(R.compose(logp.astype(np.float64), lse.astype(np.float64)[row_of], sum_x[row_of], V, 0.0),
                          -logp.astype(np.float64))
