"""row_lse_kernel (csrc/softmax_topk.hip) behind logsoftmax_topk, lse_gather and lse_gather_multi, in the forms the engine runs, through
the strided lab hooks rvb_test_logsoftmax_topk_ex / rvb_test_lse_gather_ex / rvb_test_lse_gather_multi_ex.

Shapes (V, ld), one failure mode each: (10001, 10004) the engine's form (16-byte vectors over V >> 2, a one-element scalar tail, pad
columns never read); (1025, 1028) one full batch then a one-element tail; (1027, 1028) a three-element tail; (1024, 1024) exactly one
batch; (2052, 2052) a partial second batch; (1003, 1003) the scalar path alone; (1000, 1024) wide padding; (65, 68) and (64, 64)
k = 64 with every lane maximum used; (48, 48) most lanes empty; (5, 8) k = V.  k = 1, 10, 64 where k <= V, and k = V on the small
shapes.  The 16 rows of a case go through in launches of 9, 4, 1 and 2 rows: a ragged last block, exactly one block, fewer rows than a
block.  Everything runs with the pad columns filled with 1e30 and again with NaN, and must give the same bits.

Rows (ROW_*; a row a shape is too small for is a plain N(0, 2) row): a maximum at index 0 and at V - 1; an exact tie across the
vector / tail boundary; an all-equal row (the exclusion-scan fallback); a 300-way tie at the top; exactly 256 and exactly 257 elements
equal to the maximum, in all 64 lanes (the last row pass C handles and the first that falls back); the top 12 values inside one lane's
slice (the lane-maxima threshold lies far below the true k-th value); -inf everywhere but three entries; the first 1024 entries -inf
(add_batch's early return, then a first finite batch); a row scaled by 20; a narrow row whose two largest values sit at 0 and V - 1,
the blank ids of the penalty runs, and must drop out of the top k when penalised by 2.5.

References.  Top-k is exact: the kernel orders the (penalised) fp32 logits by value descending, index ascending, which is
np.argsort(-x, kind="stable"); every row is compared with array_equal, ties included.  logp / tv: fp64 log_softmax of the fp32 logits
(after the fp32 subtraction of the penalty), held to the bound tests/test_row_xent_gpu.py derives, 3e-6 max(1, M / 16) with
M = max(|lse|, max |logp|) of the row (the unscaled rows are checked to stay below 32); -inf is compared for equality.
Bit-identities: tv = logp[row, ti]; tv / ti with logp null and non-null; lse_gather (with and without penalty, a target equal to the
blank included) and lse_gather_multi = logp of logsoftmax_topk gathered; at (10001, 10004) row_xent's logp = lse_gather_multi's.

Measured on an MI355X:
(V, ld): logsoftmax_topk logp / tv error on the unscaled rows, fraction of its bound the scaled row uses | the same for lse_gather and
lse_gather_multi.  All k, both penalties and blank ids, both pad fills:
  (10001, 10004): 1.92e-06, 0.226 | 1.92e-06, 0.226
  (1025, 1028): 1.92e-06, 0.156 | 1.2e-06, 0.156
  (1027, 1028): 1.43e-06, 0.271 | 1.01e-06, 0.0743
  (1024, 1024): 1.35e-06, 0.232 | 9.45e-07, 0.232
  (2052, 2052): 1.65e-06, 0.139 | 1.1e-06, 0.139
  (1003, 1003): 1.52e-06, 0.316 | 1.45e-06, 0.124
  (1000, 1024): 1.82e-06, 0.156 | 9.87e-07, 0.086
  (65, 68): 8.65e-07, 0.31 | 6.8e-07, 0.114
  (64, 64): 8.19e-07, 0.293 | 6.02e-07, 0.109
  (48, 48): 8.24e-07, 0.294 | 7.58e-07, 0.235
  (5, 8): 4.31e-07, 0.247 | 4.31e-07, 0.247
Every bit-identity held on every shape, the engine's form (10001 in rows of 10004; k = 1, 10, 64; no penalty, penalty 2.5 on blank 0
and on blank 10000) included; no index differed from the exact order on any row.
"""
import functools

import numpy as np
import pytest

import att_score_ref as R
from reverb_amd import _lib
from reverb_amd._lib import dptr, fptr, iptr

SHAPES = [(10001, 10004), (1025, 1028), (1027, 1028), (1024, 1024), (2052, 2052), (1003, 1003), (1000, 1024), (65, 68), (64, 64), (48, 48),
          (5, 8)]
(ROW_PLAIN, ROW_MAX0, ROW_MAXLAST, ROW_TIE_BOUNDARY, ROW_ALL_EQUAL, ROW_TIE300, ROW_TIE256, ROW_TIE257, ROW_ONE_LANE, ROW_INF3,
 ROW_INF1024, ROW_SCALED, ROW_BLANKS_ON_TOP, ROW_PLAIN2, ROW_PLAIN3, ROW_PLAIN4) = range(16)
NROW = 16
SLICES = [(0, 9), (9, 13), (13, 14), (14, 16)]             # launches of 9, 4, 1 and 2 rows
COUNTS = [1, 3, 0, 70, 2, 1, 1, 5, 2, 2, 0, 1, 4, 3, 0, 2]  # targets per row of lse_gather_multi: none, more than lanes
PEN = 2.5
LANE = 37
BOUND = 3e-6


def _tail0(V, ld):
    return (V >> 2) * 4 if ld % 4 == 0 else 0


def _lane(i, V, ld):
    t0 = _tail0(V, ld)
    return (i // 4) % 64 if i < t0 else (i - t0) % 64


@functools.lru_cache(maxsize=None)
def _case(V, ld):
    rng = np.random.default_rng(4100 + V)
    x = (rng.standard_normal((NROW, V)) * 2).astype(np.float32)
    t0 = _tail0(V, ld)
    x[ROW_MAX0, 0] = x[ROW_MAX0].max() + 1.0
    x[ROW_MAXLAST, V - 1] = x[ROW_MAXLAST].max() + 1.0
    a, b = (t0 - 1, t0) if 0 < t0 < V else (V // 3, V - 2)
    x[ROW_TIE_BOUNDARY, a] = x[ROW_TIE_BOUNDARY, b] = x[ROW_TIE_BOUNDARY].max() + 1.0
    x[ROW_ALL_EQUAL] = 0.25
    x[ROW_TIE300] = 0.5
    x[ROW_TIE300, (V - 300 if V >= 600 else V // 2):] = 0.75
    planted = {"tie": (a, b)}
    if V >= 258:
        idx = np.arange(256) * ((V - 1) // 257)
        assert {_lane(int(i), V, ld) for i in idx} == set(range(64)) and idx[-1] < V - 1
        x[ROW_TIE256, idx] = x[ROW_TIE256].max() + 1.0
        x[ROW_TIE257, np.append(idx, V - 1)] = x[ROW_TIE257].max() + 1.0
        planted["tie256"] = idx
    if V >= 1000:
        if t0:
            idx = np.array([(64 * u + LANE) * 4 + c for u in range(3) for c in range(4)])
        else:
            idx = LANE + 64 * np.arange(12)
        assert idx.max() < max(t0, V if not t0 else 0) and {_lane(int(i), V, ld) for i in idx} == {LANE}
        x[ROW_ONE_LANE, idx] = x[ROW_ONE_LANE].max() + 1.0 + rng.permutation(12).astype(np.float32) / 16
        planted["one_lane"] = idx
    x[ROW_INF3] = -np.inf
    x[ROW_INF3, [1, V // 2, V - 1]] = [0.5, -1.0, 0.5]
    if V > 1024:
        x[ROW_INF1024, :1024] = -np.inf
    x[ROW_SCALED] *= 20.0
    x[ROW_BLANKS_ON_TOP] *= 0.15
    top = x[ROW_BLANKS_ON_TOP, 1:V - 1].max()
    x[ROW_BLANKS_ON_TOP, 0] = top + 0.25
    x[ROW_BLANKS_ON_TOP, V - 1] = top + 0.125
    x.setflags(write=False)
    return x, planted


@functools.lru_cache(maxsize=None)
def _reference(V, ld, pen, blank):
    """-> (penalised fp32 logits, fp64 log-probs, fp64 lse, the exact order of every row); computed once per form, read-only"""
    x = _case(V, ld)[0].copy()
    if pen != 0.0:
        x[:, blank] = x[:, blank] - np.float32(pen)             # the fp32 subtraction RowReader makes
    x64 = x.astype(np.float64)
    with np.errstate(invalid="ignore"):
        lp = R.log_softmax(x64)
    lp[np.isneginf(x64)] = -np.inf
    lse = R.row_stats(np.where(np.isneginf(x64), -1e300, x64))[0]
    order = np.argsort(-x, axis=1, kind="stable")
    for a in (x, lp, lse, order):
        a.setflags(write=False)
    return x, lp, lse, order


def _padded(V, ld, fill):
    p = np.full((NROW, ld), fill, np.float32)
    p[:, :V] = _case(V, ld)[0]
    return p


def _topk(lib, padded, V, ld, k, pen, blank, with_logp=True):
    """logsoftmax_topk over the 16 rows in the launches of SLICES -> tv, ti, lp (None without logp); outputs NaN / -2 filled"""
    tv = np.full((NROW, k), np.nan, np.float32); ti = np.full((NROW, k), -2, np.int32)
    lp = np.full((NROW, V), np.nan, np.float32) if with_logp else None
    for r0, r1 in SLICES:
        rows = np.ascontiguousarray(padded[r0:r1])
        otv, oti = np.full((r1 - r0, k), np.nan, np.float32), np.full((r1 - r0, k), -2, np.int32)
        olp = np.full((r1 - r0, V), np.nan, np.float32) if with_logp else None
        _lib.check(lib.rvb_test_logsoftmax_topk_ex(fptr(rows), r1 - r0, V, ld, k, pen, blank, fptr(otv), iptr(oti), fptr(olp)),
                   "rvb_test_logsoftmax_topk_ex")
        tv[r0:r1], ti[r0:r1] = otv, oti
        if with_logp:
            lp[r0:r1] = olp
    return tv, ti, lp


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _row_scale(lp_ref, lse_ref):
    """M = max(|lse|, max finite |logp|) per row and the factor max(1, M / 16) of the bound, 1 on all but the scaled row"""
    M = np.maximum(np.abs(lse_ref), np.where(np.isfinite(lp_ref), np.abs(lp_ref), 0.0).max(axis=1))
    plain = np.arange(NROW) != ROW_SCALED
    assert np.all(M[plain] < 32.0), "the unscaled rows must lie where the 3e-6 bound was derived"
    scale = np.ones(NROW)
    scale[ROW_SCALED] = max(1.0, M[ROW_SCALED] / 16.0)
    return scale


def _err(got, ref, scale_rows):
    """|got - ref| / scale where ref is finite; -inf must match exactly"""
    inf = np.isneginf(ref)
    assert np.array_equal(np.isneginf(got), inf), "-inf entries differ"
    assert not np.isnan(got).any(), "an element was not written"
    with np.errstate(invalid="ignore"):
        return np.where(inf, 0.0, np.abs(got.astype(np.float64) - ref)) / scale_rows


def _ks(V):
    return [k for k in (1, 10, 64) if k <= V] + ([V] if V < 64 else [])


def _forms(V):
    return [(0.0, 0), (PEN, 0), (PEN, V - 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("V,ld", SHAPES)
def test_logsoftmax_topk_every_form(lib, V, ld):
    x, planted = _case(V, ld)
    pad_big, pad_nan = _padded(V, ld, 1e30), _padded(V, ld, np.nan)
    worst_plain, worst_scaled = 0.0, 0.0
    for pen, blank in _forms(V):
        xp, lp_ref, lse_ref, order = _reference(V, ld, pen, blank)
        scale = _row_scale(lp_ref, lse_ref)
        for k in _ks(V):
            tv, ti, lp = _topk(lib, pad_big, V, ld, k, pen, blank)
            what = "V %d ld %d k %d penalty %g blank %d" % (V, ld, k, pen, blank)
            for r in range(NROW):
                assert np.array_equal(ti[r], order[r, :k]), "%s row %d: %s != %s" % (what, r, ti[r][:12], order[r, :k][:12])
            rows = np.arange(NROW)[:, None]
            assert np.array_equal(_bits(tv), _bits(lp[rows, ti])), what + ": tv is not logp at ti"
            e_lp = _err(lp, lp_ref, scale[:, None])
            e_tv = _err(tv, lp_ref[rows, order[:, :k]], scale[:, None])
            plain = np.arange(NROW) != ROW_SCALED
            worst_plain = max(worst_plain, e_lp[plain].max(), e_tv[plain].max())
            worst_scaled = max(worst_scaled, e_lp[ROW_SCALED].max(), e_tv[ROW_SCALED].max())
            assert max(e_lp.max(), e_tv.max()) <= BOUND, what
            # the pad columns are never read: NaN there gives the same bits; and logp is optional
            tv2, ti2, lp2 = _topk(lib, pad_nan, V, ld, k, pen, blank)
            assert np.array_equal(ti2, ti) and np.array_equal(_bits(tv2), _bits(tv)) and np.array_equal(_bits(lp2), _bits(lp)), what
            tv3, ti3, _ = _topk(lib, pad_big, V, ld, k, pen, blank, with_logp=False)
            assert np.array_equal(ti3, ti) and np.array_equal(_bits(tv3), _bits(tv)), what + ": logp null changes the top-k"
            # what the planted rows are there for, by name
            if pen == 0.0:
                assert ti[ROW_MAX0, 0] == 0 and ti[ROW_MAXLAST, 0] == V - 1 and ti[ROW_TIE_BOUNDARY, 0] == planted["tie"][0]
                assert ti[ROW_ALL_EQUAL].tolist() == list(range(k))
                if k >= 2:
                    assert ti[ROW_TIE_BOUNDARY, 1] == planted["tie"][1]
                if "tie256" in planted:
                    assert ti[ROW_TIE256].tolist() == planted["tie256"][:k].tolist() == ti[ROW_TIE257].tolist()
                if "one_lane" in planted and k >= 10:
                    assert set(ti[ROW_ONE_LANE, :10].tolist()) <= set(planted["one_lane"].tolist())
                if k >= 10:
                    assert ti[ROW_INF3, :3].tolist() == [1, V - 1, V // 2] and np.all(np.isneginf(tv[ROW_INF3, 3:]))
                    rest = [i for i in range(V) if i not in (1, V // 2, V - 1)][:k - 3]
                    assert ti[ROW_INF3, 3:].tolist() == rest
                assert np.isfinite(lse_ref[ROW_INF3]) and np.all(np.isneginf(lp[ROW_INF3, 2:V // 2]))
            else:
                if V >= 1000:
                    assert blank not in ti[ROW_BLANKS_ON_TOP] and blank not in ti[ROW_MAX0 if blank == 0 else ROW_MAXLAST][:1]
                if k == V:
                    assert ti[ROW_ALL_EQUAL, -1] == blank and ti[ROW_BLANKS_ON_TOP, 0] == (V - 1 if blank == 0 else 0)
                elif blank == 0:
                    assert ti[ROW_ALL_EQUAL].tolist() == list(range(1, k + 1))
    print("logsoftmax_topk V %d ld %d: logp / tv error %.3g on the unscaled rows, the scaled row uses %.3g of its bound"
          % (V, ld, worst_plain, worst_scaled / BOUND))


@pytest.mark.gpu
@pytest.mark.parametrize("V,ld", SHAPES)
def test_lse_gather_and_multi_every_form(lib, V, ld):
    x, planted = _case(V, ld)
    rng = np.random.default_rng(77 + V)
    t0 = _tail0(V, ld)
    worst_plain, worst_scaled = 0.0, 0.0
    for fill in (1e30, np.nan):
        padded = _padded(V, ld, fill)
        for pen, blank in _forms(V):
            xp, lp_ref, lse_ref, _ = _reference(V, ld, pen, blank)
            scale = _row_scale(lp_ref, lse_ref)
            _, _, lp = _topk(lib, padded, V, ld, 1, pen, blank)
            tgt = rng.integers(0, V, NROW).astype(np.int32)
            tgt[[0, 1, 2, 3, 4, 5]] = [blank, 0, V - 1, planted["tie"][0], planted["tie"][1], V - 1 - blank]
            tgt[ROW_INF3], tgt[ROW_INF1024], tgt[ROW_BLANKS_ON_TOP] = V // 2, V - 1, blank
            got = np.full(NROW, np.nan, np.float32)
            for r0, r1 in SLICES:
                out = np.full(r1 - r0, np.nan, np.float32)
                _lib.check(lib.rvb_test_lse_gather_ex(fptr(np.ascontiguousarray(padded[r0:r1])), r1 - r0, V, ld,
                                                      iptr(np.ascontiguousarray(tgt[r0:r1])), pen, blank, fptr(out)), "rvb_test_lse_gather_ex")
                got[r0:r1] = out
            what = "V %d ld %d penalty %g blank %d pad %g" % (V, ld, pen, blank, fill)
            rows = np.arange(NROW)
            assert np.array_equal(_bits(got), _bits(lp[rows, tgt])), what + ": lse_gather differs in bits from logsoftmax_topk's logp"
            e = _err(got, lp_ref[rows, tgt], scale)
            assert e.max() <= BOUND, what
            worst_plain = max(worst_plain, np.delete(e, ROW_SCALED).max()); worst_scaled = max(worst_scaled, e[ROW_SCALED])
        # the CSR form (no penalty in the launcher)
        xp, lp_ref, lse_ref, _ = _reference(V, ld, 0.0, 0)
        scale = _row_scale(lp_ref, lse_ref)
        _, _, lp = _topk(lib, padded, V, ld, 1, 0.0, 0)
        ptr = np.concatenate([[0], np.cumsum(COUNTS)]).astype(np.int32)
        tgt = rng.integers(0, V, int(ptr[-1])).astype(np.int32)
        tgt[ptr[1]], tgt[ptr[3]], tgt[ptr[3] + 1], tgt[ptr[3] + 69] = 0, V - 1, max(t0 - 1, 0), min(t0, V - 1)
        row_of = np.repeat(np.arange(NROW), COUNTS)
        got = np.full(int(ptr[-1]), np.nan, np.float32)
        for r0, r1 in SLICES:
            sub_ptr = (ptr[r0:r1 + 1] - ptr[r0]).astype(np.int32)
            sub_tgt = np.ascontiguousarray(tgt[ptr[r0]:ptr[r1]])
            out = np.full(max(int(sub_ptr[-1]), 1), np.nan, np.float32)
            _lib.check(lib.rvb_test_lse_gather_multi_ex(fptr(np.ascontiguousarray(padded[r0:r1])), r1 - r0, V, ld, iptr(sub_ptr),
                                                        iptr(sub_tgt), fptr(out)), "rvb_test_lse_gather_multi_ex")
            got[ptr[r0]:ptr[r1]] = out[:int(sub_ptr[-1])]
        assert np.array_equal(_bits(got), _bits(lp[row_of, tgt])), "V %d ld %d: lse_gather_multi differs in bits from logp" % (V, ld)
        e = _err(got, lp_ref[row_of, tgt], scale[row_of])
        assert e.max() <= BOUND
        worst_plain = max(worst_plain, e[row_of != ROW_SCALED].max()); worst_scaled = max(worst_scaled, e[row_of == ROW_SCALED].max())
        if (V, ld) == (10001, 10004) and fill == 1e30:
            # row_xent on the same rows and targets: the gap tests/test_row_xent_gpu.py names (its sibling's hook had no stride)
            n = 9
            logp = np.full(int(ptr[n]), np.nan, np.float32); lse = np.full(n, np.nan, np.float32)
            sum_x = np.full(n, np.nan, np.float64); top1 = np.full(n, -1, np.int32)
            rows9 = np.ascontiguousarray(padded[:n])
            _lib.check(lib.rvb_test_row_xent(fptr(rows9), n, V, ld, iptr(np.ascontiguousarray(ptr[:n + 1])),
                                             iptr(np.ascontiguousarray(tgt[:ptr[n]])), fptr(logp), fptr(lse), dptr(sum_x), iptr(top1)),
                       "rvb_test_row_xent")
            assert np.array_equal(_bits(logp), _bits(got[:ptr[n]])), "row_xent's logp differs in bits from the strided lse_gather_multi"
    print("lse_gather / lse_gather_multi V %d ld %d: error %.3g on the unscaled rows, the scaled row uses %.3g of its bound"
          % (V, ld, worst_plain, worst_scaled / BOUND))


@pytest.mark.gpu
@pytest.mark.parametrize("V,ld", [(10001, 10004), (5, 8)])
def test_refusals_leave_the_outputs_as_filled(lib, V, ld):
    padded = np.ascontiguousarray(_padded(V, ld, 1e30)[:4])
    for k, v, l in [(0, V, ld), (65, V, ld), (V + 1 if V < 64 else 65, V, ld), (1, V, V - 1)]:
        n = max(k, 1)
        tv, ti, lp = np.full((4, n), 7.0, np.float32), np.full((4, n), 7, np.int32), np.full((4, V), 7.0, np.float32)
        assert lib.rvb_test_logsoftmax_topk_ex(fptr(padded), 4, v, l, k, 0.0, 0, fptr(tv), iptr(ti), fptr(lp)) == -1, (k, v, l)
        assert np.all(tv == 7.0) and np.all(ti == 7) and np.all(lp == 7.0)
    assert b"ld < V" in lib.rvb_last_error()
