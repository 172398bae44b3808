"""csrc/gemm.hip and csrc/gemm2.hip in the forms the engines launch, through rvb_test_gemm_ex (any GemmArgs a run_gemm builds): the
fp32 residual in the output buffer itself, logits rows padded to 16 bytes with N % 4 != 0, A offset into its allocation,
overlapping rows (lda < K), a null bias, LeakyReLU, M down to 1 and the cut between the two kernel families, a long K with
alpha = sqrt(d).  Two kinds of assertion, as in tests/test_attention_kernels_gpu.py:

(a) every output element against fp64 on the rounded operands, within gemm_ref.bound: a bound that follows from the formats, and
    that tests/test_gemm_ref.py shows (without a GPU) to hold for an emulation of the kernels and to notice seven broken ones;
(b) bit-identity where the arithmetic per element is the same: in place against out of place, A at an offset against A at the
    start, padded rows against packed ones, variant switches that must not change the kernel.

Outputs start as NaN: a column past N or a row past M that is not NaN afterwards was written.  Every test asserts which kernel
family ran (`path` of the hook against gemm2_applicable's conditions).  The worst err / bound of every call is recorded with
tests/test_diar_gpu.py's _record (test = "gemm_forms"), as the attention tests record theirs."""
import ctypes

import numpy as np
import pytest

import gemm_ref as G
from gemm_ref import BF16, F32
from reverb_amd import _lib
from reverb_amd._lib import fptr

pytestmark = pytest.mark.gpu
E_HIP = -2


def _record(**kw):
    from test_diar_gpu import _record as rec
    rec(test="gemm_forms", **kw)


def _ids(cases):
    return [G.case_id(c) for c in cases]


def _call(lib, case, inplace=None, c_rows=0, expect_rc=0, **override):
    """one rvb_test_gemm_ex call -> (C [rows][ldc], path, (a_deq, w_deq)).  Out of place C goes up NaN-filled; in place it goes up
    as the residual (pad columns and rows past M NaN)."""
    inplace = case["inplace"] if inplace is None else inplace
    M, N, K, ldc = case["M"], case["N"], case["K"], case["ldc"]
    rows = c_rows or M
    a = _lib.GemmTestArgs()
    a.dtype, a.M, a.N, a.K, a.lda, a.ldw, a.ldc, a.ldres = case["dtype"], M, N, K, case["lda"], case["ldw"], ldc, case["ldres"]
    a.act, a.alpha, a.a_row0, a.c_rows = case["act"], case["alpha"], case["a_row0"], c_rows
    a.out_f32, a.out_fp8, a.in_fp8 = int(case["out"] == "f32"), int(case["out"] == "fp8"), int(case["in_fp8"])
    a.a_scale, a.out_scale = case["a_scale"], case["out_scale"]
    A = case["A_raw"] if case["in_fp8"] else case["A"]
    W = case["W_raw"] if case["in_fp8"] else case["W"]
    a.a_elems = A.size
    C = np.full((rows, ldc), np.nan, np.float32)
    res = None
    if inplace:
        C[:M] = case["res"]
        a.inplace = 1
    elif case["res"] is not None:
        res = np.ascontiguousarray(case["res"])
    deq = (np.empty_like(A), np.empty_like(W)) if case["in_fp8"] else (None, None)
    a.A, a.W, a.bias, a.res, a.C, a.a_deq, a.w_deq = fptr(A), fptr(W), fptr(case["bias"]), fptr(res), fptr(C), fptr(deq[0]), fptr(deq[1])
    for k, v in override.items():
        setattr(a, k, v)
    rc = lib.rvb_test_gemm_ex(ctypes.byref(a))
    if rc == E_HIP:               # a HIP error (a fault included) ends the session: nothing more is started on that device
        pytest.exit("rvb_test_gemm_ex: HIP error on %s: %r" % (G.case_id(case), lib.rvb_last_error()), returncode=3)
    if expect_rc == 0:
        _lib.check(rc, "rvb_test_gemm_ex")
    assert rc == expect_rc, (rc, lib.rvb_last_error())
    return C, a.path, deq


def _within(case, C, what, **rec):
    """columns < N of rows < M inside the bound, every other element still NaN -> worst err / bound (recorded)"""
    M, N = case["M"], case["N"]
    assert np.isnan(C[:M, N:]).all(), "%s: a pad column was written" % what
    assert np.isnan(C[M:]).all(), "%s: a row past M was written" % what
    ref, bnd = G.reference(case), G.bound(case)
    got = C[:M, :N].astype(np.float64)
    assert not np.isnan(got).any(), "%s: %d elements never stored" % (what, int(np.isnan(got).sum()))
    err = np.abs(got - ref)
    r = float((err / bnd).max()) if err.size else 0.0
    print("%s: worst err / bound %.3f" % (what, r))
    _record(form=case["form"], case=G.case_id(case), ratio=r, **rec)
    bad = err > bnd
    assert not bad.any(), "%s: %d elements outside the bound, worst err / bound %.3g (err %.3g)" % (what, int(bad.sum()), r, float(err[bad].max()))
    return r


def _same_bits(X, Y, what):
    X, Y = np.ascontiguousarray(X, np.float32), np.ascontiguousarray(Y, np.float32)
    diff = X.view(np.uint32) != Y.view(np.uint32)
    assert not diff.any(), "%s: %d elements differ, first at %s" % (what, int(diff.sum()), tuple(np.argwhere(diff)[0]))


class _Switches:
    """gemm2 flags / kernel variant for the calls inside, defaults restored whatever happens"""

    def __init__(self, lib, flags=None, variant=0):
        self.lib, self.flags, self.variant = lib, flags, variant

    def __enter__(self):
        if self.flags is not None:
            self.lib.rvb_test_set_gemm2_opts(self.flags, -2)
        self.lib.rvb_test_set_gemm_variant(self.variant)

    def __exit__(self, *exc):
        self.lib.rvb_test_set_gemm2_opts(-1, -1)
        self.lib.rvb_test_set_gemm_variant(0)


# ------------------------------------------------------------------------------------------------------------ in-place residual
INPLACE = [(c, fl) for c in G.inplace_cases() for fl in ((0, 32, 1024, 8192) if c["dtype"] == BF16 else (None,))]


@pytest.mark.parametrize("case,flags", INPLACE, ids=["%s-flags%s" % (G.case_id(c), fl) for c, fl in INPLACE])
def test_residual_in_the_output_buffer(lib, case, flags):
    """run_gemm(..., x, d, M, true, alpha, ACT_NONE, x, d): att_out, pw2, ff2, ffm2, self_out, src_out.  The residual is read by the
    accumulator preload (flags 32), the prefetched ring of the generic epilogue (flags 1024, and every ragged tile) or the ring of
    the epilogue with inline-asm stores (full tiles, flags 0 and 8192 = the same on 32x32x16 MFMAs); M = 40 runs gemm.hip, and so does
    every f32 call.  N = 262 in packed rows takes the element-wise epilogue, in rows of 264 the ragged segment of the vector one.
    Within the bound, pad columns untouched, and bit for bit what the same call gives with the residual in a buffer of its own.
    Worst err / bound seen on an MI355X: 0.013 under flags 0, 1024 and 8192, 0.032 under flags 32 (the preload rounds res / alpha
    into the accumulator, which the bound's S does not count) and 0.032 on f32; no case differed in place."""
    with _Switches(lib, flags):
        C, path, _ = _call(lib, case)
        assert path == G.expected_path(case)
        sep, path2, _ = _call(lib, case, inplace=False, ldres=case["ldc"])
        assert path2 == path
    _within(case, C, G.case_id(case), flags=flags, path=path)
    _same_bits(C[:, :case["N"]], sep[:, :case["N"]], "in place vs out of place")
    assert np.isnan(sep[:, case["N"]:]).all()


def test_residual_in_the_output_buffer_fp8(lib):
    """the same through the fp8 kernel (e4m3 operands, fp32 out, alpha 0.5: the feed-forward's second GEMM in RVB_FP8 mode), against
    fp64 on the values the quantised operands stand for, with the bound tests/test_fp8_gpu.py states for that kernel (seen: 0.060
    of it)"""
    case = G.fp8_inplace_case()
    C, path, (ad, wd) = _call(lib, case)
    assert path == 2
    deq = dict(case, A=ad, W=wd)
    assert np.abs(ad - case["A_raw"]).max() <= np.abs(case["A_raw"]).max() / 16 + 1e-6          # the operands are e4m3 at the stated scales
    assert np.abs(wd - case["W_raw"]).max() <= np.abs(case["W_raw"]).max() / 16 + 1e-6
    np.testing.assert_array_equal(ad, case["A"])          # ... and the host quantisation is the one gemm_ref emulates
    _within(deq, C, G.case_id(case), path=path)
    sep, _, _ = _call(lib, case, inplace=False, ldres=case["ldc"])
    _same_bits(C, sep, "fp8: in place vs out of place")


# ------------------------------------------------------------------------------------------------------------ padded logits rows
LOGITS = G.logits_cases()


@pytest.mark.parametrize("case", LOGITS, ids=_ids(LOGITS))
def test_padded_logits_rows_from_an_offset_into_the_encoder_output(lib, case):
    """The CTC / decoder output GEMMs: fp32 to ldc = (V + 3) & ~3 with N = V, A = enc_out + r0 * d.  bf16: gemm2's vector epilogue
    with a ragged last segment (N = 1001 .. 1003), a whole one (1000), two pad segments (ldc 1008); f32: gemm.hip.  Columns >= N and
    three rows past M stay NaN; columns < N are bit for bit what the call with A at the start of its allocation gives.  Worst
    err / bound seen: bf16 0.007, f32 0.017."""
    M, N = case["M"], case["N"]
    C, path, _ = _call(lib, case, c_rows=M + 3)
    assert path == G.expected_path(case) == (2 if case["dtype"] == BF16 else 1)
    _within(case, C, G.case_id(case), path=path)
    start = dict(case, A=np.ascontiguousarray(case["A"][case["a_row0"] * case["lda"]:]), a_row0=0)
    C0, _, _ = _call(lib, start)
    _same_bits(C[:M, :N], C0[:, :N], "a_row0 = 37 vs 0")


# ------------------------------------------------------------------------------------------------------------ vec_ok / res_acc
COND = [(c, fl) for c in G.condition_cases() for fl in ((0, 32) if c["dtype"] == BF16 else (None,))]      # gemm2's switches do not reach f32


@pytest.mark.parametrize("case,flags", COND, ids=["%s-flags%s" % (G.case_id(c), fl) for c, fl in COND])
def test_conditions_the_vector_epilogue_declares(lib, case, flags):
    """One case per false branch of vec_ok / res_acc in gemm2.hip: bf16 rows of N + 2 elements (no 16-byte rows: element-wise
    stores), a residual with ldres = N + 1 (no 16-byte residual vectors: element-wise, and no accumulator preload under flags 32),
    and ldc = N + 8 with everything aligned, which must be the packed call bit for bit.  The f32 engine runs the same calls on
    gemm.hip.  Worst err / bound seen: 0.986 with bf16 output (the half ulp of the output rounding is most of that bound), at most
    0.007 (bf16) and 0.016 (f32) with fp32 output."""
    with _Switches(lib, flags):
        C, path, _ = _call(lib, case)
        assert path == G.expected_path(case)
        _within(case, C, G.case_id(case), flags=flags, path=path)
        if case["form"] == "cond_padded":
            P, _, _ = _call(lib, dict(case, ldc=case["N"]))
            _same_bits(C[:, :case["N"]], P, "ldc = N + 8 vs packed")


# ------------------------------------------------------------------------------------------------------------ overlapping rows
OVERLAP = [(c, v) for c in G.overlap_cases() for v in ((0, 1) if c["dtype"] == BF16 and c["lda"] == 64 else (0,))]


@pytest.mark.parametrize("case,variant", OVERLAP, ids=["%s-variant%d" % (G.case_id(c), v) for c, v in OVERLAP])
def test_overlapping_rows_of_the_sincnet_convolutions(lib, case, variant):
    """SincNet conv layers 2 / 3 as a GEMM over the [frames][cin] activation: lda = cin, K = 5 cin, N = 64, with and without a bias.
    cin = 80 (K = 400, no multiple of 64) runs gemm.hip on both engines; cin = 64 (K = 320) is gemm2_applicable on bf16 and runs the
    LDS-DMA loop, whose per-lane row offsets then step by lda < K; variant 1 sends the same call to gemm.hip.  The reference is
    Conv1d in fp64 (tests/test_gemm_ref.py).  Worst err / bound seen: 0.946 with bf16 output on all three paths, 0.005 on f32."""
    want = 2 if (case["dtype"] == BF16 and case["lda"] == 64 and variant == 0) else 1
    if case["dtype"] == BF16 and case["lda"] == 64:
        assert G.gemm2_applicable(case) and case["K"] % 64 == 0 and case["lda"] % 8 == 0 and case["M"] >= 128 and case["N"] >= 64
    else:
        assert G.expected_path(case) == 1
    with _Switches(lib, variant=variant):
        C, path, _ = _call(lib, case)
    assert path == want == G.expected_path(case, variant)
    _within(case, C, G.case_id(case), variant=variant, path=path)


# ------------------------------------------------------------------------------------------------------------ LeakyReLU, null bias
LRELU = G.lrelu_cases()


@pytest.mark.parametrize("case", LRELU, ids=_ids(LRELU))
def test_leaky_relu_without_bias_stays_on_the_small_kernel(lib, case):
    """The diarization network's linear layers: a null bias and ACT_LRELU, which gemm2 refuses, so that even variant 2 ("gemm2
    whenever applicable") must run gemm.hip and give the same bits.  Symmetric operands: about half the outputs are negative.
    Worst err / bound seen: 0.952 (bf16 output), 0.006 (f32)."""
    neg = float((G.reference(case) < 0).mean())
    assert 0.4 < neg < 0.6, neg
    with _Switches(lib, variant=0):
        C, path, _ = _call(lib, case)
    with _Switches(lib, variant=2):
        C2, path2, _ = _call(lib, case)
    assert path == path2 == 1 and not G.gemm2_applicable(case)
    _within(case, C, G.case_id(case), path=path)
    _same_bits(C, C2, "variant 0 vs variant 2")


# ------------------------------------------------------------------------------------------------------------ small M, the cut
CUT = G.cut_cases()


@pytest.mark.parametrize("case", CUT, ids=_ids(CUT))
def test_small_m_and_the_cut_between_the_kernels(lib, case):
    """The decoder's M = R rows, down to 1, and both sides of gemm2_applicable's M >= 128 and N >= 64 (bf16: gemm.hip below, gemm2
    from there on; f32: gemm.hip throughout), with SiLU and alpha = 0.5 in front of bf16 and fp32 outputs.  Three rows past M stay
    NaN.  Worst err / bound seen: 0.984 with bf16 output, 0.005 (bf16 operands) and 0.014 (f32) with fp32 output."""
    C, path, _ = _call(lib, case, c_rows=case["M"] + 3)
    assert path == G.expected_path(case) == (2 if case["dtype"] == BF16 and case["M"] >= 128 and case["N"] >= 64 else 1)
    _within(case, C, G.case_id(case), path=path)


@pytest.mark.parametrize("dtype,out", [(BF16, "bf16"), (BF16, "f32"), (F32, "f32")])
def test_rows_agree_across_the_cut(lib, dtype, out):
    """the first 127 rows of the M = 129 problem (gemm2 on bf16) against the M = 127 problem on the same operands (gemm.hip): two
    kernels, so not the same bits, but each within its bound of the same reference -- they agree within the sum of the bounds
    (seen: 0.002 of it with fp32 output; the bf16 outputs and the f32 engine's came out equal)"""
    big = G.make("cut", dtype, 129, 192, 128, 650, act=G.ACT_SILU, alpha=0.5, out=out)
    small = dict(big, M=127, A=np.ascontiguousarray(big["A"][:127 * 128]))
    Cb, pb, _ = _call(lib, big)
    Cs, ps, _ = _call(lib, small)
    assert (pb, ps) == ((2, 1) if dtype == BF16 else (1, 1))
    np.testing.assert_array_equal(G.reference(big)[:127], G.reference(small))
    tol = G.bound(big)[:127] + G.bound(small)
    d = np.abs(Cb[:127].astype(np.float64) - Cs)
    _record(form="cut_agree", case=G.case_id(big), ratio=float((d / tol).max()))
    assert (d <= tol).all(), float((d / tol).max())


# ------------------------------------------------------------------------------------------------------------ long K
LONG = G.long_k_cases()


@pytest.mark.parametrize("case", LONG, ids=_ids(LONG))
def test_long_odd_k_with_alpha(lib, case):
    """embed_out: K = F2 * d, here 19 K steps of 64 (bf16, gemm2) / 38 of 32 (f32), alpha = 8, fp32 out.  Worst err / bound seen:
    0.001 (bf16), 0.002 (f32)."""
    C, path, _ = _call(lib, case)
    assert path == G.expected_path(case)
    _within(case, C, G.case_id(case), path=path)


# ------------------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("dtype", [BF16, F32])
def test_refusals(lib, dtype):
    """gemm() itself: M = 0 is done before it starts (OK, C untouched: four canary rows); K, lda or ldw that are no multiple of the
    16-byte vector are E_ARG in gemm()'s words; ACT_GLU with a residual is E_UNSUPPORTED.  A refused call leaves C as it was."""
    ve = 8 if dtype == BF16 else 4
    base = G.make("refusal", dtype, 16, 64, 64, 900, res=True)
    C, _, _ = _call(lib, dict(base, M=0, res=None, ldres=0), c_rows=4)
    assert C.shape == (4, 64) and np.isnan(C).all()
    big = dict(base, A=np.concatenate([base["A"], base["A"]]))          # room for any stride below
    for kw in (dict(K=64 - ve // 2), dict(lda=64 + ve // 2), dict(ldw=64 + ve // 2, W=np.ascontiguousarray(np.pad(base["W"], ((0, 0), (0, ve // 2)))))):
        C, _, _ = _call(lib, dict(big, **kw), expect_rc=G.E_ARG)
        assert b"gemm: K, lda, ldw" in lib.rvb_last_error(), (kw, lib.rvb_last_error())
        assert np.isnan(C).all()
    glu = G.make("refusal", dtype, 256, 128, 64, 901, act=G.ACT_GLU, res=True, out="bf16")
    C, _, _ = _call(lib, glu, expect_rc=G.E_UNSUPPORTED)
    assert b"ACT_GLU" in lib.rvb_last_error() and np.isnan(C).all()
