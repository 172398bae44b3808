"""Every form of the row-norm, GLU + depthwise-convolution, conv1 and small elementwise kernels (csrc/elementwise.hip, gather_pairs of
csrc/softmax_topk.hip) against the fp64 references of tests/elementwise_ref.py, each through the launcher the engine calls
(csrc/test_api.h).  Every row of an input has its own mean and scale and every per-channel vector is random and asymmetric, so a
row or column mix-up cannot pass; outputs start as NaN.  Tolerances are the project's own, named at each assert."""
import ctypes
import math

import numpy as np
import pytest

import elementwise_ref as R
from reverb_amd import _lib
from reverb_amd._lib import fptr, iptr
from test_kernels_gpu import _assert_glu_dwconv
from util import bf16_round, rnd, f32, i32

pytestmark = pytest.mark.gpu
F32, BF16 = 0, 1
E_ARG = -1


# ------------------------------------------------------------------------------------------------ rownorm
def _rows(rng, M, d):
    """[M][d] with a mean (+-5) and a scale (0.5 .. 4) of its own per row."""
    return f32(rng.uniform(-5, 5, (M, 1)) + rng.uniform(0.5, 4, (M, 1)) * rng.standard_normal((M, d)))


def _affine(rng, d):
    return f32(rng.uniform(0.5, 1.5, d) * rng.choice([-1.0, 1.0], d, p=[0.2, 0.8])), f32(0.5 * rng.standard_normal(d))


def _norm_call(lib, dtype, x, g, b, mode=0, silu=0, add=None, out_kind="f32", scale=1.0, x_bf16=0, g2=None, b2=None, out2_fp8=0,
               scale2=1.0, eps=1e-5, eps2=1e-3):
    """One rvb_test_rownorm_ex call -> (rc, out, out2, sat, sat2); out / out2 NaN-filled on the way in."""
    M, d = x.shape
    out = np.full((M, d), np.nan, np.float32)
    out2 = np.full((M, d), np.nan, np.float32) if g2 is not None else None
    a = _lib.NormTestArgs()
    a.dtype, a.x_bf16, a.mode, a.silu, a.M, a.d = dtype, x_bf16, mode, silu, M, d
    a.out_f32, a.out_fp8, a.out2_fp8 = int(out_kind == "f32"), int(out_kind == "fp8"), out2_fp8
    a.eps, a.eps2, a.out_scale, a.out2_scale = eps, eps2, scale, scale2
    a.x, a.gamma, a.beta, a.add, a.gamma2, a.beta2, a.out, a.out2 = fptr(x), fptr(g), fptr(b), fptr(add), fptr(g2), fptr(b2), fptr(out), fptr(out2)
    rc = lib.rvb_test_rownorm_ex(ctypes.byref(a))
    return rc, out, out2, a.sat, a.sat2


def _assert_kind(got, ref, kind, scale=None, what=""):
    assert np.isfinite(got).all(), what
    if kind == "f32":
        print(f"{what}: max |error| of the fp32 output {np.abs(got - ref).max():.3g}")
        np.testing.assert_allclose(got, ref, rtol=1e-5, atol=4e-5, err_msg=what)       # fp32 output: test_rownorm / test_layernorm_to_fp8
    elif kind == "bf16":
        np.testing.assert_allclose(got, ref, rtol=1e-2, atol=1e-2, err_msg=what)       # one bf16 rounding: test_rownorm
    else:
        np.testing.assert_allclose(got, ref, rtol=0.07, atol=float(scale) * 2.0 ** -9 * 1.01, err_msg=what)   # one e4m3 rounding: test_layernorm_to_fp8


def _fp8_scale(ref):
    return np.float32(np.abs(ref).max() * 2 / 448)          # as test_layernorm_to_fp8: nothing clips


# (TWO, SW) as launch_rownorm lists them: SW bit 0 bf16 input, 1 LayerNorm, 2 SiLU, 3 add, 4 fp8 second output
_NINE = [(False, 2), (False, 2 | 4 | 1), (False, 4 | 1), (False, 2 | 4), (False, 4), (True, 2), (True, 2 | 8), (True, 2 | 16), (True, 2 | 8 | 16)]
# ... and at 512 < d <= 1024 the combinations that fall through to the generic NV = 4 kernel: affine without SiLU, LN + add without a
# second stage, bf16 input with LN and no SiLU, a second stage behind SiLU
_GENERIC4 = [(False, 0), (False, 2 | 8), (False, 2 | 1), (True, 2 | 4)]


def _norm_forms(d, combos):
    for two, sw in combos:
        if not (sw & (1 | 16)):
            yield (F32, d, two, sw, "f32")
        for kind in (("f32",) if two else ("bf16", "f32", "fp8")):
            yield (BF16, d, two, sw, kind)


_FORMS = [f for d in (640, 1024, 256, 1280) for f in _norm_forms(d, _NINE)] + list(_norm_forms(640, _GENERIC4))
_NORM_SEEN = {}


def _norm_case(lib, dtype, M, d, two, sw, kind, seed=0):
    """One form on fresh inputs against fp64; returns what the bit-identity check needs."""
    rng = np.random.default_rng(seed + d * 7 + sw)
    x = _rows(rng, M, d)
    if sw & 1:
        x = bf16_round(x)
    g, b = _affine(rng, d)
    g2, b2 = _affine(rng, d) if two else (None, None)
    add = rnd(dtype, rng.standard_normal((M, d)) * 2) if sw & 8 else None
    mode, silu, o2f8 = (0 if sw & 2 else 1), int(bool(sw & 4)), int(bool(sw & 16))
    ref, ref2 = R.rownorm(x, g, b, 1e-5, mode, bool(silu), add, g2, b2, 1e-3)
    scale = _fp8_scale(ref) if kind == "fp8" else 1.0
    scale2 = _fp8_scale(ref2) if o2f8 else 1.0
    what = f"dtype {dtype} M {M} d {d} TWO {two} SW {sw} out {kind}"
    rc, out, out2, sat, sat2 = _norm_call(lib, dtype, x, g, b, mode, silu, add, kind, scale, sw & 1, g2, b2, o2f8, scale2)
    assert rc == 0, what
    _assert_kind(out, ref, kind, scale, what)
    assert (sat, sat2) == (0, 0), what
    if two:
        _assert_kind(out2, ref2, "fp8" if o2f8 else ("f32" if dtype == F32 else "bf16"), scale2, what + " (out2)")
        if dtype == F32:
            # the second stage reads "exactly what a separate pass would read": the first output is that of the one-stage call
            rc, one, _, _, _ = _norm_call(lib, dtype, x, g, b, mode, silu, add, kind, scale, sw & 1)
            assert rc == 0 and np.array_equal(out, one), what
    return out


@pytest.mark.parametrize("dtype,d,two,sw,kind", _FORMS)
def test_rownorm_every_instantiation(lib, dtype, d, two, sw, kind):
    """The nine compile-time (TWO, SW) forms at d = 640 and 1024, the same switches on the generic NV = 2 (d = 256) and NV = 8
    (d = 1280) kernels, and the four combinations that fall through to the generic NV = 4 kernel at d = 640; in every engine and
    output type rownorm() accepts for them.  fp32 outputs at d = 1280 are held to the project's fp32 bound like the others: the float32
    emulation (elementwise_ref.rownorm with dt = float32) errs by at most 1.0e-6 in the first and 1.6e-6 in the second stage on
    these inputs at d = 1024, 1280 and 2048 alike, far inside rtol 1e-5 + atol 4e-5, so the longer sums give no reason to widen it.
    (The bit-identity check of the f32 engine found: at 512 < d <= 1024 the compiler contracted the variance's squares to FMAs in the
    generic kernel and not in the compile-time forms, so the fused LN + add -> LN pair and the one-stage LN + add differed in the last
    bit of rstd; sq4() in elementwise.hip now writes the roundings out.)"""
    _norm_case(lib, dtype, 37, d, two, sw, kind)


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("d", [8, 504, 512, 520, 1024, 1032, 2048])
def test_rownorm_column_edges(lib, dtype, d):
    """The first and the last d of every NV, LN + add, fp32 output."""
    _norm_case(lib, dtype, 37, d, False, 2 | 8, "f32", seed=1)


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("d", [12, 2056])
def test_rownorm_refuses_other_widths(lib, dtype, d):
    rng = np.random.default_rng(d)
    x = _rows(rng, 5, d)
    g, b = _affine(rng, d)
    rc, out, _, _, _ = _norm_call(lib, dtype, x, g, b)
    assert rc == E_ARG and np.isnan(out).all()


@pytest.mark.parametrize("dtype,M,d,two,sw,kind", [
    (F32, 1, 64, False, 2, "f32"), (BF16, 1, 640, True, 2, "f32"),
    (F32, 3, 640, True, 2 | 8, "f32"), (BF16, 3, 64, False, 2 | 4 | 1, "bf16"),        # a workgroup whose last wave has no row
    (F32, 5, 64, True, 2, "f32"), (BF16, 5, 640, False, 2, "fp8"),
    (F32, 16387, 640, False, 2, "f32"),              # waves own two or three rows: the compile-time LN form
    (BF16, 16387, 640, True, 2, "f32"),              # ... the TWO form
    (BF16, 16387, 640, False, 2 | 4 | 1, "bf16"),    # ... bf16 input + SiLU
    (F32, 16387, 64, False, 2 | 8, "f32"),           # ... the generic NV = 2 kernel
    (BF16, 16387, 64, True, 2 | 16, "f32"),
    (F32, 8195, 1280, False, 2, "f32"),              # NV = 8: waves 0 .. 2 own a second row
    (BF16, 8195, 1280, True, 2 | 8, "f32"),
])
def test_rownorm_row_edges_and_the_row_pipeline(lib, dtype, M, d, two, sw, kind):
    """The launcher starts min(ceil(M / 4), 2048) workgroups of 4 waves: only from M = 8193 on does a wave prefetch a real second row
    (load_row(row + nwaves, nx) ... v = nx).  Every row is checked."""
    _norm_case(lib, dtype, M, d, two, sw, kind, seed=M)


@pytest.mark.parametrize("d", [1024, 256])
@pytest.mark.parametrize("stage", [1, 2])
def test_rownorm_saturation_counts(lib, stage, d):
    """sat / sat2 count exactly the values beyond +-448 * scale, and those come back as +-448 * scale.  The scale sits in the middle of
    the widest gap among the 200 largest |reference| values, so fp32 error (1e-5) cannot move a value across it."""
    M = 37
    rng = np.random.default_rng(d + stage)
    x = _rows(rng, M, d)
    g, b = _affine(rng, d)
    g2, b2 = _affine(rng, d)
    ref1, ref2 = R.rownorm(x, g, b, 1e-5, gamma2=g2, beta2=b2, eps2=1e-3)
    ref = ref1 if stage == 1 else ref2
    scale, want, ratio = R.clip_scale(ref)
    print(f"d {d} stage {stage}: widest gap ratio {ratio:.5f}, {want} values above 448 * {float(scale):.6g}")
    assert ratio >= 1.001 and 0 < want < 200, ratio          # a condition on the inputs

    def run(s):
        if stage == 1:
            rc, out, _, sat, sat2 = _norm_call(lib, BF16, x, g, b, out_kind="fp8", scale=s)
            return rc, out, sat, sat2
        rc, o1, out, sat, sat2 = _norm_call(lib, BF16, x, g, b, out_kind="f32", g2=g2, b2=b2, out2_fp8=1, scale2=s)
        _assert_kind(o1, ref1, "f32")
        return rc, out, sat2, sat
    rc, out, sat, other = run(scale)
    assert rc == 0 and other == 0
    clipped = np.abs(ref) > 448.0 * float(scale)
    assert sat == want == int(clipped.sum())
    assert np.array_equal(out[clipped], (np.sign(ref[clipped]) * (np.float32(448.0) * scale)).astype(np.float32))
    _assert_kind(out[~clipped], ref[~clipped], "fp8", scale)
    rc, out, sat, other = run(_fp8_scale(ref))
    assert rc == 0 and (sat, other) == (0, 0)
    _assert_kind(out, ref, "fp8", _fp8_scale(ref))


# ------------------------------------------------------------------------------------------------ glu_dwconv
def _dw_inputs(rng, dtype, B, T, d, K, gated):
    G = rnd(dtype, rng.standard_normal((B, T, d if gated else 2 * d)) * rng.uniform(0.5, 2, d if gated else 2 * d))
    pb = f32(rng.standard_normal(2 * d))
    w = f32(rng.standard_normal((d, K)) / math.sqrt(K))
    b = f32(rng.standard_normal(d))
    return G, pb, w, b


def _dw_call(lib, dtype, G, pb, w, b, lens, K, word, hist=None, hist_rows=0):
    B, T = G.shape[:2]
    d = w.shape[0]
    out = np.full((B, T, d), np.nan, np.float32)
    rc = lib.rvb_test_glu_dwconv(dtype, fptr(G), fptr(pb), fptr(w), fptr(b), iptr(lens), fptr(out), B, T, d, K, word, fptr(hist), hist_rows)
    return rc, out


_GATED_SHAPES = [(15, 8, 1, None), (31, 128, 127, None), (31, 128, 128, None), (31, 136, 129, None), (3, 200, 300, None), (1, 264, 70, None),
                 (31, 64, 3, None), (15, 72, 40, [40, 0, 5])]


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("causal", [0, 1])
@pytest.mark.parametrize("K,d,T,lens", _GATED_SHAPES)
def test_glu_dwconv_gated_form(lib, dtype, causal, K, d, T, lens):
    """GluDwArgs::gated (what the bf16 engine runs by default): G is [B][T][d], gated by the pointwise GEMM's epilogue -- the row
    stride d, the unread second half and the pass-through of the value, against fp64; one tile, a tile and a row, two channel tiles,
    d no multiple of the tile, a window wider than the sequence, an empty sequence."""
    B = 3
    rng = np.random.default_rng(K * 1000 + d + T)
    lens = i32(lens if lens is not None else [T, max(T - 9, 1), min(5, T)])
    G, pb, w, b = _dw_inputs(rng, dtype, B, T, d, K, True)
    ref = R.glu_dwconv(G, pb, w, b, lens, K, bool(causal), True)
    rc, out = _dw_call(lib, dtype, G, pb, w, b, lens, K, causal | 4)
    assert rc == 0 and np.isfinite(out).all()
    if dtype == F32:
        np.testing.assert_allclose(out, ref, rtol=2e-5, atol=1e-4)          # fp32 depthwise convolution: _assert_glu_dwconv
    else:
        # a gated bf16 value goes to LDS as it is; the only bf16 rounding left is that of the bias-GLU value in padded and
        # left-context frames: _assert_glu_dwconv's bound (2^-8 per tap, 1 % slack, 1e-4 of fp32 noise) restricted to those taps
        frames, filled = R.glu_frames(G, pb, lens, K, bool(causal), True)
        bound = R.dwconv(np.abs(frames) * filled[..., None], np.abs(w), None, K, bool(causal)) * 2.0 ** -8
        err = np.abs(out - ref)
        assert np.all(err <= 1.01 * bound + 1e-4), float((err - 1.01 * bound).max())
    # bf16 output = the fp32 output rounded once (test_bf16_engine_dwconv_output_and_norm_input asserts it for the ungated form)
    rc, o16 = _dw_call(lib, dtype, G, pb, w, b, lens, K, causal | 4 | 2)
    assert rc == 0
    np.testing.assert_array_equal(o16, bf16_round(out))


def test_glu_dwconv_gated_form_refusals(lib):
    rng = np.random.default_rng(0)
    for dtype, d, causal, hist_rows in ((BF16, 16, 1, 3), (F32, 16, 1, 3), (BF16, 12, 0, 0), (BF16, 20, 1, 0), (F32, 6, 0, 0), (F32, 10, 1, 0)):
        G, pb, w, b = _dw_inputs(rng, dtype, 1, 9, d, 7, True)
        hist = rnd(dtype, rng.standard_normal((6, 2 * d))) if hist_rows else None
        rc, out = _dw_call(lib, dtype, G, pb, w, b, i32([9]), 7, causal | 4, hist, hist_rows)
        assert rc == E_ARG and np.isnan(out).all(), (dtype, d)
        assert b"gated" in lib.rvb_last_error()


def _ungated_case(lib, dtype, B, K, d, T, causal, hist_rows, seed):
    import torch
    rng = np.random.default_rng(seed)
    lens = i32([T] if B == 1 else [T, max(T - 9, 1), min(5, T)])
    G, pb, w, b = _dw_inputs(rng, dtype, B, T, d, K, False)
    hist = rnd(dtype, rng.standard_normal((K - 1, 2 * d))) if hist_rows else None
    frames, _ = R.glu_frames(G, pb, lens, K, bool(causal), False, hist, hist_rows)
    ref = R.dwconv(frames, w, b, K, bool(causal))
    rc, out = _dw_call(lib, dtype, G, pb, w, b, lens, K, causal, hist, hist_rows)
    assert rc == 0 and np.isfinite(out).all()
    # the existing bound of test_glu_dwconv: fp32 rtol 2e-5 / atol 1e-4; bf16 one rounding of the gated value per tap
    _assert_glu_dwconv(out, ref, torch.from_numpy(frames).transpose(1, 2), w, dtype, 0 if causal else (K - 1) // 2)


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("d", [6, 130, 202])
@pytest.mark.parametrize("K,T", [(15, 70), (31, 130)])
def test_glu_dwconv_scalar_staging_path(lib, dtype, d, K, T):
    """d % (16 / sizeof(T)) != 0: rows are no whole 16-byte vectors and the staging loop loads element by element -- no model shape
    takes it, so no other test does."""
    _ungated_case(lib, dtype, 3, K, d, T, 0, 0, d + K)


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_glu_dwconv_scalar_staging_path_with_history(lib, dtype):
    _ungated_case(lib, dtype, 1, 15, 130, 70, 1, 9, 5)


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("T", [3, 17])
def test_glu_dwconv_window_wider_than_the_sequence(lib, dtype, T):
    _ungated_case(lib, dtype, 3, 31, 64, T, 0, 0, T)


# ------------------------------------------------------------------------------------------------ conv1
def _conv1_inputs(B, T0, d, seed):
    F0 = 80
    rng = np.random.default_rng(seed)
    feats = f32(rng.standard_normal((B, T0, F0)) * 4 + 15 + rng.uniform(-3, 3, (B, T0, 1)))
    mean = f32(15 + rng.standard_normal(F0)); istd = f32(0.25 + 0.05 * rng.random(F0))
    w = f32(rng.standard_normal((d, 1, 3, 3)) / 3 * rng.uniform(0.5, 2, (d, 1, 1, 1))); b = f32(rng.standard_normal(d))
    return feats, mean, istd, w, b


def _conv1_call(lib, dtype, ins, scale=0.0, amax=None, want_sat=False):
    feats, mean, istd, w, b = ins
    B, T0, F0 = feats.shape
    d = w.shape[0]
    out = np.full((B, (T0 - 3) // 2 + 1, (F0 - 3) // 2 + 1, d), np.nan, np.float32)
    slot = f32([amax]) if amax is not None else None
    sat = ctypes.c_uint32(0)
    rc = lib.rvb_test_conv1_ex(dtype, fptr(feats), fptr(mean), fptr(istd), fptr(w), fptr(b), fptr(out), B, T0, F0, d, scale, fptr(slot),
                               ctypes.byref(sat) if want_sat else None)
    return rc, out, (slot[0] if slot is not None else None), sat.value


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("d", [32, 640, 2048])
@pytest.mark.parametrize("T0", [39, 41])
def test_conv1_running_amax(lib, dtype, d, T0):
    """The running maximum the calibration of the conv2 fp8 scale rests on.  T1 = 19 / 20: the last workgroup has 3 / 4 rows.  At
    d = 640 (80 channel groups, 3 f1 slots) lanes 48-63 of the last wave leave the kernel before the wave reduction, which compiles to
    ds_bpermute_b32; the maximum must be right there as well, i.e. the shuffle must read nothing but zero from the lanes that have
    exited (every value is >= 0, so a zero is neutral and a stale register is not)."""
    ins = _conv1_inputs(2, T0, d, d + T0)
    ref = R.conv1(*ins)
    want = ref.max()
    rc, out, amax, _ = _conv1_call(lib, dtype, ins, amax=0.0)
    assert rc == 0 and np.isfinite(out).all()
    tol = 2e-5 if dtype == F32 else 1e-2                                     # test_conv1_cmvn
    np.testing.assert_allclose(out, ref, rtol=tol, atol=tol * 4)
    print(f"dtype {dtype} d {d} T0 {T0}: amax {amax!r} reference {want!r}")
    assert amax > 0 and abs(float(amax) - want) <= 2e-5 * want              # the maximum of the fp32 values, before any bf16 rounding
    preset = np.float32(2 * want)
    rc, _, kept, _ = _conv1_call(lib, dtype, ins, amax=preset)
    assert rc == 0 and kept.tobytes() == preset.tobytes()                    # a running maximum: a larger one stays, bit for bit


@pytest.mark.parametrize("d", [128, 640])
def test_conv1_fp8_output_and_saturation_count(lib, d):
    ins = _conv1_inputs(2, 39, d, d)
    ref = R.conv1(*ins)
    scale = _fp8_scale(ref)
    rc, out, _, sat = _conv1_call(lib, BF16, ins, scale=scale, want_sat=True)
    assert rc == 0 and sat == 0
    _assert_kind(out, ref, "fp8", scale)
    scale, want, ratio = R.clip_scale(ref)
    print(f"d {d}: widest gap ratio {ratio:.5f}, {want} values above 448 * {float(scale):.6g}")
    assert ratio >= 1.001 and 0 < want < 200, ratio                          # a condition on the inputs
    rc, out, _, sat = _conv1_call(lib, BF16, ins, scale=scale, want_sat=True)
    clipped = ref > 448.0 * float(scale)
    assert rc == 0 and sat == want == int(clipped.sum())
    assert np.all(out[clipped] == np.float32(448.0) * scale)
    _assert_kind(out[~clipped], ref[~clipped], "fp8", scale)
    rc, out, _, _ = _conv1_call(lib, F32, ins, scale=scale)                  # fp8 output belongs to the bf16 engine
    assert rc == E_ARG and np.isnan(out).all()


# ------------------------------------------------------------------------------------------------ small kernels
@pytest.mark.parametrize("d", [8, 256, 1000])
def test_embed_tokens(lib, d):
    rows, vocab, n_pos = 37, 50, 64
    rng = np.random.default_rng(d)
    E = f32(rng.standard_normal((vocab, d)) * rng.uniform(0.5, 2, (vocab, 1))); pe = f32(rng.standard_normal((n_pos, d)))
    tok = i32(rng.integers(0, vocab, rows)); pos = i32(rng.permutation(n_pos)[:rows])
    tok[5] = tok[20] = tok[0]; pos[7] = pos[3]; tok[-1] = vocab - 1; pos[-1] = n_pos - 1      # repeated, out of order, the last rows
    scale = np.float32(math.sqrt(d))
    out = np.full((rows, d), np.nan, np.float32)
    _lib.check(lib.rvb_test_embed(fptr(E), vocab, fptr(pe), n_pos, iptr(tok), iptr(pos), fptr(out), rows, d, scale))
    e, p = E[tok].astype(np.float64) * float(scale), pe[pos].astype(np.float64)
    # one fp32 rounding of each term; contracted to an FMA or not, the result is within it
    assert np.all(np.abs(out - (e + p)) <= 2.0 ** -23 * (np.abs(e) + np.abs(p)))


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("n", [1, 255, 257, 600001])
def test_amax_abs(lib, dtype, n):
    """n = 600001 is more than 2048 blocks x 256 threads: the grid-stride loop."""
    rng = np.random.default_rng(n)
    x = rnd(dtype, rng.standard_normal(n))
    x[-1] = -7.5 if n > 1 else -0.3125                      # the largest magnitude: negative, in the last element
    assert np.abs(x[:-1]).max(initial=0) < 7.5

    def run(v, slot):
        s = f32([slot])
        _lib.check(lib.rvb_test_amax_abs(dtype, fptr(v), v.size, fptr(s)))
        return s[0]
    assert run(x, 0.0) == abs(x[-1])
    assert run(x, 1e-30) == abs(x[-1])
    assert run(x, 16.25) == np.float32(16.25)               # a larger slot stays
    assert run(np.zeros(n, np.float32), 1e-30) == np.float32(1e-30) and run(np.zeros(n, np.float32), 0.0) == 0.0     # nothing to fold


def _convert_values(n, seed):
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    nan = (bits & 0x7f800000 == 0x7f800000) & (bits & 0x007fffff != 0)
    bits[nan] &= 0xff800000                                  # NaN payloads -> infinities
    special = np.array([0x3f808000, 0x3f818000, 0x3f808001, 0x3f807fff,      # ties (to even: down, up), just above / below a tie
                        0x00000001, 0x00008000, 0x00018000, 0x807fffff,      # denormals (a tie among them)
                        0x7f800000, 0xff800000, 0x3fffffff, 0x7f7fffff,      # +-inf, up into the next binade, up into infinity
                        0x00000000, 0x80000000, 0x3f800000, 0xc0490fdb], np.uint32)
    k = min(n, special.size)
    bits[:k] = special[:k]
    return bits.view(np.float32)


@pytest.mark.parametrize("n", [1, 257, 1100003])
def test_convert_f32(lib, n):
    """bf16: round to nearest even, bit for bit util.bf16_round (more than 4096 x 256 elements: the grid-stride loop); f32: a copy."""
    x = _convert_values(n, n)
    for dtype in (BF16, F32):
        out = np.full(n, np.nan, np.float32)
        _lib.check(lib.rvb_test_convert_f32(dtype, fptr(x), fptr(out), n))
        want = bf16_round(x) if dtype == BF16 else x
        assert np.array_equal(out.view(np.uint32), want.view(np.uint32)), dtype


@pytest.mark.parametrize("rows", [1, 4, 7])
@pytest.mark.parametrize("row_bytes", [16, 256, 1280])
def test_gather_cache(lib, rows, row_bytes):
    R_, L = 5, 7
    rng = np.random.default_rng(rows + row_bytes)
    src = rng.integers(0, 256, (R_, L, row_bytes), dtype=np.uint8)
    dst = np.full((R_, L, row_bytes), 0xA5, np.uint8)
    parent = i32([3, 3, 0, 4, 1])
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    _lib.check(lib.rvb_test_gather_cache(vp(src), vp(dst), iptr(parent), R_, L, rows, row_bytes))
    assert np.array_equal(dst[:, :rows], src[parent][:, :rows])
    assert np.all(dst[:, rows:] == 0xA5)


def test_gather_cache_refuses_rows_that_are_no_whole_vectors(lib):
    src = np.zeros((5, 7, 24), np.uint8); dst = np.full((5, 7, 24), 0xA5, np.uint8)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert lib.rvb_test_gather_cache(vp(src), vp(dst), iptr(i32([3, 3, 0, 4, 1])), 5, 7, 4, 24) == E_ARG
    assert np.all(dst == 0xA5)


@pytest.fixture(scope="module")
def pair_table():
    return f32(np.random.default_rng(11).standard_normal((37, 10001)))


@pytest.mark.parametrize("n", [1, 256, 257, 5000])
def test_gather_pairs(lib, pair_table, n):
    rows, V = pair_table.shape
    rng = np.random.default_rng(n)
    row, col = i32(rng.integers(0, rows, n)), i32(rng.integers(0, V, n))
    row[-1], col[-1] = rows - 1, V - 1                       # the last row and the last column
    if n > 2:
        row[1], col[1] = row[0], col[0]                      # a duplicate
        row[2], col[2] = 0, V - 1
    out = np.full(n, np.nan, np.float32)
    _lib.check(lib.rvb_test_gather_pairs(fptr(pair_table), rows, V, iptr(row), iptr(col), n, fptr(out)))
    assert np.array_equal(out, pair_table[row, col])


def test_gather_pairs_of_nothing(lib, pair_table):
    out = np.full(4, -77.0, np.float32)
    _lib.check(lib.rvb_test_gather_pairs(fptr(pair_table), 37, 10001, None, None, 0, fptr(out)))
    assert np.all(out == -77.0)
