"""The numpy references of tests/elementwise_ref.py against torch's float64 operators (a wrong reference is caught without a GPU),
and the argument checks the new hooks of csrc/test_api.h make before they look for a device."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import elementwise_ref as R
from reverb_amd import _lib
from util import f32, i32


def _t(a):
    return torch.from_numpy(np.asarray(a, np.float64))


@pytest.mark.parametrize("M,d", [(1, 8), (5, 64), (37, 640), (3, 1280)])
@pytest.mark.parametrize("mode,silu,use_add,two", [(0, 0, 0, 0), (0, 1, 0, 0), (1, 1, 0, 0), (1, 0, 1, 0), (0, 0, 1, 1), (0, 0, 0, 1), (0, 1, 0, 1)])
def test_rownorm_reference_against_torch(M, d, mode, silu, use_add, two):
    rng = np.random.default_rng(M * 1000 + d)
    x = rng.uniform(-5, 5, (M, 1)) + rng.uniform(0.5, 4, (M, 1)) * rng.standard_normal((M, d))
    g, b, g2, b2 = (rng.uniform(0.5, 1.5, d), rng.standard_normal(d), rng.uniform(0.5, 1.5, d), rng.standard_normal(d))
    add = rng.standard_normal((M, d)) if use_add else None
    out, out2 = R.rownorm(x, g, b, 1e-5, mode, bool(silu), add, g2 if two else None, b2 if two else None, 1e-3)
    want = F.layer_norm(_t(x), (d,), _t(g), _t(b), 1e-5) if mode == 0 else _t(x) * _t(g) + _t(b)
    if silu:
        want = F.silu(want)
    if use_add:
        want = want + _t(add)
    np.testing.assert_allclose(out, want.numpy(), rtol=1e-12, atol=1e-12)
    if two:
        np.testing.assert_allclose(out2, F.layer_norm(want, (d,), _t(g2), _t(b2), 1e-3).numpy(), rtol=1e-12, atol=1e-12)
    else:
        assert out2 is None
    # the float32 emulation is the same function at another precision
    e1, _ = R.rownorm(f32(x), g, b, 1e-5, mode, bool(silu), add, dt=np.float32)
    assert e1.dtype == np.float32
    np.testing.assert_allclose(e1, R.rownorm(f32(x), g, b, 1e-5, mode, bool(silu), add)[0], rtol=1e-4, atol=1e-4)


_DW_SHAPES = [(15, 8, 1, 0, 0), (31, 6, 17, 0, 0), (3, 10, 40, 0, 0), (1, 4, 9, 0, 0), (31, 8, 3, 1, 0), (8, 6, 20, 1, 0), (15, 4, 12, 1, 9),
              (2, 4, 5, 1, 1)]


# the gated form has no streaming history
@pytest.mark.parametrize("gated,K,d,T,causal,hist_rows", [(g,) + s for s in _DW_SHAPES for g in (False, True) if not (g and s[4])])
def test_glu_dwconv_reference_against_torch(gated, K, d, T, causal, hist_rows):
    rng = np.random.default_rng(K * 100 + T)
    B = 1 if hist_rows else 3
    lens = i32([T] if hist_rows else [T, max(T - 9, 0), min(5, T)])
    G2 = rng.standard_normal((B, T, 2 * d))
    hist = rng.standard_normal((K - 1, 2 * d))
    pb, w, b = rng.standard_normal(2 * d), rng.standard_normal((d, K)), rng.standard_normal(d)
    # torch, the way the module computes it: masked frames carry the pointwise bias, the left context too unless it is cached
    Gd = _t(G2).clone()
    for bi in range(B):
        Gd[bi, int(lens[bi]):] = _t(pb)
    if causal:
        left = _t(pb).repeat(B, K - 1, 1)
        if hist_rows:
            left[0, K - 1 - hist_rows:] = _t(hist)[K - 1 - hist_rows:]
        Gd = torch.cat([left, Gd], 1)
    glu = F.glu(Gd.transpose(1, 2), dim=1)
    want = F.conv1d(glu, _t(w).unsqueeze(1), _t(b), padding=0 if causal else (K - 1) // 2, groups=d).transpose(1, 2).numpy()
    Gin = F.glu(_t(G2), dim=2).numpy() if gated else G2
    got = R.glu_dwconv(Gin, pb, w, b, lens, K, bool(causal), gated, hist if hist_rows else None, hist_rows)
    assert got.shape == (B, T, d)
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12)
    frames, filled = R.glu_frames(Gin, pb, lens, K, bool(causal), gated, hist if hist_rows else None, hist_rows)
    np.testing.assert_allclose(frames, glu.transpose(1, 2).numpy(), rtol=1e-12, atol=1e-12)
    lead = K - 1 if causal else 0
    assert filled.shape == frames.shape[:2]
    for bi in range(B):
        assert filled[bi, :lead - hist_rows].all() and not filled[bi, lead - hist_rows:lead + int(lens[bi])].any()
        assert filled[bi, lead + int(lens[bi]):].all()


@pytest.mark.parametrize("B,T0,F0,d", [(2, 39, 80, 8), (1, 41, 23, 24), (3, 3, 3, 8), (1, 4, 80, 16)])
def test_conv1_reference_against_torch(B, T0, F0, d):
    rng = np.random.default_rng(T0 + d)
    feats = rng.standard_normal((B, T0, F0)) * 4 + 15
    mean, istd = 15 + rng.standard_normal(F0), 0.25 + 0.05 * rng.random(F0)
    w, b = rng.standard_normal((d, 1, 3, 3)), rng.standard_normal(d)
    want = torch.relu(F.conv2d(((_t(feats) - _t(mean)) * _t(istd)).unsqueeze(1), _t(w), _t(b), stride=2)).permute(0, 2, 3, 1).numpy()
    got = R.conv1(feats, mean, istd, w, b)
    assert got.shape == want.shape
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12)


def test_clip_scale_sits_in_the_widest_gap():
    ref = np.array([[-10.0, 9.0, 8.9, -4.0], [3.9, 0.0, 3.0, -8.8]])
    scale, count, ratio = R.clip_scale(ref)
    assert count == 4 and abs(ratio - 2.2) < 1e-12                       # the gap 8.8 -> 4.0
    assert abs(448 * float(scale) - np.sqrt(8.8 * 4.0)) < 1e-5
    scale, count, ratio = R.clip_scale(ref, top=3)                       # only 10, 9, 8.9 are looked at: the gap 10 -> 9
    assert count == 1 and abs(ratio - 10 / 9) < 1e-12


def test_new_hooks_refuse_bad_arguments_before_any_device_work(lib):
    """The hooks of tests/test_elementwise_kernels_gpu.py check indices and sizes (E_ARG = -1) before they look for a device, so these
    hold with and without a GPU; outputs keep their sentinel."""
    f, ip = _lib.fptr, _lib.iptr
    z = np.zeros(64, np.float32)
    out = np.full(64, -77.0, np.float32)
    tok, pos = i32([0, 4]), i32([1, 0])
    assert lib.rvb_test_embed(f(z), 4, f(z), 2, ip(tok), ip(pos), f(out), 2, 8, 1.0) == -1            # token 4 of a table of 4
    assert lib.rvb_test_embed(f(z), 8, f(z), 1, ip(tok), ip(pos), f(out), 2, 8, 1.0) == -1            # position 1 of a table of 1
    assert lib.rvb_test_gather_pairs(f(z), 4, 16, ip(i32([3])), ip(i32([16])), 1, f(out)) == -1       # column 16 of 16
    assert lib.rvb_test_gather_pairs(f(z), 4, 16, ip(i32([4])), ip(i32([0])), 1, f(out)) == -1        # row 4 of 4
    src, dst = np.zeros(64, np.uint8), np.full(64, 0xA5, np.uint8)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert lib.rvb_test_gather_cache(vp(src), vp(dst), ip(i32([0, 2])), 2, 2, 1, 16) == -1            # parent 2 of 2 hypotheses
    assert lib.rvb_test_gather_cache(vp(src), vp(dst), ip(i32([0, 1])), 2, 2, 3, 16) == -1            # 3 rows of a cache of 2
    assert lib.rvb_test_amax_abs(0, f(z), 0, f(out)) == -1
    assert lib.rvb_test_convert_f32(2, f(z), f(out), 4) == -1
    assert lib.rvb_test_conv1_ex(0, f(z), f(z), f(z), f(z), f(z), f(out), 1, 2, 8, 8, 0.0, None, None) == -1   # two frames: no output row
    a = _lib.NormTestArgs()
    a.dtype, a.M, a.d, a.out_fp8 = 1, 2, 8, 1
    a.x = a.gamma = a.beta = f(z)
    a.out = f(out)
    assert lib.rvb_test_rownorm_ex(ctypes.byref(a)) == -1                                             # fp8 output without a scale
    a.out_fp8, a.gamma2 = 0, f(z)
    assert lib.rvb_test_rownorm_ex(ctypes.byref(a)) == -1                                             # gamma2 without beta2 / out2
    assert lib.rvb_test_rownorm_ex(None) == -1
    assert np.all(out == -77.0) and np.all(dst == 0xA5)
