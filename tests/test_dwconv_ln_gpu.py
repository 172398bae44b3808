"""dwconv_ln_kernel (csrc/elementwise.hip): the bf16 offline convolution module's depthwise conv + LayerNorm + SiLU in one
persistent kernel, against the two kernels it replaces (glu_dw_kernel, gated, bf16 output -> rownorm_kernel<bf16, bf16, 4, false, 7>),
bit for bit; against the fp64 references of tests/elementwise_ref.py; and inside the encoder through the lab switch RVB_DW_FUSE.

The shapes are the smallest at which the kernel can go wrong.  A workgroup owns a contiguous range of the [B * T] rows and walks it
16 rows at a time over a window of 15 + 16 + 15 input rows, so with B = 3 and T = 20 / 47 / 130 and 1, 2, 7 or B * T / 5 workgroups
the ranges begin and end in the middle of chunks, chunk boundaries fall inside a step's outputs and inside either halo, one window
holds a whole chunk and both of its paddings (T = 20 < K = 31), a step lies wholly inside one chunk (T = 130: the unmasked path), the
last step of a range is partial, and the ring of 64 LDS rows wraps (ranges longer than 18 rows)."""
import math

import numpy as np
import pytest

import elementwise_ref as R
from reverb_amd._lib import fptr, iptr
from util import bf16_round, f32, i32

pytestmark = pytest.mark.gpu
BF16 = 1
K, B, EPS = 31, 3, 1e-5


def _inputs(d, T, lens):
    rng = np.random.default_rng(d * 1000 + T * 10 + len(lens) + int(lens[0]))
    G = bf16_round(rng.standard_normal((B, T, d)) * rng.uniform(0.5, 2, d))          # gated already: [B][T][d]
    pb = f32(rng.standard_normal(2 * d))
    w = f32(rng.standard_normal((d, K)) / math.sqrt(K))
    b = f32(rng.standard_normal(d))
    g = f32(rng.uniform(0.5, 1.5, d) * rng.choice([-1.0, 1.0], d, p=[0.2, 0.8]))
    be = f32(0.5 * rng.standard_normal(d))
    return G, pb, w, b, i32(lens), g, be


def _call(lib, ins, grid, two=False):
    G, pb, w, b, lens, g, be = ins
    _, T, d = G.shape
    xn = np.full((B, T, d), np.nan, np.float32)
    xn2 = np.full((B, T, d), np.nan, np.float32) if two else None
    dc2 = np.full((B, T, d), np.nan, np.float32) if two else None
    rc = lib.rvb_test_dwconv_ln(fptr(G), fptr(pb), fptr(w), fptr(b), iptr(lens), fptr(g), fptr(be), EPS, fptr(xn), fptr(xn2), fptr(dc2),
                                B, T, d, K, grid)
    assert rc == 0, lib.rvb_last_error()
    return xn, xn2, dc2


def _lens_sets(T):
    return [[0, 1, T], [15, T - 1, T]]


_SHAPES = [(d, T, s) for d in (640, 1024) for T in (20, 47, 130) for s in (0, 1)]


@pytest.mark.parametrize("d,T,s", _SHAPES)
def test_same_bits_as_the_two_kernels(lib, d, T, s):
    """xn of the one kernel == xn of glu_dwconv + rownorm on the bits, for the launcher's own grid and for 1, 2, 7 and B * T / 5
    workgroups; lengths 0, 1, 15, T - 1 and T."""
    ins = _inputs(d, T, _lens_sets(T)[s])
    xn, two, _ = _call(lib, ins, 0, two=True)
    assert np.isfinite(two).all()
    for grid in (0, 1, 2, 7, B * T // 5):
        got = xn if grid == 0 else _call(lib, ins, grid)[0]
        assert np.isfinite(got).all(), (grid, int(np.isnan(got).sum()))
        diff = got.view(np.uint32) != two.view(np.uint32)
        assert not diff.any(), "grid %d: %d of %d values differ, first at (chunk, frame, channel) %s" % (
            grid, int(diff.sum()), diff.size, tuple(int(v) for v in np.argwhere(diff)[0]))


def test_more_workgroups_than_rows(lib):
    """Workgroups with an empty range leave; the others own one row each."""
    ins = _inputs(640, 20, [20, 3, 0])
    _, two, _ = _call(lib, ins, 0, two=True)
    got = _call(lib, ins, B * 20 + 9)[0]
    assert np.array_equal(got.view(np.uint32), two.view(np.uint32))


@pytest.mark.parametrize("d", [640, 1024])
def test_against_fp64(lib, d):
    """The chain against tests/elementwise_ref.py with the bounds tests/test_elementwise_kernels_gpu.py holds the two kernels to.  The
    one kernel keeps the depthwise output in LDS, so the chain is closed through the two-kernel run of the same entry point: its
    fp32 depthwise output within the gated form's bound (test_glu_dwconv_gated_form), the bf16 tensor between the kernels equal to
    that output rounded once, and the one kernel's xn within one bf16 rounding of LayerNorm + SiLU (fp64) of that tensor
    (_assert_kind "bf16": rtol 1e-2, atol 1e-2)."""
    T = 47
    lens = [T, 15, 0]
    ins = _inputs(d, T, lens)
    G, pb, w, b, lens, g, be = ins
    xn, _, dconv = _call(lib, ins, 7, two=True)
    out32 = np.full((B, T, d), np.nan, np.float32)
    assert lib.rvb_test_glu_dwconv(BF16, fptr(G), fptr(pb), fptr(w), fptr(b), iptr(lens), fptr(out32), B, T, d, K, 4, fptr(None), 0) == 0
    ref = R.glu_dwconv(G, pb, w, b, lens, K, False, True)
    frames, filled = R.glu_frames(G, pb, lens, K, False, True)
    bound = R.dwconv(np.abs(frames) * filled[..., None], np.abs(w), None, K, False) * 2.0 ** -8
    err = np.abs(out32 - ref)
    print("d %d: depthwise max |error| %.3g" % (d, err.max()))
    assert np.all(err <= 1.01 * bound + 1e-4), float((err - 1.01 * bound).max())
    np.testing.assert_array_equal(dconv, bf16_round(out32))
    want, _ = R.rownorm(dconv.reshape(B * T, d), g, be, EPS, R.NORM_LN, True)
    print("d %d: norm max |error| %.3g" % (d, np.abs(xn.reshape(B * T, d) - want).max()))
    np.testing.assert_allclose(xn.reshape(B * T, d), want, rtol=1e-2, atol=1e-2)


def test_refuses_what_the_predicate_refuses(lib):
    for d, k in ((512, 31), (1152, 31), (576, 31), (640, 30)):
        rng = np.random.default_rng(d)
        G = bf16_round(rng.standard_normal((B, 9, d)))
        xn = np.full((B, 9, d), np.nan, np.float32)
        z = f32(np.zeros(2 * d))
        w = f32(np.zeros((d, k)))
        rc = lib.rvb_test_dwconv_ln(fptr(G), fptr(z), fptr(w), fptr(z), iptr(i32([9, 9, 9])), fptr(z), fptr(z), EPS, fptr(xn), fptr(None),
                                    fptr(None), B, 9, d, k, 0)
        assert rc == -1 and np.isnan(xn).all(), (d, k)
        assert b"dwconv_ln" in lib.rvb_last_error()


# ------------------------------------------------------------------------------------------------ inside the encoder
def _tiny_model(d, causal=False):
    from reverb_amd import synth
    m = dict(d=d, h=8, ff=d, blocks=2, dff=64, dblocks=1, K=31, vocab=48)
    cfg = synth._make_config(m, "layer_norm")
    cfg["encoder_conf"]["causal"] = bool(causal)
    return cfg, synth.make_state_dict(cfg, 0)


def _encode(cfg, sd, flag, monkeypatch, slice0):
    from reverb_amd.engine import Engine
    chunk = 403                                            # 100 encoder frames per chunk: both slices have the 128 rows the GLU GEMM wants
    rng = np.random.default_rng(5)
    x = f32(rng.standard_normal((5, chunk, 80)))
    lens = i32([chunk, 150, chunk, 40, chunk])
    monkeypatch.setenv("RVB_DW_FUSE", flag)
    monkeypatch.setenv("RVB_SLICE0", str(slice0))
    eng = Engine(cfg, sd, dtype="bf16", device=0, max_chunks=8, chunk_frames=chunk)
    try:
        eng.reset_timings()
        eng.encode(x, lens, 4)
        return eng.encoder_out().copy(), int(eng.timing("rownorm")["launches"]), int(eng.timing("glu_dwconv")["launches"])
    finally:
        eng.close()


def test_encoder_output_is_the_same_with_and_without_the_fused_kernel(monkeypatch, lab):
    """A batch of five chunks encoded in two slices (3 + 2) by a two-block d = 640 model: the encoder output with RVB_DW_FUSE=1
    equals that with RVB_DW_FUSE=0 bit for bit, and the fused run launches one row norm fewer per block and slice."""
    cfg, sd = _tiny_model(640)
    e0, n0, c0 = _encode(cfg, sd, "0", monkeypatch, 3)
    e1, n1, c1 = _encode(cfg, sd, "1", monkeypatch, 3)
    assert np.isfinite(e0).all()
    assert np.array_equal(e0.view(np.uint32), e1.view(np.uint32))
    assert c0 == c1 == 2 * 2 and n0 - n1 == 2 * 2, (n0, n1, c0, c1)


@pytest.mark.parametrize("d,causal", [(512, False), (640, True)])
def test_shapes_the_predicate_refuses_still_encode(monkeypatch, lab, d, causal):
    """d = 512 and a causal convolution module run the two kernels whatever the switch says."""
    cfg, sd = _tiny_model(d, causal)
    e0, n0, _ = _encode(cfg, sd, "0", monkeypatch, 3)
    e1, n1, _ = _encode(cfg, sd, "1", monkeypatch, 3)
    assert np.isfinite(e1).all() and n0 == n1
    assert np.array_equal(e0.view(np.uint32), e1.view(np.uint32))
