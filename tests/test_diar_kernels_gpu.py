"""Kernel-level parity of the segmentation network's kernels (csrc/diar.hip) and the embedding's statistics pooling
(csrc/resnet.hip tstp_pool), each called through its rvb_test_* hook, against a plain fp64 numpy reference on the same
rounded operands.

Tolerances follow the rounding model of each kernel and are computed per element: an fp32 sum of K terms is off by at
most K u sum|terms| (u = 2^-24, one rounding per fused multiply-add), every bf16 rounding point adds half a bf16 ulp
(at most 2^-8 of the value: 8 significant bits), and where the reference cannot round at the kernel's points (the LSTM's
h_t, which feeds back) the bound is the one measured on an MI355X times a small factor, as noted next to it.  Every test names a subtle fault it catches."""
import ctypes

import numpy as np
import pytest
import torch

from reverb_amd import _lib
from reverb_amd._lib import fptr, iptr
from util import bf16_round, rnd, f32, i32
# the fp64 references and derived bounds live in tests/diar_stage_ref.py, shared with the bf16-storage restatement of the network
from diar_stage_ref import (U32, HB, LSTM_F32_MAX, LSTM_BF16_MAX, LSTM_BF16_MEAN, half_ulp as _half_ulp, check_within as _check_within,
                            pool_norm_ref as _pool_norm_ref, conv1d5_ref, lstm_ref as _lstm_ref, classifier_ref)

# ... and the TSTP reference in tests/emb_conv_ref.py, shared with the bf16 embedding network's stage checks
from emb_conv_ref import nearest_map as _nearest_map, tstp_ref as _tstp_ref

pytestmark = pytest.mark.gpu
F32, BF16 = 0, 1


# ------------------------------------------------------------------------------------ window_stats
@pytest.mark.parametrize("kind", ["speech", "silence", "dc"])
@pytest.mark.parametrize("length,step,first,nwin", [(160000, 16000, 2, 5), (4001, 1000, 3, 7), (4003, 996, 1, 4)])
def test_window_stats(lib, kind, length, step, first, nwin):
    """fp64 partial sums, one pass: mean rounded once to fp32, rstd = 1 / sqrt(var + eps) rounded once -> rtol 4u on both, plus
    an fp64 cancellation term (1e-13 of the second moment) that matters only for the 100-sigma DC offset.  Catches: the scalar
    tail of len = 4001 / 4003 dropped or counted twice (the mean moves by x / len = 2.5e-4 sigma), the window base taken as
    first * step without the block index, or a two-pass variance forgotten for the DC case (float one-pass loses all digits)."""
    rng = np.random.default_rng(length + first)
    n = (first + nwin - 1) * step + length + 17
    if kind == "silence":
        wave = np.zeros(n, np.float32)
    elif kind == "dc":
        wave = f32(100.0 + rng.standard_normal(n))                  # DC offset of 100x the standard deviation
    else:
        wave = f32(0.1 * rng.standard_normal(n) + 0.003)
    stats = np.empty((nwin, 2), np.float32)
    _lib.check(lib.rvb_test_window_stats(fptr(wave), n, first, nwin, step, length, 1e-5, fptr(stats)))
    for w in range(nwin):
        x = wave[(first + w) * step:(first + w) * step + length].astype(np.float64)
        mean = x.mean()
        var = ((x - mean) ** 2).mean()
        rstd = 1.0 / np.sqrt(var + 1e-5)
        m2 = (x * x).mean()
        assert abs(stats[w, 0] - mean) <= 4 * U32 * abs(mean) + 1e-300, (w, stats[w, 0], mean)
        assert abs(stats[w, 1] - rstd) <= (4 * U32 + 1e-13 * m2 / (var + 1e-5)) * rstd, (w, stats[w, 1], rstd)
    if kind == "silence":
        assert np.all(stats[:, 0] == 0) and np.allclose(stats[:, 1], 1 / np.sqrt(1e-5), rtol=4 * U32)


def test_window_stats_refuses_a_step_that_breaks_vector_alignment(lib):
    wave = np.zeros(10000, np.float32)
    stats = np.empty((2, 2), np.float32)
    assert lib.rvb_test_window_stats(fptr(wave), 10000, 0, 2, 998, 4000, 1e-5, fptr(stats)) != 0


# ------------------------------------------------------------------------------------ sinc filter bank
def _sinc_ref(wave, filt, stride, n_frames):
    ks = filt.shape[1]
    idx = np.arange(n_frames)[:, None] * stride + np.arange(ks)[None, :]
    fr = wave.astype(np.float64)[idx]                                # [n_frames][ks]
    return fr @ filt.astype(np.float64).T, np.abs(fr) @ np.abs(filt.astype(np.float64)).T


SINC_SHAPES = ([(n, 80, 251, 10) for n in (1, 191, 192, 193, 1023, 1024, 1025, 22900)] +
               [(1025, 40, 129, 4), (193, 1, 129, 4), (1100, 80, 251, 5), (300, 40, 129, 5), (2, 1, 251, 5)])
# bf16 output at the frame counts that end a partial block in either form, and at the odd stride
SINC_CASES = ([(F32,) + c for c in SINC_SHAPES] +
              [(BF16,) + c for c in SINC_SHAPES if c[0] in (193, 1025, 22900, 1100, 300)])


@pytest.mark.parametrize("form", ["mfma", "valu"])
@pytest.mark.parametrize("dtype,n_frames,nf,ksize,stride", SINC_CASES)
def test_sinc_conv(lib, monkeypatch, lab, form, dtype, n_frames, nf, ksize, stride):
    """Both forms (RVD_SINC_MFMA = 1: v_mfma_f32_32x32x2_f32, 1 024 frames per workgroup, even strides only -- stride 5 takes the
    VALU form either way; 0: the VALU form, 192 frames per workgroup), fp32 accumulation over ksize taps: |err| <= ksize u
    sum|w x| (+ half a bf16 ulp of the output).  Frame counts straddle both forms' workgroup sizes.  Catches: the last partial
    block's frames dropped or shifted, a k-slot of the MFMA form that starts at tap 125 instead of 126, filter f + 40 of the VALU
    form's filter pair written to f, the sample window of a block starting one stride late."""
    monkeypatch.setenv("RVD_SINC_MFMA", "1" if form == "mfma" else "0")
    rng = np.random.default_rng(n_frames * 7 + nf + stride)
    n_samples = (n_frames - 1) * stride + ksize
    wave = f32(rng.standard_normal(n_samples) * 0.3)
    filt = f32(rng.standard_normal((nf, ksize)) / np.sqrt(ksize))
    out = np.empty((n_frames, nf), np.float32)
    _lib.check(lib.rvb_test_sinc_conv(dtype, fptr(wave), n_samples, fptr(filt), nf, ksize, stride, n_frames, fptr(out)))
    ref, mag = _sinc_ref(wave, filt, stride, n_frames)
    tol = ksize * U32 * mag
    _check_within(out, ref, tol + _half_ulp(dtype, ref, tol) + 1e-30, "sinc %s" % form)


def test_sinc_conv_refuses_what_neither_form_covers(lib):
    wave = np.zeros(5000, np.float32)
    filt = np.zeros((81, 251), np.float32)
    out = np.empty((100, 81), np.float32)
    assert lib.rvb_test_sinc_conv(F32, fptr(wave), 5000, fptr(filt), 81, 251, 10, 100, fptr(out)) != 0      # 81 filters
    assert lib.rvb_test_sinc_conv(F32, fptr(wave), 5000, fptr(filt), 80, 251, 17, 100, fptr(out)) != 0      # stride 17
    assert lib.rvb_test_sinc_conv(F32, fptr(wave), 5000, fptr(filt), 80, 252, 10, 100, fptr(out)) != 0      # 252 taps


# ------------------------------------------------------------------------------------ pool_norm
POOL_FIRST = [  # frames_in, W, frame0, frames per step, C, ld_out
    (15975, 3, 1601, 1600, 80, 80),          # the product's shape (160 000 samples, stride 10), craw_frame0 != 0
    (601, 4, 0, 200, 80, 80),                # frames_in % 3 == 1
    (602, 2, 7, 150, 80, 80),                # frames_in % 3 == 2
    (8, 5, 3, 3, 80, 80),                    # 2 pooled frames: fewer than every form's slots
    (4, 2, 0, 1, 80, 80),                    # 1 pooled frame: variance 0 everywhere
    (301, 2, 5, 100, 56, 64),                # C < ld_out, C a multiple of 8: the vector form must not take it (reads past the row)
    (301, 2, 5, 100, 60, 64),                # C < ld_out
]


@pytest.mark.parametrize("form", ["f32", "bf16_scalar", "bf16_vec"])
@pytest.mark.parametrize("frames_in,W,frame0,fstep,C,ld_out", POOL_FIRST)
def test_pool_norm_first_block(lib, monkeypatch, lab, form, frames_in, W, frame0, fstep, C, ld_out):
    """First block: |a craw + off| with a = wn_gamma rstd_w and off = (wn_beta - a mean_w) fsum_c, max-pooled by 3, normalised over
    the pooled frames with fp64 statistics (one pass) and leaky-relu'd; pad channels C .. ld_out exactly 0.  Channel 3 is
    constant (variance 0: rstd = 1 / sqrt(eps), output = beta).  Catches: craw_frame0 or the per-window frame step ignored, the
    last pooled frame of frames_in % 3 != 0 mis-counted, pad columns left unwritten (the output buffer starts at 3.4e38), the
    affine correction's sign flipped (|.| after it, not before)."""
    dtype = F32 if form == "f32" else BF16
    monkeypatch.setenv("RVD_POOLNORM_VEC", "1" if form == "bf16_vec" else "0")
    rng = np.random.default_rng(frames_in + C)
    TP = frames_in // 3
    rows = frame0 + (W - 1) * fstep + 3 * TP
    craw = rnd(dtype, rng.standard_normal((rows, C)) * 2.0 + 0.5)
    craw[:, 3] = craw[0, 3]
    stats = f32(np.stack([rng.standard_normal(W) * 0.1, 1.0 + rng.random(W) * 5], 1))
    fsum = f32(rng.standard_normal(C))
    gamma, beta = f32(0.5 + rng.random(C)), f32(rng.standard_normal(C))
    wg, wb = 0.8, 0.05
    out = np.empty((W * TP, ld_out), np.float32)
    _lib.check(lib.rvb_test_pool_norm(dtype, 1, None, 0, 0, frames_in, C, ld_out, fptr(gamma), fptr(beta), 1e-5, W, fptr(craw), rows,
                                      frame0, fstep, fptr(stats), fptr(fsum), wg, wb, fptr(out)))
    y, tol = _pool_norm_ref(dtype, True, None, W, frames_in, C, ld_out, gamma, beta, 1e-5, craw, frame0, fstep, stats, fsum, wg, wb)
    got = out.reshape(W, TP, ld_out)
    assert np.all(got[:, :, C:] == 0), "pad channels not zero"
    _check_within(got[:, :, :C], y, tol, "pool_norm first %s" % form)
    want = beta[3] if beta[3] > 0 else 0.01 * beta[3]               # constant channel: (v - mean) = 0, whatever rstd
    assert np.abs(got[:, :, 3] - want).max() <= tol[:, :, 3].max()


POOL_LATER = [  # rows_in, frames_in, W, C, ld_in, ld_out
    (5325, 5325, 3, 60, 64, 64),             # layer 2 of the product (frames_in % 3 == 0)
    (1779, 1775, 2, 60, 64, 64),             # rows_in > frames_in, frames_in % 3 == 2
    (700, 601, 3, 80, 80, 80),               # C == ld_out, frames_in % 3 == 1
    (9, 7, 4, 60, 64, 64),                   # 2 pooled frames
    (400, 400, 2, 40, 48, 64),               # rows narrower than ld_out: the vector form must not take it
]


@pytest.mark.parametrize("form", ["f32", "bf16_scalar", "bf16_vec"])
@pytest.mark.parametrize("rows_in,frames_in,W,C,ld_in,ld_out", POOL_LATER)
def test_pool_norm_later_block(lib, monkeypatch, lab, form, rows_in, frames_in, W, C, ld_in, ld_out):
    """Later blocks: max-pool 3 of the conv output, instance norm, leaky relu; bound as for the first block.  Channel 5 carries a
    DC offset of 1 000 over a spread of 1 (one-pass fp64 variance: still exact to 1e-10), channel 7 is constant.  The input's pad
    channels hold 1e4: read into a statistic they would show.  Catches: a window's rows taken at frames_in instead of rows_in,
    pad columns unwritten, a slot stride that skips or repeats pooled frames when there are fewer of them than slots."""
    dtype = F32 if form == "f32" else BF16
    monkeypatch.setenv("RVD_POOLNORM_VEC", "1" if form == "bf16_vec" else "0")
    rng = np.random.default_rng(rows_in + C)
    TP = frames_in // 3
    x = rng.standard_normal((W * rows_in, ld_in)) * 1.5
    x[:, C:] = 1e4
    x[:, 5] += 1000.0
    x[:, 7] = -0.75
    x = rnd(dtype, x)
    gamma, beta = f32(0.5 + rng.random(C)), f32(rng.standard_normal(C))
    out = np.empty((W * TP, ld_out), np.float32)
    _lib.check(lib.rvb_test_pool_norm(dtype, 0, fptr(x), rows_in, ld_in, frames_in, C, ld_out, fptr(gamma), fptr(beta), 1e-5, W, None, 0,
                                      0, 0, None, None, 0.0, 0.0, fptr(out)))
    y, tol = _pool_norm_ref(dtype, False, x, W, frames_in, C, ld_out, gamma, beta, 1e-5, rows_in=rows_in)
    got = out.reshape(W, TP, ld_out)
    assert np.all(got[:, :, C:] == 0), "pad channels not zero"
    _check_within(got[:, :, :C], y, tol, "pool_norm later %s" % form)


# ------------------------------------------------------------------------------------ conv1d5
@pytest.mark.parametrize("cin", [80, 64])
@pytest.mark.parametrize("M", [1, 5, 255, 256, 257, 4097, 256 * 256 + 1, 3 * 256 * 256 + 77])
def test_conv1d5(lib, cin, M):
    """SincNet conv layers 2 / 3 on the persistent thin-GEMM kernel (bf16 operands, fp32 accumulation of 5 cin products):
    |err| <= 5 cin u sum|a w| + half a bf16 ulp.  256 * 256 + 1 and 3 * 256 * 256 + 77 rows give every workgroup of a 256-CU
    part two to four 256-frame tiles through the double-buffered LDS handoff; the device input has rows M + 4 .. M + 7 at 1e30
    (an over-read shows), cin 64 carries random values in its 4 pad channels (zero weights).  Catches: a dropped or shifted last
    tile, a stale second LDS buffer (tile n + grid computed from tile n's rows), the K tail of the last half MFMA step not
    zeroed (cin 80: K = 400), pad filters 60 .. 63 not zero."""
    cr = 80 if cin == 80 else 60
    rng = np.random.default_rng(M + cin)
    A = bf16_round(rng.standard_normal((M + 4, cin)))
    Wt = bf16_round(rng.standard_normal((60, cr, 5)) / np.sqrt(5 * cr))
    bias = f32(rng.standard_normal(60) * 0.1)
    out = np.empty((M, 64), np.float32)
    _lib.check(lib.rvb_test_conv1d5(cin, fptr(A), M + 4, fptr(Wt), fptr(bias), fptr(out), M))
    ref, tol = conv1d5_ref(A, Wt, bias, M, cin)
    assert np.all(out[:, 60:] == 0), "pad filters not zero"
    _check_within(out[:, :60], ref, tol, "conv1d5")


# ------------------------------------------------------------------------------------ LSTM layer
LSTM_CASES = [(1, 1, 64), (3, 2, 256), (15, 37, 64), (16, 37, 256), (17, 37, 64), (17, 2, 256), (33, 589, 64), (40, 589, 256),
              (1, 589, 256)]


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("W,T,inp", LSTM_CASES)
def test_lstm_layer(lib, dtype, W, T, inp):
    """One bidirectional layer (hidden 128) as the engine runs it: the input-projection GEMM into the recurrence kernel's column
    order (lstm_pack_inproj, shared with the engine), then lstm_recurrence (16 windows per block; 17 / 33 / 40 windows run blocks
    1 and 2 and a partial last block).  Some units are driven to pre-activations of +-25 .. 40 (saturated gates on the bf16
    exp2 / rcp path).  Bounds: f32 1e-4 (fp32 sums of in + 128 terms per step carried through 589 steps of a contracting
    recurrence; the MI355X measured 3.7e-5 at 40 x 589 x 256, 6e-6 elsewhere); bf16 max 4e-2, mean 5e-5 (h_t is rounded to bf16
    every step on both sides, but a rounding that falls the other way near a tie is one bf16 ulp of |h|, 3.9e-3, that feeds
    back: measured max 1.6e-2 = 4 ulps, mean 9e-6).  Forward and reverse halves are checked separately.  Catches: an
    i / f gate swap, a reverse direction that starts at t = 0, a 16-unit group of the gate permutation off by one, the clamped
    windows of a partial block written out, the second block reading block 0's windows."""
    H = 128
    rng = np.random.default_rng(W * 1000 + T + inp)
    cr = 60 if inp == 64 else inp
    x = np.zeros((W * T, inp))
    x[:, :cr] = rng.standard_normal((W * T, cr))
    x = rnd(dtype, x)
    w_ih = np.zeros((2, 4 * H, inp))
    w_ih[:, :, :cr] = rng.standard_normal((2, 4 * H, cr)) / np.sqrt(cr)
    w_ih = rnd(dtype, w_ih)
    w_hh = rnd(dtype, rng.standard_normal((2, 4 * H, H)) / np.sqrt(H))     # contracting: 1.5 / sqrt(H) let a rounding grow 1e3x
    b_ih = rng.standard_normal((2, 4 * H)) * 0.2
    b_hh = rng.standard_normal((2, 4 * H)) * 0.2
    sat = rng.choice(4 * H, 24, replace=False)
    b_ih[:, sat] += rng.choice([-1.0, 1.0], (2, 24)) * rng.uniform(25, 40, (2, 24))
    b_ih, b_hh = f32(b_ih), f32(b_hh)
    out = np.empty((W * T, 2 * H), np.float32)
    _lib.check(lib.rvb_test_lstm_layer(dtype, fptr(x), W, T, inp, fptr(w_ih), fptr(w_hh), fptr(b_ih), fptr(b_hh), fptr(out)))
    ref = _lstm_ref(dtype, x, W, T, w_ih, w_hh, b_ih, b_hh)
    for d, name in ((0, "forward"), (1, "reverse")):
        e = np.abs(out[:, d * H:(d + 1) * H] - ref[:, d * H:(d + 1) * H])
        if dtype == F32:
            assert e.max() < LSTM_F32_MAX, (name, e.max())
        else:
            assert e.max() < LSTM_BF16_MAX and e.mean() < LSTM_BF16_MEAN, (name, e.max(), e.mean())


# ------------------------------------------------------------------------------------ classifier + log-softmax
CLS_CASES = [  # C, in, ldx, M, bias offset
    (7, 128, 128, 3534, 0.0), (7, 128, 136, 257, 1000.0), (16, 256, 264, 256, 0.0), (16, 256, 256, 255, 1000.0),
    (1, 8, 16, 255, 0.0), (16, 8, 8, 1, 0.0), (7, 256, 256, 257, 0.0)]


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("C,inp,ldx,M,offset", CLS_CASES)
def test_classifier(lib, dtype, C, inp, ldx, M, offset):
    """logp = log_softmax(x W^T + b) with fp32 dot products of `in` terms started from the bias: |err| <= (in + 2) u sum|x w| +
    |b|) twice (logit and the log-sum-exp's maximum) + 8 u |logsumexp|; an offset of 1e3 on the biases puts the logits around 1e3.
    Rows 0 and 1 are equal and classes 2 and 5 have equal weights and biases: an exact tie whenever they lead, which must go to
    class 2, the first index (torch.argmax).  Elsewhere the argmax must agree with the reference where its top two differ by more
    than twice the bound.  Columns in .. ldx of x hold 1e6.  Catches: ties going to the last index (a >= for the >), the row
    stride ldx replaced by in, the maximum not subtracted (exp overflows at 1e3), the last of 16 classes dropped."""
    rng = np.random.default_rng(C * 100 + inp + M)
    x = rng.standard_normal((M, ldx))
    x[:, inp:] = 1e6
    if M > 1:
        x[0] = x[1]
    x = rnd(dtype, x)
    w = rng.standard_normal((C, inp)) / np.sqrt(inp)
    b = rng.standard_normal(C) + offset
    if C >= 6:
        w[5], b[5] = w[2], b[2]
        b[2] = b[5] = (x[0, :inp].astype(np.float64) @ w[:C].T.astype(np.float64) + b[:C]).max() - x[0, :inp] @ w[2] + 1.0
    w, b = f32(w), f32(b)
    logp = np.empty((M, C), np.float32)
    cls = np.full(M, 99, np.uint8)
    _lib.check(lib.rvb_test_classifier(dtype, fptr(x), ldx, fptr(w), fptr(b), fptr(logp), cls.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                       M, inp, C))
    ref, tol, z = classifier_ref(x[:, :inp], w, b)
    _check_within(logp, ref, tol, "classifier logp")
    if C == 1:
        assert np.all(logp == 0) and np.all(cls == 0)
    if C >= 6:                    # classes 2 and 5 tie exactly (same weights, bias and summation); where they lead, 2 wins
        lead = z[:, 2] - np.delete(z, [2, 5], 1).max(1) > 2 * tol[:, 0]
        assert lead[0] and np.all(cls[lead] == 2), cls[lead]
    srt = np.sort(z, 1)
    clear = (srt[:, -1] - srt[:, -2] > 2 * tol[:, 0]) if C > 1 else np.ones(M, bool)
    assert np.array_equal(cls[clear], z.argmax(1)[clear])


def test_classifier_picks_the_first_of_equal_logits(lib):
    """All 16 classes equal (identical weight rows and biases): the argmax is class 0 on every row, logp = -log 16."""
    M, inp, C = 300, 64, 16
    rng = np.random.default_rng(3)
    x = f32(rng.standard_normal((M, inp)))
    w = f32(np.tile(rng.standard_normal(inp), (C, 1)))
    b = f32(np.full(C, 0.25))
    logp = np.empty((M, C), np.float32)
    cls = np.full(M, 99, np.uint8)
    for dtype in (F32, BF16):
        _lib.check(lib.rvb_test_classifier(dtype, fptr(x), inp, fptr(w), fptr(b), fptr(logp), cls.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                           M, inp, C))
        assert np.all(cls == 0)
        np.testing.assert_allclose(logp, -np.log(16.0), rtol=0, atol=8 * U32 * 1e3)


def test_classifier_refuses_shapes_it_does_not_cover(lib):
    x = np.zeros((4, 264), np.float32)
    w = np.zeros((17, 264), np.float32)
    b = np.zeros(17, np.float32)
    logp = np.empty((4, 17), np.float32)
    assert lib.rvb_test_classifier(F32, fptr(x), 264, fptr(w), fptr(b), fptr(logp), None, 4, 128, 17) != 0      # 17 classes
    assert lib.rvb_test_classifier(F32, fptr(x), 264, fptr(w), fptr(b), fptr(logp), None, 4, 264, 7) != 0       # 264 inputs


# ------------------------------------------------------------------------------------ TSTP statistics pooling
@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("mask_len,TT", [(589, 125), (589, 256), (100, 256), (7, 3), (589, 1)])
def test_tstp(lib, dtype, mask_len, TT):
    """Masked mean / std over trunk frames, frame weights = the mask resampled by torch's nearest interpolation (the index map is
    taken from F.interpolate itself), statistics in fp64: v1 = sum w + 1e-8, mean = sum w x / v1, var = sum w (x - mean)^2 /
    (v1 - sum w^2 / v1 + 1e-8).  Items per window: binary, soft, all-zero, one active frame that the resampling keeps, one that
    it drops (when the ratio drops any), in an order unlike item_b's.  Bounds: the kernel's fp32 v1 and denominator (their 1e-8
    terms are below fp32 resolution) and fp64 sums -> mean within 8 TT u sum w|x| / v1; std within 8 TT u std (1 + (v1 +
    v2 / v1) / den) plus sqrt(s1 / den) times the mean's error; plus half a bf16 ulp.  Catches: a floor / round mismatch in the
    mask map (the dropped frame would count), weights taken from another item's mask, the bordered plane indexed without its
    border (reads the 1e3 border), a biased / unbiased denominator swap."""
    rng = np.random.default_rng(mask_len * 3 + TT)
    B, F, C = 3, 2, 40
    idx = _nearest_map(mask_len, TT)
    kept = np.unique(idx)
    dropped = np.setdiff1d(np.arange(mask_len), kept)
    masks = [(rng.random(mask_len) < 0.4).astype(np.float32), rng.random(mask_len).astype(np.float32),
             np.zeros(mask_len, np.float32)]
    one = np.zeros(mask_len, np.float32)
    one[kept[len(kept) // 2]] = 1.0
    masks.append(one)
    if len(dropped):
        gone = np.zeros(mask_len, np.float32)
        gone[dropped[len(dropped) // 2]] = 1.0
        masks.append(gone)
    masks.append(np.ones(mask_len, np.float32))
    n_items = len(masks)
    item_b = i32([(2 * k + 1) % B for k in range(n_items)])       # 1, 0, 2, 1, ...: not the items' order
    mask = f32(np.stack(masks))
    x = rnd(dtype, rng.standard_normal((B, F, TT, C)) * 0.7 + 0.3)
    stats = np.empty((n_items, 2 * C * F), np.float32)
    _lib.check(lib.rvb_test_tstp(dtype, fptr(x), B, iptr(item_b), fptr(mask), mask_len, n_items, F, TT, C, fptr(stats)))
    for it in range(n_items):
        w = mask[it, idx].astype(np.float64)                          # [TT]
        xv = x[item_b[it]].astype(np.float64).transpose(2, 0, 1)      # [C][F][TT]
        s1 = w.sum()
        mean, std, m_tol, s_tol = _tstp_ref(dtype, xv, w)
        got = stats[it].reshape(2, C, F)
        _check_within(got[0], mean, m_tol, "tstp mean, item %d" % it)
        _check_within(got[1], std, s_tol, "tstp std, item %d" % it)
        if s1 == 0:
            assert np.all(got == 0), "an empty mask gives zero statistics"
