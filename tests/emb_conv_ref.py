"""fp64 references and derived bounds of the speaker-embedding network's kernels (csrc/resnet.hip conv_kernel / emb_conv1_kernel /
tstp_kernel, conv_gemm.hip, conv_row64.hip, conv_stream.hip, conv_block.hip, conv_s2.hip), shared by the kernel tests
(tests/test_emb_conv_kernels_gpu.py, tests/test_diar_kernels_gpu.py test_tstp) and the stage-by-stage check of the bf16 engine on its
own stored tensors (oracle/emb_bf16_ref.py, tests/emb_bf16_checks.py).  Nothing here needs a GPU.

Bounds follow the rounding model and hold for every element: an fp32 sum of K products plus the bias (and the residual) is off by
at most (K + 2) u sum|terms| (u = 2^-24); K counts the fused shortcut's channels when it rides in the K loop.  A bf16 output adds
half a bf16 ulp, at most 2^-8 of the value."""
import numpy as np

F32, BF16 = 0, 1
U32 = 2.0 ** -24          # fp32 unit roundoff
HB = 2.0 ** -8            # half a bf16 ulp, relative to the value: at most 2^-8 (8 significant bits)


def check_within(got, ref, tol, what):
    """every element within its bound; returns the worst error / bound ratio"""
    err = np.abs(got.astype(np.float64) - ref)
    bad = err > tol
    assert not bad.any(), "%s: %d elements outside the bound, worst err %.3g at bound %.3g (max err %.3g)" % (
        what, int(bad.sum()), float(err[bad].max()), float(np.asarray(tol * np.ones_like(err))[bad][np.argmax(err[bad])]),
        float(err.max()))
    return float((err / np.maximum(tol, 1e-300)).max())


def conv_ref(op, relu, batches=None):
    """fp64 convolution of the rounded operands (3x3 pad 1 or 1x1, stride s; + the 1x1 / stride2 shortcut) -> (ref, bound
    (K + 2) u sum|terms|), for the windows `batches` (default all).  op: x [B][Fi][Ti][Cin], w [Cout][Cin][k][k], bias [Cout] fp32,
    res [B][Fo][To][Cout] or None, x2 [B][Fi2][Ti2][Cin2] / w2 [Cout][Cin2] or None, stride, stride2."""
    import torch
    sel = slice(None) if batches is None else list(batches)
    x, w, s = op["x"][sel].astype(np.float64), op["w"].astype(np.float64), op["stride"]
    B, Fi, Ti, Cin = x.shape
    Cout, k = w.shape[0], w.shape[2]
    Fo, To = (Fi - 1) // s + 1, (Ti - 1) // s + 1
    K = k * k * Cin

    def conv(a, wt, stride, pad):
        """fp64 sum of products and sum of their magnitudes, [B * Fo * To][Cout] each (torch's fp64 convolution: plain sums)"""
        ta, tw = torch.from_numpy(np.ascontiguousarray(a.transpose(0, 3, 1, 2))), torch.from_numpy(np.ascontiguousarray(wt))
        with torch.no_grad():
            y = torch.nn.functional.conv2d(ta, tw, stride=stride, padding=pad)[:, :, :Fo, :To]
            m = torch.nn.functional.conv2d(ta.abs(), tw.abs(), stride=stride, padding=pad)[:, :, :Fo, :To]
        return (y.permute(0, 2, 3, 1).reshape(-1, Cout).numpy().copy(), m.permute(0, 2, 3, 1).reshape(-1, Cout).numpy().copy())
    acc, mag = conv(x, w, s, 1 if k == 3 else 0)
    if op["x2"] is not None:
        x2 = op["x2"][sel].astype(np.float64)
        a2, m2 = conv(x2, op["w2"].astype(np.float64).reshape(Cout, -1, 1, 1), op["stride2"], 0)
        acc += a2
        mag += m2
        K += x2.shape[-1]
    acc += op["bias"]
    mag += np.abs(op["bias"].astype(np.float64))
    if op["res"] is not None:
        r = op["res"][sel].astype(np.float64).reshape(-1, Cout)
        acc += r
        mag += np.abs(r)
    ref = np.maximum(acc, 0.0) if relu else acc
    return ref.reshape(B, Fo, To, Cout), ((K + 2) * U32 * mag).reshape(B, Fo, To, Cout)


def conv_ref_pixels(op, relu, pix):
    """the same reference for single output pixels pix [n][3] = (b, fo, to): 3x3 convolutions without a shortcut"""
    x, w, s = op["x"], op["w"].astype(np.float64), op["stride"]
    Fi, Ti = x.shape[1:3]
    Cout, Cin = w.shape[:2]
    acc = np.zeros((len(pix), Cout))
    mag = np.zeros_like(acc)
    for kh in range(3):
        for kw in range(3):
            f, t = s * pix[:, 1] + kh - 1, s * pix[:, 2] + kw - 1
            inside = ((f >= 0) & (f < Fi) & (t >= 0) & (t < Ti))[:, None]
            a = np.where(inside, x[pix[:, 0], np.clip(f, 0, Fi - 1), np.clip(t, 0, Ti - 1)], 0.0).astype(np.float64)
            acc += a @ w[:, :, kh, kw].T
            mag += np.abs(a) @ np.abs(w[:, :, kh, kw]).T
    acc += op["bias"]
    mag += np.abs(op["bias"].astype(np.float64))
    if op["res"] is not None:
        r = op["res"][pix[:, 0], pix[:, 1], pix[:, 2]].astype(np.float64)
        acc += r
        mag += np.abs(r)
    return (np.maximum(acc, 0.0) if relu else acc), (9 * Cin + 2) * U32 * mag


def conv_bound(dtype, ref, tol):
    """the accumulation bound plus the output's rounding: half a bf16 ulp of a value known to within tol"""
    return tol + (HB * (np.abs(ref) + tol) if dtype == BF16 else 0.0) + 1e-30


def stem_ref(plane, w, bias):
    """The stem, Conv2d(1, C, 3, pad 1) + folded BatchNorm + ReLU, in fp64 on one window's plane [F][T] (= fbank - mean, the fp32
    subtraction the kernel makes), w [C][1][3][3] and bias [C] fp32 (folded) -> (ref [F][T][C], accumulation bound 11 u sum|terms|:
    nine fused multiply-adds from the bias)."""
    plane = np.asarray(plane, np.float64)
    F, T = plane.shape
    C = w.shape[0]
    p = np.pad(plane, 1)
    acc = np.zeros((F, T, C))
    mag = np.zeros_like(acc)
    for kh in range(3):
        for kw in range(3):
            sl = p[kh:kh + F, kw:kw + T][:, :, None]
            acc += sl * w[:, 0, kh, kw].astype(np.float64)
            mag += np.abs(sl) * np.abs(w[:, 0, kh, kw].astype(np.float64))
    acc += bias
    mag += np.abs(np.asarray(bias, np.float64))
    return np.maximum(acc, 0.0), 11 * U32 * mag


def nearest_map(mask_len, TT):
    """torch.nn.functional.interpolate(mode='nearest') from mask_len mask frames to TT trunk frames, taken from torch itself"""
    import torch
    src = torch.arange(mask_len, dtype=torch.float32).reshape(1, 1, mask_len)
    return torch.nn.functional.interpolate(src, size=TT, mode="nearest").reshape(TT).long().numpy()


def tstp_ref(dtype, xv, w):
    """Masked statistics pooling of one item in fp64: xv [C][F][TT] (the stored trunk output of its window), w [TT] the resampled
    frame weights.  v1 = sum w + 1e-8, mean = sum w x / v1, var = sum w (x - mean)^2 / (v1 - sum w^2 / v1 + 1e-8).
    -> (mean [C][F], std [C][F], bound of the mean, bound of the std).  Bounds: the kernel's fp32 v1 and denominator (their 1e-8
    terms are below fp32 resolution) and fp64 sums -> mean within 8 TT u sum w|x| / v1; std within 8 TT u std (1 + (v1 + v2 / v1) /
    den) plus sqrt(s1 / den) times the mean's error; plus half a bf16 ulp of each output."""
    xv, w = np.asarray(xv, np.float64), np.asarray(w, np.float64)
    TT = w.shape[0]
    half = (lambda ref, tol: HB * (np.abs(ref) + tol)) if dtype == BF16 else (lambda ref, tol: 0.0)
    s1, s2 = w.sum(), (w * w).sum()
    v1 = s1 + 1e-8
    mean = (xv * w).sum(-1) / v1
    den = v1 - s2 / v1 + 1e-8
    std = np.sqrt((w * (xv - mean[..., None]) ** 2).sum(-1) / den)
    m_tol = 8 * TT * U32 * (np.abs(xv) * w).sum(-1) / v1
    m_tol = m_tol + half(mean, m_tol) + 1e-30
    dm = np.abs(mean) * (4 * TT * U32 + 2e-8 / max(s1, 1e-8)) + m_tol
    s_tol = 8 * TT * U32 * std * (1 + (v1 + s2 / v1) / den) + np.sqrt(s1 / den) * dm
    s_tol = s_tol + half(std, s_tol) + 1e-30
    return mean, std, m_tol, s_tol
