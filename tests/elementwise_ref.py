"""Plain numpy restatements of the row / elementwise kernels of csrc/elementwise.hip, for tests/test_elementwise_kernels_gpu.py.
Every function computes in `dt` (float64 by default: the reference; float32: an emulation of the kernel's own arithmetic, used as
a yardstick for rounding error).  tests/test_elementwise_ref.py checks them against torch's float64 operators without a GPU."""
import numpy as np

NORM_LN, NORM_AFFINE = 0, 1


def _silu(v):
    return v / (1 + np.exp(-v))


def layer_norm(x, gamma, beta, eps, dt=np.float64):
    x = np.asarray(x, dt)
    mu = x.mean(1, keepdims=True, dtype=dt)
    var = ((x - mu) ** 2).mean(1, keepdims=True, dtype=dt)
    return ((x - mu) / np.sqrt(var + dt(eps)) * np.asarray(gamma, dt) + np.asarray(beta, dt)).astype(dt)


def rownorm(x, gamma, beta, eps, mode=NORM_LN, silu=False, add=None, gamma2=None, beta2=None, eps2=0.0, dt=np.float64):
    """NormArgs: out = [SiLU]((x - mean) * rstd * gamma + beta | x * gamma + beta) [+ add]; out2 = LayerNorm(out; gamma2, beta2, eps2)
    when gamma2 is given (else None).  Biased variance, as nn.LayerNorm."""
    if mode == NORM_LN:
        out = layer_norm(x, gamma, beta, eps, dt)
    else:
        out = np.asarray(x, dt) * np.asarray(gamma, dt) + np.asarray(beta, dt)
    if silu:
        out = _silu(out)
    if add is not None:
        out = out + np.asarray(add, dt)
    out = out.astype(dt)
    out2 = layer_norm(out, gamma2, beta2, eps2, dt) if gamma2 is not None else None
    return out, out2


def glu_frames(G, pw1_bias, lens, K, causal=False, gated=False, hist=None, hist_rows=0):
    """The gated value of every frame the depthwise convolution reads, before the convolution's own zero padding:
    frames [B][T (+ K - 1 in front when causal)][d] and filled [B][frames] = True where the frame is GLU of the pointwise bias --
    rows t >= lens[b] (they were zeroed in front of pointwise_conv1) and, causal, left-context rows older than the `hist_rows` real
    ones.  G is [B][T][2d] (a | b halves; hist [K-1][2d] likewise), or [B][T][d] already gated."""
    G = np.asarray(G, np.float64)
    pb = np.asarray(pw1_bias, np.float64)
    B, T = G.shape[:2]
    d = pb.shape[0] // 2
    bias_glu = pb[:d] / (1 + np.exp(-pb[d:]))
    val = G if gated else G[..., :d] / (1 + np.exp(-G[..., d:]))
    filled = np.arange(T)[None, :] >= np.asarray(lens)[:, None]
    frames = np.where(filled[..., None], bias_glu, val)
    if causal:
        left = np.broadcast_to(bias_glu, (B, K - 1, d)).copy()
        lfill = np.ones((B, K - 1), bool)
        if hist_rows:
            h = np.asarray(hist, np.float64)[K - 1 - hist_rows:]
            left[0, K - 1 - hist_rows:] = h[:, :d] / (1 + np.exp(-h[:, d:]))
            lfill[0, K - 1 - hist_rows:] = False
        frames = np.concatenate([left, frames], 1)
        filled = np.concatenate([lfill, filled], 1)
    return frames, filled


def dwconv(frames, w, b, K, causal=False):
    """Depthwise Conv1d over time: frames [B][N][d] as glu_frames returns them, w [d][K], b [d] (None: no bias) -> [B][T][d].
    Non-causal: "same" zero padding of (K - 1) / 2 on both sides; causal: the K - 1 leading frames are the left context."""
    frames = np.asarray(frames, np.float64)
    w = np.asarray(w, np.float64)
    B, N, d = frames.shape
    if causal:
        T, ext = N - (K - 1), frames
    else:
        T, pad = N, (K - 1) // 2
        ext = np.zeros((B, N + K - 1, d))
        ext[:, pad:pad + N] = frames
    out = np.zeros((B, T, d)) + (0 if b is None else np.asarray(b, np.float64))
    for k in range(K):
        out += ext[:, k:k + T] * w[:, k]
    return out


def glu_dwconv(G, pw1_bias, w, b, lens, K, causal=False, gated=False, hist=None, hist_rows=0):
    frames, _ = glu_frames(G, pw1_bias, lens, K, causal, gated, hist, hist_rows)
    return dwconv(frames, w, b, K, causal)


def conv1(feats, mean, istd, w, b):
    """CMVN + Conv2d(1, d, 3, stride 2) + ReLU: feats [B][T0][F0], w [d][1][3][3] -> [B][T1][F1][d] (NHWC)."""
    xn = (np.asarray(feats, np.float64) - np.asarray(mean, np.float64)) * np.asarray(istd, np.float64)
    w = np.asarray(w, np.float64)
    B, T0, F0 = xn.shape
    T1, F1 = (T0 - 3) // 2 + 1, (F0 - 3) // 2 + 1
    out = np.zeros((B, T1, F1, w.shape[0])) + np.asarray(b, np.float64)
    for kh in range(3):
        for kw in range(3):
            out += xn[:, kh:kh + 2 * T1 - 1:2, kw:kw + 2 * F1 - 1:2, None] * w[:, 0, kh, kw]
    return np.maximum(out, 0)


def clip_scale(ref, top=200):
    """An fp8 scale at which clipping is unambiguous: 448 * scale sits in the geometric middle of the widest gap between neighbours
    among the `top` largest |ref|.  Returns (scale as float32, number of |ref| above 448 * scale, the gap's ratio)."""
    a = np.sort(np.abs(np.asarray(ref, np.float64)).ravel())[::-1][:top]
    a = a[a > 0]
    ratio = a[:-1] / a[1:]
    i = int(ratio.argmax())
    scale = np.float32(np.sqrt(a[i] * a[i + 1]) / 448.0)
    return scale, int((np.abs(ref) > 448.0 * float(scale)).sum()), float(ratio[i])
