"""fp64 references and derived bounds of the segmentation network's stages, shared by the kernel tests
(tests/test_diar_kernels_gpu.py: each kernel through its rvb_test_* hook on random operands), the bf16-storage restatement of the
whole network (oracle/diar_bf16_ref.py) and the stage-by-stage checks of the engine's own tensors (tests/test_diar_bf16_gpu.py).
Nothing here needs a GPU.

Tolerances follow the rounding model of each kernel and are computed per element: an fp32 sum of K terms is off by at most
K u sum|terms| (u = 2^-24, one rounding per fused multiply-add), every bf16 rounding point adds half a bf16 ulp (at most 2^-8 of
the value: 8 significant bits), and where the reference cannot round at the kernel's points (the LSTM's h_t, which feeds back)
the bound is the one measured on an MI355X times a small factor (LSTM_BF16_MAX / LSTM_BF16_MEAN)."""
import numpy as np

from util import bf16_round

F32, BF16 = 0, 1
U32 = 2.0 ** -24          # fp32 unit roundoff
HB = 2.0 ** -8            # half a bf16 ulp, relative to the value: at most 2^-8 (8 significant bits)

# test_lstm_layer's bounds: f32 max; bf16 max and mean of |h - ref| per direction (measured max 1.6e-2 = 4 ulps, mean 9e-6)
LSTM_F32_MAX = 1e-4
LSTM_BF16_MAX, LSTM_BF16_MEAN = 4e-2, 5e-5


def half_ulp(dtype, ref, tol=0.0):
    """the output rounding of a value known to within tol of ref"""
    return HB * (np.abs(ref) + tol) if dtype == BF16 else 0.0


def check_within(got, ref, tol, what):
    err = np.abs(got.astype(np.float64) - ref)
    bad = err > tol
    assert not bad.any(), "%s: %d elements outside the bound, worst err %.3g at bound %.3g (max err %.3g)" % (
        what, int(bad.sum()), float(err[bad].max()), float(np.asarray(tol * np.ones_like(err))[bad][np.argmax(err[bad])]),
        float(err.max()))
    return float(err.max())


# ------------------------------------------------------------------------------------ pool_norm
def pool_norm_ref(dtype, first, xin, W, frames_in, C, ld_out, gamma, beta, eps, craw=None, frame0=0, fstep=0, stats=None,
                  fsum=None, wn_gamma=1.0, wn_beta=0.0, rows_in=0, win=None, details=None):
    """fp64: max-pool 3 -> instance norm over the pooled frames -> leaky relu 0.01.  Returns (y [W][TP][C], bound).
    win (first block, optional): window w reads craw from frame frame0 + win[w] * fstep instead of frame0 + w * fstep.
    details (optional dict): receives the intermediate fp64 values pooled [W][TP][C], P (the pooled magnitudes) [W][TP][C], mean and
    g = gamma / sqrt(var + eps) [W][C], for callers that bound further inputs of their own."""
    TP = frames_in // 3
    ys, tols = [], []
    for w in range(W):
        if first:
            a = wn_gamma * float(stats[w, 1])
            off = (wn_beta - a * float(stats[w, 0])) * fsum.astype(np.float64)
            r0 = frame0 + (w if win is None else int(win[w])) * fstep
            raw = craw[r0:r0 + 3 * TP].astype(np.float64)               # [3TP][C]
            v = np.abs(a * raw + off)
            mag = np.abs(a * raw) + np.abs(off)
        else:
            raw = xin[w * rows_in:w * rows_in + 3 * TP, :C].astype(np.float64)
            v = raw
            mag = np.abs(raw)
        pooled = v.reshape(TP, 3, C).max(1)
        P = mag.reshape(TP, 3, C).max(1)
        mean = pooled.mean(0)
        var = ((pooled - mean) ** 2).mean(0)
        g = gamma.astype(np.float64) / np.sqrt(var + eps)
        y = (pooled - mean) * g + beta
        y = np.where(y > 0, y, 0.01 * y)
        # fp32 on the pooled value, the affine correction, scale / shift and the fma: 64 u |g| (P + |mean|) + 16 u |beta|
        tol = 64 * U32 * np.abs(g) * (P + np.abs(mean)) + 16 * U32 * np.abs(beta)
        ys.append(y)
        tols.append(tol)
        if details is not None:
            for k, v in (("pooled", pooled), ("P", P), ("mean", mean), ("g", g)):
                details.setdefault(k, []).append(v)
    if details is not None:
        for k in details:
            details[k] = np.stack(details[k])
    y, tol = np.stack(ys), np.stack(tols)
    if dtype == BF16:
        tol = tol + HB * (np.abs(y) + tol)
    return y, tol + 1e-30


# ------------------------------------------------------------------------------------ conv1d5
def conv1d5_ref(A, Wt, bias, M, cin):
    """SincNet conv layers 2 / 3, fp64: out[m][o] = bias[o] + sum_{k < 5, c} A[m + k][c] Wt[o][c][k] for m < M.  A [>= M + 4][>= cr]
    (bf16 values; columns from cr = Wt.shape[1] on are pad channels, which carry zero weights), Wt [60][cr][5] (bf16 values), bias
    fp32.  Returns (ref [M][60], bound): bf16 operands, fp32 accumulation of 5 cin products started from the bias (cin = the
    kernel's row width, pad channels included) -> (5 cin + 1) u sum|a w| + half a bf16 ulp."""
    cr = Wt.shape[1]
    A64, W64 = A[:, :cr].astype(np.float64), Wt.astype(np.float64)
    ref = np.tile(bias.astype(np.float64), (M, 1))
    mag = np.tile(np.abs(bias.astype(np.float64)), (M, 1))
    for k in range(5):
        ref += A64[k:k + M] @ W64[:, :, k].T
        mag += np.abs(A64[k:k + M]) @ np.abs(W64[:, :, k]).T
    tol = (5 * cin + 1) * U32 * mag
    return ref, tol + half_ulp(BF16, ref, tol) + 1e-30


# ------------------------------------------------------------------------------------ LSTM layer
def sig(x):
    return 0.5 * (1.0 + np.tanh(0.5 * x))


def lstm_ref(dtype, x, W, T, w_ih, w_hh, b_ih, b_hh, store=None, fed_back=None):
    """fp64 bidirectional layer on the rounded operands; the projection rounded where the GEMM stores it and h_t rounded after
    every step where the kernel stores it (bf16); the cell state stays unrounded (the kernel keeps it in fp32 registers).
    store (optional): the rounding applied at those two points instead of dtype's, a function (name, fp64 array) -> fp64 array
    with name 'xproj' or 'h'.
    fed_back (optional, [W * T][2 H]): a run's own STORED output.  The h_{t-1} that enters step t's gates is then taken from it (the
    value the kernel stored and read back, exact in bf16) instead of from this reference's previous step, so that every step is
    checked from the kernel's stored input and a rounding that fell the other way is not carried through the recurrence; the cell
    state is still this reference's own, carried in fp64 from the first step.
    Returns [W * T][2 H] (forward | reverse)."""
    H = w_hh[0].shape[1]
    if store is None:
        store = (lambda name, v: bf16_round(v).astype(np.float64)) if dtype == BF16 else (lambda name, v: v)
    out = np.zeros((W, T, 2 * H))
    xw = x.astype(np.float64).reshape(W, T, -1)
    fb = None if fed_back is None else np.asarray(fed_back, np.float64).reshape(W, T, 2 * H)
    for d in range(2):
        xp = xw @ w_ih[d].astype(np.float64).T + (b_ih[d].astype(np.float64) + b_hh[d].astype(np.float64))
        xp = store("xproj", xp)
        whh = w_hh[d].astype(np.float64)
        h = np.zeros((W, H))
        c = np.zeros((W, H))
        for s in range(T):
            t = T - 1 - s if d else s
            if fb is not None and s > 0:
                h = fb[:, t + 1 if d else t - 1, d * H:(d + 1) * H]
            g = xp[:, t] + h @ whh.T
            i, f, gg, o = sig(g[:, :H]), sig(g[:, H:2 * H]), np.tanh(g[:, 2 * H:3 * H]), sig(g[:, 3 * H:])
            c = f * c + i * gg
            h = store("h", o * np.tanh(c))
            out[:, t, d * H:(d + 1) * H] = h
    return out.reshape(W * T, 2 * H)


# ------------------------------------------------------------------------------------ classifier + log-softmax
def classifier_ref(x, w, b):
    """logp = log_softmax(x W^T + b) in fp64; x [M][in] (the stored values), w fp32 [C][in], b fp32 [C].  Returns (logp, bound
    [M][1], logits): fp32 dot products of `in` terms started from the bias: |err| <= (in + 2) u (sum|x w| + |b|) twice (logit and the
    log-sum-exp's maximum) + 8 u |logsumexp| + 1e-6."""
    inp = x.shape[1]
    xx, w64, b64 = x.astype(np.float64), w.astype(np.float64), b.astype(np.float64)
    z = xx @ w64.T + b64
    mx = z.max(1, keepdims=True)
    lse = mx + np.log(np.exp(z - mx).sum(1, keepdims=True))
    mag = (np.abs(xx) @ np.abs(w64).T + np.abs(b64)).max(1, keepdims=True)
    tol = 2 * (inp + 2) * U32 * mag + 8 * U32 * np.abs(lse) + 1e-6
    return z - lse, tol, z
