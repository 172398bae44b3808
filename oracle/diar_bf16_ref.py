"""TEST INFRASTRUCTURE ONLY (oracle) -- never imported by the product path.

A restatement of oracle/diar_ref.py's PyanNet in fp64 arithmetic that rounds to bf16 (round to nearest even, tests/util.py
bf16_round: fp64 -> fp32 -> bf16, the engine's accumulators being fp32) exactly where the bf16 engine stores bf16, and nowhere
else.  It is the yardstick of what bf16 STORAGE costs: the engine's distance from the fp32 oracle is held to this restatement's
distance from it (tests/test_diar_bf16_gpu.py, fixture tests/golden/diar_bf16_yardstick.json written by
oracle/gen_golden_diar_bf16.py).  torch.autocast('cpu', bfloat16) cannot serve: it rounds the 251-tap sinc convolution of the
raw waveform, which the engine keeps in fp32.

Storage points (reverb_amd/csrc/..., read from segment_impl, diar_engine.hip:297-368, and finalize_impl, :226-293):

  tensor                                   stored by                                             read by
  craw    sinc conv of the RAW waveform    diar.hip:76-77 / :143 (sinc kernels, Cvt<O>)          diar_engine.hip:326 (pool_norm, first block:
          (shared by every window)         called at diar_engine.hip:985                         |a (craw - mean fsum) + b fsum|, kernels.h:371)
  a1      block 1 output [p1][80]          diar.hip:302 / :400 (pool_norm), diar_engine.hip:325  :330 conv 2
  c2      conv 2 output  [p1][64]          diar.hip:541 (conv1d5), diar_engine.hip:330           :332 pool_norm
  a2      block 2 output [p2][64]          diar_engine.hip:333                                   :335 conv 3
  c3      conv 3 output  [p2][64]          diar_engine.hip:335                                   :337 pool_norm
  a3      block 3 output [589][64]         diar_engine.hip:338                                   :346 input projection of LSTM layer 0
  xproj   x W_ih^T + b_ih + b_hh [8H]      GEMM epilogue, diar_engine.hip:346                    :349 recurrence
  h       every LSTM layer's h_t           diar.hip:685-687: ONE rounded value goes to the       next step, next layer (:346) or linear 0 (:355)
                                           output tensor and to the LDS copy the next step reads
  l0, l1  linear outputs (after LeakyReLU) GEMM epilogue, diar_engine.hip:355                    next linear / classifier (:359)
  weights conv 2, conv 3 (:200), W_ih (:268), W_hh (:270), linear (:280): pack_T, diar_engine.hip:128-135 (convert_f32, RNE)

Not rounded: biases, norm parameters (fp32 uploads, up_f32), window statistics (fp32 from fp64 sums), the pooling statistics
(fp64), the cell state c (fp32 registers), the sinc filters and their sums, the classifier's weights (:286) and logp (fp32).
The fast exp2 / rcp sigmoid and tanh of GateMath<bf16_t> (diar.hip:586-589) are NOT modelled: they are arithmetic, not storage.

The stage functions below are what pyannet_bf16 is made of; each can be run on given inputs (the engine's own stored tensors,
exact in bf16) and returns the fp64 result BEFORE the output rounding together with the stage's derived bound, which they share
with the kernel tests (tests/diar_stage_ref.py, tests/gemm_ref.py).
"""
from __future__ import annotations

import os
import sys
from typing import Callable, Dict, Optional

import numpy as np
import torch

from . import diar_ref as R

_TESTS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests")
if _TESTS not in sys.path:
    sys.path.insert(0, _TESTS)
import diar_stage_ref as SR          # noqa: E402  (tests/: the fp64 stage references and bounds shared with the kernel tests)
import gemm_ref as GR                # noqa: E402
from util import bf16_round          # noqa: E402

SINC_K, SINC_STRIDE = 251, 10
EPS = 1e-5
JITTER = 2.0 ** -20                  # the size of an fp32 summation-order difference in a sum of ~ 100 terms


def bf16_trunc(x):
    """float32 -> bfloat16 by dropping the low 16 bits (round toward zero) -> float32: the mutant's rounding"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    return (x.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32).reshape(x.shape)


class Storage:
    """The rounding of every stored tensor: 'bf16' (RNE), 'trunc' (mutant), 'none' (fp64 oracle).  jitter_seed: every value is
    multiplied by 1 +- 2^-20 (random sign per element) before it is rounded, which moves the values that sit next to a tie the
    way another fp32 summation order would.  Weights are converted once at load from given fp32 values (no sum, no order):
    they are rounded without jitter.  hook (optional): called as hook(name, stored) -> stored on every activation, for mutants."""

    def __init__(self, storage: str = "bf16", jitter_seed: Optional[int] = None, hook: Optional[Callable] = None):
        if storage not in ("bf16", "trunc", "none"):
            raise ValueError("storage must be 'bf16', 'trunc' or 'none'")
        self.storage = storage
        self.rng = np.random.default_rng(jitter_seed) if jitter_seed is not None else None
        self.hook = hook

    def weight(self, w):
        w = np.asarray(w, np.float64)
        if self.storage == "none":
            return w
        return (bf16_round(w) if self.storage == "bf16" else bf16_trunc(w)).astype(np.float64)

    def __call__(self, name: str, x):
        x = np.asarray(x, np.float64)
        if self.storage != "none":
            if self.rng is not None:
                x = x * (1.0 + JITTER * (2.0 * self.rng.integers(0, 2, x.shape) - 1.0))
            x = (bf16_round(x) if self.storage == "bf16" else bf16_trunc(x)).astype(np.float64)
        if self.hook is not None:
            x = self.hook(name, x)
        return x


def _np(sd, k):
    v = sd[k]
    return (v.detach().numpy() if isinstance(v, torch.Tensor) else np.asarray(v))


def dims(window_samples: int = R.WINDOW):
    """frames per window after each step: f1 sinc frames, p1 pooled, f2 conv 2 frames, p2, f3, p3 (15975, 5325, 5321, 1773, 1769, 589)"""
    f1 = (window_samples - SINC_K) // SINC_STRIDE + 1
    p1 = f1 // 3
    f2 = p1 - 4
    p2 = f2 // 3
    f3 = p2 - 4
    return dict(f1=f1, p1=p1, f2=f2, p2=p2, f3=f3, p3=f3 // 3)


# ------------------------------------------------------------------------------------ stages
def sinc_filter_bank(sd):
    """-> (filt fp64 [80][251], fsum fp64 [80]): the oracle's filters (fp32, as the engine's) and their sums rounded to fp32 as
    diar_engine.hip:180-184 keeps them"""
    filt = R.sinc_filters(torch.as_tensor(_np(sd, "sincnet.conv1d.0.filterbank.low_hz_")).float(),
                          torch.as_tensor(_np(sd, "sincnet.conv1d.0.filterbank.band_hz_")).float())[:, 0].numpy().astype(np.float64)
    return filt, filt.sum(1).astype(np.float32).astype(np.float64)


def sinc_raw(filt, wave, n_frames=None):
    """fp64 sinc convolution of a waveform [S] (un-normalised), stride 10 -> [n_frames][80], before any rounding"""
    wave = np.asarray(wave, np.float64).reshape(-1)
    n = (wave.shape[0] - SINC_K) // SINC_STRIDE + 1 if n_frames is None else n_frames
    out = np.empty((n, filt.shape[0]))
    for t0 in range(0, n, 16384):
        t1 = min(n, t0 + 16384)
        idx = np.arange(t0, t1)[:, None] * SINC_STRIDE + np.arange(SINC_K)[None, :]
        out[t0:t1] = wave[idx] @ filt.T
    return out


def window_stats(wav):
    """wav [W][S] -> fp64 [W][2] = (mean, 1 / sqrt(biased var + eps)): the waveform's instance norm"""
    wav = np.asarray(wav, np.float64)
    mean = wav.mean(1)
    var = ((wav - mean[:, None]) ** 2).mean(1)
    return np.stack([mean, 1.0 / np.sqrt(var + EPS)], 1)


def first_block(sd, wav, craw, frame0=0, fstep=None, win=None, dtype=SR.BF16, details=None, stats=None, fsum=None):
    """First SincNet block from the waveform windows wav [W][S] (for the instance-norm statistics) and the STORED raw sinc
    convolution craw [rows][80] (window w from row frame0 + (win[w] or w) * fstep; fstep None: f1 rows per window, back to back):
    |a craw + (b - a mean) fsum| -> max-pool 3 -> instance norm -> leaky relu.  -> (a1 fp64 [W][p1][80] before rounding, bound); details: see
    diar_stage_ref.pool_norm_ref.  stats [W][2], fsum [80] (optional): the checked run's own stored window statistics and filter
    sums (fp32), which the kernel takes as given, instead of the fp64 values computed here from wav and the oracle's filters."""
    W = wav.shape[0]
    f1 = (wav.shape[1] - SINC_K) // SINC_STRIDE + 1
    if fsum is None:
        _, fsum = sinc_filter_bank(sd)
    return SR.pool_norm_ref(dtype, True, None, W, f1, craw.shape[1], craw.shape[1],
                            _np(sd, "sincnet.norm1d.0.weight"), _np(sd, "sincnet.norm1d.0.bias"), EPS, craw=craw, frame0=frame0,
                            fstep=f1 if fstep is None else fstep, stats=window_stats(wav) if stats is None else np.asarray(stats, np.float64),
                            fsum=np.asarray(fsum, np.float64),
                            wn_gamma=float(_np(sd, "sincnet.wav_norm1d.weight")[0]), wn_beta=float(_np(sd, "sincnet.wav_norm1d.bias")[0]),
                            win=win, details=details)


def conv_stage(x, W, rows_in, weight, bias):
    """SincNet conv 2 / 3 on a stored activation x [W * rows_in][ld] (ld = 80, or 64 with pad channels 60..63): window w's frames
    0 .. rows_in - 5.  weight [60][cin][5] as stored (rounded), bias fp32.  -> (fp64 [W][rows_in - 4][60] before rounding, bound)."""
    M = rows_in - 4
    refs, tols = [], []
    for w in range(W):
        r, t = SR.conv1d5_ref(x[w * rows_in:(w + 1) * rows_in], weight, bias, M, x.shape[1])
        refs.append(r)
        tols.append(t)
    return np.stack(refs), np.stack(tols)


def pool_norm_stage(x, W, rows_in, frames_in, gamma, beta, dtype=SR.BF16):
    """Later SincNet blocks on a stored conv output x [W * rows_in][ld]: window w's rows w * rows_in .. + frames_in.
    -> (fp64 [W][frames_in // 3][60] before rounding, bound)."""
    C = gamma.shape[0]
    return SR.pool_norm_ref(dtype, False, x, W, frames_in, C, x.shape[1], gamma, beta, EPS, rows_in=rows_in)


def lstm_weights(sd, layer, st: Storage):
    """-> w_ih [2][4H][in], w_hh [2][4H][H] (as stored), b_ih, b_hh [2][4H] (fp32) of one layer, forward | reverse"""
    ks = [("lstm.%s_l%d%s" % (n, layer, suf)) for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh") for suf in ("", "_reverse")]
    a = [_np(sd, k) for k in ks]
    return (np.stack([st.weight(a[0]), st.weight(a[1])]), np.stack([st.weight(a[2]), st.weight(a[3])]),
            np.stack(a[4:6]).astype(np.float64), np.stack(a[6:8]).astype(np.float64))


def lstm_stage(x, W, T, w_ih, w_hh, b_ih, b_hh, st: Optional[Storage] = None, fed_back=None):
    """One bidirectional LSTM layer on a stored input x [W * T][in] (pad columns beyond w_ih's width are ignored); xproj and
    every h_t go through st (default: bf16 RNE, as tests/test_diar_kernels_gpu.py test_lstm_layer).  -> [W * T][2H], rounded at
    the stage's own points: h feeds back, so there is no 'before rounding'.  Its bound is measured, not derived:
    diar_stage_ref.LSTM_BF16_MAX / LSTM_BF16_MEAN per direction.  fed_back: the checked run's stored output [W * T][2H], whose
    h_{t-1} -- a stored input of step t like any other -- then enters every step's gates (diar_stage_ref.lstm_ref)."""
    st = st or Storage("bf16")
    return SR.lstm_ref(SR.BF16, x[:, :w_ih.shape[2]], W, T, w_ih, w_hh, b_ih, b_hh, store=st, fed_back=fed_back)


def linear_stage(x, weight, bias):
    """leaky_relu(x W^T + b) on a stored input x [M][in], weight as stored, bias fp32 -> (fp64 [M][out] before rounding, bound of
    the GEMM with bf16 output: tests/gemm_ref.py bound())."""
    M, K = x.shape
    case = dict(form="linear", dtype=GR.BF16, M=M, N=weight.shape[0], K=K, lda=K, ldw=K, ldc=weight.shape[0], a_row0=0, alpha=1.0,
                act=GR.ACT_LRELU, out="bf16", in_fp8=False, inplace=False, A=np.ascontiguousarray(x).reshape(-1),
                W=np.asarray(weight), bias=np.asarray(bias), res=None, ldres=0)
    return GR.reference(case), GR.bound(case)


def classifier_stage(x, weight, bias):
    """log_softmax(x Wc^T + bc) on a stored input x [M][in]; weights and bias fp32 -> (logp fp64 [M][C], bound [M][1])"""
    logp, tol, _ = SR.classifier_ref(x, weight, bias)
    return logp, tol


# ------------------------------------------------------------------------------------ the network
def pyannet_bf16(sd, wav, taps: Optional[dict] = None, storage: str = "bf16", jitter_seed: Optional[int] = None, hook=None, craw=None):
    """PyanNet.forward as the bf16 engine stores it: wav (B,1,S) torch / numpy -> log-probabilities fp64 numpy [B][589][7].
    storage 'none' is the fp64 oracle, 'trunc' truncates at the same points (a mutant); jitter_seed: see Storage.
    taps (dict): every stored tensor by name -- craw a1 c2 a2 c3 a3 xproj<l> h<l> l<i> -- plus 'sincnet' [B][589][60] and 'lstm'
    [B][589][2H] as diar_ref.pyannet gives them.  craw (optional): sinc_raw of every window [B][f1][80], unrounded, to save
    recomputing it over runs that differ in storage or jitter only.  hook: see Storage (mutants); hook('w_ih<l>', w) is also
    called on every layer's stored W_ih [2][4H][in] and hook('lstm_out<l>', x) on every layer's whole output [B * 589][2H]."""
    st = Storage(storage, jitter_seed, hook)
    wav = (wav.detach().numpy() if isinstance(wav, torch.Tensor) else np.asarray(wav)).astype(np.float64)
    wav = wav.reshape(wav.shape[0], -1)
    B = wav.shape[0]
    d = dims(wav.shape[1])
    T = {} if taps is None else taps
    filt, _ = sinc_filter_bank(sd)
    if craw is None:
        craw = np.stack([sinc_raw(filt, wav[w]) for w in range(B)])
    T["craw"] = st("craw", craw).reshape(B * d["f1"], -1)
    y, _ = first_block(sd, wav, T["craw"])
    T["a1"] = x = st("a1", y).reshape(B * d["p1"], -1)
    rows = d["p1"]
    for i in (1, 2):
        w = st.weight(_np(sd, "sincnet.conv1d.%d.weight" % i))
        y, _ = conv_stage(x, B, rows, w, _np(sd, "sincnet.conv1d.%d.bias" % i))
        T["c%d" % (i + 1)] = x = st("c%d" % (i + 1), y).reshape(B * (rows - 4), -1)
        y, _ = pool_norm_stage(x, B, rows - 4, rows - 4, _np(sd, "sincnet.norm1d.%d.weight" % i), _np(sd, "sincnet.norm1d.%d.bias" % i))
        rows = (rows - 4) // 3
        T["a%d" % (i + 1)] = x = st("a%d" % (i + 1), y).reshape(B * rows, -1)
    T["sincnet"] = x.reshape(B, rows, -1).copy()
    layer = 0
    while "lstm.weight_ih_l%d" % layer in sd:
        w_ih, w_hh, b_ih, b_hh = lstm_weights(sd, layer, st)
        if hook is not None:
            w_ih = hook("w_ih%d" % layer, w_ih)
        x = lstm_stage(x, B, rows, w_ih, w_hh, b_ih, b_hh,
                       st=lambda name, v, l=layer: st("xproj%d" % l if name == "xproj" else "h%d" % l, v))
        if hook is not None:
            x = hook("lstm_out%d" % layer, x)
        T["h%d" % layer] = x
        layer += 1
    T["lstm"] = x.reshape(B, rows, -1).copy()
    i = 0
    while "linear.%d.weight" % i in sd:
        y, _ = linear_stage(x, st.weight(_np(sd, "linear.%d.weight" % i)), _np(sd, "linear.%d.bias" % i))
        T["l%d" % i] = x = st("l%d" % i, y)
        i += 1
    logp, _ = classifier_stage(x, _np(sd, "classifier.weight"), _np(sd, "classifier.bias"))
    return logp.reshape(B, rows, -1)


# ------------------------------------------------------------------------------------ the six metrics
MARGIN = 0.1
COUNTS = ("argmax_diff", "argmax_diff_confident")
MEANS = ("mean_abs_dp", "sincnet_mean_rel")


def metrics(logp, sinc, ref_logp, ref_sinc) -> Dict[str, float]:
    """A run (logp [B][T][C], its 'sincnet' tap) against the fp32 oracle's: frames; frames whose oracle top-2 margin (in
    log-probability) exceeds 0.1 ('confident'); argmax differences among all / among the confident frames; mean |p - q| over
    frames and classes; mean |tap - ref| / mean |ref| of the SincNet tap."""
    logp, ref_logp = np.asarray(logp, np.float64), np.asarray(ref_logp, np.float64)
    q = np.exp(ref_logp)
    srt = np.sort(ref_logp, -1)
    conf = srt[..., -1] - srt[..., -2] > MARGIN
    diff = logp.argmax(-1) != ref_logp.argmax(-1)
    ref_sinc = np.asarray(ref_sinc, np.float64)
    return dict(frames=int(diff.size), confident=int(conf.sum()), argmax_diff=int(diff.sum()),
                argmax_diff_confident=int((diff & conf).sum()), mean_abs_dp=float(np.abs(np.exp(logp) - q).mean()),
                sincnet_mean_rel=float(np.abs(np.asarray(sinc, np.float64) - ref_sinc).mean() / np.abs(ref_sinc).mean()))


def outside_yardstick(m, yard, factor=1.25, floor=4):
    """-> list of the metrics of m that exceed the bound: counts <= factor * yardstick + floor frames, means <= factor * yardstick"""
    bad = [k for k in COUNTS if m[k] > factor * yard[k] + floor]
    return bad + [k for k in MEANS if m[k] > factor * yard[k]]
