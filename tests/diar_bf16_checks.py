"""Stage-by-stage check of a bf16 run of the segmentation network on its OWN stored tensors: every stage's stored input, exact in
bf16, goes through the fp64 stage function of oracle/diar_bf16_ref.py, and the stored output must lie inside that stage's derived
bound (the kernel tests' bound, tests/diar_stage_ref.py and tests/gemm_ref.py, which already contains the output's bf16 half
ulp).  Used on the engine's tensors (tests/test_diar_bf16_gpu.py, through DiarEngine.tap) and, without a GPU, on the
restatement's own and on mutants of them (tests/test_diar_bf16_ref.py).  Nothing here needs a GPU.

The first block is checked from the stored raw sinc convolution (craw) and the two small fp32 inputs the kernel takes as given,
as its kernel test does: the window statistics and the filter sums, the run's own when it stored them (the engine's "stats" and
"fsum" taps), else the fp64 values computed from the waveform and the oracle's filters (the restatement's own tensors)."""
import numpy as np

import diar_stage_ref as SR
from oracle import diar_bf16_ref as B

U32 = SR.U32
STAGES = ("block1", "conv2", "pool_norm2", "conv3", "pool_norm3", "lstm_last", "linear0", "linear1", "classifier")


def _err(got, ref):
    return np.abs(np.asarray(got, np.float64) - ref)


def check_stages(sd, wav, T, frame0=0, fstep=None, win=None, stages=STAGES):
    """sd: the state dict; wav [W][S] the windows' samples (for the waveform statistics); T: the stored tensors --
      craw [rows][80] (window w from row frame0 + (win[w] or w) * fstep), stats [W][2] and fsum [80] (optional, fp32), a1 [W][p1][80], c2 [W][r2][>= 60] (r2 >= f2 rows per window),
      a2 [W][p2][>= 60], c3 [W][r3][>= 60], a3 [W][589][>= 60], lstm_prev / lstm [W][589][2H], linear0 / linear1 [W][589][D], logp [W][589][C].
    -> (figures, failures): per stage the worst |err| / bound ratio (LSTM: max and mean |err| per direction), and a list of
    messages, one per stage outside its bound or tensor with non-zero pad columns.  Callers assert that the list is empty."""
    W = wav.shape[0]
    d = B.dims(wav.shape[1])
    st = B.Storage("bf16")
    fig, bad = {}, []

    def within(name, got, ref, tol):
        r = _err(got, ref) / tol
        fig[name] = float(r.max())
        if r.max() > 1.0:
            bad.append("%s: %d of %d elements outside the bound, worst %.3g x the bound" % (name, int((r > 1).sum()), r.size, r.max()))

    def pads(name, C):
        # of a conv output only the rows the network reads: a window's last 4 rows run on into the next window or the buffer's slack
        t = T[name][:, :d["f2"]] if name == "c2" else T[name][:, :d["f3"]] if name == "c3" else T[name]
        if t.shape[-1] > C and np.any(t[..., C:] != 0):
            bad.append("%s: pad columns %d.. not zero" % (name, C))

    C = B._np(sd, "sincnet.norm1d.1.weight").shape[0]
    if "block1" in stages:
        y, tol = B.first_block(sd, wav, T["craw"], frame0, fstep, win, stats=T.get("stats"), fsum=T.get("fsum"))
        within("block1", T["a1"], y, tol)
    if "conv2" in stages:
        w2 = st.weight(B._np(sd, "sincnet.conv1d.1.weight"))
        y, tol = B.conv_stage(T["a1"].reshape(W * d["p1"], -1), W, d["p1"], w2, B._np(sd, "sincnet.conv1d.1.bias"))
        within("conv2", T["c2"][:, :d["f2"], :C], y, tol)
    if "pool_norm2" in stages:
        r2 = T["c2"].shape[1]
        y, tol = B.pool_norm_stage(T["c2"].reshape(W * r2, -1), W, r2, d["f2"], B._np(sd, "sincnet.norm1d.1.weight"),
                                   B._np(sd, "sincnet.norm1d.1.bias"))
        within("pool_norm2", T["a2"][..., :C], y, tol)
    if "conv3" in stages:
        w3 = st.weight(B._np(sd, "sincnet.conv1d.2.weight"))
        y, tol = B.conv_stage(T["a2"].reshape(W * d["p2"], -1), W, d["p2"], w3, B._np(sd, "sincnet.conv1d.2.bias"))
        within("conv3", T["c3"][:, :d["f3"], :C], y, tol)
    if "pool_norm3" in stages:
        r3 = T["c3"].shape[1]
        y, tol = B.pool_norm_stage(T["c3"].reshape(W * r3, -1), W, r3, d["f3"], B._np(sd, "sincnet.norm1d.2.weight"),
                                   B._np(sd, "sincnet.norm1d.2.bias"))
        within("pool_norm3", T["a3"][..., :C], y, tol)
    for name in ("c2", "a2", "c3", "a3"):
        if name in T:
            pads(name, C)
    layers = 0
    while "lstm.weight_ih_l%d" % layers in sd:
        layers += 1
    H2 = T["lstm"].shape[-1]
    if "lstm_last" in stages:
        # The layer's stored inputs are the previous layer's output AND its own h_{t-1}, which the kernel stores (rounded once) and
        # reads back: both are fed to the fp64 layer exactly as stored, so each of the 589 steps is checked from the engine's own
        # tensors.  ('free': the same reference fed its OWN h_{t-1} instead, reported only -- there one rounding that falls the
        # other way is carried on by the recurrence, on reference and kernel alike.)
        xin, got = T["lstm_prev"].reshape(W * d["p3"], -1), T["lstm"].reshape(W * d["p3"], H2)
        wts = B.lstm_weights(sd, layers - 1, st)
        for tag, ref in (("", B.lstm_stage(xin, W, d["p3"], *wts, fed_back=got)), ("free_", B.lstm_stage(xin, W, d["p3"], *wts))):
            e = _err(got, ref)
            for k, nm in ((0, "forward"), (1, "reverse")):
                ek = e[:, k * (H2 // 2):(k + 1) * (H2 // 2)]
                fig["lstm_last_%s%s_max" % (tag, nm)], fig["lstm_last_%s%s_mean" % (tag, nm)] = float(ek.max()), float(ek.mean())
                if not tag and not (ek.max() < SR.LSTM_BF16_MAX and ek.mean() < SR.LSTM_BF16_MEAN):
                    bad.append("lstm_last %s: max |err| %.3g (bound %.3g), mean %.3g (bound %.3g)" % (nm, ek.max(), SR.LSTM_BF16_MAX,
                                                                                                 ek.mean(), SR.LSTM_BF16_MEAN))
    x = T["lstm"].reshape(W * d["p3"], H2)
    for i in (0, 1):
        if "linear%d" % i in stages:
            y, tol = B.linear_stage(x, st.weight(B._np(sd, "linear.%d.weight" % i)), B._np(sd, "linear.%d.bias" % i))
            within("linear%d" % i, T["linear%d" % i].reshape(y.shape), y, tol)
        x = T["linear%d" % i].reshape(W * d["p3"], -1)
    if "classifier" in stages:
        y, tol = B.classifier_stage(x, B._np(sd, "classifier.weight"), B._np(sd, "classifier.bias"))
        within("classifier", T["logp"].reshape(y.shape), y, tol)
    return fig, bad
