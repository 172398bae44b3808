"""Stage-by-stage check of a bf16 run of the conformer encoder on its OWN stored tensors, and the small model the check runs on.
Every stage's stored input, exact in bf16 or fp32, goes through the fp64 stage function of oracle/asr_bf16_ref.py, and the stored
output must lie inside that stage's derived bound (the kernel tests' bounds: tests/gemm_ref.py, tests/attention_ref.py, and for the
row kernels the fp32 tolerance of their kernel tests plus the output's bf16 half ulp).  Used on the engine's tensors
(tests/test_asr_bf16_gpu.py, through Engine.encoder_tap) and, without a GPU, on the restatement's own tensors and on mutants of
them (tests/test_asr_bf16_ref.py).  Nothing here needs a GPU.

Every row is checked, valid and masked alike: the engine computes every row of a chunk (queries beyond the valid length attend the
valid keys; the depthwise convolution reads the GLU of the pointwise bias for frames beyond it), so the restatement defines them all."""
import numpy as np

from oracle import asr_bf16_ref as A
from reverb_amd import synth

MODEL = "forms64"
CHUNK_FRAMES = 603                 # T2 = 150: two full 64-key tiles and a partial one
LENS = (603, 335)                  # encoder lengths 150 and 83: chunk 1's masked keys lie inside a tile, its halo frames are masked
CAT = (1.0, 0.0)
BLOCK_STAGES = ("h_ffm", "x_ffm", "xn_mha", "qkv", "ao", "x_att", "xn_conv", "glu", "dconv", "xn_cnn", "x_conv", "xn_ff", "y", "h_ff",
                "x_ff", "x_out", "next")
FRONT_STAGES = ("X1", "X2", "x0", "xn0")
GEMM_ORDER = ("ffm1", "ffm2", "qkv", "att_out", "pw1", "pw2", "lsl", "ff1", "ff2")


def small_case(seed=0, cnn_module_norm="layer_norm", lens=LENS):
    """-> (cfg, sd, feats [B][603][80] fp32, lens): the small model of MODEL with weight seed `seed`, on the synthetic audio's fbank"""
    from oracle import fbank_ref
    cfg = synth.make_config(MODEL, cnn_module_norm)
    sd = synth.make_state_dict(cfg, seed, synth.CTC_GAMMA, synth.CTC_BLANK_BIAS[("small", 0)])
    fb = fbank_ref.fbank(synth.synth_audio(0.01 * (CHUNK_FRAMES * len(lens)) + 0.5))
    feats = np.zeros((len(lens), CHUNK_FRAMES, 80), np.float32)
    for b, n in enumerate(lens):
        feats[b, :n] = fb[b * CHUNK_FRAMES:b * CHUNK_FRAMES + n]
    return cfg, sd, feats, np.asarray(lens, np.int32)


def forms_of(cfg, lens, T0=CHUNK_FRAMES):
    """the forms the engine must choose for this batch (CPU restatement of its conditions) as check_stages takes them"""
    D = A.dims(cfg, T0)
    return A.expected_forms(cfg, len(lens) * D["T2"], D["T2"])


def decode_forms(raw, is_lsl):
    """Engine.encoder_tap('forms') of a block -> dict(prefold, glu_fused, gemm2 = {name: bool})"""
    names = [n for n in GEMM_ORDER if n != "lsl" or is_lsl]
    assert len(raw) == 2 + len(names), "forms tap: %r" % (raw,)
    return dict(prefold=bool(raw[0]), glu_fused=bool(raw[1]), gemm2={n: v == 2 for n, v in zip(names, raw[2:])})


def check_stages(sd, cfg, feats, lens, T, block, forms, W=None):
    """T: the stored tensors of one position by the engine's tap names (block: x_in xn_ffm ... next, pos_keys; front end: X1 X2 x0
    xn0); block = 0 .. blocks - 1, or `blocks` for the front end; forms: dict(prefold, glu_fused) -- what ran.
    -> (figures, failures): per stage the worst |err| / bound, and one message per stage outside its bound."""
    feats = np.asarray(feats, np.float64)
    D = A.dims(cfg, feats.shape[1])
    d, T2, heads, K, nb = D["d"], D["T2"], D["heads"], D["K"], D["blocks"]
    le = A.enc_lens(lens)
    W = W or A.load_weights(sd, cfg, CAT, T2)
    fig, bad = {}, []

    def within(name, got, ref_tol):
        ref, tol = ref_tol
        got = np.asarray(got, np.float64).reshape(ref.shape)
        r = np.abs(got - ref) / tol
        r = np.where(np.isnan(r), np.inf, r)
        fig[name] = float(r.max())
        if r.max() > 1.0:
            bad.append("%s: %d of %d elements outside the bound, worst %.3g x the bound" % (name, int((r > 1).sum()), r.size, r.max()))

    if block == nb:
        within("X1", T["X1"], A.conv1(W, feats))
        within("X2", T["X2"], A.conv2(W, np.asarray(T["X1"], np.float32)))
        within("x0", T["x0"], A.embed(W, np.asarray(T["X2"], np.float64), d))
        within("xn0", T["xn0"], A.norm(T["x0"], W["blocks"][0]["norm_ff_macaron"]))
        return fig, bad
    L = dict(W["blocks"][block])
    if "pos_keys" in T:          # the engine's own table, as loaded (a stored input of the qkv GEMM and of the attention kernel)
        L["pos_keys"] = np.asarray(T["pos_keys"], np.float64)
    f64 = lambda n: np.asarray(T[n], np.float64)      # noqa: E731
    f1, f2 = A.ffn(f64("xn_ffm"), L["ffm1"], L["ffm2"], f64("x_in"))
    within("h_ffm", T["h_ffm"], f1())
    within("x_ffm", T["x_ffm"], f2(f64("h_ffm")))
    within("xn_mha", T["xn_mha"], A.norm(f64("x_ffm"), L["norm_mha"]))
    within("qkv", T["qkv"], A.qkv(L, f64("xn_mha"), T2, forms["prefold"]))
    within("ao", T["ao"], A.attention(L, f64("qkv"), le, T2, heads, forms["prefold"]))
    within("x_att", T["x_att"], A.att_out(L, f64("ao"), f64("x_ffm")))
    within("xn_conv", T["xn_conv"], A.norm(f64("x_att"), L["norm_conv"]))
    within("glu", T["glu"], A.pw1_glu(L, f64("xn_conv"), forms["glu_fused"]))
    within("dconv", T["dconv"], A.dwconv(L, f64("glu"), le, T2, K, forms["glu_fused"]))
    within("xn_cnn", T["xn_cnn"], A.cnn_norm(L, f64("dconv")))
    within("x_conv", T["x_conv"], A.pw2(L, f64("xn_cnn"), f64("x_att")))
    within("xn_ff", T["xn_ff"], A.norm(f64("x_conv"), L["norm_ff"]))
    ffin = f64("xn_ff")
    if L["is_lsl"]:
        within("y", T["y"], A.lsl(L, ffin))
        ffin = f64("y")
    f1, f2 = A.ffn(ffin, L["ff1"], L["ff2"], f64("x_conv"))
    within("h_ff", T["h_ff"], f1())
    within("x_ff", T["x_ff"], f2(f64("h_ff")))
    nxt = W["blocks"][block + 1]["norm_ff_macaron"] if block + 1 < nb else W["after"]
    xo, nx = A.norm_final(L, f64("x_ff"), f64("y") if L["is_lsl"] else None, nxt)
    within("x_out", T["x_out"], xo)
    within("next", T["next"], nx)
    return fig, bad
