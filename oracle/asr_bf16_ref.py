"""TEST INFRASTRUCTURE ONLY (oracle) -- never imported by the product path.

A restatement of oracle/model_ref.py's offline encoder_forward + ctc_logprobs in fp64 arithmetic that rounds to bf16 (round to
nearest even, tests/util.py bf16_round: fp64 -> fp32 -> bf16, the engine's accumulators being fp32) exactly where the bf16 engine
stores or feeds bf16, and nowhere else.  It is the yardstick of what bf16 STORAGE costs the conformer encoder: the engine's distance
from the fp32 oracle is held to this restatement's distance from it (tests/test_asr_bf16_gpu.py, fixture
tests/golden/asr_bf16_yardstick.json written by oracle/gen_golden_asr_bf16.py), and every stage of the engine, run on the engine's
own stored inputs, to the stage functions below (tests/asr_bf16_checks.py on the taps of rvb_get_encoder_tap).

Storage points, read from encode_impl and encoder_layer (reverb_amd/csrc/engine_encode.hip, E: below) and finalize_impl
(csrc/engine_weights.hip, W:).  "epilogue" = the GEMM's one conversion of its fp32 accumulator (gemm.hip:167, gemm2.hip's epilogues).

  tensor (tap)         stored by                                                     read by
  X1                   conv1 + ReLU, E:353 (subsample_conv1, conv_s2.hip)            E:367 conv2 (implicit GEMM)
  X2                   conv2 + ReLU epilogue, E:367                                  E:371 embed_out
  xn0 / xn_ffm         LayerNorm norm_ff_macaron of block 0, E:375; of block i + 1:  E:71 ffm1
                       the second output of block i's final norm, E:240 ("next")
  h_ffm, h_ff          SiLU epilogue, E:71 / E:231                                   E:74 / E:234 w_2
  xn_mha               E:82                                                          E:92 / E:94 qkv
  qkv                  epilogue E:94; pre-folded E:92: the K third is k + p          E:135 attention (q, K' or k, v)
                       (p: pos_keys row of the frame, bf16) in ONE rounding,
                       gemm.hip:165-167 / GemmArgs::rowadd
  ao                   attention.hip:409-410 (pack2_bf16 of o / l), E:135            E:138 linear_out
  xn_conv              E:146                                                         E:162 / E:164 pointwise_conv1
  glu                  fused (E:162, ACT_GLU): ONE rounding of a * sigmoid(b);       E:183 depthwise convolution
                       un-fused (E:164): a | b, each rounded, and the kernel
                       rounds the gate once more into LDS (elementwise.hip:404,489)
  dconv                depthwise output, elementwise.hip:569 (out_bf16, E:177)       E:209 conv-module norm (x_bf16)
  xn_cnn               norm (LayerNorm or folded BatchNorm) + SiLU, E:209            E:212 pointwise_conv2
  xn_ff                E:221                                                         E:225 language mix, or E:231 w_1
  y                    language-specific blocks: epilogue E:225                      E:231 w_1, and E:240 (added after norm_final)
  next / enc_out       E:240: LayerNorm (next block's norm_ff_macaron, or            next block's E:71; E:387 CTC head (enc_out)
                       after_norm) of the fp32 x_out IN REGISTERS
  weights              rounded ONCE from fp32 at load (pack_T, W:13-22, convert_f32): conv2 (W:222), embed_out (W:232), ctc (W:236),
                       ffm1 ffm2 ff1 ff2 qkv att_out pw1 pw2 (W:256-262, 276), the interleaved pw1_glu copy (W:273: the same values in
                       another order), the language mix (W:92-111: mixed in fp32 on the host, then rounded once)
  pos_keys             a rounded GEMM RESULT: bf16 sinusoid table (W:246) x bf16 linear_pos weights, epilogue W:315-316
  inside attn_kernel   register operands the bf16 MFMA takes (attention.hip): (q + u) * log2e / sqrt(dk) :150, (q + v) * .. :151
                       (two-product form only), the probabilities before P.V :362-365; masked-frame fill of the depthwise
                       kernel: bf16 of GLU(pointwise bias), elementwise.hip:484,489

Not rounded: the fp32 residual stream x (every x_* tap) and x_out; biases and norm parameters; bias_u / bias_v; the fp32 pos_bias
table (v - u) . p (W:320-322); CMVN; conv1's weights (fp32: conv1_w.as<float>(), E:354) and the depthwise weights; the logits and the
log-softmax (E:387-389).
NOT modelled, being arithmetic and not storage: the hardware exp2 / rcp of SiLU, the GLU gate and the softmax, the fp32 summation
orders of the MFMA chains and reductions, the online softmax's rescaling, fp32 rsqrt of the norms.  Their size is what the stage
bounds allow beside the output's half ulp, and what the jittered yardstick runs sample.

Masked rows: the engine computes every row of a chunk (q_len = T2 for every chunk, E:276; keys beyond the valid length are masked;
the depthwise convolution reads the bias's gate for frames beyond it) and does not zero the convolution module's output there as
the oracle does (convolution.py:141): rows beyond a chunk's valid length differ from the oracle's from the first block on, never
reach a valid row, and are DEFINED here as the engine computes them.  The metrics use valid frames only.
"""
from __future__ import annotations

import math
import os
import sys
from typing import Dict, Optional

import numpy as np
import torch

from . import model_ref as M
from .diar_bf16_ref import Storage, bf16_trunc      # noqa: F401  (one Storage for both restatements)

_TESTS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests")
if _TESTS not in sys.path:
    sys.path.insert(0, _TESTS)
import attention_ref as AR           # noqa: E402  (tests/: the fp64 references and bounds shared with the kernel tests)
import elementwise_ref as EW         # noqa: E402
import gemm_ref as GR                # noqa: E402
from util import bf16_round, f32     # noqa: E402

U32, UB = GR.U32, GR.UB
EPS = 1e-5
FORMS_DEFAULT = dict(prefold=True, glu_fused=True)
MUTANTS = ("trunc", "trunc_dconv", "kp_twice", "glu_halves", "next_from_rounded", "p_before_max")


def _np(sd, k):
    v = sd[k]
    return (v.detach().numpy() if isinstance(v, torch.Tensor) else np.asarray(v))


def dims(cfg, T0):
    ec = cfg["encoder_conf"]
    d, F0 = ec["output_size"], cfg["input_dim"]
    T1, F1 = (T0 - 3) // 2 + 1, (F0 - 3) // 2 + 1
    T2, F2 = (T1 - 3) // 2 + 1, (F1 - 3) // 2 + 1
    return dict(d=d, heads=ec["attention_heads"], dk=d // ec["attention_heads"], ff=ec["linear_units"], blocks=ec["num_blocks"],
                K=ec["cnn_module_kernel"], V=cfg["output_dim"], F0=F0, T0=T0, T1=T1, F1=F1, T2=T2, F2=F2)


def enc_lens(lens):
    """mask[:, :, 2::2][:, :, 2::2] (subsampling.py:226): frames 6 + 4 j < len"""
    lens = np.asarray(lens, np.int64)
    return np.where(lens > 6, (lens - 7) // 4 + 1, 0).astype(np.int32)


def expected_forms(cfg, M_rows, T2, dtype_bf16=True):
    """What encoder_layer chooses for a bf16 offline batch of M_rows rows (engine_encode.hip `prefold`, gemm_glu_supported,
    gemm2_applicable), computed on the CPU: -> dict(prefold, glu_fused, gemm2 = {name: bool})."""
    D = dims(cfg, 7)
    d, ff, dk = D["d"], D["ff"], D["dk"]
    prefold = dtype_bf16 and 32 < dk <= 64 and T2 <= 16384 and d % 8 == 0

    def g2(N, K, act=GR.ACT_NONE):
        return GR.gemm2_applicable(dict(dtype=GR.BF16, M=M_rows, N=N, K=K, lda=K, ldw=K, act=act))
    # csrc/gemm2.hip gemm_glu_supported: gemm2 applies, N % 16 == 0, the output rows (ldc = d) are whole 16-byte vectors
    glu = dtype_bf16 and g2(2 * d, d) and (2 * d) % 16 == 0 and d % 8 == 0
    return dict(prefold=prefold, glu_fused=glu,
                gemm2=dict(ffm1=g2(ff, d, GR.ACT_SILU), ffm2=g2(d, ff), qkv=g2(3 * d, d), att_out=g2(d, d), pw1=g2(2 * d, d), pw2=g2(d, d),
                           lsl=g2(d, d), ff1=g2(ff, d, GR.ACT_SILU), ff2=g2(d, ff)))


# ------------------------------------------------------------------------------------ weights as the engine keeps them
def load_weights(sd, cfg, cat_embs, T2, st: Optional[Storage] = None):
    """-> dict of everything finalize_impl packs (engine_weights.hip:193-329), fp64 arrays holding the stored values: GEMM weights
    through st.weight (one rounding from fp32), biases / norm parameters / conv1 / depthwise weights / bias_u / bias_v as fp32.
    pos_keys [T2][d] per block is a GEMM OUTPUT (rounded table x rounded weights, rounded once more: st('pos_keys', .))."""
    st = st or Storage("bf16")
    D = dims(cfg, 7)
    d, F2, nb = D["d"], D["F2"], D["blocks"]
    g = lambda k: _np(sd, k).astype(np.float64)     # noqa: E731
    W = dict(mean=g("encoder.global_cmvn.mean"), istd=g("encoder.global_cmvn.istd"),
             conv1_w=g("encoder.embed.conv.0.weight"), conv1_b=g("encoder.embed.conv.0.bias"),
             # conv2 [co][ci][kh][kw] -> [co][(kh * 3 + kw) * d + ci]; out.0 [o][c * F2 + f] -> [o][f * d + c] (engine_weights.hip:215-232)
             conv2_w=st.weight(_np(sd, "encoder.embed.conv.2.weight").transpose(0, 2, 3, 1).reshape(d, 9 * d)),
             conv2_b=g("encoder.embed.conv.2.bias"),
             embed_w=st.weight(_np(sd, "encoder.embed.out.0.weight").reshape(d, d, F2).transpose(0, 2, 1).reshape(d, F2 * d)),
             embed_b=g("encoder.embed.out.0.bias"),
             after=(g("encoder.after_norm.weight"), g("encoder.after_norm.bias")),
             ctc_w=st.weight(_np(sd, "ctc.ctc_lo.weight")), ctc_b=g("ctc.ctc_lo.bias"), blocks=[])
    pe = st.weight(M.sinusoid_pe(T2, d).numpy())
    cat = np.asarray(cat_embs, np.float32)
    norm = cfg["encoder_conf"].get("cnn_module_norm", "batch_norm")
    for i in range(nb):
        p = "encoder.encoders.%d" % i
        lin = lambda n: (st.weight(_np(sd, p + n + ".weight").reshape(_np(sd, p + n + ".weight").shape[0], -1)), g(p + n + ".bias"))   # noqa: E731
        L = dict(ffm1=lin(".feed_forward_macaron.w_1"), ffm2=lin(".feed_forward_macaron.w_2"), ff1=lin(".feed_forward.w_1"),
                 ff2=lin(".feed_forward.w_2"), att_out=lin(".self_attn.linear_out"), pw1=lin(".conv_module.pointwise_conv1"),
                 pw2=lin(".conv_module.pointwise_conv2"))
        L["qkv"] = (st.weight(np.concatenate([_np(sd, p + ".self_attn.linear_%s.weight" % n) for n in "qkv"])),
                    np.concatenate([g(p + ".self_attn.linear_%s.bias" % n) for n in "qkv"]))
        L["bias_u"], L["bias_v"] = g(p + ".self_attn.pos_bias_u").reshape(-1), g(p + ".self_attn.pos_bias_v").reshape(-1)
        L["dw_w"], L["dw_b"] = g(p + ".conv_module.depthwise_conv.weight")[:, 0, :], g(p + ".conv_module.depthwise_conv.bias")
        for n in ("norm_ff_macaron", "norm_mha", "norm_conv", "norm_ff", "norm_final"):
            L[n] = (g("%s.%s.weight" % (p, n)), g("%s.%s.bias" % (p, n)))
        cn = p + ".conv_module.norm"
        if norm == "layer_norm":
            L["cnn_norm"], L["cnn_mode"] = (g(cn + ".weight"), g(cn + ".bias")), EW.NORM_LN
        else:      # BatchNorm1d (eval) folded on the host in fp32 (engine_weights.hip:297-309)
            gg = f32(f32(_np(sd, cn + ".weight")) / np.sqrt(f32(f32(_np(sd, cn + ".running_var")) + np.float32(1e-5))))
            bb = f32(f32(_np(sd, cn + ".bias")) - f32(f32(_np(sd, cn + ".running_mean")) * gg))
            L["cnn_norm"], L["cnn_mode"] = (gg.astype(np.float64), bb.astype(np.float64)), EW.NORM_AFFINE
        L["is_lsl"] = (p + ".language_layers.0.weight") in sd
        if L["is_lsl"]:       # W = sum_i c_i W_i folded on the host in fp32 (pack_lsl, engine_weights.hip:92-111), then rounded once
            w = b = None
            for j in range(len(cat)):
                tw, tb = f32(_np(sd, "%s.language_layers.%d.weight" % (p, j))), f32(_np(sd, "%s.language_layers.%d.bias" % (p, j)))
                w, b = (f32(cat[j] * tw), f32(cat[j] * tb)) if w is None else (f32(w + f32(cat[j] * tw)), f32(b + f32(cat[j] * tb)))
            L["lsl"] = (st.weight(w), b.astype(np.float64))
        wpos = st.weight(_np(sd, p + ".self_attn.linear_pos.weight"))
        L["pos_keys"] = st("pos_keys", pe @ wpos.T)
        W["blocks"].append(L)
    return W


# ------------------------------------------------------------------------------------ bounds of the row kernels
def _out_bf16(ref, b):
    """+ the one rounding of the output to bf16: half a unit in the last place, taken at |ref| + the arithmetic error (gemm_ref.bound)"""
    return b + GR.bf16_half_ulp(np.abs(ref) + b)


def _norm_bound(ref, out_bf16, gain=1.0):
    """rownorm's arithmetic is fp32 whatever it stores: its error is what tests/test_elementwise_kernels_gpu.py holds the fp32 output
    to (rtol 1e-5 + atol 4e-5, _assert_kind), times `gain` where a second pass amplifies it; a bf16 output adds its one rounding."""
    b = gain * (1e-5 * np.abs(ref) + 4e-5)
    return _out_bf16(ref, b) if out_bf16 else b + 1e-30


def _near_tie(v32):
    """fp32 values within 2^-20 (relative) of the middle between two bf16 neighbours: a last-bit difference of the fp32 arithmetic
    that produced them can send their rounding the other way"""
    u = np.ascontiguousarray(v32, np.float32).view(np.uint32) & np.uint32(0xFFFF)
    return np.abs(u.astype(np.int64) - 0x8000) <= 8


# ------------------------------------------------------------------------------------ stages: stored inputs -> (fp64 result, bound)
WANT_BOUNDS = True      # encoder_bf16 switches the GEMM stages' bounds off while it runs (it uses the results only): at r640's shapes they
#                         cost twice the GEMMs themselves


def _gemm(A, W, bias, act=GR.ACT_NONE, alpha=1.0, res=None, out="bf16", rowadd=None):
    A = np.ascontiguousarray(A)
    Mr, K = A.shape
    case = dict(form="asr", dtype=GR.BF16, M=Mr, N=W.shape[0], K=K, lda=K, ldw=K, ldc=W.shape[0], a_row0=0, alpha=float(alpha), act=act,
                out=out, in_fp8=False, inplace=res is not None, A=A.reshape(-1), W=np.asarray(W), bias=np.asarray(bias),
                res=None if res is None else np.asarray(res), ldres=0 if res is None else W.shape[0])
    if rowadd is not None:
        case["rowadd"] = rowadd
    return GR.reference(case), (GR.bound(case) if WANT_BOUNDS else None)


def conv1(W, feats):
    """CMVN + Conv2d(1, d, 3, 2) + ReLU on the fp32 features (conv1's weights are fp32: conv1_w.as<float>()) -> X1 [B][T1][F1][d].
    Bound: the fp32 tolerance of test_conv1_cmvn (rtol 2e-5, atol 8e-5) + the output's bf16 rounding."""
    y = EW.conv1(feats, W["mean"], W["istd"], W["conv1_w"], W["conv1_b"])
    return y, _out_bf16(y, 2e-5 * np.abs(y) + 8e-5)


def conv2(W, X1):
    """Conv2d(d, d, 3, 2) + ReLU as the implicit GEMM the engine runs on the stored X1 [B][T1][F1][d] -> X2 rows [B * T2 * F2][d]"""
    B, T1, F1, d = X1.shape
    T2, F2 = (T1 - 3) // 2 + 1, (F1 - 3) // 2 + 1
    A = np.empty((B, T2, F2, 9, d), np.float32)
    for kh in range(3):
        for kw in range(3):
            A[:, :, :, kh * 3 + kw] = X1[:, kh:kh + 2 * T2 - 1:2, kw:kw + 2 * F2 - 1:2]
    return _gemm(A.reshape(B * T2 * F2, 9 * d), W["conv2_w"], W["conv2_b"], act=GR.ACT_RELU)


def embed(W, X2, d):
    """linear(X2 as [M][F2 * d]) * sqrt(d) -> the fp32 residual stream x0 [M][d]"""
    return _gemm(X2.reshape(-1, W["embed_w"].shape[1]), W["embed_w"], W["embed_b"], alpha=math.sqrt(d), out="f32")


def norm(x, gb, mode=EW.NORM_LN, silu=False):
    """a LayerNorm (or the folded BatchNorm, then SiLU: cnn_norm) of stored rows -> the bf16 operand xn of the next GEMM"""
    y, _ = EW.rownorm(x, gb[0], gb[1], EPS, mode, silu)
    return y, _norm_bound(y, True, 1.1 if silu else 1.0)


def cnn_norm(L, dconv):
    return norm(dconv, L["cnn_norm"], L["cnn_mode"], True)


def ffn(xn, w1, w2, x):
    """one feed-forward module in its two stored steps; returns a function pair so that each runs on stored inputs:
    h = SiLU(xn W1^T + b1) (bf16), x' = x + 0.5 (h W2^T + b2) (fp32, in place)"""
    return (lambda: _gemm(xn, w1[0], w1[1], act=GR.ACT_SILU)), (lambda h: _gemm(h, w2[0], w2[1], alpha=0.5, res=x, out="f32"))


def qkv(L, xn, T2, prefold):
    """the fused q | k | v projection; prefold: the K third is stored as k + p (p = the block's positional keys of the row's frame,
    GemmArgs::rowadd) in ONE rounding"""
    d = xn.shape[1]
    ra = dict(add=L["pos_keys"][:T2], col0=d) if prefold else None
    return _gemm(xn, L["qkv"][0], L["qkv"][1], rowadd=ra)


def attn_case(L, qkv_st, lens_enc, T2, heads, prefold):
    d = qkv_st.shape[1] // 3
    B = len(lens_enc)
    start = (np.arange(B) * T2).astype(np.int32)
    return dict(dtype=AR.BF16, heads=heads, dk=d // heads, nseq=B, q_len=np.full(B, T2, np.int32), kv_len=np.asarray(lens_enc, np.int32),
                q_start=start, kv_start=start, causal=False, q_pos0=np.zeros(B, np.int32), chunk=0, left=-1, pos=True, p_off=0,
                kv_index=None, q=qkv_st[:, :d], k=qkv_st[:, d:2 * d], v=qkv_st[:, 2 * d:], p=L["pos_keys"][:T2], bu=f32(L["bias_u"]),
                bv=f32(L["bias_v"]), k_prefolded=bool(prefold))


def attention(L, qkv_st, lens_enc, T2, heads, prefold):
    """rel-pos attention of the stored qkv buffer (queries: all T2 rows of a chunk; keys: its valid frames) -> (ao fp64, bound)"""
    ref, bnd, _ = AR._ref_bound(attn_case(L, qkv_st, lens_enc, T2, heads, prefold))
    return ref, bnd


def attention_stored(L, qkv_st, lens_enc, T2, heads, prefold, st: Storage, mut=None):
    """what the kernel stores: the emulation of its register roundings (attention_ref._emulate), each through st"""
    rq = None if st.storage == "bf16" and st.rng is None and st.hook is None else (lambda x: st("attn_reg", f32(x)))
    if st.storage == "none":
        return attention(L, qkv_st, lens_enc, T2, heads, prefold)[0]
    return AR._emulate(attn_case(L, qkv_st, lens_enc, T2, heads, prefold), mut=mut, rq=rq)


def att_out(L, ao, x):
    return _gemm(ao, L["att_out"][0], L["att_out"][1], res=x, out="f32")


def pw1_glu(L, xn, fused):
    """pointwise_conv1 (+ GLU in the epilogue when fused: ONE rounding of a * sigmoid(b); else the two halves a | b [M][2d], each
    rounded).  Fused bound: the accumulation errors e_a, e_b of both columns (gemm_ref.bound's first term) through the gate
    (sigmoid <= 1, |a| sigmoid' <= |a| / 4), the fast sigmoid (exp2 and rcp at EXP_MEASURED each, the argument's rounding), the
    product, and the output's rounding."""
    w, b = L["pw1"]
    if not fused:
        return _gemm(xn, w, b)
    d = w.shape[0] // 2
    A = np.asarray(xn, np.float64)
    pre = A @ w.T + b
    if not WANT_BOUNDS:
        return pre[:, :d] / (1.0 + np.exp(-pre[:, d:])), None
    e = 1.1 * (2 * A.shape[1] + 8) * U32 * (np.abs(A) @ np.abs(w).T + np.abs(b))
    a, g = pre[:, :d], pre[:, d:]
    sg = 1.0 / (1.0 + np.exp(-g))
    y = a * sg
    bnd = e[:, :d] * sg + 0.25 * np.abs(a) * e[:, d:] + (4.0 * AR.EXP_MEASURED[AR.BF16] + (np.abs(g) + 4.0) * U32) * np.abs(y)
    return y, _out_bf16(y, bnd) + 1e-30


def glu_gate_bf16(L, st: Optional[Storage] = None):
    """the gated value of a masked frame as the depthwise kernel stages it: GLU of the pointwise bias in fp32, kept in bf16 in LDS
    (elementwise.hip Gate<bf16_t>::put) -> (stored fp64 [d], near_tie [d])"""
    pb = f32(L["pw1"][1])
    d = pb.shape[0] // 2
    v = f32(pb[:d] / f32(np.float32(1.0) + f32(np.exp(f32(-pb[d:])))))
    stored = bf16_round(v).astype(np.float64) if st is None else st("glu_fill", v)
    return stored, _near_tie(v)


def dwconv(L, glu_st, lens_enc, T2, K, fused, fill=None):
    """the depthwise convolution on the stored GLU output [M][d] (fused) or the stored halves [M][2d] (the kernel gates them in
    fp32 with its fast sigmoid and keeps the gate in bf16 in LDS: a third rounding, modelled here as round-to-nearest of the fp64 gate).
    Frames at and beyond a chunk's valid length are the bf16 gate of the pointwise bias.  -> (dconv fp64 [M][d], bound): an fp32 FMA
    chain of K taps and the bias, 2 (K + 1) u32 sum|w g| + |b|; the output's rounding; un-fused, one bf16 ulp (2^-8) of every gate
    (test_glu_dwconv's bound); and a bf16 ulp of the fill value on the channels where its fp32 value sits next to a tie."""
    B = len(lens_enc)
    G = np.asarray(glu_st, np.float64).reshape(B, T2, -1)
    d = L["dw_w"].shape[0]
    if not fused:
        G = bf16_round(G[..., :d] / (1.0 + np.exp(-G[..., d:]))).astype(np.float64)
    fv, tie = glu_gate_bf16(L) if fill is None else fill
    filled = np.arange(T2)[None, :] >= np.asarray(lens_enc)[:, None]
    frames = np.where(filled[..., None], fv, G)
    y = EW.dwconv(frames, L["dw_w"], L["dw_b"], K)
    mag = EW.dwconv(np.abs(frames), np.abs(L["dw_w"]), None, K) + np.abs(L["dw_b"])
    b = 2 * (K + 1) * U32 * mag
    if not fused:
        b = b + 2.0 ** -8 * EW.dwconv(np.abs(frames) * ~filled[..., None], np.abs(L["dw_w"]), None, K)
    b = b + 2.0 ** -8 * EW.dwconv(np.abs(frames) * (filled[..., None] & tie), np.abs(L["dw_w"]), None, K)
    return y.reshape(B * T2, d), _out_bf16(y, b).reshape(B * T2, d) + 1e-30


def pw2(L, xn, x):
    return _gemm(xn, L["pw2"][0], L["pw2"][1], res=x, out="f32")


def lsl(L, xn):
    """the language-specific mix y = xn Wmix^T + bmix (bf16), which feeds the feed-forward and is added after norm_final"""
    return _gemm(xn, L["lsl"][0], L["lsl"][1])


def norm_final(L, x, y, nxt):
    """x_out = LayerNorm(x) (+ y) kept in fp32, and in the same pass next = LayerNorm(x_out; the next block's norm_ff_macaron or
    after_norm) stored in bf16 -- from the fp32 x_out in registers, not from a stored value.  -> (x_out, bound), (next, bound): the second
    norm passes x_out's error on with gain |gamma2| rstd2 (<= twice the single-pass error where that gain is below 1)."""
    out, out2 = EW.rownorm(x, L["norm_final"][0], L["norm_final"][1], EPS, add=y, gamma2=nxt[0], beta2=nxt[1], eps2=EPS)
    rstd2 = 1.0 / np.sqrt(out.var(1, keepdims=True) + EPS)
    gain = 1.0 + np.maximum(1.0, np.abs(nxt[0])[None, :] * rstd2)
    return (out, _norm_bound(out, False)), (out2, _norm_bound(out2, True, gain))


def ctc(W, enc, blank_penalty=0.0, blank_id=0):
    """log_softmax(enc Wctc^T + b) of the stored encoder output; logits and log-probabilities stay fp32 -> (logp fp64, bound [M][1]):
    a log-softmax moves by at most twice the largest logit error of its row, plus the fp32 evaluation (the exponentials at EXP_REL,
    the sum of V terms, the logarithm, the subtraction)."""
    z, bz = _gemm(enc, W["ctc_w"], W["ctc_b"], out="f32")
    z = z.copy()
    z[:, blank_id] -= blank_penalty
    m = z.max(1, keepdims=True)
    lse = m + np.log(np.exp(z - m).sum(1, keepdims=True))
    if bz is None:
        return z - lse, None
    tol = 2 * bz.max(1, keepdims=True) + 2 * AR.EXP_REL[AR.BF16] + (z.shape[1] + 8) * U32 + 4 * U32 * (np.abs(z).max(1, keepdims=True) + np.abs(lse))
    return z - lse, tol


# ------------------------------------------------------------------------------------ the network
def encoder_bf16(sd, cfg, feats, lens, cat_embs=(1.0, 0.0), taps: Optional[dict] = None, storage: str = "bf16",
                 jitter_seed: Optional[int] = None, hook=None, forms: Optional[dict] = None, mutant: Optional[str] = None,
                 blank_penalty: float = 0.0):
    """encoder_forward + ctc_logprobs as the bf16 engine stores them: feats [B][T0][80] fp32, lens [B] -> (encoder_out fp64
    [B][T2][d], logp fp64 [B][T2][V]).  storage 'none' is the fp64 oracle, 'trunc' truncates at the same points; jitter_seed, hook:
    see Storage.  forms: dict(prefold, glu_fused) -- the form the engine ran.  taps (dict): every stored tensor, front end by name
    (X1 X2 x0 xn0), blocks as taps[block][name] with the engine's tap names.  mutant: one of MUTANTS (a deliberately wrong engine):
      trunc_dconv        dconv alone is truncated
      kp_twice           pre-folded key: k is stored, then k + p is stored (two roundings)
      glu_halves         fused GLU: both halves are rounded, then gated and rounded (three roundings)
      next_from_rounded  norm_final's second LayerNorm reads x_out rounded to bf16 instead of the fp32 one
      p_before_max       attention: the probabilities are rounded before the row maximum is subtracted"""
    global WANT_BOUNDS
    keep, WANT_BOUNDS = WANT_BOUNDS, False
    try:
        return _encoder_bf16(sd, cfg, feats, lens, cat_embs, taps, storage, jitter_seed, hook, forms, mutant, blank_penalty)
    finally:
        WANT_BOUNDS = keep


def _encoder_bf16(sd, cfg, feats, lens, cat_embs, taps, storage, jitter_seed, hook, forms, mutant, blank_penalty):
    fm = dict(FORMS_DEFAULT)
    fm.update(forms or {})
    st = Storage("trunc" if mutant == "trunc" else storage, jitter_seed, hook)
    feats = (feats.detach().numpy() if isinstance(feats, torch.Tensor) else np.asarray(feats)).astype(np.float64)
    B, T0 = feats.shape[:2]
    D = dims(cfg, T0)
    d, T2, heads, K = D["d"], D["T2"], D["heads"], D["K"]
    le = enc_lens(lens)
    W = load_weights(sd, cfg, cat_embs, T2, st)
    T = {} if taps is None else taps
    rnd1 = (lambda v: v) if st.storage == "none" else (lambda v: bf16_round(v).astype(np.float64))
    T["X1"] = X1 = st("X1", conv1(W, feats)[0])
    T["X2"] = X2 = st("X2", conv2(W, f32(X1))[0])
    T["x0"] = x = embed(W, X2, d)[0]
    T["xn0"] = xn = st("xn", norm(x, W["blocks"][0]["norm_ff_macaron"])[0])
    for i, L in enumerate(W["blocks"]):
        t = T[i] = {"x_in": x, "xn_ffm": xn, "pos_keys": L["pos_keys"]}
        f1, f2 = ffn(xn, L["ffm1"], L["ffm2"], x)
        t["h_ffm"] = h = st("h", f1()[0])
        t["x_ffm"] = x = f2(h)[0]
        t["xn_mha"] = xn = st("xn", norm(x, L["norm_mha"])[0])
        if mutant == "kp_twice" and fm["prefold"]:
            y = st("qkv", qkv(L, xn, T2, False)[0])
            y[:, d:2 * d] = st("qkv", y[:, d:2 * d] + np.tile(L["pos_keys"][:T2], (B, 1)))
            t["qkv"] = y
        else:
            t["qkv"] = y = st("qkv", qkv(L, xn, T2, fm["prefold"])[0])
        t["ao"] = ao = attention_stored(L, y, le, T2, heads, fm["prefold"], st, "p_before_max" if mutant == "p_before_max" else None)
        t["x_att"] = x = att_out(L, ao, x)[0]
        t["xn_conv"] = xn = st("xn", norm(x, L["norm_conv"])[0])
        if mutant == "glu_halves" and fm["glu_fused"]:
            ab = st("glu", pw1_glu(L, xn, False)[0])
            g = st("glu", ab[:, :d] / (1.0 + np.exp(-ab[:, d:])))
        else:
            g = st("glu", pw1_glu(L, xn, fm["glu_fused"])[0])
        t["glu"] = g
        fill = None if st.storage == "bf16" and st.rng is None else (glu_gate_bf16(L, st)[0] if st.storage != "none" else
                                                                     L["pw1"][1][:d] / (1.0 + np.exp(-L["pw1"][1][d:])), np.zeros(d, bool))
        if st.storage == "none" and not fm["glu_fused"]:
            g = g[:, :d] / (1.0 + np.exp(-g[:, d:]))
        y = dwconv(L, g, le, T2, K, fm["glu_fused"] or st.storage == "none", fill)[0]
        t["dconv"] = dc = bf16_trunc(y).astype(np.float64) if mutant == "trunc_dconv" else st("dconv", y)
        t["xn_cnn"] = xn = st("xn", cnn_norm(L, dc)[0])
        t["x_conv"] = x = pw2(L, xn, x)[0]
        t["xn_ff"] = xn = st("xn", norm(x, L["norm_ff"])[0])
        yl = None
        if L["is_lsl"]:
            t["y"] = yl = xn = st("y", lsl(L, xn)[0])
        f1, f2 = ffn(xn, L["ff1"], L["ff2"], x)
        t["h_ff"] = h = st("h", f1()[0])
        t["x_ff"] = x = f2(h)[0]
        nxt = W["blocks"][i + 1]["norm_ff_macaron"] if i + 1 < len(W["blocks"]) else W["after"]
        (xo, _), (nx, _) = norm_final(L, x, yl, nxt)
        if mutant == "next_from_rounded":
            nx = EW.layer_norm(rnd1(xo), nxt[0], nxt[1], EPS)
        t["x_out"] = x = xo
        t["next"] = xn = st("xn", nx)
    T["enc_out"] = xn
    logp, _ = ctc(W, xn, blank_penalty, cfg["ctc_conf"]["ctc_blank_id"])
    return xn.reshape(B, T2, d), logp.reshape(B, T2, -1)


def oracle_fp32(sd, cfg, feats, lens, cat_embs=(1.0, 0.0)):
    """oracle/model_ref.py on the same weights and features -> (encoder_out [B][T2][d], logp [B][T2][V]) as fp64 numpy"""
    tsd = M.to_torch_sd(sd)
    with torch.no_grad():
        enc, _ = M.encoder_forward(tsd, cfg, torch.as_tensor(np.asarray(feats, np.float32)), torch.as_tensor(np.asarray(lens)).long(),
                                   torch.tensor(list(cat_embs), dtype=torch.float32))
        logp = M.ctc_logprobs(tsd, enc)
    return enc.numpy().astype(np.float64), logp.numpy().astype(np.float64)


# ------------------------------------------------------------------------------------ the six metrics
MARGIN = 0.1
COUNTS = ("argmax_diff", "argmax_diff_confident")
MEANS = ("mean_abs_dlogp", "max_abs_dlogp_confident", "enc_rel_l2", "enc_one_minus_cos")


def golden_arrays(ref_enc, ref_logp, t_step=1, d_step=1):
    """what the metrics need of the fp32 oracle, small enough to commit for a big model: per frame the top-1 label, its
    log-probability and the top-2 margin, and encoder_out sampled every t_step frames and d_step channels"""
    ref_logp = np.asarray(ref_logp, np.float64)
    srt = np.sort(ref_logp, -1)
    return dict(argmax=ref_logp.argmax(-1).astype(np.int32), top1=srt[..., -1].astype(np.float32),
                gap=(srt[..., -1] - srt[..., -2]).astype(np.float32), enc_sample=np.asarray(ref_enc)[:, ::t_step, ::d_step].astype(np.float32),
                steps=np.array([t_step, d_step], np.int32))


def metrics_golden(enc, logp, g, lens) -> Dict[str, float]:
    """metrics() against golden_arrays of the oracle (encoder_out figures over the sampled frames and channels)"""
    le = enc_lens(lens)
    B, T2 = g["argmax"].shape
    ts, ds = (int(v) for v in g["steps"])
    valid = np.arange(T2)[None, :] < le[:, None]
    logp = np.asarray(logp, np.float64)
    top = g["argmax"].astype(np.int64)
    diff = (logp.argmax(-1) != top)[valid]
    conf = (g["gap"] > MARGIN)[valid]
    dl = np.abs(np.take_along_axis(logp, top[..., None], 2)[..., 0] - g["top1"].astype(np.float64))[valid]
    vs = valid[:, ::ts]
    a, b = np.asarray(enc, np.float64)[:, ::ts, ::ds][vs].ravel(), g["enc_sample"].astype(np.float64)[vs].ravel()
    return dict(frames=int(valid.sum()), confident=int(conf.sum()), argmax_diff=int(diff.sum()), argmax_diff_confident=int((diff & conf).sum()),
                mean_abs_dlogp=float(dl.mean()), max_abs_dlogp_confident=float(dl[conf].max()) if conf.any() else 0.0,
                enc_rel_l2=float(np.linalg.norm(a - b) / np.linalg.norm(b)),
                enc_one_minus_cos=float(1.0 - (a @ b) / (np.linalg.norm(a) * np.linalg.norm(b))))


def metrics(enc, logp, ref_enc, ref_logp, lens) -> Dict[str, float]:
    """A run against the fp32 oracle's, over the valid frames (t < encoder length of the chunk): frames whose CTC argmax differs;
    those among the frames the oracle decides with a top-2 margin above 0.1 ('confident', RefBf16.frame_disagreement's
    definition); mean |delta log p| of the oracle's top-1 label; its maximum over the confident frames; relative L2 error and
    1 - cosine of encoder_out."""
    le = enc_lens(lens)
    B, T2 = logp.shape[:2]
    valid = np.arange(T2)[None, :] < le[:, None]
    ref_logp, logp = np.asarray(ref_logp, np.float64)[valid], np.asarray(logp, np.float64)[valid]
    a, b = np.asarray(enc, np.float64)[valid].ravel(), np.asarray(ref_enc, np.float64)[valid].ravel()
    srt = np.sort(ref_logp, -1)
    conf = srt[:, -1] - srt[:, -2] > MARGIN
    top = ref_logp.argmax(-1)
    diff = logp.argmax(-1) != top
    dl = np.abs(np.take_along_axis(logp, top[:, None], 1) - np.take_along_axis(ref_logp, top[:, None], 1))[:, 0]
    return dict(frames=int(valid.sum()), confident=int(conf.sum()), argmax_diff=int(diff.sum()), argmax_diff_confident=int((diff & conf).sum()),
                mean_abs_dlogp=float(dl.mean()), max_abs_dlogp_confident=float(dl[conf].max()) if conf.any() else 0.0,
                enc_rel_l2=float(np.linalg.norm(a - b) / np.linalg.norm(b)),
                enc_one_minus_cos=float(1.0 - (a @ b) / (np.linalg.norm(a) * np.linalg.norm(b))))


ENC_FACTOR = {"enc_rel_l2": 1.05, "enc_one_minus_cos": 1.05 ** 2}


def outside_yardstick(m, yard, factor=1.25, floor=4):
    """-> list of the metrics of m beyond the bound: counts <= factor * yardstick + floor frames, the log-probability figures
    <= factor * yardstick (the diarization precedent's margin: they are decided by a handful of frames, and the seven yardstick runs
    themselves spread by 30 % on them).  The two encoder_out figures are averages over 16 000 to 60 000 values on which the seven runs
    of a case agree within 0.4 % (relative L2; 1.3 % on r640_chunk's sample) and 0.9 % (1 - cosine, its square; 2.6 %): 1.25 there would accept an engine that loses a
    fifth more than storage costs -- the mutant whose final norm feeds the next block from a rounded x_out sits at 1.053 -- so they
    are held to 1.05 (and its square): ten times the small model's spread, four times r640_chunk's.  Chosen from the restatement's runs alone."""
    bad = [k for k in COUNTS if m[k] > factor * yard[k] + floor]
    return bad + [k for k in MEANS if m[k] > ENC_FACTOR.get(k, factor) * yard[k]]
