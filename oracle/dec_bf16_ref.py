"""TEST INFRASTRUCTURE ONLY (oracle) -- never imported by the product path.

A restatement of oracle/model_ref.py's decoder_forward ON A PREFIX TRIE (the batch rvb_attention_rescore and rvb_attention_score run:
one decoder row per distinct prefix of a chunk, csrc/trie.h) in fp64 arithmetic that rounds to bf16 exactly where the bf16 engine
stores or feeds bf16, and nowhere else.  It is the yardstick of what bf16 STORAGE costs the bidirectional attention decoder, and
every stage of the engine, run on the engine's own stored inputs, is held to the stage functions below (tests/dec_bf16_checks.py on
the taps of rvb_get_decoder_tap).  Storage, the GEMM / attention / row-norm references and their bounds are the encoder
restatement's (oracle/asr_bf16_ref.py, tests/gemm_ref.py, tests/attention_ref.py, tests/elementwise_ref.py).

Storage points, read from decoder_forward and decoder_memory_kv (reverb_amd/csrc/engine_decode.hip, D: below) and pack_decoder
(csrc/engine_weights.hip, W:).  "epilogue" = the GEMM's one conversion of its fp32 accumulator.

  tensor (tap)      stored by                                                          read by
  x_emb             embed_tokens (elementwise.hip embed_kernel): E[tok] * sqrt(d) +    the residual stream of layer 0
                    pe[pos], fp32 table and weights, fp32 out
  xn1 xn2 xn3       run_norm of the fp32 residual stream dx, bf16 out (e->dxn)         qkv / src_q / the language mix or ff1
  qkv               epilogue of self_qkv, [R][3d] (e->dqkv)                            self attention: q, k, v at stride 3d
  ao_self           attention.hip (pack2_bf16 of o / l): the 16-query trie form,       self_out
                    causal, keys through kv_index (the hypothesis' path), q_pos0
  x_self x_src x_ff the in-place residual GEMMs self_out / src_out / ff2 on the        the next norm
                    fp32 dx: NOT rounded
  q                 epilogue of src_q (e->dq)                                          cross attention
  kvmem             epilogue of src_kv on the stored encoder output (bf16 enc_out),    cross attention: k, v at stride 2d
                    [M][2d]; rvb_prepare_rescoring or the call itself
  ao_src            attention.hip: one query sequence per chunk over the chunk's       src_out
                    valid frames, not causal
  y                 language-specific layers: epilogue of the language mix (e->dy)     ff1
  h                 epilogue of ff1 after ReLU (e->dh)                                 ff2
  xn_after          run_norm after_norm (eps 1e-5)                                     the output layer
  logits, logp      fp32: the output GEMM's fp32 epilogue (rows of Vld = (V + 3) & ~3), lse_gather_multi / row_xent
  weights           rounded ONCE from fp32 at load (pack_T, W:13-22): self_qkv (q | k | v concatenated), self_out, src_q, src_kv
                    (k | v), src_out, ff1, ff2, output_layer, and the language mix (pack_lsl, W:92-111: W = sum_i c_i W_i mixed in
                    fp32 on the host, then rounded once)
  inside attention  the register operands the bf16 MFMA takes (attention_ref._emulate): q * log2e / sqrt(dk), the probabilities

Not rounded: embed (fp32, D.embed.as<float>()), pe_f32, biases, norm parameters, the residual stream, the logits, the log-softmax.
LayerNorm eps: norm1 / norm2 / norm3 of a language-specific layer 1e-12, of a plain layer 1e-5 (W:176, `L.is_lsl ? 1e-12f : 1e-5f`:
decoder_layer.py:241-243 vs :56-58); after_norm 1e-5 (W:169).
NOT modelled, being arithmetic and not storage: as in asr_bf16_ref (exp2 / rcp, fp32 summation orders, the online softmax).

Bounds.  GEMM stages: gemm_ref.bound (in-place residual: res = the stored dx; every A here is dense, lda = K -- the strided operands
are the attention's).  Attentions: attention_ref._ref_bound.  Row norms: asr_bf16_ref._norm_bound.  logp: what
tests/test_rowlse_kernels_gpu.py holds lse_gather_multi / row_xent to, 3e-6 max(1, M / 16), M = max(|lse|, max |logp|) of the row,
against the fp64 log-softmax of the stored fp32 logits.  x_emb, derived here from its three operations (u32 = 2^-24):
  * the product e * sqrt(d) and the sum with p each round once (or once together, fused): <= 2 u32 (|e| sqrt(d) + |p|) taken at 3 to
    cover sqrt(d) itself rounded to fp32;
  * the table: entry (pos, i) is sin or cos of the fp32 angle pos * div_i, div_i = expf(i c), c = -ln(10000) / d.  The engine's libm
    and the restatement's (torch, as the reference) may differ by one unit in the last place in expf and in sin / cos, and the argument
    i c rounds once: the angle moves by at most pos div_i (|i c| + 4) u32 and the value by that (|sin'| <= 1) plus 2 u32.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

from . import asr_bf16_ref as A
from . import model_ref as M
from .asr_bf16_ref import AR, EW, GR, Storage, _np, f32

U32 = GR.U32
EPS, EPS_LSL = 1e-5, 1e-12
LOGP_BOUND = 3e-6          # tests/test_rowlse_kernels_gpu.py BOUND
TRIE_ARRAYS = ("tok", "pos", "path", "hq_start", "hq_len", "hq_pos0", "hkv_start", "hkv_len", "crow_start", "crow_len", "tgt_ptr", "tgt", "work")
SIDES = ("left_decoder", "right_decoder")
LAYER_STAGES = ("xn1", "qkv", "ao_self", "x_self", "xn2", "q", "kvmem", "ao_src", "x_src", "xn3", "y", "h", "x_ff")
HEAD_STAGES = ("xn_after", "logits", "logp")
MUTANTS = ("trunc", "sibling", "causal_plus1", "q_from_xn1", "kv_unrounded_mem", "lang_swapped", "no_relu", "right_unreversed")


def dims(cfg):
    dc = cfg["decoder_conf"]
    d, heads, V = cfg["encoder_conf"]["output_size"], dc["attention_heads"], cfg["output_dim"]
    return dict(d=d, heads=heads, dk=d // heads, ff=dc["linear_units"], layers=dc["num_blocks"], r_layers=dc.get("r_num_blocks", 0), V=V,
                Vld=(V + 3) & ~3)


# ------------------------------------------------------------------------------------ the forms the engine must choose
def expected_forms(cfg, R, position, is_lsl, dtype_bf16=True):
    """What decoder_forward's calls select for R trie rows (gemm()'s gemm2_applicable; attention.hip dispatch_attn: q_block 16 -> one wave
    of 16 queries, no positional keys; the cross attention -> the plain 8-wave form), as the `forms` tap lists them."""
    D = dims(cfg)
    d, ff, dk = D["d"], D["ff"], D["dk"]

    def g(N, K, act=GR.ACT_NONE):
        return 2 if dtype_bf16 and GR.gemm2_applicable(dict(dtype=GR.BF16, M=R, N=N, K=K, lda=K, ldw=K, act=act)) else 1
    if position == D["layers"]:
        return [g(D["V"], d)]
    dkp = next(p for p in (32, 64, 96, 128) if dk <= p)
    att = lambda nw: [2 if dtype_bf16 else 4, dkp, 0, nw, 0, 32, 1, 1]      # noqa: E731
    return [g(3 * d, d)] + att(1) + [g(d, d), g(d, d)] + att(8) + [g(d, d)] + ([g(d, d)] if is_lsl else []) + [g(ff, d, GR.ACT_RELU), g(d, ff)]


# ------------------------------------------------------------------------------------ weights as the engine keeps them
def load_weights(sd, cfg, side, cat_embs, st: Optional[Storage] = None):
    """-> dict of what pack_decoder packs for `side`: GEMM weights through st.weight (one rounding from fp32), embed / biases / norm
    parameters as fp32 values; per layer the eps its three norms run with."""
    st = st or Storage("bf16")
    p = "decoder." + side
    g = lambda k: _np(sd, k).astype(np.float64)     # noqa: E731
    lin = lambda n: (st.weight(_np(sd, n + ".weight")), g(n + ".bias"))       # noqa: E731
    cat = np.asarray(cat_embs, np.float32)
    W = dict(embed=g(p + ".embed.0.weight"), after=(g(p + ".after_norm.weight"), g(p + ".after_norm.bias")), out=lin(p + ".output_layer"),
             layers=[])
    j = 0
    while (p + ".decoders.%d.norm1.weight" % j) in sd:
        q = p + ".decoders.%d" % j
        cc = lambda names: (st.weight(np.concatenate([_np(sd, q + n + ".weight") for n in names])),      # noqa: E731
                            np.concatenate([g(q + n + ".bias") for n in names]))
        L = dict(qkv=cc([".self_attn.linear_q", ".self_attn.linear_k", ".self_attn.linear_v"]), self_out=lin(q + ".self_attn.linear_out"),
                 src_q=lin(q + ".src_attn.linear_q"), src_kv=cc([".src_attn.linear_k", ".src_attn.linear_v"]),
                 src_out=lin(q + ".src_attn.linear_out"), ff1=lin(q + ".feed_forward.w_1"), ff2=lin(q + ".feed_forward.w_2"))
        for n in ("norm1", "norm2", "norm3"):
            L[n] = (g("%s.%s.weight" % (q, n)), g("%s.%s.bias" % (q, n)))
        L["is_lsl"] = (q + ".language_layers.0.weight") in sd
        L["eps"] = EPS_LSL if L["is_lsl"] else EPS
        if L["is_lsl"]:       # mixed in fp32 on the host (pack_lsl), then rounded once
            w = b = None
            for i in range(len(cat)):
                tw, tb = f32(_np(sd, "%s.language_layers.%d.weight" % (q, i))), f32(_np(sd, "%s.language_layers.%d.bias" % (q, i)))
                w, b = (f32(cat[i] * tw), f32(cat[i] * tb)) if w is None else (f32(w + f32(cat[i] * tw)), f32(b + f32(cat[i] * tb)))
            L["lsl"] = (st.weight(w), b.astype(np.float64))
        W["layers"].append(L)
        j += 1
    return W


# ------------------------------------------------------------------------------------ stages: stored inputs -> (fp64 result, bound)
def x_emb(W, trie):
    """E[tok] * sqrt(d) + pe[pos] in fp32 -> (fp64 [R][d], bound): see the docstring"""
    E = W["embed"]
    d = E.shape[1]
    tok, pos = np.asarray(trie["tok"], np.int64), np.asarray(trie["pos"], np.int64)
    pe = M.sinusoid_pe(int(pos.max()) + 1, d).numpy().astype(np.float64)
    y = E[tok] * math.sqrt(d) + pe[pos]
    c = -(math.log(10000.0) / d)
    i = (np.arange(d) // 2 * 2).astype(np.float64)
    ang = pos[:, None] * np.exp(i * c)[None, :] * (np.abs(i * c)[None, :] + 4.0) * U32
    return y, 3 * U32 * (np.abs(E[tok]) * math.sqrt(d) + np.abs(pe[pos])) + 2 * U32 + ang + 1e-30


def norm(x, gb, eps):
    y, _ = EW.rownorm(x, gb[0], gb[1], eps)
    return y, A._norm_bound(y, True)


def gemm(A_, lin, act=GR.ACT_NONE, res=None, out="bf16"):
    return A._gemm(A_, lin[0], lin[1], act=act, res=res, out=out)


def self_attn_case(qkv_st, trie, heads, q_pos0_shift=0, path=None):
    d = qkv_st.shape[1] // 3
    n = len(trie["hq_start"])
    i32 = lambda k: np.asarray(trie[k], np.int32)       # noqa: E731
    return dict(dtype=AR.BF16, heads=heads, dk=d // heads, nseq=n, q_start=i32("hq_start"), q_len=i32("hq_len"), q_pos0=i32("hq_pos0") + q_pos0_shift,
                kv_start=i32("hkv_start"), kv_len=i32("hkv_len"), kv_index=i32("path") if path is None else np.asarray(path, np.int32),
                causal=True, chunk=0, left=-1, pos=False, p_off=0, q=qkv_st[:, :d], k=qkv_st[:, d:2 * d], v=qkv_st[:, 2 * d:])


def src_attn_case(q_st, kvmem_st, trie, enc_lens, T2, heads):
    d = q_st.shape[1]
    B = len(enc_lens)
    return dict(dtype=AR.BF16, heads=heads, dk=d // heads, nseq=B, q_start=np.asarray(trie["crow_start"], np.int32),
                q_len=np.asarray(trie["crow_len"], np.int32), q_pos0=np.zeros(B, np.int32), kv_start=(np.arange(B) * T2).astype(np.int32),
                kv_len=np.asarray(enc_lens, np.int32), kv_index=None, causal=False, chunk=0, left=-1, pos=False, p_off=0, q=q_st,
                k=kvmem_st[:, :d], v=kvmem_st[:, d:])


def attention(case):
    ref, bnd, _ = AR._ref_bound(case)
    return ref, bnd


def _attention_stored(case, st: Storage):
    if st.storage == "none":
        return attention(case)[0]
    rq = None if st.storage == "bf16" and st.rng is None and st.hook is None else (lambda x: st("attn_reg", f32(x)))
    return AR._emulate(case, rq=rq)


def logits(W, xn, V):
    return gemm(xn, W["out"], out="f32")


def logp(lg, trie):
    """fp64 log-softmax of the stored fp32 logits [R][>= V] (pad columns cut by the caller) at every (row, target) of the trie's CSR, in
    slot order -> (logp [P], bound [P])"""
    lg = np.asarray(lg, np.float64)
    m = lg.max(1, keepdims=True)
    lse = (m + np.log(np.exp(lg - m).sum(1, keepdims=True)))[:, 0]
    ptr, tgt = np.asarray(trie["tgt_ptr"], np.int64), np.asarray(trie["tgt"], np.int64)
    rows = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    Mx = np.maximum(np.abs(lse), np.abs(lg - lse[:, None]).max(1))
    return lg[rows, tgt] - lse[rows], (LOGP_BOUND * np.maximum(1.0, Mx / 16.0))[rows]


# ------------------------------------------------------------------------------------ the network
def decoder_bf16(sd, cfg, side, trie, memory, enc_lens, cat_embs=(1.0, 0.0), taps: Optional[dict] = None, storage: str = "bf16",
                 jitter_seed: Optional[int] = None, hook=None, mutant: Optional[str] = None, memory_raw=None):
    """decoder `side` over the trie batch as the bf16 engine stores it: memory [B][T2][d] (the encoder output; stored bf16: rounded
    here through Storage), enc_lens [B] -> (logits fp64 [R][V], logp fp64 [P] in slot order).  taps (dict): taps[layer][name],
    taps[layers][name] for the head, taps["trie"].  mutant: one of MUTANTS (a deliberately wrong decoder; right_unreversed is made by
    the caller, who passes the wrong trie):
      sibling           one key of one hypothesis' path is a sibling branch's row (memory_raw unused)
      causal_plus1      every query sees one key more than the causal mask allows
      q_from_xn1        the cross attention's query projected from xn1 instead of xn2
      kv_unrounded_mem  memory keys / values projected from the un-rounded encoder output (memory_raw)
      lang_swapped      the language mix with the two category weights swapped
      no_relu           h without ReLU"""
    keep, A.WANT_BOUNDS = A.WANT_BOUNDS, False
    try:
        return _decoder_bf16(sd, cfg, side, trie, memory, enc_lens, cat_embs, taps, storage, jitter_seed, hook, mutant, memory_raw)
    finally:
        A.WANT_BOUNDS = keep


def sibling_path(trie):
    """trie['path'] with ONE entry swapped for a sibling's row: a key of the last hypothesis that shares a prefix with an earlier one
    and then diverges -- its first own row's position, read from the earlier hypothesis' branch instead"""
    path = np.array(trie["path"], np.int32)
    pos = np.asarray(trie["pos"])
    for h in range(len(trie["hq_start"]) - 1, -1, -1):
        p0, n = int(trie["hq_pos0"][h]), int(trie["hq_len"][h])
        if n < 2 or p0 < 2:
            continue
        own = int(trie["hq_start"][h])                   # position p0 on this branch
        sib = [r for r in range(len(pos)) if pos[r] == p0 and r != own and _parent(trie, r) == path[trie["hkv_start"][h] + p0 - 1]]
        if sib:
            path[trie["hkv_start"][h] + p0] = sib[0]
            return path
    raise ValueError("no hypothesis with a sibling branch")


def _parent(trie, row):
    for h in range(len(trie["hq_start"])):
        s, n = int(trie["hkv_start"][h]), int(trie["hkv_len"][h])
        seg = list(trie["path"][s:s + n])
        if row in seg:
            k = seg.index(row)
            return seg[k - 1] if k else -1
    return -1


def _decoder_bf16(sd, cfg, side, trie, memory, enc_lens, cat_embs, taps, storage, jitter_seed, hook, mutant, memory_raw):
    st = Storage("trunc" if mutant == "trunc" else storage, jitter_seed, hook)
    D = dims(cfg)
    d, heads, V = D["d"], D["heads"], D["V"]
    cat = tuple(cat_embs)[::-1] if mutant == "lang_swapped" else cat_embs
    W = load_weights(sd, cfg, side, cat, st)
    memory = np.asarray(memory, np.float64)
    B, T2 = memory.shape[:2]
    mem = st("enc_out", memory.reshape(B * T2, d))
    if mutant == "kv_unrounded_mem":
        mem = np.asarray(memory_raw, np.float64).reshape(B * T2, d)
    T = {} if taps is None else taps
    T["trie"] = {k: np.asarray(trie[k], np.int32) for k in TRIE_ARRAYS}
    x = x_emb(W, trie)[0]
    for li, L in enumerate(W["layers"]):
        t = T[li] = {"x_in": x}
        if li == 0:
            t["x_emb"] = x
        t["kvmem"] = kv = st("kvmem", gemm(mem, L["src_kv"])[0])
        t["xn1"] = xn1 = st("xn", norm(x, L["norm1"], L["eps"])[0])
        t["qkv"] = qkv = st("qkv", gemm(xn1, L["qkv"])[0])
        case = self_attn_case(qkv, trie, heads, 1 if mutant == "causal_plus1" else 0, sibling_path(trie) if mutant == "sibling" else None)
        t["ao_self"] = ao = _attention_stored(case, st)
        t["x_self"] = x = gemm(ao, L["self_out"], res=x, out="f32")[0]
        t["xn2"] = xn2 = st("xn", norm(x, L["norm2"], L["eps"])[0])
        t["q"] = q = st("q", gemm(xn1 if mutant == "q_from_xn1" else xn2, L["src_q"])[0])
        t["ao_src"] = ao = _attention_stored(src_attn_case(q, kv, trie, enc_lens, T2, heads), st)
        t["x_src"] = x = gemm(ao, L["src_out"], res=x, out="f32")[0]
        t["xn3"] = z = st("xn", norm(x, L["norm3"], L["eps"])[0])
        if L["is_lsl"]:
            t["y"] = z = st("y", gemm(z, L["lsl"])[0])
        t["h"] = h = st("h", gemm(z, L["ff1"], act=GR.ACT_NONE if mutant == "no_relu" else GR.ACT_RELU)[0])
        t["x_ff"] = x = gemm(h, L["ff2"], res=x, out="f32")[0]
    t = T[len(W["layers"])] = {"x_in": x}
    t["xn_after"] = xn = st("xn", norm(x, W["after"], EPS)[0])
    t["logits"] = lg = logits(W, xn, V)[0]
    t["logp"] = lp = logp(lg, trie)[0]
    return lg, lp
