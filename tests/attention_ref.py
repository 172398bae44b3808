"""CPU side of the attention checks (csrc/attention.hip), shared by tests/test_attention_kernels_gpu.py (the kernel in every form) and
oracle/asr_bf16_ref.py (the bf16 encoder's restatement): plain fp64 softmax attention of the rounded operands, the per-element bound
of the kernel's error that follows from what the kernel rounds, and a numpy emulation of the kernel's rounding points with named
mutants.  Nothing here needs a GPU.

A case is a dict: dtype (F32 / BF16), heads, dk, nseq, q_len, kv_len, q_start, kv_start [nseq], causal, q_pos0, chunk, left, pos,
p_off, kv_index, q [Rq][d], k / v [Rk][d], p [rows][d], bu / bv [d] -- operands as the compute dtype holds them.  With
case["k_prefolded"] set, `k` holds K' = bf16(k + p) as the qkv GEMM's epilogue stored it (GemmArgs::rowadd, attention.hip FOLD 2):
the scores are (q + u).K' + (v - u).p and K' is an exact input, so the bound carries no rounding of the key operand."""
import math

import numpy as np

from util import bf16_round, f32

F32, BF16 = 0, 1
U32 = 2.0 ** -24          # fp32 unit roundoff
UB = 2.0 ** -9            # bf16 unit roundoff (8 significant bits, round to nearest even)
# Relative error of the exponential the kernel calls, the one term of the bound that does not follow from the formats (the ISA text
# gives no figure).  Measured once on an MI355X against fp64 over [-64, 0] (4 M arguments, a third of them within [-2, 0]): the
# hardware exp2 (`__builtin_amdgcn_exp2f`, bf16 path) 1.396 * 2^-24, expf (f32 path) 1.388 * 2^-24; used with a factor 2 margin.
EXP_MEASURED = {BF16: 1.4 * 2.0 ** -24, F32: 1.4 * 2.0 ** -24}
EXP_REL = {t: 2.0 * e for t, e in EXP_MEASURED.items()}


def _rnd(dtype, a):
    return bf16_round(f32(a)) if dtype == BF16 else f32(a)


def _admitted(case, s, i):
    """[lo, hi) of the keys query i of sequence s may see"""
    kl = int(case["kv_len"][s])
    lo, hi = 0, kl
    if case["causal"]:
        hi = min(hi, int(case["q_pos0"][s]) + i + 1)
    cs, left = case["chunk"], case["left"]
    if cs > 0:
        hi = min(hi, (i // cs + 1) * cs)
        if left >= 0:
            lo = max((i // cs - left) * cs, 0)
    return lo, max(hi, lo)


# ------------------------------------------------------------------------------------------------------------------ reference and bound
def _seq_operands(case, s, h, mut=None):
    """fp64 views of one (sequence, head): Q [ql][dk], K, V [kl][dk], P [kl][dk] or None, mask [ql][kl] (True = admitted)"""
    dk = case["dk"]
    sl = slice(h * dk, (h + 1) * dk)
    qs, ql, ks, kl = (int(case[n][s]) for n in ("q_start", "q_len", "kv_start", "kv_len"))
    rows = np.arange(ks, ks + kl) if case["kv_index"] is None else case["kv_index"][ks:ks + kl]
    Q = case["q"][qs:qs + ql, sl].astype(np.float64)
    K = case["k"][rows][:, sl].astype(np.float64)
    vsl = sl
    if mut == "head":          # broken: head h + 1's columns for v
        h2 = (h + 1) % case["heads"]
        vsl = slice(h2 * dk, (h2 + 1) * dk)
    V = case["v"][rows][:, vsl].astype(np.float64)
    P = case["p"][case["p_off"]:case["p_off"] + kl, sl].astype(np.float64) if case["pos"] else None
    mask = np.zeros((ql, kl), bool)
    for i in range(ql):
        lo, hi = _admitted(case, s, i)
        mask[i, lo:hi] = True
    return Q, K, V, P, mask, sl, qs, ql


def _ref_bound(case, fold=False):
    """fp64 softmax attention of the rounded operands, and the per-element bound of the kernel's error.

    What the kernel rounds (u = 2^-9 for bf16, u32 = 2^-24), scores in nats, c = 1 / sqrt(dk):
      * bf16 query operand bf16((q + bias) * log2e * c): the fp32 sum and product and the fp32 constant cost 4 u32, the rounding u, all
        relative to each term; the keys are read as they are.  Two products: the score is an fp32 sum of n = dk (no p) or 2 dk terms,
        |error| <= (n + 2) u32 sum|terms|.  So delta[q, j] = (u + (n + 6) u32) * A[q, j],  A = c * sum_e |(q+u)_e k_e| + |(q+v)_e p_e|.
      * folded: the key operand is bf16(fl(k + p)): another u + u32 on each term of B = c * sum_e |(q+u)_e (k+p)_e|; the per-key
        constant is an fp32 sum of dk terms of (v-u)_e p_e (dk + 2 roundings, one more for the scale) and seeds the accumulator:
        delta = (2 u + u^2 + (dk + 8) u32) * B + (2 dk + 6) u32 * c * sum_e |(v-u)_e p_e|.
        With case["k_prefolded"] the key operand K' is read as stored: delta = (u + (dk + 8) u32) * B' + the same constant term,
        B' = c * sum_e |(q+u)_e K'_e|.
      * f32: no operand rounding: delta = (n + 6) u32 * A (sum, the fp32 biased q, the division by sqrt(dk)).
      * weights: exp2 / expf of (score - running max) has relative error EXP_REL; the subtraction rounds its argument (u32 * range);
        every later tile multiplies numerator and denominator by the SAME factor exp(m_old - m_new), so its error cancels between them
        except for one fp32 rounding each.  Per key: theta = delta + (tiles + 1) (EXP_REL + 2 u32) + u32 * range.
      * the probability is rounded to bf16 (u) for P.V only; P.V and the denominator are fp32 sums over the keys ((kv + 2) u32 each);
        the quotient and the output rounding: u (bf16) or 2 u32 (f32) of |ref|.
    With w = softmax weights:  out = sum w_j (1 + theta_j)(1 + rho_j) v_j / sum w_j (1 + theta_j), hence
      |out - ref| <= (expm1(2 max_j theta) + u_p + (2 kv + 2 tiles + 8) u32) * sum_j w_j |v_j| + (u_out + 3 u32) |ref| + 1e-30."""
    dtype, dk, heads = case["dtype"], case["dk"], case["heads"]
    d = heads * dk
    bf = dtype == BF16
    pre = bool(case.get("k_prefolded"))
    Rq = case["q"].shape[0]
    ref, bound, wts = np.zeros((Rq, d)), np.full((Rq, d), 1e-30), {}
    c = 1.0 / math.sqrt(dk)
    for s in range(case["nseq"]):
        if case["kv_len"][s] == 0 or case["q_len"][s] == 0:
            continue
        for h in range(heads):
            Q, K, V, P, mask, sl, qs, ql = _seq_operands(case, s, h)
            kl = K.shape[0]
            if P is not None:
                bu, bv = case["bu"][sl].astype(np.float64), case["bv"][sl].astype(np.float64)
                Cm = (np.abs(bv - bu) @ np.abs(P).T) * c
                if pre:
                    S = ((Q + bu) @ K.T + ((bv - bu) @ P.T)[None, :]) * c
                    delta = (UB + (dk + 8) * U32) * (np.abs(Q + bu) @ np.abs(K).T) * c + (2 * dk + 6) * U32 * Cm[None, :]
                else:
                    S = ((Q + bu) @ K.T + (Q + bv) @ P.T) * c
                    if fold:
                        B = (np.abs(Q + bu) @ np.abs(K + P).T) * c
                        delta = (2 * UB + UB * UB + (dk + 8) * U32) * B + (2 * dk + 6) * U32 * Cm[None, :]
                    else:
                        A = (np.abs(Q + bu) @ np.abs(K).T + np.abs(Q + bv) @ np.abs(P).T) * c
                        delta = ((UB if bf else 0.0) + (2 * dk + 6) * U32) * A
            else:
                S = (Q @ K.T) * c
                delta = ((UB if bf else 0.0) + (dk + 6) * U32) * (np.abs(Q) @ np.abs(K).T) * c
            S = np.where(mask, S, -np.inf)
            any_key = mask.any(1)
            m = np.where(any_key, S.max(1, initial=-np.inf), 0.0)
            W = np.exp(S - m[:, None])
            W = np.where(any_key[:, None], W / np.maximum(W.sum(1, keepdims=True), 1e-300), 0.0)
            tiles = (kl + 63) // 64
            rng_ = np.where(mask, m[:, None] - S, 0.0).max(1)
            theta = np.where(mask, delta, 0.0).max(1) + (tiles + 1) * (EXP_REL[dtype] + 2 * U32) + U32 * rng_
            r = W @ V
            mag = W @ np.abs(V)
            up, uo = (UB, UB) if bf else (0.0, 2 * U32)
            ref[qs:qs + ql, sl] = r
            bound[qs:qs + ql, sl] = (np.expm1(2 * theta) + up + (2 * kl + 2 * tiles + 8) * U32)[:, None] * mag + (uo + 3 * U32) * np.abs(r) + 1e-30
            wts[(s, h)] = W
    return ref, bound, wts


def _emulate(case, fold=False, mut=None, rq=None):
    """numpy emulation of the kernel: rounds where the kernel rounds, accumulates in fp64.  mut = a deliberately broken kernel:
    'drop' (last key of every 64-key tile, and the sequence's last key, left out), 'shift' (key j + 1's row read for key j),
    'head' (v from head h + 1), 'const' (fold: the constant of key j + 1), 'p_before_max' (the probabilities are rounded to bf16
    as exp2(score), before the row maximum is subtracted, and scaled afterwards).  rq (optional): the rounding of every register
    operand and of the output, in place of round-to-nearest-even (the restatement's storage: jitter, truncation)."""
    dtype, dk, heads = case["dtype"], case["dk"], case["heads"]
    bf = dtype == BF16
    pre = bool(case.get("k_prefolded"))
    out = np.zeros((case["q"].shape[0], heads * dk))
    if rq is None:
        rq = (lambda x: bf16_round(f32(x)).astype(np.float64)) if bf else (lambda x: f32(x).astype(np.float64))
    qscale = float(np.float32(1.44269504) / np.float32(math.sqrt(dk))) if bf else 1.0
    for s in range(case["nseq"]):
        if case["kv_len"][s] == 0 or case["q_len"][s] == 0:
            continue
        for h in range(heads):
            Q, K, V, P, mask, sl, qs, ql = _seq_operands(case, s, h, mut)
            kl = K.shape[0]
            if mut == "shift":
                idx = np.minimum(np.arange(kl) + 1, kl - 1)
                K, V = K[idx], V[idx]
            if P is not None:
                bu, bv = case["bu"][sl].astype(np.float64), case["bv"][sl].astype(np.float64)
                qu, qv = rq(f32(Q + bu) * np.float32(qscale)), rq(f32(Q + bv) * np.float32(qscale))
                if fold or pre:
                    Cj = f32(((bv - bu) * P).sum(1)).astype(np.float64) * qscale
                    if mut == "const":
                        Cj = Cj[np.minimum(np.arange(kl) + 1, kl - 1)]
                    S = Cj[None, :] + qu @ (K if pre else rq(f32(K) + f32(P))).T
                else:
                    S = qu @ K.T + qv @ P.T
            else:
                S = (rq(f32(Q) * np.float32(qscale)) if bf else Q) @ K.T
            if not bf:
                S = S / math.sqrt(dk)
            if mut == "drop":
                mask = mask.copy()
                mask[:, 63::64] = False
                mask[:, kl - 1] = False
            S = np.where(mask, f32(S).astype(np.float64), -np.inf)
            any_key = mask.any(1)
            m = np.where(any_key, S.max(1, initial=-np.inf), 0.0)
            Pr = f32(np.exp2(S - m[:, None]) if bf else np.exp(S - m[:, None])).astype(np.float64)
            l = Pr.sum(1)
            Pv = rq(np.exp2(S)) * np.exp2(-m)[:, None] if mut == "p_before_max" else rq(Pr)
            o = (Pv @ V) / np.where(l > 0, l, 1.0)[:, None]
            out[qs:qs + ql, sl] = rq(np.where(any_key[:, None], o, 0.0))
    return out


def _ratio(got, ref, bound):
    return float((np.abs(got.astype(np.float64) - ref) / bound).max())
