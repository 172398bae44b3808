"""CPU side of tests/test_gemm_forms_gpu.py: the GEMM calls the engines build (csrc/gemm.hip, csrc/gemm2.hip through gemm()), as
plain dictionaries; an fp64 reference of C = res + alpha * act(A W^T + bias) on the rounded operands; a per-element bound of the
kernels' error that follows from the number formats; and a float32 numpy emulation of the kernels' rounding points with named
mutants (deliberately broken kernels), with which tests/test_gemm_ref.py proves on any machine that the bound holds for a
correct kernel and notices each mutant.  Nothing here needs a GPU.

A case is a dict: dtype (F32 / BF16), M, N, K, lda, ldw, ldc, ldres, a_row0, alpha, act, out ('f32' / 'bf16' / 'fp8'), in_fp8,
A (flat, a_elems = (a_row0 + M - 1) * lda + K values as the compute dtype holds them; row m of the kernel's A starts at element
(a_row0 + m) * lda, so lda < K means overlapping rows), W [N][ldw], bias [N] or None, res [M][ldres] or None, inplace (the fp32
output buffer is the residual: res is then what C holds on the way in, ldres = ldc, pad columns NaN), form (what it is here for)."""
import math

import numpy as np

from util import bf16_round, f32

F32, BF16 = 0, 1
ACT_NONE, ACT_SILU, ACT_RELU, ACT_LRELU, ACT_GLU = 0, 1, 2, 3, 4
U32 = 2.0 ** -24          # fp32 unit roundoff
UB = 2.0 ** -9            # bf16 unit roundoff
E_ARG, E_UNSUPPORTED = -1, -5
MUTANTS = ("drop_kvec", "bias_shift", "res_ldc", "store_n", "alpha_first", "row_k", "inplace_after")


def rnd(dtype, a):
    return bf16_round(f32(a)) if dtype == BF16 else f32(a)


def e4m3_round(x):
    """nearest e4m3 value (round to nearest even, saturating at 448, below 2^-10 -> 0): csrc/common.h f32_to_fp8_host, decoded"""
    x = np.asarray(x, np.float64)
    v = np.abs(x)
    e = np.floor(np.log2(np.maximum(v, 2.0 ** -20)))
    step = 2.0 ** (np.maximum(e, -6.0) - 3.0)
    q = np.minimum(np.rint(v / step) * step, 448.0)
    q = np.where(v < 2.0 ** -10, 0.0, q)
    return np.sign(x) * q


def bf16_half_ulp(x):
    """half the spacing of bf16 (8 significant bits) at |x|: UB * 2^(floor(log2 |x|) + 1); the smallest normal's below 2^-126"""
    e = np.floor(np.log2(np.maximum(np.abs(x), 2.0 ** -126)))
    return UB * 2.0 ** (e + 1.0)


def gemm2_applicable(case):
    """csrc/gemm2.hip gemm2_applicable for the calls built here (no convolution gather), and gemm()'s choice on top of it with the
    variant switch at 0: bf16 operands go to the 256x256 LDS-DMA kernels when this holds, f32 stays on gemm.hip."""
    if case.get("in_fp8"):
        return case["K"] % 128 == 0 and case["lda"] % 16 == 0 and case["ldw"] % 16 == 0 and case["M"] >= 1 and case["N"] >= 64 \
            and case["act"] != ACT_LRELU
    bke = 64 if case["dtype"] == BF16 else 32
    if case["K"] % bke or case["lda"] % (bke // 8) or case["ldw"] % (bke // 8):
        return False
    return case["M"] >= 128 and case["N"] >= 64 and case["act"] != ACT_LRELU


def expected_path(case, variant=0):
    """2 = gemm2.hip, 1 = gemm.hip (what the hook reports in `path`)"""
    if case.get("in_fp8"):
        return 2
    return 2 if variant != 1 and (case["dtype"] == BF16 or variant == 2) and gemm2_applicable(case) else 1


def a_elems(M, K, lda, a_row0):
    return (a_row0 + M - 1) * lda + K if M > 0 else 0


def a_view(case, row_stride=None):
    """the kernel's A [M][K] out of the flat allocation (a gather: rows overlap when lda < K)"""
    ld = case["lda"] if row_stride is None else row_stride
    idx = (case["a_row0"] * case["lda"] + np.arange(case["M"])[:, None] * ld + np.arange(case["K"])[None, :]) % max(case["A"].size, 1)
    return case["A"][idx]


def make(form, dtype, M, N, K, seed, *, lda=None, ldw=None, ldc=None, ldres=None, a_row0=0, alpha=1.0, act=ACT_NONE, out="f32",
         bias=True, res=False, inplace=False, in_fp8=False, a_scale_ops=1.0):
    """random asymmetric operands: A ~ N(0, a_scale_ops^2), W ~ N(0, 1 / K) with a per-channel factor in [1, 2), bias and residual
    ~ N(0, 1); everything rounded to what the kernel reads"""
    rng = np.random.default_rng(seed)
    lda = K if lda is None else lda
    ldw = K if ldw is None else ldw
    ldc = N if ldc is None else ldc
    if dtype == F32 and out == "bf16":
        out = "f32"               # the f32 engine writes fp32
    A = rng.standard_normal(a_elems(M, K, lda, a_row0)) * a_scale_ops
    W = rng.standard_normal((N, ldw)) / math.sqrt(K) * (1.0 + rng.random((N, 1)))
    case = dict(form=form, dtype=dtype, M=M, N=N, K=K, lda=lda, ldw=ldw, ldc=ldc, a_row0=a_row0, alpha=float(alpha), act=act, out=out,
                in_fp8=bool(in_fp8), inplace=bool(inplace), a_scale=1.0, out_scale=1.0)
    if in_fp8:                    # the hook quantises: A per tensor at a_scale, W per output channel (rvb_test_gemm_fp8)
        case["a_scale"] = float(np.abs(A).max() * 2 / 448)
        case["A_raw"], case["W_raw"] = f32(A), f32(W)
        ws = np.abs(f32(W)[:, :K]).max(1, keepdims=True).astype(np.float64) / 448.0
        ws = f32(ws).astype(np.float64)
        case["A"] = f32(e4m3_round(f32(f32(A) / np.float32(case["a_scale"]))) * np.float32(case["a_scale"]))
        case["W"] = f32(e4m3_round(f32(f32(W) / f32(ws))) * f32(ws))
    else:
        case["A"], case["W"] = rnd(dtype, A), rnd(dtype, W)
    case["bias"] = f32(rng.standard_normal(N)) if bias else None
    if inplace:
        r = np.full((M, ldc), np.nan, np.float32)
        r[:, :N] = rng.standard_normal((M, N))
        case["res"], case["ldres"] = r, ldc
    elif res:
        case["ldres"] = N if ldres is None else ldres
        case["res"] = f32(rng.standard_normal((M, case["ldres"])))
    else:
        case["res"], case["ldres"] = None, 0
    return case


def case_id(c):
    return "%s-%s-%dx%dx%d-lda%d-ldc%d-a%g-%s%s" % (c["form"], "bf16" if c["dtype"] == BF16 else "f32", c["M"], c["N"], c["K"], c["lda"],
                                                     c["ldc"], c["alpha"], c["out"], "" if c["bias"] is not None else "-nobias")


def _act64(v, act):
    if act == ACT_SILU:
        return v / (1.0 + np.exp(-v))
    if act == ACT_RELU:
        return np.maximum(v, 0.0)
    if act == ACT_LRELU:
        return np.where(v > 0.0, v, 0.01 * v)
    return v


def _parts(case):
    A, W = a_view(case).astype(np.float64), case["W"][:, :case["K"]].astype(np.float64)
    b = case["bias"].astype(np.float64) if case["bias"] is not None else np.zeros(case["N"])
    pre = A @ W.T + b
    S = np.abs(A) @ np.abs(W).T + np.abs(b)
    r = case["res"][:, :case["N"]].astype(np.float64) if case["res"] is not None else np.zeros((case["M"], case["N"]))
    ra = case.get("rowadd")
    if ra is not None:        # GemmArgs::rowadd: C[m][col0 + j] += add[m % rows][j], in fp32 after alpha and the residual, before the
        add = np.asarray(ra["add"], np.float64)     # one rounding -- for the bound it is a second residual (one more fp32 addition)
        r = r.copy()
        r[:, ra["col0"]:ra["col0"] + add.shape[1]] += add[np.arange(case["M"]) % add.shape[0]]
    return pre, S, r


def reference(case):
    """fp64 res + alpha * act(A W^T + bias) on the rounded operands, [M][N]"""
    pre, _, r = _parts(case)
    return r + case["alpha"] * _act64(pre, case["act"])


def bound(case):
    """Per-element bound of |kernel - reference|, from the formats alone (nothing here is fitted to a kernel):
      * accumulation: the kernel sums the K products and the bias in fp32 in some order; any order of n + 1 terms errs by at most
        n u32 sum|terms| to first order; taken at two unit roundoffs per term as the attention bound does: (2 K + 8) u32 S with
        S = sum_k |a_k w_k| + |bias|.  The products of bf16 (and e4m3) values are exact in fp32, those of fp32 values round once:
        inside the factor 2.
      * the activation passes that error on through its slope: |SiLU'| <= 1.0998, ReLU and LeakyReLU 1, hence the factor 1.1.
        SiLU itself is x * rcp(1 + exp2(-log2e x)) in the bf16 kernels (x / (1 + expf(-x)) in the f32 one): exponential and
        reciprocal at the measured relative error of the hardware exponential (EXP_MEASURED of tests/test_attention_kernels_gpu.py,
        with its factor 2 margin) each, the rounding of the exponent's argument (|x| u32, and the fp32 constant), one addition and
        one product: (4 EXP_MEASURED + (|x| + 4) u32) |SiLU(x)|.
      * the epilogue multiplies by alpha and adds the residual: 3 u32 (|alpha act| + |res|).
      * the output format: one rounding to nearest.  For bf16 that is half a unit in the last place of the result, 2^(e - 8) for
        |result| in [2^e, 2^(e + 1)): between u_bf16 |result| (UB = 2^-9, reached just below a power of two) and 2 u_bf16 |result|
        (just above one).  u_bf16 |result| alone is NOT a bound of a correct rounding: the emulation below, which rounds the fp32
        value to nearest even and does nothing else, reaches 1.92 times it on 300 x 256 outputs.  The half ulp is taken at
        |result| + the fp32 error above, so that a value the fp32 error carries across a power of two is covered.  For e4m3 the
        term of tests/test_fp8_gpu.py (7 % of the value + the subnormal step at the output scale).
    fp8 operands: the scaled MFMA aligns the 64 products of an instruction before it adds them, which no fp32 chain models; the
    bound is the one tests/test_fp8_gpu.py states for that kernel on the de-quantised operands (2e-3 relative + 2e-3 absolute for
    fp32 output, 1e-2 + 1e-2 for bf16)."""
    pre, S, r = _parts(case)
    act = _act64(pre, case["act"])
    ref = r + case["alpha"] * act
    al = abs(case["alpha"])
    if case.get("in_fp8"):
        if case["out"] == "f32":
            return 2e-3 + 2e-3 * np.abs(ref)
        if case["out"] == "bf16":
            return 1e-2 + 1e-2 * np.abs(ref)
        return 0.07 * np.abs(ref) + case["out_scale"] * 2.0 ** -9 * 1.01
    e = 1.1 * (2 * case["K"] + 8) * U32 * S
    if case["act"] == ACT_SILU:
        from attention_ref import EXP_MEASURED
        e = e + (4.0 * EXP_MEASURED[case["dtype"]] + (np.abs(pre) + 4.0) * U32) * np.abs(act)
    # (with a row-periodic addend -- the engine builds it without a residual, so r is the addend alone -- one more addition: 4 u32)
    b = al * e + (4 if case.get("rowadd") is not None else 3) * U32 * (al * np.abs(act) + np.abs(r))
    if case["out"] == "bf16":
        b = b + bf16_half_ulp(np.abs(ref) + b)
    elif case["out"] == "fp8":
        b = b + 0.07 * np.abs(ref) + case["out_scale"] * 2.0 ** -9 * 1.01
    return b + 1e-30


def _act32(v, act):
    v = f32(v)
    if act == ACT_SILU:
        return f32(v / f32(np.float32(1.0) + f32(np.exp(f32(-v)))))
    if act == ACT_RELU:
        return np.maximum(v, np.float32(0))
    if act == ACT_LRELU:
        return np.where(v > 0, v, f32(np.float32(0.01) * v))
    return v


def emulate(case, mut=None):
    """float32 numpy with the kernels' rounding points: K steps of 128 bytes (64 bf16 / 32 f32 / 128 e4m3 elements), each step's
    partial sum rounded to fp32 and added to an fp32 accumulator; bias, activation, alpha, residual in fp32; one rounding to the
    output format.  -> C [M][ldc] with NaN where nothing was stored.  mut = a deliberately broken kernel:
      drop_kvec      one 8-element K vector (k = 8 .. 15) of one row (the middle one) is left out
      bias_shift     column n takes bias[n + 1]
      res_ldc        the residual is addressed with ldc where ldres is meant
      store_n        the store is addressed with N where ldc is meant
      alpha_first    alpha is applied before the activation
      row_k          row m reads A at m * K instead of m * lda
      inplace_after  (in place) row m takes its residual after row m - 1 has been stored over it: it reads row m - 1's result"""
    M, N, K, ldc = case["M"], case["N"], case["K"], case["ldc"]
    A = a_view(case, K if mut == "row_k" else None).astype(np.float64)
    W = case["W"][:, :K].astype(np.float64)
    if mut == "drop_kvec":
        A = A.copy()
        A[M // 2, 8:16] = 0.0
    step = 128 if case.get("in_fp8") else (64 if case["dtype"] == BF16 else 32)
    acc = np.zeros((M, N), np.float32)
    for k0 in range(0, K, step):
        acc = f32(acc + f32(A[:, k0:k0 + step] @ W[:, k0:k0 + step].T))
    if case["bias"] is not None:
        b = case["bias"]
        if mut == "bias_shift":
            b = b[np.minimum(np.arange(N) + 1, N - 1)]
        acc = f32(acc + b)
    al = np.float32(case["alpha"])
    v = f32(_act32(f32(acc * al), case["act"])) if mut == "alpha_first" else f32(_act32(acc, case["act"]) * al)
    if case["res"] is not None:
        if mut == "res_ldc":
            flat = case["res"].reshape(-1)
            r = flat[(np.arange(M)[:, None] * ldc + np.arange(N)[None, :]) % flat.size]
        else:
            r = case["res"][:, :N]
        if mut == "inplace_after":
            out = np.empty((M, N), np.float32)
            out[0] = f32(v[0] + r[0])
            for m in range(1, M):
                out[m] = f32(v[m] + out[m - 1])
            v = out
        else:
            v = f32(v + r)
    if case["out"] == "bf16":
        v = bf16_round(v)
    elif case["out"] == "fp8":
        v = f32(e4m3_round(f32(v / np.float32(case["out_scale"]))) * np.float32(case["out_scale"]))
    C = np.full(M * ldc, np.nan, np.float32)
    ld = N if mut == "store_n" else ldc
    C[(np.arange(M)[:, None] * ld + np.arange(N)[None, :]).reshape(-1)] = v.reshape(-1)
    return C.reshape(M, ldc)


def applies(mut, case):
    """whether the mutant changes anything a correct test could see on this case"""
    if mut == "drop_kvec":
        return case["K"] >= 16
    if mut == "bias_shift":
        return case["bias"] is not None and case["N"] > 1
    if mut == "res_ldc":
        return case["res"] is not None and case["ldres"] != case["ldc"]
    if mut == "store_n":
        return case["ldc"] != case["N"] and case["M"] > 1
    if mut == "alpha_first":
        return case["act"] == ACT_SILU and case["alpha"] != 1.0          # ReLU and LeakyReLU commute with a positive factor
    if mut == "row_k":
        return case["lda"] != case["K"] and case["M"] > 1
    if mut == "inplace_after":
        return case["inplace"] and case["M"] > 1
    raise ValueError(mut)


def ratio(got, ref, bnd):
    """worst err / bound over the N valid columns; an element that is NaN (never stored) counts as infinitely wrong"""
    err = np.abs(got[:, :ref.shape[1]].astype(np.float64) - ref)
    err = np.where(np.isnan(err), np.inf, err)
    return float((err / bnd).max()) if err.size else 0.0


# ---------------------------------------------------------------------------------------------------------------- the cases
INPLACE_SHAPES = [(512, 512, 128, 512),       # all full 256x256 tiles: the epilogue with inline-asm stores
                  (515, 264, 64, 264),        # ragged both ways, one K step
                  (300, 262, 64, 262),        # N % 4 != 0, packed rows: no 16-byte rows, the element-wise epilogue
                  (300, 262, 64, 264),        # N % 4 != 0 in rows padded to 16 bytes: the ragged segment of the vector epilogue
                  (40, 256, 128, 256)]        # M < 128: gemm.hip
LOGIT_N = [(1001, 1004), (1002, 1004), (1003, 1004), (1000, 1000), (1001, 1008)]
CUT_SHAPES = [(1, 192, 128), (7, 192, 128), (127, 192, 128), (128, 192, 128), (129, 192, 128), (256, 63, 128), (256, 64, 128),
              (256, 65, 128)]


def inplace_cases():
    out = []
    for dtype in (BF16, F32):
        for i, (M, N, K, ldc) in enumerate(INPLACE_SHAPES):
            for alpha in (1.0, 0.5):
                out.append(make("inplace", dtype, M, N, K, 100 + i, ldc=ldc, alpha=alpha, inplace=True))
    return out


def fp8_inplace_case():
    return make("inplace_fp8", BF16, 512, 256, 128, 150, alpha=0.5, inplace=True, in_fp8=True, a_scale_ops=1.7)


def logits_cases(a_row0=37):
    return [make("logits", dtype, 300, N, 128, 200 + i, ldc=ldc, a_row0=a_row0) for dtype in (BF16, F32) for i, (N, ldc) in enumerate(LOGIT_N)]


def condition_cases():
    out = []
    for dtype in (BF16, F32):
        out.append(make("cond_ldc_bytes", dtype, 300, 256, 128, 300, ldc=258, out="bf16"))          # ldc * sizeof(OutT) % 16 != 0
        out.append(make("cond_ldres", dtype, 300, 256, 128, 301, res=True, ldres=257, alpha=0.5))    # ldres % 4 != 0
        out.append(make("cond_padded", dtype, 300, 256, 128, 302, ldc=264, res=True, ldres=256))     # everything aligned, ldc = N + 8
    return out


def overlap_cases():
    return [make("overlap", dtype, 300, 64, 5 * cin, 400 + cin + b, lda=cin, bias=bool(b), out="bf16")
            for dtype in (BF16, F32) for cin in (80, 64) for b in (0, 1)]


def lrelu_cases():
    return [make("lrelu", dtype, 200, 128, 256, 500, act=ACT_LRELU, bias=False, out="bf16") for dtype in (BF16, F32)]


def cut_cases():
    out = []
    for dtype in (BF16, F32):
        for i, (M, N, K) in enumerate(CUT_SHAPES):
            for o in (("bf16", "f32") if dtype == BF16 else ("f32",)):
                out.append(make("cut", dtype, M, N, K, 600 + i, act=ACT_SILU, alpha=0.5, out=o))
    return out


def long_k_cases():
    return [make("long_k", dtype, 300, 128, 1216, 700, alpha=8.0) for dtype in (BF16, F32)]


def all_cases():
    return (inplace_cases() + [fp8_inplace_case()] + logits_cases() + condition_cases() + overlap_cases() + lrelu_cases() + cut_cases() +
            long_k_cases())
