"""Kernel-level checks of csrc/attention.hip in every form dispatch_attn can return, called through rvb_test_attention_ex (any call
the engine builds: fused qkv / kv buffers, strided output, positional rows from an offset, the folded positional term, index list,
work list, block sizes, masks, lab switches).  Two kinds of assertion:

(a) every output element within a bound derived from what the kernel rounds (see _ref_bound), against plain fp64 softmax attention
    of the same rounded operands.  The inputs are built so that the bound is small against what a single suspicious key contributes:
    small scores, values with an O(1) signature per key / head / sequence, and for every query one key at a tile or fragment edge
    that carries 20..50 % of the softmax weight (_make).  Dropping, duplicating or mis-indexing such a key moves the output by many
    times the bound.  The CPU tests at the top prove that on a numpy emulation of the kernel's rounding points, on any machine.
(b) bit-identity between forms whose arithmetic per query is the same (layouts, block sizes, launch orders, the fold's variants,
    batch neighbours, index lists, positional offsets): no tolerance at all.

Every GPU test asserts which instantiation ran (`ran` of the hook): a test that meant to reach a form and reached another fails.
The worst error-to-bound ratio of each form is recorded with tests/test_diar_gpu.py's _record."""
import ctypes as C
import math

import numpy as np
import pytest

from reverb_amd import _lib
from reverb_amd._lib import fptr, iptr
from util import bf16_round, f32, i32

gpu = pytest.mark.gpu
# the fp64 reference, the bound and the emulation of the kernel's rounding points live in tests/attention_ref.py (shared with the bf16
# encoder's restatement, oracle/asr_bf16_ref.py)
from attention_ref import (BF16, EXP_MEASURED, EXP_REL, F32, U32, UB, _admitted, _emulate, _ratio, _ref_bound, _rnd,  # noqa: E402,F401
                           _seq_operands)
E_ARG, E_UNSUPPORTED = -1, -5
LAB_OCC3, LAB_MF1, LAB_PADK16 = 1, 2, 4
SENTINEL = -77.0          # exact in bf16


def _record(**kw):
    from test_diar_gpu import _record as rec
    rec(**kw)


# ------------------------------------------------------------------------------------------------------------------ inputs
# Score scale: q and k entries ~ N(0, s^2) with s = 1.25 / dk^(1/4), so that sum_e |q_e k_e| / sqrt(dk) is about 1 for an ordinary
# (query, key) pair (p at 0.7 of that, the biases at 0.3).  Edge boost: query i aims at one key e(i) of its sequence's edge list; both get
# a multiple of a unit direction of their own such that their score stands log(keys admitted) + logit(W_EDGE) nats above the rest, which
# gives that key about W_EDGE of the query's softmax weight (0.5 nat is added for the weight the bulk gains from its own spread).  With
# these values the numpy emulation of the kernel stays below 0.3 of the bound on every case of CPU_CASES, and every broken emulation
# exceeds the bound by a factor of 29 or more on the cases meant for it (test_bound_*; both figures printed there).
W_EDGE = 0.45
EDGE_KEYS = (0, 15, 16, 31, 32, 47, 48, 63, 64, 65, 127, 128)


def _make(seed, dtype, heads, dk, q_len, kv_len, pos=False, causal=False, q_pos0=None, chunk=0, left=-1, self_rows=True, p_rows=None,
          p_off=0):
    """One attention problem on packed buffers: q [Rq][d], k / v [Rk][d] (self_rows: queries and keys share the row layout, sequence s
    at rows s * max(q_len, kv_len)...), p [p_rows][d], biases; operands rounded to the compute dtype."""
    rng = np.random.default_rng(seed)
    d, nseq = heads * dk, len(q_len)
    q_len, kv_len = i32(q_len), i32(kv_len)
    if self_rows:
        span = np.maximum(q_len, kv_len)
        q_start = i32(np.concatenate([[0], np.cumsum(span)[:-1]]))
        kv_start = q_start.copy()
        Rq = Rk = max(int(span.sum()), 1)
    else:
        q_start = i32(np.concatenate([[0], np.cumsum(q_len)[:-1]]))
        kv_start = i32(np.concatenate([[0], np.cumsum(kv_len)[:-1]]))
        Rq, Rk = max(int(q_len.sum()), 1), max(int(kv_len.sum()), 1)
    s0 = 1.25 / dk ** 0.25
    q = s0 * rng.standard_normal((Rq, d))
    k = s0 * rng.standard_normal((Rk, d))
    j = np.arange(Rk)[:, None]
    c = np.arange(d)[None, :]
    v = np.sin(0.37 * j * (1 + c % 7) + c) + 0.25 * rng.standard_normal((Rk, d))
    case = dict(dtype=dtype, heads=heads, dk=dk, nseq=nseq, q_len=q_len, kv_len=kv_len, q_start=q_start, kv_start=kv_start,
                causal=bool(causal), q_pos0=i32(q_pos0 if q_pos0 is not None else np.zeros(nseq)), chunk=chunk, left=left,
                pos=bool(pos), p_off=p_off, kv_index=None, targets={})
    # positional rows of the edge keys get +-1 nat along (v - u) further down; the aiming query allows for it
    pos_sign = {e: (1 if n % 2 else -1) for n, e in enumerate(sorted(set(EDGE_KEYS) | {int(x) - 1 for x in kv_len if x > 0}))} if pos else {}
    for s in range(nseq):
        ks, kl, qs, ql = int(kv_start[s]), int(kv_len[s]), int(q_start[s]), int(q_len[s])
        for h in range(heads):          # the (sequence, head)'s signature: a key from the neighbouring head or sequence shows
            v[ks:ks + kl, h * dk:(h + 1) * dk] += 0.5 * ((s * heads + h) % 5 - 2)
        if kl == 0:
            continue
        edges = sorted({e for e in EDGE_KEYS + (kl - 1, (kl - 1) // 64 * 64, kl - 2) if 0 <= e < kl})
        boosted = set()

        def boost_key(e):
            if e not in boosted:
                boosted.add(e)
                for h in range(heads):
                    k[ks + e, h * dk:(h + 1) * dk] += _amp_key(dk) * _gdir(e, h, dk)
        for e in edges:
            boost_key(e)
        for i in range(ql):
            lo, hi = _admitted(case, s, i)
            if hi <= lo:
                continue
            cand = [e for e in edges if lo <= e < hi] + [lo, hi - 1]
            e = cand[i % len(cand)]
            boost = math.log(max(hi - lo - 1, 1)) + math.log(W_EDGE / (1 - W_EDGE)) + 0.5 - pos_sign.get(e, 0)
            if hi - lo < 2 or boost <= 0:
                continue
            boost_key(e)
            for h in range(heads):
                q[qs + i, h * dk:(h + 1) * dk] += boost * math.sqrt(dk) / _amp_key(dk) * _gdir(e, h, dk)
            case["targets"][(s, i)] = e
    case["q"], case["k"], case["v"] = _rnd(dtype, q), _rnd(dtype, k), _rnd(dtype, v)
    if pos:
        pr = p_rows if p_rows is not None else p_off + int(kv_len.max())
        p = 0.7 * s0 * rng.standard_normal((pr, d))
        case["bu"], case["bv"] = f32(0.3 * s0 * rng.standard_normal(d)), f32(0.3 * s0 * rng.standard_normal(d))
        # the positional rows of the edge keys get +-1 nat along (v - u): the fold's per-key constant of such a key differs from its
        # neighbours' by about a nat, so a constant read one key off moves a 40 % key's weight by a factor e
        diff = (case["bv"].astype(np.float64) - case["bu"]).reshape(heads, dk)
        for e, sign in pos_sign.items():
            if p_off + e < pr:
                for h in range(heads):
                    p[p_off + e, h * dk:(h + 1) * dk] += sign * math.sqrt(dk) * diff[h] / (diff[h] @ diff[h])
        case["p"] = _rnd(dtype, p)
    else:
        case["p"] = case["bu"] = case["bv"] = None
    return case


def _amp_key(dk):
    """what an edge key gets along its direction (the aiming query's share carries the rest of the boost: their product is
    boost * sqrt(dk)); the same for every sequence, so that hypotheses that share a prefix agree on its keys"""
    return math.sqrt(6.0 * math.sqrt(dk))


_GDIR = {}


def _gdir(e, h, dk):
    """the unit direction of key position e in head h: a function of (e, h, dk) alone"""
    if (e, h, dk) not in _GDIR:
        g = np.random.default_rng([e, h, dk]).standard_normal(dk)
        _GDIR[(e, h, dk)] = g / np.linalg.norm(g)
    return _GDIR[(e, h, dk)]


def _check_within(got, ref, bound, what):
    err = np.abs(got.astype(np.float64) - ref)
    bad = err > bound
    assert not bad.any(), "%s: %d elements outside the bound, worst err / bound %.3g (err %.3g)" % (
        what, int(bad.sum()), float((err / bound).max()), float(err[bad].max()))
    return float((err / bound).max())


# ------------------------------------------------------------------------------------------------------------------ CPU: bound vs emulation
def _cpu_cases():
    out = []
    for dtype in (BF16, F32):
        out.append(("enc2p", _make(1, dtype, 2, 64, [129, 129, 129], [129, 92, 0], pos=True), False, ("drop", "shift", "head")))
        out.append(("enc2p80", _make(2, dtype, 2, 80, [257, 257], [257, 220], pos=True), False, ("drop", "shift", "head")))
        out.append(("nopos", _make(3, dtype, 3, 32, [65, 17], [65, 17]), False, ("drop", "shift", "head")))
        out.append(("causal", _make(4, dtype, 2, 64, [70, 20], [134, 36], causal=True, q_pos0=[64, 16], self_rows=False), False,
                    ("drop", "shift", "head")))
        out.append(("chunk", _make(5, dtype, 2, 64, [200], [200], pos=True, chunk=16, left=2), False, ("shift", "head")))
    out.append(("fold", _make(6, BF16, 2, 64, [129, 129], [129, 64], pos=True), True, ("drop", "shift", "head", "const")))
    out.append(("fold48", _make(7, BF16, 3, 48, [512], [512], pos=True), True, ("drop", "shift", "head", "const")))
    return out


CPU_CASES = _cpu_cases()


@pytest.mark.parametrize("name,case,fold,muts", CPU_CASES, ids=["%s-%s" % (c[0], "bf16" if c[1]["dtype"] else "f32") for c in CPU_CASES])
def test_bound_holds_for_the_emulated_kernel_and_fails_for_broken_ones(name, case, fold, muts):
    """No GPU: the numpy emulation of the kernel's rounding points stays under the bound on every element, and each deliberately
    broken emulation (a tile's last key dropped, key j + 1 read for key j, the neighbouring head's v, the constant of key j + 1)
    exceeds it by a clear factor."""
    ref, bound, _ = _ref_bound(case, fold)
    good = _check_within(_emulate(case, fold), ref, bound, name)
    print("%s: emulation worst err / bound %.3f" % (name, good))
    assert good < 1.0
    for mut in muts:
        r = _ratio(_emulate(case, fold, mut), ref, bound)
        print("%s: broken emulation '%s' worst err / bound %.1f" % (name, mut, r))
        assert r > 5.0, "the bound would not notice '%s' on %s (ratio %.2f)" % (mut, name, r)


@pytest.mark.parametrize("name,case,fold,muts", CPU_CASES, ids=["%s-%s" % (c[0], "bf16" if c[1]["dtype"] else "f32") for c in CPU_CASES])
def test_edge_keys_carry_weight_in_every_fragment(name, case, fold, muts):
    """No GPU: in every 16-query fragment of every (sequence, head) some query gives at least 20 % of its softmax weight to the edge
    key it aims at (10 % in a tail fragment of fewer than four queries), and none gives it everything."""
    _, _, wts = _ref_bound(case, fold)
    for (s, h), W in wts.items():
        ql = W.shape[0]
        for f0 in range(0, ql, 16):
            ws = [W[i, case["targets"][(s, i)]] for i in range(f0, min(f0 + 16, ql)) if (s, i) in case["targets"]]
            if not ws:
                continue          # a fragment whose queries see a single key each
            floor = 0.2 if len(ws) >= 4 else 0.1          # a tail fragment of one or two queries has no choice of key
            assert max(ws) >= floor, "%s seq %d head %d fragment %d: heaviest aimed-at key has %.3f" % (name, s, h, f0 // 16, max(ws))
            assert min(ws) < 0.95          # and never the whole of it: the other keys still count


# ------------------------------------------------------------------------------------------------------------------ GPU call
def _call(lib, case, layout="packed", o_pad=0, q_block=0, work=None, plain=0, fold=0, prefolded=0, cap=None, lab=0, max_q=0, p_buf=None,
          p_off=None, q_pad=0, expect_rc=0):
    """one rvb_test_attention_ex call -> (out [Rq][d], ran tuple).  layout: 'packed' (three buffers of stride d), 'qkv' (one fused
    buffer of stride 3d: q | k | v; self attention rows), 'kv' (q of stride d, k | v fused at stride 2d)."""
    dtype, heads, dk = case["dtype"], case["heads"], case["dk"]
    d = heads * dk
    q, k, v = case["q"], case["k"], case["v"]
    if prefolded:          # what the qkv GEMM's epilogue writes: k + p of the key's place in its sequence, fp32 sum, rounded once
        k = k.copy()
        for s in range(case["nseq"]):
            ks, kl = int(case["kv_start"][s]), int(case["kv_len"][s])
            n = min(kl, case["p"].shape[0] - case["p_off"])
            k[ks:ks + n] = bf16_round(k[ks:ks + n] + case["p"][case["p_off"]:case["p_off"] + n])
    a = _lib.AttnTestArgs()
    keep = []

    def buf(x):
        x = np.ascontiguousarray(x, np.float32)
        keep.append(x)
        return x
    if layout == "qkv":
        assert q.shape[0] == k.shape[0]
        fused = buf(np.concatenate([q, k, v], 1))
        bufs = [(fused, 0), (fused, d), (fused, 2 * d)]
    elif layout == "kv":
        fused = buf(np.concatenate([k, v], 1))
        bufs = [(buf(q), 0), (fused, 0), (fused, d)]
    else:
        bufs = [(buf(np.pad(q, ((0, 0), (0, q_pad)))), 0), (buf(k), 0), (buf(v), 0)]
    for name, (b, col) in zip("qkv", bufs):
        setattr(a, name, fptr(b))
        setattr(a, name + "_rows", b.shape[0]); setattr(a, name + "_stride", b.shape[1]); setattr(a, name + "_col", col)
    o_col = 4 if o_pad >= 8 else 0
    out = buf(np.full((q.shape[0], d + o_pad), SENTINEL, np.float32))
    a.out, a.o_rows, a.o_stride, a.o_col = fptr(out), out.shape[0], out.shape[1], o_col
    a.dtype, a.heads, a.dk, a.nseq = dtype, heads, dk, case["nseq"]
    if case["pos"]:
        p = buf(case["p"] if p_buf is None else p_buf)
        a.p, a.p_rows, a.p_stride, a.p_col = fptr(p), p.shape[0], p.shape[1], 0
        a.p_off = case["p_off"] if p_off is None else p_off
        a.bias_u, a.bias_v = fptr(buf(case["bu"])), fptr(buf(case["bv"]))
    for n in ("q_start", "q_len", "kv_start", "kv_len"):
        setattr(a, n, iptr(buf_i(keep, case[n])))
    if case["causal"]:
        a.q_pos0 = iptr(buf_i(keep, case["q_pos0"]))
    if case["kv_index"] is not None:
        a.kv_index, a.n_index = iptr(buf_i(keep, case["kv_index"])), len(case["kv_index"])
    if work is not None:
        w = buf_i(keep, np.asarray(work).reshape(-1))
        a.work, a.n_work = iptr(w), len(w) // 2
    a.max_q, a.q_block, a.causal, a.chunk, a.left, a.plain_order = max_q, q_block, int(case["causal"]), case["chunk"], case["left"], plain
    a.fold, a.k_prefolded, a.lab = fold, prefolded, lab
    if fold:
        a.fold_kv_cap = cap if cap is not None else (int(case["kv_len"].max()) + 63) // 64 * 64
    rc = lib.rvb_test_attention_ex(C.byref(a))
    if expect_rc == 0:
        _lib.check(rc, "rvb_test_attention_ex")
    else:
        assert rc == expect_rc, "expected %d, got %d" % (expect_rc, rc)
    res = out[:, o_col:o_col + d]
    # columns outside the heads, and rows no sequence owns, keep their sentinel
    owned = np.zeros(out.shape[0], bool)
    if expect_rc == 0:
        for s in range(case["nseq"]):
            owned[int(case["q_start"][s]):int(case["q_start"][s]) + int(case["q_len"][s])] = True
    assert np.all(out[:, :o_col] == SENTINEL) and np.all(out[:, o_col + d:] == SENTINEL), "padding columns of out were written"
    assert np.all(res[~owned] == SENTINEL), "rows outside every sequence were written"
    assert np.all(res[owned] != SENTINEL) or not owned.any()
    return res.copy(), tuple(a.ran)


def buf_i(keep, x):
    x = i32(x)
    keep.append(x)
    return x


def _work_list(case, qb):
    return [(s, q0) for s in range(case["nseq"]) for q0 in range(0, int(case["q_len"][s]), qb)]


def _form(dtype, dkp, pos, nw, fold=0, padk=32, occ=1, mf=1):
    return (2 if dtype == BF16 else 4, dkp, int(pos), nw, fold, padk, occ, mf)


def _dkp(dk):
    return 32 if dk <= 32 else 64 if dk <= 64 else 96 if dk <= 96 else 128


def _owned(case):
    m = np.zeros(case["q"].shape[0], bool)
    for s in range(case["nseq"]):
        m[int(case["q_start"][s]):int(case["q_start"][s]) + int(case["q_len"][s])] = True
    return m


def _bound_check(lib, case, what, form, fold=False, **kw):
    got, ran = _call(lib, case, fold=int(fold), **kw)
    assert ran == form, "%s: meant to run %s, ran %s" % (what, form, ran)
    ref, bound, _ = _ref_bound(case, fold)
    own = _owned(case)
    return got, _check_within(got[own], ref[own], bound[own], what)


DKS = (16, 32, 48, 64, 80, 96, 104, 128)
TS = (1, 17, 64, 65, 128, 129, 257, 517)
ENC_GRID = [(dk, T, (1, 3, 8)[(i + t) % 3]) for i, dk in enumerate(DKS) for t, T in enumerate(TS) if (i + t) % 2 == 0]


# ------------------------------------------------------------------------------------------------------------------ (a) bounds per form
@gpu
@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("pos", [True, False])
def test_encoder_two_products(lib, dtype, pos):
    """Encoder form (two products, and the same without positional keys) over dk x T with kv_len {T, T - 37, 0}: catches a key of a
    tile dropped or doubled, a wrong tail mask at kv_len = 1, 17, 64, 65, ..., 517, and padding dims (dk 48, 80, 104) read as data."""
    worst = {}
    for dk, T, heads in ENC_GRID:
        case = _make(dk * 1000 + T, dtype, heads, dk, [T, T, T], [T, max(T - 37, 1), 0], pos=pos)
        got, r = _bound_check(lib, case, "encoder dk %d T %d heads %d" % (dk, T, heads), _form(dtype, _dkp(dk), pos, 8))
        assert np.all(got[2 * T:3 * T] == 0)          # a sequence without keys: zeros
        worst[_dkp(dk)] = max(worst.get(_dkp(dk), 0.0), r)
    for dkp, r in sorted(worst.items()):
        _record(test="attn_encoder", dtype=dtype, pos=pos, dkp=dkp, worst_err_over_bound=r)


@gpu
@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("heads,nseq", [(1, 3), (8, 1), (3, 3), (3, 7)])
def test_xcd_remap_of_the_grid(lib, dtype, heads, nseq):
    """(sequence, head) groups below 8, exactly 8, 8 + 1 and 16 + 5 with three query blocks each: both branches of the XCD remap and its
    boundary; the remapped order, the plain order and the work list give the same bits."""
    T = 257
    case = _make(heads * 100 + nseq, dtype, heads, 64, [T] * nseq, [T - 5 * s for s in range(nseq)], pos=True)
    form = _form(dtype, 64, True, 8)
    got, r = _bound_check(lib, case, "remap %d groups" % (heads * nseq), form, layout="qkv")
    plain, ran = _call(lib, case, layout="qkv", plain=1)
    assert ran == form and np.array_equal(got, plain)
    wl, ran = _call(lib, case, layout="qkv", work=_work_list(case, 128))
    assert ran == form and np.array_equal(got, wl)
    _record(test="attn_xcd_remap", dtype=dtype, groups=heads * nseq, worst_err_over_bound=r)


@gpu
@pytest.mark.parametrize("dk", [40, 48, 64])
@pytest.mark.parametrize("T", [63, 64, 65, 127, 129, 257])
def test_folded_forms(lib, dk, T):
    """The folded positional term in its four instantiations (FOLD 1, FOLD 2, two fragments per wave, OCC 6) and the 16-byte K pad of
    the two-product form, p_rows = kv_len so the table's clamp serves the rest of the last tile: each within the folded bound and all
    folded ones equal bit for bit (same operands bf16(k + p), same constants, same tile order).  Catches a constant read one key off,
    the second fragment's rows dropped, a spill of the squeezed form clobbering state."""
    heads = 3
    case = _make(dk * 10 + T, BF16, heads, dk, [T, T], [T, max(T - 37, 1)], pos=True, p_rows=T)
    f1, r1 = _bound_check(lib, case, "fold 1", _form(BF16, 64, True, 8, fold=1), fold=True, layout="qkv")
    big = T > 128
    f2, r2 = _bound_check(lib, case, "fold 2", _form(BF16, 64, True, 8, fold=2, occ=4 if big else 1, mf=2 if big else 1), fold=True, prefolded=1)
    f2s, r3 = _bound_check(lib, case, "fold 2, one fragment", _form(BF16, 64, True, 8, fold=2), fold=True, prefolded=1, lab=LAB_MF1)
    f6, r4 = _bound_check(lib, case, "fold 2, OCC 6", _form(BF16, 64, True, 8, fold=2, occ=6), fold=True, prefolded=1, lab=LAB_OCC3)
    assert np.array_equal(f1, f2) and np.array_equal(f2, f2s) and np.array_equal(f2, f6)
    p32, r5 = _bound_check(lib, case, "two products", _form(BF16, 64, True, 8))
    p16, r6 = _bound_check(lib, case, "two products, PADK 16", _form(BF16, 64, True, 8, padk=16), lab=LAB_PADK16)
    assert np.array_equal(p32, p16)
    for name, r in (("fold1", r1), ("fold2_mf2" if big else "fold2", r2), ("fold2", r3), ("fold2_occ6", r4), ("padk16", r6)):
        _record(test="attn_fold", form=name, dk=dk, T=T, worst_err_over_bound=r)


@gpu
def test_product_shapes(lib):
    """16 heads x 64 at T = 512 (folded with two fragments per wave, as the bf16 engine runs it) and the 268 M model's 8 heads x 80 at
    T = 512 from the fused qkv buffer, in both dtypes."""
    case = _make(11, BF16, 16, 64, [512, 512], [512, 475], pos=True)
    _, r = _bound_check(lib, case, "16 x 64, T 512, prefolded", _form(BF16, 64, True, 8, fold=2, occ=4, mf=2), fold=True, prefolded=1)
    _record(test="attn_product_16x64", dtype=BF16, worst_err_over_bound=r)
    for dtype in (BF16, F32):
        case = _make(12, dtype, 8, 80, [512, 512], [512, 475], pos=True)
        _, r = _bound_check(lib, case, "8 x 80, T 512", _form(dtype, 96, True, 8), layout="qkv")
        _record(test="attn_product_8x80", dtype=dtype, worst_err_over_bound=r)


@gpu
def test_fold_kv_cap_limits(lib):
    """fold_kv_cap 16384 is accepted with a short sequence; 16448 and a value that is no multiple of 64 are refused (E_ARG), out untouched."""
    case = _make(13, BF16, 2, 64, [70], [70], pos=True)
    ref, _ = _call(lib, case, fold=1)
    got, ran = _call(lib, case, fold=1, cap=16384)
    assert ran == _form(BF16, 64, True, 8, fold=1) and np.array_equal(got, ref)
    _call(lib, case, fold=1, cap=16448, expect_rc=E_ARG)
    _call(lib, case, fold=1, cap=100, expect_rc=E_ARG)
    _call(lib, case, fold=1, cap=64, expect_rc=E_ARG)          # does not cover kv_len 70: the hook's own check


@gpu
@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("dk", [64, 80])
@pytest.mark.parametrize("chunk,left", [(16, -1), (16, 2), (7, 1), (64, 0), (200, 3)])
def test_chunk_mask(lib, dtype, dk, chunk, left):
    """subsequent_chunk_mask inside the kernel, with the first and the last key each query's window admits weighted: catches a window
    that starts or ends one key off, and a tile loop that skips the window's first tile."""
    case = _make(chunk * 31 + left + dk, dtype, 2, dk, [300, 77], [300, 77], pos=True, chunk=chunk, left=left)
    _, r = _bound_check(lib, case, "chunk %d left %d" % (chunk, left), _form(dtype, _dkp(dk), True, 8), layout="qkv")
    _record(test="attn_chunk_mask", dtype=dtype, dk=dk, chunk=chunk, left=left, worst_err_over_bound=r)


def _trie_case(seed, dtype, dk, pos0s, q_lens):
    """hypothesis 0 is the trunk; hypothesis s shares its first q_pos0[s] keys with it (the trunk's rows, through the index list) and
    owns the q_len[s] keys after them"""
    trunk = max(pos0s) + 1
    q_len, pos0 = [trunk] + list(q_lens), [0] + list(pos0s)
    kv_len = [p0 + ql for p0, ql in zip(pos0, q_len)]
    case = _make(seed, dtype, 2, dk, q_len, kv_len, causal=True, q_pos0=pos0, self_rows=False)
    index, starts = [], []
    for s in range(len(q_len)):
        starts.append(len(index))
        ks = int(case["kv_start"][s])
        index += list(range(pos0[s])) + list(range(ks + pos0[s], ks + kv_len[s]))          # trunk = sequence 0 = rows 0 ..
    case["kv_index"], case["kv_start"] = i32(index), i32(starts)
    return case


@gpu
@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("dk", [64, 80])
def test_decoder_self_attention_over_a_trie(lib, dtype, dk):
    """Causal self attention of hypotheses that share prefixes (index list, q_pos0 in {0, 1, 15, 16, 63, 64}, path lengths across 64 and
    128) with one-wave blocks from a work list and with 128-query blocks from the grid: each within the bound, both equal bit for bit.
    Catches a causal diagonal shifted by q_pos0, an index list read at the wrong offset, a last admitted key lost at a tile edge."""
    case = _trie_case(dk, dtype, dk, [1, 15, 16, 63, 64, 64, 0], [3, 50, 49, 2, 1, 70, 130])
    g16, r = _bound_check(lib, case, "trie, one-wave blocks", _form(dtype, _dkp(dk), False, 1), q_block=16, work=_work_list(case, 16))
    g128, r2 = _bound_check(lib, case, "trie, grid", _form(dtype, _dkp(dk), False, 8))
    assert np.array_equal(g16, g128)
    _record(test="attn_trie", dtype=dtype, dk=dk, worst_err_over_bound=max(r, r2))


@gpu
@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("dk", [64, 80])
def test_cross_attention(lib, dtype, dk):
    """Cross attention as the decoder calls it: q of stride d, k | v fused at stride 2d, query sequences of 1, 130, 300 and 17 rows over
    memories of 41, 64, 90 and 512 frames.  Catches v read from the k half, and a memory shorter than a tile read past its end."""
    case = _make(dk + 7, dtype, 4, dk, [1, 130, 300, 17], [41, 64, 90, 512], self_rows=False)
    got, r = _bound_check(lib, case, "cross attention", _form(dtype, _dkp(dk), False, 8), layout="kv")
    packed, _ = _call(lib, case)
    assert np.array_equal(got, packed)
    _record(test="attn_cross", dtype=dtype, dk=dk, worst_err_over_bound=r)


@gpu
@pytest.mark.parametrize("heads,dk,rows,off", [(1, 64, 100, 0), (4, 64, 513, 0), (3, 40, 255, 7), (8, 80, 300, 1)])
def test_pos_bias_table(lib, heads, dk, rows, off):
    """attention_pos_bias on its own: c[h][j] = (v - u)[h] . p[j][h] * scale, an fp32 sum of dk terms: |err| <= (dk + 2) u32 sum|terms| * scale."""
    rng = np.random.default_rng(rows)
    d = heads * dk
    p = bf16_round(rng.standard_normal((rows, d)))
    bu, bv = f32(rng.standard_normal(d)), f32(rng.standard_normal(d))
    scale = float(np.float32(1.44269504) / np.float32(math.sqrt(dk)))
    out = np.full((heads, rows - off), np.nan, np.float32)
    _lib.check(lib.rvb_test_attention_pos_bias(fptr(p), rows, d, 0, off, fptr(bu), fptr(bv), heads, dk, scale, fptr(out)))
    diff = (bv.astype(np.float64) - bu).reshape(heads, dk)
    P = p[off:].astype(np.float64).reshape(rows - off, heads, dk)
    ref = np.einsum("he,jhe->hj", diff, P) * scale
    bound = (dk + 2) * U32 * np.einsum("he,jhe->hj", np.abs(diff), np.abs(P)) * scale + 1e-30
    r = _check_within(out, ref, bound, "pos_bias")
    _record(test="attn_pos_bias", heads=heads, dk=dk, rows=rows, worst_err_over_bound=r)


# ------------------------------------------------------------------------------------------------------------------ (b) bit-identity
@gpu
@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("dk", [32, 64, 80, 128])
def test_block_sizes_give_the_same_bits(lib, dtype, dk):
    """NW = 1 (work list), 4, 8, 16 without positional keys and NW = 4, 8, 16 with them: a query's chain does not depend on how many
    waves share its key tiles (a block that covers more queries only walks more fully masked tiles, which change nothing).  256-query
    blocks exist for bf16 with dk <= 64; elsewhere they are refused (E_UNSUPPORTED), out untouched."""
    for pos in (False, True):
        case = _make(dk + 3 * pos, dtype, 3, dk, [257, 130, 16], [257, 93, 16], pos=pos, causal=not pos)
        base, r = _bound_check(lib, case, "q_block 128", _form(dtype, _dkp(dk), pos, 8))
        g64, r64 = _bound_check(lib, case, "q_block 64", _form(dtype, _dkp(dk), pos, 4), q_block=64)
        assert np.array_equal(base, g64)
        _record(test="attn_q_block", dtype=dtype, dk=dk, pos=pos, nw=4, worst_err_over_bound=r64)
        if not pos:
            g16, ran = _call(lib, case, q_block=16, work=_work_list(case, 16))
            assert ran == _form(dtype, _dkp(dk), False, 1) and np.array_equal(base, g16)
        if dtype == BF16 and dk <= 64:
            g256, r256 = _bound_check(lib, case, "q_block 256", _form(dtype, _dkp(dk), pos, 16), q_block=256)
            assert np.array_equal(base, g256)
            _record(test="attn_q_block", dtype=dtype, dk=dk, pos=pos, nw=16, worst_err_over_bound=r256)
        else:
            _call(lib, case, q_block=256, expect_rc=E_UNSUPPORTED)


@gpu
@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("dk", [48, 64, 80])
def test_layouts_give_the_same_bits(lib, dtype, dk):
    """Packed buffers, the fused qkv buffer (stride 3d), k | v at stride 2d, an out stride with padding (vector stores) and one that is
    not 8 / 16-byte aligned (the scalar store fallback): the same bits, padding untouched.  Catches a stride used for the wrong operand."""
    case = _make(dk, dtype, 3, dk, [200, 129], [200, 129], pos=True)
    base, ran = _call(lib, case)
    for kw in (dict(layout="qkv"), dict(layout="kv"), dict(o_pad=8), dict(o_pad=1), dict(o_pad=3), dict(layout="qkv", o_pad=17)):
        got, ran2 = _call(lib, case, **kw)
        assert ran2 == ran and np.array_equal(base, got), kw
    if dtype == BF16 and 32 < dk <= 64:
        fb, ranf = _call(lib, case, fold=1, prefolded=1)
        assert ranf == _form(BF16, 64, True, 8, fold=2, occ=4, mf=2)
        for kw in (dict(layout="qkv"), dict(o_pad=1), dict(o_pad=8)):          # the second fragment's scalar stores too
            got, ran2 = _call(lib, case, fold=1, prefolded=1, **kw)
            assert ran2 == ranf and np.array_equal(fb, got), kw


@gpu
@pytest.mark.parametrize("dtype,fold", [(F32, 0), (BF16, 0), (BF16, 2)])
def test_batch_invariance(lib, dtype, fold):
    """A sequence computed alone and at every position of a ragged batch whose other sequences have lengths on both sides of 128 and 256
    and zero: the same bits.  Catches state carried from one (sequence, head) to the next and a max_q-dependent path."""
    T = 200
    others = [100, 130, 0, 250, 260]
    for place in range(len(others) + 1):
        lens = others[:place] + [T] + others[place:]
        batch = _make(77, dtype, 2, 64, lens, lens, pos=True, p_rows=260)
        s0 = int(batch["q_start"][place])
        alone = dict(batch)
        alone.update(nseq=1, q_len=i32([T]), kv_len=i32([T]), q_start=i32([s0]), kv_start=i32([s0]), q_pos0=i32([0]))
        kw = dict(fold=1, prefolded=1) if fold else {}
        gb, ranb = _call(lib, batch, **kw)
        ga, rana = _call(lib, alone, **kw)
        assert ranb == rana
        assert np.array_equal(gb[s0:s0 + T], ga[s0:s0 + T]), "sequence at place %d differs from itself alone" % place


@gpu
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_index_list_gives_the_same_bits(lib, dtype):
    """Contiguous keys, the same through an identity index list, and through a permuted one with the k / v rows permuted to match."""
    case = _make(5, dtype, 2, 64, [70, 130], [70, 130], causal=True)
    base, ran = _call(lib, case)
    ident = dict(case, kv_index=i32(np.arange(200)))
    got, ran2 = _call(lib, ident)
    assert ran2 == ran and np.array_equal(base, got)
    perm = np.random.default_rng(1).permutation(200)
    inv = np.argsort(perm)
    shuf = dict(case, kv_index=i32(inv), k=case["k"][perm], v=case["v"][perm])          # key j now lives in row inv[j]
    got, ran2 = _call(lib, shuf)
    assert ran2 == ran and np.array_equal(base, got)


@gpu
@pytest.mark.parametrize("dtype,fold", [(F32, 0), (BF16, 0), (BF16, 1)])
@pytest.mark.parametrize("off", [0, 1, 63, 64, 200])
def test_streaming_form(lib, dtype, fold, off):
    """The streaming encoder call: 16 new frames attend to 40 cached + 16 new keys held at stride 2d, positional rows (and the fold's
    table) from row `off` = offset - cache_len of a long p.  Within the bound, and the same bits as the call on a copy of p's suffix."""
    case = _make(off + 1, dtype, 3, 64, [16, 16], [56, 56], pos=True, self_rows=False, p_rows=300, p_off=off)
    form = _form(dtype, 64, True, 8, fold=fold)
    got, r = _bound_check(lib, case, "streaming, offset %d" % off, form, fold=bool(fold), layout="kv")
    suffix, ran = _call(lib, case, fold=fold, layout="kv", p_buf=case["p"][off:].copy(), p_off=0)
    assert ran == form and np.array_equal(got, suffix)
    _record(test="attn_streaming", dtype=dtype, fold=fold, off=off, worst_err_over_bound=r)


# ------------------------------------------------------------------------------------------------------------------ refusals
@gpu
def test_refusals_leave_out_untouched(lib):
    """Every E_ARG / E_UNSUPPORTED branch of attention() and dispatch_attn returns its code and writes nothing (_call checks that the
    whole of `out` still holds its sentinel)."""
    def mk(dtype, dk, heads=2, pos=True):
        return _make(1, dtype, heads, dk, [20], [20], pos=pos)
    _call(lib, mk(BF16, 12), expect_rc=E_ARG)                                  # dk no multiple of the 16-byte vector (bf16: 8)
    _call(lib, mk(F32, 6, pos=False), expect_rc=E_ARG)                        # (f32: 4)
    _call(lib, mk(BF16, 72), fold=1, prefolded=1, expect_rc=E_ARG)            # prefolded keys outside the folded form's dk range
    _call(lib, mk(BF16, 64), fold=1, prefolded=1, q_block=64, expect_rc=E_ARG)   # ... or its block size
    _call(lib, mk(BF16, 64), q_block=32, expect_rc=E_ARG)                      # no such block size
    _call(lib, mk(BF16, 64), q_block=16, work=[(0, 0)], expect_rc=E_ARG)      # one-wave blocks with positional keys
    _call(lib, mk(F32, 64), q_block=256, expect_rc=E_UNSUPPORTED)             # 256-query blocks: bf16 only
    _call(lib, mk(BF16, 80), q_block=256, expect_rc=E_UNSUPPORTED)            # ... with dk <= 64
    _call(lib, mk(BF16, 136, heads=1), expect_rc=E_UNSUPPORTED)                # dk > 128
    _call(lib, mk(F32, 132, heads=1, pos=False), expect_rc=E_UNSUPPORTED)
    _call(lib, mk(BF16, 64), q_pad=4, expect_rc=E_ARG)                         # a row stride that is no multiple of the vector
    _call(lib, mk(F32, 64), q_pad=2, expect_rc=E_ARG)
