"""Stage-by-stage check of a bf16 run of the rescoring decoder on its OWN stored tensors, the case it runs on, and the end-to-end
figures.  Every stage's stored input, exact in bf16 or fp32, goes through the fp64 stage function of oracle/dec_bf16_ref.py, and the
stored output must lie inside that stage's derived bound.  Used on the engine's tensors (tests/test_dec_bf16_gpu.py, through
Engine.decoder_tap) and, without a GPU, on the restatement's own tensors and on mutants of them (tests/test_dec_bf16_ref.py).
Nothing here needs a GPU: the trie is built by the engine's own host code (rvb_test_build_trie).

The case: model forms64 (d 256, 4 heads of 64 as r640's, dff 256, 3 decoder layers, first and last language-specific, V 500) on the
memory of asr_bf16_checks.small_case (two chunks, encoder lengths 150 and 83).  Transcripts (TOKEN_SEED): chunk 0 -- one of 40 tokens
(its 41 owned rows span three 16-query blocks, boundaries at rows 16 and 32 inside them), three that share its first 20 tokens and
then diverge for 8 (owned rows start at position 21), one single token; chunk 1 -- two identical ones of 30 tokens (the second owns
no row: no work item) and one of 35.  Left trie 132 rows, right trie more (reversed sequences share suffixes): every GEMM has
M >= 128 and runs on gemm2, tests/test_dec_bf16_ref.py asserts it."""
import ctypes

import numpy as np
import torch

import asr_bf16_checks as AC
from oracle import dec_bf16_ref as Dc
from oracle import model_ref as M
from reverb_amd import _lib
from reverb_amd._lib import iptr

CAT = AC.CAT
TOKEN_SEED = 2          # chosen so that the oracle alone keeps near-ties below 2 % of the targets (tests/test_dec_bf16_ref.py)


def transcripts(seed=TOKEN_SEED, V=500):
    """-> (sequences, chunk_of) in chunk order; tokens in [1, V - 2] (0 is the blank, V - 1 sos / eos)"""
    rng = np.random.default_rng(seed)
    tk = lambda n: [int(v) for v in rng.integers(1, V - 1, n)]      # noqa: E731
    a = tk(40)
    seqs = [a] + [a[:20] + tk(8) for _ in range(3)] + [[(a[0] % (V - 2)) + 1]]
    same = tk(30)
    seqs1 = [same, list(same), tk(35)]
    return seqs + seqs1, [0] * len(seqs) + [1] * len(seqs1)


def build_trie(seqs, chunk_of, n_chunks, sos, eos, reversed_):
    """the engine's own trie builder on the host (rvb_test_build_trie) -> dict of dec_bf16_ref.TRIE_ARRAYS + pair_slot; what the hook
    does not return follows from what it does: hkv (a hypothesis' path: len + 1 entries, back to back), crow (a chunk's rows are
    contiguous and start with its first hypothesis' first new row), work (one item per 16 owned rows)."""
    lib = _lib.load_test()
    lens = np.array([len(s) for s in seqs], np.int32)
    toks = np.array([t for s in seqs for t in s] + [0], np.int32)
    n = len(seqs)
    P = int(lens.sum() + n)
    out = {k: np.full(m, -7, np.int32) for k, m in dict(tok=P, pos=P, path=P, hq_start=n, hq_len=n, hq_pos0=n, tgt_ptr=P + 1, tgt=P,
                                                        pair_slot=P).items()}
    n_rows, n_work = ctypes.c_int32(0), ctypes.c_int32(0)
    ch = np.array(chunk_of, np.int32)
    _lib.check(lib.rvb_test_build_trie(iptr(toks), iptr(lens), iptr(ch), n, n_chunks, sos, eos, int(reversed_), ctypes.byref(n_rows),
                                       *(iptr(out[k]) for k in ("tok", "pos", "path", "hq_start", "hq_len", "hq_pos0", "tgt_ptr", "tgt", "pair_slot")),
                                       ctypes.byref(n_work)), "rvb_test_build_trie")
    R = n_rows.value
    t = {k: out[k][:R] for k in ("tok", "pos")}
    t["tgt_ptr"] = out["tgt_ptr"][:R + 1]
    for k in ("path", "hq_start", "hq_len", "hq_pos0", "tgt", "pair_slot"):
        t[k] = out[k]
    t["hkv_len"] = lens + 1
    t["hkv_start"] = (np.cumsum(lens + 1) - (lens + 1)).astype(np.int32)
    cs, cl = np.zeros(n_chunks, np.int32), np.zeros(n_chunks, np.int32)
    for b in range(n_chunks):
        mine = np.nonzero(ch == b)[0]
        if len(mine):
            cs[b] = t["hq_start"][mine[0]]
            nxt = np.nonzero(ch > b)[0]
            cl[b] = (t["hq_start"][nxt[0]] if len(nxt) else R) - cs[b]
    t["crow_start"], t["crow_len"] = cs, cl
    t["work"] = np.array([v for h in range(n) for q0 in range(0, int(t["hq_len"][h]), 16) for v in (h, q0)], np.int32)
    assert len(t["work"]) == 2 * n_work.value
    return t


def sd64(sd):
    return {k: (v.double() if v.dtype.is_floating_point else v) for k, v in M.to_torch_sd(sd).items()}


def oracle_logits(s64, cfg, side, memory, enc_lens, seqs, chunk_of, cat=CAT):
    """oracle/model_ref.py decoder_forward in fp64, one sequence at a time on its chunk's valid frames (the right decoder on the reversed
    tokens) -> list of logits [L + 1][V]"""
    sos = cfg["output_dim"] - 1
    out = []
    with torch.no_grad():
        for s, b in zip(seqs, chunk_of):
            n = int(enc_lens[b])
            mem = torch.from_numpy(np.asarray(memory[b, :n], np.float64))[None]
            seq = list(s) if side == "left_decoder" else list(s)[::-1]
            lg = M.decoder_forward(s64, cfg, side, mem, torch.ones(1, 1, n, dtype=torch.bool), torch.tensor([[sos] + seq]),
                                   torch.tensor([len(seq) + 1]), torch.tensor(list(cat), dtype=torch.float64))
            out.append(lg[0].numpy())
    return out


def log_softmax(x):
    m = x.max(-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(-1, keepdims=True))


def per_sequence(trie, rows_values):
    """values per trie row -> list per hypothesis of the values along its path ([L + 1][...])"""
    return [rows_values[trie["path"][s:s + n]] for s, n in zip(trie["hkv_start"], trie["hkv_len"])]


def targets(seqs, side, eos):
    return [np.array((list(s) if side == "left_decoder" else list(s)[::-1]) + [eos]) for s in seqs]


def end_to_end(logp_seq, top1_seq, oracle, tg):
    """one decoder against the fp64 oracle over all target positions: logp_seq / top1_seq per sequence ([L + 1] each), oracle = the
    logits per sequence, tg = the targets -> dict(max_dlogp, rms_dlogp, argmax_diff, positions)"""
    dl, diff = [], 0
    for lp, t1, lg, t in zip(logp_seq, top1_seq, oracle, tg):
        want = log_softmax(lg)[np.arange(len(t)), t]
        dl.append(np.abs(np.asarray(lp, np.float64) - want))
        diff += int((np.asarray(t1) != lg.argmax(1)).sum())
    dl = np.concatenate(dl)
    return dict(max_dlogp=float(dl.max()), rms_dlogp=float(np.sqrt((dl ** 2).mean())), argmax_diff=diff, positions=int(dl.size))


def restatement_figures(sd, cfg, side, trie, memory, enc_lens, oracle, tg, **kw):
    """end_to_end of one restatement run (pair_slot maps a hypothesis' positions to the CSR slots of logp)"""
    lg, lp = Dc.decoder_bf16(sd, cfg, side, trie, memory, enc_lens, CAT, **kw)
    ps, k = trie["pair_slot"], np.concatenate([[0], np.cumsum(trie["hkv_len"])])
    lp_seq = [lp[ps[k[i]:k[i + 1]]] for i in range(len(trie["hkv_len"]))]
    return end_to_end(lp_seq, [v.argmax(1) for v in per_sequence(trie, lg)], oracle, tg)


JITTERS = 6
FACTOR, FLOOR = 1.25, 2          # the encoder precedent's margins: 1.25 x on the log-prob figures, + 2 positions on the count


def yardstick(sd, cfg, side, trie, memory, enc_lens, oracle, tg):
    """the largest of each figure over the plain restatement run and JITTERS jittered Storage runs -> (yardstick, runs)"""
    runs = [restatement_figures(sd, cfg, side, trie, memory, enc_lens, oracle, tg)]
    runs += [restatement_figures(sd, cfg, side, trie, memory, enc_lens, oracle, tg, jitter_seed=100 + j) for j in range(JITTERS)]
    return {k: max(r[k] for r in runs) for k in ("max_dlogp", "rms_dlogp", "argmax_diff")}, runs


def outside_yardstick(m, yard):
    bad = [k for k in ("max_dlogp", "rms_dlogp") if m[k] > FACTOR * yard[k]]
    return bad + (["argmax_diff"] if m["argmax_diff"] > yard["argmax_diff"] + FLOOR else [])


def decode_forms(raw, position, layers, is_lsl):
    """Engine.decoder_tap('forms') -> dict(gemm = {name: 1 | 2}, attention = {self: [8], src: [8]}) (head: gemm = {out: ..} per slab)"""
    if position == layers:
        return dict(gemm={"out%d" % i: v for i, v in enumerate(raw)}, attention={})
    names = ["qkv", "self_out", "src_q", "src_out"] + (["lsl"] if is_lsl else []) + ["ff1", "ff2"]
    assert len(raw) == len(names) + 16, "forms tap: %r" % (raw,)
    g = [raw[0], raw[9], raw[10], raw[19]] + list(raw[20:])
    return dict(gemm=dict(zip(names, g)), attention={"self": list(raw[1:9]), "src": list(raw[11:19])})


def check_stages(W, cfg, T, position, memory, enc_lens, want_trie=None):
    """T: the stored tensors of one position by the engine's tap names, T['trie'] the batch as the engine built it; position
    0 .. layers - 1, or `layers` for the head; memory [B][T2][d]: the stored encoder output; want_trie: the batch the transcripts
    must give (stage 'trie': every array equal).  -> (figures, failures): per stage the worst |err| / bound over EVERY element, and one
    message per stage outside its bound."""
    D = Dc.dims(cfg)
    d, heads, V, nl = D["d"], D["heads"], D["V"], len(W["layers"])
    trie = T["trie"]
    fig, bad = {}, []

    def within(name, got, ref_tol):
        ref, tol = ref_tol
        got = np.asarray(got, np.float64).reshape(ref.shape)
        r = np.abs(got - ref) / tol
        r = np.where(np.isnan(r), np.inf, r)
        fig[name] = float(r.max())
        if r.max() > 1.0:
            bad.append("%s: %d of %d elements outside the bound, worst %.3g x the bound" % (name, int((r > 1).sum()), r.size, r.max()))

    if want_trie is not None:
        diff = [k for k in Dc.TRIE_ARRAYS if not np.array_equal(np.asarray(trie[k]), np.asarray(want_trie[k]))]
        fig["trie"] = float("inf") if diff else 0.0
        if diff:
            bad.append("trie: the engine's batch differs from the transcripts' in %s" % diff)
    f64 = lambda n: np.asarray(T[n], np.float64)      # noqa: E731
    if position == nl:
        within("xn_after", T["xn_after"], Dc.norm(f64("x_in"), W["after"], Dc.EPS))
        lg = f64("logits")[:, :V]
        within("logits", lg, Dc.logits(W, f64("xn_after"), V))
        within("logp", T["logp"], Dc.logp(lg, trie))
        return fig, bad
    L = W["layers"][position]
    mem = np.asarray(memory, np.float64)
    B, T2_ = mem.shape[:2]
    if position == 0:
        within("x_emb", T["x_emb"], Dc.x_emb(W, trie))
        if not np.array_equal(np.asarray(T["x_emb"]), np.asarray(T["x_in"])):
            bad.append("x_in of layer 0 is not x_emb")
    within("kvmem", T["kvmem"], Dc.gemm(mem.reshape(B * T2_, d), L["src_kv"]))
    within("xn1", T["xn1"], Dc.norm(f64("x_in"), L["norm1"], L["eps"]))
    within("qkv", T["qkv"], Dc.gemm(f64("xn1"), L["qkv"]))
    within("ao_self", T["ao_self"], Dc.attention(Dc.self_attn_case(f64("qkv"), trie, heads)))
    within("x_self", T["x_self"], Dc.gemm(f64("ao_self"), L["self_out"], res=f64("x_in"), out="f32"))
    within("xn2", T["xn2"], Dc.norm(f64("x_self"), L["norm2"], L["eps"]))
    within("q", T["q"], Dc.gemm(f64("xn2"), L["src_q"]))
    within("ao_src", T["ao_src"], Dc.attention(Dc.src_attn_case(f64("q"), f64("kvmem"), trie, enc_lens, T2_, heads)))
    within("x_src", T["x_src"], Dc.gemm(f64("ao_src"), L["src_out"], res=f64("x_self"), out="f32"))
    within("xn3", T["xn3"], Dc.norm(f64("x_src"), L["norm3"], L["eps"]))
    ffin = f64("xn3")
    if L["is_lsl"]:
        within("y", T["y"], Dc.gemm(ffin, L["lsl"]))
        ffin = f64("y")
    within("h", T["h"], Dc.gemm(ffin, L["ff1"], act=Dc.GR.ACT_RELU))
    within("x_ff", T["x_ff"], Dc.gemm(f64("h"), L["ff2"], res=f64("x_src"), out="f32"))
    return fig, bad
