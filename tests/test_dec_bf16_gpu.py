"""The bf16 rescoring decoder (rvb_attention_rescore / rvb_attention_score: decoder_forward over a prefix trie) held to a
bf16-STORAGE restatement (oracle/dec_bf16_ref.py), on a small model that takes the benchmark's code paths (tests/dec_bf16_checks.py:
heads of 64, every GEMM on gemm2, first and last layer language-specific, a trie with shared prefixes, a hypothesis whose owned rows
cross two 16-query block boundaries, a duplicate that owns no row).

Stage by stage: Engine.set_decoder_tap selects one position of one decoder, the stored tensors of that position are read back
(rvb_get_decoder_tap) and every stage's stored input -- exact in bf16 / fp32 -- goes through the fp64 stage function; the stored
output must lie inside that stage's derived bound, every element of every tensor.  The `forms` tap must equal what the CPU restatement
of the engine's conditions selects.  End to end: max and rms of |logp - fp64 oracle| and the arg-max disagreements of each decoder stay
within the restatement's own figures on the same memory (1.25 x, + 2 positions).  The taps change nothing: a tapped run returns the
bits of an untapped one, and an untapped run launches what decoder_forward launched before the taps."""
import json

import numpy as np
import pytest

import asr_bf16_checks as AC
import dec_bf16_checks as C
from oracle import dec_bf16_ref as Dc
from reverb_amd._lib import fptr
from reverb_amd.engine import Engine, RvbError
from test_longform_gpu import _record

pytestmark = pytest.mark.gpu
BEAM = 10
RW = 0.3
LAYERS = 3
LAYER_TAPS = ("x_in", "kvmem", "xn1", "qkv", "ao_self", "x_self", "xn2", "q", "ao_src", "x_src", "xn3", "h", "x_ff")
HEAD_TAPS = ("x_in", "xn_after", "logits", "logp")


class Ctx:
    def __init__(self):
        self.cfg, self.sd, self.feats, self.lens = AC.small_case(0)
        self.seqs, self.chunk_of = C.transcripts()
        self.eos = self.cfg["output_dim"] - 1
        self.W = {side: Dc.load_weights(self.sd, self.cfg, side, C.CAT) for side in Dc.SIDES}
        self.trie = {side: C.build_trie(self.seqs, self.chunk_of, 2, self.eos, self.eos, side == "right_decoder") for side in Dc.SIDES}
        self.eng = Engine(self.cfg, self.sd, dtype="bf16", device=0, max_chunks=2, chunk_frames=self.feats.shape[1], cat_embs=AC.CAT)
        self.encode()
        self.mem = self.eng.encoder_out().astype(np.float64)
        self.enc_lens = self.eng.encoder_lens()
        assert self.enc_lens.tolist() == [150, 83]

    def encode(self):
        self.eng.encode(self.feats, self.lens, BEAM)

    def score(self):
        return self.eng.attention_score(self.seqs, self.chunk_of, reverse_weight=RW, lsm_weight=0.1)

    def taps(self, position, is_lsl):
        names = HEAD_TAPS if position == LAYERS else LAYER_TAPS + (("y",) if is_lsl else ()) + (("x_emb",) if position == 0 else ())
        T = {n: self.eng.decoder_tap(n) for n in names}
        T["trie"] = self.eng.decoder_tap("trie")
        return T


@pytest.fixture(scope="module")
def ctx():
    c = Ctx()
    yield c
    c.eng.close()


def _check_position(ctx, side_i, position, want_trie, what):
    """the taps of the pass just made: `forms` against the CPU restatement of the engine's conditions, then every stage"""
    side = Dc.SIDES[side_i]
    is_lsl = position < LAYERS and ctx.W[side]["layers"][position]["is_lsl"]
    T = ctx.taps(position, is_lsl)
    R = len(T["trie"]["tok"])
    raw = ctx.eng.decoder_tap("forms")
    assert raw == Dc.expected_forms(ctx.cfg, R, position, is_lsl), "%s: forms tap %r" % (what, raw)
    forms = C.decode_forms(raw, position, LAYERS, is_lsl)
    fig, bad = C.check_stages(ctx.W[side], ctx.cfg, T, position, ctx.mem, ctx.enc_lens, want_trie)
    print("%s, %s position %d (R = %d): worst |err| / bound per stage %s" % (what, side, position, R, json.dumps({k: round(v, 3) for k, v in fig.items()})))
    _record(case="dec_bf16_stages", path=what, side=side, position=position, rows=R, forms=forms, worst_ratio=fig)
    assert not bad, "\n".join(bad)
    return forms


@pytest.mark.parametrize("side_i,position", [(0, 0), (0, 1), (0, 2), (0, 3), (1, 0), (1, 3)],
                         ids=["left-layer0_lsl", "left-layer1", "left-layer2_lsl", "left-head", "right-layer0_lsl", "right-head"])
def test_every_stage_of_a_tapped_position_lies_inside_its_bound(ctx, side_i, position):
    """One rvb_attention_score per tapped position, both decoders; nothing is left out: every element of every tapped tensor, the batch
    itself (the `trie` tap against the trie the transcripts give: the right decoder must have been fed the reversed tokens)."""
    ctx.eng.set_decoder_tap(side_i, position)
    try:
        ctx.score()
        forms = _check_position(ctx, side_i, position, ctx.trie[Dc.SIDES[side_i]], "attention_score")
    finally:
        ctx.eng.set_decoder_tap(0, -1)
    assert all(v == 2 for v in forms["gemm"].values()), "the case must run every GEMM on gemm2: %r" % (forms,)


@pytest.mark.parametrize("position", [0, 3], ids=["layer0_lsl", "head"])
def test_rescoring_path_is_held_to_the_same_bounds(ctx, position):
    """prefix beam + rescoring with the memory keys / values made beforehand by rvb_prepare_rescoring: the trie is the n-best lists'
    (stitched from the per-chunk tries the search workers built), kvmem is what the earlier call left."""
    eng = ctx.eng
    ctx.encode()
    eng.set_decoder_tap(0, position)
    try:
        from reverb_amd._lib import check
        check(eng.lib.rvb_prepare_rescoring(eng.handle, 1), "rvb_prepare_rescoring")
        pref = eng.prefix_beam()
        eng.rescore(pref, 0.3, RW)
        nbest = [list(h) for p in pref for h in p.nbest]
        chunk_of = [b for b, p in enumerate(pref) for _ in p.nbest]
        want = C.build_trie(nbest, chunk_of, 2, ctx.eos, ctx.eos, False)
        _check_position(ctx, 0, position, want, "rescore")
    finally:
        eng.set_decoder_tap(0, -1)


def test_end_to_end_stays_within_the_restatements_own_figures(ctx):
    """Per decoder: max and rms of |logp - oracle| over all target positions and the arg-max disagreements, the oracle being
    oracle/model_ref.py's decoder in fp64 on the engine's stored encoder_out, one sequence at a time.  Held to the largest of the
    restatement's own figures over its plain run and six jittered Storage runs on the same memory (computed here: the yardstick comes
    from the restatement and the oracle only), times 1.25 on the log-prob figures, + 2 positions on the count."""
    s64 = C.sd64(ctx.sd)
    for side_i, side in enumerate(Dc.SIDES):
        ctx.eng.set_decoder_tap(side_i, LAYERS)
        try:
            got = ctx.score()
            lg = ctx.eng.decoder_tap("logits")[:, :ctx.cfg["output_dim"]]
            trie = ctx.eng.decoder_tap("trie")
        finally:
            ctx.eng.set_decoder_tap(0, -1)
        oracle = C.oracle_logits(s64, ctx.cfg, side, ctx.mem, ctx.enc_lens, ctx.seqs, ctx.chunk_of)
        tg = C.targets(ctx.seqs, side, ctx.eos)
        top1 = [v.argmax(1) for v in C.per_sequence(trie, lg)]
        if side_i == 0:
            assert all(np.array_equal(g["top1_l"], t) for g, t in zip(got, top1)), "top1_l is not the arg-max of the stored logits"
        m = C.end_to_end([g["logp_l" if side_i == 0 else "logp_r"] for g in got], top1, oracle, tg)
        yard, _ = C.yardstick(ctx.sd, ctx.cfg, side, ctx.trie[side], ctx.mem, ctx.enc_lens, oracle, tg)
        print("%s: engine %s\n%s  yardstick %s" % (side, json.dumps(m), " " * len(side), json.dumps(yard)))
        _record(case="dec_bf16_yardstick", side=side, engine=m, yardstick=yard)
        bad = C.outside_yardstick(m, yard)
        assert not bad, "%s: %s beyond the yardstick bound (1.25 x; + 2 positions): engine %r, yardstick %r" % (side, bad, m, yard)


# what one rvb_attention_score with both decoders launches right after an rvb_encode, counted from decoder_forward and
# decoder_memory_kv as they were before the taps, per decoder: GEMMs = 3 memory K/V + 6 per layer (qkv, self_out, src_q, src_out, ff1,
# ff2) + the language mix of layers 0 and 2 + 1 output slab; row norms 3 per layer + after_norm; two attentions per layer
LAUNCHES = {"gemm": 2 * (3 + 3 * 6 + 2 + 1), "rownorm": 2 * (3 * 3 + 1), "attention": 2 * 6, "embed": 2, "lse_gather": 2}


def test_taps_change_nothing_and_cost_nothing_when_off(ctx):
    eng = ctx.eng

    def run(side_i, position):
        eng.set_decoder_tap(side_i, position)
        ctx.encode()
        eng.reset_timings()
        got = ctx.score()
        n = {k: int(eng.timing(k)["launches"]) for k in LAUNCHES}
        return np.concatenate([g["logp_l"] for g in got]), np.concatenate([g["logp_r"] for g in got]), [g["loss_l"] for g in got], n
    try:
        l0, r0, s0, n0 = run(0, -1)
        assert n0 == LAUNCHES, (n0, LAUNCHES)
        for side_i, position in [(0, 0), (0, 1), (0, 2), (0, 3), (1, 0), (1, 1), (1, 2), (1, 3)]:
            l1, r1, s1, n1 = run(side_i, position)
            assert n1 == LAUNCHES, (side_i, position, n1)
            assert np.array_equal(l0.view(np.uint32), l1.view(np.uint32)) and np.array_equal(r0.view(np.uint32), r1.view(np.uint32)) \
                and s0 == s1, "tapping side %d position %d changed the result" % (side_i, position)
        l2, r2, s2, n2 = run(0, -1)
        assert n2 == LAUNCHES and np.array_equal(l0.view(np.uint32), l2.view(np.uint32)) and np.array_equal(r0.view(np.uint32), r2.view(np.uint32))
        with pytest.raises(RvbError, match="no tap named"):
            eng.decoder_tap("qkv")                  # off: the kept copies are gone
    finally:
        eng.set_decoder_tap(0, -1)
    _record(case="dec_bf16_launches", untapped=n0)


def test_tap_refusals_by_name_leave_the_kept_taps_alone(ctx):
    eng = ctx.eng
    eng.set_decoder_tap(0, 1)
    try:
        ctx.score()
        kept = {n: eng.decoder_tap(n).copy() for n in ("qkv", "x_ff")}
        forms = eng.decoder_tap("forms")

        def untouched():
            return all(np.array_equal(eng.decoder_tap(n), v) for n, v in kept.items()) and eng.decoder_tap("forms") == forms
        sentinel = np.full(4, -77.0, np.float32)
        for name in (b"nothing", b"y", b"logits"):        # an unknown name; names this position does not keep
            assert eng.lib.rvb_get_decoder_tap(eng.handle, name, fptr(sentinel), sentinel.size) != 0 and np.all(sentinel == -77.0)
            assert b"rvb_get_decoder_tap: no tap named " + name in eng.lib.rvb_last_error()
        assert eng.lib.rvb_get_decoder_tap(eng.handle, b"qkv", fptr(sentinel), sentinel.size) != 0 and np.all(sentinel == -77.0)
        assert b"rvb_get_decoder_tap: qkv holds" in eng.lib.rvb_last_error()
        assert untouched()
        for side_i, position in ((0, LAYERS + 1), (0, -2), (2, 0), (-1, 0)):
            with pytest.raises(RvbError, match="rvb_set_decoder_tap"):
                eng.set_decoder_tap(side_i, position)
            assert untouched(), "a refused switch touched the kept taps"
        # more trie rows than one logit slab: the head keeps everything but the logits, and says why
        rng = np.random.default_rng(3)
        long_seqs = [[int(v) for v in rng.integers(1, ctx.eos, 4100)] for _ in range(2)]
        eng.set_decoder_tap(0, LAYERS)
        got = eng.attention_score(long_seqs, [0, 1], reverse_weight=0.0)
        xn = eng.decoder_tap("xn_after").copy()
        assert xn.shape[0] == 8202 and np.all(np.isfinite(got[0]["logp_l"]))
        with pytest.raises(RvbError, match="rvb_get_decoder_tap: logits are not kept for 8202 trie rows"):
            eng.decoder_tap("logits")
        assert np.array_equal(eng.decoder_tap("xn_after"), xn) and np.array_equal(eng.decoder_tap("logp"), np.concatenate([g["logp_l"] for g in got]))
    finally:
        eng.set_decoder_tap(0, -1)
    fp8 = Engine(ctx.cfg, ctx.sd, dtype="fp8", device=0, max_chunks=2, chunk_frames=ctx.feats.shape[1], cat_embs=AC.CAT)
    try:
        with pytest.raises(RvbError, match="rvb_set_decoder_tap: not available on an fp8 engine"):
            fp8.set_decoder_tap(0, 0)
        fp8.set_decoder_tap(0, -1)
    finally:
        fp8.close()
