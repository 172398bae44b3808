"""The bf16 conformer encoder held to a bf16-STORAGE restatement (oracle/asr_bf16_ref.py), on a small model that takes the code
paths of the benchmark's r640 (tests/asr_bf16_checks.py: dk 64 -> the key pre-folded by the qkv GEMM, GLU in the pointwise GEMM's
epilogue, every GEMM on gemm2; first and last block language-specific).

Stage by stage: Engine.set_encoder_tap selects one position (the front end, or a block), the stored tensors of that position are
read back (rvb_get_encoder_tap), and every stage's stored input -- exact in bf16 / fp32 -- goes through the fp64 stage function;
the stored output must lie inside that stage's derived bound.  Every element of every row is checked, valid and masked alike: the
engine leaves no row of a chunk unspecified (see asr_bf16_checks).  End to end: the engine's six metrics against the fp32 oracle
stay within the restatement's own (tests/golden/asr_bf16_yardstick.json; asr_bf16_ref.outside_yardstick: 1.25 x + 4 frames on the
log-probability figures, 1.05 x and its square on the two encoder_out figures), for the small model and for the first two chunks of
the benchmark's r640.  The taps change
nothing: a tapped run gives the bits of an untapped one, and an untapped run launches what the encoder launched before the taps."""
import json
import os

import numpy as np
import pytest

import asr_bf16_checks as C
from oracle import asr_bf16_ref as A
from reverb_amd.engine import Engine, RvbError
from test_longform_gpu import _record

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
BEAM = 10
with open(os.path.join(HERE, "golden", "asr_bf16_yardstick.json")) as f:
    YARD = json.load(f)
NPZ = np.load(os.path.join(HERE, "golden", "asr_bf16_yardstick.npz"))


class Case:
    def __init__(self, name):
        y = YARD["cases"][name]
        self.name, self.yard = name, y["yardstick"]
        self._oracle = self._W = self.g = None
        if name == "r640_chunk":       # the long-form golden's model and features; of the fp32 oracle, what the fixture stores
            from golden_util import LongCase
            lc = LongCase(name)
            self.cfg, self.feats, self.cat = lc.cfg, np.concatenate([lc.chunk_feats(c)[0] for c in range(2)]), tuple(lc.cat)
            self.lens = np.array(lc.js["lens"][:2], np.int32)
            assert self.lens.tolist() == y["lens"]
            self.sd = lc.sd
            self.g = {k: NPZ["%s_%s" % (name, k)] for k in ("argmax", "top1", "gap", "enc_sample", "steps")}
        else:
            self.cfg, self.sd, self.feats, self.lens = C.small_case(y["weights_seed"], y["cnn_module_norm"])
            self.cat = C.CAT
        self.D = A.dims(self.cfg, self.feats.shape[1])
        self.want_forms = A.expected_forms(self.cfg, len(self.lens) * self.D["T2"], self.D["T2"])

    @property
    def W(self):
        if self._W is None:
            self._W = A.load_weights(self.sd, self.cfg, self.cat, self.D["T2"])
        return self._W

    def engine(self, max_chunks=2, dtype="bf16"):
        return Engine(self.cfg, self.sd, dtype=dtype, device=0, max_chunks=max_chunks, chunk_frames=self.feats.shape[1], cat_embs=self.cat)

    def oracle(self):
        if self._oracle is None:
            self._oracle = A.oracle_fp32(self.sd, self.cfg, self.feats, self.lens, C.CAT)
        return self._oracle


_CASES = {}


def _case(name):
    if name == "r640_chunk":
        return Case(name)              # not kept: its state dict is 2.7 GB
    if name not in _CASES:
        _CASES[name] = Case(name)
    return _CASES[name]


def _taps(eng, block, nb, is_lsl):
    names = C.FRONT_STAGES if block == nb else ("x_in", "xn_ffm", "pos_keys") + tuple(n for n in C.BLOCK_STAGES if n != "y" or is_lsl)
    return {n: eng.encoder_tap(n) for n in names}


def _check_forms(case, raw, block):
    """the forms that ran, against what the CPU restatement of the engine's conditions says these shapes select: a run in another
    form fails here rather than being checked against the wrong restatement"""
    nb = case.D["blocks"]
    if block == nb:
        assert raw == [2, 2], "front end: conv2 and embed_out must run on gemm2, forms tap %r" % (raw,)
        return None
    is_lsl = case.W["blocks"][block]["is_lsl"]
    got = C.decode_forms(raw, is_lsl)
    want = case.want_forms
    assert got["prefold"] == want["prefold"] and got["glu_fused"] == want["glu_fused"], (got, want)
    assert got["gemm2"] == {n: want["gemm2"][n] for n in got["gemm2"]}, (got, want)
    assert got["prefold"] and got["glu_fused"] and all(got["gemm2"].values()), "the small model must take the benchmark's forms: %r" % (got,)
    return got


@pytest.mark.parametrize("block", [3, 0, 1, 2], ids=["front_end", "block0_lsl", "block1", "block2_lsl"])
def test_every_stage_of_a_tapped_position_lies_inside_its_bound(block):
    """One encode per tapped position; check_stages on the engine's own stored tensors must return no failure.  Nothing is left
    out: every element of every tapped tensor, rows beyond a chunk's valid length included."""
    case = _case("forms64_seed0")
    nb = case.D["blocks"]
    eng = case.engine()
    try:
        eng.set_encoder_tap(block)
        eng.encode(case.feats, case.lens, BEAM)
        assert eng.encoder_lens().tolist() == [150, 83]
        forms = _check_forms(case, eng.encoder_tap("forms"), block)
        T = _taps(eng, block, nb, block < nb and case.W["blocks"][block]["is_lsl"])
    finally:
        eng.close()
    fig, bad = C.check_stages(case.sd, case.cfg, case.feats, case.lens, T, block, forms, case.W)
    print("position %d: worst |err| / bound per stage %s" % (block, json.dumps({k: round(v, 3) for k, v in fig.items()})))
    _record(case="asr_bf16_stages", position=block, forms=forms, worst_ratio=fig)
    assert not bad, "\n".join(bad)


def test_stage_check_follows_the_two_product_and_unfused_forms(monkeypatch, lab):
    """The forms of the rounds before the pre-folded key and the fused GLU (lab switches RVB_ATTN_PREFOLD=0, RVB_GLU_FUSE=0): the
    `forms` tap reports them, and the restatement's stage functions in those forms hold the engine's stored tensors -- qkv without
    the addend, attention as two products with its second register operand, pointwise_conv1 as two rounded halves that the
    depthwise kernel gates and rounds once more."""
    monkeypatch.setenv("RVB_ATTN_PREFOLD", "0")
    monkeypatch.setenv("RVB_GLU_FUSE", "0")
    case = _case("forms64_seed0")
    eng = case.engine()
    try:
        eng.set_encoder_tap(0)
        eng.encode(case.feats, case.lens, BEAM)
        forms = C.decode_forms(eng.encoder_tap("forms"), True)
        assert not forms["prefold"] and not forms["glu_fused"] and all(forms["gemm2"].values()), forms
        T = _taps(eng, 0, case.D["blocks"], True)
    finally:
        eng.close()
    assert T["glu"].shape[1] == 2 * case.D["d"]
    fig, bad = C.check_stages(case.sd, case.cfg, case.feats, case.lens, T, 0, forms, case.W)
    print("block 0, two products / un-fused GLU: %s" % json.dumps({k: round(v, 3) for k, v in fig.items()}))
    _record(case="asr_bf16_stages", position=0, forms=forms, worst_ratio=fig)
    assert not bad, "\n".join(bad)


def test_ctc_head_on_the_stored_encoder_output_lies_inside_its_bound():
    """the logits and the log-softmax stay fp32: the kept top-k log-probabilities against the fp64 head on the stored encoder_out"""
    case = _case("forms64_seed0")
    eng = case.engine()
    try:
        eng.encode(case.feats, case.lens, BEAM)
        enc = eng.encoder_out().astype(np.float64)
        tv, ti = eng.ctc_topk()
    finally:
        eng.close()
    logp, tol = A.ctc(case.W, enc.reshape(-1, enc.shape[-1]))
    want = np.take_along_axis(logp, ti.reshape(logp.shape[0], -1).astype(np.int64), 1)
    r = np.abs(tv.reshape(want.shape) - want) / tol
    print("ctc: worst |err| / bound %.3f" % r.max())
    _record(case="asr_bf16_stages", position="ctc", worst_ratio=float(r.max()))
    assert r.max() <= 1.0
    # and they are the k largest: nothing outside the kept set exceeds the smallest kept value by more than the bound
    rest = logp.copy()
    np.put_along_axis(rest, ti.reshape(logp.shape[0], -1).astype(np.int64), -np.inf, 1)
    assert np.all(rest.max(1, keepdims=True) <= want.min(1, keepdims=True) + 2 * tol)


def _engine_metrics(case, eng):
    enc = eng.encoder_out().astype(np.float64)
    logp = np.stack([eng.ctc_logprobs(b) for b in range(len(case.lens))]).astype(np.float64)
    if case.g is not None:
        return A.metrics_golden(enc, logp, case.g, case.lens)
    renc, rlogp = case.oracle()
    return A.metrics(enc, logp, renc, rlogp, case.lens)


@pytest.mark.parametrize("name", sorted(YARD["cases"]))
def test_engine_stays_within_the_storage_yardstick(name):
    """the engine's six metrics against the fp32 oracle (recomputed on the host; r640_chunk: as the fixture stores it), within what the
    restatement's own runs lose times asr_bf16_ref.outside_yardstick's margins: 1.25 x (+ 4 frames on the two counts) on the
    log-probability figures, the diarization precedent's; 1.05 x (and its square) on the two encoder_out figures.  Both come from the
    restatement's runs alone.  r640_chunk runs the benchmark's own shapes, and its `forms` are asserted on its last block."""
    case = _case(name)
    eng = case.engine()
    try:
        if case.g is not None:
            eng.set_encoder_tap(case.D["blocks"] - 1)
        eng.encode(case.feats, case.lens, BEAM)
        if case.g is not None:
            forms = C.decode_forms(eng.encoder_tap("forms"), True)
            assert forms["prefold"] and forms["glu_fused"] and all(forms["gemm2"].values()), forms
        m = _engine_metrics(case, eng)
    finally:
        eng.close()
    print("%s: engine %s\n%s  yardstick %s" % (name, json.dumps(m), " " * len(name), json.dumps(case.yard)))
    _record(case="asr_bf16_yardstick", name=name, engine=m, yardstick=case.yard)
    bad = A.outside_yardstick(m, case.yard)
    assert not bad, "%s: %s beyond the yardstick bound (1.25 x + 4 frames; encoder_out 1.05 x): engine %r, yardstick %r" % (name, bad, m, case.yard)


# what one rvb_encode of this batch (B = 2: one slice, M = 300 rows < one logit slab) launches, counted from encode_impl and
# encoder_layer as they were before the taps: GEMMs conv2 + embed_out + 8 per block + the language mix of blocks 0 and 2 + the CTC
# head; row norms: the first + 5 per block (the final norm writes the next block's first)
LAUNCHES = {"gemm": 2 + 3 * 8 + 2 + 1, "rownorm": 1 + 3 * 5, "attention": 3, "glu_dwconv": 3, "subsample": 1, "ctc_topk": 1}


def test_taps_change_nothing_and_cost_nothing_when_off():
    """encoder_out and the CTC top-k of a run tapped at any position equal those of an untapped run bit for bit, and the untapped
    run's launch counts are those of the encoder without taps (a tapped run adds copies, not launches: the counts stay)."""
    case = _case("forms64_seed0")
    eng = case.engine()
    try:
        def run(block):
            eng.set_encoder_tap(block)
            eng.reset_timings()
            eng.encode(case.feats, case.lens, BEAM)
            tv, ti = eng.ctc_topk()
            return eng.encoder_out().copy(), tv.copy(), ti.copy(), {k: int(eng.timing(k)["launches"]) for k in LAUNCHES}
        e0, v0, i0, n0 = run(-1)
        assert n0 == LAUNCHES, (n0, LAUNCHES)
        for block in (3, 0, 1, 2):
            e1, v1, i1, n1 = run(block)
            assert n1 == LAUNCHES, (block, n1)
            assert np.array_equal(e0.view(np.uint32), e1.view(np.uint32)) and np.array_equal(v0.view(np.uint32), v1.view(np.uint32)) \
                and np.array_equal(i0, i1), "tapping position %d changed the result" % block
        e2, v2, i2, n2 = run(-1)
        assert n2 == LAUNCHES and np.array_equal(e0.view(np.uint32), e2.view(np.uint32)) and np.array_equal(i0, i2)
        with pytest.raises(RvbError, match="no tap named"):
            eng.encoder_tap("qkv")                  # off: the kept copies are gone
    finally:
        eng.close()
    _record(case="asr_bf16_launches", untapped=n0)


def test_chunk_encoded_alone_is_held_to_the_same_stage_bounds():
    """Chunk 1 (encoder length 83) encoded alone: M = 150 rows, other GEMM grids than as row 1 of the batch of two.  The engine does
    not promise the bits of another batch shape (the GEMM's tile schedule follows M), so the lone run is held to the same stage
    bounds at the front end and at both kinds of block; whether the bits happen to agree is recorded, not asserted."""
    case = _case("forms64_seed0")
    feats, lens = case.feats[1:2], case.lens[1:2]
    eng = case.engine()
    try:
        eng.encode(case.feats, case.lens, BEAM)
        pair = eng.encoder_out()[1].copy()
        figs = {}
        for block in (3, 0, 1):
            eng.set_encoder_tap(block)
            eng.encode(feats, lens, BEAM)
            forms = _check_forms(case, eng.encoder_tap("forms"), block)
            T = _taps(eng, block, 3, block == 0)
            fig, bad = C.check_stages(case.sd, case.cfg, feats, lens, T, block, forms, case.W)
            assert not bad, "lone chunk, position %d:\n%s" % (block, "\n".join(bad))
            figs[block] = max(fig.values())
        same = bool(np.array_equal(eng.encoder_out()[0].view(np.uint32), pair.view(np.uint32)))
    finally:
        eng.close()
    print("lone chunk: worst ratios %s, bits equal to row 1 of the pair: %s" % (figs, same))
    _record(case="asr_bf16_lone_chunk", worst_ratio=figs, bit_identical_to_batch_row=same)


def test_tap_refusals_by_name_leave_the_kept_taps_alone():
    case = _case("forms64_seed0")
    eng = case.engine(max_chunks=16)
    try:
        eng.set_encoder_tap(1)
        eng.encode(case.feats, case.lens, BEAM)
        kept = eng.encoder_tap("qkv").copy()
        # a batch that is encoded in two slices
        f16, l16 = np.repeat(case.feats[:1], 16, 0), np.repeat(case.lens[:1], 16)
        with pytest.raises(RvbError, match="rvb_set_encoder_tap"):
            eng.encode(f16, l16, BEAM)
        assert np.array_equal(eng.encoder_tap("qkv"), kept), "a refused encode touched the kept taps"
        sentinel = np.full(4, -77.0, np.float32)
        from reverb_amd._lib import fptr
        assert eng.lib.rvb_get_encoder_tap(eng.handle, b"qkv", fptr(sentinel), sentinel.size) != 0 and np.all(sentinel == -77.0)
        assert b"rvb_get_encoder_tap" in eng.lib.rvb_last_error()
        with pytest.raises(RvbError, match="rvb_set_encoder_tap"):
            eng.set_encoder_tap(case.D["blocks"] + 1)
        # the streaming form
        with pytest.raises(RvbError, match="rvb_set_encoder_tap"):
            eng.stream_begin()
            eng.forward_chunk(case.feats[0, :67])
        eng.set_encoder_tap(-1)
        eng.stream_begin()
        with pytest.raises(RvbError, match="rvb_set_encoder_tap"):
            eng.set_encoder_tap(0)
    finally:
        eng.close()
    # fp8 states 1 and 2: the engine's first encode calibrates, every later one runs the fp8 GEMMs
    eng = case.engine(dtype="fp8")
    try:
        with pytest.raises(RvbError, match="rvb_set_encoder_tap"):
            eng.set_encoder_tap(0)
    finally:
        eng.close()
