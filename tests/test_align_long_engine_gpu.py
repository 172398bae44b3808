"""Long-form forced alignment through the engine (rvb_ctc_align_long_* / Engine.align_long_* / ReverbASR.align(long_form=...)) on the
synthetic "tiny" model: one lattice over several encoded batches.

The bound is test_align_engine_gpu.py's, derived there: for a transcript that is the greedy collapse of the same log-probs the
per-frame arg-max path is the optimum, and the fp32 score lies within T * 2^-24 * |score| of the sum of the top-1 log-probs.  The
precondition -- no chunk ends in the non-blank label the next one starts with, so the concatenated arg-max path is an alignment of the
concatenated transcript -- is asserted on the device's own labels."""
import logging

import numpy as np
import pytest

import force_align_ref as R
from reverb_amd import synth
from reverb_amd._lib import RvbError
from reverb_amd.ctc_align import AlignResult
from test_align_engine_gpu import CHUNK, LONG_SECONDS, LONG_SEED, argmax_facts, check_greedy_alignment, engine, feats_of

pytestmark = pytest.mark.gpu


def batches(eng, lens, mc):
    """encode the resident file batch by batch (beam 2: the top-2 are what argmax_facts reads) -> the first chunk of each"""
    for c0 in range(0, len(lens), mc):
        eng.encode(None, lens[c0:c0 + mc], 2, 0.0, first_chunk=c0, T0=CHUNK)
        yield c0


def greedy_transcript(eng, lens, mc):
    return [t for _ in batches(eng, lens, mc) for g in eng.greedy() for t in g.tokens]


def align_long(eng, lens, mc, tokens, window_states=0):
    """-> (AlignResult over the whole file, window, margin, top-1 ids, top-1 values, any tie, greedy token frames), the facts
    collected during the same encodes that fed the lattice"""
    enc = [(int(n) - 7) // 4 + 1 for n in lens]
    used = eng.align_long_begin(tokens, sum(enc), window_states)
    facts, frames, off = [], [], 0
    for c0 in batches(eng, lens, mc):
        assert eng.encoder_lens().tolist() == enc[c0:c0 + mc]
        facts += argmax_facts(eng)
        for g, n in zip(eng.greedy(), eng.encoder_lens()):
            frames += [off + f for f in g.ctc_frames]
            off += int(n)
        eng.align_long_feed()
    labels, begin, end, score, margin = eng.align_long_finish()
    emit, off = [], 0
    for _ in batches(eng, lens, mc):
        n = int(eng.encoder_lens().sum())
        emit.append(eng.align_long_emissions(labels[off:off + n]))
        off += n
    eng.align_long_end()
    emit = np.concatenate(emit)
    peak = [int(b + np.argmax(emit[b:e + 1])) for b, e in zip(begin, end)]
    res = AlignResult(list(tokens), labels.tolist(), begin.tolist(), end.tolist(), peak, np.exp(emit[peak]).tolist(), score, 0, enc)
    for (a, _, _), (b, _, _) in zip(facts, facts[1:]):
        assert not (a[-1] != eng.cfg.blank_id and a[-1] == b[0]), "precondition: a chunk ends in the label the next starts with"
    ids, vals = np.concatenate([f[0] for f in facts]), np.concatenate([f[1] for f in facts])
    return res, used, margin, ids, vals, any(f[2] for f in facts), frames


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_three_batches_default_window(dtype):
    eng = engine("tiny", dtype, max_chunks=1)
    lens = feats_of(eng, synth.synth_audio(50.0, seed=21))
    assert len(lens) == 3
    tokens = greedy_transcript(eng, lens, 1)
    assert tokens, "the synthetic model emitted nothing"
    res, used, margin, ids, vals, tie, frames = align_long(eng, lens, 1, tokens)
    check_greedy_alignment(res, ids, vals, tie, frames)
    S_pad = (2 * len(tokens) + 1 + 31) // 32 * 32
    assert used == S_pad and margin == used                   # the window holds the lattice and never moves: no frame counts
    assert res.chunk_frame(int(sum(res.chunk_lens[:2])) + 3) == (2, 3)
    eng.close()


def test_a_small_window_gives_the_same_labels():
    eng = engine("tiny", "f32", max_chunks=5)
    lens = feats_of(eng, synth.synth_audio(LONG_SECONDS, seed=LONG_SEED))
    assert len(lens) == 24
    tokens = greedy_transcript(eng, lens, 5)
    print("tokens", len(tokens))
    assert 2 * len(tokens) + 1 > 512, "lengthen the audio: the lattice must be longer than two windows"
    wide = align_long(eng, lens, 5, tokens)
    check_greedy_alignment(*[wide[k] for k in (0, 3, 4, 5, 6)])
    small = align_long(eng, lens, 5, tokens, window_states=256)
    assert small[1] == 256 and wide[1] > 512
    print("margin at 256 states:", small[2])
    assert 0 <= small[2] < 256
    assert small[0].labels == wide[0].labels and small[0].begin == wide[0].begin
    assert np.float32(small[0].score).tobytes() == np.float32(wide[0].score).tobytes()
    eng.close()


def test_front_end(tmp_path, caplog):
    from reverb_amd.reverb import load_model
    mdir = synth.write_model_dir(str(tmp_path / "m"), "tiny")
    wav = str(tmp_path / "three.wav")
    synth.write_wav(wav, synth.synth_audio(50.0, seed=21))
    whole = load_model(mdir, gpu=0, dtype="f32", max_chunks=3)
    whole.transcribe(wav, mode="ctc_greedy_search", format="txt")        # leaves the file resident
    n = whole.engine.fbank()
    nl = np.full(3, CHUNK, np.int32); nl[-1] = n - 2 * CHUNK
    whole.engine.encode(None, nl, 2, 0.0, T0=CHUNK)
    tokens = [t for g in whole.engine.greedy() for t in g.tokens]
    want = whole.align(wav, tokens=tokens, format="ctm").split("\n")
    want_js = whole.align(wav, tokens=tokens, format="json")
    assert "window_states" not in want_js                        # today's path, untouched
    want_ali = whole.align(wav, tokens=tokens, format="ali")
    forced = whole.align(wav, tokens=tokens, format="ctm", long_form=True).split("\n")
    whole.engine.close()
    two = load_model(mdir, gpu=0, dtype="f32", max_chunks=2)
    with pytest.raises(ValueError, match="max_chunks"):
        two.align(wav, tokens=tokens, format="ctm", long_form=False)
    with pytest.raises(ValueError, match="one-batch"):
        two.align(wav, tokens=tokens, format="json", posteriors=True)
    with pytest.raises(ValueError):
        two.align(wav, transcript="a {b|c}", alternatives=True)
    for got in (two.align(wav, tokens=tokens, format="ctm", long_form=True).split("\n"), two.align(wav, tokens=tokens, format="ctm").split("\n"),
                forced):
        assert len(got) == len(want) > 3
        for g, w in zip(got, want):
            assert g.split()[:-1] == w.split()[:-1]                # every column but the confidence
            assert 0.0 < float(g.split()[-1]) <= 1.0
    js = two.align(wav, tokens=tokens, format="json")
    assert js["window_states"] == (2 * len(tokens) + 1 + 31) // 32 * 32 and js["window_margin"] == js["window_states"]
    assert [t["start_ms"] for t in js["tokens"]] == [t["start_ms"] for t in want_js["tokens"]]
    assert [t["end_ms"] for t in js["tokens"]] == [t["end_ms"] for t in want_js["tokens"]]
    assert two.align(wav, tokens=tokens, format="ali") == want_ali and want_ali.startswith("three.wav [")
    assert not [r for r in caplog.records if r.levelno >= logging.WARNING and "window_tokens" in r.getMessage()]
    two.engine.close()


def test_order_errors_and_independence():
    eng = engine("tiny", "f32", max_chunks=2)
    with pytest.raises(RvbError, match=r"\(-3\).*rvb_ctc_align_long_feed before rvb_ctc_align_long_begin"):
        eng.align_long_feed()
    lens = feats_of(eng, synth.synth_audio(50.0, seed=21))
    modes = ["ctc_greedy_search", "ctc_prefix_beam_search", "attention_rescoring"]
    eng.encode(None, lens[:2], 4, 0.0, first_chunk=0, T0=CHUNK)
    before = eng.search(modes, 0.1, 0.0)
    tokens = greedy_transcript(eng, lens, 2)
    total = sum((int(n) - 7) // 4 + 1 for n in lens)
    with pytest.raises(RvbError, match="empty transcript"):
        eng.align_long_begin([], total)
    with pytest.raises(RvbError, match="window_states 300 must be 0"):
        eng.align_long_begin(tokens, total, 300)
    with pytest.raises(RvbError, match=r"\(-3\).*before rvb_ctc_align_long_begin"):      # a refused begin leaves nothing open
        eng.align_long_feed()
    eng.align_long_begin(tokens, total)
    eng.encode(None, lens[:2], 2, 0.0, first_chunk=0, T0=CHUNK)
    eng.align_long_feed()
    with pytest.raises(RvbError, match=r"\(-3\).*finish before all %d frames were fed" % total):
        eng.align_long_finish()
    # the one-batch aligner between begin and finish works and does not disturb the long lattice
    g0 = eng.greedy()
    one = eng.align([g.tokens for g in g0 if g.tokens], [(b, 1) for b, g in enumerate(g0) if g.tokens])
    assert all(R.collapse(r.labels).tolist() == r.tokens for r in one)
    with pytest.raises(RvbError, match=r"\(-3\).*frames are used up"):                   # both chunks again: more than the lattice has left
        eng.align_long_feed()
    eng.encode(None, lens[2:], 2, 0.0, first_chunk=2, T0=CHUNK)
    eng.align_long_feed()
    labels, begin, end, score, margin = eng.align_long_finish()
    assert R.collapse(labels).tolist() == tokens
    with pytest.raises(RvbError, match=r"\(-3\).*frames are used up"):
        eng.align_long_feed()
    ref = align_long(eng, lens, 2, tokens)[0]
    assert labels.tolist() == ref.labels and np.float32(score).tobytes() == np.float32(ref.score).tobytes()
    # 3e: the search path after a long alignment equals the search path before it
    eng.encode(None, lens[:2], 4, 0.0, first_chunk=0, T0=CHUNK)
    after = eng.search(modes, 0.1, 0.0)
    for m in modes:
        assert [r.tokens for r in after[m]] == [r.tokens for r in before[m]]
    eng.close()
