"""Forced alignment through the engine (rvb_ctc_align / Engine.align / ReverbASR.align) on the synthetic models.

The bounds are derived, not tuned.  A Viterbi score is a sum of T fp32 terms accumulated in fp32: each addition rounds by at most half
an ulp of a partial sum no larger in magnitude than the total (all terms are <= 0), i.e. by |score| * 2^-24, so the fp32 score is within
T * 2^-24 * |score| of the exact sum of its own path.  For a transcript that is the greedy collapse of the same log-probs, the per-frame
arg-max path is a valid alignment and no path can beat the per-frame maximum, so it is the optimum."""
import numpy as np
import pytest

import force_align_ref as R
from reverb_amd import synth
from reverb_amd.engine import Engine

pytestmark = pytest.mark.gpu
CHUNK = 2051
EPS = 2.0 ** -24


def feats_of(eng, pcm, chunk=CHUNK):
    eng.upload_pcm(pcm)
    n = eng.fbank()
    nch = -(-n // chunk)
    lens = np.full(nch, chunk, np.int32)
    lens[-1] = n - (nch - 1) * chunk
    return lens


def engine(name, dtype, max_chunks=4):
    cfg, sd = synth.calibrated_state_dict(name)
    return Engine(cfg, sd, dtype=dtype, device=0, max_chunks=max_chunks, chunk_frames=CHUNK)


def argmax_facts(eng):
    """per chunk: top-1 ids / values over the valid frames, and whether any frame has a top-1 / top-2 tie"""
    v, i = eng.ctc_topk()
    lens = eng.encoder_lens()
    return [(i[b, :lens[b], 0], v[b, :lens[b], 0], bool(np.any(v[b, :lens[b], 0] == v[b, :lens[b], 1]))) for b in range(eng.batch)]


def check_greedy_alignment(res, ids, vals, tie, greedy_frames):
    T = len(ids)
    want = float(np.sum(vals.astype(np.float64)))
    print("score %.6f, sum of top-1 %.6f, bound %.3g, T %d" % (res.score, want, T * EPS * abs(want), T))
    assert abs(res.score - want) <= T * EPS * abs(want)
    if not tie:
        assert res.labels == ids.tolist()
        assert res.begin == list(greedy_frames)
    assert R.collapse(res.labels).tolist() == res.tokens
    for b, e, p in zip(res.begin, res.end, res.peak):
        assert b <= p <= e
    assert all(b2 > e1 for e1, b2 in zip(res.end, res.begin[1:]))
    assert all(0.0 < c <= 1.0 for c in res.confidence)


@pytest.mark.parametrize("name,dtype", [("tiny", "f32"), ("tiny", "bf16"), ("small", "f32"), ("small", "bf16")])
def test_per_chunk_greedy_transcript_is_the_argmax_path(name, dtype):
    """3a: transcript = the engine's own greedy tokens, one sequence per chunk."""
    eng = engine(name, dtype)
    lens = feats_of(eng, synth.synth_audio(50.0, seed=21))
    assert len(lens) == 3
    eng.encode(None, lens, 2, 0.0, T0=CHUNK)
    greedy = eng.greedy()
    facts = argmax_facts(eng)
    keep = [b for b in range(eng.batch) if greedy[b].tokens]
    assert keep, "the synthetic model emitted nothing"
    res = eng.align([greedy[b].tokens for b in keep], [(b, 1) for b in keep])
    for r, b in zip(res, keep):
        ids, vals, tie = facts[b]
        check_greedy_alignment(r, ids, vals, tie, greedy[b].ctc_frames)
        assert r.chunk_lens == [int(eng.encoder_lens()[b])] and r.first_chunk == b
        # confidence = exp of the token's log-prob at its peak frame (the tap recomputes the log-probs: compare loosely)
        lp = eng.ctc_logprobs(b)
        got = np.array(r.confidence)
        ref = np.exp(lp[np.array(r.peak), np.array(r.tokens)])
        assert np.allclose(got, ref, rtol=1e-3, atol=1e-6)
    eng.close()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_arbitrary_feasible_transcript(dtype):
    """3b: greedy tokens with seeded substitutions and deletions.  Both the aligner's path and the fp64 optimum are scored in fp64 on
    the tap's log-probs; the aligner worked in fp32 on its own copy, so its path may fall short of the optimum by the rounding of two
    fp32-accumulated sums: 2 * T * 2^-24 * |optimum|."""
    eng = engine("tiny", dtype)
    lens = feats_of(eng, synth.synth_audio(30.0, seed=33))
    eng.encode(None, lens, 2, 0.0, T0=CHUNK)
    greedy = eng.greedy()
    rng = np.random.default_rng(5)
    V, blank = eng.cfg.vocab, eng.cfg.blank_id
    for b in range(eng.batch):
        toks = [t for t in greedy[b].tokens if rng.random() > 0.15]                      # deletions
        toks = [int(rng.integers(1, V - 1)) if rng.random() < 0.2 else t for t in toks]  # substitutions
        toks = [t for t in toks if t != blank]
        T = int(eng.encoder_lens()[b])
        if not toks or R.min_frames(toks) > T:
            continue
        r = eng.align([toks], [(b, 1)])[0]
        lp = eng.ctc_logprobs(b)[:T]
        assert R.collapse(r.labels, blank).tolist() == toks
        opt = R.optimum64(lp, toks, blank)
        got = R.path_score64(lp, r.labels)
        print("chunk %d: path %.6f optimum %.6f bound %.3g" % (b, got, opt, 2 * T * EPS * abs(opt)))
        assert opt - got <= 2 * T * EPS * abs(opt)
        assert abs(r.score - got) <= 2 * T * EPS * abs(opt)
    eng.close()


def test_second_align_sees_the_second_input_and_transcribe_is_untouched():
    """3e: no stale alpha / back-pointer state; the search path after an alignment equals the search path before it."""
    eng = engine("tiny", "f32")
    modes = ["ctc_greedy_search", "ctc_prefix_beam_search", "attention_rescoring"]

    def run(seed, seconds):
        lens = feats_of(eng, synth.synth_audio(seconds, seed=seed))
        eng.encode(None, lens, 4, 0.0, T0=CHUNK)
        return eng.search(modes, 0.1, 0.0)

    first = run(41, 25.0)
    toks1 = [r.tokens for r in first["ctc_greedy_search"]]
    a1 = eng.align(toks1)
    again = eng.search(modes, 0.1, 0.0)
    for m in modes:
        assert [r.tokens for r in again[m]] == [r.tokens for r in first[m]]
    second = run(42, 43.0)
    toks2 = [r.tokens for r in second["ctc_greedy_search"]]
    a2 = eng.align(toks2)
    facts = argmax_facts(eng)
    for r, (ids, vals, tie), g in zip(a2, facts, second["ctc_greedy_search"]):
        check_greedy_alignment(r, ids, vals, tie, g.ctc_frames)
    assert [r.labels for r in a1] != [r.labels for r in a2[:len(a1)]]
    back = run(41, 25.0)
    assert [r.labels for r in eng.align(toks1)] == [r.labels for r in a1]
    for m in modes:
        assert [r.tokens for r in back[m]] == [r.tokens for r in first[m]]
    eng.close()


def test_requests_the_engine_refuses():
    from reverb_amd._lib import RvbError, check, iptr
    eng = engine("tiny", "f32")
    one, zero = np.ones(1, np.int32), np.zeros(1, np.int32)
    with pytest.raises(RvbError, match="before rvb_encode"):
        check(eng.lib.rvb_ctc_align(eng.handle, iptr(one), iptr(one), 1, iptr(zero), iptr(one), None, None, None, None, None, None),
              "rvb_ctc_align")
    lens = feats_of(eng, synth.synth_audio(25.0, seed=41))
    eng.encode(None, lens, 2, 0.0, T0=CHUNK)
    with pytest.raises(RvbError, match="chunk range"):
        eng.align([[1, 2]], [(1, 2)])
    with pytest.raises(RvbError, match="empty transcript"):
        eng.align([[]], [(0, 1)])
    with pytest.raises(RvbError, match="blank"):
        eng.align([[1, eng.cfg.blank_id]], [(0, 1)])
    with pytest.raises(RvbError, match="outside"):
        eng.align([[eng.cfg.vocab]], [(0, 1)])
    with pytest.raises(RvbError, match="infeasible"):
        eng.align([[1, 2] * 400], [(1, 1)])                  # 800 tokens against the short last chunk
    with pytest.raises(RvbError, match="16383 tokens"):
        eng.align([[1] * 16384], [(0, 2)])
    eng.close()


LONG_SEED, LONG_CHUNKS = 12, 24
LONG_SECONDS = (LONG_CHUNKS - 1) * 20.51 + 6.0


def test_long_form_one_sequence_over_the_whole_file(tmp_path):
    """3c: 24 chunks (23 full + one of 148 encoder frames: 11 924 frames), ONE sequence over all chunks, transcript = the concatenated
    greedy tokens.  rvb_ctc_align walks the log-probs in the slabs rvb_encode computed them in -- per slice of the batch, 8192 rows at
    a time -- and a 24-chunk batch is encoded as slices of 17 + 7 chunks, so the pass crosses an 8192-row slab boundary (after chunk
    16), a slice boundary (after chunk 17) and a partial chunk; 18 chunks would be slices of 13 + 5 and never fill a slab.
    Audio seed 12: on the CPU oracle (oracle/model_ref.py encoder_forward + ctc_logprobs of calibrated_state_dict("tiny"), fp32,
    verbatimicity 1) no chunk of synth_audio(477.73 s, seed=12) ends in a non-blank arg-max label that the next chunk starts with
    (seeds 11, 14 and 15 hold too), so the concatenated per-frame arg-max path is a valid alignment of the concatenated transcript
    and the argument of 3a covers the whole file.  The precondition is asserted on the device's own labels below."""
    from reverb_amd.reverb import load_model
    pcm = synth.synth_audio(LONG_SECONDS, seed=LONG_SEED)
    for dtype in ("f32", "bf16"):
        eng = engine("tiny", dtype, max_chunks=LONG_CHUNKS)
        lens = feats_of(eng, pcm)
        assert len(lens) == LONG_CHUNKS and lens[-1] < CHUNK
        eng.encode(None, lens, 2, 0.0, T0=CHUNK)
        assert int(eng.encoder_lens()[:17].sum()) > 8192 and eng.encoder_lens()[-1] < 512
        greedy = eng.greedy()
        facts = argmax_facts(eng)
        for (a, _, _), (b, _, _) in zip(facts, facts[1:]):
            assert not (a[-1] != eng.cfg.blank_id and a[-1] == b[0]), "precondition: a chunk ends in the label the next starts with"
        tokens = [t for g in greedy for t in g.tokens]
        res = eng.align([tokens], [(0, LONG_CHUNKS)])[0]
        ids = np.concatenate([f[0] for f in facts]); vals = np.concatenate([f[1] for f in facts])
        starts = np.concatenate([[0], np.cumsum(eng.encoder_lens())[:-1]])
        frames = [int(starts[b]) + f for b, g in enumerate(greedy) for f in g.ctc_frames]
        check_greedy_alignment(res, ids, vals, any(f[2] for f in facts), frames)
        assert res.chunk_frame(int(starts[17]) + 3) == (17, 3) and res.chunk_frame(int(starts[-1]) + 147) == (LONG_CHUNKS - 1, 147)
        eng.close()
    mdir = synth.write_model_dir(str(tmp_path / "m"), "tiny")
    wav = str(tmp_path / "long.wav")
    synth.write_wav(wav, pcm)
    asr = load_model(mdir, gpu=0, dtype="f32", max_chunks=LONG_CHUNKS)
    want = asr.transcribe(wav, mode="ctc_greedy_search", format="ctm").split("\n")
    n = asr.engine.fbank()
    nl = np.full(LONG_CHUNKS, CHUNK, np.int32); nl[-1] = n - (LONG_CHUNKS - 1) * CHUNK
    asr.engine.encode(None, nl, 2, 0.0, T0=CHUNK)
    tokens = [t for g in asr.engine.greedy() for t in g.tokens]
    got = asr.align(wav, tokens=tokens, format="ctm").split("\n")
    assert len(got) == len(want) > 100
    for g, w in zip(got, want):
        assert g.split()[:-1] == w.split()[:-1]            # every column but the confidence (greedy results carry none: 0.00)
        assert w.split()[-1] == "0.00" and 0.0 < float(g.split()[-1]) <= 1.0
    # 3d: the text path
    text = asr.transcribe(wav, mode="ctc_greedy_search", format="txt")
    ctm = asr.align(wav, transcript=text, format="ctm").split("\n")
    assert [l.split()[4] for l in ctm] == text.split()
    t0 = [float(l.split()[2]) for l in ctm]
    assert all(b >= a for a, b in zip(t0, t0[1:])) and 0.0 <= t0[0] and t0[-1] + float(ctm[-1].split()[3]) <= LONG_SECONDS
    js = asr.align(wav, tokens=tokens, format="json")
    assert len(js["tokens"]) == len(tokens) and all(a["start_ms"] < a["end_ms"] for a in js["tokens"])
    ali = asr.align(wav, tokens=tokens, format="ali")
    assert ali.startswith("long.wav [") and len(ali.split(",")) == int(asr.engine.encoder_lens().sum())
    with pytest.raises(ValueError):
        asr.align(wav)
    with pytest.raises(ValueError):
        asr.align(wav, transcript="a", tokens=[1])
