"""Phrase search through the engine (rvb_ctc_find / Engine.find / ReverbASR.find / bin/find_wav) on the tiny fp32 model and the 25 s of
synthetic audio in two chunks that test_align_wild_engine_gpu.py uses.  The yardstick is tests/ctc_find_ref.py on the engine's own
log-probs (rvb_get_ctc_logprobs per chunk, row maxima taken in numpy): bit for bit, since the kernel only subtracts, adds and compares."""
import json

import numpy as np
import pytest

import ctc_find_ref as R
from reverb_amd import synth
from reverb_amd.engine import Engine

pytestmark = pytest.mark.gpu
CHUNK = 2051
MIN_SCORE = -2.0


@pytest.fixture(scope="module")
def enc():
    """the encoded batch, its log-probs and greedy tokens, shared by the tests (none of them changes it)"""
    cfg, sd = synth.calibrated_state_dict("tiny")
    eng = Engine(cfg, sd, dtype="f32", device=0, max_chunks=4, chunk_frames=CHUNK)
    eng.upload_pcm(synth.synth_audio(25.0, seed=41))
    n = eng.fbank()
    nch = -(-n // CHUNK)
    lens = np.full(nch, CHUNK, np.int32)
    lens[-1] = n - (nch - 1) * CHUNK
    assert nch == 2
    eng.encode(None, lens, 2, 0.0, T0=CHUNK)
    elens = eng.encoder_lens()
    lp = [eng.ctc_logprobs(c)[:int(elens[c])].copy() for c in range(2)]
    greedy = eng.greedy()
    assert len(greedy[0].tokens) >= 12 and len(greedy[1].tokens) >= 3
    yield eng, lp, greedy
    eng.close()


def unique_run(toks, n, lo=0):
    """the first n-gram of toks[lo:] that occurs once in toks"""
    for i in range(lo, len(toks) - n + 1):
        g = toks[i:i + n]
        if sum(toks[j:j + n] == g for j in range(len(toks) - n + 1)) == 1:
            return i, g
    raise AssertionError("no unique n-gram")


def expected(lp_seqs, phrases, min_score, cap, max_hits, blank):
    out = []
    for y in phrases:
        per = []
        for lp in lp_seqs:
            n, _, hits = R.find(lp, lp.max(axis=1), y, blank, np.float32(min_score * len(y)), cap, max_hits)
            per.append((n, [(s, e, np.float32(v).tobytes()) for s, e, v in hits]))
        out.append(per)
    return out


def as_tuples(found):
    return [[[(h.start_frame, h.end_frame, np.float32(h.score).tobytes()) for h in seq] for seq in per] for per in found]


def phrases_of(greedy, vocab):
    t0 = list(greedy[0].tokens)
    rng = np.random.default_rng(3)
    return [t0[3:6], t0[:1], t0[7:9], rng.integers(1, vocab - 1, size=4).tolist(), t0[-2:] + list(greedy[1].tokens[:2])]


def test_find_equals_the_reference_bit_for_bit(enc):
    eng, lp, greedy = enc
    blank = eng.cfg.blank_id
    phrases = [p for p in phrases_of(greedy, eng.cfg.vocab) if blank not in p]
    for ranges, seqs in (([(0, 2)], [np.concatenate(lp)]), ([(0, 1), (1, 1)], lp)):
        found = eng.find(phrases, ranges, MIN_SCORE, 16)
        cap = eng.last_find["max_candidates"]
        want = expected(seqs, phrases, MIN_SCORE, cap, 16, blank)
        assert as_tuples(found) == [[hits for _, hits in per] for per in want]
        print("ranges", ranges, "hits per phrase", [[len(s) for s in per] for per in found], "calls", eng.last_find)
        lens = eng.encoder_lens()
        for per in found:
            for i, seq in enumerate(per):
                for h in seq:
                    first = ranges[i][0]
                    before = int(lens[first:h.chunk].sum())
                    assert h.start_frame == before + h.frame_in_chunk and 0 <= h.frame_in_chunk < lens[h.chunk]
    assert eng.find(phrases) == eng.find(phrases, [(0, 2)], -1.0, 64)          # the defaults: one sequence over the batch


def test_a_phrase_of_the_greedy_string_scores_zero_at_its_frames(enc):
    eng, _, greedy = enc
    toks, frames = list(greedy[0].tokens), list(greedy[0].ctc_frames)
    i, g = unique_run(toks, 3, 2)
    hits = eng.find([g], [(0, 1)], -0.01, 8)[0][0]
    zero = [h for h in hits if h.score == 0.0]
    assert [(h.start_frame, h.end_frame) for h in zero] == [(frames[i], frames[i + 2])]
    assert zero[0].chunk == 0 and zero[0].frame_in_chunk == frames[i] and zero[0].score_per_token == 0.0


def test_a_phrase_across_the_chunk_boundary_needs_the_two_chunk_sequence(enc):
    eng, _, greedy = enc
    t0, t1 = list(greedy[0].tokens), list(greedy[1].tokens)
    f0, f1 = list(greedy[0].ctc_frames), list(greedy[1].ctc_frames)
    assert t0[-1] != t1[0], "precondition: the two chunks do not meet inside one token run"
    g = t0[-2:] + t1[:2]
    both = t0 + t1
    assert sum(both[j:j + 4] == g for j in range(len(both) - 3)) == 1
    T0 = int(eng.encoder_lens()[0])
    whole = eng.find([g], [(0, 2)], -0.01, 8)[0][0]
    assert [(h.start_frame, h.end_frame, h.score) for h in whole if h.score == 0.0] == [(f0[-2], T0 + f1[1], 0.0)]
    hit = [h for h in whole if h.score == 0.0][0]
    assert (hit.chunk, hit.frame_in_chunk) == (0, f0[-2])
    per_chunk = eng.find([g], [(0, 1), (1, 1)], -0.01, 8)[0]
    assert per_chunk == [[], []]


def test_an_overflowing_candidate_cap_is_retried_once(enc):
    eng, lp, greedy = enc
    blank = eng.cfg.blank_id
    phrases = [list(greedy[0].tokens[:1]), list(greedy[0].tokens[3:5])]
    found = eng.find(phrases, [(0, 2)], -np.inf, 8, max_candidates=1)
    assert eng.last_find["calls"] == 2
    counts = [len(R.candidates(np.concatenate(lp), np.concatenate(lp).max(axis=1), y, blank, -np.inf)) for y in phrases]
    assert eng.last_find["max_candidates"] == max(counts) > 1
    want = expected([np.concatenate(lp)], phrases, -np.inf, max(counts), 8, blank)
    assert as_tuples(found) == [[hits for _, hits in per] for per in want]
    assert eng.find(phrases, [(0, 2)], -np.inf, 8, max_candidates=max(counts)) == found and eng.last_find["calls"] == 1


def test_find_wav_writes_what_the_api_returns(tmp_path, monkeypatch):
    from reverb_amd import reverb
    from reverb_amd.bin import find_wav
    mdir = synth.write_model_dir(str(tmp_path / "m"), "tiny")
    wav = str(tmp_path / "talk.wav")
    synth.write_wav(wav, synth.synth_audio(25.0, seed=41))
    asr = reverb.load_model(mdir, gpu=0, dtype="f32", max_chunks=4)
    words = asr.transcribe(wav, mode="ctc_greedy_search", format="txt").split()
    assert len(words) >= 6
    terms = [words[1], " ".join(words[3:5]), words[-1]]
    lst = tmp_path / "terms.txt"
    lst.write_text("\n".join(terms) + "\n\n", encoding="utf-8")
    api = asr.find(wav, phrases=terms, min_score=-1.0, max_hits=16)
    assert [r["phrase"] for r in api] == terms and sum(len(r["hits"]) for r in api) >= 1
    for r in api:
        assert all(0.0 <= h["start"] < h["end"] and h["score"] >= np.float32(-1.0 * len(r["tokens"])) and 0.0 < h["confidence"] <= 1.0
                   for h in r["hits"])
        assert [h["end_frame"] for h in r["hits"]] == sorted(h["end_frame"] for h in r["hits"])
    assert asr.find(wav, phrase_file=str(lst), min_score=-1.0, max_hits=16) == api
    with pytest.raises(ValueError, match="exactly one"):
        asr.find(wav)
    monkeypatch.setattr(reverb, "load_model", lambda *a, **k: asr)            # the tool under test is the writer, not the loader
    common = ["--model", mdir, "--audio_file", wav, "--phrase_list", str(lst), "--result_dir", str(tmp_path / "out"), "--max_hits", "16",
              "--dtype", "f32", "--max_chunks", "4"]
    find_wav.main(common)
    assert json.loads((tmp_path / "out" / "talk.find.json").read_text(encoding="utf-8")) == json.loads(json.dumps(api))
    find_wav.main(common + ["--format", "ctm"])
    lines = [l.split() for l in (tmp_path / "out" / "talk.find.ctm").read_text(encoding="utf-8").split("\n")]
    assert len(lines) == sum(len(r["hits"]) for r in api)
    assert all(l[0] == "talk.wav" and l[1] == "0" and len(l) == 6 for l in lines)
    assert sorted(l[4] for l in lines) == sorted("_".join(r["phrase"].split()) for r in api for _ in r["hits"])
    starts = [float(l[2]) for l in lines]
    assert starts == sorted(starts)
    asr.engine.close()
