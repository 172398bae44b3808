"""Full-sum scoring through the engine (rvb_ctc_score / Engine.score / ReverbASR.score) on the synthetic model, 2 chunks.

The restatement runs on rvb_get_ctc_logprobs, which recomputes the CTC head in a launch of its own shape: in f32 the two sets of
log-probs agree to fp32 rounding of a d_model-long dot product, so loglik is compared at the kernel's own ceiling of 1e-5 nats per
frame plus T * 1e-5 for the log-probs (d_model = 64 terms of 2^-24 relative on values of magnitude <= 10: < 1e-5 per frame)."""
import json

import numpy as np
import pytest

import ctc_score_ref as R
from reverb_amd import synth
from reverb_amd.ctc_align import align_to_json
from reverb_amd.engine import Engine

pytestmark = pytest.mark.gpu
CHUNK = 2051


@pytest.fixture(scope="module")
def encoded():
    cfg, sd = synth.calibrated_state_dict("tiny")
    eng = Engine(cfg, sd, dtype="f32", device=0, max_chunks=4, chunk_frames=CHUNK)
    eng.upload_pcm(synth.synth_audio(30.0, seed=21))
    n = eng.fbank()
    nch = -(-n // CHUNK)
    assert nch == 2
    lens = np.full(nch, CHUNK, np.int32)
    lens[-1] = n - (nch - 1) * CHUNK
    eng.encode(None, lens, 2, 0.0, T0=CHUNK)
    toks = [g.tokens for g in eng.greedy()]
    assert all(toks)
    yield eng, toks
    eng.close()


def test_score_matches_the_restatement_per_chunk_and_over_both(encoded):
    eng, toks = encoded
    lens = eng.encoder_lens()
    lps = [eng.ctc_logprobs(b)[:int(lens[b])] for b in range(2)]
    blank = eng.cfg.blank_id
    per = eng.score(toks, posteriors=True)
    whole = eng.score([toks[0] + toks[1]], [(0, 2)], posteriors=True)[0]
    cases = [(per[0], lps[0], toks[0]), (per[1], lps[1], toks[1]), (whole, np.concatenate(lps), toks[0] + toks[1])]
    for got, lp, y in cases:
        T = lp.shape[0]
        assert got["n_frames"] == T and got["n_tokens"] == len(y)
        ref_ll, ref = R.score(lp, y, blank)
        print("T %d L %d loglik %.9g ref %.9g err %.3g" % (T, len(y), got["loglik"], ref_ll, abs(got["loglik"] - ref_ll)))
        assert abs(got["loglik"] - ref_ll) <= 2e-5 * T
        assert np.abs(np.array(got["peak_posterior"]) - ref["peak_post"]).max() <= 2e-3
        assert (np.abs(np.array(got["occupancy"]) - ref["occupancy"]) / ref["occupancy"]).max() <= 2e-3
    fwd = eng.score(toks)
    assert [f["loglik"] for f in fwd] == [p["loglik"] for p in per] and "occupancy" not in fwd[0]


def test_loglik_is_at_least_the_viterbi_score_and_ranks_candidates(encoded):
    eng, toks = encoded
    ali = eng.align(toks)
    sc = eng.score(toks)
    for a, s in zip(ali, sc):
        assert s["loglik"] >= a.score - 1e-5 * s["n_frames"]
    y = list(toks[0])
    wrong = list(y)
    wrong[len(y) // 2] = 1 + (wrong[len(y) // 2] % (eng.cfg.vocab - 2))
    wrong = [t for t in wrong if t != eng.cfg.blank_id]
    both = eng.score([y, wrong], [(0, 1), (0, 1)])                 # two candidate transcripts of the same chunk in one launch
    assert both[0]["loglik"] == sc[0]["loglik"] and both[0]["loglik"] > both[1]["loglik"]


def test_reverb_score_and_align_json(tmp_path, encoded):
    from reverb_amd.reverb import load_model
    mdir = synth.write_model_dir(str(tmp_path / "m"), "tiny")
    wav = str(tmp_path / "a.wav")
    synth.write_wav(wav, synth.synth_audio(30.0, seed=21))
    asr = load_model(mdir, gpu=0, dtype="f32", max_chunks=4)
    text = asr.transcribe(wav, mode="ctc_greedy_search", format="txt")
    out = asr.score(wav, transcript=text)
    assert sorted(out) == ["loglik", "loglik_per_token", "n_frames", "n_tokens", "viterbi_score"]
    assert out["loglik"] >= out["viterbi_score"] - 1e-5 * out["n_frames"] and out["loglik_per_token"] == out["loglik"] / out["n_tokens"]
    full = asr.score(wav, transcript=text, posteriors=True)
    assert sorted(full) == sorted(list(out) + ["occupancy", "mean_time", "peak_posterior"]) and full["loglik"] == out["loglik"]
    assert len(full["occupancy"]) == len(full["mean_time"]) == len(full["peak_posterior"]) == out["n_tokens"]
    assert all(0.0 < p <= 1.0 + 1e-3 for p in full["peak_posterior"])
    # json without posteriors: what align_to_json makes of the engine's alignment, as before; with: three more fields per token
    plain = asr.align(wav, transcript=text, format="json")
    ids = list(asr.tokenizer.tokenize(text)[1])
    res = asr.engine.align([ids], [(0, 2)])[0]
    want = align_to_json(res, asr.tokenizer, CHUNK, asr.input_frame_length, asr.output_frame_length)
    assert json.dumps(plain, ensure_ascii=False, indent=1) == json.dumps(want, ensure_ascii=False, indent=1)
    assert sorted(plain["tokens"][0]) == ["confidence", "end_ms", "id", "piece", "start_ms"]
    rich = asr.align(wav, transcript=text, format="json", posteriors=True)
    assert sorted(rich["tokens"][0]) == ["confidence", "end_ms", "id", "mean_time", "occupancy", "peak_posterior", "piece", "start_ms"]
    for a, b in zip(plain["tokens"], rich["tokens"]):
        assert all(b[k] == a[k] for k in a)
    assert asr.align(wav, transcript=text, format="ctm") == asr.align(wav, transcript=text, format="ctm", posteriors=True)
    with pytest.raises(ValueError):
        asr.score(wav)
