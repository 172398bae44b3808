"""Long-form full-sum scoring through the engine (rvb_ctc_score_long_* / Engine.score_long_* / ReverbASR.score(long_form=...)) on the
synthetic "tiny" model: one full-sum lattice over several encoded batches.

Bounds: |loglik - reference| <= 1e-5 * T and the posterior tolerances of tests/test_ctc_score_window_gpu.py, which derive them.  Where
the window holds the whole lattice and ONE batch holds the file, the long calls must give Engine.score's bits."""
import json
import logging

import numpy as np
import pytest

from reverb_amd import synth
from reverb_amd._lib import RvbError
from test_align_engine_gpu import CHUNK, LONG_SECONDS, LONG_SEED, engine, feats_of
from test_align_long_engine_gpu import align_long, batches, greedy_transcript
from test_ctc_score_window_gpu import LL_PER_FRAME, TOL_MEAN, TOL_OCC, TOL_POST

pytestmark = pytest.mark.gpu


def score_long(eng, lens, mc, tokens, window_states=0, posteriors=True, between=None):
    """-> (loglik, per-token dict or None, window)"""
    enc = [(int(n) - 7) // 4 + 1 for n in lens]
    used = eng.score_long_begin(tokens, sum(enc), window_states, posteriors)
    starts = []
    for c0 in batches(eng, lens, mc):
        starts.append(c0)
        eng.score_long_feed()
        if between:
            between()
    ll = eng.score_long_loglik()
    post = None
    if posteriors:
        for c0 in reversed(starts):
            eng.encode(None, lens[c0:c0 + mc], 2, 0.0, first_chunk=c0, T0=CHUNK)
            eng.score_long_feed_back()
        post = eng.score_long_finish()
    eng.score_long_end()
    return ll, post, used


def close_to(got, ref, T):
    (ll, post), (rll, rpost) = got, ref
    assert abs(ll - rll) <= LL_PER_FRAME * T
    occ, rocc = np.array(post["occupancy"]), np.array(rpost["occupancy"])
    mean, rmean = np.array(post["mean_frame"]), np.array(rpost["mean_frame"])
    e_post = np.abs(np.array(post["peak_posterior"]) - np.array(rpost["peak_posterior"])).max()
    e_occ = (np.abs(occ - rocc) / rocc).max()
    e_mean = (np.abs(mean - rmean) / np.maximum(rmean, 1.0)).max()
    print("loglik %.9g vs %.9g, peak_post %.3g occupancy %.3g mean_frame %.3g" % (ll, rll, e_post, e_occ, e_mean))
    assert e_post <= TOL_POST and e_occ <= TOL_OCC and e_mean <= TOL_MEAN


def test_one_batch_gives_score_bits_and_three_batches_agree():
    pcm = synth.synth_audio(50.0, seed=21)
    eng = engine("tiny", "f32", max_chunks=3)
    lens = feats_of(eng, pcm)
    assert len(lens) == 3
    tokens = greedy_transcript(eng, lens, 3)
    assert tokens, "the synthetic model emitted nothing"
    T = sum((int(n) - 7) // 4 + 1 for n in lens)
    ll, post, used = score_long(eng, lens, 3, tokens)
    assert used == (2 * len(tokens) + 1 + 31) // 32 * 32
    eng.encode(None, lens, 2, 0.0, first_chunk=0, T0=CHUNK)
    one = eng.score([tokens], [(0, 3)], posteriors=True)[0]
    assert ll == one["loglik"], "loglik differs from Engine.score's on one batch"
    for key in ("occupancy", "mean_frame", "peak_posterior", "peak_frame"):
        assert post[key] == one[key], key + " differs from Engine.score's on one batch"
    assert score_long(eng, lens, 3, tokens, posteriors=False)[0] == ll
    eng.close()
    eng = engine("tiny", "f32", max_chunks=1)
    lens = feats_of(eng, pcm)
    ll3, post3, _ = score_long(eng, lens, 1, tokens)
    close_to((ll3, post3), (one["loglik"], one), T)
    eng.close()


def test_a_small_window_on_24_chunks():
    eng = engine("tiny", "f32", max_chunks=5)
    lens = feats_of(eng, synth.synth_audio(LONG_SECONDS, seed=LONG_SEED))
    assert len(lens) == 24
    tokens = greedy_transcript(eng, lens, 5)
    T = sum((int(n) - 7) // 4 + 1 for n in lens)
    assert 2 * len(tokens) + 1 > 256 + 64, "the lattice is wider than the small window"
    vit = align_long(eng, lens, 5, tokens)[0].score
    wide, _, _ = score_long(eng, lens, 5, tokens, posteriors=False)
    small, post, used = score_long(eng, lens, 5, tokens, 256)
    print("T %d L %d loglik wide %.6f small %.6f viterbi %.6f" % (T, len(tokens), wide, small, vit))
    assert used == 256
    assert small <= wide + LL_PER_FRAME * T
    assert small >= vit - LL_PER_FRAME * T, "the policy lost the best path"
    assert sum(post["occupancy"]) <= T * (1 + TOL_OCC)
    eng.close()


def test_order_errors_and_independence():
    eng = engine("tiny", "f32", max_chunks=2)
    with pytest.raises(RvbError, match=r"\(-3\).*rvb_ctc_score_long_feed before rvb_ctc_score_long_begin"):
        eng.score_long_feed()
    lens = feats_of(eng, synth.synth_audio(50.0, seed=21))
    modes = ["ctc_greedy_search", "ctc_prefix_beam_search"]
    tokens = greedy_transcript(eng, lens, 2)
    total = sum((int(n) - 7) // 4 + 1 for n in lens)
    with pytest.raises(RvbError, match="window_states 300 must be 0"):
        eng.score_long_begin(tokens, total, 300)
    with pytest.raises(RvbError, match=r"\(-3\).*before rvb_ctc_score_long_begin"):      # a refused begin leaves nothing open
        eng.score_long_feed()
    plain = score_long(eng, lens, 2, tokens)
    ref_align = align_long(eng, lens, 2, tokens)[0]
    eng.score_long_begin(tokens, total, 0, False)
    eng.encode(None, lens[:2], 2, 0.0, first_chunk=0, T0=CHUNK)
    eng.score_long_feed()
    with pytest.raises(RvbError, match=r"\(-3\).*loglik before all %d frames were fed" % total):
        eng.score_long_loglik()
    eng.encode(None, lens[2:], 2, 0.0, first_chunk=2, T0=CHUNK)
    eng.score_long_feed()
    assert eng.score_long_loglik() == plain[0]
    with pytest.raises(RvbError, match=r"\(-3\).*without posteriors"):
        eng.score_long_feed_back()
    # ascending batches in the backward sweep: the first batch is not the one the forward sweep saw last
    eng.score_long_begin(tokens, total, 0, True)
    for c0 in batches(eng, lens, 2):
        eng.score_long_feed()
    eng.score_long_loglik()
    eng.encode(None, lens[:2], 2, 0.0, first_chunk=0, T0=CHUNK)
    with pytest.raises(RvbError, match=r"\(-3\).*descending order: expected batch 1"):
        eng.score_long_feed_back()
    eng.score_long_end()
    # a long alignment and a search interleaved between begin and finish change nothing
    eng.encode(None, lens[:2], 4, 0.0, first_chunk=0, T0=CHUNK)
    before = eng.search(modes, 0.1, 0.0)
    enc = [(int(n) - 7) // 4 + 1 for n in lens]
    eng.align_long_begin(tokens, total)
    eng.score_long_begin(tokens, total, 0, True)
    for c0 in (0, 2):
        eng.encode(None, lens[c0:c0 + 2], 4, 0.0, first_chunk=c0, T0=CHUNK)
        eng.align_long_feed()
        found = eng.search(modes, 0.1, 0.0)
        eng.score_long_feed()
        if c0 == 0:
            for m in modes:
                assert [r.tokens for r in found[m]] == [r.tokens for r in before[m]]
    labels, _, _, score, _ = eng.align_long_finish()
    ll = eng.score_long_loglik()
    for c0 in (2, 0):
        eng.encode(None, lens[c0:c0 + 2], 2, 0.0, first_chunk=c0, T0=CHUNK)
        eng.score_long_feed_back()
    post = eng.score_long_finish()
    eng.align_long_end()
    eng.score_long_end()
    assert ll == plain[0] and post == plain[1]
    assert labels.tolist() == ref_align.labels and np.float32(score).tobytes() == np.float32(ref_align.score).tobytes()
    eng.close()


def test_front_end(tmp_path, caplog):
    from reverb_amd.bin import align_wav
    from reverb_amd.reverb import load_model
    mdir = synth.write_model_dir(str(tmp_path / "m"), "tiny")
    wav = str(tmp_path / "three.wav")
    synth.write_wav(wav, synth.synth_audio(50.0, seed=21))
    whole = load_model(mdir, gpu=0, dtype="f32", max_chunks=3)
    text = " ".join(whole.transcribe(wav, mode="ctc_greedy_search", format="txt").split())      # leaves the file resident
    assert text
    n = whole.engine.fbank()
    nl = np.full(3, CHUNK, np.int32); nl[-1] = n - 2 * CHUNK
    whole.engine.encode(None, nl, 2, 0.0, T0=CHUNK)
    tokens = [t for g in whole.engine.greedy() for t in g.tokens]
    want = whole.score(wav, tokens=tokens, posteriors=True)
    assert "window_states" not in want                           # today's path, untouched
    whole.engine.close()
    two = load_model(mdir, gpu=0, dtype="f32", max_chunks=2)
    got = two.score(wav, tokens=tokens, posteriors=True)
    assert set(got) == set(want) | {"window_states", "window_margin"}
    T = want["n_frames"]
    assert got["n_frames"] == T and got["n_tokens"] == len(tokens)
    assert abs(got["loglik"] - want["loglik"]) <= LL_PER_FRAME * T
    assert got["window_states"] == (2 * len(tokens) + 1 + 31) // 32 * 32 == got["window_margin"]
    assert len(got["occupancy"]) == len(tokens) and np.abs(np.array(got["occupancy"]) - np.array(want["occupancy"])).max() <= 1e-2
    with pytest.raises(ValueError, match="max_chunks"):
        two.score(wav, tokens=tokens, long_form=False)
    with pytest.raises(ValueError, match="attention"):
        two.score(wav, tokens=tokens, attention=True)
    assert not [r for r in caplog.records if r.levelno >= logging.WARNING and "window_tokens" in r.getMessage()]
    two.engine.close()
    tfile = tmp_path / "three.txt"
    tfile.write_text(text, encoding="utf-8")
    out = tmp_path / "out"
    base = ["--model", mdir, "--audio_file", wav, "--transcript_file", str(tfile), "--result_dir", str(out), "--dtype", "f32",
            "--max_chunks", "2", "--format", "json"]
    align_wav.main(base + ["--long_form", "--score", "--posteriors"])
    sc = json.loads((out / "three.score.json").read_text())
    assert len(sc["occupancy"]) == sc["n_tokens"] and "window_states" in sc
    assert "occupancy" not in json.loads((out / "three.json").read_text())["tokens"][0]
    with pytest.raises(SystemExit):
        align_wav.main(base + ["--long_form", "--alternatives"])
