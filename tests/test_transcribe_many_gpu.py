"""Many recordings in one pass on the device: Engine.upload_batch / fbank_batch / decode_batch against the single-recording calls on
the same engine, ReverbASR.transcribe_modes_many against transcribe_modes, and recognize_wav --audio_list against --audio_file.
Everything is compared with == : the batch gives each recording the frames, chunks and padding it has alone, and chunks do not see
each other (test_engine_gpu.py::test_batch_composition_does_not_change_results), so there is no tolerance to state.

The five items are cut from Case("tiny_ln").pcm (30 s; chunk_size = case.chunk = 2051 frames, max_chunks = 4): an int16 piece of 1.3
chunks (chunks 0-1), a float32 piece (chunk 2), an int16 piece labelled 8 kHz that the device resampler doubles to two chunks (chunks
3-4: it straddles the two encodes), a 300-sample piece without a frame, and the whole recording (chunks 5-6)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from golden_util import Case
from reverb_amd import synth
from reverb_amd._lib import RvbError
from reverb_amd.engine import Engine

pytestmark = pytest.mark.gpu
MODES = ["ctc_greedy_search", "ctc_prefix_beam_search", "attention_rescoring", "attention", "joint_decoding"]
MAX_CHUNKS = 4


@pytest.fixture(scope="module")
def case():
    return Case("tiny_ln")


def _items(case):
    pcm = case.pcm
    n13 = 400 + 160 * (int(1.3 * case.chunk) - 1)
    return [(pcm[:n13], 16000),
            (pcm[16000:16000 + 8 * 16000].astype(np.float32) * np.float32(0.731), 16000),
            (np.ascontiguousarray(pcm[3000:3000 + 12 * 16000]), 8000),
            (np.ascontiguousarray(pcm[5000:5300]), 16000),
            (pcm, 16000)]


def _same(a, b):
    assert list(a.tokens) == list(b.tokens)
    assert a.times == b.times and a.ctc_frames == b.ctc_frames and a.end_times == b.end_times
    assert a.tokens_confidence == b.tokens_confidence
    assert a.score == b.score and a.confidence == b.confidence
    assert a.nbest == b.nbest and a.nbest_scores == b.nbest_scores and a.nbest_times == b.nbest_times


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_engine_batch_equals_the_single_calls(case, dtype):
    items = _items(case)
    chunk = case.chunk
    eng = Engine(case.cfg, case.sd, dtype=dtype, device=0, max_chunks=MAX_CHUNKS, chunk_frames=chunk, cat_embs=case.cat)
    args = (MODES, chunk, case.beam, case.ctc_weight, case.reverse_weight)
    alone = []
    for wave, rate in items:
        eng.upload_pcm(wave, rate)
        nf, feats = eng.fbank(return_feats=True)
        alone.append((nf, feats, eng.decode_resident(nf, *args)))
    n16 = eng.upload_batch(items)
    assert n16.tolist() == [len(items[0][0]), len(items[1][0]), 2 * len(items[2][0]), 300, len(items[4][0])]
    nfr, first, feats = eng.fbank_batch(chunk, return_feats=True)
    assert nfr.tolist() == [a[0] for a in alone] and nfr[3] == 0
    assert first.tolist() == [0, 2, 3, 5, 5, 7] and first[-1] > MAX_CHUNKS          # recording 2 straddles the two encodes
    live = np.zeros(len(feats), bool)
    for r, (nf, want, _) in enumerate(alone):
        r0 = int(first[r]) * chunk
        assert np.array_equal(feats[r0:r0 + nf].view(np.uint32), want.view(np.uint32)), "features of recording %d" % r
        live[r0:r0 + nf] = True
    assert np.all(feats[~live].view(np.uint32) == 0)
    got = eng.decode_batch(*args)
    assert len(got) == len(items)
    for r, (_, _, want) in enumerate(alone):
        for m in MODES:
            assert len(got[r][m]) == len(want[m]) == first[r + 1] - first[r], (r, m)
            for a, b in zip(got[r][m], want[m]):
                _same(a, b)
    assert got[3] == {m: [] for m in MODES}
    eng.close()


def test_state_and_profile(case):
    items = _items(case)
    chunk = case.chunk
    eng = Engine(case.cfg, case.sd, dtype="f32", device=0, max_chunks=MAX_CHUNKS, chunk_frames=chunk, cat_embs=case.cat)
    with pytest.raises(RvbError, match="rvb_upload_batch"):
        eng.fbank_batch(chunk)                              # nothing uploaded as a batch
    eng.upload_pcm(*items[0])
    nf = eng.fbank()
    before = eng.decode_resident(nf, ["ctc_greedy_search"], chunk, case.beam, 0.0, 0.0)["ctc_greedy_search"]
    with pytest.raises(RvbError, match="rvb_upload_batch"):
        eng.fbank_batch(chunk)                              # a single upload is no batch
    eng.set_profiling(True)
    eng.reset_timings()
    encodes = []
    encode = eng.encode
    eng.encode = lambda *a, **k: (encodes.append(1), encode(*a, **k))[1]
    eng.upload_batch(items)
    got = eng.decode_batch(["ctc_greedy_search"], chunk, case.beam, 0.0, 0.0)
    assert eng.timing("fbank")["launches"] == 1 and eng.timing("fbank")["ms"] > 0.0
    assert eng.timing("resample")["launches"] == 1
    assert len(encodes) == -(-7 // MAX_CHUNKS) == 2
    eng.set_profiling(False)
    with pytest.raises(RvbError, match="rvb_fbank_batch"):
        eng.fbank()                                         # the engine holds a batch
    with pytest.raises(RvbError, match="rvb_get_waveform"):
        eng.waveform()
    eng.upload_pcm(*items[0])                               # a single upload replaces the batch
    assert eng.fbank() == nf
    after = eng.decode_resident(nf, ["ctc_greedy_search"], chunk, case.beam, 0.0, 0.0)["ctc_greedy_search"]
    assert [list(r.tokens) for r in after] == [list(r.tokens) for r in before] == [list(r.tokens) for r in got[0]["ctc_greedy_search"]]
    assert any(len(r.tokens) for r in after)
    eng.close()


@pytest.fixture(scope="module")
def files(case, tmp_path_factory):
    """(model directory, the five items as WAVE files): the float item is written as int16 PCM, which is what a WAVE file of it holds"""
    d = tmp_path_factory.mktemp("many")
    model = str(d / "model")
    synth.write_model_dir(model, "tiny_ln", sd=case.sd, cfg=case.cfg)
    paths = []
    for i, (wave, rate) in enumerate(_items(case)):
        paths.append(str(d / ("rec%d.wav" % i)))
        synth.write_wav(paths[-1], np.asarray(wave).astype(np.int16), rate)
    return model, paths


def test_transcribe_many_equals_transcribe(case, files):
    import reverb_amd
    model, paths = files
    asr = reverb_amd.load_model(model, dtype="f32", max_chunks=MAX_CHUNKS)
    kw = dict(chunk_size=case.chunk, beam_size=case.beam, ctc_weight=case.ctc_weight)
    ctm_modes = [m for m in MODES if m != "attention"]           # `attention` carries no times: text only
    for fmt, modes in (("ctm", ctm_modes), ("txt", MODES)):
        want = [asr.transcribe_modes(p, modes, format=fmt, **kw) for p in paths]
        many = asr.transcribe_modes_many(paths, modes, format=fmt, **kw)
        assert many == want
        assert many[3] == [""] * len(modes) and any(len(s) > 0 for s in many[4])
        # three groups under a budget of 50 s (26.7 + 8 | 24 + 0.02 | 30), each loaded ahead on two threads: the same strings
        assert asr.transcribe_modes_many(paths, modes, format=fmt, group_seconds=50.0, load_threads=2, **kw) == want
    gone = os.path.join(os.path.dirname(paths[0]), "not_there.wav")
    mixed = paths[:2] + [gone] + paths[2:]
    got = asr.transcribe_modes_many(mixed, ctm_modes, format="ctm", errors="skip", **kw)
    assert got[2] is None and got[:2] + got[3:] == want_ctm(asr, paths, ctm_modes, kw)
    with pytest.raises(OSError, match="not_there.wav"):
        asr.transcribe_modes_many(mixed, ctm_modes, format="ctm", **kw)
    assert asr.transcribe_many(paths[:1], mode="attention_rescoring", format="ctm", **kw) == \
        [asr.transcribe(paths[0], mode="attention_rescoring", format="ctm", **kw)]
    with pytest.raises(NotImplementedError, match="transcribe"):
        asr.transcribe_modes_many(paths, ctm_modes, simulate_streaming=True, **kw)
    # (waveform, rate) pairs: the strings of the files, under the pair's index as its CTM name
    pairs = [(np.asarray(w).astype(np.int16), r) for w, r in _items(case)]
    by_pair = asr.transcribe_modes_many(pairs, ["attention_rescoring"], format="ctm", **kw)
    by_path = asr.transcribe_modes_many(paths, ["attention_rescoring"], format="ctm", **kw)
    assert [s[0].replace("rec%d.wav" % i, str(i)) for i, s in enumerate(by_path)] == [s[0] for s in by_pair]
    asr.engine.close()


def want_ctm(asr, paths, modes, kw):
    return [asr.transcribe_modes(p, modes, format="ctm", **kw) for p in paths]


def test_recognize_wav_audio_list(case, files, tmp_path):
    """--audio_list in a process of its own (the console entry) against --audio_file runs of the same entry point"""
    from reverb_amd.bin import recognize_wav
    model, paths = files
    three = [paths[0], paths[3], paths[2]]
    lst = tmp_path / "list.txt"
    lst.write_text("# three of the five\n" + "\n".join(three) + "\n\n")
    modes = ["ctc_prefix_beam_search", "attention_rescoring"]
    common = ["--model", model, "--dtype", "f32", "--max_chunks", str(MAX_CHUNKS), "--chunk_size", str(case.chunk), "--modes"] + modes
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "reverb_amd.bin.recognize_wav", "--audio_list", str(lst), "--result_dir", str(tmp_path / "many")] + common,
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    for p in three:
        recognize_wav.main(["--audio_file", p, "--result_dir", str(tmp_path / "single")] + common)
    for m in modes:
        assert sorted(os.listdir(tmp_path / "many" / m)) == sorted(os.listdir(tmp_path / "single" / m)) == ["rec0.ctm", "rec2.ctm", "rec3.ctm"]
        for name in os.listdir(tmp_path / "many" / m):
            a, b = (tmp_path / "many" / m / name).read_text(), (tmp_path / "single" / m / name).read_text()
            assert a == b and (len(a) > 0) == (name != "rec3.ctm")
