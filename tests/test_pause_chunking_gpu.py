"""Chunks cut at pauses through the engine and the API: Engine.pause_chunks / decode_resident / decode_batch with chunking="pauses",
ReverbASR.transcribe*(chunking="pauses") and recognize_wav --chunking pauses.

The cuts are checked with the replay check of tests/pause_ref.py; everything downstream of the cuts is compared with ==, because a
piece in its chunk slot is exactly the input a host caller would hand to encode(feats, lens): the same rows, the same zero tail, and
chunks do not see each other (test_engine_gpu.py::test_batch_composition_does_not_change_results).

Case("tiny_ln"), max_chunks 4, engine chunk_frames 2051, decode chunk_size 256, search 96, on the 30 s recording and on noise bursts
separated by silence."""
import os
import subprocess
import sys

import numpy as np
import pytest

import pause_ref as P
from conftest import ROOT
from golden_util import Case
from reverb_amd import synth
from reverb_amd._lib import RvbError
from reverb_amd.engine import Engine
from test_transcribe_many_gpu import MODES, _items, _same

pytestmark = pytest.mark.gpu
MAX_CHUNKS, CS, SEARCH, H = 4, 256, 96, 10


@pytest.fixture(scope="module")
def case():
    return Case("tiny_ln")


@pytest.fixture(scope="module")
def audio(case):
    return {"speech": case.pcm, "bursts": P.burst_audio(30.0, 0)}


def _engine(case, dtype):
    return Engine(case.cfg, case.sd, dtype=dtype, device=0, max_chunks=MAX_CHUNKS, chunk_frames=case.chunk, cat_embs=case.cat)


def _slots(feats, starts, lens, cs):
    x = np.zeros((len(starts), cs, 80), np.float32)
    for k, (s, n) in enumerate(zip(starts, lens)):
        x[k, :n] = feats[s:s + n]
    return x


def _host_decode(eng, case, x, lens):
    """the same pieces fed from the host: encode(feats, lens) + search, max_chunks at a time"""
    out = {m: [] for m in MODES}
    for s in range(0, len(lens), MAX_CHUNKS):
        from reverb_amd.engine import joint_topk
        eng.encode(x[s:s + MAX_CHUNKS], lens[s:s + MAX_CHUNKS], case.beam, topk=joint_topk(MODES, case.beam))
        part = eng.search(MODES, case.ctc_weight, case.reverse_weight)
        for m in MODES:
            out[m].extend(part[m])
    return out


def _same_all(got, want):
    for m in MODES:
        assert len(got[m]) == len(want[m]), m
        for a, b in zip(got[m], want[m]):
            _same(a, b)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_pause_chunks_and_resident_decode(case, audio, dtype):
    eng = _engine(case, dtype)
    assert case.chunk == 2051
    for name, pcm in audio.items():
        eng.upload_pcm(pcm)
        nf, feats = eng.fbank(return_feats=True)
        first, starts, lens, packed = eng.pause_chunks(CS, SEARCH, H, return_feats=True)
        P.replay_check(feats, starts, CS, SEARCH, H)
        assert first.tolist() == [0, len(starts)] and lens.tolist() == P.lens_of(starts.tolist(), nf)
        assert len(starts) > MAX_CHUNKS                                  # pieces straddle encodes
        want = _slots(feats, starts, lens, CS)
        assert np.array_equal(packed.view(np.uint32).reshape(want.shape), want.view(np.uint32)), name
        if name == "bursts":
            floor = feats.min()               # the device fbank's own value of a silent bin (an ulp from the oracle's FLOOR)
            assert abs(float(floor) - float(P.FLOOR)) < 2e-6
            for c in starts[1:]:
                assert np.all(feats[c - 10:c + 10] == floor), c
        # a second call with other parameters works from the frame-ordered features that were kept
        _, st2, ln2, pk2 = eng.pause_chunks(64, 16, 1, return_feats=True)
        P.replay_check(feats, st2, 64, 16, 1)
        assert np.array_equal(pk2.view(np.uint32).reshape(-1, 64, 80), _slots(feats, st2, ln2, 64).view(np.uint32))

        got, got_starts = eng.decode_resident(nf, MODES, CS, case.beam, case.ctc_weight, case.reverse_weight, chunking="pauses",
                                              pause_search=SEARCH, pause_smooth=H)
        assert got_starts == starts.tolist()
        _same_all(got, _host_decode(eng, case, want, lens))
        n_tok = {m: sum(len(r.tokens) for r in got[m]) for m in MODES}
        print(name, dtype, len(starts), "pieces, tokens per mode", n_tok)
        if name == "speech":       # the synthetic model's CTC head emits tokens on it; its decoders alone end at once on pieces this short
            assert all(n_tok[m] > 0 for m in MODES[:3]), n_tok
    eng.close()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_a_short_recording_is_the_fixed_chunk(case, dtype):
    eng = _engine(case, dtype)
    eng.upload_pcm(case.pcm[:400 + 160 * 255])                          # 256 frames: one piece
    nf = eng.fbank()
    assert nf == 256
    args = (nf, MODES, CS, case.beam, case.ctc_weight, case.reverse_weight)
    got, starts = eng.decode_resident(*args, chunking="pauses", pause_search=SEARCH)
    assert starts == [0]
    _same_all(got, eng.decode_resident(*args))                           # fixed, after pauses, without a new fbank
    _same_all(got, eng.decode_resident(*args, chunking="fixed"))
    eng.close()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_decode_batch_equals_the_single_decodes(case, dtype):
    items = _items(case)
    eng = _engine(case, dtype)
    args = (MODES, CS, case.beam, case.ctc_weight, case.reverse_weight)
    kw = dict(chunking="pauses", pause_search=SEARCH, pause_smooth=H)
    alone = []
    for wave, rate in items:
        eng.upload_pcm(wave, rate)
        alone.append(eng.decode_resident(eng.fbank(), *args, **kw))
    eng.upload_batch(items)
    got, got_starts = eng.decode_batch(*args, **kw)
    assert len(got) == len(items) == len(got_starts)
    for r, (want, want_starts) in enumerate(alone):
        assert got_starts[r] == want_starts, r
        _same_all(got[r], want)
    assert got[3] == {m: [] for m in MODES} and got_starts[3] == []
    assert sum(map(len, got_starts)) > 2 * MAX_CHUNKS
    # the fixed decode of the same batch afterwards is what it is without the pause decode in between
    fixed = eng.decode_batch(*args)
    eng.upload_batch(items)
    for a, b in zip(fixed, eng.decode_batch(*args)):
        _same_all(a, b)
    eng.close()


def test_state_and_profile(case, audio):
    eng = _engine(case, "f32")
    with pytest.raises(RvbError, match="rvb_pause_chunks: no features are resident"):
        eng.pause_chunks(CS, SEARCH, H)
    with pytest.raises(RvbError, match="rvb_pause_chunks: chunk_size 4000 exceeds"):
        eng.pause_chunks(4000, 96, H)
    modes = ["ctc_greedy_search", "attention_rescoring"]
    args = (modes, case.chunk, case.beam, case.ctc_weight, case.reverse_weight)
    eng.upload_pcm(audio["speech"])
    nf = eng.fbank()
    before = eng.decode_resident(nf, *args)
    eng.set_profiling(True)
    eng.reset_timings()
    _, starts, lens = eng.pause_chunks(CS, SEARCH, H)
    t = eng.timing("pause_chunks")
    assert t["launches"] == 1 and t["ms"] > 0.0
    eng.pause_chunks(CS, 7, 1)
    assert eng.timing("pause_chunks")["launches"] == 2
    eng.set_profiling(False)
    # a capacity that is too small reports the count and leaves everything as it was
    import ctypes as C
    from reverb_amd import _lib
    first, n = np.full(2, -7, np.int64), C.c_int64(0)
    st, ln = np.full(2, -7, np.int32), np.full(2, -7, np.int32)
    rc = eng.lib.rvb_pause_chunks(eng.handle, CS, SEARCH, H, first.ctypes.data_as(_lib._i64p), _lib.iptr(st), _lib.iptr(ln), 2, C.byref(n), None)
    assert rc == -1 and n.value == len(starts) and b"capacity 2 is too small" in eng.lib.rvb_last_error()
    assert np.all(first == -7) and np.all(st == -7) and np.all(ln == -7)
    # a later upload + fbank + fixed decode gives what it gave before: the layout is restored
    eng.upload_pcm(audio["speech"])
    assert eng.fbank() == nf
    for m in modes:
        for a, b in zip(eng.decode_resident(nf, *args)[m], before[m]):
            _same(a, b)
    eng.close()


@pytest.fixture(scope="module")
def files(case, audio, tmp_path_factory):
    d = tmp_path_factory.mktemp("pauses")
    model = str(d / "model")
    synth.write_model_dir(model, "tiny_ln", sd=case.sd, cfg=case.cfg)
    paths = []
    for name, pcm in (("speech", audio["speech"]), ("bursts", audio["bursts"]), ("short", audio["speech"][:300]),
                      ("part", audio["speech"][8000:8000 + 5 * 16000])):
        paths.append(str(d / (name + ".wav")))
        synth.write_wav(paths[-1], pcm, 16000)
    return model, paths


def test_reverb_asr(case, files):
    import reverb_amd
    model, paths = files
    asr = reverb_amd.load_model(model, dtype="f32", max_chunks=MAX_CHUNKS)
    kw = dict(chunk_size=CS, beam_size=case.beam, ctc_weight=case.ctc_weight, format="ctm")
    pk = dict(chunking="pauses", pause_search=SEARCH, pause_smooth=H)
    single = [asr.transcribe(p, mode="attention_rescoring", **kw, **pk) for p in paths]
    assert asr.transcribe_many(paths, mode="attention_rescoring", **kw, **pk) == single
    assert single[2] == "" and len(single[0]) > 0 and len(single[3]) > 0
    modes = ["ctc_prefix_beam_search", "attention_rescoring"]
    assert asr.transcribe_modes_many(paths, modes, **kw, **pk) == [asr.transcribe_modes(p, modes, **kw, **pk) for p in paths]
    # the defaults of the two parameters: search = chunk_size // 4, smooth = 10
    assert asr.transcribe(paths[0], chunking="pauses", **kw) == asr.transcribe(paths[0], chunking="pauses", pause_search=64, pause_smooth=10, **kw)
    # "fixed" is the keyword absent
    fixed = asr.transcribe(paths[0], mode="attention_rescoring", **kw)
    assert asr.transcribe(paths[0], mode="attention_rescoring", chunking="fixed", **kw) == fixed
    assert asr.transcribe_many(paths[:2], mode="attention_rescoring", chunking="fixed", **kw) == \
        asr.transcribe_many(paths[:2], mode="attention_rescoring", **kw)
    assert single[0] != fixed                                            # the cuts moved
    # CTM times follow the pieces: every time lies inside the recording (the arithmetic itself: tests/test_pause_output.py)
    t = [float(line.split()[2]) for line in single[0].split("\n")]
    assert min(t) >= 0.0 and max(t) < 30.0
    for call in (asr.transcribe, lambda p, **k: asr.transcribe_modes(p, modes, **k), lambda p, **k: asr.transcribe_many([p], **k),
                 lambda p, **k: asr.transcribe_modes_many([p], modes, **k)):
        with pytest.raises(NotImplementedError, match="simulate_streaming"):
            call(paths[0], chunking="pauses", simulate_streaming=True, decoding_chunk_size=16, **kw)
    with pytest.raises(ValueError, match="chunking"):
        asr.transcribe(paths[0], chunking="silence", **kw)
    asr.engine.close()


def test_recognize_wav_chunking_pauses(case, files, tmp_path):
    """--chunking pauses with --audio_list in a process of its own against --audio_file runs and against the API"""
    import reverb_amd
    from reverb_amd.bin import recognize_wav
    model, paths = files
    lst = tmp_path / "list.txt"
    lst.write_text("\n".join(paths[:3]) + "\n")
    common = ["--model", model, "--dtype", "f32", "--max_chunks", str(MAX_CHUNKS), "--chunk_size", str(CS), "--modes", "attention_rescoring",
              "--beam_size", str(case.beam), "--ctc_weight", str(case.ctc_weight),
              "--chunking", "pauses", "--pause_search_frames", str(SEARCH), "--pause_smooth_frames", str(H)]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "reverb_amd.bin.recognize_wav", "--audio_list", str(lst), "--result_dir", str(tmp_path / "many")] + common,
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    for p in paths[:3]:
        recognize_wav.main(["--audio_file", p, "--result_dir", str(tmp_path / "single")] + common)
    asr = reverb_amd.load_model(model, dtype="f32", max_chunks=MAX_CHUNKS)
    for p in paths[:3]:
        name = os.path.basename(p).replace(".wav", ".ctm")
        a = (tmp_path / "many" / "attention_rescoring" / name).read_text()
        assert a == (tmp_path / "single" / "attention_rescoring" / name).read_text()
        assert a == asr.transcribe(p, mode="attention_rescoring", format="ctm", chunk_size=CS, beam_size=case.beam, ctc_weight=case.ctc_weight,
                                   chunking="pauses", pause_search=SEARCH, pause_smooth=H)
    asr.engine.close()
