"""Many recordings in one pass (rvd_upload_pcm_many, rvd_segment_windows, SpeakerDiarization.diarize_many) against each recording
alone, in f32 and bf16, on synthetic weights.

The expectation is identity of bit patterns, not closeness: a window's result does not depend on the batch it is computed in
(tests/test_diar_gpu.py pins that), and the packed layout gives every valid window exactly the samples and zeros it has when its
recording is uploaded alone.  The recordings are cut from one synthetic conversation: 47.3 s (39 windows), 3.2 s (a single padded
window), 10.0 s (a single full window), 12.0 s (three windows, no tail), 10.5 s (a full window and a tail)."""
import io

import numpy as np
import pytest

from reverb_amd import diarization as D
from reverb_amd import synth, synth_diar
from reverb_amd.diar_engine import window_count, window_layout

pytestmark = pytest.mark.gpu

RATE = 16000
CUTS = [(0.0, 47.3), (50.0, 3.2), (55.0, 10.0), (66.0, 12.0), (80.0, 10.5)]      # (start, length) seconds in the conversation
COUNTS = [39, 1, 1, 3, 2]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.shape, a.dtype, a.tobytes()


def rttm(ann):
    buf = io.StringIO()
    ann.write_rttm(buf)
    return buf.getvalue()


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    d = tmp_path_factory.mktemp("diar_many")
    model = synth_diar.write_pipeline_dir(str(d / "pipe"))
    talk = synth_diar.synth_conversation(92.0, seed=3)
    pcms = [np.ascontiguousarray(talk[int(round(a * RATE)):int(round(a * RATE)) + int(round(n * RATE))]) for a, n in CUTS]
    assert [len(p) for p in pcms] == [756800, 51200, 160000, 192000, 168000]
    wavs = []
    for i, p in enumerate(pcms):
        wavs.append(str(d / f"rec{i}.wav"))
        synth.write_wav(wavs[-1], p)
    empty = str(d / "empty.wav")
    synth.write_wav(empty, np.zeros(0, np.int16))
    return model, pcms, wavs, empty


@pytest.fixture(scope="module", params=["f32", "bf16"])
def pipe(request, data):
    p = D.Pipeline.from_pretrained(data[0], dtype=request.param).to("cuda")
    yield p
    p.engine.close()


@pytest.fixture(scope="module")
def alone(pipe, data):
    """Every recording uploaded alone: log-probabilities, classes, the embedding fbank of its first and last window, and the
    embeddings of the items embedding_items_from_classes makes of its classes.  Computed once per dtype, never changed."""
    eng = pipe.engine
    out = []
    for pcm in data[1]:
        W = eng.upload(pcm)
        logp, classes = eng.segment(), eng.segment_classes()
        wi, si, masks = D.embedding_items_from_classes(classes, True, 400, eng.cfg["window_samples"])
        emb = eng.embed(wi.astype(np.int64), masks) if wi.size else np.zeros((0, eng.cfg["emb_dim"]), np.float32)
        out.append(dict(W=W, logp=logp, classes=classes, fb=(eng.emb_fbank(0), eng.emb_fbank(W - 1)), items=(wi, si, masks), emb=emb))
    return out


def _packed_results(eng, first, alone):
    """The same quantities from the packed upload that is resident: per recording, by its global windows."""
    out = []
    for r, a in enumerate(alone):
        gw = first[r] + np.arange(a["W"], dtype=np.int64)
        wi, si, masks = a["items"]
        out.append(dict(logp=eng.segment_windows(gw), classes=eng.segment_classes_windows(gw),
                        fb=(eng.emb_fbank(int(gw[0])), eng.emb_fbank(int(gw[-1]))),
                        emb=eng.embed(first[r] + wi.astype(np.int64), masks) if wi.size else np.zeros((0, eng.cfg["emb_dim"]), np.float32)))
    return out


def _assert_same(got, want, what):
    for r, (g, a) in enumerate(zip(got, want)):
        for key in ("logp", "classes", "emb"):
            assert bits(g[key]) == bits(a[key]), (what, "recording", r, key, int(np.sum(g[key] != a[key])))
        for k in (0, 1):
            assert bits(g["fb"][k]) == bits(a["fb"][k]), (what, "recording", r, "fbank of its first / last window", k)


def test_packed_upload_gives_every_recording_the_results_it_has_alone(pipe, data, alone):
    eng = pipe.engine
    pcms = data[1]
    assert [a["W"] for a in alone] == COUNTS
    assert [eng.num_windows(len(p)) for p in pcms] == [window_count(len(p), 160000, 16000) for p in pcms] == COUNTS
    assert eng.num_windows(0) == window_count(0, 160000, 16000) == 0
    # the layout: with an empty recording in the middle and one at the end, as window_layout states it
    seq = pcms[:2] + [np.zeros(0, np.int16)] + pcms[2:] + [np.zeros(0, np.int16)]
    first, total = eng.upload_many(seq)
    want = window_layout([len(p) for p in seq], 160000, 16000)
    assert first.dtype == np.int64 and list(first) == list(want) == [0, 48, 58, 58, 68, 80, 91]
    assert total == eng.n_windows == 82
    first = np.delete(first, [2, 6])
    packed = _packed_results(eng, first, alone)
    _assert_same(packed, alone, "packed")
    # all valid windows in ONE call, in recording order and in another order: rows follow the list
    gw = np.concatenate([first[r] + np.arange(COUNTS[r], dtype=np.int64) for r in range(len(pcms))])
    cls = eng.segment_classes_windows(gw)
    assert bits(cls) == bits(np.concatenate([a["classes"] for a in alone]))
    perm = np.random.default_rng(0).permutation(len(gw))
    assert bits(eng.segment_classes_windows(gw[perm])) == bits(cls[perm])
    # the front end again from the resident samples: the packed results again
    assert eng.rerun_resident() == 82
    _assert_same(_packed_results(eng, first, alone), alone, "rerun_resident")
    # indices outside the layout are refused before anything runs
    from reverb_amd._lib import RvbError
    for bad in ([82], [-1], [0, 5, 82]):
        with pytest.raises(RvbError, match="outside the uploaded audio"):
            eng.segment_windows(np.array(bad, np.int64))
    # a plain upload afterwards: a single recording again
    assert eng.upload(pcms[3]) == 3 == eng.n_windows
    assert bits(eng.segment()) == bits(alone[3]["logp"])
    assert bits(eng.emb_fbank(2)) == bits(alone[3]["fb"][1])
    with pytest.raises(RvbError, match="outside the uploaded audio"):
        eng.segment_windows(np.array([3], np.int64))
    # nothing but empty recordings: no audio resident, nothing to rerun
    first0, total0 = eng.upload_many([np.zeros(0, np.int16)])
    assert list(first0) == [0] and total0 == 0
    with pytest.raises(RvbError, match="upload audio first"):
        eng.rerun_resident()


def test_diarize_many_equals_the_loop(pipe, data):
    _, pcms, wavs, empty = data
    loop = [pipe(w) for w in wavs]
    want = [rttm(a) for a in loop]
    print("turns per recording:", [t.count("\n") for t in want])
    assert any(want)                                                 # the synthetic model does find turns
    got = pipe.diarize_many(wavs)
    assert [a.uri for a in got] == [f"rec{i}" for i in range(len(wavs))]
    assert [rttm(a) for a in got] == want
    t = pipe.timings
    assert t["windows"] == sum(COUNTS) and t["recordings"] == len(wavs) and t["groups"] == 1 and 0 < t["embeddings"] <= 3 * sum(COUNTS)
    for key in ("upload", "segmentation", "embedding", "linkage", "total"):
        assert t[key] > 0.0, key
    # two groups (60 s of audio hold the first two recordings, the other three follow): the same strings
    assert [rttm(a) for a in pipe.diarize_many(wavs, group_seconds=60.0)] == want
    assert pipe.timings["groups"] == 2
    # a zero-sample file between the others: an empty annotation, the neighbours unchanged
    mixed = pipe.diarize_many(wavs[:2] + [empty] + wavs[2:])
    assert mixed[2].uri == "empty" and len(mixed[2]) == 0 and rttm(mixed[2]) == ""
    assert [rttm(a) for a in mixed[:2] + mixed[3:]] == want
    # per-file speaker numbers
    ns = [2, None, 1, 2, None]
    want_ns = [rttm(pipe(w, num_speakers=k)) for w, k in zip(wavs, ns)]
    assert [rttm(a) for a in pipe.diarize_many(wavs, num_speakers=ns)] == want_ns
    assert [rttm(a) for a in pipe.diarize_many(wavs, max_speakers=2)] == [rttm(pipe(w, max_speakers=2)) for w in wavs]
    with pytest.raises(ValueError, match="num_speakers"):
        pipe.diarize_many(wavs, num_speakers=[2, 2])
    # centroids come back as from the single call
    pairs = pipe.diarize_many(wavs + [empty], return_embeddings=True)
    for w, (ann, cen), text in zip(wavs, pairs, want):
        a1, c1 = pipe(w, return_embeddings=True)
        assert rttm(ann) == text == rttm(a1)
        assert bits(cen) == bits(c1)
    assert len(pairs[-1][0]) == 0 and pairs[-1][1].shape == (0, pipe.cfg["emb_dim"])
    # waveform dictionaries go through _load as in __call__
    import torch
    files = [{"waveform": torch.from_numpy(p.astype(np.float32) / 32768.0)[None], "sample_rate": RATE, "uri": f"rec{i}"}
             for i, p in enumerate(pcms)]
    assert [rttm(a) for a in pipe.diarize_many(files)] == want


def test_cli_audio_list_writes_what_the_positional_form_writes(data, tmp_path):
    model, _, wavs, _ = data
    from reverb_amd.bin import infer_pyannote3
    infer_pyannote3.main(wavs + ["--out-dir", str(tmp_path / "a"), "--pipeline-model", model])
    lst = tmp_path / "files.txt"
    lst.write_text("\n".join(wavs[:3]) + "\n\n" + "\n".join(wavs[3:]) + "\n")
    infer_pyannote3.main(["--audio-list", str(lst), "--out-dir", str(tmp_path / "b"), "--pipeline-model", model])
    for i in range(len(wavs)):
        a, b = (tmp_path / "a" / f"rec{i}.rttm").read_text(), (tmp_path / "b" / f"rec{i}.rttm").read_text()
        assert a == b
    assert any((tmp_path / "a" / f"rec{i}.rttm").read_text() for i in range(len(wavs)))
    with pytest.raises(SystemExit):
        infer_pyannote3.main(["--out-dir", str(tmp_path / "c"), "--pipeline-model", model])
