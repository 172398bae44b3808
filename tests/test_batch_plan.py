"""Many recordings in one pass, the parts that need no GPU: the layout rvb_batch_plan gives (include/rvb.h), the refusals of the three
new calls before any device work, reverb.plan_groups and the --audio_list flag of recognize_wav."""
import ctypes as C

import numpy as np
import pytest

from reverb_amd import _lib
from reverb_amd.reverb import plan_groups

p64 = lambda a: a.ctypes.data_as(_lib._i64p)
CAP = 65536


def plan(lib, ns, chunk):
    ns = np.ascontiguousarray(ns, np.int64)
    nf, first = np.full(len(ns), -1, np.int64), np.full(len(ns) + 1, -1, np.int64)
    assert lib.rvb_batch_plan(p64(ns), len(ns), chunk, p64(nf), p64(first), None) == 0, lib.rvb_last_error()
    lens = np.full(max(int(first[-1]), 1), -1, np.int32)
    nf2, first2 = np.empty_like(nf), np.empty_like(first)
    assert lib.rvb_batch_plan(p64(ns), len(ns), chunk, p64(nf2), p64(first2), _lib.iptr(lens)) == 0
    assert np.array_equal(nf, nf2) and np.array_equal(first, first2)
    return nf, first, lens[:int(first[-1])]


@pytest.mark.parametrize("chunk", [7, 16, 2051])
def test_batch_plan_against_a_numpy_restatement(lib, chunk):
    rng = np.random.default_rng(5)
    ns = np.concatenate([[0, 399, 400, 559, 560, 400 + 160 * (3 * chunk + 4)], rng.integers(0, 400 + 160 * 3 * chunk, 200)]).astype(np.int64)
    nf, first, lens = plan(lib, ns, chunk)
    want_nf = np.where(ns < 400, 0, 1 + (ns - 400) // 160)          # Kaldi snip_edges, per recording
    assert np.array_equal(nf, want_nf) and nf[:6].tolist() == [0, 0, 1, 1, 2, 3 * chunk + 5]
    want_chunks = -(-want_nf // chunk)
    assert first[0] == 0 and np.array_equal(np.diff(first), want_chunks)
    assert np.all(np.diff(first) >= 0) and first[0] == first[1] == first[2]      # frameless recordings: equal neighbours
    assert len(lens) == first[-1] and lens.min() >= 1 and lens.max() <= chunk
    for r in range(len(ns)):
        mine = lens[first[r]:first[r + 1]]
        assert mine.sum() == nf[r]
        assert np.all(mine[:-1] == chunk)                            # only a recording's last chunk holds a remainder
    assert lens[first[5]:first[6]].tolist() == [chunk] * 3 + [5]


def _msg(lib):
    return lib.rvb_last_error().decode()


def test_batch_plan_refusals(lib):
    ns, nf, first = np.array([400], np.int64), np.zeros(1, np.int64), np.zeros(2, np.int64)
    for args in ((None, 1, 7, p64(nf), p64(first), None), (p64(ns), 1, 7, None, p64(first), None), (p64(ns), 1, 7, p64(nf), None, None)):
        assert lib.rvb_batch_plan(*args) == -1 and "rvb_batch_plan" in _msg(lib) and "null" in _msg(lib)
    for n in (0, -1):
        assert lib.rvb_batch_plan(p64(ns), n, 7, p64(nf), p64(first), None) == -1 and "n_rec" in _msg(lib)
    assert lib.rvb_batch_plan(p64(ns), CAP + 1, 7, p64(nf), p64(first), None) == -5 and "65536" in _msg(lib)
    assert lib.rvb_batch_plan(p64(ns), 1, 6, p64(nf), p64(first), None) == -1 and "chunk_size" in _msg(lib)
    neg = np.array([-1], np.int64)
    assert lib.rvb_batch_plan(p64(neg), 1, 7, p64(nf), p64(first), None) == -1 and "negative" in _msg(lib)
    big = np.full(CAP, 560, np.int64)                                # the cap itself is taken
    nfb, fb = np.zeros(CAP, np.int64), np.zeros(CAP + 1, np.int64)
    assert lib.rvb_batch_plan(p64(big), CAP, 7, p64(nfb), p64(fb), None) == 0 and fb[-1] == CAP


def test_upload_batch_refuses_its_arguments_before_any_device_work(lib):
    """Every argument is checked before the engine is looked at, so a NULL engine shows that no device work came first."""
    pcm = np.zeros(800, np.int16)
    data = (C.c_void_p * 1)(pcm.ctypes.data)
    fmt, ns, rate = np.array([2], np.int32), np.array([800], np.int64), np.array([16000], np.int32)
    call = lambda d=data, f=fmt, n=ns, r=rate, k=1: lib.rvb_upload_batch(None, d, None if f is None else _lib.iptr(f), None if n is None else p64(n),
                                                                         None if r is None else _lib.iptr(r), k)
    assert call() == -1 and "null engine" in _msg(lib)               # everything else was in order
    for kw in (dict(d=None), dict(f=None), dict(n=None), dict(r=None)):
        assert call(**kw) == -1 and "null argument" in _msg(lib)
    for k in (0, -3):
        assert call(k=k) == -1 and "n_rec" in _msg(lib)
    assert call(k=CAP + 1) == -5 and "65536" in _msg(lib)
    for bad in (1, 3, 5, 0):                                         # U8, I32, F64, nothing
        assert call(f=np.array([bad], np.int32)) == -1 and "sample_format" in _msg(lib) and "recording 0" in _msg(lib)
    assert call(n=np.array([-1], np.int64)) == -1 and "negative" in _msg(lib)
    for bad in (999, 384001, 0, -16000):
        assert call(r=np.array([bad], np.int32)) == -1 and "sample_rate" in _msg(lib)
    assert call(d=(C.c_void_p * 1)(None)) == -1 and "null pointer" in _msg(lib)
    out = np.zeros(1, np.int64)
    assert lib.rvb_batch_n_samples(None, p64(out)) == -1 and "rvb_batch_n_samples" in _msg(lib)


def test_fbank_batch_refuses_its_arguments_before_any_device_work(lib):
    nf, first = np.zeros(1, np.int64), np.zeros(2, np.int64)
    assert lib.rvb_fbank_batch(None, 6, None, p64(nf), p64(first)) == -1 and "chunk_size" in _msg(lib)
    assert lib.rvb_fbank_batch(None, 7, None, p64(nf), p64(first)) == -1 and "null" in _msg(lib)


def test_fbank_batch_hook_refuses_before_any_device_work(lib):
    pcm = np.zeros(800, np.int16)
    data = (C.c_void_p * 2)(pcm.ctypes.data, pcm.ctypes.data)
    fmt, ns = np.array([2, 2], np.int32), np.array([800, 800], np.int64)
    out = np.zeros((2 * 7 + 4) * 80, np.float32)
    off = np.array([0, 799], np.int64)                               # the second recording would overlap the first
    assert lib.rvb_test_fbank_batch(data, _lib.iptr(fmt), p64(ns), p64(off), 2, 7, _lib.fptr(out)) == -1 and "overlap" in _msg(lib)
    assert lib.rvb_test_fbank_batch(data, _lib.iptr(fmt), p64(ns), None, 2, 6, _lib.fptr(out)) == -1


def test_plan_groups():
    assert plan_groups([], 10.0) == []
    d = [3.0, 4.0, 5.0, 30.0, 1.0, 1.0, 9.0, 0.0, 10.0, 0.5]
    g = plan_groups(d, 10.0)
    assert [i for grp in g for i in grp] == list(range(len(d)))      # order kept, every index exactly once
    for grp in g:
        assert grp and (sum(d[i] for i in grp) <= 10.0 or len(grp) == 1)
    assert g == [[0, 1], [2], [3], [4, 5], [6, 7], [8], [9]]
    assert plan_groups([1.0] * 5, 3600.0) == [[0, 1, 2, 3, 4]]
    rng = np.random.default_rng(0)
    d = rng.uniform(0.0, 50.0, 300).tolist()
    g = plan_groups(d, 60.0)
    assert [i for grp in g for i in grp] == list(range(300))
    assert all(sum(d[i] for i in grp) <= 60.0 or len(grp) == 1 for grp in g)
    for a, b in zip(g, g[1:]):                                       # greedy: the next recording did not fit
        assert sum(d[i] for i in a) + d[b[0]] > 60.0


def test_recognize_wav_argument_parsing(tmp_path, capsys):
    from reverb_amd.bin import recognize_wav as R
    base = ["--model", "m", "--result_dir", "o"]
    a = R.get_args(base + ["--audio_file", "a.wav"])
    assert a.audio_file == "a.wav" and a.audio_list is None and a.audio_files is None and a.modes == ["attention_rescoring"]
    assert a.chunk_size == 2051 and a.beam_size == 10
    lst = tmp_path / "list.txt"
    lst.write_text("# calls of Monday\n/x/a.wav\n\n  /y/b.flac  \n#/z/c.wav\n")
    a = R.get_args(base + ["--audio_list", str(lst)])
    assert a.audio_file is None and a.audio_files == ["/x/a.wav", "/y/b.flac"]
    for argv in (base, base + ["--audio_file", "a.wav", "--audio_list", str(lst)]):
        with pytest.raises(SystemExit):
            R.get_args(argv)
        assert "exactly one" in capsys.readouterr().err
    lst.write_text("/x/a.wav\n/y/a.flac\n")
    with pytest.raises(SystemExit):
        R.get_args(base + ["--audio_list", str(lst)])
    assert "a.ctm" in capsys.readouterr().err
    with pytest.raises(ValueError, match="a.ctm"):
        R.read_audio_list(str(lst))
    import wenet.bin.recognize_wav as W
    assert W.get_args is R.get_args
