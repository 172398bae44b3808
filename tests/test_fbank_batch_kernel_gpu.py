"""fbank_batch_kernel (csrc/fbank.hip: the segmented fbank behind rvb_fbank_batch) through the lab hook rvb_test_fbank_batch, against
fbank_kernel on each recording alone (rvb_test_fbank_ex, itself held to its fp64 interval by test_fbank_kernels_gpu.py): the rows of
every recording are the same BITS, every padding row is exactly zero, and the four sentinel rows behind the last chunk keep their
all-ones bytes.

The recordings are cut from fbank_bound_ref.inputs().  Case "middle" has the frame counts 1, 2, 0 (399 samples), 3, 5, 0 (no sample),
4, 1, 37, 7: the recording boundaries fall at frames 1, 3, 6, 11, 15, 16, 53 -- at every position of a four-wave block.  That list sums
to 60 frames, a whole number of blocks, so the cases "first" (both frameless recordings in front, 53 frames) and "last" (both behind, 59
frames) are the ones whose last block has dead waves.  int16 and float recordings alternate (two of the float ones hold fractions, the
others widened int16); the int16 recordings are placed with a one-sample gap, so that they start at odd and at even offsets of the
packed buffer.  chunk_size 7, 16 and 2051: several chunks per recording, one chunk with a tail, one chunk for everything."""
import ctypes as C

import numpy as np
import pytest

import fbank_bound_ref as B
from oracle import fbank_ref
from reverb_amd import _lib
from reverb_amd._lib import fptr

pytestmark = pytest.mark.gpu
INPUTS = B.inputs()
p64 = lambda a: a.ctypes.data_as(_lib._i64p)
N399, N0 = -399, -1            # the two frameless recordings: 399 samples, no sample
CASES = {"middle": [1, 2, N399, 3, 5, N0, 4, 1, 37, 7],
         "first": [N399, N0, 1, 2, 3, 5, 4, 1, 37],
         "last": [1, 2, 3, 5, 4, 37, 7, N0, N399]}


def _recordings(frames):
    recs = []
    for i, f in enumerate(frames):
        n = {N399: 399, N0: 0}.get(f, B._len(f) if f > 0 else 0)
        src = INPUTS[11 if i == 3 else 12 if i == 7 else i][1]          # 11, 12: float waveforms with fractions
        x = np.ascontiguousarray(src[:n])
        assert len(x) == n
        x = x.astype(np.float32) if i % 2 else x
        assert x.dtype == (np.float32 if i % 2 else np.int16)
        recs.append(x)
    return recs


def _alone(lib, x):
    nf = fbank_ref.num_frames(len(x))
    out = np.zeros((nf + 4, 80), np.float32)
    if x.dtype == np.int16:
        rc = lib.rvb_test_fbank_ex(x.ctypes.data_as(_lib._i16p), None, len(x), fptr(out))
    else:
        rc = lib.rvb_test_fbank_ex(None, fptr(x), len(x), fptr(out))
    _lib.check(rc, "rvb_test_fbank_ex")
    return out[:nf]


@pytest.fixture(scope="module")
def alone(lib):
    """case -> [features of each recording through fbank_kernel alone]: computed once, read by every chunk_size"""
    return {name: [_alone(lib, x) for x in _recordings(frames)] for name, frames in CASES.items()}


def _batch(lib, recs, chunk, gap=1):
    ns = np.array([len(x) for x in recs], np.int64)
    fmt = np.array([4 if x.dtype == np.float32 else 2 for x in recs], np.int32)
    off, end = np.zeros(len(recs), np.int64), {2: 0, 4: 0}
    for i, x in enumerate(recs):
        off[i] = end[fmt[i]] + (gap if fmt[i] == 2 else 0)
        end[fmt[i]] = off[i] + len(x)
    nf, first = np.zeros(len(recs), np.int64), np.zeros(len(recs) + 1, np.int64)
    _lib.check(lib.rvb_batch_plan(p64(ns), len(recs), chunk, p64(nf), p64(first), None), "rvb_batch_plan")
    rows = int(first[-1]) * chunk
    out = np.zeros((rows + 4, 80), np.float32)
    data = (C.c_void_p * len(recs))(*[x.ctypes.data if len(x) else None for x in recs])
    _lib.check(lib.rvb_test_fbank_batch(data, _lib.iptr(fmt), p64(ns), p64(off), len(recs), chunk, fptr(out)), "rvb_test_fbank_batch")
    assert np.all(out[rows:].view(np.uint32) == 0xFFFFFFFF), "the sentinel rows behind the last chunk were written"
    return out[:rows], nf, first, off, fmt


@pytest.mark.parametrize("chunk", [7, 16, 2051])
@pytest.mark.parametrize("case", list(CASES))
def test_every_recording_has_the_bits_of_the_single_kernel(lib, alone, case, chunk):
    recs = _recordings(CASES[case])
    got, nf, first, off, fmt = _batch(lib, recs, chunk)
    assert nf.tolist() == [max(f, 0) for f in CASES[case]]
    if case == "middle":
        assert nf.sum() % 4 == 0 and sorted(set((np.cumsum(nf)[:-1] % 4).tolist())) == [0, 1, 2, 3]
    else:
        assert nf.sum() % 4 != 0
    i16_off = off[fmt == 2]
    assert (i16_off % 2 == 1).any() and (i16_off % 2 == 0).any()
    live = np.zeros(len(got), bool)
    for r, want in enumerate(alone[case]):
        r0 = int(first[r]) * chunk
        mine = got[r0:r0 + int(nf[r])]
        assert not np.isnan(mine).any(), "a live row was not written"
        assert np.array_equal(mine.view(np.uint32), want.view(np.uint32)), "recording %d differs from fbank_kernel on it alone" % r
        live[r0:r0 + int(nf[r])] = True
        assert first[r + 1] - first[r] == -(-int(nf[r]) // chunk)
    assert live.sum() == nf.sum()
    assert np.all(got[~live].view(np.uint32) == 0), "a padding row is not exactly zero"


@pytest.mark.parametrize("kind", ["int16", "float"])
def test_a_batch_of_one_is_the_single_kernel(lib, kind):
    """the guard against a change of the shared body: same samples, same bits, through either kernel"""
    x = np.ascontiguousarray(INPUTS[2][1] if kind == "int16" else INPUTS[12][1])
    want = _alone(lib, x)
    got, nf, first, _, _ = _batch(lib, [x], 16, gap=0)
    assert nf[0] == len(want) and first[1] == -(-len(want) // 16)
    assert np.array_equal(got[:len(want)].view(np.uint32), want.view(np.uint32))
    assert np.all(got[len(want):].view(np.uint32) == 0)


def test_a_batch_without_a_frame_writes_only_nothing(lib):
    recs = [np.zeros(399, np.int16), np.zeros(0, np.float32), np.zeros(120, np.float32)]
    got, nf, first, _, _ = _batch(lib, recs, 7)
    assert got.shape == (0, 80) and nf.tolist() == [0, 0, 0] and first.tolist() == [0, 0, 0, 0]
