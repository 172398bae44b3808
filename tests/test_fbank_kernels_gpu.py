"""fbank_kernel<int16_t> / fbank_kernel<float> (csrc/fbank.hip) through the lab hook rvb_test_fbank_ex, and fbank_any_kernel through
rvb_compute_feats, against the interval tests/fbank_bound_ref.py derives from an fp64 reference: every feature of every input lies
inside it, no entry excluded.  The inputs (fbank_bound_ref.inputs) have 37 .. 40 frames, so the last block has 1, 2, 3 and 0 dead
waves sharing its barriers, end exactly on the last sample or leave 159 samples over, and cover speech, a near-silent signal, full-scale
noise, tones and a square wave, exact inputs (a constant, zeros: the log floor on every bin), an impulse, DC-heavy signals where the
fp32 rounding of the mean dominates, and two float waveforms for the float instantiation.  The hook gives the kernel a waveform buffer
of exactly n_samples elements and a feature buffer with four sentinel rows after the last frame, which must come back untouched.
The fraction of the interval each input uses is printed; fbank_bound_ref's docstring records it next to the CPU restatement's."""
import ctypes as C

import numpy as np
import pytest

import fbank_bound_ref as B
from oracle import fbank_ref
from reverb_amd import _lib
from reverb_amd._lib import fptr

pytestmark = pytest.mark.gpu
INPUTS = B.inputs()


def _run(lib, x):
    """-> feats [frames][80] after checking that the four rows behind them still hold the all-ones bytes"""
    nf = fbank_ref.num_frames(len(x))
    out = np.zeros((nf + 4, 80), np.float32)
    if x.dtype == np.int16:
        rc = lib.rvb_test_fbank_ex(x.ctypes.data_as(_lib._i16p), None, len(x), fptr(out))
    else:
        assert x.dtype == np.float32
        rc = lib.rvb_test_fbank_ex(None, fptr(x), len(x), fptr(out))
    _lib.check(rc, "rvb_test_fbank_ex")
    assert np.all(out[nf:].view(np.uint32) == 0xFFFFFFFF), "rows after the last frame were written"
    assert not np.isnan(out[:nf]).any(), "a feature was not written"
    return out[:nf]


@pytest.mark.parametrize("name,x", INPUTS, ids=[n for n, _ in INPUTS])
def test_every_feature_is_inside_its_interval(lib, name, x):
    x = np.ascontiguousarray(x)
    got = _run(lib, x)
    lo, mid, hi = B.interval(x)
    frac = B.fraction(got, lo, mid, hi)
    print("fbank interval, kernel, %-22s %2d frames: fraction used %.3f" % (name, len(got), frac.max()))
    assert got.shape == mid.shape
    assert np.all(got >= lo) and np.all(got <= hi), "fraction %.3f" % frac.max()
    if x.dtype == np.int16:
        # the kernel widens int16 to the same floats: the float instantiation gives the same bits
        same = _run(lib, x.astype(np.float32))
        assert np.array_equal(same.view(np.uint32), got.view(np.uint32)), "fbank_f32 on the widened samples differs from fbank"
    if name in ("constant 1234", "zeros"):
        # the DC removal is exact, every bin is logf of something in [0, eps]: the floor
        floor = np.log(fbank_ref.EPS)
        assert np.all(np.abs(got - floor) <= 2 * np.spacing(np.abs(floor)))


def test_too_short_for_a_frame_writes_nothing(lib):
    x = np.ascontiguousarray(INPUTS[0][1][:399])
    assert _run(lib, x).shape == (0, 80)
    assert _run(lib, x.astype(np.float32)).shape == (0, 80)


def test_the_old_hook_is_the_new_one(lib):
    x = np.ascontiguousarray(INPUTS[0][1])
    old = np.full((fbank_ref.num_frames(len(x)), 80), np.nan, np.float32)
    _lib.check(lib.rvb_test_fbank(x.ctypes.data_as(_lib._i16p), len(x), fptr(old)))
    assert np.array_equal(old.view(np.uint32), _run(lib, x).view(np.uint32))


@pytest.mark.parametrize("ms,win,nmel,shift_ms", [(16.1, 257, 128, 10.0), (32.0, 512, 1, 10.0), (16.1, 257, 1, 6.25), (32.0, 512, 128, 12.5)])
def test_compute_feats_at_the_window_extremes(ms, win, nmel, shift_ms):
    """fbank_any_kernel at the shortest and the longest window rvb_compute_feats accepts, with the most and the fewest mel bins, held
    to the same interval generalised to (win, shift, nmel)"""
    product = _lib.load()
    shift = int(16000 * shift_ms * 0.001)
    assert int(16000 * ms * 0.001) == win
    for name in ("speech", "float DC + fractions", "tone 1 kHz"):
        wave = np.ascontiguousarray(dict(INPUTS)[name].astype(np.float32))
        want = 1 + (len(wave) - win) // shift
        n = C.c_int64(0)
        got = np.full((want, nmel), np.nan, np.float32)
        _lib.check(product.rvb_compute_feats(0, fptr(wave), wave.size, nmel, float(ms), float(shift_ms), fptr(got), C.byref(n)))
        assert n.value == want
        lo, mid, hi = B.interval(wave, win, shift, nmel)
        frac = B.fraction(got, lo, mid, hi)
        print("fbank interval, rvb_compute_feats window %d shift %d, %d mel bins, %-22s: fraction used %.3f"
              % (win, shift, nmel, name, frac.max()))
        assert np.all(got >= lo) and np.all(got <= hi), "fraction %.3f" % frac.max()
