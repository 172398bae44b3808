"""tests/fbank_bound_ref.py on the CPU: the fp64 reference agrees with the oracle, an fp32 restatement of fbank_kernel stays inside the
derived interval on every input of the GPU test (the fraction used is printed per input), and the interval has teeth: wrong
front ends leave it.  No GPU is needed; the hooks' argument refusals, which come before any device work, are checked here too."""
import numpy as np
import pytest

import fbank_bound_ref as B
from oracle import fbank_ref
from reverb_amd import _lib, synth

INPUTS = B.inputs()
SPEECH = INPUTS[0][1]


def test_reference_agrees_with_the_oracle():
    """the mixed-precision oracle (fp32 frames, pocketfft) and the fp64 reference, at the tolerance tests/test_kernels_gpu.py has"""
    pcm = synth.synth_audio(3.3, seed=7)
    lo, mid, hi = B.interval(pcm)
    want = fbank_ref.fbank(pcm)
    assert mid.shape == want.shape == (fbank_ref.num_frames(len(pcm)), 80)
    assert np.abs(mid - want).max() <= 1e-3
    assert np.all(lo < mid) and np.all(mid < hi)


def test_inputs_cover_the_frame_count_edges():
    counts = {name: fbank_ref.num_frames(len(x)) for name, x in INPUTS}
    assert {c % 4 for c in counts.values()} == {0, 1, 2, 3}
    assert counts["one frame"] == 1 and all(24 <= c <= 48 for n, c in counts.items() if n != "one frame")
    left = {name: (len(x) - 400) % 160 for name, x in INPUTS}
    assert left["noise"] == 159 and left["speech"] == 0                     # 159 samples over / ends on the last sample
    assert {str(x.dtype) for _, x in INPUTS} == {"int16", "float32"}


@pytest.mark.parametrize("name,x", INPUTS, ids=[n for n, _ in INPUTS])
def test_fp32_restatement_stays_inside_the_interval(name, x):
    lo, mid, hi = B.interval(x)
    got = B.restate32(x)
    frac = B.fraction(got, lo, mid, hi)
    # the claim the interval rests on: the spectrum's error vector is within eps_X in 2-norm
    _, X, E = B.ref64(x)
    re, im = B.restate32(x, spectrum=True)
    err = np.sqrt(((re - X.real) ** 2 + (im - X.imag) ** 2).sum(axis=1))
    ex = B.spectrum_bound(x, E)
    sfrac = np.where(ex > 0, err / np.where(ex > 0, ex, 1.0), np.where(err > 0, np.inf, 0.0))
    print("fbank interval, fp32 restatement, %-22s %2d frames: fraction used %.3f, of the spectrum bound %.3f"
          % (name, len(got), frac.max(), sfrac.max()))
    assert got.shape == mid.shape and np.all(np.isfinite(got))
    assert np.all(got >= lo) and np.all(got <= hi), "fraction %.3f" % frac.max()
    assert sfrac.max() <= 1.0


def test_mean_rounding_term_is_needed():
    """without the d_mean term the fp32 restatement leaves the interval on 20000 + {0, 1} (mel bin 0)"""
    x = dict(INPUTS)["20000 + {0,1}"]
    mel, X, E = B.ref64(x)
    re, im = B.restate32(x, spectrum=True)
    err = np.sqrt(((re - X.real) ** 2 + (im - X.imag) ** 2).sum(axis=1))
    assert (err / (B.RHO * np.sqrt(B.NFFT * E))).max() > 1.0 >= (err / B.spectrum_bound(x, E)).max()


MUTANTS = [("pre-emphasis 0.95", dict(preemph=0.95)), ("plain Hann", dict(window_power=1.0)), ("mean over 512", dict(mean_over=512)),
           ("frame shift 161", dict(shift=161)), ("mel rows shifted by one bin", dict(mel_shift=1))]


@pytest.mark.parametrize("name,kw", MUTANTS, ids=[n for n, _ in MUTANTS])
def test_a_wrong_front_end_leaves_the_interval(name, kw):
    lo, mid, hi = B.interval(SPEECH)
    got = B.restate32(SPEECH, **kw)
    n = min(len(got), len(mid))
    frac = B.fraction(got[:n], lo[:n], mid[:n], hi[:n])
    print("mutant %-28s: largest fraction %.3g, %.1f %% of the features outside" % (name, frac.max(), 100.0 * (frac > 1).mean()))
    assert frac.max() > 1.0


def test_conjugated_twiddles_show_in_the_spectrum_not_in_the_power():
    """a real frame's conjugated spectrum has the same power, so the features cannot see this mutant; re / im against the fp64 DFT
    do: the honest restatement is within eps_X, the conjugated one far outside on a frame that is not symmetric"""
    _, X, E = B.ref64(SPEECH)
    ex = B.spectrum_bound(SPEECH, E)
    for conj, inside in ((False, True), (True, False)):
        re, im = B.restate32(SPEECH, conj_twiddles=conj, spectrum=True)
        err = np.sqrt(((re - X.real) ** 2 + (im - X.imag) ** 2).sum(axis=1))
        assert np.all(err <= ex) if inside else np.all(err > 100 * ex)
    assert np.array_equal(B.restate32(SPEECH, conj_twiddles=True), B.restate32(SPEECH))


def test_zero_for_the_sample_before_the_frame_is_an_equivalent_mutant():
    """`x[-1] := 0` instead of x[0] changes only y[0] = (x[0] - 0.97 x[-1]) window[0], and the povey window's first tap is exactly
    0: the mutant computes the same bits on every input, so no check of the features can tell it apart (nor need one)."""
    window, _ = B.tables()
    assert window[0] == 0.0 and window[-1] == 0.0
    for name, x in INPUTS[:3]:
        assert np.array_equal(B.restate32(x, first_prev_zero=True), B.restate32(x))


def test_exact_inputs_sit_on_the_log_floor():
    floor = np.log(fbank_ref.EPS)
    for name in ("constant 1234", "zeros"):
        got = B.restate32(dict(INPUTS)[name])
        assert np.all(np.abs(got - floor) <= 2 * np.spacing(np.abs(floor)))


@pytest.mark.parametrize("ms,win,nmel", [(16.1, 257, 128), (32.0, 512, 1)])
def test_interval_at_the_window_extremes(ms, win, nmel):
    assert int(16000 * ms * 0.001) == win
    x = SPEECH.astype(np.float32)
    lo, mid, hi = B.interval(x, win, 160, nmel)
    got = B.restate32(x, win, 160, nmel)
    assert got.shape == (1 + (len(x) - win) // 160, nmel)
    frac = B.fraction(got, lo, mid, hi)
    print("fbank interval, fp32 restatement, window %d, %d mel bins: fraction used %.3f" % (win, nmel, frac.max()))
    assert frac.max() <= 1.0


def test_hooks_refuse_bad_arguments_before_any_device_work():
    """V < 1, ld < V, a target outside [0, V) and a ptr that does not ascend from 0 are refused by name (E_ARG = -1) before the hooks
    look for a device, so this holds with and without a GPU; the outputs stay as the caller filled them."""
    lib = _lib.load_test()
    x = np.zeros((2, 8), np.float32)
    tv, ti, out = np.full((2, 2), 7.0, np.float32), np.full((2, 2), 7, np.int32), np.full(4, 7.0, np.float32)
    f, i = _lib.fptr, _lib.iptr

    def topk(V, ld):
        return lib.rvb_test_logsoftmax_topk_ex(f(x), 2, V, ld, 2, 0.0, 0, f(tv), i(ti), None)

    def gather(V, ld, tgt):
        return lib.rvb_test_lse_gather_ex(f(x), 2, V, ld, i(np.array(tgt, np.int32)), 0.0, 0, f(out))

    def multi(V, ld, ptr, tgt):
        return lib.rvb_test_lse_gather_multi_ex(f(x), 2, V, ld, i(np.array(ptr, np.int32)), i(np.array(tgt, np.int32)), f(out))

    assert topk(8, 7) == -1 and b"rvb_test_logsoftmax_topk_ex: ld < V" in lib.rvb_last_error()
    assert topk(0, 8) == -1 and b"rvb_test_logsoftmax_topk_ex: V < 1" in lib.rvb_last_error()
    assert gather(8, 7, [0, 0]) == -1 and b"rvb_test_lse_gather_ex: ld < V" in lib.rvb_last_error()
    assert gather(0, 8, [0, 0]) == -1 and b"V < 1" in lib.rvb_last_error()
    assert gather(8, 8, [0, 8]) == -1 and b"rvb_test_lse_gather_ex: target outside" in lib.rvb_last_error()
    assert gather(8, 8, [-1, 0]) == -1
    assert multi(8, 7, [0, 1, 2], [0, 0]) == -1 and b"rvb_test_lse_gather_multi_ex: ld < V" in lib.rvb_last_error()
    assert multi(0, 8, [0, 1, 2], [0, 0]) == -1 and b"V < 1" in lib.rvb_last_error()
    assert multi(8, 8, [0, 1, 2], [0, 8]) == -1 and b"target outside" in lib.rvb_last_error()
    assert multi(8, 8, [0, 2, 1], [0, 0]) == -1 and b"ptr decreases" in lib.rvb_last_error()
    assert multi(8, 8, [1, 1, 2], [0, 0]) == -1 and b"ptr[0] must be 0" in lib.rvb_last_error()
    # the hooks without a stride are calls of these
    assert lib.rvb_test_lse_gather(f(x), 2, 8, i(np.array([0, 9], np.int32)), f(out)) == -1
    assert lib.rvb_test_lse_gather_multi(f(x), 2, 8, i(np.array([0, 1, 2], np.int32)), i(np.array([0, 0], np.int32)), 3, f(out)) == -1
    feats = np.full((4, 80), 7.0, np.float32)
    pcm = np.zeros(400, np.int16)
    assert lib.rvb_test_fbank_ex(None, None, 400, f(feats)) == -1 and b"rvb_test_fbank_ex" in lib.rvb_last_error()
    assert lib.rvb_test_fbank_ex(pcm.ctypes.data_as(_lib._i16p), f(x), 400, f(feats)) == -1
    assert np.all(tv == 7.0) and np.all(ti == 7) and np.all(out == 7.0) and np.all(feats == 7.0)
