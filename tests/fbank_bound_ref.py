"""The interval every log-mel feature of the fbank kernels (csrc/fbank.hip) must lie in, from an fp64 reference and a derived bound.

Reference (`ref64`): the kernel's algorithm in fp64 -- frame, subtract the mean, pre-emphasis with x[-1] := x[0], povey window, 512-point
DFT, power, mel projection -- with the oracle's fp32 tables (oracle/fbank_ref.py window and mel banks, the fp32 constant 0.97f) widened
to fp64 and an exact DFT.  It returns mel64 [frame][m], the spectrum X [frame][257] and the windowed frame's energy E = sum y^2.

Bound (`interval`), with u = 2^-24 and N = 512.  The computed spectrum differs from the exact one by a vector of 2-norm at most

    eps_X = rho sqrt(N E) + sqrt(N) 0.03 d_mean ||window||_2          rho = (9 * 5 + 4) u

rho: Higham's bound of the radix-2 FFT, log2 N (mu + gamma_4) with twiddles rounded to fp32 (mu = u), relative to ||X||_2 = sqrt(N E)
(Parseval), plus one rounding each for the DC subtraction, the pre-emphasis product, its difference and the window product.  d_mean is
the rounding of the frame mean, which shifts every sample alike: after the pre-emphasis 0.03 of it is left, times the window, and a
DFT multiplies a 2-norm by sqrt(N).  For int16 input the sum of `win` samples is exact (below 2^24) and d_mean = 2 u |mean| (the
division and the conversion of `win`); for float input d_mean = (win + 2) u max|x| of the frame (any summation order).
The filter weights are at most 1, so by Cauchy-Schwarz over the bins of a filter

    |mel - mel64| <= D = 2 sqrt(mel64) eps_X + eps_X^2 + (max(30, widest filter) + 10) u mel64

the last term being the fp32 power (3 roundings) and the sequential fp32 mel sum (80 bins at a 400-sample window: at most 30 terms,
i.e. 40 u).  The feature must lie in [log max(mel64 - D, eps), log max(mel64 + D, eps)], each end widened by 4 units in the last
place (fp32) of max(|end|, 1) for logf: the interval form needs no special case at the log floor.

`restate32` is an fp32 numpy restatement of the kernel (the same radix-2 decimation-in-time order, fp32 tables, the wave's butterfly
sum) and takes the mutants tests/test_fbank_bound_ref.py uses to show that the interval has teeth.  `inputs()` are the waveforms both
the CPU test and tests/test_fbank_kernels_gpu.py run.

Largest fraction of the interval's half-width used (0 = the fp64 value, 1 = the end of the interval), per input, by the fp32
restatement on the CPU / by fbank_kernel on an MI355X (tests/test_fbank_kernels_gpu.py prints them):
    speech                 0.025 / 0.088
    speech/4000            0.011 / 0.029
    noise                  0.027 / 0.103
    tone 1 kHz             0.031 / 0.123
    tone 2 kHz             0.029 / 0.029
    square                 0.017 / 0.073
    constant 1234          0.000 / 0.136
    zeros                  0.114 / 0.136
    impulse                0.114 / 0.136
    20000 + {0,1}          0.117 / 0.117
    -32768 + {0,1,2}       0.078 / 0.078
    float pcm * 0.7391     0.017 / 0.042
    float DC + fractions   0.022 / 0.022
    one frame              0.020 / 0.062
(0.11 - 0.14 on the inputs that sit on the log floor is half a unit in the last place of logf against the 4 the interval allows.)
fbank_any_kernel through rvb_compute_feats at (window, shift, mel bins), the largest over three inputs, on the MI355X:
(257, 160, 128) 0.097, (512, 160, 1) 0.057, (257, 100, 1) 0.073, (512, 200, 128) 0.068.
"""
import numpy as np

from oracle import fbank_ref

U = 2.0 ** -24
NFFT, NBIN = 512, 257
EPS = float(fbank_ref.EPS)
PREEMPH = float(np.float32(0.97))
RHO = (9 * 5 + 4) * U


def tables(win=400, nmel=80):
    """(window [win], banks [nmel][257]) as the oracle builds them in fp32."""
    window = fbank_ref.povey_window(win)
    banks = np.concatenate([fbank_ref.mel_banks(nmel, NFFT, 16000.0), np.zeros((nmel, 1), np.float32)], axis=1)
    return window, banks


def _frames(x, win, shift):
    n = fbank_ref.num_frames(len(x), win, shift)
    return x[np.arange(n)[:, None] * shift + np.arange(win)[None, :]]


def ref64(x, win=400, shift=160, nmel=80):
    """-> mel64 [frames][nmel], X [frames][257] complex, E [frames], all fp64; x: int16 or float waveform at int16 scale."""
    window, banks = tables(win, nmel)
    f = _frames(np.asarray(x).astype(np.float64), win, shift)
    f = f - f.mean(axis=1, keepdims=True)
    y = (f - PREEMPH * np.concatenate([f[:, :1], f[:, :-1]], axis=1)) * window.astype(np.float64)
    X = np.fft.rfft(y, n=NFFT, axis=1)
    mel = (X.real ** 2 + X.imag ** 2) @ banks.astype(np.float64).T
    return mel, X, (y * y).sum(axis=1)


def spectrum_bound(x, E, win=400, shift=160):
    """eps_X per frame (docstring)."""
    window, _ = tables(win, 1)
    x = np.asarray(x)
    f = _frames(x.astype(np.float64), win, shift)
    if x.dtype == np.int16:
        d_mean = 2 * U * np.abs(f.mean(axis=1))
    else:
        d_mean = (win + 2) * U * np.abs(f).max(axis=1)
    return RHO * np.sqrt(NFFT * E) + np.sqrt(NFFT) * 0.03 * d_mean * np.linalg.norm(window.astype(np.float64))


def _widen(v, sign):
    return v + sign * 4.0 * np.spacing(np.maximum(np.abs(v), 1.0).astype(np.float32)).astype(np.float64)


def interval(x, win=400, shift=160, nmel=80):
    """-> (lo, mid, hi) [frames][nmel] fp64: the ends of the interval and the fp64 feature itself."""
    mel, _, E = ref64(x, win, shift, nmel)
    ex = spectrum_bound(x, E, win, shift)[:, None]
    _, banks = tables(win, nmel)
    widest = int((banks > 0).sum(axis=1).max())
    D = 2 * np.sqrt(mel) * ex + ex * ex + (max(30, widest) + 10) * U * mel
    lo = np.log(np.maximum(mel - D, EPS))
    hi = np.log(np.maximum(mel + D, EPS))
    return _widen(lo, -1.0), np.log(np.maximum(mel, EPS)), _widen(hi, 1.0)


def fraction(feats, lo, mid, hi):
    """Signed distance of each feature from the fp64 value as a fraction of its side of the interval (> 1: outside)."""
    feats = np.asarray(feats, np.float64)
    return np.where(feats >= mid, (feats - mid) / (hi - mid), (mid - feats) / (mid - lo))


def restate32(x, win=400, shift=160, nmel=80, preemph=0.97, window_power=0.85, mean_over=None, conj_twiddles=False, mel_shift=0,
              first_prev_zero=False, spectrum=False):
    """fbank_kernel in fp32 numpy.  The keyword arguments past nmel are the mutants; spectrum=True returns (re, im) [frames][257]."""
    f32 = np.float32
    window, banks = tables(win, nmel)
    if window_power != 0.85:
        i = np.arange(win, dtype=np.float64)
        window = ((0.5 - 0.5 * np.cos(2.0 * np.pi * i / (win - 1))) ** window_power).astype(f32)
    if mel_shift:
        banks = np.roll(banks, mel_shift, axis=1)
    f = _frames(np.asarray(x).astype(f32), win, shift)
    nfr = f.shape[0]
    # lane l sums its elements l, l + 64, ... in turn, then the xor butterfly over the 64 lanes
    pad = np.zeros((nfr, 512), f32)
    pad[:, :win] = f
    part = np.zeros((nfr, 64), f32)
    for i in range(8):
        part = part + pad[:, 64 * i:64 * i + 64]
    for o in (32, 16, 8, 4, 2, 1):
        part = part + part[:, np.arange(64) ^ o]
    mean = part[:, :1] / f32(mean_over or win)
    f = f - mean
    prev = np.concatenate([f[:, :1], f[:, :-1]], axis=1)
    if first_prev_zero:
        prev[:, 0] = 0
    y = np.zeros((nfr, NFFT), f32)
    y[:, :win] = (f - f32(preemph) * prev) * window
    rev = np.array([int(format(j, "09b")[::-1], 2) for j in range(NFFT)])
    re = np.empty_like(y)
    re[:, rev] = y
    im = np.zeros_like(y)
    k = np.arange(256)
    twr = np.cos(2.0 * np.pi * k / NFFT).astype(f32)
    twi = (-np.sin(2.0 * np.pi * k / NFFT)).astype(f32)
    if conj_twiddles:
        twi = -twi
    b = np.arange(256)
    for s in range(9):
        half = 1 << s
        j = b & (half - 1)
        i0 = ((b >> s) << (s + 1)) + j
        i1 = i0 + half
        wr, wi = twr[j << (8 - s)], twi[j << (8 - s)]
        ar, ai, br, bi = re[:, i0], im[:, i0], re[:, i1], im[:, i1]
        tr = wr * br - wi * bi
        ti = wr * bi + wi * br
        re[:, i0], im[:, i0], re[:, i1], im[:, i1] = ar + tr, ai + ti, ar - tr, ai - ti
    if spectrum:
        return re[:, :NBIN], im[:, :NBIN]
    pw = re[:, :NBIN] * re[:, :NBIN] + im[:, :NBIN] * im[:, :NBIN]
    acc = np.zeros((nfr, nmel), f32)
    for bin_ in range(NBIN):          # ascending bins; a zero weight adds an exact zero
        acc = acc + pw[:, bin_:bin_ + 1] * banks[None, :, bin_]
    return np.log(np.maximum(acc, fbank_ref.EPS))


def _len(frames, extra=0):
    return 400 + 160 * (frames - 1) + extra


def inputs():
    """[(name, waveform)]: int16, or float32 at int16 scale.  Frame counts 37 .. 40 (n_frames % 4 = 1, 2, 3, 0); most lengths end
    exactly on the last frame (n = 400 + 160 j), `noise` leaves 159 samples over."""
    from reverb_amd import synth
    rng = np.random.default_rng(2024)
    speech = synth.synth_audio(0.5, seed=7)
    t = np.arange(_len(40), dtype=np.float64) / 16000.0
    i16 = lambda a: np.asarray(a).astype(np.int16)
    out = [
        ("speech", speech[:_len(37)]),
        ("speech/4000", i16(speech[:_len(38)] // 4000)),
        ("noise", i16(rng.integers(-32768, 32768, _len(38, 159)))),
        ("tone 1 kHz", i16(np.round(32767.0 * np.sin(2 * np.pi * 1000.0 * t[:_len(39)])))),
        ("tone 2 kHz", i16(np.round(32767.0 * np.sin(2 * np.pi * 2000.0 * t[:_len(40)])))),
        ("square", i16(np.where((np.arange(_len(37)) // 40) % 2 == 0, 32767, -32768))),
        ("constant 1234", np.full(_len(38), 1234, np.int16)),
        ("zeros", np.zeros(_len(39), np.int16)),
        ("impulse", i16(np.arange(_len(40)) == 1000) * np.int16(30000)),
        ("20000 + {0,1}", i16(20000 + rng.integers(0, 2, _len(37)))),
        ("-32768 + {0,1,2}", i16(-32768 + rng.integers(0, 3, _len(38)))),
        ("float pcm * 0.7391", (speech[:_len(39)].astype(np.float32) * np.float32(0.7391))),
        ("float DC + fractions", (np.float32(12345.678) + rng.random(_len(40)).astype(np.float32))),
        ("one frame", speech[:400]),
    ]
    return out
