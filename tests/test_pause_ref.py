"""tests/pause_ref.py against itself: the fp64 and fp32 restatements of the pause-cut definition agree on the inputs the GPU tests use, the
replay check accepts the definition's own cuts and refuses wrong ones, and the properties the definition promises hold.  No GPU."""
import numpy as np
import pytest

import pause_ref as P
from oracle import fbank_ref
from reverb_amd import synth

SHAPES = [(cs, s, h) for cs in (16, 64, 256) for s in sorted({7, cs // 4, cs - 7}) for h in (1, 10, 64)]
VALID = [(cs, s, h) for cs, s, h in SHAPES if 7 <= s <= cs - 7]


@pytest.fixture(scope="module")
def real_feats():
    return {"speech": fbank_ref.fbank(synth.synth_audio(30.0)), "bursts": fbank_ref.fbank(P.burst_audio(30.0, 0))}


def _int_feats(n, seed):
    return np.random.default_rng(seed).integers(-20, 21, size=(n, 80)).astype(np.float32)


def test_the_shapes_of_the_gpu_tests():
    # chunk_size 16 with search = chunk_size // 4 = 4 is below the 7 frames a piece needs: the one shape of the grid that is refused
    assert sorted(set(SHAPES) - set(VALID)) == [(16, 4, 1), (16, 4, 10), (16, 4, 64)]
    with pytest.raises(AssertionError):
        P.cuts(_int_feats(40, 0), 16, 4, 10)


@pytest.mark.parametrize("cs,search,h", VALID)
def test_properties_on_integer_features(cs, search, h):
    for n in (0, 1, 6, cs, cs + 1, cs + 7, 3000):
        x = _int_feats(n, n)
        st = P.cuts(x, cs, search, h)
        assert st == P.cuts(x, cs, search, h, np.float32)            # integer sums are exact in fp32
        P.check_tiling(st, n, cs)
        P.replay_check(x, st, cs, search, h)
        if n <= cs:
            assert st == ([0] if n else [])
        if n == cs + 1:
            assert len(st) == 2
        # the last minimum wins: brute force over the window
        e = x.astype(np.float64).sum(axis=1)
        for k in range(1, len(st)):
            lo, hi = st[k - 1] + cs - search, min(st[k - 1] + cs, n - 7)
            s = [sum(e[min(max(c + j, 0), n - 1)] for j in range(-h, h)) for c in range(lo, hi + 1)]
            assert st[k] == lo + max(i for i, v in enumerate(s) if v == min(s))


def test_constant_features_cut_at_hi():
    x = np.full((1000, 80), P.FLOOR, np.float32)
    for dt in (np.float64, np.float32):
        st = P.cuts(x, 64, 16, 10, dt)
        assert st[:-1] == list(range(0, 64 * (len(st) - 1), 64)) and all(b - a == 64 for a, b in zip(st[:-2], st[1:-1]))
        assert st[-1] == min(st[-2] + 64, 1000 - 7)


def test_nan_windows_cut_at_hi_and_nan_is_never_chosen():
    x = _int_feats(600, 3)
    x[40:300] = np.nan                              # wider than a window: every candidate of the first cuts is NaN
    st = P.cuts(x, 64, 16, 10)
    assert st[1] == 64 and st[2] == 128
    P.replay_check(x, st, 64, 16, 10)
    y = _int_feats(200, 4)
    y[60] = np.nan                                   # s is NaN for c in 51 .. 70: of [48, 64] only 48 .. 50 are left
    assert 48 <= P.cuts(y, 64, 16, 10)[1] <= 50


def test_replay_check_refuses_wrong_cuts(real_feats):
    x = real_feats["bursts"]
    st = P.cuts(x, 256, 96, 10)
    P.replay_check(x, st, 256, 96, 10)
    s = P.smoothed(P.loudness(x), 10)
    loud = 160 + int(np.argmax(s[160:257]))
    after = lambda c0: [0, c0] + [c0 + c for c in P.cuts(x[c0:], 256, 96, 10)[1:]]      # a first cut at c0, then valid tiling
    with pytest.raises(AssertionError, match="above the minimum"):
        P.replay_check(x, after(loud), 256, 96, 10)
    with pytest.raises(AssertionError, match="outside"):
        P.replay_check(x, after(100), 256, 96, 10)
    with pytest.raises(AssertionError):
        P.replay_check(x, st[:-1], 256, 96, 10)      # the last piece would exceed chunk_size (or a piece is missing)


@pytest.mark.parametrize("cs,search,h", VALID)
def test_fp32_and_fp64_agree_on_the_real_inputs(real_feats, cs, search, h):
    """The two restatements give the same cuts wherever the smoothing window (2h frames) is no longer than a chunk.  With 2h = 128 and
    chunk_size 16 or 64 the window spans several bursts and pauses, neighbouring candidates differ only by which silent frames (all
    e = 80 * FLOOR) they hold, their true s ties exactly and the order of the additions decides: there the fp32 and fp64 cuts differ
    on the burst audio (first at piece 26 of (16, 7, 64): 312 against 311), each within the bound of the other, which the replay check
    confirms."""
    for name, x in real_feats.items():
        a, b = P.cuts(x, cs, search, h), P.cuts(x, cs, search, h, np.float32)
        if 2 * h <= cs:
            assert a == b, name
        P.replay_check(x, a, cs, search, h)
        P.replay_check(x, b, cs, search, h)
        # the bound holds for numpy's own fp32 sums
        s64, s32 = P.smoothed(P.loudness(x), h), P.smoothed(P.loudness(x, np.float32), h)
        assert np.all(np.abs(s32.astype(np.float64) - s64) <= P.delta(x, h))


def test_delta_is_about_014_at_h10(real_feats):
    d = P.delta(real_feats["speech"], 10)
    assert 0.02 < np.median(d) < 0.3


@pytest.mark.parametrize("seed", range(5))
def test_burst_cuts_land_in_silence(seed):
    x = fbank_ref.fbank(P.burst_audio(30.0, seed))
    st = P.cuts(x, 256, 96, 10)
    assert st == P.cuts(x, 256, 96, 10, np.float32) and len(st) > 4
    for c in st[1:]:
        assert np.all(x[c - 10:c + 10] == P.FLOOR), c
