"""The windowed CTC Viterbi without a GPU: the numpy restatement (tests/force_align_window_ref.py) against the exact one
(tests/force_align_ref.py), the window policy of the library (rvb_test_ctc_window_next_lo, host code) against the restatement's, and the
refusals of the lab hook rvb_test_ctc_viterbi_window, which all come before any device work."""
import numpy as np
import pytest

import force_align_ref as R
import force_align_window_ref as WR
from reverb_amd import _lib

DECOY_SEED = 5             # searched: seeds 5, 6, 13 and 16 of 0..19 drop the true path and touch the window edge


def same(got, want):
    assert np.array_equal(got[0], want[0])
    assert np.float32(got[1]).tobytes() == np.float32(want[1]).tobytes()


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("slab", [8192, 37])
def test_a_window_that_holds_the_lattice_is_the_exact_alignment(kind, slab):
    lp, y, T = R.make_case(3, 300, 16, 40, kind)
    labels, score, lo, margin = WR.force_align_window(lp, y, 0, slab)
    same((labels, score), R.force_align(lp, y))
    assert not lo.any() and margin == WR.effective_window(len(y), 0) == 96      # no frame counts: both edges are the lattice's own
    lp, y, T = R.make_case(4, 700, 16, 150, kind)                               # S = 301 rounded up: 320 < 512
    same(WR.force_align_window(lp, y, 512, slab)[:2], R.force_align(lp, y))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_a_planted_path_in_a_lattice_five_windows_long(seed):
    lp, y, _ = R.make_case(seed, 1500, 16, 640, "random")                          # S = 1281 = 5 W
    labels, score, lo, margin = WR.force_align_window(lp, y, 256, 97)
    same((labels, score), R.force_align(lp, y))
    assert margin > 0
    assert np.all(np.diff(lo) >= 0) and np.all(lo % 32 == 0) and lo[0] == 0 and lo[-1] + 256 >= 1281 - 1
    assert len(set(lo.tolist())) > 10                                           # the window really moved


def test_the_decoy_makes_the_window_drop_the_true_path():
    lp, y = WR.decoy_case(DECOY_SEED)
    labels, score, lo, margin = WR.force_align_window(lp, y, WR.DECOY_W, 8192)
    exact = R.force_align(lp, y)
    opt = R.optimum64(lp, y)
    print("windowed %.4f exact fp32 %.4f optimum fp64 %.4f margin %d" % (score, exact[1], opt, margin))
    assert float(score) < opt - 100.0 and abs(float(exact[1]) - opt) < 1e-2     # not a rounding matter
    assert margin == 0
    assert R.collapse(labels).tolist() == y.tolist()                            # still an alignment of the transcript
    assert abs(R.path_score64(lp, labels) - float(score)) < 1e-2


def test_wildcards_in_the_restatement_match_the_appended_column():
    """the wildcard as an extra column w + bias with label V (how tests/test_force_align_wild_ref.py states it) against w= / bias= here"""
    lp, y, _ = R.make_case(9, 500, 12, 120, "random")
    w = np.ascontiguousarray(lp.max(1))
    bias = np.float32(-0.5)
    ext = np.ascontiguousarray(np.concatenate([lp, (w + bias).astype(np.float32)[:, None]], 1))
    yw = np.array(y, np.int64); yw[40:60] = WR.WILDCARD; yw = np.concatenate([yw[:41], yw[60:]])
    yv = np.where(yw == WR.WILDCARD, 12, yw)
    want = R.force_align(ext, yv)
    got = WR.force_align_window(lp, yw, 0, 64, w=w, bias=-0.5)
    assert np.array_equal(np.where(got[0] == WR.WILDCARD, 12, got[0]), want[0]) and got[1].tobytes() == want[1].tobytes()


def chain(lib, rng, S, T, W):
    """the policy called as the driver calls it, launch after launch, with arbitrary best states inside the window"""
    lo = 0
    S_pad = WR.pad32(S)
    for f0, f1 in WR.segments(T, W, int(rng.integers(1, 3 * W))):
        hi_reach = min(lo + W, S, 2 * f0 + 2)
        best = -1 if f0 == 0 or rng.random() < 0.05 or hi_reach <= lo else int(rng.integers(lo, hi_reach))
        want = WR.next_lo(S, T, W, f0, f1, lo, best)
        got = lib.rvb_test_ctc_window_next_lo(S, T, W, f0, f1, lo, best)
        assert got == want, (S, T, W, f0, f1, lo, best, got, want)
        assert got % 32 == 0 and got >= lo and 0 <= got <= S_pad - W
        assert got + W - 1 >= S - 2 - 2 * (T - f1)                               # the end stays reachable
        lo = got
        yield 1
    assert lo + W - 1 >= S - 2


def test_the_policy_of_the_library_is_the_restatements(lib):
    rng = np.random.default_rng(2025)
    calls = 0
    while calls < 4000:
        W = int(rng.choice([256, 512, 1024, 4096]))
        L = int(rng.integers(W // 2, 6 * W))
        S = 2 * L + 1
        T = int(L + rng.integers(0, 2 * L))
        calls += sum(chain(lib, rng, S, T, min(W, WR.pad32(S))))
    assert lib.rvb_test_ctc_window_next_lo(1001, 600, 256, 0, 64, 0, -1) == 0


def test_align_wav_keeps_the_one_batch_options_off_the_long_form():
    from reverb_amd.bin.align_wav import get_args
    base = ["--model", "m", "--audio_file", "a.wav", "--transcript_file", "t.txt", "--result_dir", "out"]
    args = get_args(base + ["--long_form", "--window_tokens", "4096", "--wildcard", "<star>"])
    assert args.long_form and args.window_tokens == 4096
    assert get_args(base).long_form is False and get_args(base).window_tokens is None
    for extra in (["--long_form", "--score"], ["--window_tokens", "512", "--posteriors"], ["--long_form", "--alternatives"],
                  ["--window_tokens", "0"]):
        with pytest.raises(SystemExit):
            get_args(base + extra)


def hook(lib, lp, y, window=0, w=None, bias=0.0, slab=64, T=None, L=None, blank=0):
    lp = np.ascontiguousarray(lp, np.float32)
    y = np.ascontiguousarray(y, np.int32)
    T = lp.shape[0] if T is None else T
    n = max(min(T, 1 << 16), 1)
    labels, lo = np.full(n, -7, np.int32), np.full(n, -7, np.int32)
    score, margin = np.full(1, 123.0, np.float32), np.full(1, -7, np.int32)
    rc = lib.rvb_test_ctc_viterbi_window(_lib.fptr(lp), T, lp.shape[1], None if w is None else _lib.fptr(w), bias, _lib.iptr(y),
                                         len(y) if L is None else L, blank, slab, window, _lib.iptr(labels), _lib.fptr(score),
                                         _lib.iptr(lo), _lib.iptr(margin))
    untouched = np.all(labels == -7) and np.all(lo == -7) and score[0] == 123.0 and margin[0] == -7
    return rc, lib.rvb_last_error().decode(), untouched


def test_the_hook_refuses_before_any_device_work(lib):
    lp, y, _ = R.make_case(1, 20, 8, 5, "random")
    w = np.ascontiguousarray(lp.max(axis=1))
    for bad in (100, 300, 65536, -256):
        rc, msg, clean = hook(lib, lp, y, window=bad)
        assert rc == -1 and "window_states %d must be 0" % bad in msg and "multiple of 256" in msg and clean
    rc, msg, clean = hook(lib, lp, y, L=0);                   assert rc == -1 and "empty transcript" in msg and clean
    rc, msg, clean = hook(lib, lp, [1, 0, 2]);                assert rc == -1 and "token 1 is the blank id 0" in msg and clean
    rc, msg, clean = hook(lib, lp, [1, 8, 2]);                assert rc == -1 and "token id 8 outside [0, 8)" in msg and clean
    rc, msg, clean = hook(lib, lp, [1, WR.WILDCARD, 2]);      assert rc == -1 and "token id -2 outside" in msg and clean   # w == NULL: no wildcard
    rc, msg, clean = hook(lib, lp[:5], [1, 2, 2, 2, 3])
    assert rc == -1 and "infeasible" in msg and "2 adjacent repeats need at least 7 frames, the lattice has 5" in msg and clean
    rc, msg, clean = hook(lib, lp, y, T=(1 << 20) + 1);       assert rc == -5 and "frames exceed the cap" in msg and clean
    rc, msg, clean = hook(lib, lp, y, w=w, bias=0.5);         assert rc == -1 and "bias" in msg and clean
    rc, msg, clean = hook(lib, lp, y, bias=float("nan"));     assert rc == -1 and "bias" in msg and clean
    rc, msg, clean = hook(lib, lp, y, slab=0);                assert rc == -1 and "slab_rows >= 1" in msg and clean
    rc, msg, clean = hook(lib, lp, y, blank=8);               assert rc == -1 and "blank id outside" in msg and clean
