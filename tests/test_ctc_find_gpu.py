"""The CTC phrase-search kernel (csrc/ctc_find.hip) and its host code through the lab hook rvb_test_ctc_find: raw candidates and hits
IDENTICAL to the numpy reference (tests/ctc_find_ref.py, itself validated by exhaustive enumeration in test_ctc_find_ref.py) --
start, end and count as integers, the score as fp32 bits.  The kernel does one fp32 subtraction and one fp32 addition per cell and
comparisons, so there is nothing to tolerate."""
import numpy as np
import pytest

import ctc_find_ref as R
from reverb_amd import _lib

pytestmark = pytest.mark.gpu
BLANK = 0


def run(lib, lp, Ts, phrases, thr, slab, max_cand=64, max_hits=8, w=None, V=None):
    lp = np.ascontiguousarray(lp, np.float32)
    V = lp.shape[1] if V is None else V
    tok = np.ascontiguousarray(np.concatenate([np.asarray(p, np.int32) for p in phrases]), np.int32)
    tl = np.array([len(p) for p in phrases], np.int32)
    thr = np.asarray(thr, np.float32)
    Ts = np.asarray(Ts, np.int32)
    pairs = len(tl) * len(Ts)
    cnt = np.full(pairs, -7, np.int64)
    re_, rs, rv = np.full((pairs, max_cand), -7, np.int32), np.full((pairs, max_cand), -7, np.int32), np.full((pairs, max_cand), 123.0, np.float32)
    nh = np.full(pairs, -7, np.int32)
    hs, he, hv = np.full((pairs, max_hits), -7, np.int32), np.full((pairs, max_hits), -7, np.int32), np.full((pairs, max_hits), 123.0, np.float32)
    rc = lib.rvb_test_ctc_find(_lib.fptr(lp), _lib.iptr(Ts), len(Ts), V, None if w is None else _lib.fptr(w), _lib.iptr(tok), _lib.iptr(tl),
                               len(tl), _lib.fptr(thr), BLANK, slab, max_cand, max_hits, cnt.ctypes.data_as(_lib._i64p), _lib.iptr(re_),
                               _lib.iptr(rs), _lib.fptr(rv), _lib.iptr(nh), _lib.iptr(hs), _lib.iptr(he), _lib.fptr(hv))
    if rc != 0:
        return rc, lib.rvb_last_error().decode()
    out = []
    for p in range(pairs):
        k = int(min(cnt[p], max_cand))
        assert np.all(re_[p, k:] == -7) and np.all(rv[p, k:] == 123.0)        # slots past the kept ones are not written
        raw = [(int(re_[p, j]), int(rs[p, j]), rv[p, j].tobytes()) for j in range(k)]
        hits = [(int(hs[p, j]), int(he[p, j]), hv[p, j].tobytes()) for j in range(int(nh[p]))]
        out.append((int(cnt[p]), raw, hits))
    return 0, out


def want(lp, Ts, phrases, thr, max_cand=64, max_hits=8, w=None):
    lp = np.asarray(lp, np.float32)
    w = lp.max(axis=1) if w is None else w
    out, offs = [], np.concatenate([[0], np.cumsum(Ts)])
    for p, y in enumerate(phrases):
        for i in range(len(Ts)):
            a, b = int(offs[i]), int(offs[i + 1])
            n, kept, hits = R.find(lp[a:b], w[a:b], y, BLANK, thr[p], max_cand, max_hits)
            out.append((n, [(e, s, np.float32(v).tobytes()) for e, s, v in kept], [(s, e, np.float32(v).tobytes()) for s, e, v in hits]))
    return out


def case(seed, T, V, grid=False):
    rng = np.random.default_rng(seed)
    if grid:
        return -(rng.integers(0, 17, size=(T, V)).astype(np.float32) / 8.0)
    return np.log(rng.dirichlet(np.full(V, 0.3), size=T) + 1e-30).astype(np.float32)


def check(lib, lp, Ts, phrases, thr, slab, **kw):
    rc, got = run(lib, lp, Ts, phrases, thr, slab, **kw)
    assert rc == 0, got
    exp = want(lp, Ts, phrases, thr, **{k: v for k, v in kw.items() if k != "V"})
    assert got == exp
    return got


INF = -np.inf


def test_single_token_phrase(lib):
    got = check(lib, case(1, 37, 11), [37], [[4]], [INF], 64)
    assert got[0][0] >= 1


def test_two_tokens_equal_and_different(lib):
    lp = case(2, 37, 6)
    a = check(lib, lp, [37], [[3, 3]], [INF], 64)
    b = check(lib, lp, [37], [[3, 2]], [INF], 64)
    assert a[0][0] >= 1 and b[0][0] >= 1


def test_thirty_two_tokens_fill_the_wave_and_thirty_three_are_refused(lib):
    rng = np.random.default_rng(3)
    y = rng.integers(1, 40, size=32).tolist()
    y[5] = y[4]                                                 # one repeat
    lp = case(3, 90, 40)
    got = check(lib, lp, [90], [y], [INF], 64, max_cand=128)
    assert got[0][0] >= 1
    rc, msg = run(lib, lp, [90], [y + [7]], [INF], 64)
    assert rc == -5 and "33 tokens exceed the cap of 32" in msg


def test_one_frame_and_fewer_frames_than_tokens(lib):
    lp = case(4, 1, 6)
    got = check(lib, lp, [1], [[2], [2, 3]], [INF, INF], 64)
    assert got[0][0] == 1 and got[1] == (0, [], [])
    got = check(lib, case(5, 3, 6), [3], [[1, 1, 2, 3]], [INF], 64)          # needs 5 frames
    assert got[0] == (0, [], [])


@pytest.mark.parametrize("V,grid", [(5, True), (257, False)])
def test_slab_cuts_do_not_matter(lib, V, grid):
    lp = case(6, 37, V, grid)
    rng = np.random.default_rng(6)
    phrases = [[1], [2, 2], rng.integers(1, V, size=7).tolist(), [3, 1, 4]]
    thr = [INF] * len(phrases)
    runs = [check(lib, lp, [37], phrases, thr, slab) for slab in (1, 8, 37, 64)]
    assert runs[0] == runs[1] == runs[2] == runs[3]
    assert sum(r[0] for r in runs[0]) >= 10


def test_five_phrases_three_sequences(lib):
    V = 40
    rng = np.random.default_rng(7)
    Ts = [37, 1, 20]
    lp = case(7, sum(Ts), V)
    phrases = [rng.integers(1, V, size=n).tolist() for n in (1, 2, 7, 32, 3)]
    for slab in (64, 5):                                        # 15 pairs: 3 full workgroups and a quarter
        got = check(lib, lp, Ts, phrases, [INF] * 5, slab)
    assert len(got) == 15 and sum(g[0] for g in got) >= 10


def test_tie_inputs_of_the_cpu_test(lib):
    """the 1/8 grid at V = 5: every phrase of up to 3 tokens, where the tie order decides start frames and arrivals"""
    phrases = [list(y) for y in R.all_phrases(5, BLANK, 3)]
    for seed, T in enumerate([1, 2, 3, 4, 5, 6, 7, 7]):
        rng = np.random.default_rng(seed)
        lp = -(rng.integers(0, 17, size=(T, 5)).astype(np.float32) / 8.0)
        check(lib, lp, [T], phrases, [INF] * len(phrases), 3, max_cand=8)


def test_a_finite_threshold_splits_the_arrivals(lib):
    lp = case(8, 37, 6)
    allc = R.candidates(lp, lp.max(axis=1), [2, 5], BLANK, INF)
    cut = sorted(float(v) for _, _, v in allc)[len(allc) // 2]
    got = check(lib, lp, [37], [[2, 5], [2, 5]], [INF, cut], 8)
    assert 0 < got[1][0] < got[0][0] == len(allc)


def test_the_candidate_cap_keeps_the_first_and_counts_all(lib):
    lp, y, seed = None, [1], 0
    while True:                                                 # a case where the reference has exactly 5 arrivals
        lp = case(100 + seed, 12, 4)
        if len(R.candidates(lp, lp.max(axis=1), y, BLANK, INF)) == 5:
            break
        seed += 1
    got = check(lib, lp, [12], [y], [INF], 5, max_cand=2)
    assert got[0][0] == 5 and len(got[0][1]) == 2
    full = check(lib, lp, [12], [y], [INF], 5, max_cand=5)
    assert full[0][1][:2] == got[0][1]


def test_host_supplied_row_maxima_are_used(lib):
    """w is an input: with w = row maxima + 0.5 every score moves, and the hook's own maxima (w = null) equal numpy's"""
    lp = case(9, 20, 9)
    w = np.ascontiguousarray(lp.max(axis=1) + np.float32(0.5))
    check(lib, lp, [20], [[3, 1]], [INF], 7, w=w)
    rc, got = run(lib, lp, [20], [[3, 1]], [INF], 7, w=np.ascontiguousarray(lp.max(axis=1)))
    assert rc == 0 and got == check(lib, lp, [20], [[3, 1]], [INF], 7)
