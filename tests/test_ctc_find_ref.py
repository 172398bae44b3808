"""The numpy reference of the CTC phrase search (tests/ctc_find_ref.py) against exhaustive enumeration, on inputs where fp32 sums are
exact and ties are frequent; a planted phrase; the suppression rule on hand-made lists.  No GPU."""
import numpy as np

import ctc_find_ref as R

V, BLANK = 5, 0


def grid_case(seed, T):
    """log-probs on a grid of 1/8 in [-2, 0]: every sum of up to T of them (and of the row maxima) is exact in fp32"""
    rng = np.random.default_rng(seed)
    lp = -(rng.integers(0, 17, size=(T, V)).astype(np.float32) / 8.0)
    return lp, lp.max(axis=1)


def test_reference_equals_exhaustive_enumeration():
    n_arrivals, stats = 0, {}
    for seed, T in enumerate([1, 2, 3, 4, 5, 6, 7, 7]):
        lp, w = grid_case(seed, T)
        for y in R.all_phrases(V, BLANK, 3):
            got = R.candidates(lp, w, y, BLANK, -np.inf)
            want = R.brute_force(lp, w, y, BLANK, stats)
            assert [(e, s) for e, s, _ in got] == [(e, s) for e, s, _ in want], (seed, T, y)
            assert [float(v) for _, _, v in got] == [v for _, _, v in want], (seed, T, y)
            n_arrivals += len(got)
    print("arrivals", n_arrivals, "frames whose best score several paths reach", stats["ties"])
    assert n_arrivals > 1000 and stats["ties"] > 100   # the cases do exercise arrivals, and the tie order


def test_a_planted_phrase_scores_zero_at_its_frames():
    rng = np.random.default_rng(5)
    T, y = 30, [3, 3, 1, 4]
    lp = np.log(rng.dirichlet(np.ones(V), size=T)).astype(np.float32)
    path = {10: 3, 11: 3, 12: 0, 13: 3, 14: 1, 15: 4, 16: 4}        # 3 3 b 3 1 4 4: the repeat needs its blank
    for t in range(T):
        top = path.get(t, 2)                                        # elsewhere token 2, which the phrase does not hold
        lp[t, top] = lp[t].max() + np.float32(0.5)
    w = lp.max(axis=1)
    got = R.candidates(lp, w, y, BLANK, -np.inf)
    zero = [(e, s) for e, s, v in got if v == 0.0]
    assert zero == [(15, 10)]                                       # the arrival: the first frame of the last token
    assert all(v < 0.0 for e, s, v in got if (e, s) != (15, 10))
    hits = R.suppress(got, 4)
    assert (10, 15, np.float32(0.0)) in hits
    assert R.candidates(lp, w, y, BLANK, 0.0) == [(15, 10, np.float32(0.0))]


def test_threshold_and_cap():
    lp, w = grid_case(11, 7)
    allc = R.candidates(lp, w, [1], BLANK, -np.inf)
    assert len(allc) >= 3
    cut = sorted(float(v) for _, _, v in allc)[len(allc) // 2]
    some = R.candidates(lp, w, [1], BLANK, cut)
    assert some == [c for c in allc if c[2] >= cut] and 0 < len(some) < len(allc)
    n, kept, hits = R.find(lp, w, [1], BLANK, -np.inf, 2, 8)
    assert n == len(allc) and kept == allc[:2]
    assert hits == R.suppress(allc[:2], 8)


def test_suppression_on_hand_made_lists():
    f = np.float32
    # (end, start, score)
    c = [(5, 2, f(-1.0)), (6, 4, f(-0.5)), (9, 7, f(-2.0)), (12, 6, f(-0.25)), (20, 20, f(-3.0))]
    # -0.25 [6, 12] wins and removes [4, 6] (meets at 6) and [7, 9]; [2, 5] and [20, 20] stay
    assert R.suppress(c, 8) == [(2, 5, f(-1.0)), (6, 12, f(-0.25)), (20, 20, f(-3.0))]
    assert R.suppress(c, 2) == [(2, 5, f(-1.0)), (6, 12, f(-0.25))]             # the two best, in order of end
    assert R.suppress(c, 1) == [(6, 12, f(-0.25))]
    # equal scores: the earlier end first, then the earlier start
    c = [(8, 5, f(-1.0)), (6, 3, f(-1.0)), (6, 2, f(-1.0))]
    assert R.suppress(c, 8) == [(2, 6, f(-1.0))]
    c = [(8, 7, f(-1.0)), (6, 3, f(-1.0)), (6, 2, f(-1.0))]
    assert R.suppress(c, 8) == [(2, 6, f(-1.0)), (7, 8, f(-1.0))]
    # touching spans overlap ([a, b] is closed), neighbours do not
    assert R.suppress([(4, 0, f(-1.0)), (9, 4, f(-2.0))], 8) == [(0, 4, f(-1.0))]
    assert R.suppress([(4, 0, f(-1.0)), (9, 5, f(-2.0))], 8) == [(0, 4, f(-1.0)), (5, 9, f(-2.0))]
    assert R.suppress([], 3) == []
