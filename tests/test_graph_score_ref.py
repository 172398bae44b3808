"""The fp64 restatement of the full-sum score over a token graph (tests/graph_score_ref.py) against what is known independently: the
chain reference (ctc_score_ref), enumeration of the readings (ctc_score_ref.loglik per node path of graph_align_ref.paths), and the
identities the definitions imply."""
import numpy as np
import pytest

import ctc_score_ref as C
import graph_align_ref as G
import graph_score_ref as R

V = 12


def _lp(seed, T, scale=2.0):
    lp, _ = C.make_lattice(seed, T, V, 1, scale=scale)
    return lp


def _enumerate(lp, tokens, preds, finals):
    """-> (loglik, visit per node) by summing ctc_score_ref.loglik over every node path"""
    ps = G.paths(preds, finals)
    lls = np.array([C.loglik(lp, [tokens[j] for j in p]) for p in ps])
    m = lls.max()
    ll = m + np.log(np.exp(lls - m).sum())
    visit = np.zeros(len(tokens))
    for p, l in zip(ps, lls):
        visit[p] += np.exp(l - ll)
    return ll, visit, ps, lls


@pytest.mark.parametrize("L,T,repeats", [(1, 1, ()), (1, 7, ()), (5, 12, (2,)), (9, 30, (3, 4)), (40, 60, (10,))])
def test_a_chain_is_the_chain_reference(L, T, repeats):
    lp, y = C.make_lattice(3, T, V, L, scale=2.0, repeats_at=repeats)
    ll0, ref = C.score(lp, y)
    ll, out = R.score(lp, *G.chain(y))
    assert abs(ll - ll0) < 1e-10
    assert abs(R.loglik(lp, *G.chain(y)) - ll0) < 1e-10
    for k in ("occupancy", "mean_frame", "peak_post"):
        np.testing.assert_allclose(out[k], ref[k], rtol=1e-9, atol=1e-12)
    np.testing.assert_array_equal(out["peak_frame"], ref["peak_frame"])
    np.testing.assert_allclose(out["visit"], 1.0, atol=1e-10)


@pytest.mark.parametrize("seed", range(12))
def test_random_graphs_against_enumeration(seed):
    rng = np.random.default_rng(seed)
    y = [int(t) for t in rng.integers(1, V, 5)]
    items = G.around(rng, y, V) if seed % 2 == 0 else G.groups(rng, y[:4], V, n_alt=3)
    tokens, preds, finals = G.build(items)
    lp = _lp(seed, 2 * len(tokens) + 6)
    ll0, visit0, _, _ = _enumerate(lp, tokens, preds, finals)
    ll, out = R.score(lp, tokens, preds, finals)
    assert abs(ll - ll0) < 1e-10
    assert abs(R.loglik(lp, tokens, preds, finals) - ll) < 1e-12
    np.testing.assert_allclose(out["visit"], visit0, atol=1e-10)
    assert np.all(out["occupancy"] >= out["visit"] - 1e-12)      # a visited node holds at least one frame
    assert np.all(out["peak_post"] <= 1 + 1e-12)


def test_two_paths_that_spell_the_same_count_twice():
    lp = _lp(1, 9)
    a = [3, 5]
    tokens, preds, finals = G.build([("choice", [[("tok", t) for t in a], [("tok", t) for t in a]])])
    ll, out = R.score(lp, tokens, preds, finals)
    assert abs(ll - (C.loglik(lp, a) + np.log(2.0))) < 1e-12
    np.testing.assert_allclose(out["visit"], 0.5, atol=1e-12)


def test_the_openings_of_a_group_and_its_skip_sum_to_one():
    rng = np.random.default_rng(5)
    lp = _lp(5, 20)
    items = [("tok", 2), ("choice", [[("tok", 4), ("tok", 5)], [("tok", 6)], [("tok", 7), ("tok", 4)]]), ("tok", 3),
             ("choice", [[("tok", 8), ("tok", 9)], []]), ("tok", 1)]
    tokens, preds, finals = G.build(items)
    ll, out = R.score(lp, tokens, preds, finals)
    assert abs(out["visit"][[1, 3, 4]].sum() - 1.0) < 1e-10      # the three branches of the first group open at nodes 1, 3 and 4
    _, _, ps, lls = _enumerate(lp, tokens, preds, finals)
    opening = 7                                                  # the optional group opens at node 7 (tokens 8 9)
    assert tokens[opening] == 8
    skip = sum(np.exp(l - ll) for p, l in zip(ps, lls) if opening not in p)
    assert 0 < skip < 1 and abs(out["visit"][opening] + skip - 1.0) < 1e-10
    assert abs(out["visit"][0] - 1.0) < 1e-10 and abs(out["visit"][-1] - 1.0) < 1e-10


@pytest.mark.parametrize("seed", range(4))
def test_the_sum_is_no_less_than_the_best_path(seed):
    rng = np.random.default_rng(100 + seed)
    y = [int(t) for t in rng.integers(1, V, 8)]
    tokens, preds, finals = G.build(G.around(rng, y, V))
    lp = _lp(seed, 2 * len(tokens) + 4)
    _, _, best = G.graph_align(lp, tokens, preds, finals)
    assert R.loglik(lp, tokens, preds, finals) >= float(best) - 1e-3     # the fp32 rounding of the Viterbi sum


def test_no_mass_gives_mean_frame_minus_one_and_an_infeasible_graph_raises():
    lp = _lp(2, 6).astype(np.float64)
    lp[:, 7] = -np.inf                                           # token 7 cannot be emitted: its branch carries nothing
    tokens, preds, finals = G.build([("tok", 2), ("choice", [[("tok", 7)], [("tok", 5)]])])
    ll, out = R.score(lp, tokens, preds, finals)
    assert out["occupancy"][1] == 0 and out["mean_frame"][1] == -1 and out["visit"][1] == 0
    assert not np.any(np.isnan(np.concatenate([out[k] for k in ("visit", "occupancy", "mean_frame", "peak_post")])))
    with pytest.raises(ValueError, match="infeasible"):
        R.loglik(lp[:1], *G.chain([2, 5]))


def test_a_large_graph_runs_in_seconds():
    rng = np.random.default_rng(0)
    y = [int(t) for t in rng.integers(1, V, 1025)]
    tokens, preds, finals = G.build(G.groups(rng, y, V, n_alt=4))            # 4100 nodes, in-degree 4, readings of 1025 tokens
    assert len(tokens) == 4100
    lp = _lp(0, 1100)
    ll, out = R.score(lp, tokens, preds, finals)
    assert np.isfinite(ll) and abs(R.loglik(lp, tokens, preds, finals) - ll) < 1e-9
    np.testing.assert_allclose(out["visit"].reshape(-1, 4).sum(1), 1.0, atol=1e-9)   # the four openings of every group
