"""The graph aligner's kernels (csrc/ctc_graph.hip) through the lab hook rvb_test_ctc_viterbi_graph, against the numpy restatement
tests/graph_align_ref.py and, on chains, against the shipped chain aligner (rvb_test_ctc_viterbi_wild).  Labels and nodes are compared
identically and scores bit for bit: the only arithmetic is fp32 addition, so there is no tolerance anywhere in this file."""
import numpy as np
import pytest

import force_align_ref as R
import graph_align_ref as G
from reverb_amd import _lib

pytestmark = pytest.mark.gpu
W = G.W
BIASES = (0.0, -0.75)


def pack(graphs):
    tok = np.concatenate([np.asarray(g[0], np.int32) for g in graphs])
    nn = np.array([len(g[0]) for g in graphs], np.int32)
    off = np.concatenate([np.concatenate([[0], np.cumsum([len(p) for p in g[1]])]) for g in graphs]).astype(np.int32)
    prd = np.array([p for g in graphs for ps in g[1] for p in ps], np.int32)
    fin = np.concatenate([np.asarray(g[2], np.uint8) for g in graphs])
    return tuple(np.ascontiguousarray(a) for a in (tok, nn, off, prd, fin))


def hook(lib, lps, graphs, slab, w="rows", bias=0.0, blank=0):
    """-> rc, [(labels, frame_node, score) per lattice]"""
    lp = np.ascontiguousarray(np.concatenate(lps))
    Ts = np.array([len(x) for x in lps], np.int32)
    wv = np.ascontiguousarray(lp.max(axis=1)) if isinstance(w, str) else w
    tok, nn, off, prd, fin = pack(graphs)
    labels, fnode = np.full(len(lp), -7, np.int32), np.full(len(lp), -7, np.int32)
    score = np.full(len(lps), 123.0, np.float32)
    rc = lib.rvb_test_ctc_viterbi_graph(_lib.fptr(lp), _lib.iptr(Ts), len(lps), lp.shape[1], _lib.fptr(wv), bias, _lib.iptr(tok), _lib.iptr(nn),
                                        _lib.iptr(off), _lib.iptr(prd), _lib.u8ptr(fin), blank, slab, _lib.iptr(labels), _lib.iptr(fnode),
                                        _lib.fptr(score))
    if rc != 0:
        assert np.all(labels == -7) and np.all(fnode == -7) and np.all(score == 123.0)      # a refusal writes nothing
        return rc, None
    ends = np.cumsum(Ts)
    return rc, [(labels[e - t:e], fnode[e - t:e], score[i]) for i, (e, t) in enumerate(zip(ends, Ts))]


def run(lib, lp, graph, slab, bias=0.0):
    rc, out = hook(lib, [lp], [graph], slab, bias=bias)
    _lib.check(rc, "rvb_test_ctc_viterbi_graph")
    return out[0]


def same(got, want):
    bad = np.nonzero(got[0] != want[0])[0]
    assert bad.size == 0, "labels differ at %d frames, first %s" % (bad.size, bad[:5])
    bad = np.nonzero(got[1] != want[1])[0]
    assert bad.size == 0, "nodes differ at %d frames, first %s" % (bad.size, bad[:5])
    assert np.float32(got[2]).tobytes() == np.float32(want[2]).tobytes(), (got[2], want[2])


def truth(lp, graph, bias=0.0):
    return G.graph_align(lp, *graph, w=lp.max(axis=1), bias=bias)


def chain_hook(lib, lp, w, bias, y, slab):
    T, V = lp.shape
    labels, score = np.full(T, -7, np.int32), np.zeros(1, np.float32)
    _lib.check(lib.rvb_test_ctc_viterbi_wild(_lib.fptr(lp), T, V, _lib.fptr(w), bias, _lib.iptr(np.ascontiguousarray(y, np.int32)), len(y), 0,
                                             slab, _lib.iptr(labels), _lib.fptr(score)), "rvb_test_ctc_viterbi_wild")
    return labels, score[0]


SMALL = [(1, 1), (7, 2)]
LARGE = [(512, 199), (8192 + 3, 3000)]


@pytest.mark.parametrize("kind", ["random", "quant"])
@pytest.mark.parametrize("T,L", SMALL + LARGE)
def test_chains_equal_the_restatement_and_the_shipped_aligner(lib, T, L, kind):
    lp, y, _ = R.make_case(300 + T % 97 + L, T, 48, L, kind)
    w = np.ascontiguousarray(lp.max(axis=1))
    slabs = (8192, 64, 1) if (T, L) in SMALL else (8192, 1000)
    yw = np.array(y, np.int32)
    yw[::5] = W
    for tokens, biases in ((y, (0.0,)), (yw, BIASES)):
        for bias in biases:
            want = truth(lp, G.chain(tokens), bias)
            shipped = chain_hook(lib, lp, w, bias, tokens, 1000)
            assert shipped[0].tolist() == want[0].tolist() and np.float32(shipped[1]).tobytes() == want[2].tobytes()
            for slab in slabs:
                same(run(lib, lp, G.chain(tokens), slab, bias), want)


# N about 50 (one node per thread), about 1000 (the largest one-per-thread grid), and more than 2048 (four per thread)
@pytest.mark.parametrize("kind", ["random", "quant"])
@pytest.mark.parametrize("L,T,star", [(20, 90, 0.0), (20, 90, 0.5), (400, 1300, 0.0), (400, 1300, 0.3), (1000, 2500, 0.2)])
def test_random_graphs_of_alternatives_and_optionals(lib, L, T, star, kind):
    lp, y, _ = R.make_case(17 + L, T, 40, L, kind)
    graph = G.build(G.around(np.random.default_rng([L, int(star * 10)]), y, 40, p_star=star))
    assert any(len(p) > 1 for p in graph[1]) and sum(graph[2]) >= 1
    for bias in (BIASES if star else (0.0,)):
        want = truth(lp, graph, bias)
        for slab in (8192, 333):
            same(run(lib, lp, graph, slab, bias), want)


@pytest.mark.parametrize("kind", ["random", "quant"])
def test_exactly_the_node_cap(lib, kind):
    """2048 groups of 4 single-node alternatives = 8192 nodes (eight per thread, every LDS slot), each node with 4 predecessors"""
    lp, y, _ = R.make_case(5, 2600, 32, 2048, kind)
    graph = G.build(G.groups(np.random.default_rng(8), y, 32))
    assert len(graph[0]) == 8192 and len(graph[1][-1]) == 4
    want = truth(lp, graph)
    same(run(lib, lp, graph, 8192), want)
    same(run(lib, lp, graph, 1000), want)


def test_an_optional_wildcard_between_all_groups(lib):
    """1300 groups of 4 with [<star>] between them: 6499 nodes (eight per thread), in-degree 5, 31 180 of the 32 768 arcs a graph may have"""
    lp, y, _ = R.make_case(6, 2600, 32, 1300, "quant")
    graph = G.build(G.groups(np.random.default_rng(9), y, 32, star=True))
    assert len(graph[0]) == 1300 * 5 - 1 and sum(map(len, graph[1])) == 4 + 1299 * 24
    for bias in BIASES:
        same(run(lib, lp, graph, 1000, bias), truth(lp, graph, bias))


def test_in_degree_64_and_the_last_listed_predecessor(lib):
    lp, y, _ = R.make_case(21, 40, 48, 3, "quant")
    # 64 alternatives for y[1], the right one LAST created = first listed; then the same with it first created = last listed
    for place in (63, 0):
        alts = [int(a) for a in np.random.default_rng(place).integers(1, 48, 64)]
        alts[place] = int(y[1])
        graph = G.build([("tok", y[0]), ("choice", [[("tok", a)] for a in alts]), ("tok", y[2])])
        assert len(graph[1][-1]) == 64
        got = run(lib, lp, graph, 7)
        same(got, truth(lp, graph))
    # only the last-listed predecessor is feasible: every other alternative's log-prob is -inf
    lp2 = lp.copy()
    alts = [47] + list(range(1, 46)) + list(range(1, 19))
    graph = G.build([("choice", [[("tok", a)] for a in alts]), ("tok", 46)])
    lp2[:, 1:46] = -np.inf
    want = truth(lp2, graph)
    got = run(lib, lp2, graph, 8192)
    same(got, want)
    assert len(alts) == 64 and graph[1][64][-1] == 0 and sorted(set(got[1].tolist()) - {-1}) == [0, 64]


def test_far_predecessors_cross_every_threads_range(lib):
    """a chain of 8192 nodes (eight per thread) that 600 frames can only cross over far arcs"""
    N, T = 8192, 600
    rng = np.random.default_rng(4)
    # every 97th node also listens to a random earlier node and node 8191 to node 0: 600 frames reach the end only over such arcs
    tokens = rng.integers(1, 32, N).astype(np.int32)
    preds = [[j - 1] for j in range(N)]
    for j in range(97, N, 97):
        preds[j].append(int(rng.integers(0, j - 1)))
    preds[N - 1].append(0)
    finals = [j == N - 1 for j in range(N)]
    lp, _, _ = R.make_case(9, T, 32, 2, "quant")
    got = run(lib, lp, (tokens, preds, finals), 250)
    same(got, truth(lp, (tokens, preds, finals)))
    path = sorted(set(got[1].tolist()) - {-1})
    assert path[0] == 0 and path[-1] == N - 1 and max(b - a for a, b in zip(path, path[1:])) > 4096
    # an express lane: every 41st node also listens to the node 41 behind it (another thread, another wave, and across the eight
    # node ranges of a thread), the last node to the lane's end; the planted transcript lies on the lane, and the stretches of the
    # plain chain between two lane nodes compete with each arc
    lane = list(range(0, N - 1, 41))
    lp, y, _ = R.make_case(10, T, 32, len(lane) + 1, "quant")
    tokens = rng.integers(1, 32, N).astype(np.int32)
    tokens[lane + [N - 1]] = y
    preds = [[j - 1] for j in range(N)]
    for a, b in zip(lane, lane[1:] + [N - 1]):
        preds[b].append(a)
    graph = (tokens, preds, finals)
    want = truth(lp, graph)
    path = sorted(set(want[1].tolist()) - {-1})
    assert len(lane) == 200 and path[0] == 0 and path[-1] == N - 1 and len(set(lane) & set(path)) >= 150
    for slab in (8192, 250):
        same(run(lib, lp, graph, slab), want)


def test_same_label_predecessors_do_not_take_the_token_arc(lib):
    # a a: the second a must be entered through the blank, also as an alternative and from a far predecessor
    lp, y, _ = R.make_case(2, 12, 8, 4, "quant")
    a = int(y[0])
    for items in ([("tok", a), ("tok", a)], [("tok", a), ("choice", [[("tok", a)], [("tok", 5)]]), ("tok", a)],
                  [("tok", W), ("choice", [[("tok", W)], []]), ("tok", a), ("choice", [[("tok", 3)], []]), ("tok", a)]):
        graph = G.build(items)
        for bias in BIASES:
            for T in range(len(graph[0]), 12):
                want = None
                try:
                    want = truth(lp[:T], graph, bias)
                except ValueError:
                    pass
                rc, out = hook(lib, [lp[:T]], [graph], 5, bias=bias)
                if want is None:
                    assert rc == -1 and b"infeasible" in lib.rvb_last_error()
                else:
                    assert rc == 0
                    same(out[0], want)


def test_ties_between_finals_and_the_minimum_T(lib):
    # two finals with the same label after a common prefix: equal scores, the first in index order wins (B before T)
    lp, y, _ = R.make_case(31, 30, 16, 5, "quant")
    graph = G.build([("tok", t) for t in y[:4]] + [("choice", [[("tok", y[4])], [("tok", y[4])]])])
    want = truth(lp, graph)
    got = run(lib, lp, graph, 8)
    same(got, want)
    assert got[1][got[1] >= 0][-1] == 4
    # T = the shortest path's minimum: optional words cannot be taken, repeats need their blank
    yy = [3, 3, 5]
    graph = G.build([("tok", 3), ("choice", [[("tok", 7), ("tok", 7)], []]), ("tok", 3), ("tok", 5)])
    lp4 = np.ascontiguousarray(lp[:4])
    want = truth(lp4, graph)
    got = run(lib, lp4, graph, 8192)
    same(got, want)
    assert R.collapse(got[0]).tolist() == yy
    rc, _ = hook(lib, [lp[:3]], [graph], 8192)
    assert rc == -1 and b"sequence 0: infeasible" in lib.rvb_last_error()


def test_three_lattices_of_very_different_sizes_in_one_call(lib):
    cases = []
    for seed, (L, T) in enumerate([(3, 9), (1500, 2400), (60, 700)]):
        lp, y, _ = R.make_case(50 + seed, T, 36, L, "quant")
        graph = G.build(G.around(np.random.default_rng(seed), y, 36, p_star=0.2 if seed else 0.0))
        cases.append((lp, graph))
    assert max(len(g[0]) for _, g in cases) > 2048
    for bias in BIASES:
        wants = [truth(lp, g, bias) for lp, g in cases]
        for slab in (8192, 500):
            rc, out = hook(lib, [c[0] for c in cases], [c[1] for c in cases], slab, bias=bias)
            assert rc == 0
            for got, want in zip(out, wants):
                same(got, want)
