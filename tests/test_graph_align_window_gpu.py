"""The windowed graph aligner's kernels and driver (csrc/ctc_graph_window.hip) through the lab hook rvb_test_ctc_graph_window.  Every
comparison is exact -- == on labels, nodes, score bits and min_margin -- against the numpy band restatement
(tests/graph_align_window_ref.py) replaying the windows the kernel itself reported (lo_out): the only arithmetic is fp32 addition, so
there is no tolerance anywhere in this file.  Where the window holds the graph the bits are also those of the plain graph kernel
(rvb_test_ctc_viterbi_graph) and, on a chain, of the windowed chain kernel (rvb_test_ctc_viterbi_window)."""
import numpy as np
import pytest

import force_align_ref as R
import graph_align_ref as G
import graph_align_window_ref as WR
from reverb_amd import _lib
from test_graph_align_window_ref import EDGES, pack, small_graphs

pytestmark = pytest.mark.gpu


def hook(lib, lp, graph, window, slab, w=None, bias=0.0, lo_force=None):
    """-> rc, (labels, frame_node, score, lo_out, min_margin, launches)"""
    lp = np.ascontiguousarray(lp, np.float32)
    tok, off, prd, fin = pack(graph)
    T = len(lp)
    labels, fnode, lo = (np.full(T, -7, np.int32) for _ in range(3))
    score, margin, launches = np.full(1, 123.0, np.float32), np.full(1, -7, np.int32), np.full(1, -7, np.int32)
    force = None if lo_force is None else np.ascontiguousarray(lo_force, np.int32)
    rc = lib.rvb_test_ctc_graph_window(_lib.fptr(lp), T, lp.shape[1], None if w is None else _lib.fptr(w), bias, _lib.iptr(tok), len(graph[0]),
                                       _lib.iptr(off), _lib.iptr(prd), _lib.u8ptr(fin), 0, slab, window, _lib.iptr(force), _lib.iptr(labels),
                                       _lib.iptr(fnode), _lib.fptr(score), _lib.iptr(lo), _lib.iptr(margin), _lib.iptr(launches))
    if rc != 0:
        assert all(np.all(a == -7) for a in (labels, fnode, lo, margin, launches)) and score[0] == 123.0      # a refusal writes nothing
        return rc, None
    return rc, (labels, fnode, score[0], lo, int(margin[0]), int(launches[0]))


def same(got, want):
    bad = np.nonzero(got[0] != want[0])[0]
    assert bad.size == 0, "labels differ at %d frames, first %s" % (bad.size, bad[:5])
    bad = np.nonzero(got[1] != want[1])[0]
    assert bad.size == 0, "nodes differ at %d frames, first %s" % (bad.size, bad[:5])
    assert np.float32(got[2]).tobytes() == np.float32(want[2]).tobytes(), (got[2], want[2])


def lo_properties(lo, N, W):
    assert lo[0] == 0 and np.all(lo % 64 == 0) and np.all(np.diff(lo) >= 0) and lo[-1] <= max(0, WR.pad64(N) - W)


def run(lib, lp, graph, window, slab, w=None, bias=0.0, lo_force=None):
    """the hook against the band restatement on the hook's own windows; an infeasible band must be refused after the pass, and is
    then what the restatement says of the same windows (forced) or of its own drive (policy).  -> the hook's outputs, None if refused"""
    N = len(graph[0])
    W = WR.effective_window(N, window)
    rc, got = hook(lib, lp, graph, window, slab, w, bias, lo_force)
    if rc != 0:
        assert rc == -1 and b"infeasible: no path inside the window of %d nodes" % W in lib.rvb_last_error(), lib.rvb_last_error()
        with pytest.raises(ValueError, match="infeasible"):
            if lo_force is not None:
                WR.graph_align_band(lp, *graph, W, np.repeat(np.asarray(lo_force, np.int32), slab)[:len(lp)], w=w, bias=bias)
            else:
                WR.graph_align_window(lp, *graph, window, slab, w=w, bias=bias)
        return None
    want = WR.graph_align_band(lp, *graph, W, got[3], w=w, bias=bias)
    same(got, want)
    assert got[4] == want[3], ("min_margin", got[4], want[3])
    lo_properties(got[3], N, W)
    if lo_force is not None:
        assert got[3].tolist() == np.repeat(np.asarray(lo_force, np.int32), slab)[:len(lp)].tolist() and got[5] == len(lo_force)
    return got


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_many_shifts(lib, seed):
    lp, tokens, preds, finals, _ = WR.peaked_case("around", seed, 700, 12)
    graph = (tokens, preds, finals)
    free = G.graph_align(lp, *graph)
    for slab in (97, 600):                                        # a slab edge inside a launch's reach, and outside
        got = run(lib, lp, graph, 256, slab)
        same(got, free)
        assert got[4] > 0 and got[5] > 20 and len(set(got[3].tolist())) > 20        # the window really moved
        # the library cut the launches where the restatement's policy cuts them
        mine = WR.graph_align_window(lp, *graph, 256, slab)
        assert got[3].tolist() == mine[3].tolist() and got[5] == mine[5] and got[4] == mine[4]


@pytest.mark.parametrize("W,L", EDGES)
def test_every_instantiation_at_its_edge(lib, W, L):
    lp, tokens, preds, finals, _ = WR.peaked_case("groups", 5, L, 16)
    assert len(tokens) == 4 * L > W
    got = run(lib, lp, (tokens, preds, finals), W, 600)
    assert got[4] > 0 and len(set(got[3].tolist())) >= 3


def plain_graph_hook(lib, lp, graph, slab, w, bias):
    tok, off, prd, fin = pack(graph)
    T, nn = np.array([len(lp)], np.int32), np.array([len(graph[0])], np.int32)
    labels, fnode, score = np.full(len(lp), -7, np.int32), np.full(len(lp), -7, np.int32), np.zeros(1, np.float32)
    _lib.check(lib.rvb_test_ctc_viterbi_graph(_lib.fptr(lp), _lib.iptr(T), 1, lp.shape[1], _lib.fptr(w), bias, _lib.iptr(tok), _lib.iptr(nn),
                                              _lib.iptr(off), _lib.iptr(prd), _lib.u8ptr(fin), 0, slab, _lib.iptr(labels), _lib.iptr(fnode),
                                              _lib.fptr(score)), "rvb_test_ctc_viterbi_graph")
    return labels, fnode, score[0]


def test_a_window_that_holds_the_graph_is_the_plain_kernel(lib):
    n = 0
    for lp, graph in small_graphs():
        w = np.ascontiguousarray(lp.max(axis=1))
        N = len(graph[0])
        for bias in (0.0, -0.75):
            plain = plain_graph_hook(lib, lp, graph, 1000, w, bias)
            same(plain, G.graph_align(lp, *graph, w=w, bias=bias))
            for window in (0, 512):
                for slab in (64, 600):
                    got = run(lib, lp, graph, window, slab, w, bias)
                    same(got, plain)
                    W = WR.effective_window(N, window)
                    assert not got[3].any() and got[4] == W and got[5] == -(-len(lp) // slab)       # never moved, one launch per slab
                    n += 1
    assert n == 32
    # two and four nodes per thread
    for L, star in ((500, False), (800, True)):
        lp, y, _ = R.make_case(60 + L, int(2.2 * L), 24, L, "quant")
        graph = G.build(G.groups(np.random.default_rng(L), y, 24, n_alt=3, star=star))
        w = np.ascontiguousarray(lp.max(axis=1))
        assert 1024 < len(graph[0]) <= 8192
        same(run(lib, lp, graph, 0, 333, w, -0.5), plain_graph_hook(lib, lp, graph, 1000, w, -0.5))


def test_a_chain_is_the_windowed_chain_kernel(lib):
    for kind, wild in (("random", False), ("quant", True)):
        lp, y, T = R.make_case(11, 900, 32, 400, kind)
        y = np.array(y, np.int32)
        w = np.ascontiguousarray(lp.max(axis=1))
        if wild:
            y[::7] = G.W
        labels, lo = np.full(T, -7, np.int32), np.full(T, -7, np.int32)
        score, margin = np.zeros(1, np.float32), np.zeros(1, np.int32)
        _lib.check(lib.rvb_test_ctc_viterbi_window(_lib.fptr(lp), T, 32, _lib.fptr(w) if wild else None, -0.25 if wild else 0.0, _lib.iptr(y),
                                                   len(y), 0, 128, 1024, _lib.iptr(labels), _lib.fptr(score), _lib.iptr(lo),
                                                   _lib.iptr(margin)), "rvb_test_ctc_viterbi_window")
        assert not lo.any()                                       # 801 states in a window of 1024
        got = run(lib, lp, G.chain(y), 512, 128, w if wild else None, -0.25 if wild else 0.0)
        assert got[0].tolist() == labels.tolist() and np.float32(got[2]).tobytes() == score.tobytes() and not got[3].any()


def test_optional_wildcards_across_window_shifts(lib):
    lp, graph = WR.gap_case()
    assert len(graph[0]) == 5 * 300 - 1 and G.W in graph[0]
    w = np.ascontiguousarray(lp.max(axis=1))
    for bias in (-0.5, -1.5):
        got = run(lib, lp, graph, 256, 200, w, bias)
        assert len(set(got[3].tolist())) > 10 and int(np.sum(got[0] == G.W)) > 40      # the gaps went to wildcards, in many windows
        same(got, G.graph_align(lp, *graph, w=w, bias=bias))
    # bias 0: a wildcard costs what the best label costs, so a path that never leaves the first one ties with the best partial path
    # and, being the first maximum, holds the window back until the end is out of reach: the restatement decides, here "infeasible"
    assert run(lib, lp, graph, 256, 200, w, 0.0) is None
    # flat rows in multiples of 0.25: sums are exact and ties plentiful
    flat = np.ascontiguousarray(np.round(lp * 0.05 * 4) / 4)
    run(lib, flat, graph, 256, 200, np.ascontiguousarray(flat.max(axis=1)), -0.25)


def test_in_degree_64_inside_a_moving_window(lib):
    rng = np.random.default_rng(64)
    V = 40
    head, tail = rng.integers(1, V - 1, 300), rng.integers(1, V - 1, 300)
    for place in (0, 63):                                         # the spoken alternative first / last created = last / first listed
        alts = [int(a) for a in rng.integers(1, V - 1, 64)]
        alts[place] = V - 1                                       # the only alternative with this label
        y = np.concatenate([head, [V - 1], [7], tail])
        for i in range(1, len(y)):
            while y[i] == y[i - 1]:
                y[i] = rng.integers(1, V - 1)
        graph = G.build([("tok", t) for t in y[:300]] + [("choice", [[("tok", a)] for a in alts]), ("tok", y[301])] +
                        [("tok", t) for t in y[302:]])
        assert len(graph[1][364]) == 64 and WR.max_span(graph[1])[0] == 64
        lp = WR.peaked_lp(rng, y, 1000, V)
        got = run(lib, lp, graph, 256, 170)
        same(got, G.graph_align(lp, *graph))
        t = int(np.nonzero(got[1] == 364)[0][0])
        assert got[3][t] > 0 and 300 + place in got[1].tolist()      # the wide node was entered in a window that had moved


def test_a_predecessor_below_the_window_does_not_count(lib):
    lp, graph, force, lo_of = WR.cut_case()
    got = run(lib, lp, graph, WR.CUT_W, WR.CUT_SLAB, lo_force=force)
    path = set(got[1].tolist())
    assert 447 not in path and 548 in path and got[3].tolist() == lo_of.tolist()
    # jumped before any path can have reached the overlap of the two windows: the band holds no path, refused after the pass
    assert run(lib, lp, graph, WR.CUT_W, 300, lo_force=[0, WR.CUT_LO, WR.CUT_LO, WR.CUT_LO]) is None
    # the same lattice under the policy is the unwindowed alignment or at least a band alignment: the reference decides
    run(lib, lp, graph, WR.CUT_W, 300)


def test_minus_infinity_and_the_shortest_reading(lib):
    lp, tokens, preds, finals, y = WR.peaked_case("around", 4, 400, 12)
    graph = (tokens, preds, finals)
    hole = lp.copy()
    rng = np.random.default_rng(5)
    mask = rng.random(hole.shape) < 0.15
    mask[np.arange(len(hole)), hole.argmax(axis=1)] = False        # the peak of every row stays
    hole[mask] = -np.inf
    got = run(lib, hole, graph, 256, 150)
    assert got is not None and np.isfinite(got[2])
    dead = hole.copy()
    dead[300] = -np.inf                                           # a frame nothing can emit: every state is -inf from there on
    assert run(lib, dead, graph, 256, 150) is None
    # T = the frames of the shortest reading: every frame must advance, whatever the frames say
    T = WR.min_frames(*graph)
    short = np.ascontiguousarray(lp[:T])
    run(lib, short, graph, 256, 150)
    rc, _ = hook(lib, short[:T - 1], graph, 256, 150)
    assert rc == -1 and b"shortest reading needs at least %d frames" % T in lib.rvb_last_error()
