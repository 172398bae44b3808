"""The windowed graph Viterbi without a GPU: the numpy band restatement (tests/graph_align_window_ref.py) against the unwindowed one
(tests/graph_align_ref.py), the window policy of the library (rvb_test_ctc_graph_window_next, host code) against the restatement's, the
restatement driven by that policy on peaked lattices, the refusals of the lab hook rvb_test_ctc_graph_window, which all come before
any device work, and align_wav's parser."""
import numpy as np
import pytest

import force_align_ref as R
import graph_align_ref as G
import graph_align_window_ref as WR
from reverb_amd import _lib

EDGES = [(1024, 400), (2048, 800), (4096, 1600), (8192, 2600)]       # (W, L): groups graphs of 4 L nodes, just above each instantiation


def same(got, want):
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.float32(got[2]).tobytes() == np.float32(want[2]).tobytes()


def pack(graph):
    tok = np.ascontiguousarray(graph[0], np.int32)
    off = np.concatenate([[0], np.cumsum([len(p) for p in graph[1]])]).astype(np.int32)
    prd = np.array([p for ps in graph[1] for p in ps], np.int32)
    fin = np.ascontiguousarray(graph[2], np.uint8)
    return tok, np.ascontiguousarray(off), np.ascontiguousarray(prd), fin


def small_graphs():
    for seed, (kind, kw) in enumerate([("around", {}), ("around", {"p_star": 0.3}), ("groups", {}), ("groups", {"star": True})]):
        lp, y, _ = R.make_case(40 + seed, 260, 24, 90, "quant" if seed % 2 else "random")
        rng = np.random.default_rng(seed)
        yield lp, G.build(G.around(rng, y, 24, **kw) if kind == "around" else G.groups(rng, y, 24, **kw))


def test_a_band_that_never_moves_is_the_unwindowed_alignment():
    n = 0
    for lp, graph in small_graphs():
        w = np.ascontiguousarray(lp.max(axis=1))
        for bias in (0.0, -0.75):
            want = G.graph_align(lp, *graph, w=w, bias=bias)
            W = WR.effective_window(len(graph[0]), 0)
            got = WR.graph_align_band(lp, *graph, W, np.zeros(len(lp), np.int32), w=w, bias=bias)
            same(got, want)
            assert got[3] == W                                    # no frame counts: both edges are the graph's own
            drv = WR.graph_align_window(lp, *graph, 0, 37, w=w, bias=bias)
            same(drv, want)
            assert not drv[3].any() and drv[4] == W and drv[5] == -(-len(lp) // 37)        # one launch per slab
            n += 1
    assert n == 8


def policy(lib, graph, T, V, window, queries):
    tok, off, prd, fin = pack(graph)
    q = [np.ascontiguousarray([x[k] for x in queries], np.int32) for k in range(4)]
    lo, f1 = np.full(len(queries), -7, np.int32), np.full(len(queries), -7, np.int32)
    rc = lib.rvb_test_ctc_graph_window_next(_lib.iptr(tok), len(tok), _lib.iptr(off), _lib.iptr(prd), _lib.u8ptr(fin), T, V, window,
                                            len(queries), *[_lib.iptr(a) for a in q], _lib.iptr(lo), _lib.iptr(f1))
    assert rc == 0, lib.rvb_last_error()
    return lo, f1


def test_the_policy_of_the_library_is_the_restatements(lib):
    rng = np.random.default_rng(2026)
    total = 0
    for g in range(12):
        V = 12
        L = int(rng.integers(150, 700))
        y = rng.integers(1, V, L)
        kind = g % 3
        items = G.around(rng, y, V, p_star=0.2 if kind == 1 else 0.0) if kind < 2 else G.groups(rng, y, V, star=bool(g % 2))
        graph = G.build(items)
        N = len(graph[0])
        Wn = int(rng.choice([256, 512, 1024]))
        W = WR.effective_window(N, Wn)
        tab = WR.tables(*graph)
        T = int(WR.min_frames(*graph) + rng.integers(0, 2 * L))
        top = max(0, WR.pad64(N) - W)
        queries = [(0, int(rng.integers(1, T + 1)), 0, -1)]
        for _ in range(200):
            f0 = int(rng.integers(0, T))
            fend = int(rng.integers(f0 + 1, min(T, f0 + 3 * W) + 1))
            lo_prev = 0 if f0 == 0 else int(rng.integers(0, top // 64 + 1)) * 64
            hi = min(lo_prev + W, N)
            best = -1 if f0 == 0 or rng.random() < 0.05 else int(rng.integers(lo_prev, hi))
            queries.append((f0, fend, lo_prev, best))
        lo, f1 = policy(lib, graph, T, V, Wn, queries)
        for (f0, fend, lo_prev, best), got_lo, got_f1 in zip(queries, lo.tolist(), f1.tolist()):
            want = WR.next_window(tab, N, T, W, f0, fend, lo_prev, best)
            assert (got_lo, got_f1) == want, (N, T, W, f0, fend, lo_prev, best, got_lo, got_f1, want)
            assert got_lo % 64 == 0 and lo_prev <= got_lo <= top and f0 < got_f1 <= fend
            assert got_lo == 0 or f0 > 0
            assert got_lo + W - 1 >= tab[3][min(T - got_f1, len(tab[3]) - 1)]          # the end stays reachable
        total += len(queries)
    assert total >= 2000


def test_the_policy_follows_the_library_launch_after_launch(lib):
    """the policy called as the driver calls it: every launch's answer feeds the next, with arbitrary best nodes inside the window"""
    rng = np.random.default_rng(77)
    lp, tokens, preds, finals, _ = WR.peaked_case("around", 1, 300, 12)
    graph = (tokens, preds, finals)
    N, T, W = len(tokens), len(lp), 256
    tab = WR.tables(*graph)
    queries, lo, f0 = [], 0, 0
    while f0 < T:
        fend = min(T, (f0 // 97 + 1) * 97)
        best = -1 if f0 == 0 else int(rng.integers(lo, min(lo + W, N)))
        queries.append((f0, fend, lo, best))
        lo, f0 = WR.next_window(tab, N, T, W, f0, fend, lo, best)
    got_lo, got_f1 = policy(lib, graph, T, 12, W, queries)
    assert [(a, b) for a, b in zip(got_lo.tolist(), got_f1.tolist())] == [WR.next_window(tab, N, T, W, *q) for q in queries]
    assert lo + W >= N - 1 or tab[3][0] <= lo + W - 1


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_many_shifts_on_a_planted_reading(seed):
    for kind, L, V, slab in (("around", 700, 12, 97), ("groups", 500, 12, 600)):
        lp, tokens, preds, finals, y = WR.peaked_case(kind, seed, L, V)
        want = G.graph_align(lp, tokens, preds, finals)
        labels, fnode, score, lo, margin, launches = WR.graph_align_window(lp, tokens, preds, finals, 256, slab)
        same((labels, fnode, score), want)
        assert margin > 0 and launches > 20 and len(set(lo.tolist())) > 20         # the window really moved
        assert np.all(np.diff(lo) >= 0) and np.all(lo % 64 == 0) and lo[0] == 0
        same(WR.graph_align_band(lp, tokens, preds, finals, 256, lo), want)        # the same band, replayed


@pytest.mark.parametrize("W,L", EDGES)
def test_every_instantiation_at_its_edge(W, L):
    lp, tokens, preds, finals, _ = WR.peaked_case("groups", 5, L, 16)
    assert len(tokens) == 4 * L > W
    want = G.graph_align(lp, tokens, preds, finals)
    labels, fnode, score, lo, margin, _ = WR.graph_align_window(lp, tokens, preds, finals, W, 600)
    same((labels, fnode, score), want)
    assert margin > 0 and len(set(lo.tolist())) >= 3


def test_a_band_that_cuts_a_predecessor_off():
    lp, graph, force, lo_of = WR.cut_case()
    labels, fnode, score, margin = WR.graph_align_band(lp, *graph, WR.CUT_W, lo_of)
    path = set(fnode.tolist())
    assert 447 not in path and set(range(448, 549)) <= path           # the reading through b is gone, the one through c stays
    assert margin < 64                                               # the path crossed the jump inside the overlap of the two windows
    assert G.graph_align(lp, *graph)[2] >= score
    with pytest.raises(ValueError, match="infeasible"):               # a jump before any path can have reached the overlap
        WR.graph_align_band(lp, *graph, WR.CUT_W, np.where(np.arange(len(lp)) < 300, 0, WR.CUT_LO))


def hook(lib, lp, graph, window=0, w=None, bias=0.0, slab=64, T=None, blank=0, lo_force=None):
    lp = np.ascontiguousarray(lp, np.float32)
    tok, off, prd, fin = pack(graph)
    T = lp.shape[0] if T is None else T
    n = max(min(T, 1 << 16), 1)
    labels, fnode, lo = (np.full(n, -7, np.int32) for _ in range(3))
    score, margin, launches = np.full(1, 123.0, np.float32), np.full(1, -7, np.int32), np.full(1, -7, np.int32)
    force = None if lo_force is None else np.ascontiguousarray(lo_force, np.int32)
    rc = lib.rvb_test_ctc_graph_window(_lib.fptr(lp), T, lp.shape[1], None if w is None else _lib.fptr(w), bias, _lib.iptr(tok), len(graph[0]),
                                       _lib.iptr(off), _lib.iptr(prd), _lib.u8ptr(fin), blank, slab, window, _lib.iptr(force),
                                       _lib.iptr(labels), _lib.iptr(fnode), _lib.fptr(score), _lib.iptr(lo), _lib.iptr(margin), _lib.iptr(launches))
    untouched = all(np.all(a == -7) for a in (labels, fnode, lo, margin, launches)) and score[0] == 123.0
    return rc, lib.rvb_last_error().decode(), untouched


def test_the_hook_refuses_before_any_device_work(lib):
    lp, y, _ = R.make_case(1, 40, 8, 5, "random")
    g = G.chain(y)
    for bad in (100, 300, 16384, -256):
        rc, msg, clean = hook(lib, lp, g, window=bad)
        assert rc == -1 and "window_nodes %d must be 0" % bad in msg and "multiple of 256" in msg and clean
    # an arc that a moving window cannot follow: the last of 400 nodes also listens to node 0
    far = (list(range(1, 6)) * 80, [[j - 1] for j in range(400)], [j == 399 for j in range(400)])
    far[1][399].append(0)
    lp_long = np.ascontiguousarray(np.tile(lp, (20, 1)))
    rc, msg, clean = hook(lib, lp_long, far, window=256)
    assert rc == -5 and "node 399: an arc of span 399 nodes" in msg and "wider window" in msg and clean
    # {one token | 70 tokens}: the token after the choice is 71 nodes from the short branch, a window of 256 follows 64
    jump = G.build([("tok", 1 + k % 5) for k in range(200)] + [("choice", [[("tok", 6)], [("tok", 1 + k % 5) for k in range(70)]])] +
                   [("tok", 7)] + [("tok", 1 + k % 5) for k in range(100)])
    rc, msg, clean = hook(lib, lp_long, jump, window=256)
    assert rc == -5 and "node 271: an arc of span 71 nodes" in msg and "(64)" in msg and clean
    rc, msg, clean = hook(lib, lp_long, jump, window=512)
    assert "span" not in msg and "window_nodes" not in msg            # 372 nodes: the window holds the graph, no arc is too long
    # a start predecessor counts as span j + 1
    late = (list(range(1, 7)) * 60, [[j - 1] for j in range(360)], [j == 359 for j in range(360)])
    late[1][100].append(-1)
    rc, msg, clean = hook(lib, lp_long, late, window=256)
    assert rc == -5 and "node 100: an arc of span 101 nodes" in msg and clean
    # the shortest reading against the frames: 5 tokens, one optional, a repeat that needs its blank
    g2 = G.build([("tok", 3), ("tok", 3), ("choice", [[("tok", 4)], []]), ("tok", 5)])
    assert WR.min_frames(*g2) == 4
    rc, msg, clean = hook(lib, lp[:3], g2)
    assert rc == -1 and "infeasible" in msg and "shortest reading needs at least 4 frames, the lattice has 3" in msg and clean
    # rvb_ctc_align_graph's own, in its words
    bad_graphs = [(([], [], []), "empty graph"), (([1], [[]], [True]), "node 0: empty predecessor list"),
                  (([1, 2], [[-1], [0, 0]], [False, True]), "node 1: duplicate predecessor 0"),
                  (([1, 2], [[-1], [1]], [False, True]), "node 1: predecessor 1 is not -1 (start) or an earlier node"),
                  (([1, 2], [[-1], [-2]], [False, True]), "predecessor -2 is not -1"),
                  (([1], [[-1]], [False]), "no final node"), (([1, 8], [[-1], [0]], [False, True]), "node 1: label 8 outside [0, 8)"),
                  (([1, 0], [[-1], [0]], [False, True]), "node 1: label is the blank id 0"),
                  (([1, G.W], [[-1], [0]], [False, True]), "a graph with wildcards needs w")]
    for graph, word in bad_graphs:
        rc, msg, clean = hook(lib, lp, graph)
        assert rc == -1 and word in msg and clean, (word, msg)
    many = ([1] * 66, [[-1]] * 65 + [list(range(65))], [False] * 65 + [True])
    rc, msg, clean = hook(lib, lp_long, many)
    assert rc == -5 and "node 65: in-degree 65 exceeds the cap of 64 predecessors per node" in msg and clean
    rc, msg, clean = hook(lib, lp, g, T=(1 << 20) + 1);           assert rc == -5 and "frames exceed the cap" in msg and clean
    rc, msg, clean = hook(lib, lp, g, bias=0.5);                  assert rc == -1 and "bias" in msg and clean
    rc, msg, clean = hook(lib, lp, g, bias=float("nan"));         assert rc == -1 and "bias" in msg and clean
    rc, msg, clean = hook(lib, lp, g, slab=0);                    assert rc == -1 and "slab_rows >= 1" in msg and clean
    rc, msg, clean = hook(lib, lp, g, blank=8);                   assert rc == -1 and "blank id outside" in msg and clean
    plain = G.chain(list(range(1, 6)) * 80)                      # 400 nodes, 800 frames in slabs of 300: three launches, lo <= 192
    for force, at in (([0, 32, 64], 1), ([64, 64, 64], 0), ([0, 128, 64], 2), ([0, 192, 256], 2)):
        rc, msg, clean = hook(lib, lp_long, plain, window=256, slab=300, lo_force=force)
        assert rc == -1 and "lo_force[%d] = %d must be a multiple of 64 in [0, 192]" % (at, force[at]) in msg and clean
    # more nodes and arcs than rvb_ctc_align_graph takes are no refusal here: the plan is accepted, and only then a device is asked for
    big = G.chain(np.tile(np.arange(1, 8), 2000))
    rc, msg, clean = hook(lib, np.ascontiguousarray(np.tile(lp, (400, 1))), big)
    assert (rc == 0 and not clean) or (rc != 0 and "no HIP device" in msg)


def test_align_wav_has_a_long_graph_form():
    from reverb_amd.bin.align_wav import get_args
    base = ["--model", "m", "--audio_file", "a.wav", "--transcript_file", "t.txt", "--result_dir", "out"]
    args = get_args(base + ["--alternatives", "--long_graph", "--window_nodes", "512"])
    assert args.alternatives and args.long_graph and args.window_nodes == 512
    assert get_args(base).long_graph is False and get_args(base).window_nodes is None
    assert get_args(base + ["--alternatives", "--long_graph", "--wildcard", "<star>"]).long_graph
    for extra in (["--long_graph"], ["--alternatives", "--window_nodes", "512"], ["--alternatives", "--long_graph", "--window_nodes", "0"],
                  ["--long_form", "--alternatives"]):
        with pytest.raises(SystemExit):
            get_args(base + extra)
    for excluded in (["--graph_score"], ["--score"], ["--posteriors"], ["--attention"], ["--long_form"], ["--window_tokens", "512"]):
        with pytest.raises(SystemExit):
            get_args(base + ["--alternatives", "--long_graph"] + excluded, long_score=True)


def test_the_parser_lifts_the_graph_caps_only_when_asked():
    from reverb_amd.token_graph import MAX_NODES, TokenGraph, parse_alternatives
    tok = lambda text: [ord(c) - 96 for c in text if c != " "]
    text = " ".join(["{a|b c} d"] * 2400)
    with pytest.raises(ValueError, match="RVB_CTC_GRAPH_MAX_NODES"):
        parse_alternatives(text, tok)
    g = parse_alternatives(text, tok, long_form=True)
    assert len(g) == 9600 > MAX_NODES and g.preds[-1] == [9598, 9596]
    with pytest.raises(ValueError, match="RVB_CTC_GRAPH_MAX_IN_DEGREE"):
        TokenGraph([1] * 66, [[-1]] * 65 + [list(range(65))], [False] * 65 + [True], long_form=True)
