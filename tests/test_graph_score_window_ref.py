"""The windowed full sum over token graphs without a GPU: the fp64 band restatement (tests/graph_score_window_ref.py) against the
unwindowed one (tests/graph_score_ref.py) and against a brute-force enumeration of the counted state paths, the posteriors of a frame
summed over its alive states, the near-tie condition of the GPU file's cases on the restatement alone, the refusals of the lab hook
rvb_test_ctc_score_graph_window, which all come before any device work, and align_wav's --long_graph_score."""
import numpy as np
import pytest

import ctc_score_ref as C
import force_align_ref as F
import graph_align_ref as G
import graph_align_window_ref as GW
import graph_score_ref as R
import graph_score_window_ref as WS
from reverb_amd import _lib


def pack(graph):
    tok = np.ascontiguousarray(graph[0], np.int32)
    off = np.concatenate([[0], np.cumsum([len(p) for p in graph[1]])]).astype(np.int32)
    prd = np.array([p for ps in graph[1] for p in ps], np.int32)
    fin = np.ascontiguousarray(graph[2], np.uint8)
    return tok, np.ascontiguousarray(off), np.ascontiguousarray(prd), fin


POST_CAP = 1e-3            # the largest the posterior tolerance of tests/test_ctc_graph_score_window_gpu.py may be: a larger tolerance
                           # calls more peak frames near ties, so the cap of 5 % that holds here holds at the tolerance in use


def test_a_band_that_never_moves_is_the_unwindowed_score():
    n = 0
    for seed in range(4):
        rng = np.random.default_rng(seed)
        _, y = C.make_lattice(seed, 1, 24, 40, 1.0, (2, 8, 16))
        y = [int(t) for t in y]
        g = G.build(G.around(rng, y, 24) if seed % 2 else G.groups(rng, y, 24, n_alt=3))
        lp = C.make_lattice(seed, len(g[0]) + 9, 24, 1)[0]
        want = R.score(lp, *g)
        got = WS.score(lp, *g, WS.effective_window(len(g[0]), 0), np.zeros(len(lp), np.int32), keep=True)
        assert got[0] == want[0]
        for key in want[1]:
            assert np.array_equal(got[1][key], want[1][key]), key
        assert np.abs(got[1]["post_sum"] - 1.0).max() <= 1e-12
        n += 1
    assert n == 4


SMALL = [
    # (tokens, preds, finals), W, lo_of
    (([1, 2, 3, 4], [[-1], [0], [1], [2]], [False, False, False, True]), 2, [0, 0, 1, 1, 2, 2]),
    (([1, 2, 2, 3, 4], [[-1], [0], [0, 1], [1, 2], [3]], [False, False, False, False, True]), 3, [0, 0, 1, 1, 2, 2, 2]),
    (([1, 2, 1, 3, 2, 3], [[-1], [-1, 0], [0, 1], [1, 2], [2, 3], [3, 4]], [False, False, False, False, True, True]), 3, [0, 0, 1, 2, 3, 3, 3]),
    (([1, 1, 2, 2, 3], [[-1], [0], [0, 1], [2], [2, 3]], [False, False, False, True, True]), 3, [0, 0, 0, 1, 2, 2]),
    (([2, 3, 2, 4, 4, 1], [[-1], [-1], [0, 1], [2], [2, 3], [3, 4]], [False, False, False, False, False, True]), 4, [0, 0, 2, 2, 2, 2, 2]),
    (([1, 2, 3], [[-1], [0], [0, 1]], [False, False, True]), 2, [0, 0, 1, 1]),
]


@pytest.mark.parametrize("k", range(len(SMALL)))
def test_forced_moves_on_small_graphs_equal_the_enumeration_of_counted_paths(k):
    graph, W, lo_of = SMALL[k]
    T = len(lo_of)
    assert len(graph[0]) <= 6 and T <= 7 and lo_of[-1] > 0
    rng = np.random.default_rng(k)
    logits = rng.standard_normal((T, 6))
    lp = logits - np.log(np.exp(logits).sum(1, keepdims=True))
    want_ll, want_visit = WS.brute_force(lp, *graph, W, lo_of)
    ll, res = WS.score(lp, *graph, W, lo_of, keep=True)
    assert abs(ll - want_ll) <= 1e-12
    assert np.abs(res["visit"] - want_visit).max() <= 1e-12
    assert np.abs(res["post_sum"] - 1.0).max() <= 1e-12              # also at the frames of a move
    full = R.loglik(lp, *graph)
    assert ll <= full + 1e-12


def test_a_band_that_loses_every_path_is_infeasible():
    graph, W, _ = SMALL[0]
    lp = np.log(np.full((6, 6), 1 / 6))
    with pytest.raises(ValueError, match="infeasible"):
        WS.score(lp, *graph, W, [0, 2, 2, 2, 2, 2])                   # node 1 is never alive with node 0 behind it
    with pytest.raises(ValueError, match="infeasible"):
        WS.brute_force(lp, *graph, W, [0, 2, 2, 2, 2, 2])


def near_ties(res):
    sure = res["visit"] >= 0.5
    clear = res["peak_post"] - res["second"] > POST_CAP
    return int((sure & ~clear).sum()), int(sure.sum())


def test_posteriors_sum_to_one_and_peak_frames_are_clear_on_the_cases_of_the_gpu_file():
    for tag, W, L, seed in WS.MOVING:
        lp, g = WS.moving_case(L, seed)
        assert len(g[0]) > W and max(j - p for j, ps in enumerate(g[1]) for p in ps if p >= 0) <= W // 2 - 64
        lo_of, best = WS.drive(lp, *g, W, WS.MOVING_SLAB)
        assert lo_of[-1] > 0 and len(best) > -(-len(lp) // WS.MOVING_SLAB) - 1
        ll, res = WS.score(lp, *g, W, lo_of, keep=tag == "npt1")
        skipped, sure = near_ties(res)
        assert skipped <= 0.05 * sure, (tag, skipped, sure)
        if tag == "npt1":
            assert np.abs(res["post_sum"] - 1.0).max() <= 1e-10
            assert ll <= R.loglik(lp, *g) + 1e-9
    lp, g, _, lo_of = GW.cut_case()
    ll, res = WS.score(lp, *g, GW.CUT_W, lo_of, keep=True)
    skipped, sure = near_ties(res)
    assert skipped <= 0.05 * sure, ("cut", skipped, sure)
    assert np.abs(res["post_sum"] - 1.0).max() <= 1e-10               # the frame of the jump included
    assert R.loglik(lp, *g) - ll > 1.0                               # the reading through the short branch carried mass


def test_the_live_set_is_the_plain_kernels():
    """frames to the end: T_j's is the policy's need[], B_j's one more than the nearest successor's"""
    rng = np.random.default_rng(5)
    _, y = C.make_lattice(5, 1, 24, 60, 1.0, (2, 8, 16))
    g = G.build(G.around(rng, [int(t) for t in y], 24))
    remT, remB, rem_start = WS.frames_to_end(*g)
    need = GW.tables(*g)[2]
    assert np.array_equal(remT, need)
    assert rem_start == GW.min_frames(*g)
    for j in range(len(g[0])):
        succ = [k for k in range(j + 1, len(g[0])) if j in g[1][k]]
        want = 0 if g[2][j] else min([need[k] + 1 for k in succ if need[k] < GW.FAR] or [GW.FAR])
        assert remB[j] == want


def hook(lib, lp, graph, window=0, slab=64, T=None, blank=0, lo_force=None, post=True):
    lp = np.ascontiguousarray(lp, np.float32)
    tok, off, prd, fin = pack(graph)
    T = lp.shape[0] if T is None else T
    n, N = max(min(T, 1 << 16), 1), max(len(graph[0]), 1)
    ll = np.full(1, 123.0, np.float64)
    vis, occ, mean, peak = (np.full(N, -7.0, np.float32) for _ in range(4))
    pf, lo, best, launches = np.full(N, -7, np.int32), np.full(n, -7, np.int32), np.full(n, -7, np.int32), np.full(1, -7, np.int32)
    force = None if lo_force is None else np.ascontiguousarray(lo_force, np.int32)
    outs = [_lib.fptr(a) if post else None for a in (vis, occ, mean, peak)] + [_lib.iptr(pf) if post else None]
    rc = lib.rvb_test_ctc_score_graph_window(_lib.fptr(lp), T, lp.shape[1], _lib.iptr(tok), len(graph[0]), _lib.iptr(off), _lib.iptr(prd),
                                             _lib.u8ptr(fin), blank, slab, window, _lib.iptr(force), _lib.dptr(ll), *outs, _lib.iptr(lo),
                                             _lib.iptr(best), _lib.iptr(launches))
    untouched = all(np.all(a == -7) for a in (vis, occ, mean, peak, pf, lo, best, launches)) and ll[0] == 123.0
    return rc, lib.rvb_last_error().decode(), untouched


def test_the_hook_refuses_before_any_device_work(lib):
    lp, y, _ = F.make_case(1, 40, 8, 5, "random")
    g = G.chain(y)
    for bad in (100, 300, 8192, 4352, -256):                          # 8192 is the ALIGNER's cap: fp64 states halve it
        rc, msg, clean = hook(lib, lp, g, window=bad)
        assert rc == -1 and "rvb_test_ctc_score_graph_window: window_nodes %d must be 0 (the default, 4096)" % bad in msg and clean
        assert "multiple of 256 in [256, 4096]" in msg
    rc, msg, clean = hook(lib, lp, ([1, G.W], [[-1], [0]], [False, True]))
    assert rc == -1 and "node 1: a wildcard has no full-sum score" in msg and clean
    lp_long = np.ascontiguousarray(np.tile(lp, (20, 1)))
    far = (list(range(1, 6)) * 80, [[j - 1] for j in range(400)], [j == 399 for j in range(400)])
    far[1][399].append(0)
    rc, msg, clean = hook(lib, lp_long, far, window=256)
    assert rc == -5 and "node 399: an arc of span 399 nodes" in msg and "wider window" in msg and clean
    many = ([1] * 66, [[-1]] * 65 + [list(range(65))], [False] * 65 + [True])
    rc, msg, clean = hook(lib, lp_long, many)
    assert rc == -5 and "node 65: in-degree 65 exceeds the cap of 64 predecessors per node" in msg and clean
    # 65 nodes that all listen to node 0: its out-degree is refused with posteriors only
    fan = ([1] + [2 + k % 5 for k in range(65)], [[-1]] + [[0]] * 65, [False] + [True] * 65)
    rc, msg, clean = hook(lib, lp_long, fan)
    assert rc == -5 and "node 0: out-degree 65 exceeds the cap of 64 successors per node" in msg and clean
    rc, msg, clean = hook(lib, lp_long, fan, post=False)
    assert (rc == 0 and not clean) or ("no HIP device" in msg and "out-degree" not in msg)      # the message of a success is stale
    g2 = G.build([("tok", 3), ("tok", 3), ("choice", [[("tok", 4)], []]), ("tok", 5)])
    rc, msg, clean = hook(lib, lp[:3], g2)
    assert rc == -1 and "infeasible" in msg and "shortest reading needs at least 4 frames, the lattice has 3" in msg and clean
    for graph, word in [(([], [], []), "empty graph"), (([1, 2], [[-1], [0, 0]], [False, True]), "node 1: duplicate predecessor 0"),
                        (([1], [[-1]], [False]), "no final node"), (([1, 0], [[-1], [0]], [False, True]), "node 1: label is the blank id 0")]:
        rc, msg, clean = hook(lib, lp, graph)
        assert rc == -1 and word in msg and clean, (word, msg)
    rc, msg, clean = hook(lib, lp, g, T=(1 << 20) + 1);           assert rc == -5 and "frames exceed the cap" in msg and clean
    rc, msg, clean = hook(lib, lp, g, slab=0);                    assert rc == -1 and "slab_rows >= 1" in msg and clean
    plain = G.chain(list(range(1, 6)) * 80)                      # 400 nodes, 800 frames in slabs of 300: three launches, lo <= 192
    for force, at in (([0, 32, 64], 1), ([64, 64, 64], 0), ([0, 128, 64], 2), ([0, 192, 256], 2)):
        rc, msg, clean = hook(lib, lp_long, plain, window=256, slab=300, lo_force=force)
        assert rc == -1 and "lo_force[%d] = %d must be a multiple of 64 in [0, 192]" % (at, force[at]) in msg and clean


def test_align_wav_has_a_long_graph_score_form():
    from reverb_amd.bin.align_wav import get_args
    base = ["--model", "m", "--audio_file", "a.wav", "--transcript_file", "t.txt", "--result_dir", "out"]
    args = get_args(base + ["--alternatives", "--long_graph_score", "--window_nodes", "512"], long_score=True)
    assert args.alternatives and args.long_graph_score and args.window_nodes == 512 and not args.long_graph and not args.graph_score
    assert get_args(base).long_graph_score is False
    assert get_args(base + ["--alternatives", "--long_graph", "--long_graph_score"]).long_graph_score
    for bad in (["--long_graph_score"], ["--alternatives", "--long_graph_score", "--wildcard", "<star>"],
                ["--alternatives", "--long_graph_score", "--attention"], ["--alternatives", "--long_graph_score", "--score"],
                ["--alternatives", "--long_graph_score", "--graph_score"], ["--alternatives", "--long_graph_score", "--posteriors"],
                ["--alternatives", "--long_graph_score", "--long_form"], ["--alternatives", "--long_graph_score", "--window_nodes", "0"],
                ["--alternatives", "--long_graph", "--graph_score"]):          # the last one: as before
        with pytest.raises(SystemExit):
            get_args(base + bad, long_score=True)
