"""rvd_centroid_linkage_many's device side through librvb_test.so's hook rvb_test_centroid_linkage_many (no engine needed): many
clusterings behind one batched pdist launch, one batched nn_init launch and one merge-loop launch with a workgroup per problem.

The contract is bit-identity: the batched kernels run the single call's code on a table row, so every problem's dendrogram must
`==` what rvb_test_centroid_linkage gives for the same points with ONE workgroup -- ties included -- and, independently of that, pass
the replay oracle of tests/linkage_ref.py.  The sizes cover one merge (2), empty problems between others (the offsets), sizes off the
16- and 64-lane grids (3, 17, 65, 257, 300), and a thread that owns two slots (1025)."""
import numpy as np
import pytest

import linkage_ref as ref

pytestmark = pytest.mark.gpu

SWITCHES = ("RVD_LINKAGE_MB", "RVD_LINKAGE_G", "RVD_LINKAGE_XCHG", "RVD_LINKAGE_COMPACT", "RVD_LINKAGE_GLOBAL", "RVD_LINKAGE_PROF",
            "RVD_LINKAGE_MANY_CAP")
SIZES = [2, 1, 3, 17, 64, 65, 0, 257, 1025, 300]
_cache = {}


def _env(monkeypatch, **env):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, str(value))


def many(lib, Xs, d):
    """rvb_test_centroid_linkage_many on the point sets -> (rc, list of Z, route); Z starts as -7 everywhere."""
    from reverb_amd import _lib
    ns = np.array([len(X) for X in Xs], np.int32)
    allX = np.ascontiguousarray(np.concatenate([np.asarray(X, np.float64).reshape(-1, d) for X in Xs]), np.float64)
    rows = np.maximum(ns.astype(np.int64) - 1, 0)
    Z = np.full((int(rows.sum()), 4), -7.0)
    route = np.full(len(Xs), -9, np.int32)
    rc = lib.rvb_test_centroid_linkage_many(_lib.dptr(allX), _lib.iptr(ns), len(Xs), d, _lib.dptr(Z), _lib.iptr(route))
    ends = np.cumsum(rows)
    return rc, [Z[e - r:e] for r, e in zip(rows, ends)], [int(v) for v in route]


def single(lib, X, workgroups=1):
    """The single call with one workgroup (the loop the batch must reproduce) -> Z."""
    from reverb_amd import _lib
    import ctypes as C
    X = np.ascontiguousarray(X, np.float64)
    n, d = X.shape
    Z = np.full((max(n - 1, 0), 4), -7.0)
    ran = np.zeros(4, np.int32)
    _lib.check(lib.rvb_test_centroid_linkage(_lib.dptr(X), n, d, workgroups, _lib.dptr(Z), _lib.iptr(ran), C.byref(C.c_double())),
               "rvb_test_centroid_linkage")
    return Z, [int(v) for v in ran]


def batch_inputs(d):
    """The shared batch at dimension d: blobs on the unit sphere (fp32 values in fp64, as the pipeline's unit vectors are)."""
    if d not in _cache:
        _cache[d] = [ref.blobs(n, d, seed=100 * d + n) if n else np.zeros((0, d)) for n in SIZES]
    return _cache[d]


def singles(lib, monkeypatch, d):
    """One-workgroup single-call dendrograms of the shared batch, computed once under the default switches."""
    key = ("single", d)
    if key not in _cache:
        _env(monkeypatch)
        out = []
        for X in batch_inputs(d):
            if len(X) < 2:
                out.append(np.zeros((0, 4)))
                continue
            Z, ran = single(lib, X)
            assert ran == [1, 1, 0, 0], ran
            out.append(Z)
        _cache[key] = out
    return _cache[key]


def same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("d", [8, 256])
def test_batch_equals_the_one_workgroup_single_call_and_replays(lib, monkeypatch, d):
    from reverb_amd import _lib
    Xs, want = batch_inputs(d), singles(lib, monkeypatch, d)
    _env(monkeypatch)
    rc, Zs, route = many(lib, Xs, d)
    _lib.check(rc, "rvb_test_centroid_linkage_many")
    assert route == [1 if n >= 2 else -1 for n in SIZES]
    for n, X, Z, W in zip(SIZES, Xs, Zs, want):
        assert Z.shape == (max(n - 1, 0), 4)
        assert same_bits(Z, W), (d, n, np.argwhere(Z != W)[:3])
        if n >= 2:
            ref.replay(X, Z)


def test_batch_without_compaction_runs_loop_2_and_gives_the_same_dendrograms(lib, monkeypatch):
    from reverb_amd import _lib
    Xs, want = batch_inputs(8), singles(lib, monkeypatch, 8)
    _env(monkeypatch, RVD_LINKAGE_COMPACT="0")
    rc, Zs, route = many(lib, Xs, 8)
    _lib.check(rc, "rvb_test_centroid_linkage_many")
    assert route == [2 if n >= 2 else -1 for n in SIZES]
    for n, Z, W in zip(SIZES, Zs, want):
        assert same_bits(Z, W), n


@pytest.mark.parametrize("cap", [1, 40000, 600000])
def test_batch_split_over_several_launches_gives_the_same_dendrograms(lib, monkeypatch, cap):
    """A launch holds at most 2 GiB of distance matrices; the lab switch RVD_LINKAGE_MANY_CAP (bytes) puts that limit where this
    batch has to be split: every problem a launch of its own (1); five launches (40 000: the problems of 2, 3, 17 and 64 points fit
    together, 65 more points do not); three launches, the 1025-point problem -- larger than the limit -- alone in one (600 000)."""
    from reverb_amd import _lib
    Xs, want = batch_inputs(8), singles(lib, monkeypatch, 8)
    _env(monkeypatch, RVD_LINKAGE_MANY_CAP=cap)
    rc, Zs, route = many(lib, Xs, 8)
    _lib.check(rc, "rvb_test_centroid_linkage_many")
    assert route == [1 if n >= 2 else -1 for n in SIZES]
    for n, Z, W in zip(SIZES, Zs, want):
        assert same_bits(Z, W), (cap, n)


def test_problem_of_3000_points_is_routed_to_the_single_call(lib, monkeypatch):
    from reverb_amd import _lib
    _env(monkeypatch)
    Xs = [ref.blobs(40, 8, seed=1), ref.blobs(3000, 8, seed=2), ref.blobs(40, 8, seed=3)]
    rc, Zs, route = many(lib, Xs, 8)
    _lib.check(rc, "rvb_test_centroid_linkage_many")
    assert route == [1, 0, 1]
    for X, Z in zip(Xs, Zs):
        ref.replay(X, Z)
    for i in (0, 2):
        assert same_bits(Zs[i], single(lib, Xs[i])[0])


def test_tied_distances_equal_the_single_call(lib, monkeypatch):
    """Exact duplicates tie at distance 0 and beyond: the order of tied merges is the loop's own, so the batch must take them exactly as
    the one-workgroup single call does; the oracle accepts the result as a greedy centroid linkage under some tie order."""
    from reverb_amd import _lib
    _env(monkeypatch)
    dup, lat = ref.duplicated_blobs(), np.ascontiguousarray(np.pad(ref.lattice(12, 12), ((0, 0), (0, 14))))
    assert dup.shape[1] == lat.shape[1] == 16
    Xs = [ref.blobs(30, 16, seed=5), dup, lat]
    rc, Zs, route = many(lib, Xs, 16)
    _lib.check(rc, "rvb_test_centroid_linkage_many")
    assert route == [1, 1, 1]
    for X, Z in zip(Xs, Zs):
        W, ran = single(lib, X)
        assert ran == [1, 1, 0, 0]
        assert same_bits(Z, W)
        ref.replay(X, Z)


def test_nan_row_fails_the_call_and_names_the_problem(lib, monkeypatch):
    """A NaN row never finds a partner (min_pair never takes a NaN): that problem's loop ends with status -1 after its bounded candidate
    loop, the others run to the end, and the call reports the problem's index."""
    _env(monkeypatch)
    bad = ref.blobs(40, 16, seed=40).copy()
    bad[13] = np.nan
    Xs = [ref.blobs(20, 16, seed=6), ref.blobs(33, 16, seed=7), bad, ref.blobs(20, 16, seed=8)]
    rc, _, _ = many(lib, Xs, 16)
    assert rc == -1                                                  # RVB_E_ARG
    msg = lib.rvb_last_error()
    assert b"problem 2" in msg and b"no candidate pair" in msg, msg


def test_hook_refuses_bad_arguments_and_handles_nothing_to_do(lib, monkeypatch):
    from reverb_amd import _lib
    _env(monkeypatch)
    X = np.zeros((4, 2))
    Z = np.full((3, 4), -7.0)
    route = np.full(2, -9, np.int32)
    ns = np.array([4, 0], np.int32)
    assert lib.rvb_test_centroid_linkage_many(_lib.dptr(X), _lib.iptr(ns), 0, 2, _lib.dptr(Z), _lib.iptr(route)) == -1
    assert lib.rvb_test_centroid_linkage_many(_lib.dptr(X), _lib.iptr(ns), 2, 0, _lib.dptr(Z), _lib.iptr(route)) == -1
    assert lib.rvb_test_centroid_linkage_many(_lib.dptr(X), _lib.iptr(np.array([4, -1], np.int32)), 2, 2, _lib.dptr(Z), _lib.iptr(route)) == -1
    assert np.all(Z == -7.0)
    ns = np.array([1, 0], np.int32)                                  # nothing to cluster: success, no launch, no rows
    assert lib.rvb_test_centroid_linkage_many(_lib.dptr(X), _lib.iptr(ns), 2, 2, _lib.dptr(Z), _lib.iptr(route)) == 0
    assert list(route) == [-1, -1] and np.all(Z == -7.0)
