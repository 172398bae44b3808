"""linkage.hip kernel by kernel, in every form the pipelines run, through librvb_test.so's hooks (no engine needed):

  * pdist_kernel / nn_init_kernel against an np.longdouble reference: every element written, exact symmetry, the tile skip, the d % 16
    and n % 64 tails, duplicates at exactly 0, the first-index tie rule;
  * the three one-workgroup merge loops and the multi-workgroup loop at every workgroup count rvd_set_linkage_workgroups accepts
    (the product asks for 4) and in all three exchange forms, with `ran` telling which loop really produced the result;
  * tie-free input is pinned to scipy (same merges in the same order, distances within 1e-9) and every loop is bit-identical to
    the others; input with ties (exact duplicates, lattices) goes through the replay oracle of tests/linkage_ref.py, because the order
    of tied merges is nobody's contract -- but the multi-workgroup loop must not depend on G or on the exchange form;
  * the default dispatch around n = 3000, high-dimensional noise (the rescan paths), repeated calls with another G in between, and
    the "no candidate pair" return."""
import ctypes as C

import numpy as np
import pytest
from scipy.cluster.hierarchy import fcluster, linkage

import linkage_ref as ref

pytestmark = pytest.mark.gpu

SWITCHES = ("RVD_LINKAGE_MB", "RVD_LINKAGE_G", "RVD_LINKAGE_XCHG", "RVD_LINKAGE_COMPACT", "RVD_LINKAGE_GLOBAL", "RVD_LINKAGE_PROF")
FORMS = {"A": 0, "B": 1, "C": 2}
ONE_WG = {"compact": (dict(RVD_LINKAGE_MB="0"), 1), "no_compact": (dict(RVD_LINKAGE_MB="0", RVD_LINKAGE_COMPACT="0"), 2),
          "global": (dict(RVD_LINKAGE_MB="0", RVD_LINKAGE_GLOBAL="1"), 3)}
_cache = {}


def link(lib, monkeypatch, X, workgroups=0, **env):
    """rvb_test_centroid_linkage under exactly the given lab switches -> (rc, Z, ran, retries); Z starts as -7 everywhere."""
    from reverb_amd import _lib
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, str(value))
    X = np.ascontiguousarray(X, np.float64)
    n, d = X.shape
    Z = np.full((max(n - 1, 0), 4), -7.0)
    ran = np.full(4, -1, np.int32)
    retries = C.c_double(-1.0)
    rc = lib.rvb_test_centroid_linkage(_lib.dptr(X), n, d, workgroups, _lib.dptr(Z), _lib.iptr(ran), C.byref(retries))
    return rc, Z, [int(v) for v in ran], retries.value


def ok(res):
    from reverb_amd import _lib
    _lib.check(res[0], "rvb_test_centroid_linkage")
    return res[1:]


def mb(lib, monkeypatch, X, G, form="B", **env):
    """The multi-workgroup loop by name (never a silent fall-back) at G workgroups and that exchange form; checks `ran`."""
    Z, ran, retries = ok(link(lib, monkeypatch, X, G, RVD_LINKAGE_MB="1", RVD_LINKAGE_XCHG=FORMS[form], **env))
    assert ran == [4, G, FORMS[form], 0], (len(X), G, form, ran)
    return Z, retries


def tie_free(n):
    """(X, scipy's dendrogram) of the blob input of n points; d varies with n over 4, 16, 48."""
    key = ("blobs", n)
    if key not in _cache:
        X = ref.blobs(n, (4, 16, 48)[n % 3], seed=n)
        _cache[key] = (X, linkage(X, method="centroid", metric="euclidean"))
    return _cache[key]


def one_wg(lib, monkeypatch, key, X):
    """The one-workgroup loop's dendrogram of a shared input, computed once."""
    key = ("one", key)
    if key not in _cache:
        Z, ran, _ = ok(link(lib, monkeypatch, X, 0, RVD_LINKAGE_MB="0"))
        assert ran == [1, 1, 0, 0], ran
        _cache[key] = Z
    return _cache[key]


def pinned(got, want):
    """The project's pins on tie-free input: same merges in the same order, distances within 1e-9, the same flat clustering."""
    assert got.shape == want.shape
    assert np.array_equal(got[:, [0, 1, 3]], want[:, [0, 1, 3]])
    if len(want):
        assert np.abs(got[:, 2] - want[:, 2]).max() < ref.TOL
        assert np.array_equal(fcluster(got, ref.THRESHOLD, "distance"), fcluster(want, ref.THRESHOLD, "distance"))


def same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------ pdist, nn_init
def _pdist_input(n, d, dup):
    rng = np.random.default_rng(1000 * n + d)
    X = rng.standard_normal((n, d))
    if dup:                                     # exact duplicates, some of them several times, in both triangles of every tile
        src = rng.integers(n, size=n // 2)
        X[rng.permutation(n)[:n // 2]] = X[src]
    return np.ascontiguousarray(X)


@pytest.mark.parametrize("n,d,dup", [(2, 1, False), (3, 4, False), (63, 5, False), (64, 16, False), (65, 17, False), (129, 33, False),
                                     (200, 256, False), (150, 7, True)])
def test_pdist_and_nn_init_against_longdouble(lib, n, d, dup):
    from reverb_amd import _lib
    X = _pdist_input(n, d, dup)
    D = np.zeros((n, n))
    nb = np.zeros(n, np.int32)
    md = np.zeros(n)
    _lib.check(lib.rvb_test_pdist_nn(_lib.dptr(X), n, d, _lib.dptr(D), _lib.iptr(nb), _lib.dptr(md)), "rvb_test_pdist_nn")
    assert not np.isnan(D).any()                                    # every element written (the device buffer started as NaN)
    assert D.tobytes() == np.ascontiguousarray(D.T).tobytes()       # symmetric bit for bit
    assert np.all(np.diag(D) == 0.0) and not np.signbit(np.diag(D)).any()
    XL = X.astype(np.longdouble)
    want = np.zeros((n, n), np.longdouble)
    for i in range(n):
        want[i] = np.sqrt(((XL - XL[i]) ** 2).sum(axis=1))
    # a d-term sum of non-negative products and one square root, rounded on both sides
    excess = np.abs(D - want) - (d + 4) * 2.0 ** -53 * want
    over = float((np.abs(D - want)[want > 0] / ((d + 4) * 2.0 ** -53 * want[want > 0])).max())
    print(f"pdist n={n} d={d}: worst error / bound = {over:.3f}")
    assert np.all(excess <= 0), (n, d, over)
    same = (X[:, None, :] == X[None, :, :]).all(axis=2)
    assert np.all(D[same] == 0.0)
    if dup:
        assert same.sum() > n + n // 2                              # the input really holds duplicates
    # nn_init on the D it was given: first index of the minimum of the row above the diagonal, and that element -- exact
    for x in range(n - 1):
        row = D[x, x + 1:]
        j = int(np.argmin(row))                                     # numpy: first occurrence
        assert nb[x] == x + 1 + j and md[x] == row[j], (x, nb[x], md[x])
    if dup:
        assert sum(1 for x in range(n - 1) if (D[x, x + 1:] == D[x, x + 1:].min()).sum() > 1) > 0        # a tie was decided
    assert nb[n - 1] == -1 and np.isnan(md[n - 1])                  # slot n - 1: not written (grid n - 1)


def test_pdist_hook_refuses_bad_sizes(lib):
    from reverb_amd import _lib
    X, D, nb, md = np.zeros((2, 2)), np.full((2, 2), 5.0), np.zeros(2, np.int32), np.zeros(2)
    for n, d in ((1, 2), (2, 0), (0, 2)):
        assert lib.rvb_test_pdist_nn(_lib.dptr(X), n, d, _lib.dptr(D), _lib.iptr(nb), _lib.dptr(md)) == -1
    assert np.all(D == 5.0)


# ------------------------------------------------------------------------------------ one-workgroup loops
@pytest.mark.parametrize("n", [2, 3, 64, 255, 256, 257, 512, 513, 1024, 1025, 2049])
def test_one_workgroup_loops_match_scipy_and_each_other(lib, monkeypatch, n):
    """linkage_kernel's three instantiations around the re-deal (k & 255 == 0: n = 256 / 257 / 513) and the batch-count steps
    (ecount: n = 1024 / 1025, 2048 / 2049)."""
    X, want = tie_free(n)
    got = {}
    for name, (env, loop) in ONE_WG.items():
        Z, ran, _ = ok(link(lib, monkeypatch, X, 0, **env))
        assert ran == [loop, 1, 0, 0], (name, ran)
        pinned(Z, want)
        got[name] = Z
    assert same_bits(got["compact"], got["no_compact"]) and same_bits(got["compact"], got["global"])
    _cache.setdefault(("one", ("blobs", n)), got["compact"])


def test_workgroups_1_is_the_one_workgroup_loop_even_when_the_other_is_forced(lib, monkeypatch):
    X, want = tie_free(257)
    Z, ran, _ = ok(link(lib, monkeypatch, X, 1, RVD_LINKAGE_MB="1"))
    assert ran == [1, 1, 0, 0]
    pinned(Z, want)


# ------------------------------------------------------------------------------------ multi-workgroup loop
@pytest.mark.parametrize("form", ["A", "B", "C"])
@pytest.mark.parametrize("G", [2, 4, 8, 16])
def test_multi_workgroup_loop_every_count_and_exchange_form(lib, monkeypatch, G, form):
    """n = 17: one slot beyond the first 16-slot group; 16 G + 1: every workgroup owns one group and workgroup 0 a second one."""
    for n in (17, 16 * G + 1, 600):
        X, want = tie_free(n)
        Z, _ = mb(lib, monkeypatch, X, G, form)
        pinned(Z, want)
        assert same_bits(Z, one_wg(lib, monkeypatch, ("blobs", n), X)), (n, G, form)


@pytest.mark.parametrize("G", [2, 4, 8, 16])
def test_multi_workgroup_loop_sizes(lib, monkeypatch, G):
    """Form B (the default) at sizes where workgroups own nothing (n = 2, 3), exactly one full group each (16 G), and across the
    rebuilds of the live list (257, 513, 1500)."""
    for n in (2, 3, 16 * G, 257, 513, 1500):
        X, want = tie_free(n)
        Z, _ = mb(lib, monkeypatch, X, G, "B")
        pinned(Z, want)
        assert same_bits(Z, one_wg(lib, monkeypatch, ("blobs", n), X)), (n, G)


def test_linkage_g_switch_overrides_the_argument(lib, monkeypatch):
    X, want = tie_free(257)
    Z, ran, _ = ok(link(lib, monkeypatch, X, 16, RVD_LINKAGE_MB="1", RVD_LINKAGE_G="2"))
    assert ran == [4, 2, 1, 0]                  # and form B is the default
    pinned(Z, want)
    assert same_bits(Z, one_wg(lib, monkeypatch, ("blobs", 257), X))


def test_hook_checks_its_arguments(lib, monkeypatch):
    from reverb_amd import _lib
    X = ref.blobs(8, 4, 0)
    for wg in (-1, 3, 5, 32):
        rc, Z, _, _ = link(lib, monkeypatch, X, wg)
        assert rc == -1 and np.all(Z == -7.0)
        assert b"0 (default), 1, 2, 4, 8 or 16" in lib.rvb_last_error()
    Z, ran = np.full((1, 4), -7.0), np.zeros(4, np.int32)
    assert lib.rvb_test_centroid_linkage(_lib.dptr(X), 0, 4, 0, _lib.dptr(Z), _lib.iptr(ran), None) == -1
    assert lib.rvb_test_centroid_linkage(_lib.dptr(X), 8, 0, 0, _lib.dptr(Z), _lib.iptr(ran), None) == -1
    assert lib.rvb_test_centroid_linkage(_lib.dptr(X), 46001, 4, 0, _lib.dptr(Z), _lib.iptr(ran), None) != 0
    assert b"more than 46000 points" in lib.rvb_last_error()
    assert lib.rvb_test_centroid_linkage(_lib.dptr(X), 1, 4, 0, _lib.dptr(Z), _lib.iptr(ran), None) == 0       # one point: nothing to do
    assert np.all(Z == -7.0) and list(ran) == [0, 0, 0, 0]


# ------------------------------------------------------------------------------------ default dispatch
@pytest.mark.parametrize("n,workgroups,loop,G", [(2999, 0, 1, 1), (3000, 0, 4, 16), (3000, 4, 4, 4), (3000, 1, 1, 1)])
def test_default_dispatch(lib, monkeypatch, n, workgroups, loop, G):
    """No switch set: the one-workgroup loop below 3000 points and for workgroups = 1, else the multi-workgroup loop at the count asked
    for, exchange form B.  A fall-back to the one-workgroup loop is legal (reported, not asserted): the result must be right anyway."""
    key = ("dispatch", n)
    if key not in _cache:
        X = ref.blobs(n, 32, seed=n)
        _cache[key] = (X, linkage(X, method="centroid", metric="euclidean"))
    X, want = _cache[key]
    Z, ran, _ = ok(link(lib, monkeypatch, X, workgroups))
    print(f"dispatch n={n} workgroups={workgroups}: ran = {ran}")
    if ran[3]:
        assert loop == 4 and ran[:3] == [1, 1, 0], ran
    else:
        assert ran == [loop, G, 1 if loop == 4 else 0, 0], ran
    pinned(Z, want)


# ------------------------------------------------------------------------------------ hub points: stale candidates, rescans
def test_high_dimensional_noise_runs_the_rescan_paths(lib, monkeypatch):
    key = ("noise", 1500)
    X = ref.noise(1500, 256, seed=9)
    want = linkage(X, method="centroid", metric="euclidean")
    Z1, ran, retries = ok(link(lib, monkeypatch, X, 0, RVD_LINKAGE_MB="0"))
    assert ran == [1, 1, 0, 0]
    print(f"noise n=1500 d=256: one workgroup re-evaluated {retries:.0f} stale candidates")
    assert retries > 0
    pinned(Z1, want)
    for G in (4, 16):
        Z, retries = mb(lib, monkeypatch, X, G, "B")
        print(f"noise n=1500 d=256: workgroup 0 of {G} rescanned {retries:.0f} rows")
        assert retries > 0
        pinned(Z, want)
        assert same_bits(Z, Z1), (key, G)


# ------------------------------------------------------------------------------------ ties
@pytest.mark.parametrize("name", ["duplicates", "identical", "lattice12x12", "lattice6x6x6"])
def test_tied_input_gives_a_valid_dendrogram_whatever_the_workgroups(lib, monkeypatch, name):
    """Equal distances: the merge order is not pinned (scipy orders equal heap keys by its layout, the kernels by (distance, slot), and
    the one-workgroup loop may keep an old neighbour where the multi-workgroup loop rescans), so the replay oracle decides validity.
    With exact duplicates the partition at the threshold and the sorted merge distances are still scipy's.  The multi-workgroup loop
    derives every decision from published global quantities: its result may not depend on G or on the exchange form."""
    X = ref.tie_inputs()[name]
    want = linkage(X, method="centroid", metric="euclidean")
    Z1, ran, _ = ok(link(lib, monkeypatch, X, 0, RVD_LINKAGE_MB="0"))
    assert ran == [1, 1, 0, 0]
    first = None
    for G in (2, 4, 16):
        for form in "ABC":
            Z, _ = mb(lib, monkeypatch, X, G, form)
            if first is None:
                first = Z
            assert same_bits(Z, first), (name, G, form, np.flatnonzero((Z != first).any(axis=1))[:5])
    for which, Z in (("one workgroup", Z1), ("multi-workgroup", first)):
        worst_d, worst_m = ref.replay(X, Z)
        print(f"ties {name} ({which}): distance residual {worst_d:.2e}, minimum residual {worst_m:.2e}; "
              f"same bits as the other loop: {same_bits(Z1, first)}; same merges as scipy: {np.array_equal(Z[:, :2], want[:, :2])}")
        if name in ("duplicates", "identical"):
            assert np.array_equal(ref.partition(fcluster(Z, ref.THRESHOLD, "distance")), ref.partition(fcluster(want, ref.THRESHOLD, "distance")))
            assert np.abs(np.sort(Z[:, 2]) - np.sort(want[:, 2])).max() < ref.TOL


def test_ties_among_several_slots_of_one_thread(lib, monkeypatch):
    """More than 1024 points with ties: a thread of the one-workgroup loop owns several slots, and which ones depends on the loop
    (slot mod 1024, or dealt from the live list every 256 merges).  A thread's register minimum then meets equal distances at a lower
    slot of its own, and only the (distance, slot) order of min_pair keeps the decision independent of who owns what: the three
    one-workgroup loops must agree bit for bit, and so must the multi-workgroup loop at every count and form."""
    X = ref.lattice(36, 36)
    got = {}
    for name, (env, loop) in ONE_WG.items():
        Z, ran, _ = ok(link(lib, monkeypatch, X, 0, **env))
        assert ran == [loop, 1, 0, 0], (name, ran)
        got[name] = Z
    assert same_bits(got["compact"], got["no_compact"]), np.flatnonzero((got["compact"] != got["no_compact"]).any(axis=1))[:5]
    assert same_bits(got["compact"], got["global"]), np.flatnonzero((got["compact"] != got["global"]).any(axis=1))[:5]
    first = None
    for G, form in ((2, "B"), (4, "A"), (4, "B"), (4, "C"), (16, "B")):
        Z, _ = mb(lib, monkeypatch, X, G, form)
        if first is None:
            first = Z
        assert same_bits(Z, first), (G, form)
    same = same_bits(first, got["compact"])
    for which, Z in (("one workgroup", got["compact"]),) + (() if same else (("multi-workgroup", first),)):
        worst_d, worst_m = ref.replay(X, Z)
        print(f"ties lattice36x36 ({which}): distance residual {worst_d:.2e}, minimum residual {worst_m:.2e}; same bits as the other loop: {same}")


# ------------------------------------------------------------------------------------ repeated calls
def test_repeated_calls_with_another_workgroup_count_in_between(lib, monkeypatch):
    """The control block is cleared per call and the kernel attributes are set once per process: 300 points at G = 4, 50 at the default
    (16), 300 at G = 4 again."""
    Xa, wa = tie_free(300)
    Xb, wb = tie_free(50)
    env = dict(RVD_LINKAGE_MB="1")
    Z0, r0, _ = ok(link(lib, monkeypatch, Xa, 4, **env))
    Z1, r1, _ = ok(link(lib, monkeypatch, Xb, 0, **env))
    Z2, r2, _ = ok(link(lib, monkeypatch, Xa, 4, **env))
    assert (r0, r1, r2) == ([4, 4, 1, 0], [4, 16, 1, 0], [4, 4, 1, 0])
    assert same_bits(Z0, Z2)
    pinned(Z0, wa)
    pinned(Z1, wb)


def test_one_engine_clusters_repeatedly_with_another_workgroup_count_in_between(lab, monkeypatch):
    """The same sequence on ONE DiarEngine, as the pipelined service runs it (set_linkage_workgroups between the calls)."""
    from reverb_amd import synth_diar as SD
    from reverb_amd.diar_engine import DiarEngine
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("RVD_LINKAGE_MB", "1")
    Xa, wa = tie_free(300)
    Xb, wb = tie_free(50)
    cfg = SD.make_diar_config()
    eng = DiarEngine(cfg, SD.make_segmentation_sd(cfg, 0), dtype="bf16")
    try:
        eng.set_linkage_workgroups(4)
        Z0 = eng.centroid_linkage(Xa)
        eng.set_linkage_workgroups(0)
        Z1 = eng.centroid_linkage(Xb)
        eng.set_linkage_workgroups(4)
        Z2 = eng.centroid_linkage(Xa)
    finally:
        eng.close()
    assert same_bits(Z0, Z2)
    pinned(Z0, wa)
    pinned(Z1, wb)


# ------------------------------------------------------------------------------------ non-finite input
@pytest.mark.parametrize("loop", ["one", "multi"])
def test_non_finite_row_is_refused_as_no_candidate_pair(lib, monkeypatch, loop):
    """A NaN row has no finite distance: min_pair never takes a NaN, so the other 39 points merge as usual and the last round finds
    no candidate at all.  Both loops are bounded there: the one-workgroup loop's candidate loop runs at most n - k + 1 times, and every
    rescanning round of the multi-workgroup loop validates at least its smallest stale row; both return status -1.  (The
    one-workgroup loop used to test the winning INDEX for "none": a dropped row's +inf ties with the empty minimum and wins on its
    index, so the loop went on to merge dead slot 0 at distance inf and reported success.)"""
    X = ref.blobs(40, 16, seed=40).copy()
    X[13] = np.nan
    if loop == "one":
        rc, Z, ran, _ = link(lib, monkeypatch, X, 0, RVD_LINKAGE_MB="0")
        assert ran == [1, 1, 0, 0]
    else:
        rc, Z, ran, _ = link(lib, monkeypatch, X, 4, RVD_LINKAGE_MB="1")
        assert ran == [4, 4, 1, 0]
    assert rc == -1                                                  # RVB_E_ARG
    assert b"no candidate pair" in lib.rvb_last_error()
    assert np.all(Z == -7.0)                                         # as the caller filled it
