"""The replay oracle of tests/linkage_ref.py on its own (no GPU): it accepts scipy's dendrograms on every input family the GPU tests
use, it rejects each kind of wrong dendrogram, and what the GPU tests compare with scipy under ties -- the partition at the pipeline's
threshold and the sorted merge distances -- does not depend on scipy's own tie order."""
import numpy as np
import pytest
from scipy.cluster.hierarchy import fcluster, linkage

import linkage_ref as ref

FAMILIES = dict(ref.tie_inputs(), blobs=ref.blobs(300, 16, 2), noise=ref.noise(200, 64, 7), two=ref.blobs(2, 8, 0), three=ref.blobs(3, 4, 1))


def _scipy(X):
    return linkage(X, method="centroid", metric="euclidean")


@pytest.fixture(scope="module")
def base():
    X = ref.blobs(300, 16, 2)
    return X, _scipy(X)


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_replay_accepts_scipy(name):
    X = FAMILIES[name]
    Z = _scipy(X)
    assert np.all(np.isfinite(Z))
    worst_d, worst_m = ref.replay(X, Z)
    print(f"{name}: n = {len(X)}, distance residual {worst_d:.2e}, minimum residual {worst_m:.2e}")
    assert worst_d <= 1e-13 and worst_m <= 1e-13          # far inside TOL: the oracle's own centroids are not what limits the check


def test_replay_accepts_one_point_and_refuses_a_wrong_shape():
    assert ref.replay(np.zeros((1, 3)), np.zeros((0, 4))) == (0.0, 0.0)
    with pytest.raises(ref.ReplayError) as e:
        ref.replay(np.zeros((3, 3)), np.zeros((1, 4)))
    assert e.value.check == "shape"


def _rejected(X, Z, check):
    with pytest.raises(ref.ReplayError) as e:
        ref.replay(X, Z)
    assert e.value.check == check, str(e.value)
    return e.value.k


def test_replay_rejects_a_distance_moved_by_1e_6(base):
    X, Z = base
    for k, sign in ((0, 1.0), (150, -1.0), (len(Z) - 1, 1.0)):
        W = Z.copy()
        W[k, 2] += sign * 1e-6
        assert _rejected(X, W, "distance") == k


def test_replay_rejects_a_size_off_by_one(base):
    X, Z = base
    for k, off in ((5, 1), (200, -1)):
        W = Z.copy()
        W[k, 3] += off
        assert _rejected(X, W, "size") == k


def test_replay_rejects_an_id_used_twice(base):
    X, Z = base
    W = Z.copy()
    W[41, 0] = Z[40, 0]                 # merged away one row earlier
    assert _rejected(X, W, "live") == 41
    W = Z.copy()
    W[7, 1] = len(X) + 7                # its own result
    assert _rejected(X, W, "live") == 7
    W = Z.copy()
    W[9, 0] = W[9, 1]
    assert _rejected(X, W, "live") == 9


def test_replay_rejects_an_unordered_pair(base):
    X, Z = base
    W = Z.copy()
    W[3, [0, 1]] = W[3, [1, 0]]
    assert _rejected(X, W, "order") == 3


def test_replay_rejects_two_rows_swapped(base):
    """Rows k and k + 1 that do not depend on each other, the later one at least 1e-6 farther: swapped (and the two new ids renamed in
    the rows after them, so that everything else stays consistent), the farther pair merges while the closer one is still there."""
    X, Z = base
    n = len(X)
    k = next(k for k in range(n - 2) if n + k not in Z[k + 1, :2] and Z[k + 1, 2] - Z[k, 2] > 1e-6)
    W = Z.copy()
    W[[k, k + 1]] = W[[k + 1, k]]
    ids = W[k + 2:, :2]
    a, b = ids == n + k, ids == n + k + 1
    ids[a], ids[b] = n + k + 1, n + k
    W[k + 2:, :2] = np.sort(ids, axis=1)
    assert _rejected(X, W, "minimum") == k


def test_replay_rejects_a_non_closest_pair_with_its_true_distance(base):
    X, Z = base
    a, b = (int(v) for v in Z[0, :2])
    c, e = [i for i in range(len(X)) if i not in (a, b)][:2]
    W = Z.copy()
    W[0] = (c, e, np.linalg.norm(X[c] - X[e]), 2)
    assert W[0, 2] > Z[0, 2] + 1e-6
    assert _rejected(X, W, "minimum") == 0


def test_partition_is_canonical():
    assert np.array_equal(ref.partition([7, 7, 2, 9, 2]), [0, 0, 1, 2, 1])
    assert np.array_equal(ref.partition([1, 1, 5, 3, 5]), ref.partition([7, 7, 2, 9, 2]))
    assert not np.array_equal(ref.partition([1, 1, 5, 3, 3]), ref.partition([7, 7, 2, 9, 2]))


@pytest.mark.parametrize("name", ["duplicates", "identical"])
def test_duplicate_input_partition_does_not_depend_on_row_order(name):
    """What the GPU tests compare with scipy on inputs with exact duplicates: under five row orders scipy gives the same partition at
    the threshold and the same sorted merge distances, and no merge distance is within 1e-6 of the threshold."""
    X = FAMILIES[name]
    Z = _scipy(X)
    assert np.abs(Z[:, 2] - ref.THRESHOLD).min() > 1e-6
    assert (Z[:, 2] == 0.0).sum() >= 99                   # the input really has runs of distance-0 merges
    want = ref.partition(fcluster(Z, ref.THRESHOLD, "distance"))
    rng = np.random.default_rng(5)
    for _ in range(5):
        perm = rng.permutation(len(X))
        Zp = _scipy(X[perm])
        ref.replay(X[perm], Zp)
        labels = np.empty(len(X), np.int64)
        labels[perm] = fcluster(Zp, ref.THRESHOLD, "distance")
        assert np.array_equal(ref.partition(labels), want)
        assert np.abs(np.sort(Zp[:, 2]) - np.sort(Z[:, 2])).max() < ref.TOL
        assert np.abs(Zp[:, 2] - ref.THRESHOLD).min() > 1e-6
