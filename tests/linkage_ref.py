"""Reference for the centroid-linkage tests: a replay oracle that does not depend on how ties are broken, and the inputs the tests share.

scipy.cluster.hierarchy.linkage(X, "centroid") pins the kernels on tie-free input (same merges in the same order).  With equal
distances the order of the merges is an accident of the implementation -- scipy's heap orders equal keys by its layout, the kernels by
(distance, slot) -- so there `replay` decides: it walks a dendrogram with the real fp64 centroids and accepts it exactly when every
merge joins a closest pair of the clusters alive at that moment, i.e. when it is a greedy centroid linkage under SOME tie order."""
import numpy as np

TOL = 1e-9                              # the figure the project pins linkage distances at
THRESHOLD = 0.7045654963945799          # the pipeline's clustering threshold (fcluster(Z, t, "distance"))


class ReplayError(AssertionError):
    """`check` names what failed: "shape", "live", "order", "size", "distance" or "minimum"; `k` the merge."""

    def __init__(self, check, k, text):
        super().__init__(f"merge {k}: {check}: {text}")
        self.check, self.k = check, k


def replay(X, Z, tol=TOL):
    """Walks dendrogram Z [n-1][4] over the points X [n][d] with real centroids and sizes (no Lance-Williams recurrence).  At merge k:
    both ids are alive, Z[k,0] < Z[k,1], the new cluster gets id n + k; Z[k,3] is the sum of the two sizes; |Z[k,2] - ||c_a - c_b|||
    <= tol; no pair of live centroids is closer than Z[k,2] - tol.  Raises ReplayError on the first violation.
    -> (worst |Z[k,2] - ||c_a - c_b|||, worst Z[k,2] - (smallest live distance))."""
    X = np.asarray(X, np.float64)
    Z = np.asarray(Z, np.float64)
    n = X.shape[0]
    if Z.shape != (max(n - 1, 0), 4) or not np.all(np.isfinite(Z)):
        raise ReplayError("shape", -1, f"{Z.shape} for {n} points, or a non-finite entry")
    # a cluster lives in a slot (the merged cluster takes over the slot of its second member): slot_of[id], -1 once merged away
    cent = X.copy()
    size = np.ones(n, np.int64)
    slot_of = np.full(2 * n - 1, -1, np.int64)
    slot_of[:n] = np.arange(n)
    ident = np.arange(n)                     # the id a slot holds
    # squared distances between the live slots; dead slots and the diagonal hold +inf
    P = np.empty((n, n))
    for i in range(n):
        P[i] = ((X - X[i]) ** 2).sum(axis=1)
    P[np.arange(n), np.arange(n)] = np.inf
    worst_d = worst_m = 0.0
    for k in range(n - 1):
        a, b, dist, cnt = Z[k]
        if a != int(a) or b != int(b) or not (0 <= a < n + k and 0 <= b < n + k):
            raise ReplayError("live", k, f"ids {a}, {b}")
        a, b = int(a), int(b)
        sa, sb = slot_of[a], slot_of[b]
        if sa < 0 or sb < 0 or a == b:
            raise ReplayError("live", k, f"ids {a}, {b} are not two live clusters")
        if not a < b:
            raise ReplayError("order", k, f"{a} !< {b}")
        if cnt != size[sa] + size[sb]:
            raise ReplayError("size", k, f"{cnt} != {size[sa]} + {size[sb]}")
        true = float(np.sqrt(((cent[sa] - cent[sb]) ** 2).sum()))
        worst_d = max(worst_d, abs(dist - true))
        if abs(dist - true) > tol:
            raise ReplayError("distance", k, f"{dist!r} for centroids {true!r} apart")
        low = float(np.sqrt(P.min()))
        worst_m = max(worst_m, dist - low)
        if low < dist - tol:
            i, j = np.unravel_index(np.argmin(P), P.shape)
            raise ReplayError("minimum", k, f"merged at {dist!r} while {ident[i]} and {ident[j]} are {low!r} apart")
        cent[sb] = (size[sa] * cent[sa] + size[sb] * cent[sb]) / (size[sa] + size[sb])
        size[sb] += size[sa]
        size[sa] = 0
        slot_of[a] = slot_of[b] = -1
        slot_of[n + k] = sb
        ident[sb] = n + k
        P[sa, :] = P[:, sa] = np.inf
        row = ((cent - cent[sb]) ** 2).sum(axis=1)
        row[size == 0] = np.inf
        row[sb] = np.inf
        P[sb, :] = P[:, sb] = row
    return worst_d, worst_m


def partition(labels):
    """Canonical relabelling: clusters numbered 0, 1, ... by their first member, so two labelings are the same partition exactly when
    their canonical forms are equal."""
    labels = np.asarray(labels)
    _, first, inv = np.unique(labels, return_index=True, return_inverse=True)
    rank = np.empty(len(first), np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(len(first))
    return rank[inv.reshape(-1)]


# ------------------------------------------------------------------------------------ inputs
def _sphere(X):
    return (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float32).astype(np.float64)


def blobs(n, d, seed, centers=5, spread=0.35):
    """Gaussian blobs on the unit sphere, fp32 values in fp64 (what the pipeline's embeddings are); tie-free in practice."""
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((centers, d))
    return _sphere(c[rng.integers(centers, size=n)] + spread * rng.standard_normal((n, d)))


def duplicated_blobs(n=240, dup=120, d=16, seed=31):
    """n blob points plus `dup` exact copies of rows drawn from them (digital silence, a repeated jingle), shuffled."""
    X = blobs(n, d, seed)
    rng = np.random.default_rng(seed + 1000)
    X = np.concatenate([X, X[rng.integers(n, size=dup)]])
    return np.ascontiguousarray(X[rng.permutation(len(X))])


def identical_points(same=100, others=39, d=16, seed=32):
    """`same` copies of one point among `others` blob points, shuffled."""
    X = blobs(others + 1, d, seed)
    rng = np.random.default_rng(seed + 1000)
    X = np.concatenate([np.repeat(X[:1], same, axis=0), X[1:]])
    return np.ascontiguousarray(X[rng.permutation(len(X))])


def lattice(*shape):
    """The integer lattice of that shape (row-major): every distance is tied many times over."""
    g = np.meshgrid(*[np.arange(s, dtype=np.float64) for s in shape], indexing="ij")
    return np.ascontiguousarray(np.stack([a.reshape(-1) for a in g], axis=1))


def noise(n, d, seed):
    """Normalised Gaussian noise: in high dimension a few hub points are everybody's nearest neighbour, so most candidates go stale."""
    return _sphere(np.random.default_rng(seed).standard_normal((n, d)))


def tie_inputs():
    """name -> X for the inputs with tied distances; the first two also have a partition at THRESHOLD that is compared with scipy's."""
    return {"duplicates": duplicated_blobs(), "identical": identical_points(), "lattice12x12": lattice(12, 12), "lattice6x6x6": lattice(6, 6, 6)}
