"""Test-side reference of the full-sum CTC score: an fp64 numpy statement of the forward-backward recursions, vectorised over the
states.

Extended sequence z = [b, y0, b, ..., y(L-1), b], S = 2L + 1.  alpha[0][0] = lp[0][b], alpha[0][1] = lp[0][y0];
alpha[t][s] = logsumexp(alpha[t-1][s], alpha[t-1][s-1] (, alpha[t-1][s-2] if z[s] != b and z[s] != z[s-2])) + lp[t][z[s]];
loglik = logsumexp(alpha[T-1][S-1], alpha[T-1][S-2]); beta is the mirror image and includes the emission of its own frame;
gamma[t][s] = alpha[t][s] + beta[t][s] - lp[t][z[s]] - loglik.  Per token k (state 2k + 1): occupancy = sum_t exp(gamma),
mean_frame = sum_t t exp(gamma) / occupancy, peak_post = max_t exp(gamma), peak_frame = the first frame of that maximum.
No normalisation is needed in fp64 at the sizes the tests use (|alpha| < 1e6, 1e-10 absolute)."""
import numpy as np

from force_align_ref import check_request, extend


def _lse(*xs):
    m = xs[0]
    for x in xs[1:]:
        m = np.maximum(m, x)
    mm = np.where(np.isneginf(m), 0.0, m)
    with np.errstate(divide="ignore"):
        return mm + np.log(sum(np.exp(x - mm) for x in xs))


def _skip(z, blank):
    S = len(z)
    skip = np.zeros(S, bool)
    skip[2:] = (z[2:] != blank) & (z[2:] != z[:-2])
    return skip


def _band(t, T, S):
    """the states of frame t that lie on a complete path: reachable from the start (s <= 2t + 1) and able to reach the end
    (s >= S - 2 (T - t)); alpha and beta are left at -inf outside it, where gamma is -inf anyway"""
    return max(0, S - 2 * (T - t)), min(S - 1, 2 * t + 1)


def forward(lp, y, blank=0):
    """-> (alpha [T, S] fp64, loglik)"""
    lp = np.asarray(lp, np.float64)
    T, V = lp.shape
    y = np.asarray(y, np.int64)
    check_request(T, V, y, blank)
    z = extend(y, blank)
    S = len(z)
    skip = _skip(z, blank)
    alpha = np.full((T, S), -np.inf)
    alpha[0, 0], alpha[0, 1] = lp[0, z[0]], lp[0, z[1]]
    prev = np.full(S + 2, -np.inf)
    for t in range(1, T):
        lo, hi = _band(t, T, S)
        prev[2:] = alpha[t - 1]
        p2 = np.where(skip[lo:hi + 1], prev[lo:hi + 1], -np.inf)
        alpha[t, lo:hi + 1] = _lse(prev[lo + 2:hi + 3], prev[lo + 1:hi + 2], p2) + lp[t, z[lo:hi + 1]]
    return alpha, float(_lse(alpha[-1, S - 1], alpha[-1, S - 2]))


def loglik(lp, y, blank=0):
    """fp64 log-likelihood only, O(S) memory."""
    lp = np.asarray(lp, np.float64)
    T, V = lp.shape
    y = np.asarray(y, np.int64)
    check_request(T, V, y, blank)
    z = extend(y, blank)
    S = len(z)
    skip = _skip(z, blank)
    a = np.full(S, -np.inf)
    a[0], a[1] = lp[0, z[0]], lp[0, z[1]]
    ninf1, ninf2 = np.full(1, -np.inf), np.full(2, -np.inf)
    for t in range(1, T):
        p1 = np.concatenate((ninf1, a[:-1]))
        p2 = np.where(skip, np.concatenate((ninf2, a[:-2])), -np.inf)
        a = _lse(a, p1, p2) + lp[t, z]
    return float(_lse(a[S - 1], a[S - 2]))


def backward(lp, y, blank=0):
    """-> beta [T, S] fp64 (beta[t][s] includes lp[t][z[s]])"""
    lp = np.asarray(lp, np.float64)
    T = lp.shape[0]
    z = extend(np.asarray(y, np.int64), blank)
    S = len(z)
    skip = _skip(z, blank)                               # s - 2 -> s allowed; seen from s: s -> s + 2 allowed iff skip[s + 2]
    up2 = np.concatenate((skip[2:], np.zeros(2, bool)))
    beta = np.full((T, S), -np.inf)
    beta[T - 1, S - 1], beta[T - 1, S - 2] = lp[T - 1, z[S - 1]], lp[T - 1, z[S - 2]]
    nxt = np.full(S + 2, -np.inf)
    for t in range(T - 2, -1, -1):
        lo, hi = _band(t, T, S)
        nxt[:S] = beta[t + 1]
        n2 = np.where(up2[lo:hi + 1], nxt[lo + 2:hi + 3], -np.inf)
        beta[t, lo:hi + 1] = _lse(nxt[lo:hi + 1], nxt[lo + 1:hi + 2], n2) + lp[t, z[lo:hi + 1]]
    return beta


def gamma(lp, y, blank=0):
    """-> (gamma [T, S] fp64 log-posteriors, loglik)"""
    lp64 = np.asarray(lp, np.float64)
    z = extend(np.asarray(y, np.int64), blank)
    alpha, ll = forward(lp64, y, blank)
    beta = backward(lp64, y, blank)
    g = alpha
    g += beta
    del beta
    for t in range(g.shape[0]):
        lo, hi = _band(t, g.shape[0], len(z))
        e = lp64[t, z[lo:hi + 1]]
        with np.errstate(invalid="ignore"):
            row = g[t, lo:hi + 1] - np.where(np.isneginf(e), 0.0, e) - ll
        row[np.isnan(row)] = -np.inf
        g[t, lo:hi + 1] = row
    return g, ll


def reduce_tokens(g):
    """gamma [T, S] -> dict of per-token occupancy, mean_frame, peak_post, peak_frame, and `second` = the largest posterior at any
    OTHER frame than peak_frame (how far the peak frame is from a tie)."""
    p = np.zeros((g.shape[0], g.shape[1] // 2))          # [T, L]
    tok = g[:, 1::2]
    live = ~np.isneginf(tok)
    p[live] = np.exp(tok[live])
    T = p.shape[0]
    occ = p.sum(0)
    mean = (np.arange(T)[:, None] * p).sum(0) / occ
    pf = p.argmax(0)                                     # first maximum
    peak = p[pf, np.arange(p.shape[1])]
    q = p.copy()
    q[pf, np.arange(p.shape[1])] = -1.0
    second = q.max(0) if T > 1 else np.zeros(p.shape[1])
    return {"occupancy": occ, "mean_frame": mean, "peak_post": peak, "peak_frame": pf.astype(np.int64), "second": second}


def score(lp, y, blank=0):
    """-> (loglik, per-token dict)"""
    g, ll = gamma(lp, y, blank)
    return ll, reduce_tokens(g)


def make_logits(seed, T, V, L, scale=1.0, repeats_at=(), blank=0):
    """Seeded (logits fp32 [T, V], y int32 [L]): scale * N(0, 1) logits; tokens uniform over the non-blank ids with no adjacent
    repeat except y[i] = y[i - 1] forced for every i in repeats_at."""
    rng = np.random.default_rng([seed, T, V, L])
    y = rng.integers(1, V, L).astype(np.int32)
    for i in range(1, L):
        if y[i] == y[i - 1]:
            y[i] = 1 + (y[i] % (V - 1))
    for i in sorted(repeats_at):
        if 1 <= i < L:
            y[i] = y[i - 1]
            if i + 1 < L and y[i + 1] == y[i] and (i + 1) not in repeats_at:
                y[i + 1] = 1 + (y[i + 1] % (V - 1))
    return (rng.standard_normal((T, V)) * scale).astype(np.float32), y


def log_softmax64(logits):
    x = np.asarray(logits, np.float64)
    m = x.max(1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(1, keepdims=True))


def make_lattice(seed, T, V, L, scale=1.0, repeats_at=(), blank=0):
    """Seeded (lp fp32 [T, V], y int32 [L]): the fp32 log-softmax of make_logits."""
    logits, y = make_logits(seed, T, V, L, scale, repeats_at, blank)
    m = logits.max(1, keepdims=True)
    lp = (logits - m - np.log(np.exp(logits - m).sum(1, keepdims=True, dtype=np.float32))).astype(np.float32)
    return np.ascontiguousarray(lp), y
