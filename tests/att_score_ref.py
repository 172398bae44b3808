"""fp64 numpy restatement of the attention decoder's loss and accuracy as the reference computes them for a known transcript
(ASRModel._calc_att_loss, asr_model.py:248-286): LabelSmoothingLoss (label_smoothing_loss.py:68-96) and th_accuracy
(utils/common.py:268-287).  Written from the formulas, not from the engine:

    true_dist[v] = smoothing / (V - 1) for v != target, 1 - smoothing at the target
    kl(row)      = sum_v true_dist[v] * (ln true_dist[v] - log_softmax(x)[v])          (KLDivLoss, 0 ln 0 = 0)
    loss         = sum over rows whose target is not ignore_id / (their number if normalize_length else the batch size)
    accuracy     = rows whose arg-max (first maximum) equals the target / rows, over the same rows

and the closed form the engine's host code uses, with u = smoothing / (V - 1), c = 1 - smoothing, logp_t = x[t] - lse and
sum_v log p(v) = sum_x - V lse:

    kl = c ln c + (V - 1) u ln u - c logp_t - u (sum_x - V lse - logp_t)

tests/test_att_score_ref.py pins both against tests/golden/att_score.json (the reference's own modules on the same seeded logits,
scripts/gen_golden_att_score.py)."""
import numpy as np

IGNORE_ID = -1


def log_softmax(x):
    x = np.asarray(x, np.float64)
    m = x.max(axis=-1, keepdims=True)
    return x - (m + np.log(np.exp(x - m).sum(axis=-1, keepdims=True)))


def _xlogx(p):
    return p * np.log(p) if p > 0.0 else 0.0


def kl_dense(x, target, smoothing):
    """Per row of x [N, V] (targets [N], all valid): the dense sum over the vocabulary."""
    x = np.asarray(x, np.float64)
    N, V = x.shape
    lp = log_softmax(x)
    dist = np.full((N, V), smoothing / (V - 1), np.float64)
    dist[np.arange(N), target] = 1.0 - smoothing
    with np.errstate(divide="ignore", invalid="ignore"):
        term = np.where(dist > 0.0, dist * (np.log(np.where(dist > 0.0, dist, 1.0)) - lp), 0.0)
    return term.sum(axis=1)


def compose(logp_t, lse, sum_x, V, smoothing):
    """The closed form from the three row statistics (arrays or scalars, fp64)."""
    c, u = 1.0 - smoothing, smoothing / (V - 1)
    logp_t, lse, sum_x = (np.asarray(a, np.float64) for a in (logp_t, lse, sum_x))
    return _xlogx(c) + (V - 1) * _xlogx(u) - c * logp_t - u * (sum_x - V * lse - logp_t)


def row_stats(x):
    """lse, sum of the logits and arg-max (first maximum) per row of x [N, V], fp64."""
    x = np.asarray(x, np.float64)
    m = x.max(axis=-1)
    return m + np.log(np.exp(x - m[:, None]).sum(axis=-1)), x.sum(axis=-1), x.argmax(axis=-1)


def kl_closed(x, target, smoothing):
    x = np.asarray(x, np.float64)
    lse, sum_x, _ = row_stats(x)
    return compose(x[np.arange(x.shape[0]), target] - lse, lse, sum_x, x.shape[1], smoothing)


def loss(x, targets, smoothing, normalize_length, closed=False):
    """x [B, L, V], targets [B, L] padded with IGNORE_ID -> LabelSmoothingLoss.forward."""
    x = np.asarray(x, np.float64)
    B, L, V = x.shape
    t = np.asarray(targets).reshape(-1)
    keep = t != IGNORE_ID
    rows = x.reshape(-1, V)[keep]
    kl = (kl_closed if closed else kl_dense)(rows, t[keep], smoothing)
    return kl.sum() / (int(keep.sum()) if normalize_length else B)


def accuracy(x, targets):
    """th_accuracy: (correct, positions) over the rows that are not padding."""
    x = np.asarray(x, np.float64)
    t = np.asarray(targets).reshape(-1)
    keep = t != IGNORE_ID
    pred = x.reshape(-1, x.shape[-1]).argmax(axis=-1)
    return int((pred[keep] == t[keep]).sum()), int(keep.sum())


def make_case(seed, lens, V, scale=2.0, tie=False):
    """Seeded logits [B, max(lens), V] (fp64, N(0, scale)) and targets padded with IGNORE_ID.  Half of the targets are the row's
    arg-max (so that the accuracy is not trivially 0).  tie: in row 0 of every sequence the maximum is duplicated at two indices and
    the target is the HIGHER one -- the first maximum wins the arg-max, so that row counts as wrong."""
    rng = np.random.default_rng(seed)
    B, L = len(lens), max(lens)
    x = rng.standard_normal((B, L, V)) * scale
    t = np.full((B, L), IGNORE_ID, np.int64)
    for b, n in enumerate(lens):
        t[b, :n] = rng.integers(0, V, n)
        for j in range(0, n, 2):
            t[b, j] = int(x[b, j].argmax())
        if tie:
            lo, hi = sorted(rng.choice(V, 2, replace=False).tolist())
            x[b, 0, lo] = x[b, 0, hi] = x[b, 0].max() + 1.0
            t[b, 0] = hi
    return x, t
