"""Test-side statement of hot-word context biasing: the phrase automaton and the CTC prefix beam search that carries its scores,
in plain Python floats (float64), written from the behaviour the goldens of tests/golden/context_bias.json pin down.

Graph.  Node 0 is the root (token -1, all scores 0, fail arc to itself).  Phrases are inserted token by token; a node is created
the first time its prefix is seen, with token_score = c, node_score = parent's node_score + c, and is_end / output_score =
node_score only if the phrase that CREATES it ends there (a later phrase ending on an existing node marks nothing).  Children keep
insertion order; fail and output arcs are filled breadth-first in that order.  fail(n) for a child n of p over token k: follow
p.fail; if it has k, its k-child; else step to its fail and keep stepping while k is missing, stopping at the root; take the
k-child if the stop has one.  output(n): the first is_end node on the fail chain starting AT fail(n), none once the root is
reached; its output_score is added to n's.  step(state, k): a k-child gives its token_score; else the node found by the same fail
walk from state.fail gives node_score(found) - node_score(state); either way plus output_score of the node reached.
finalize(state) = -node_score(state), whether or not state ends a phrase.

Search.  Per frame, top-k tokens outer, beam entries inner.  Every candidate entry of the frame takes its context (state, score)
the FIRST time it is touched: unchanged prefixes copy the beam entry's, extended prefixes add step() to it.  The frame's candidates
are cut to the beam by score + context score, descending, stable.  After the last frame each survivor's context score is REPLACED
by finalize of its state (not added, no re-sort); reported scores are score + that.  The un-updated Viterbi score of a repeated
token (the misspelled attribute of the original) is kept: only the peak time moves.

Also here: the seeded lattices and phrase sets the goldens and the tests regenerate their inputs from."""
import hashlib
import math
from collections import deque

import numpy as np

NEG_INF = -float("inf")


class Graph:
    def __init__(self, phrases, context_score):
        self.c = context_score
        self.token, self.kids = [-1], [{}]
        self.token_score, self.node_score, self.output_score, self.is_end = [0], [0], [0], [False]
        self.fail, self.output = [0], [None]
        for phrase in phrases:
            n = 0
            for i, k in enumerate(phrase):
                if k not in self.kids[n]:
                    end = i == len(phrase) - 1
                    ns = self.node_score[n] + context_score
                    self.kids[n][k] = len(self.token)
                    self.token.append(k); self.kids.append({})
                    self.token_score.append(context_score); self.node_score.append(ns)
                    self.output_score.append(ns if end else 0); self.is_end.append(end)
                    self.fail.append(0); self.output.append(None)
                n = self.kids[n][k]
        queue = deque(self.kids[0].values())
        while queue:
            p = queue.popleft()
            for k, n in self.kids[p].items():
                self.fail[n] = self._fail_target(self.fail[p], k)
                o = self.fail[n]
                while o is not None and not self.is_end[o]:
                    o = self.fail[o]
                    if o == 0:
                        o = None
                self.output[n] = o
                if o is not None:
                    self.output_score[n] += self.output_score[o]
                queue.append(n)

    @property
    def num_nodes(self):
        return len(self.token) - 1

    def _fail_target(self, f, k):
        """from f (already one fail step taken): f's k-child if any; else keep stepping until a node has k or the root is hit"""
        if k in self.kids[f]:
            return self.kids[f][k]
        f = self.fail[f]
        while k not in self.kids[f]:
            f = self.fail[f]
            if f == 0:
                break
        return self.kids[f].get(k, f)

    def step(self, state, k):
        if k in self.kids[state]:
            n = self.kids[state][k]
            score = self.token_score[n]
        else:
            f = self.fail[state]
            while k not in self.kids[f]:
                f = self.fail[f]
                if f == 0:
                    break
            n = self.kids[f].get(k, f)
            score = self.node_score[n] - self.node_score[state]
        return score + self.output_score[n], n

    def finalize(self, state):
        return -self.node_score[state], 0


def log_add(a, b):
    if a == NEG_INF and b == NEG_INF:
        return NEG_INF
    m = max(a, b)
    return m + math.log(math.exp(a - m) + math.exp(b - m))


class _Entry:
    def __init__(self):
        self.s = self.ns = self.v_s = self.v_ns = self.cur = NEG_INF
        self.t_s, self.t_ns = [], []
        self.state, self.bonus, self.latched = 0, 0.0, False

    def score(self):
        return log_add(self.s, self.ns)

    def viterbi(self):
        return self.v_s if self.v_s > self.v_ns else self.v_ns

    def times(self):
        return self.t_s if self.v_s > self.v_ns else self.t_ns


def search(top_logp, top_idx, num_t, beam, blank=0, graph=None):
    """top_logp / top_idx: [T][>= beam] per-frame log-probs / ids, best first.  -> dict(nbest, scores, times, context)."""
    def keep(n, src):
        if graph is not None and not n.latched:
            n.state, n.bonus, n.latched = src.state, src.bonus, True

    def advance(n, src, k):
        if graph is not None and not n.latched:
            sc, st = graph.step(src.state, k)
            n.state, n.bonus, n.latched = st, src.bonus + sc, True

    first = _Entry()
    first.s, first.v_s, first.v_ns = 0.0, 0.0, 0.0
    beam_now = [((), first)]
    for t in range(num_t):
        cand = {}

        def at(prefix):
            if prefix not in cand:
                cand[prefix] = _Entry()
            return cand[prefix]
        for j in range(beam):
            k, p = int(top_idx[t][j]), float(top_logp[t][j])
            for prefix, e in beam_now:
                if k == blank:
                    n = at(prefix)
                    n.s = log_add(n.s, e.score() + p)
                    n.v_s = e.viterbi() + p
                    n.t_s = list(e.times())
                    keep(n, e)
                elif prefix and k == prefix[-1]:
                    n = at(prefix)
                    n.ns = log_add(n.ns, e.ns + p)
                    if n.v_ns < e.v_ns + p and n.cur < p:      # v_ns itself stays: only the peak moves
                        n.cur = p
                        n.t_ns = list(e.t_ns)
                        n.t_ns[-1] = t
                    keep(n, e)
                    m = at(prefix + (k,))
                    m.ns = log_add(m.ns, e.s + p)
                    if m.v_ns < e.v_s + p:
                        m.v_ns, m.cur = e.v_s + p, p
                        m.t_ns = list(e.t_s) + [t]
                    advance(m, e, k)
                else:
                    m = at(prefix + (k,))
                    m.ns = log_add(m.ns, e.score() + p)
                    if m.v_ns < e.viterbi() + p:
                        m.v_ns, m.cur = e.viterbi() + p, p
                        m.t_ns = list(e.times()) + [t]
                    advance(m, e, k)
        ranked = sorted(cand.items(), key=lambda kv: kv[1].score() + (kv[1].bonus if graph is not None else 0.0), reverse=True)
        beam_now = ranked[:beam]
    if graph is not None:
        for _, e in beam_now:
            e.bonus, e.state = graph.finalize(e.state)
    return {"nbest": [list(p) for p, _ in beam_now],
            "scores": [e.score() + e.bonus if graph is not None else e.score() for _, e in beam_now],
            "times": [list(e.times()) for _, e in beam_now],
            "context": [e.bonus for _, e in beam_now] if graph is not None else None}


# ------------------------------------------------------------------------------------------------ seeded inputs
def make_lattice(seed, T, V, kind="random"):
    """fp32 log-softmax lattice [T, V], blank = 0.  Computed in float64 and rounded once, so that the float32 bits do not hang on
    a library's float32 exp / log; `digest` pins them.  kind "blank": the blank wins every frame by a wide margin."""
    rng = np.random.default_rng(seed)
    logits = rng.standard_normal((T, V)) * 2.0
    logits[:, 0] += 3.0
    if kind == "blank":
        logits[:, 0] += 12.0
    m = logits.max(axis=1, keepdims=True)
    lp = logits - m - np.log(np.exp(logits - m).sum(axis=1, keepdims=True))
    return np.ascontiguousarray(lp, np.float32)


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:12]


def topk(lp, beam):
    """per-frame top-`beam`, best first; ties (none in the seeded lattices) by lower id.  -> (values fp32 [T, beam], ids int32)"""
    idx = np.argsort(-lp.astype(np.float64), axis=1, kind="stable")[:, :beam]
    return np.ascontiguousarray(np.take_along_axis(lp, idx, axis=1), np.float32), np.ascontiguousarray(idx, np.int32)


def phrases_from(nbest, n=3):
    """Hot words for a lattice: token n-grams (2 and 1 long) of the lower-ranked hypotheses that the best one does not contain."""
    best = tuple(nbest[0])
    have = {best[i:i + w] for w in (1, 2) for i in range(len(best) - w + 1)}
    out = []
    for w in (2, 1):
        for h in nbest[1:]:
            for i in range(len(h) - w + 1):
                g = tuple(h[i:i + w])
                if g not in have and list(g) not in out:
                    out.append(list(g))
    return out[:n]


def stream(seed, n, V):
    """token stream for a graph walk: ids 1 .. V-1"""
    return np.random.default_rng(seed).integers(1, V, n).tolist()


# phrase sets of the graph walks: shared prefixes; a phrase that is a suffix of another ([2,3] of [1,2,3]); one that is a prefix of
# an EARLIER one ([1,2] after [1,2,3]) and of a LATER one ([4] before [4,4,2]); repeated tokens inside a phrase; single-token
# phrases; a duplicate; an empty phrase
WALK_SETS = {
    "mixed": [[1, 2, 3], [2, 3], [1, 2], [1, 2, 4], [4], [4, 4, 2], [], [2, 3], [3, 3, 3], [5]],
    "nested": [[1], [1, 1], [1, 1, 1], [2, 1, 1], [1, 2, 1, 2], [2, 1]],
    "chain": [[1, 2, 3, 4], [2, 3, 4], [3, 4], [4], [3, 1]],
}
