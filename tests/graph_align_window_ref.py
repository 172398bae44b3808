"""Test-side reference of the WINDOWED CTC alignment over a token graph (csrc/ctc_graph_window.hip): a numpy restatement of the rules of
include/rvb.h (rvb_ctc_align_graph_long_*), in fp32, vectorised over the window and independent of the kernel.

The graph, the states B_start, T_j, B_j, the candidate order and "first maximum wins" are tests/graph_align_ref.py's, and so is the padded
candidate matrix ([N, 1 + 2 D] indices into X = [B_start, T_0.., B_0.., -inf]; np.argmax returns the FIRST maximum).  What is added:
  * only the nodes lo_of[t] <= j < min(lo_of[t] + W, N) are alive at frame t, and B_start only while lo_of[t] == 0;
  * a predecessor candidate p -> T_j counts iff j is alive and p >= lo_of[t] (p = -1: iff lo_of[t] == 0); the stay candidates of an alive
    node always count; a candidate that does not count is -inf and never wins.  Here: when the window moves, everything below it is SET
    to -inf, which is the same thing, because lo never decreases and nothing below lo is alive again;
  * a node above every window so far was never written and holds -inf;
  * the path ends in the first maximum of (B_f, T_f) over the final nodes alive at the last frame, ascending;
  * min_margin: over the frames of the chosen path that sit on a node (blank frames count with their node, B_start frames do not), the
    smallest of node - lo_of[t] where lo_of[t] > 0 and lo_of[t] + W - 1 - node where lo_of[t] + W < N; W when no frame counts.
Also here: the window policy (tables(), next_window()) and a driver that cuts the launches as the library does (graph_align_window)."""
import numpy as np

from graph_align_ref import W as WILDCARD

DEFAULT_W = 8192
NINF = np.float32(-np.inf)
FAR = 1 << 30              # need[] of a node from which no final node is reached


def pad64(n):
    return (n + 63) // 64 * 64


def check_window(window_nodes):
    if window_nodes != 0 and (window_nodes < 256 or window_nodes > 8192 or window_nodes % 256):
        raise ValueError("window_nodes must be 0 or a multiple of 256 in [256, 8192]")


def effective_window(N, window_nodes):
    return min(window_nodes or DEFAULT_W, pad64(N))


class Band:
    """the lattice of one graph, advanced frame by frame with the window given for each frame"""

    def __init__(self, lp, tokens, preds, finals, W, blank=0, w=None, bias=0.0):
        lp = np.asarray(lp)
        assert lp.dtype == np.float32 and lp.ndim == 2
        self.lp, self.blank, self.W = lp, blank, W
        self.T = lp.shape[0]
        self.tokens = tokens = np.asarray(tokens, np.int64)
        self.preds, self.finals = preds, np.asarray(finals, bool)
        self.N = N = len(tokens)
        assert W % 64 == 0 and W >= 64
        D = max(len(p) for p in preds)
        SENT = 2 * N + 1
        idx = np.full((N, 1 + 2 * D), SENT, np.int64)
        idx[:, 0] = 1 + np.arange(N)
        self.from_start = np.zeros(N, bool)
        for j, ps in enumerate(preds):
            assert len(ps) >= 1 and len(set(ps)) == len(ps) and all(-1 <= p < j for p in ps)
            for k, p in enumerate(ps):
                if p < 0:
                    idx[j, 1 + 2 * k] = 0
                    self.from_start[j] = True
                else:
                    idx[j, 1 + 2 * k] = 1 + N + p
                    if tokens[p] != tokens[j]:
                        idx[j, 2 + 2 * k] = 1 + p
        self.idx = idx
        self.wild = tokens == WILDCARD
        self.cols = np.where(self.wild, blank, tokens)
        self.ew = None
        if self.wild.any():
            self.ew = (np.asarray(w, np.float32) + np.float32(bias)).astype(np.float32)
        self.X = np.full(2 * N + 2, NINF, np.float32)
        self.bpT = np.zeros((self.T, W), np.uint8)               # window-relative, as the kernel's bytes are
        self.bpB = np.zeros((self.T, W), bool)
        self.lo_of = np.zeros(self.T, np.int32)
        self.lo = 0
        self.t = 0

    def emission(self, t, a, b):
        e = self.lp[t, self.cols[a:b]].copy()
        if self.ew is not None:
            e[self.wild[a:b]] = self.ew[t]
        return e

    def frame(self, lo):
        """advance over frame self.t with the window [lo, lo + W)"""
        t, N, W, X, lp = self.t, self.N, self.W, self.X, self.lp
        assert lo % 64 == 0 and lo >= self.lo and (t > 0 or lo == 0)
        hi = min(lo + W, N)
        if lo > self.lo:                                        # below the window: never read again
            X[0] = NINF
            X[1:1 + min(lo, N)] = NINF
            X[1 + N:1 + N + min(lo, N)] = NINF
        self.lo = lo
        self.lo_of[t] = lo
        if t == 0:
            X[0] = lp[0, self.blank]
            fs = self.from_start[:hi]
            X[1:1 + hi][fs] = self.emission(0, 0, hi)[fs]
        elif hi > lo:
            cand = X[self.idx[lo:hi]]
            arg = np.argmax(cand, axis=1)
            self.bpT[t, :hi - lo] = arg
            Tn = cand[np.arange(hi - lo), arg] + self.emission(t, lo, hi)
            Tp, Bp = X[1 + lo:1 + hi], X[1 + N + lo:1 + N + hi]
            fromT = Tp > Bp
            self.bpB[t, :hi - lo] = fromT
            Bn = np.where(fromT, Tp, Bp) + lp[t, self.blank]
            if lo == 0:
                X[0] = X[0] + lp[t, self.blank]
            X[1 + lo:1 + hi] = Tn
            X[1 + N + lo:1 + N + hi] = Bn
            assert X.dtype == np.float32
        self.t = t + 1

    def best(self):
        """the node of the FIRST maximum of the window in the order B_start, T_lo, B_lo, T_lo+1, ... (B_start: node 0); -1: none finite"""
        lo, N, X = self.lo, self.N, self.X
        hi = min(lo + self.W, N)
        inter = np.empty(1 + 2 * max(hi - lo, 0), np.float32)
        inter[0] = X[0] if lo == 0 else NINF
        inter[1::2] = X[1 + lo:1 + hi]
        inter[2::2] = X[1 + N + lo:1 + N + hi]
        k = int(np.argmax(inter))
        if not inter[k] > NINF:
            return -1
        return 0 if k == 0 else lo + (k - 1) // 2

    def finish(self):
        """-> (labels [T], frame_node [T], fp32 score, min_margin); ValueError when no path inside the windows has a finite score"""
        assert self.t == self.T
        N, W, X, T = self.N, self.W, self.X, self.T
        lo = int(self.lo_of[T - 1])
        best, node, tok_state = NINF, -1, False
        for f in np.nonzero(self.finals)[0]:
            if not lo <= f < min(lo + W, N):
                continue
            if X[1 + N + f] > best:
                best, node, tok_state = X[1 + N + f], int(f), False
            if X[1 + f] > best:
                best, node, tok_state = X[1 + f], int(f), True
        if not best > NINF:
            raise ValueError("infeasible: no path inside the window with a finite score")
        labels, fnode = np.empty(T, np.int32), np.empty(T, np.int32)
        margin = W
        for t in range(T - 1, -1, -1):
            labels[t] = self.tokens[node] if tok_state else self.blank
            fnode[t] = node if tok_state else -1
            if node < 0:
                continue                                        # B_start only stays, and does not count
            lo = int(self.lo_of[t])
            i = node - lo
            assert 0 <= i < W
            if lo > 0:
                margin = min(margin, i)
            if lo + W < N:
                margin = min(margin, W - 1 - i)
            if t == 0:
                continue
            if tok_state:
                c = int(self.bpT[t, i])
                if c:
                    p = self.preds[node][(c - 1) // 2]
                    assert p >= lo or (p < 0 and lo == 0)
                    node, tok_state = p, (c - 1) % 2 == 1
            else:
                tok_state = bool(self.bpB[t, i])
        return labels, fnode, np.float32(best), int(margin)


def graph_align_band(lp, tokens, preds, finals, W, lo_of, blank=0, w=None, bias=0.0):
    """the band alignment on a GIVEN window per frame (W as the library reduced it) -> (labels, frame_node, score, min_margin)"""
    band = Band(lp, tokens, preds, finals, W, blank, w, bias)
    for t in range(band.T):
        band.frame(int(lo_of[t]))
    return band.finish()


# ------------------------------------------------------------------------------------------------ the window policy
def tables(tokens, preds, finals):
    """-> (M, startmax, need, E): M[j] the largest successor of any node <= j (j itself where there is none); startmax the highest node
    with a start predecessor; need[j] the fewest further frames from T_j to a final node (an arc between equal labels costs two: the
    blank between them); E[r] the lowest node with need <= r, for r = 0 .. len(E) - 1 (larger r: E[-1])."""
    N = len(tokens)
    M = np.arange(N, dtype=np.int64)
    startmax = -1
    succ = [[] for _ in range(N)]
    for j, ps in enumerate(preds):
        for p in ps:
            if p < 0:
                startmax = j
            else:
                M[p] = max(M[p], j)
                succ[p].append(j)
    M = np.maximum.accumulate(M)
    need = np.full(N, FAR, np.int64)
    for j in range(N - 1, -1, -1):
        if finals[j]:
            need[j] = 0
            continue
        for s in succ[j]:
            if need[s] < FAR:
                need[j] = min(need[j], need[s] + (1 if tokens[j] != tokens[s] else 2))
    top = int(need[need < FAR].max())
    E = np.full(top + 1, N, np.int64)
    for j in range(N - 1, -1, -1):
        if need[j] < FAR:
            E[need[j]] = j
    E = np.minimum.accumulate(E)
    return M, startmax, need, E


def min_frames(tokens, preds, finals):
    """the frames the graph's shortest reading needs"""
    _, _, need, _ = tables(tokens, preds, finals)
    return int(min(1 + need[j] for j, ps in enumerate(preds) if -1 in ps))


def max_span(preds):
    """-> (span, node): the largest j - p over the arcs, a start predecessor counting as j + 1"""
    return max((j - p, j) for j, ps in enumerate(preds) for p in ps)


def next_window(tab, N, T, W, f0, fend, lo_prev, best_prev):
    """The launch that starts at frame f0 of a slab that ends at fend -> (lo, f1).  Three steps, in this order."""
    M, startmax, _, E = tab
    top = max(0, pad64(N) - W)
    if f0 == 0:                                                   # 1. place the window
        lo, c = 0, startmax
    else:
        lo = (best_prev - W // 2) // 64 * 64 if best_prev >= 0 else lo_prev      # Python floors: also right below zero
        lo = min(max(lo, lo_prev, 0), top)
        c = max(best_prev, lo)
    f1 = f0                                                       # 2. as many frames as the climber stays inside for
    while f1 < fend:
        nc = int(M[c]) if f1 > 0 else c
        if f1 > f0 and lo + W < N and nc > lo + W - 1:
            break
        c = nc
        f1 += 1
    e = int(E[min(T - f1, len(E) - 1)])                           # 3. the end stays reachable
    if lo + W - 1 < e:
        lo = min(pad64(e - W + 1), top)
    return lo, f1


def graph_align_window(lp, tokens, preds, finals, window_nodes=0, slab_rows=8192, blank=0, w=None, bias=0.0):
    """the driver: slabs of slab_rows frames, each cut into launches by next_window(), which is fed the node that best() reports after
    the launch before -> (labels, frame_node, score, lo_of [T], min_margin, launches)"""
    check_window(window_nodes)
    N, T = len(tokens), len(lp)
    W = effective_window(N, window_nodes)
    if W < N and max_span(preds)[0] > W // 2 - 64:
        raise ValueError("arc span above W / 2 - 64")
    tab = tables(tokens, preds, finals)
    if T < min_frames(tokens, preds, finals):
        raise ValueError("infeasible: the shortest reading needs more frames")
    band = Band(lp, tokens, preds, finals, W, blank, w, bias)
    lo, best, launches = 0, -1, 0
    for s0 in range(0, T, slab_rows):
        s1 = min(T, s0 + slab_rows)
        f0 = s0
        while f0 < s1:
            lo, f1 = next_window(tab, N, T, W, f0, s1, lo, best)
            assert f0 < f1 <= s1
            for _ in range(f0, f1):
                band.frame(lo)
            best = band.best()
            launches += 1
            f0 = f1
    labels, fnode, score, margin = band.finish()
    return labels, fnode, score, band.lo_of.copy(), margin, launches


# ------------------------------------------------------------------------------------------------ the cases the tests share
def peaked_lp(rng, y, T, V, blank=0):
    """log-probs peaked on a random frame labelling of y: N(0, 1) logits, +4 on the planted label, then log-softmax"""
    import force_align_ref as R
    path = R.planted_path(rng, np.asarray(y), T, blank)
    logits = rng.standard_normal((T, V)).astype(np.float32)
    logits[np.arange(T), path] += np.float32(4.0)
    m = logits.max(1, keepdims=True)
    lp = (logits - m - np.log(np.exp(logits - m).sum(1, keepdims=True, dtype=np.float32))).astype(np.float32)
    return np.ascontiguousarray(lp)


def peaked_case(kind, seed, L, V, T=None, **kw):
    """a graph of tests/graph_align_ref.py's generators around a random reading y without adjacent repeats, and log-probs peaked on a
    planted frame labelling of y over T = 1.6 L frames -> (lp, tokens, preds, finals, y)"""
    import graph_align_ref as G
    rng = np.random.default_rng([seed, 7177])
    y = rng.integers(1, V, L)
    for i in range(1, L):
        while y[i] == y[i - 1]:
            y[i] = rng.integers(1, V)
    items = G.around(rng, y, V, **kw) if kind == "around" else G.groups(rng, y, V, **kw)
    tokens, preds, finals = G.build(items)
    return peaked_lp(rng, y, int(1.6 * L) if T is None else T, V), tokens, preds, finals, y


def gap_case(seed=8, L=300, V=12, cuts=(60, 150, 230, 300, 390, 450), gap=12):
    """peaked_case("groups", star=True) with stretches nobody transcribed: `gap` frames peaked on random labels inserted before each
    frame of `cuts`, which an optional wildcard between two groups absorbs when its bias is milder than the misfit
    -> (lp, (tokens, preds, finals))"""
    lp, tokens, preds, finals, _ = peaked_case("groups", seed, L, V, star=True)
    rng = np.random.default_rng([seed, 99])
    parts, prev = [], 0
    for c in cuts:
        lg = rng.standard_normal((gap, V)).astype(np.float32)
        lg[np.arange(gap), rng.integers(1, V, gap)] += np.float32(4.0)
        m = lg.max(1, keepdims=True)
        parts += [lp[prev:c], (lg - m - np.log(np.exp(lg - m).sum(1, keepdims=True, dtype=np.float32))).astype(np.float32)]
        prev = c
    parts.append(lp[prev:])
    return np.ascontiguousarray(np.concatenate(parts)), (tokens, preds, finals)


CUT_W, CUT_SLAB, CUT_LO = 512, 600, 448


def cut_case(seed=3, T=1200, V=8):
    """A window that is JUMPED (lo_force: one launch per slab of CUT_SLAB frames, windows 0 then CUT_LO) so that a predecessor of an
    alive node lies below lo: 447 tokens, then {b | c x 100}, then d, then 400 tokens.  b is node 447, the c branch nodes 448..547 and
    d node 548 with the predecessors [547, 447].  Before the jump d is above the window, after it b is below: the reading through b
    does not exist in this band, and only the overlap [448, 512) of the two windows carries the lattice over the jump.
    -> (lp, (tokens, preds, finals), lo_force, lo_of)"""
    import force_align_ref as R
    import graph_align_ref as G
    cyc = [2, 3, 4]
    items = ([("tok", cyc[k % 3]) for k in range(447)] + [("choice", [[("tok", 5)], [("tok", cyc[k % 3]) for k in range(100)]]), ("tok", 6)] +
             [("tok", cyc[k % 3]) for k in range(400)])
    graph = G.build(items)
    assert len(graph[0]) == 949 and graph[1][548] == [547, 447]
    lp, _, _ = R.make_case(seed, T, V, 5, "random")
    force = [0] + [CUT_LO] * (-(-T // CUT_SLAB) - 1)
    lo_of = np.repeat(np.array(force, np.int32), CUT_SLAB)[:T]
    return lp, graph, force, lo_of
