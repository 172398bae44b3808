"""Test-side reference of CTC alignment over a token graph (csrc/ctc_graph.hip): a numpy restatement of the rules of include/rvb.h, in
fp32, vectorised over the nodes.

States: B_start, and per node j T_j and B_j.  Frame 0: B_start = lp[0][blank], T_j = emission where -1 is a predecessor, the rest -inf.
Frame t: B_start stays; B_j = first max of (B_j, T_j); T_j = first max of (T_j, then per predecessor k in list order B_pk, T_pk), the
T_pk candidate only for a node of another label.  The candidates of all nodes form one padded [N, 1 + 2 D] matrix (padding: -inf) and
np.argmax returns the FIRST maximum.  End: first max over the finals in ascending order of (B_f, T_f).  A wildcard (label W) emits
w[t] + bias, one fp32 addition.  Also here: the graph constructions the CPU and GPU tests share."""
import numpy as np

W = -2                     # RVB_CTC_WILDCARD


def graph_align(lp, tokens, preds, finals, blank=0, w=None, bias=0.0):
    """-> (labels [T] int32, frame_node [T] int32 (-1 on a blank), fp32 score); ValueError when no path has a finite score"""
    lp = np.asarray(lp)
    assert lp.dtype == np.float32 and lp.ndim == 2
    T, _ = lp.shape
    tokens = np.asarray(tokens, np.int64)
    N = len(tokens)
    D = max(len(p) for p in preds)
    ninf = np.float32(-np.inf)
    # X = [B_start, T_0..T_{N-1}, B_0..B_{N-1}, -inf]
    SENT = 2 * N + 1
    idx = np.full((N, 1 + 2 * D), SENT, np.int64)
    idx[:, 0] = 1 + np.arange(N)
    from_start = np.zeros(N, bool)
    for j, ps in enumerate(preds):
        assert len(ps) >= 1 and len(set(ps)) == len(ps) and all(-1 <= p < j for p in ps)
        for k, p in enumerate(ps):
            if p < 0:
                idx[j, 1 + 2 * k] = 0
                from_start[j] = True
            else:
                idx[j, 1 + 2 * k] = 1 + N + p
                if tokens[p] != tokens[j]:
                    idx[j, 2 + 2 * k] = 1 + p
    wild = tokens == W
    cols = np.where(wild, blank, tokens)
    if wild.any():
        ew = (np.asarray(w, np.float32) + np.float32(bias)).astype(np.float32)

    def emission(t):
        e = lp[t, cols].copy()
        if wild.any():
            e[wild] = ew[t]
        return e

    X = np.full(2 * N + 2, ninf, np.float32)
    X[0] = lp[0, blank]
    X[1:1 + N][from_start] = emission(0)[from_start]
    bpT = np.zeros((T, N), np.uint8)
    bpB = np.zeros((T, N), bool)
    rows = np.arange(N)
    for t in range(1, T):
        cand = X[idx]
        arg = np.argmax(cand, axis=1)
        bpT[t] = arg
        Tn = cand[rows, arg] + emission(t)
        Tp, Bp = X[1:1 + N], X[1 + N:1 + 2 * N]
        bpB[t] = Tp > Bp
        Bn = np.where(bpB[t], Tp, Bp) + lp[t, blank]
        X[0] = X[0] + lp[t, blank]
        X[1:1 + N] = Tn
        X[1 + N:1 + 2 * N] = Bn
        assert X.dtype == np.float32
    best, node, tok_state = ninf, -1, False
    for f in np.nonzero(np.asarray(finals, bool))[0]:
        if X[1 + N + f] > best:
            best, node, tok_state = X[1 + N + f], int(f), False
        if X[1 + f] > best:
            best, node, tok_state = X[1 + f], int(f), True
    if not best > ninf:
        raise ValueError("infeasible: no path with a finite score")
    labels, fnode = np.empty(T, np.int32), np.empty(T, np.int32)
    for t in range(T - 1, -1, -1):
        labels[t] = tokens[node] if tok_state else blank
        fnode[t] = node if tok_state else -1
        if t == 0 or node < 0:
            continue
        if tok_state:
            c = int(bpT[t, node])
            if c:
                p = preds[node][(c - 1) // 2]
                node, tok_state = p, (c - 1) % 2 == 1
        else:
            tok_state = bool(bpB[t, node])
    return labels, fnode, np.float32(best)


def graph_align_bytes(lp, tokens, preds, finals, blank=0, w=None, bias=0.0):
    """The same alignment by the kernel's back-pointer scheme, node by node: ONE byte per node and frame, bits 0-6 = the winning
    predecessor's index + 1 (0 = stay) where a predecessor's candidate is the better of (B_p, T_p), B_p on a tie; bit 7 = B_j came
    from T_j.  Whether predecessor p gave B_p or T_p is not stored: the back-trace reads bit 7 of p's own byte of the same frame.
    -> (labels, frame_node, score) as graph_align."""
    lp = np.asarray(lp)
    T, N = len(lp), len(tokens)
    ninf = np.float32(-np.inf)
    arcs = [[(p + 1, p >= 0 and tokens[p] != tokens[j]) for p in preds[j]] for j in range(N)]

    def emission(t, j):
        return np.float32(w[t]) + np.float32(bias) if tokens[j] == W else lp[t, tokens[j]]

    pT, pB = np.full(N + 1, ninf, np.float32), np.full(N + 1, ninf, np.float32)       # slot 0 = start, slot j + 1 = node j
    pB[0] = lp[0, blank]
    for j in range(N):
        if any(s == 0 for s, _ in arcs[j]):
            pT[j + 1] = emission(0, j)
    bp = np.zeros((T, N), np.uint8)
    for t in range(1, T):
        nT, nB = pT.copy(), pB.copy()
        for j in range(N):
            best, code = pT[j + 1], 0
            for a, (s, allow) in enumerate(arcs[j]):
                c = pT[s] if (allow and pT[s] > pB[s]) else pB[s]
                if c > best:
                    best, code = c, 1 + a
            from_t = pT[j + 1] > pB[j + 1]
            nB[j + 1] = (pT[j + 1] if from_t else pB[j + 1]) + lp[t, blank]
            nT[j + 1] = best + emission(t, j)
            bp[t, j] = code | (0x80 if from_t else 0)
        nB[0] = pB[0] + lp[t, blank]
        pT, pB = nT, nB
    best, st = ninf, None
    for f in np.nonzero(np.asarray(finals, bool))[0]:
        if pB[f + 1] > best:
            best, st = pB[f + 1], 2 * (int(f) + 1)
        if pT[f + 1] > best:
            best, st = pT[f + 1], 2 * (int(f) + 1) + 1
    if st is None:
        raise ValueError("infeasible: no path with a finite score")
    states = np.zeros(T, np.int64)
    for t in range(T - 1, 0, -1):
        states[t] = st
        slot = st >> 1
        if slot == 0:
            continue
        byte = int(bp[t, slot - 1])
        if st & 1:
            code = byte & 0x7f
            if code:
                s, allow = arcs[slot - 1][code - 1]
                st = 2 * s + (int(bp[t, s - 1]) >> 7 if allow else 0)
        else:
            st = 2 * slot + (byte >> 7)
    states[0] = st
    labels = np.array([tokens[(s >> 1) - 1] if s & 1 else blank for s in states], np.int32)
    fnode = np.array([(s >> 1) - 1 if s & 1 else -1 for s in states], np.int32)
    return labels, fnode, np.float32(best)


def chain(y):
    n = len(y)
    return list(y), [[j - 1] for j in range(n)], [j == n - 1 for j in range(n)]


def build(items):
    """items: a sequence of ("tok", id) and ("choice", [sequence, ...]) (an empty sequence = optional) -> (tokens, preds, finals), the
    construction of reverb_amd.token_graph: nodes left to right, a node's predecessors = its entry set, nearest first, -1 last"""
    tokens, preds = [], []

    def go(seq, entry):
        for kind, v in seq:
            if kind == "tok":
                tokens.append(int(v))
                preds.append(sorted(entry, reverse=True))
                entry = [len(tokens) - 1]
            else:
                exits = []
                for br in v:
                    for x in go(br, entry):
                        if x not in exits:
                            exits.append(x)
                entry = exits
        return entry

    exits = go(items, [-1])
    return tokens, preds, [j in exits for j in range(len(tokens))]


def paths(preds, finals):
    """every path (list of nodes) from a start predecessor to a final node"""
    N = len(preds)
    succ = [[] for _ in range(N)]
    for j, ps in enumerate(preds):
        for p in ps:
            if p >= 0:
                succ[p].append(j)
    out = []

    def walk(j, acc):
        acc = acc + [j]
        if finals[j]:
            out.append(acc)
        for s in succ[j]:
            walk(s, acc)

    for j, ps in enumerate(preds):
        if -1 in ps:
            walk(j, [])
    return out


def around(rng, y, V, p_choice=0.5, p_filler=0.2, p_star=0.0, max_branch=3, n_alt=3):
    """a random expression one reading of which is y: some tokens stand alone, some runs of y are one branch of a choice among random
    other branches, optional fillers and (p_star) optional wildcards stand between them"""
    items, i = [], 0
    while i < len(y):
        if rng.random() < p_star:
            items.append(("choice", [[("tok", W)], []]))
        if rng.random() < p_filler:
            items.append(("choice", [[("tok", int(t)) for t in rng.integers(1, V, rng.integers(1, max_branch + 1))], []]))
        if rng.random() < p_choice:
            n = int(min(rng.integers(1, max_branch + 1), len(y) - i))
            branches = [[("tok", int(t)) for t in rng.integers(1, V, rng.integers(1, max_branch + 1))] for _ in range(rng.integers(1, n_alt + 1))]
            branches.insert(int(rng.integers(0, len(branches) + 1)), [("tok", int(t)) for t in y[i:i + n]])
            items.append(("choice", branches))
            i += n
        else:
            items.append(("tok", int(y[i])))
            i += 1
    return items


def groups(rng, y, V, n_alt=4, star=False):
    """len(y) groups of n_alt single-node alternatives, one of them y[g] at a random place; star: an optional wildcard before every
    group but the first"""
    items = []
    for g, t in enumerate(y):
        if star and g:
            items.append(("choice", [[("tok", W)], []]))
        alts = [int(a) for a in rng.integers(1, V, n_alt)]
        alts[int(rng.integers(0, n_alt))] = int(t)
        items.append(("choice", [[("tok", a)] for a in alts]))
    return items
