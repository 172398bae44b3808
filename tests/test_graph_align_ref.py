"""The numpy restatement of the graph aligner (tests/graph_align_ref.py) against force_align, and the parser of reverb_amd.token_graph.
No tolerance anywhere: labels are equal and scores have equal bits."""
import numpy as np
import pytest

import force_align_ref as R
import graph_align_ref as G
from reverb_amd import token_graph as TG
from reverb_amd.token_graph import TokenGraph, parse_alternatives

W = G.W
KINDS = ("random", "quant", "repeat", "neginf", "min_t_quant")


def bits(x):
    return np.float32(x).tobytes()


def chain_truth(lp, w, bias, y):
    """force_align on [lp | w + bias] with the wildcard as label V (the construction of tests/test_force_align_wild_gpu.py)"""
    V = lp.shape[1]
    ext = np.ascontiguousarray(np.concatenate([lp, (w + np.float32(bias)).astype(np.float32)[:, None]], axis=1))
    labels, score = R.force_align(ext, np.where(np.asarray(y) == W, V, y))
    return np.where(labels == V, W, labels).astype(np.int32), score


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("T,L", [(1, 1), (7, 2), (60, 17), (300, 120)])
def test_on_a_chain_it_is_force_align(kind, T, L):
    lp, y, T = R.make_case(40 + T + L, T, 24, L, kind)
    labels, fnode, score = G.graph_align(lp, *G.chain(y))
    want, ws = R.force_align(lp, y)
    assert labels.tolist() == want.tolist() and bits(score) == bits(ws)
    assert R.collapse(labels).tolist() == list(y) and np.all((fnode >= 0) == (labels != 0))
    # wildcards at every fifth token and at an adjacent pair; on min_t the pair needs one more frame than there is
    yw = np.array(y, np.int32)
    yw[::5] = W
    if L >= 2 and not kind.startswith("min_t"):
        yw[L // 2 - 1:L // 2 + 1] = W
    if T < R.min_frames(yw):
        return
    w = lp.max(axis=1)
    for bias in (0.0, -0.75):
        labels, _, score = G.graph_align(lp, *G.chain(yw), w=w, bias=bias)
        want, ws = chain_truth(lp, w, bias, yw)
        assert labels.tolist() == want.tolist() and bits(score) == bits(ws)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("seed", range(6))
def test_a_small_graph_scores_as_its_best_path(kind, seed):
    rng = np.random.default_rng([seed, 77])
    V = 12
    for _ in range(50):
        L = int(rng.integers(1, 6))
        lp, y, T = R.make_case(1000 * seed + L, int(rng.integers(L + 4, 30)), V, L, kind)
        tokens, preds, finals = G.build(G.around(rng, y, V, p_choice=0.6, p_filler=0.3, max_branch=2, n_alt=2))
        all_paths = G.paths(preds, finals)
        if len(tokens) <= 12 and len(all_paths) <= 64:
            break
    else:
        pytest.fail("no small graph drawn")
    assert len(all_paths) >= 2 or len(tokens) == L
    best = None
    for p in all_paths:
        try:
            labels, score = R.force_align(lp, [tokens[j] for j in p])
        except ValueError:                                   # this reading does not fit into T frames
            continue
        if best is None or score > best[1]:
            best = (labels, score, p)
    assert best is not None
    labels, fnode, score = G.graph_align(lp, tokens, preds, finals)
    assert bits(score) == bits(best[1])
    if kind == "random":
        assert labels.tolist() == best[0].tolist()
        keep = np.ones(len(fnode), bool); keep[1:] = fnode[1:] != fnode[:-1]
        assert [int(j) for j in fnode[keep] if j >= 0] == best[2]


@pytest.mark.parametrize("kind", ["quant", "random", "min_t_quant", "neginf"])
def test_the_one_byte_back_pointer_decodes_to_the_same_path(kind):
    """csrc/ctc_graph.hip stores the winning predecessor's index and reads whether it gave its blank or its token from that
    predecessor's own blank bit; restated node by node (graph_align_bytes) it gives the path of the candidate-by-candidate rules,
    ties (quantised log-probs), wildcards and both biases included"""
    n = 0
    for seed in range(30):
        rng = np.random.default_rng([seed, KINDS.index(kind)])
        L = int(rng.integers(1, 7))
        lp, y, T = R.make_case(seed, int(rng.integers(L + 3, 26)), 6, L, kind)
        g = G.build(G.around(rng, y, 6, p_choice=0.6, p_filler=0.4, p_star=0.3, max_branch=2, n_alt=2))
        w = lp.max(axis=1)
        for bias in (0.0, -0.75):
            try:
                want = G.graph_align(lp, *g, w=w, bias=bias)
            except ValueError:
                with pytest.raises(ValueError):
                    G.graph_align_bytes(lp, *g, w=w, bias=bias)
                continue
            got = G.graph_align_bytes(lp, *g, w=w, bias=bias)
            assert got[0].tolist() == want[0].tolist() and got[1].tolist() == want[1].tolist() and bits(got[2]) == bits(want[2])
            n += 1
    assert n >= 30


def test_the_python_caps_are_the_librarys():
    from reverb_amd import _lib
    out = [np.zeros(1, np.int32) for _ in range(4)]
    assert _lib.load().rvb_ctc_align_graph_limits(*[_lib.iptr(o) for o in out]) == 0
    assert [int(o[0]) for o in out][:3] == [TG.MAX_NODES, TG.MAX_IN_DEGREE, TG.MAX_ARCS]


def test_an_infeasible_graph_is_refused():
    lp, y, _ = R.make_case(3, 4, 8, 3, "random")
    with pytest.raises(ValueError, match="infeasible"):
        G.graph_align(lp[:2], *G.chain(y))


# ---------------------------------------------------------------- the parser
def tok(text):
    """one id per letter, words ignored: a = 1, b = 2, ..."""
    return [ord(c) - 96 for c in text if c != " "]


def graph(text, **kw):
    g = parse_alternatives(text, tok, **kw)
    return g.tokens, g.preds, [j for j, f in enumerate(g.finals) if f]


def test_plain_text_is_a_chain():
    g = parse_alternatives("ab c", tok)
    c = TokenGraph.chain([1, 2, 3])
    assert (g.tokens, g.preds, g.finals) == (c.tokens, c.preds, c.finals) == ([1, 2, 3], [[-1], [0], [1]], [False, False, True])
    assert g.words == ["ab c", "", ""] and g.text_of([0, 1, 2]) == "ab c"


def test_choice_optional_and_nesting():
    assert graph("a {b|c d} e") == ([1, 2, 3, 4, 5], [[-1], [0], [0], [2], [3, 1]], [4])
    assert graph("a [b] c") == graph("a {b|} c") == ([1, 2, 3], [[-1], [0], [1, 0]], [2])
    assert graph("a {b|c|} d") == ([1, 2, 3, 4], [[-1], [0], [0], [2, 1, 0]], [3])
    # nesting: a then (b then optional c, or d) then e
    assert graph("a {b [c]|d} e") == ([1, 2, 3, 4, 5], [[-1], [0], [1], [0], [3, 2, 1]], [4])
    assert graph("[a|b] c") == ([1, 2, 3], [[-1], [-1], [1, 0, -1]], [2])


def test_leading_and_trailing_optionals_give_start_predecessors_and_several_finals():
    assert graph("[a] b [c]") == ([1, 2, 3], [[-1], [0, -1], [1]], [1, 2])
    assert graph("[a] [b]") == ([1, 2], [[-1], [0, -1]], [0, 1])             # the empty path is not a reading
    assert graph("{a|b}") == ([1, 2], [[-1], [-1]], [0, 1])


def test_escapes_and_the_wildcard_word():
    g = parse_alternatives(r"a\{b \| \\", lambda s: [ord(c) for c in s if c != " "])
    assert g.tokens == [ord(c) for c in "a{b|\\"]
    g = parse_alternatives("a <star> b [<star>] c", tok, wildcard="<star>")
    assert g.tokens == [1, W, 2, W, 3] and g.preds == [[-1], [0], [1], [2], [3, 2]]
    assert g.words == ["a", "<star>", "b", "<star>", "c"] and g.text_of([0, 1, 2, 4]) == "a <star> b c"
    assert parse_alternatives("a <star> b", lambda s: [7] * len(s.split())).tokens == [7, 7, 7]     # no marker given: a word


@pytest.mark.parametrize("text,word", [("walk{s|ed}", "inside the word"), ("{a|b}c", "inside the word"), ("a [b", "unbalanced"),
                                       ("a } b", "unbalanced"), ("{a|b] c", "unbalanced"), ("a ] b", "unbalanced"), ("a | b", "unbalanced"),
                                       ("{|}", "empty"), ("", "empty"), ("[ ]", "empty"), ("a\\b", "backslash"), ("a\\", "backslash")])
def test_what_the_parser_refuses(text, word):
    with pytest.raises(ValueError, match=word):
        parse_alternatives(text, tok)


def test_caps_are_refused_by_name():
    with pytest.raises(ValueError, match="RVB_CTC_GRAPH_MAX_NODES"):
        parse_alternatives("a" * (TG.MAX_NODES + 1), tok)
    assert len(parse_alternatives("a" * TG.MAX_NODES, tok)) == TG.MAX_NODES
    many = "{" + "|".join("a" * 1 for _ in range(TG.MAX_IN_DEGREE + 1)) + "} b"
    with pytest.raises(ValueError, match="RVB_CTC_GRAPH_MAX_IN_DEGREE"):
        parse_alternatives(many, tok)
    ok = "{" + "|".join("a" for _ in range(TG.MAX_IN_DEGREE)) + "} b"
    assert len(parse_alternatives(ok, tok).preds[-1]) == TG.MAX_IN_DEGREE
    with pytest.raises(ValueError, match="RVB_CTC_GRAPH_MAX_ARCS"):
        parse_alternatives(" ".join([ok[:-2]] * 10), tok)          # 9 x 64 x 64 arcs between ten groups of 64
    with pytest.raises(ValueError, match="RVB_CTC_GRAPH_MAX_IN_DEGREE"):
        TokenGraph([1] * 66, [[-1]] * 65 + [list(range(65))], [False] * 65 + [True])
    for bad in (([], [], []), ([1], [[]], [True]), ([1, 2], [[-1], [0, 0]], [False, True]), ([1, 2], [[-1], [1]], [False, True]),
                ([1], [[-1]], [False]), ([1, 2], [[-1], [-2]], [False, True])):
        with pytest.raises(ValueError):
            TokenGraph(*bad)
