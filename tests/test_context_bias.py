"""Hot-word context biasing on the host (no GPU): the native ContextGraph and the biased prefix beam search of csrc/search.cpp behind
the lab hooks rvb_test_context_walk / rvb_test_prefix_beam_context, the plain-Python statement tests/context_bias_ref.py, and the
Python surface (reverb_amd/context_graph.py), all against tests/golden/context_bias.json -- written by the unmodified reference
(scripts/gen_golden_context_bias.py)."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import context_bias_ref as R  # noqa: E402
from reverb_amd import _lib  # noqa: E402
from reverb_amd._lib import dptr, fptr, iptr  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "context_bias.json")) as _f:
    G = json.load(_f)
PLAIN = {(p["lat"], p["beam"]): p for p in G["plain"]}


def flat(phrases):
    lens = np.array([len(p) for p in phrases], np.int32)
    toks = np.array([t for p in phrases for t in p] + [0], np.int32)        # + [0]: never a zero-size buffer
    return toks, lens


def lattice(name):
    L = G["lattices"][name]
    lp = R.make_lattice(L["seed"], L["T"], L["V"], L["kind"])
    assert R.digest(lp) == L["digest"], "the seeded lattice is not the one the golden was computed on"
    return lp, L


def native_walk(phrases, score, stream, vocab=64, blank=0):
    lib = _lib.load_test()
    toks, lens = flat(phrases)
    st = np.array(list(stream) + [0], np.int32)
    n = len(stream)
    nodes = C.c_int32(-1)
    sc, nd, fin = np.zeros(n + 1, np.float64), np.zeros(n + 1, np.int32), np.zeros(n + 1, np.float64)
    _lib.check(lib.rvb_test_context_walk(iptr(toks), iptr(lens), len(phrases), score, vocab, blank, iptr(st), n, C.byref(nodes), dptr(sc),
                                         iptr(nd), dptr(fin)), "rvb_test_context_walk")
    return nodes.value, [[sc[i], int(nd[i]), fin[i]] for i in range(n)]


def native_search(tv, ti, T, beam, phrases, score, vocab=64, blank=0):
    """phrases None: no graph at all; []: a graph of the root alone"""
    lib = _lib.load_test()
    tv = np.ascontiguousarray(tv, np.float32); ti = np.ascontiguousarray(ti, np.int32)
    toks, lens = flat(phrases or [])
    ml = max(T, 1)
    n = np.zeros(1, np.int32); tok = np.full((beam, ml), -1, np.int32); ln = np.zeros(beam, np.int32)
    tim = np.full((beam, ml), -1, np.int32); tl = np.zeros(beam, np.int32); sc = np.zeros(beam, np.float64); cx = np.zeros(beam, np.float64)
    _lib.check(lib.rvb_test_prefix_beam_context(fptr(tv), iptr(ti), T, beam, blank, vocab, iptr(toks), iptr(lens),
                                                -1 if phrases is None else len(phrases), score, iptr(n), iptr(tok), iptr(ln), iptr(tim),
                                                iptr(tl), dptr(sc), dptr(cx)), "rvb_test_prefix_beam_context")
    k = int(n[0])
    return {"nbest": [tok[i, :ln[i]].tolist() for i in range(k)], "scores": sc[:k].tolist(),
            "times": [tim[i, :tl[i]].tolist() for i in range(k)], "context": cx[:k].tolist()}


# ------------------------------------------------------------------------------------------------ the graph
def test_walk_sets_cover_what_the_issue_lists():
    """shared prefixes, a suffix of another phrase, a prefix of another (earlier and later), repeated tokens, single tokens, a
    duplicate, an empty phrase -- and the golden walks use these sets"""
    m = R.WALK_SETS["mixed"]
    assert [1, 2, 3] in m and [1, 2, 4] in m                                   # shared prefix
    assert [2, 3] in m and m.index([1, 2]) > m.index([1, 2, 3]) and m.index([4]) < m.index([4, 4, 2])
    assert m.count([2, 3]) == 2 and [] in m and [5] in m and [3, 3, 3] in m
    assert {w["set"] for w in G["walks"]} == set(R.WALK_SETS)


@pytest.mark.parametrize("i", range(len(G["walks"])))
def test_native_graph_walk_equals_the_reference_step_for_step(i):
    w = G["walks"][i]
    nodes, steps = native_walk(R.WALK_SETS[w["set"]], w["c"], R.stream(w["seed"], w["n"], w["V"]))
    assert nodes == w["nodes"]
    assert len(steps) == len(w["steps"]) == w["n"]
    for got, want in zip(steps, w["steps"]):
        assert got[0] == want[0] and got[1] == want[1] and got[2] == want[2], (got, want)      # float64 ==, node ids equal


@pytest.mark.parametrize("i", range(len(G["walks"])))
def test_restated_graph_walk_equals_the_reference(i):
    w = G["walks"][i]
    g = R.Graph(R.WALK_SETS[w["set"]], w["c"])
    assert g.num_nodes == w["nodes"]
    state = 0
    for tok, want in zip(R.stream(w["seed"], w["n"], w["V"]), w["steps"]):
        sc, state = g.step(state, tok)
        assert [sc, state, g.finalize(state)[0]] == want


def test_graph_walk_from_a_random_graph_native_equals_restatement():
    """beyond the goldens: random phrase sets over a tiny alphabet (dense overlaps), native vs restatement, exact"""
    rng = np.random.default_rng(7)
    for trial in range(60):
        V = int(rng.integers(3, 7))
        phrases = [rng.integers(1, V, int(rng.integers(0, 5))).tolist() for _ in range(int(rng.integers(1, 9)))]
        score = [6.0, 0.1, 2.5, -1.5][trial % 4]
        toks = rng.integers(1, V, 50).tolist()
        g = R.Graph(phrases, score)
        nodes, steps = native_walk(phrases, score, toks)
        assert nodes == g.num_nodes
        state = 0
        for tok, got in zip(toks, steps):
            sc, state = g.step(state, tok)
            assert got == [sc, state, g.finalize(state)[0]], (trial, phrases)


# ------------------------------------------------------------------------------------------------ the search
def _check_against_golden(got, want):
    assert got["nbest"] == want["nbest"]
    assert got["times"] == want["times"]
    # as tests/test_search_native.py compares the unbiased search with the reference's goldens
    assert got["scores"] == pytest.approx(want["scores"], rel=0, abs=1e-9)


def test_search_cases_cover_what_the_issue_lists():
    beams = {s["beam"] for s in G["searches"]}
    scores = {s["c"] for s in G["searches"]}
    assert beams == {1, 3, 10} and scores == {0.0, 3.0, 6.0}
    assert any(G["lattices"][s["lat"]]["T"] == 1 for s in G["searches"]) and any(G["lattices"][s["lat"]]["kind"] == "blank" for s in G["searches"])
    six = [s for s in G["searches"] if s["c"] == 6.0 and s["beam"] >= 3]
    moved = [s for s in six if s["biased"]["nbest"][0] != PLAIN[(s["lat"], s["beam"])]["nbest"][0]]
    assert len(six) >= 4 and 2 * len(moved) >= len(six)


@pytest.mark.parametrize("i", range(len(G["searches"])))
def test_native_biased_search_equals_the_reference(i):
    s = G["searches"][i]
    lp, L = lattice(s["lat"])
    tv, ti = R.topk(lp, s["beam"])
    got = native_search(tv, ti, L["T"], s["beam"], L["phrases"], s["c"])
    _check_against_golden(got, s["biased"])
    # the context score a hypothesis ends with is finalize's: minus the node score of the state it stopped in, a multiple of c
    assert all(c <= 0 and (s["c"] == 0 or (c / s["c"]) == round(c / s["c"])) for c in got["context"])
    _check_against_golden(native_search(tv, ti, L["T"], s["beam"], None, 0.0), PLAIN[(s["lat"], s["beam"])])


@pytest.mark.parametrize("i", range(len(G["searches"])))
def test_restated_search_equals_the_reference_and_the_native_search_bit_for_bit(i):
    s = G["searches"][i]
    lp, L = lattice(s["lat"])
    tv, ti = R.topk(lp, s["beam"])
    ref = R.search(tv, ti, L["T"], s["beam"], 0, R.Graph(L["phrases"], s["c"]))
    _check_against_golden(ref, s["biased"])
    _check_against_golden(R.search(tv, ti, L["T"], s["beam"], 0, None), PLAIN[(s["lat"], s["beam"])])
    got = native_search(tv, ti, L["T"], s["beam"], L["phrases"], s["c"])
    assert got["nbest"] == ref["nbest"] and got["times"] == ref["times"]
    assert got["scores"] == ref["scores"] and got["context"] == ref["context"]                  # float64, same order of operations


def test_random_biased_searches_native_equals_restatement_bit_for_bit():
    """wider than the goldens: longer lattices, quantised log-probs (exact ties in the pruning: the stable order decides), beams
    wider than the vocabulary allows new prefixes for, negative and fractional bonuses"""
    rng = np.random.default_rng(3)
    for trial in range(60):
        V, T = int(rng.integers(3, 9)), int(rng.integers(1, 40))
        beam = min(int(rng.integers(1, 7)), V)
        lp = R.make_lattice(1000 + trial, T, V, "blank" if trial % 11 == 0 else "random")
        if trial % 3 == 0:
            lp = (np.round(lp * 2) / 2).astype(np.float32)
        tv, ti = R.topk(lp, beam)
        phrases = [rng.integers(1, V, int(rng.integers(0, 4))).tolist() for _ in range(int(rng.integers(0, 6)))]
        score = [6.0, 3.0, 0.3, -2.0, 0.0][trial % 5]
        n_t = T - (trial % 3 if T > 3 else 0)
        ref = R.search(tv, ti, n_t, beam, 0, R.Graph(phrases, score))
        got = native_search(tv, ti, n_t, beam, phrases, score)
        assert got == ref, (trial, phrases, score)


def _existing_topk_cases():
    from golden_util import CASES, Case
    for name in CASES:
        case = Case(name)
        for b in range(len(case.golden("ctc_prefix_beam_search"))):
            T = int(case.js["encoder_lens"][b])
            yield name, b, case.arrays["topk_val"][b], case.arrays["topk_idx"][b], T, case.beam, case.golden("ctc_prefix_beam_search")[b]


def test_zero_score_graph_empty_graph_and_no_graph_are_bit_identical_on_the_existing_goldens():
    lib = _lib.load_test()
    checked = 0
    for name, b, tv, ti, T, beam, g in _existing_topk_cases():
        tv = np.ascontiguousarray(tv, np.float32); ti = np.ascontiguousarray(ti, np.int32)
        none = native_search(tv, ti, T, beam, None, 0.0, vocab=1 << 20)
        # the hook the existing tests use (prefix_beam_search without the graph argument)
        ml = max(T, 1)
        n = np.zeros(1, np.int32); tok = np.full((beam, ml), -1, np.int32); ln = np.zeros(beam, np.int32)
        tim = np.full((beam, ml), -1, np.int32); tl = np.zeros(beam, np.int32); sc = np.zeros(beam, np.float64)
        _lib.check(lib.rvb_test_prefix_beam(fptr(tv), iptr(ti), T, beam, 0, iptr(n), iptr(tok), iptr(ln), iptr(tim), iptr(tl), dptr(sc)))
        k = int(n[0])
        assert none["nbest"] == [tok[i, :ln[i]].tolist() for i in range(k)] == g["nbest"]
        assert np.array(none["scores"]).tobytes() == sc[:k].tobytes()
        # phrases taken from the case's own hypotheses, so that the zero-score graph does leave its root
        phrases = [h[:2] for h in g["nbest"] if len(h) >= 2][:3] + [h[-1:] for h in g["nbest"] if h][:2]
        for label, ph, score in (("empty graph", [], 6.0), ("zero score", phrases, 0.0)):
            got = native_search(tv, ti, T, beam, ph, score, vocab=1 << 20)
            assert got["nbest"] == none["nbest"] and got["times"] == none["times"], (name, b, label)
            assert np.array(got["scores"]).tobytes() == np.array(none["scores"]).tobytes(), (name, b, label)
        checked += 1
    assert checked >= 8


# ------------------------------------------------------------------------------------------------ argument checks
def test_phrases_are_checked_by_name_before_any_device_is_looked_for():
    """rvb_set_context_graph's checks (ContextGraph::check), reached through the lab hooks: an engine cannot be created without a
    device, and these must not need one."""
    lib = _lib.load_test()
    tv, ti = np.zeros((2, 2), np.float32), np.zeros((2, 2), np.int32)
    n = np.zeros(1, np.int32)

    def search(toks, lens, n_phrases, vocab=10, blank=0):
        return lib.rvb_test_prefix_beam_context(fptr(tv), iptr(ti), 2, 2, blank, vocab, toks, lens, n_phrases, 6.0, iptr(n), None, None, None,
                                                None, None, None)
    t = np.array([1, 2, 0, 3], np.int32); ln = np.array([2, 2], np.int32)
    assert search(iptr(t), iptr(ln), 2) == -1 and b"phrase 1 position 0" in lib.rvb_last_error() and b"blank" in lib.rvb_last_error()
    assert search(iptr(t), iptr(ln), 2, blank=9) == 0                                   # the same ids with another blank are fine
    t = np.array([1, 2, 3, 10], np.int32)
    assert search(iptr(t), iptr(ln), 2) == -1 and b"phrase 1 position 1" in lib.rvb_last_error() and b"outside [0, 10)" in lib.rvb_last_error()
    t = np.array([1, -1, 3, 4], np.int32)
    assert search(iptr(t), iptr(ln), 2) == -1 and b"phrase 0 position 1" in lib.rvb_last_error()
    t = np.array([1, 2, 3, 4], np.int32); bad = np.array([2, -2], np.int32)
    assert search(iptr(t), iptr(bad), 2) == -1 and b"negative length" in lib.rvb_last_error()
    assert search(iptr(t), None, 2) == -1 and search(None, iptr(ln), 2) == -1           # null pointers
    assert search(None, iptr(np.zeros(2, np.int32)), 2) == 0                            # ... unless every phrase is empty
    assert lib.rvb_test_context_walk(iptr(t), iptr(bad), 2, 6.0, 10, 0, None, 0, None, None, None, None) == -1
    assert lib.rvb_test_context_walk(iptr(t), iptr(ln), 2, 6.0, 10, 0, None, 3, None, None, None, None) == -1       # steps without a stream
    # the product entry point refuses a null engine before it reads anything
    prod = _lib.load()
    assert prod.rvb_set_context_graph(None, iptr(t), iptr(ln), 2, 6.0) == -1 and b"null engine" in prod.rvb_last_error()


# ------------------------------------------------------------------------------------------------ Python surface
def test_tokenize_and_graph_construction_equal_the_reference(tmp_path):
    from reverb_amd.context_graph import ContextGraph, tokenize
    import wenet.utils.context_graph as W
    assert W.ContextGraph is ContextGraph and W.tokenize is tokenize
    tk = G["tokenize"]
    path = tmp_path / "hot.txt"
    path.write_text("\n".join(tk["lines"]) + "\n", encoding="utf8")
    assert tokenize(str(path), tk["table"]) == tk["ids"]
    assert tokenize(str(path), {k: v for k, v in tk["table"].items() if k != "<unk>"}) == tk["ids_no_unk"]
    assert [] in tk["ids"]                                                               # the empty line is an empty phrase
    g = ContextGraph(str(path), tk["table"], context_score=3.0)
    h = ContextGraph.from_token_ids(tk["ids"], 3.0)
    assert g.context_list == h.context_list == tk["ids"] and g.context_score == h.context_score == 3.0
    assert g.num_nodes == h.num_nodes == R.Graph(tk["ids"], 3.0).num_nodes
    assert ContextGraph(str(path), tk["table"]).context_score == 6.0
    for a, b in zip(g.flat(), h.flat()):
        assert a.dtype == np.int32 and a.tobytes() == b.tobytes()
    # both build the same native graph
    st = R.stream(9, 40, 7)
    assert native_walk(g.context_list, g.context_score, st) == native_walk(h.context_list, h.context_score, st)
    assert native_walk(g.context_list, 3.0, st)[0] == g.num_nodes


def test_tokenize_with_a_bpe_model_path_uses_the_tokenizer(tmp_path):
    """no sentencepiece file at the path: RevBpeTokenizer.text2tokens cuts by longest match against the unit table"""
    from reverb_amd.context_graph import tokenize
    table = {"<blank>": 0, "<unk>": 1, "▁ab": 2, "c": 3, "▁c": 4, "ab": 5}
    path = tmp_path / "hot.txt"
    path.write_text("abc c\n\nabab\n", encoding="utf8")
    assert tokenize(str(path), table, bpe_model=str(tmp_path / "missing.model")) == [[2, 3, 3], [], [2, 5]]      # a word the table has whole ("c") is taken whole


def test_num_nodes_counts_like_the_reference():
    from reverb_amd.context_graph import ContextGraph
    for w in G["walks"]:
        assert ContextGraph.from_token_ids(R.WALK_SETS[w["set"]], w["c"]).num_nodes == w["nodes"]
