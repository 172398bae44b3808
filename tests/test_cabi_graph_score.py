"""rvb_ctc_score_graph and its lab hook check their arguments before any device work: these hold with and without a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from reverb_amd import _lib

W = -2
ARG, UNSUPPORTED = -1, -5


@pytest.fixture(scope="module")
def tlib():
    return _lib.load_test()


def test_the_header_declares_it_and_the_product_exports_it():
    text = open(os.path.join(ROOT, "include", "rvb.h")).read()
    decl = re.search(r"int rvb_ctc_score_graph\(([^;]*)\);", text)
    assert decl and len(decl.group(1).split(",")) == 15 == len(_lib.SIGNATURES["rvb_ctc_score_graph"][1])
    assert "rvb_ctc_score_graph" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "log 2" in text[text.index("rvb_ctc_score for a transcript with ALTERNATIVES"):decl.start()]      # duplicates count twice: said so
    lib = C.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "rvb_ctc_score_graph")
    assert not hasattr(lib, "rvb_test_ctc_score_graph")               # the hook is not part of the product
    assert hasattr(_lib.load_test(), "rvb_test_ctc_score_graph")
    hook = re.search(r"int rvb_test_ctc_score_graph\(([^;]*)\);", open(os.path.join(ROOT, "reverb_amd", "csrc", "test_api.h")).read())
    assert hook and len(hook.group(1).split(",")) == 17 == len(_lib.TEST_SIGNATURES["rvb_test_ctc_score_graph"][1])


def test_null_engine_is_reported():
    lib = _lib.load()
    one, u, d = np.ones(1, np.int32), np.ones(1, np.uint8), np.zeros(1, np.float64)
    ip = _lib.iptr
    assert lib.rvb_ctc_score_graph(None, ip(one), ip(one), ip(one), ip(one), _lib.u8ptr(u), 1, ip(one), ip(one), _lib.dptr(d), None, None, None,
                                   None, None) == ARG
    assert b"rvb_ctc_score_graph: null engine" in lib.rvb_last_error()


def _hook(lib, graphs, T=(20,), V=8, blank=0, slab=64, post=True, n_seq=None):
    """graphs: [(tokens, preds, finals)] -> (rc, message); asserts that a refusal wrote nothing"""
    rng = np.random.default_rng(0)
    M = max(int(sum(max(t, 0) for t in T)), 1)
    lp = np.log(rng.dirichlet(np.ones(V), size=M)).astype(np.float32)
    tok = np.ascontiguousarray(np.concatenate([np.asarray(g[0], np.int32) for g in graphs] + [np.zeros(1, np.int32)]), np.int32)
    nn = np.array([len(g[0]) for g in graphs], np.int32)
    off = np.concatenate([np.concatenate([[0], np.cumsum([len(p) for p in g[1]])]) for g in graphs]).astype(np.int32)
    prd = np.array([p for g in graphs for ps in g[1] for p in ps] + [0], np.int32)
    fin = np.concatenate([np.asarray(g[2], np.uint8) for g in graphs] + [np.zeros(1, np.uint8)])
    Ts = np.asarray(T, np.int32)
    n = len(tok)
    ll = np.full(len(Ts), 123.0, np.float64)
    fl = [np.full(n, -7.0, np.float32) for _ in range(4)]
    pf = np.full(n, -7, np.int32)
    outs = [_lib.fptr(a) if post else None for a in fl] + [_lib.iptr(pf) if post else None]
    rc = lib.rvb_test_ctc_score_graph(_lib.fptr(lp), _lib.iptr(Ts), len(Ts) if n_seq is None else n_seq, V, _lib.iptr(tok), _lib.iptr(nn),
                                      _lib.iptr(off), _lib.iptr(prd), _lib.u8ptr(fin), blank, slab, _lib.dptr(ll), *outs)
    untouched = np.all(ll == 123.0) and all(np.all(a == -7.0) for a in fl) and np.all(pf == -7)
    assert rc == 0 or untouched                             # a refusal writes nothing
    return rc, lib.rvb_last_error().decode()


def chain(ids):
    n = len(ids)
    return list(ids), [[j - 1] for j in range(n)], [j == n - 1 for j in range(n)]


def test_the_hook_refuses_by_name_before_any_device_work(tlib):
    lib = tlib
    ok = chain([1, 2, 3])
    rc, msg = _hook(lib, [ok, chain([1, W, 2])], T=(9, 9))
    assert rc == ARG and msg.startswith("rvb_test_ctc_score_graph: sequence 1: node 1: a wildcard has no full-sum score")
    rc, msg = _hook(lib, [ok, ([], [], [])], T=(20, 20));        assert rc == ARG and "sequence 1: empty graph" in msg
    rc, msg = _hook(lib, [chain([1, 8])]);                       assert rc == ARG and "node 1: label 8 outside [0, 8)" in msg
    rc, msg = _hook(lib, [chain([1, -3])]);                      assert rc == ARG and "node 1: label -3 outside" in msg
    rc, msg = _hook(lib, [ok, chain([1, 0, 2])], T=(9, 9));      assert rc == ARG and "sequence 1: node 1: label is the blank id 0" in msg
    rc, msg = _hook(lib, [([1, 2], [[-1], [1]], [0, 1])]);       assert rc == ARG and "node 1: predecessor 1 is not" in msg
    rc, msg = _hook(lib, [([1, 2], [[-1], [-2]], [0, 1])]);      assert rc == ARG and "node 1: predecessor -2 is not" in msg
    rc, msg = _hook(lib, [([1, 2, 3], [[-1], [0], [1, 0, 1]], [0, 0, 1])]); assert rc == ARG and "node 2: duplicate predecessor 1" in msg
    rc, msg = _hook(lib, [([1, 2], [[-1], []], [0, 1])]);        assert rc == ARG and "node 1: empty predecessor list" in msg
    rc, msg = _hook(lib, [([1, 2], [[-1], [0]], [0, 0])]);       assert rc == ARG and "sequence 0: no final node" in msg
    rc, msg = _hook(lib, [ok], blank=8);                         assert rc == ARG and "blank id outside" in msg
    rc, msg = _hook(lib, [ok], n_seq=0);                         assert rc == ARG and "n_seq >= 1" in msg
    rc, msg = _hook(lib, [ok], slab=0);                          assert rc == ARG and "slab_rows >= 1" in msg
    rc, msg = _hook(lib, [ok], T=(0,));                          assert rc == ARG and "sequence 0: need T >= 1" in msg
    # caps
    rc, msg = _hook(lib, [chain([1 + j % 7 for j in range(8193)])], T=(8200,))
    assert rc == UNSUPPORTED and "8193 nodes exceed the cap of 8192 nodes" in msg
    wide = ([1] * 65 + [2], [[-1]] * 65 + [list(range(64, -1, -1))], [0] * 65 + [1])
    rc, msg = _hook(lib, [wide]);                                assert rc == UNSUPPORTED and "node 65: in-degree 65 exceeds the cap of 64" in msg
    # infeasible: the shortest reading of the graph needs more frames than there are (1 1 needs a blank between)
    rc, msg = _hook(lib, [ok, chain([1, 1, 2])], T=(9, 3))
    assert rc == ARG and "sequence 1: infeasible: no path of 3 frames through the graph ends in a final node with a finite score" in msg
    rc, msg = _hook(lib, [([1, 2, 3], [[-1], [0], [0]], [0, 0, 1])], T=(1,), post=False)
    assert rc == ARG and "infeasible: no path of 1 frames" in msg


def fan(n):
    """node 0, then n nodes that all follow it, each final: node 0 has out-degree n, every in-degree is 1"""
    return [1] + [2 + j % 5 for j in range(n)], [[-1]] + [[0]] * n, [0] + [1] * n


def test_the_out_degree_cap_applies_to_posteriors_only(tlib):
    rc, msg = _hook(tlib, [chain([1, 2]), fan(65)], T=(9, 9))
    assert rc == UNSUPPORTED and "sequence 1: node 0: out-degree 65 exceeds the cap of 64" in msg
    rc, msg = _hook(tlib, [fan(65)], post=False)                 # forward only: not refused for the degree
    assert rc in (0, -2)
    assert rc == 0 or "no HIP device" in msg
    rc, msg = _hook(tlib, [fan(64)])                             # at the cap: runs (the message of a success is stale)
    assert rc == 0 or (rc == -2 and "no HIP device" in msg)


def test_a_valid_request_runs_or_reports_the_missing_device(tlib):
    rc, msg = _hook(tlib, [([1, 2, 3, 4], [[-1], [-1], [1, 0], [2]], [0, 0, 1, 1])])
    assert rc in (0, -2)                                        # runs on a GPU, "no HIP device" (RVB_E_HIP) without
    assert rc == 0 or "no HIP device" in msg
