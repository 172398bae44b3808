"""rvb_ctc_align_graph, its limits call and its lab hook check their arguments before any device work: these hold with and without a GPU."""
import ctypes as C
import os
import re

import numpy as np

from conftest import ROOT
from reverb_amd import _lib

W = -2


def test_the_header_declares_them_and_the_product_exports_them():
    text = open(os.path.join(ROOT, "include", "rvb.h")).read()
    for name, value in (("MAX_NODES", 8192), ("MAX_IN_DEGREE", 64), ("MAX_ARCS", 32768)):
        assert re.search(r"#define\s+RVB_CTC_GRAPH_%s\s+%d\b" % (name, value), text)
    for name, n_args in (("rvb_ctc_align_graph", 19), ("rvb_ctc_align_graph_limits", 4)):
        decl = re.search(r"int %s\(([^;]*)\);" % name, text)
        assert decl and len(re.sub(r"/\*.*?\*/", "", decl.group(1)).split(",")) == n_args == len(_lib.SIGNATURES[name][1])
        assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = C.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "rvb_ctc_align_graph") and hasattr(lib, "rvb_ctc_align_graph_limits")
    assert not hasattr(lib, "rvb_test_ctc_viterbi_graph")          # the hook is not part of the product
    assert hasattr(_lib.load_test(), "rvb_test_ctc_viterbi_graph")
    hook = re.search(r"int rvb_test_ctc_viterbi_graph\(([^;]*)\);", open(os.path.join(ROOT, "reverb_amd", "csrc", "test_api.h")).read())
    assert hook and len(hook.group(1).split(",")) == 16 == len(_lib.TEST_SIGNATURES["rvb_test_ctc_viterbi_graph"][1])


def test_the_limits_are_the_defines():
    lib = _lib.load()
    out = [np.zeros(1, np.int32) for _ in range(4)]
    assert lib.rvb_ctc_align_graph_limits(*[_lib.iptr(o) for o in out]) == 0
    assert [int(o[0]) for o in out] == [8192, 64, 32768, 1048576]
    assert lib.rvb_ctc_align_graph_limits(None, None, None, None) == 0


def test_null_engine_is_reported():
    lib = _lib.load()
    one, f, u = np.ones(1, np.int32), np.zeros(1, np.float32), np.ones(1, np.uint8)
    ip = _lib.iptr
    assert lib.rvb_ctc_align_graph(None, ip(one), ip(one), ip(one), ip(one), _lib.u8ptr(u), 1, ip(one), ip(one), 0.0, None, None, None, None,
                                   None, None, None, None, _lib.fptr(f)) == -1
    assert b"rvb_ctc_align_graph: null engine" in lib.rvb_last_error()


def _hook(lib, graphs, T=(20,), V=8, bias=0.0, blank=0, slab=64, w="rows", n_seq=None):
    """graphs: [(tokens, preds, finals)]"""
    rng = np.random.default_rng(0)
    M = max(int(sum(max(t, 0) for t in T)), 1)
    lp = np.log(rng.dirichlet(np.ones(V), size=M)).astype(np.float32)
    wv = np.ascontiguousarray(lp.max(axis=1)) if isinstance(w, str) else w
    tok = np.ascontiguousarray(np.concatenate([np.asarray(g[0], np.int32) for g in graphs] + [np.zeros(1, np.int32)]), np.int32)
    nn = np.array([len(g[0]) for g in graphs], np.int32)
    off = np.concatenate([np.concatenate([[0], np.cumsum([len(p) for p in g[1]])]) for g in graphs]).astype(np.int32)
    prd = np.array([p for g in graphs for ps in g[1] for p in ps] + [0], np.int32)
    fin = np.concatenate([np.asarray(g[2], np.uint8) for g in graphs] + [np.zeros(1, np.uint8)])
    Ts = np.asarray(T, np.int32)
    labels, fnode, score = np.full(M, -7, np.int32), np.full(M, -7, np.int32), np.full(len(Ts), 123.0, np.float32)
    rc = lib.rvb_test_ctc_viterbi_graph(_lib.fptr(lp), _lib.iptr(Ts), len(Ts) if n_seq is None else n_seq, V, None if wv is None else _lib.fptr(wv),
                                        bias, _lib.iptr(tok), _lib.iptr(nn), _lib.iptr(off), _lib.iptr(prd), _lib.u8ptr(fin), blank, slab,
                                        _lib.iptr(labels), _lib.iptr(fnode), _lib.fptr(score))
    untouched = np.all(labels == -7) and np.all(fnode == -7) and np.all(score == 123.0)
    assert rc == 0 or untouched                             # a refusal writes nothing
    return rc, lib.rvb_last_error().decode()


def chain(ids):
    n = len(ids)
    return list(ids), [[j - 1] for j in range(n)], [j == n - 1 for j in range(n)]


def test_the_hook_refuses_by_name_before_any_device_work(lib):
    ARG, UNSUPPORTED = -1, -5
    ok = chain([1, 2, 3])
    rc, msg = _hook(lib, [ok, ([], [], [])], T=(20, 20));        assert rc == ARG and "sequence 1: empty graph" in msg
    rc, msg = _hook(lib, [chain([1, 8])]);                       assert rc == ARG and "node 1: label 8 outside [0, 8)" in msg
    rc, msg = _hook(lib, [chain([1, -3])]);                      assert rc == ARG and "node 1: label -3 outside" in msg
    rc, msg = _hook(lib, [ok, chain([1, 0, 2])], T=(9, 9));      assert rc == ARG and "sequence 1: node 1: label is the blank id 0" in msg
    rc, msg = _hook(lib, [([1, 2], [[-1], [1]], [0, 1])]);       assert rc == ARG and "node 1: predecessor 1 is not" in msg
    rc, msg = _hook(lib, [([1, 2], [[-1], [-2]], [0, 1])]);      assert rc == ARG and "node 1: predecessor -2 is not" in msg
    rc, msg = _hook(lib, [([1, 2, 3], [[-1], [0], [1, 0, 1]], [0, 0, 1])]); assert rc == ARG and "node 2: duplicate predecessor 1" in msg
    rc, msg = _hook(lib, [([1, 2], [[-1], [-1, 0, -1]], [0, 1])])
    assert rc == ARG and "node 1: duplicate predecessor -1" in msg
    rc, msg = _hook(lib, [([1, 2], [[-1], []], [0, 1])]);        assert rc == ARG and "node 1: empty predecessor list" in msg
    rc, msg = _hook(lib, [([1, 2], [[-1], [0]], [0, 0])]);       assert rc == ARG and "sequence 0: no final node" in msg
    for bias in (0.5, float("nan"), float("-inf")):
        rc, msg = _hook(lib, [ok], bias=bias);                   assert rc == ARG and "wildcard_bias must be finite and <= 0" in msg
    rc, msg = _hook(lib, [ok], blank=8);                         assert rc == ARG and "blank id outside" in msg
    rc, msg = _hook(lib, [ok], n_seq=0);                         assert rc == ARG and "n_seq >= 1" in msg
    rc, msg = _hook(lib, [ok], slab=0);                          assert rc == ARG and "slab_rows >= 1" in msg
    rc, msg = _hook(lib, [ok], T=(0,));                          assert rc == ARG and "sequence 0: need T >= 1" in msg
    rc, msg = _hook(lib, [chain([1, W, 2])], w=None);            assert rc == ARG and "wildcards needs w" in msg
    # caps
    rc, msg = _hook(lib, [chain([1 + j % 7 for j in range(8193)])])
    assert rc == UNSUPPORTED and "8193 nodes exceed the cap of 8192 nodes" in msg
    wide = ([1] * 65 + [2], [[-1]] * 65 + [list(range(64, -1, -1))], [0] * 65 + [1])
    rc, msg = _hook(lib, [wide]);                                assert rc == UNSUPPORTED and "node 65: in-degree 65 exceeds the cap of 64" in msg
    many = ([1] * 64 + [2] * 600, [[-1]] * 64 + [list(range(63, -1, -1))] * 600, [0] * 64 + [1] * 600)
    rc, msg = _hook(lib, [many]);                                assert rc == UNSUPPORTED and "cap of 32768 arcs" in msg
    rc, msg = _hook(lib, [chain([1])], T=(2 ** 20 + 1,), V=2)
    assert rc == UNSUPPORTED and "1048577 frames exceed the cap of 1048576 frames" in msg


def test_a_valid_request_runs_or_reports_the_missing_device(lib):
    rc, msg = _hook(lib, [([1, 2, 3, W], [[-1], [-1], [1, 0], [2]], [0, 0, 1, 1])])
    assert rc in (0, -2)                                        # runs on a GPU, "no HIP device" (RVB_E_HIP) without
    assert rc == 0 or "no HIP device" in msg
