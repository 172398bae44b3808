"""rvb_ctc_score_graph_long_*: the header declares the seven calls, the product exports them, limits answers without a device and a
null engine is reported by every call.  These hold with and without a GPU."""
import ctypes as C
import os
import re

import numpy as np

from conftest import ROOT
from reverb_amd import _lib

ARG = -1
CALLS = {"limits": 4, "begin": 9, "feed": 1, "loglik": 2, "feed_back": 1, "finish": 6, "end": 1}


def test_the_header_declares_the_seven_calls_and_the_product_exports_them():
    text = open(os.path.join(ROOT, "include", "rvb.h")).read()
    lib = C.CDLL(_lib.LIB_PATH)
    for name, n_args in CALLS.items():
        full = "rvb_ctc_score_graph_long_" + name
        decl = re.search(r"int %s\(([^;]*)\);" % full, text)
        assert decl and len(decl.group(1).split(",")) == n_args == len(_lib.SIGNATURES[full][1]), full
        assert hasattr(lib, full), full
    assert "rvb_ctc_score_graph_long_begin" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "a windowed full sum over graphs" not in text              # what rvb_ctc_align_graph_long_* no longer calls "not offered"
    assert "several graphs per call" in text
    assert not hasattr(lib, "rvb_test_ctc_score_graph_window")        # the hook is not part of the product
    assert hasattr(_lib.load_test(), "rvb_test_ctc_score_graph_window")
    hook = re.search(r"int rvb_test_ctc_score_graph_window\(([^;]*)\);", open(os.path.join(ROOT, "reverb_amd", "csrc", "test_api.h")).read())
    assert hook and len(hook.group(1).split(",")) == 21 == len(_lib.TEST_SIGNATURES["rvb_test_ctc_score_graph_window"][1])


def test_limits_answer_without_a_device():
    lib = _lib.load()
    out = [np.full(1, -7, np.int32) for _ in range(4)]
    assert lib.rvb_ctc_score_graph_long_limits(*[_lib.iptr(a) for a in out]) == 0
    frames, degree, max_w, default_w = (int(a[0]) for a in out)
    assert (max_w, default_w) == (4096, 4096) and degree == 64 and frames == 1 << 20
    assert lib.rvb_ctc_score_graph_long_limits(None, None, None, None) == 0
    align = [np.full(1, -7, np.int32) for _ in range(4)]
    assert lib.rvb_ctc_align_graph_long_limits(*[_lib.iptr(a) for a in align]) == 0
    assert int(align[2][0]) == 8192                                  # the aligner keeps its own cap


def test_a_null_engine_is_reported_by_every_call():
    lib = _lib.load()
    one, u, d, f = np.ones(2, np.int32), np.ones(1, np.uint8), np.zeros(1, np.float64), np.zeros(1, np.float32)
    ip = _lib.iptr
    calls = {"begin": (None, ip(one), 1, ip(one), ip(one), _lib.u8ptr(u), 10, 0, 0), "feed": (None,), "loglik": (None, _lib.dptr(d)),
             "feed_back": (None,), "finish": (None, _lib.fptr(f), None, None, None, None), "end": (None,)}
    for name, args in calls.items():
        full = "rvb_ctc_score_graph_long_" + name
        assert getattr(lib, full)(*args) == ARG, full
        assert (full + ": null engine").encode() in lib.rvb_last_error()
