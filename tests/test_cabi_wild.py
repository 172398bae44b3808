"""rvb_ctc_align_wild and its lab hook check their arguments before any device work: these hold with and without a GPU."""
import os
import re

import numpy as np

import force_align_ref as R
from conftest import ROOT
from reverb_amd import _lib

W = -2


def test_the_header_names_the_wildcard():
    text = open(os.path.join(ROOT, "include", "rvb.h")).read()
    assert re.search(r"#define\s+RVB_CTC_WILDCARD\s+\(-2\)", text)
    from reverb_amd.ctc_align import WILDCARD
    assert WILDCARD == W


def test_null_engine_and_null_arguments_are_reported():
    lib = _lib.load()
    one = np.ones(1, np.int32)
    ip = _lib.iptr
    assert lib.rvb_ctc_align_wild(None, ip(one), ip(one), 1, ip(one), ip(one), 0.0, None, None, None, None, None, None) == -1
    assert b"rvb_ctc_align_wild: null engine" in lib.rvb_last_error()
    assert lib.rvb_ctc_align(None, ip(one), ip(one), 1, ip(one), ip(one), None, None, None, None, None, None) == -1
    assert b"rvb_ctc_align: null engine" in lib.rvb_last_error()


def _hook(lib, lp, w, bias, y, slab=64, T=None, L=None, blank=0):
    lp = np.ascontiguousarray(lp, np.float32)
    y = np.ascontiguousarray(y, np.int32)
    T = lp.shape[0] if T is None else T
    labels = np.full(max(min(T, 1 << 16), 1), -7, np.int32)
    score = np.full(1, 123.0, np.float32)
    rc = lib.rvb_test_ctc_viterbi_wild(_lib.fptr(lp), T, lp.shape[1], None if w is None else _lib.fptr(w), bias, _lib.iptr(y),
                                       len(y) if L is None else L, blank, slab, _lib.iptr(labels), _lib.fptr(score))
    assert rc == 0 or (np.all(labels == -7) and score[0] == 123.0)          # a refusal writes nothing
    return rc, lib.rvb_last_error().decode()


def test_the_hook_refuses_out_of_range_requests_before_any_device_work(lib):
    lp, y, _ = R.make_case(1, 20, 8, 5, "random")
    w = np.ascontiguousarray(lp.max(axis=1))
    y = np.array(y, np.int32)
    y[2] = W
    rc, msg = _hook(lib, lp, None, 0.0, y);                 assert rc == -1 and "null argument" in msg
    rc, msg = _hook(lib, lp, w, 0.0, y, L=0);               assert rc == -1 and "empty transcript" in msg
    rc, msg = _hook(lib, lp, w, 0.0, y, T=0);               assert rc == -1 and "T >= 1" in msg
    rc, msg = _hook(lib, lp, w, 0.0, y, slab=0);            assert rc == -1 and "slab_rows >= 1" in msg
    rc, msg = _hook(lib, lp, w, 0.5, y);                    assert rc == -1 and "bias" in msg
    rc, msg = _hook(lib, lp, w, float("nan"), y);           assert rc == -1 and "bias" in msg
    rc, msg = _hook(lib, lp, w, 0.0, [1, 8, W]);            assert rc == -1 and "token id 8 outside [0, 8)" in msg
    rc, msg = _hook(lib, lp, w, 0.0, [1, -3, W]);           assert rc == -1 and "outside" in msg
    rc, msg = _hook(lib, lp, w, 0.0, [1, 0, W]);            assert rc == -1 and "blank" in msg
    rc, msg = _hook(lib, lp, w, 0.0, y, blank=8);           assert rc == -1 and "blank id outside" in msg
    rc, msg = _hook(lib, lp[:5], w[:5], 0.0, [1, W, W, 2, 3])
    assert rc == -1 and "infeasible" in msg and "1 adjacent repeats need at least 6 frames" in msg
    rc, msg = _hook(lib, lp, w, 0.0, [W] * 16384, L=16384); assert rc == -5 and "16383 tokens" in msg
    rc, msg = _hook(lib, lp, w, 0.0, y, T=(1 << 20) + 1);   assert rc == -5 and "frames exceed the cap" in msg
    # the plain hook knows no wildcard
    out = np.full(20, -7, np.int32); sc = np.full(1, 123.0, np.float32)
    assert lib.rvb_test_ctc_viterbi(_lib.fptr(lp), 20, 8, _lib.iptr(y), 5, 0, 64, _lib.iptr(out), _lib.fptr(sc)) == -1
    assert b"token id -2 outside" in lib.rvb_last_error() and np.all(out == -7) and sc[0] == 123.0
