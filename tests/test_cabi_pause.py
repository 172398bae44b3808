"""rvb_pause_chunks and its lab hooks check their arguments before any device work: these hold with and without a GPU."""
import ctypes as C
import os
import re

import numpy as np

from conftest import ROOT
from reverb_amd import _lib

ARG, HIP = -1, -2


def _args(text, name):
    decl = re.search(r"int %s\(([^;]*)\);" % name, text)
    assert decl, name
    return len(re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(","))


def test_the_header_declares_it_and_the_product_exports_it():
    text = open(os.path.join(ROOT, "include", "rvb.h")).read()
    assert _args(text, "rvb_pause_chunks") == 10 == len(_lib.SIGNATURES["rvb_pause_chunks"][1])
    assert _args(text, "rvb_fixed_chunks") == 1 == len(_lib.SIGNATURES["rvb_fixed_chunks"][1])
    assert "THE DEFINITION" in text and "LAST c in [lo, hi]" in text          # stated once, here
    assert "rvb_pause_chunks" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = C.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "rvb_pause_chunks") and hasattr(lib, "rvb_fixed_chunks")
    hooks = open(os.path.join(ROOT, "reverb_amd", "csrc", "test_api.h")).read()
    for name, n in (("rvb_test_pause_cuts", 11), ("rvb_test_gather_chunks", 7)):
        assert not hasattr(lib, name)                       # the hooks are not part of the product
        assert hasattr(_lib.load_test(), name)
        assert _args(hooks, name) == n == len(_lib.TEST_SIGNATURES[name][1])


def _call(lib, chunk_size, search, h):
    first, n = np.full(2, -7, np.int64), C.c_int64(-7)
    starts, lens = np.full(4, -7, np.int32), np.full(4, -7, np.int32)
    rc = lib.rvb_pause_chunks(None, chunk_size, search, h, first.ctypes.data_as(_lib._i64p), _lib.iptr(starts), _lib.iptr(lens), 4,
                              C.byref(n), None)
    assert n.value == -7 and np.all(first == -7) and np.all(starts == -7) and np.all(lens == -7)       # a refusal writes nothing
    return rc, lib.rvb_last_error().decode()


def test_arguments_are_refused_by_name_before_the_engine_is_touched():
    lib = _lib.load()
    rc, msg = _call(lib, 256, 64, 0);        assert rc == ARG and "rvb_pause_chunks: h = 0" in msg
    rc, msg = _call(lib, 256, 64, 65);       assert rc == ARG and "rvb_pause_chunks: h = 65" in msg and "[1, 64]" in msg
    rc, msg = _call(lib, 6, 7, 10);          assert rc == ARG and "rvb_pause_chunks: chunk_size must be at least 7" in msg
    rc, msg = _call(lib, 256, 6, 10);        assert rc == ARG and "rvb_pause_chunks: search = 6" in msg
    rc, msg = _call(lib, 256, 250, 10);      assert rc == ARG and "search = 250" in msg and "chunk_size - 7 = 249" in msg
    rc, msg = _call(lib, 16, 4, 10);         assert rc == ARG and "search = 4" in msg       # chunk_size // 4 of the smallest test shape
    rc, msg = _call(lib, 256, 64, 10);       assert rc == ARG and "rvb_pause_chunks: null engine" in msg
    assert lib.rvb_fixed_chunks(None) == ARG and b"rvb_fixed_chunks: null engine" in lib.rvb_last_error()


def _cuts_hook(lib, n_rows=40, row0=(0,), n_frames=(40,), chunk_size=16, search=7, h=1, capacity=64):
    x = np.zeros((max(n_rows, 1), 80), np.float32)
    r0, nf = np.asarray(row0, np.int64), np.asarray(n_frames, np.int64)
    starts, counts = np.full(max(capacity, 1), -7, np.int32), np.full(len(r0), -7, np.int32)
    rc = lib.rvb_test_pause_cuts(_lib.fptr(x), n_rows, r0.ctypes.data_as(_lib._i64p), nf.ctypes.data_as(_lib._i64p), len(r0), chunk_size,
                                 search, h, _lib.iptr(starts), capacity, _lib.iptr(counts))
    assert rc == 0 or (np.all(starts == -7) and np.all(counts == -7))
    return rc, lib.rvb_last_error().decode()


def test_the_hooks_refuse_by_name_before_any_device_work(lib):
    rc, msg = _cuts_hook(lib, h=0);                          assert rc == ARG and "rvb_test_pause_cuts: h = 0" in msg
    rc, msg = _cuts_hook(lib, h=65);                         assert rc == ARG and "h = 65" in msg
    rc, msg = _cuts_hook(lib, search=4);                     assert rc == ARG and "rvb_test_pause_cuts: search = 4" in msg
    rc, msg = _cuts_hook(lib, search=10);                    assert rc == ARG and "search = 10" in msg
    rc, msg = _cuts_hook(lib, chunk_size=6);                 assert rc == ARG and "chunk_size must be at least 7" in msg
    rc, msg = _cuts_hook(lib, n_frames=(41,));               assert rc == ARG and "recording 0 lies outside the 40 rows" in msg
    rc, msg = _cuts_hook(lib, row0=(0, -1), n_frames=(5, 5)); assert rc == ARG and "recording 1" in msg
    rc, msg = _cuts_hook(lib)
    assert rc in (0, HIP) and (rc == 0 or "no HIP device" in msg)          # a valid request: runs on a GPU
    x = np.zeros((20, 80), np.float32)
    out = np.full((2 * 16 + 1, 80), -7.0, np.float32)

    def gather(src, lens, chunk_size=16, n_rows=20):
        s, ln = np.asarray(src, np.int64), np.asarray(lens, np.int32)
        rc = lib.rvb_test_gather_chunks(_lib.fptr(x), n_rows, s.ctypes.data_as(_lib._i64p), _lib.iptr(ln), len(s), chunk_size, _lib.fptr(out))
        assert rc == 0 or np.all(out == -7.0)
        return rc, lib.rvb_last_error().decode()
    rc, msg = gather([0, 10], [10, 11]);                     assert rc == ARG and "rvb_test_gather_chunks: piece 1 lies outside the 20 rows" in msg
    rc, msg = gather([0, 2], [17, 7]);                       assert rc == ARG and "piece 0" in msg and "exceeds chunk_size" in msg
    rc, msg = gather([0, -1], [7, 7]);                       assert rc == ARG and "piece 1" in msg
    rc, msg = gather([0, 2], [7, 7], chunk_size=6);          assert rc == ARG and "bad argument" in msg
    rc, msg = gather([0, 4], [16, 7])
    assert rc in (0, HIP) and (rc == 0 or "no HIP device" in msg)
