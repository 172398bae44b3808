"""The packed layout of rvd_upload_pcm_many as reverb_amd.diar_engine.window_layout states it, and what of the three new rvd_ calls
can be checked without a device: header, binding, export, and the refusals that come before any device work.  That window_layout's
window counts are rvd_num_windows' and its table is the library's is asserted on the GPU (tests/test_diar_many_gpu.py: both need an
engine)."""
import ctypes as C
import os
import re

import numpy as np

from conftest import ROOT
from reverb_amd import _lib
from reverb_amd.diar_engine import window_count, window_layout

RATE, WINDOW, STEP = 16000, 160000, 16000
SECONDS = [47.3, 3.2, 10.0, 12.0, 10.5, 0.0]
SAMPLES = [int(round(s * RATE)) for s in SECONDS]
NEW = ("rvd_upload_pcm_many", "rvd_segment_windows", "rvd_centroid_linkage_many")


def test_window_counts():
    assert SAMPLES == [756800, 51200, 160000, 192000, 168000, 0]
    assert [window_count(n, WINDOW, STEP) for n in SAMPLES] == [39, 1, 1, 3, 2, 0]
    # the rule, case by case: a full window every step while one fits, plus a zero-padded tail for what is left over
    assert window_count(1, WINDOW, STEP) == 1 and window_count(WINDOW - 1, WINDOW, STEP) == 1
    assert window_count(WINDOW + 1, WINDOW, STEP) == 2 and window_count(WINDOW + STEP, WINDOW, STEP) == 2
    assert window_count(-5, WINDOW, STEP) == 0


def _check_layout(samples):
    first = window_layout(samples, WINDOW, STEP)
    counts = [window_count(n, WINDOW, STEP) for n in samples]
    assert first.dtype == np.int64 and first.shape == (len(samples),)
    spans = []
    for f, W, n in zip(first, counts, samples):
        f = int(f)
        if W == 0:
            continue
        start = f * STEP                                             # every recording starts on a multiple of the step
        own = (W + WINDOW // STEP - 1) * STEP                        # its own zero-padded length ...
        assert own == (W - 1) * STEP + WINDOW >= n                   # ... which is what it has alone, and holds its samples
        # every valid window [start + w step, + window) lies inside the recording's span
        assert start + (W - 1) * STEP + WINDOW == start + own
        spans.append((f, W, start, start + own))
    for (f0, W0, a0, b0), (f1, W1, a1, b1) in zip(spans, spans[1:]):
        assert b0 == a1                                              # back to back: no sample shared, none wasted
        assert f1 - (f0 + W0) == WINDOW // STEP - 1 == 9             # exactly 9 global indices straddle the boundary
        # ... and every one of them really does straddle it, so none is a window of either recording
        for g in range(f0 + W0, f1):
            assert g * STEP < b0 < g * STEP + WINDOW
    # an empty recording takes no space: its entry is where the next recording starts
    nxt = 0
    for f, W in zip(first, counts):
        assert int(f) == nxt
        if W:
            nxt += W + 9
    return first, counts


def test_layout_of_the_test_recordings():
    first, counts = _check_layout(SAMPLES)
    assert list(first) == [0, 48, 58, 68, 80, 91]
    total = max(int(f) + W for f, W in zip(first, counts) if W)
    assert total == 82
    # valid windows of different recordings share no sample
    owner = np.full((total - 1) * STEP + WINDOW, -1, np.int64)
    for r, (f, W) in enumerate(zip(first, counts)):
        for w in range(W):
            seg = owner[(int(f) + w) * STEP:(int(f) + w) * STEP + WINDOW]
            assert np.all((seg == -1) | (seg == r))
            seg[:] = r


def test_layout_with_empty_recordings_anywhere():
    for samples in ([0, 51200, 0, 0, 192000, 0], [0], [0, 0], [160000], [1, 1, 1]):
        _check_layout(samples)
    assert list(window_layout([0, 51200, 0, 192000], WINDOW, STEP)) == [0, 0, 10, 10]
    assert list(window_layout([], WINDOW, STEP)) == []


def test_new_calls_are_declared_bound_and_exported():
    text = open(os.path.join(ROOT, "include", "rvd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _lib.load()                                                # the product library
    for name in NEW:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", code)
        assert m, f"include/rvd.h does not declare {name}"
        assert name in _lib.DIAR_SIGNATURES
        res, args = _lib.DIAR_SIGNATURES[name]
        assert res is C.c_int and len(args) == len(m.group(1).split(",")), name
        assert hasattr(lib, name), f"librvb.so does not export {name}"
    hooks = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "reverb_amd", "csrc", "test_api.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+rvb_test_centroid_linkage_many\s*\(([^)]*)\)", hooks)
    assert m and len(m.group(1).split(",")) == 6 == len(_lib.TEST_SIGNATURES["rvb_test_centroid_linkage_many"][1])


def test_refusals_that_need_no_device():
    lib = _lib.load()
    pcm = np.zeros(16, np.int16)
    ptrs = (C.POINTER(C.c_int16) * 1)(pcm.ctypes.data_as(C.POINTER(C.c_int16)))
    lens = (C.c_int64 * 1)(16)
    first = (C.c_int64 * 1)(-7)
    total = C.c_int64(-7)
    assert lib.rvd_upload_pcm_many(None, ptrs, lens, 1, first, C.byref(total)) == -1         # RVB_E_ARG
    assert b"rvd_upload_pcm_many" in lib.rvd_last_error() and b"null engine" in lib.rvd_last_error()
    for n_rec in (0, -3):
        assert lib.rvd_upload_pcm_many(None, ptrs, lens, n_rec, first, C.byref(total)) == -1
        assert b"n_rec" in lib.rvd_last_error()
    assert first[0] == -7 and total.value == -7                      # refused before anything is written
    win = (C.c_int64 * 1)(0)
    assert lib.rvd_segment_windows(None, win, 1, None) == -1
    assert b"rvd_segment_windows" in lib.rvd_last_error()
    x = (C.c_double * 4)(0, 0, 1, 1)
    z = (C.c_double * 4)()
    ns = (C.c_int32 * 1)(2)
    assert lib.rvd_centroid_linkage_many(None, x, ns, 1, 2, z) == -1
    assert b"rvd_centroid_linkage_many" in lib.rvd_last_error()
