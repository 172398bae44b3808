"""The slab feed the CTC lattice drivers share (csrc/ctc_slabs.h), on the host alone: rvb_test_slab_windows runs the row checks, the
window step of every slab and the coverage check over plain descriptors, and the reference is numpy.searchsorted."""
import ctypes as C

import numpy as np
import pytest

from reverb_amd import _lib

E_ARG, E_STATE = -1, -3
PREFIXES = ["ctc align", "ctc align graph", "ctc score", "ctc find"]
T2 = 8                                                     # rows per chunk; rows past a chunk's valid frames are padding


def chunk_rows(chunks, valid):
    """the rows of a sequence over `chunks`: the first valid[c] rows of each"""
    return np.concatenate([c * T2 + np.arange(valid[c]) for c in chunks]).astype(np.int32)


VALID = [5, 3, 5, 3]
SEQS = [chunk_rows([0, 1], VALID), chunk_rows([2, 3], VALID), chunk_rows([1, 2], VALID)]   # the third shares chunks with both
M = len(VALID) * T2


def slabs_of(size, descending, m=M):
    """as the drivers' callers cut them: ascending from row 0, descending in slabs that end at the last row"""
    if not descending:
        return [(r0, min(size, m - r0)) for r0 in range(0, m, size)]
    return [(max(0, r1 - size), r1 - max(0, r1 - size)) for r1 in range(m, 0, -size)]


def feed(who, seqs, slabs, descending):
    lib = _lib.load_test()
    n_seq, n_slabs = len(seqs), len(slabs)
    rows = np.ascontiguousarray(np.concatenate(list(seqs) + [np.zeros(1, np.int32)]), np.int32)
    T = np.array([len(s) for s in seqs], np.int32)
    sl = np.ascontiguousarray(np.array(slabs, np.int32).reshape(-1, 2))
    win = np.full((max(n_slabs, 1), n_seq, 2), -1, np.int32)
    any_, touch = np.full(max(n_slabs, 1), -1, np.int32), np.full(max(n_slabs, 1), -1, np.int32)
    fed, covered = C.c_int32(-1), C.c_int32(-1)
    rc = lib.rvb_test_slab_windows(who.encode(), _lib.iptr(rows), _lib.iptr(T), n_seq, _lib.iptr(sl), n_slabs, int(descending),
                                   _lib.iptr(win), _lib.iptr(any_), _lib.iptr(touch), C.byref(fed), C.byref(covered))
    return rc, lib.rvb_last_error().decode(), win[:n_slabs], any_[:n_slabs], touch[:n_slabs], fed.value, covered.value


def reference(seqs, slabs, descending):
    """per slab and sequence (f0, f1), per slab whether any sequence has a frame in it"""
    at = [(len(s), len(s)) if descending else (0, 0) for s in seqs]
    win, hit = [], []
    for r0, n in slabs:
        some = False
        for i, s in enumerate(seqs):
            f0, f1 = int(np.searchsorted(s, r0, "left")), int(np.searchsorted(s, r0 + n, "left"))
            if f0 < f1:
                at[i], some = (f0, f1), True
            else:
                at[i] = (at[i][0],) * 2 if descending else (at[i][1],) * 2      # the empty window where the sequence stands
        win.append(list(at))
        hit.append(some)
    return np.array(win, np.int32).reshape(len(slabs), len(seqs), 2), np.array(hit, np.int32)


@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("size", [1, 3, 8, 64])
def test_windows_match_searchsorted_and_tile(size, descending):
    slabs = slabs_of(size, descending)
    rc, msg, win, any_, touch, fed, covered = feed("ctc score", SEQS, slabs, descending)
    assert rc == 0 and fed == len(slabs) and covered == 1, msg
    want, hit = reference(SEQS, slabs, descending)
    assert np.array_equal(win, want)
    assert np.array_equal(any_, hit) and np.array_equal(touch, hit)
    for i, s in enumerate(SEQS):                           # the non-empty windows of a sequence tile [0, T) in sweep order
        spans = [tuple(w) for w in win[:, i] if w[0] < w[1]]
        spans = spans[::-1] if descending else spans
        assert spans[0][0] == 0 and spans[-1][1] == len(s)
        assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))


@pytest.mark.parametrize("descending", [False, True])
def test_sequence_without_frames_is_never_touched_and_covered(descending):
    seqs = [np.zeros(0, np.int32), SEQS[0]]                # the finder allows T = 0
    slabs = slabs_of(3, descending, 2 * T2)
    rc, msg, win, any_, touch, fed, covered = feed("ctc find", seqs, slabs, descending)
    assert rc == 0 and covered == 1, msg
    assert np.all(win[:, 0] == 0)
    want, hit = reference(seqs, slabs, descending)
    assert np.array_equal(win, want) and np.array_equal(touch, hit)


@pytest.mark.parametrize("descending", [False, True])
def test_slab_of_padding_rows_changes_nothing(descending):
    pad = (VALID[0], T2 - VALID[0])                        # rows 5 .. 7: past chunk 0's frames, before chunk 1's
    slabs = [(T2, T2), pad, (0, VALID[0])] if descending else [(0, VALID[0]), pad, (T2, T2)]
    rc, msg, win, any_, touch, fed, covered = feed("ctc align", SEQS[:1], slabs, descending)
    assert rc == 0 and covered == 1, msg
    assert list(touch) == [1, 0, 1] and list(any_) == [1, 0, 1]
    stand = win[0, 0, 0] if descending else win[0, 0, 1]   # where the sequence stood after the first slab
    assert tuple(win[1, 0]) == (stand, stand)
    assert np.array_equal(win, reference(SEQS[:1], slabs, descending)[0])


@pytest.mark.parametrize("who", PREFIXES)
@pytest.mark.parametrize("slabs", [[(0, T2), (0, T2)], [(T2, T2), (0, T2)]], ids=["twice", "out_of_order"])
def test_ascending_refuses_a_slab_twice_or_out_of_order(who, slabs):
    rc, msg, win, any_, touch, fed, covered = feed(who, SEQS, slabs + slabs_of(T2, False)[2:], False)
    assert rc == E_STATE and msg == who + ": slabs must arrive in row order"
    assert fed == (1 if slabs[0][0] == 0 else 0) and covered == 0


@pytest.mark.parametrize("slabs", [[(3 * T2, T2), (3 * T2, T2)], [(2 * T2, T2), (3 * T2, T2)]], ids=["twice", "out_of_order"])
def test_descending_refuses_a_slab_twice_or_out_of_order(slabs):
    rc, msg, win, any_, touch, fed, covered = feed("ctc score", SEQS, slabs, True)
    assert rc == E_STATE and msg == "ctc score: the backward sweep takes the slabs in descending row order"
    assert fed == (1 if slabs[0][0] == 3 * T2 else 0) and covered == 0


@pytest.mark.parametrize("who", PREFIXES)
def test_stopping_a_slab_early_fails_the_coverage_check(who):
    last = max(int(s[-1]) for s in SEQS)                   # the slabs after this row's hold padding only
    slabs = [s for s in slabs_of(3, False) if s[0] + s[1] <= last]
    rc, msg, win, any_, touch, fed, covered = feed(who, SEQS, slabs, False)
    assert rc == E_STATE and msg == who + ": the slabs did not cover every frame of a sequence"
    assert fed == len(slabs) and covered == 0
    assert np.array_equal(win, reference(SEQS, slabs, False)[0])


def test_stopping_the_backward_sweep_early_fails_its_coverage_check():
    slabs = slabs_of(3, True)
    rc, msg, win, any_, touch, fed, covered = feed("ctc score", SEQS, slabs[:-1], True)
    assert rc == E_STATE and msg == "ctc score: the backward sweep did not reach the first frame of a sequence"
    assert fed == len(slabs) - 1 and covered == 0


def test_rows_that_do_not_increase_are_refused_by_sequence():
    bad = SEQS[1].copy()
    bad[3] = bad[2]
    rc, msg, *_ = feed("rvb_ctc_find", [SEQS[0], bad], [(0, M)], False)
    assert rc == E_ARG and msg == "rvb_ctc_find: sequence 1: frame rows must increase"
