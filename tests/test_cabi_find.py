"""rvb_ctc_find and its lab hook check their arguments before any device work: these hold with and without a GPU."""
import ctypes as C
import os
import re

import numpy as np

from conftest import ROOT
from reverb_amd import _lib


def test_the_header_declares_it_and_the_product_exports_it():
    text = open(os.path.join(ROOT, "include", "rvb.h")).read()
    assert re.search(r"#define\s+RVB_CTC_FIND_MAX_TOKENS\s+32", text)
    decl = re.search(r"int rvb_ctc_find\(([^;]*)\);", text)
    assert decl and len(re.sub(r"/\*.*?\*/", "", decl.group(1)).split(",")) == 15 == len(_lib.SIGNATURES["rvb_ctc_find"][1])
    assert "rvb_ctc_find" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = C.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "rvb_ctc_find")
    assert not hasattr(lib, "rvb_test_ctc_find")           # the hook is not part of the product
    assert hasattr(_lib.load_test(), "rvb_test_ctc_find")
    hook = re.search(r"int rvb_test_ctc_find\(([^;]*)\);", open(os.path.join(ROOT, "reverb_amd", "csrc", "test_api.h")).read())
    assert hook and len(hook.group(1).split(",")) == 21 == len(_lib.TEST_SIGNATURES["rvb_test_ctc_find"][1])


def test_null_engine_is_reported():
    lib = _lib.load()
    one, f = np.ones(1, np.int32), np.zeros(1, np.float32)
    ip = _lib.iptr
    assert lib.rvb_ctc_find(None, ip(one), ip(one), 1, _lib.fptr(f), ip(one), ip(one), 1, 4, 4, ip(one), ip(one), ip(one), _lib.fptr(f),
                            None) == -1
    assert b"rvb_ctc_find: null engine" in lib.rvb_last_error()


def _hook(lib, phrases, T=(20,), V=8, thr=None, blank=0, slab=64, max_cand=16, max_hits=4, w="rows", tok_lens=None, lp=None,
          n_phrases=None, n_seq=None):
    rng = np.random.default_rng(0)
    M = max(int(sum(max(t, 0) for t in T)), 1)
    if lp is None:
        lp = np.log(rng.dirichlet(np.ones(V), size=M)).astype(np.float32)
    wv = np.ascontiguousarray(lp.max(axis=1)) if isinstance(w, str) else w
    tok = np.ascontiguousarray(np.concatenate([np.asarray(p, np.int32) for p in phrases] + [np.zeros(1, np.int32)]), np.int32)
    tl = np.array([len(p) for p in phrases] if tok_lens is None else tok_lens, np.int32)
    thr = np.full(len(tl), -np.inf, np.float32) if thr is None else np.asarray(thr, np.float32)
    Ts = np.asarray(T, np.int32)
    n_p, n_s = len(tl) if n_phrases is None else n_phrases, len(Ts) if n_seq is None else n_seq
    pairs, mc, mh = max(len(tl) * len(Ts), 1), max(min(max_cand, 64), 1), max(max_hits, 1)
    cnt = np.full(pairs, -7, np.int64)
    re_, rs, nh = np.full(pairs * mc, -7, np.int32), np.full(pairs * mc, -7, np.int32), np.full(pairs, -7, np.int32)
    rv, hv = np.full(pairs * mc, 123.0, np.float32), np.full(pairs * mh, 123.0, np.float32)
    hs, he = np.full(pairs * mh, -7, np.int32), np.full(pairs * mh, -7, np.int32)
    rc = lib.rvb_test_ctc_find(_lib.fptr(lp), _lib.iptr(Ts), n_s, V, None if wv is None else _lib.fptr(wv), _lib.iptr(tok), _lib.iptr(tl),
                               n_p, _lib.fptr(thr), blank, slab, max_cand, max_hits, cnt.ctypes.data_as(_lib._i64p), _lib.iptr(re_),
                               _lib.iptr(rs), _lib.fptr(rv), _lib.iptr(nh), _lib.iptr(hs), _lib.iptr(he), _lib.fptr(hv))
    untouched = (np.all(cnt == -7) and np.all(re_ == -7) and np.all(rs == -7) and np.all(nh == -7) and np.all(hs == -7) and
                 np.all(he == -7) and np.all(rv == 123.0) and np.all(hv == 123.0))
    assert rc == 0 or untouched                             # a refusal writes nothing
    return rc, lib.rvb_last_error().decode()


def test_the_hook_refuses_by_name_before_any_device_work(lib):
    ARG, UNSUPPORTED, NOMEM = -1, -5, -4
    ok = [[1, 2], [3]]
    rc, msg = _hook(lib, [[1, 2], []]);                          assert rc == ARG and "phrase 1: empty phrase" in msg
    rc, msg = _hook(lib, [[1, 8]]);                              assert rc == ARG and "token id 8 outside [0, 8)" in msg
    rc, msg = _hook(lib, [[1, -3]]);                             assert rc == ARG and "outside" in msg
    rc, msg = _hook(lib, [[1, 0, 2]]);                           assert rc == ARG and "token 1 is the blank id 0" in msg
    rc, msg = _hook(lib, ok, blank=8);                           assert rc == ARG and "blank id outside" in msg
    rc, msg = _hook(lib, ok, n_phrases=0);                       assert rc == ARG and "n_phrases >= 1" in msg
    rc, msg = _hook(lib, ok, n_seq=0);                           assert rc == ARG and "n_seq >= 1" in msg
    rc, msg = _hook(lib, ok, max_cand=0);                        assert rc == ARG and "max_candidates >= 1" in msg
    rc, msg = _hook(lib, ok, max_hits=0);                        assert rc == ARG and "max_hits >= 1" in msg
    rc, msg = _hook(lib, ok, slab=0);                            assert rc == ARG and "slab_rows >= 1" in msg
    rc, msg = _hook(lib, ok, thr=[-1.0, 0.5]);                   assert rc == ARG and "phrase 1: threshold" in msg
    rc, msg = _hook(lib, ok, thr=[float("nan"), -1.0]);          assert rc == ARG and "phrase 0: threshold" in msg
    rc, msg = _hook(lib, ok, T=(20, -1));                        assert rc == ARG and "sequence 1" in msg
    rc, msg = _hook(lib, [list(range(1, 8)) * 5][:1], tok_lens=[33])
    assert rc == UNSUPPORTED and "33 tokens exceed the cap of 32" in msg and "rvb_ctc_align_wild" in msg
    rc, msg = _hook(lib, [[1]] * 4, T=(5, 5, 5, 5), max_cand=2 ** 31 - 1)
    assert rc == NOMEM and "%d bytes of candidate buffers" % (16 * (2 ** 31 - 1) * 12) in msg
    # a row maximum that is not finite
    lp = np.log(np.random.default_rng(1).dirichlet(np.ones(8), size=20)).astype(np.float32)
    w = np.ascontiguousarray(lp.max(axis=1)); w[7] = np.inf
    rc, msg = _hook(lib, ok, lp=lp, w=w);                        assert rc == ARG and "row maximum of frame 7 is not finite" in msg
    bad = lp.copy(); bad[3] = -np.inf
    rc, msg = _hook(lib, ok, lp=bad, w=None);                    assert rc == ARG and "row maximum of frame 3 is not finite" in msg
    rc, msg = _hook(lib, ok, lp=lp, w=None)
    assert rc in (0, -2)                                        # a valid request: runs on a GPU, "no HIP device" (RVB_E_HIP) without
    assert rc == 0 or "no HIP device" in msg
