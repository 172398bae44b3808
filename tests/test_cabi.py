"""The C-ABI shared library loads on a CPU-only box and exports every symbol include/rvb.h
declares; without a GPU the product path fails loudly (no CPU fallback)."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import HAVE_GPU, ROOT
from reverb_amd import _lib


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "rvb.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(rvb_[a-z0-9_]+)\s*\(", text)))


def test_every_declared_symbol_is_exported_and_bound():
    lib = _lib.load()                                   # the PRODUCT library
    names = declared_symbols()
    assert len(names) >= 30
    for n in names:
        assert hasattr(lib, n), f"librvb.so does not export {n}"
        assert n in _lib.SIGNATURES, f"{n} has no ctypes prototype in reverb_amd/_lib.py"
    assert sorted(_lib.SIGNATURES) == names


def test_product_library_carries_no_test_hooks(lib):
    """the rvb_test_* hooks live in librvb_test.so (csrc/test_api.h); the product .so exports the two
    public headers and nothing else of the C ABI."""
    import subprocess
    assert not any(n.startswith("rvb_test_") for n in declared_symbols())
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True)
    if nm.returncode == 0:
        exported = {l.split()[-1] for l in nm.stdout.splitlines() if l.strip()}
        assert not [n for n in exported if n.startswith(("rvb_test_", "rvd_test_"))]
        c_abi = {n for n in exported if re.fullmatch(r"rv[bd]_[a-z0-9_]+", n)}
        assert c_abi == set(_lib.SIGNATURES) | set(_lib.DIAR_SIGNATURES), c_abi ^ (set(_lib.SIGNATURES) | set(_lib.DIAR_SIGNATURES))
    product = _lib.load()
    text = open(os.path.join(ROOT, "reverb_amd", "csrc", "test_api.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    hooks = sorted(set(re.findall(r"\b(rvb_test_[a-z0-9_]+)\s*\(", text)))
    assert hooks == sorted(_lib.TEST_SIGNATURES) and len(hooks) >= 20
    for n in hooks:
        assert hasattr(lib, n), f"librvb_test.so does not export {n}"
        assert not hasattr(product, n), f"librvb.so exports the test hook {n}"


def test_version_and_frame_count(lib):
    assert b"gfx950" in lib.rvb_version()
    assert lib.rvb_num_frames(399) == 0 and lib.rvb_num_frames(400) == 1 and lib.rvb_num_frames(57600000) == 359998


def test_struct_layout_matches_header():
    text = open(os.path.join(ROOT, "include", "rvb.h")).read()
    body = text[text.index("typedef struct rvb_model_cfg {"):text.index("} rvb_model_cfg;")]
    fields = re.findall(r"int32_t\s+([a-z_0-9]+);", body)
    assert fields == [f[0] for f in _lib.ModelCfg._fields_]
    assert fields[0] == "struct_size" and _lib.ModelCfg().struct_size == 4 * len(fields)


def _integration_stub_fields(struct_comment):
    """Field names of the ctypes stub INTEGRATION.md shows for `struct_comment` (the list a maintainer would paste)."""
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    at = text.index("# struct " + struct_comment)
    body = text[at:text.index(")]", at)]
    return re.findall(r'"([a-z_0-9]+)"', body)


def test_integration_stub_binds_the_header_field_for_field():
    """the document's stub had 19 fields against the header's 20.  The stub is parsed out of the
    document and compared with the headers, for both config structs and the audio info struct."""
    for header, struct, comment in (("rvb.h", "rvb_model_cfg", "rvb_model_cfg"), ("rvd.h", "rvd_model_cfg", "rvd_model_cfg")):
        text = open(os.path.join(ROOT, "include", header)).read()
        text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
        body = text[text.index("typedef struct %s {" % struct):text.index("} %s;" % struct)]
        assert _integration_stub_fields(comment) == re.findall(r"int32_t\s+([a-z_0-9]+);", body), header
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rvb.h")).read(), flags=re.S)
    body = text[text.index("typedef struct rvb_audio_info {"):text.index("} rvb_audio_info;")]
    assert _integration_stub_fields("rvb_audio_info") == re.findall(r"int(?:32|64)_t\s+([a-z_0-9]+);", body)


def test_a_binding_of_another_size_is_refused_by_name(lib):
    """A struct one field short (what following the stale document produced) or long must not be read: RVB_E_ARG."""
    assert lib.rvb_model_cfg_size() == ctypes.sizeof(_lib.ModelCfg) and lib.rvd_model_cfg_size() == ctypes.sizeof(_lib.DiarCfg)
    h = ctypes.c_void_p()
    for size in (ctypes.sizeof(_lib.ModelCfg) - 4, ctypes.sizeof(_lib.ModelCfg) + 4, 0):
        cfg = _lib.ModelCfg(struct_size=size)
        assert lib.rvb_create(ctypes.byref(cfg), 0, ctypes.byref(h)) == -1 and b"ABI mismatch" in lib.rvb_last_error()
    dcfg = _lib.DiarCfg(struct_size=ctypes.sizeof(_lib.DiarCfg) - 4)
    assert lib.rvd_create(ctypes.byref(dcfg), 0, ctypes.byref(h)) == -1 and b"ABI mismatch" in lib.rvd_last_error()


@pytest.mark.skipif(HAVE_GPU, reason="checks the no-GPU failure mode")
def test_fails_loudly_without_gpu(lib):
    from reverb_amd import synth
    from reverb_amd.engine import Engine
    cfg = synth.make_config("tiny")
    with pytest.raises(_lib.RvbError, match="no HIP device"):
        Engine(cfg, {}, dtype="f32")
    out = np.zeros(4, np.float32)
    rc = lib.rvb_test_gemm(0, _lib.fptr(out), _lib.fptr(out), None, None, _lib.fptr(out), 1, 1, 4, 1.0, 0, 1, 0, 0, 0, 0, 0)
    assert rc != 0 and b"no CPU fallback" in lib.rvb_last_error()


def test_diarization_kernel_hooks_refuse_out_of_range_shapes_before_any_device_work(lib):
    """The hooks of tests/test_diar_kernels_gpu.py check that the host buffers cover what the kernel will read (E_ARG = -1)
    before they look for a device, so these hold with and without a GPU."""
    f = _lib.fptr
    z = np.zeros(4096, np.float32)
    ib = np.array([0, 3], np.int32)
    assert lib.rvb_test_window_stats(f(z), 4096, 1, 2, 2048, 2048, 1e-5, f(z)) == -1          # window 2 ends past the wave
    assert lib.rvb_test_sinc_conv(0, f(z), 4096, f(z), 1, 251, 10, 400, f(z)) == -1           # 400 frames need 4 241 samples
    assert lib.rvb_test_pool_norm(1, 1, None, 0, 0, 30, 8, 8, f(z), f(z), 1e-5, 2, f(z), 20, 0, 5, f(z), f(z), 1.0, 0.0,
                                  f(z)) == -1                                                 # window 1 reads craw rows 5 .. 34
    assert lib.rvb_test_pool_norm(0, 0, f(z), 9, 8, 9, 16, 16, f(z), f(z), 1e-5, 2, None, 0, 0, 0, None, None, 1.0, 0.0,
                                  f(z)) == -1                                                 # 16 channels in rows of 8
    assert lib.rvb_test_conv1d5(80, f(z), 10, f(z), f(z), f(z), 7) == -1                        # M + 4 rows needed
    assert lib.rvb_test_conv1d5(72, f(z), 20, f(z), f(z), f(z), 7) == -1                        # 80 or 64 input channels
    assert lib.rvb_test_lstm_layer(0, f(z), 1, 1, 60, f(z), f(z), f(z), f(z), f(z)) == -1     # in % 8
    assert lib.rvb_test_classifier(0, f(z), 8, f(z), f(z), f(z), None, 4, 16, 2) == -1        # ldx < in
    assert lib.rvb_test_tstp(0, f(z), 3, _lib.iptr(ib), f(z), 10, 2, 1, 4, 8, f(z)) == -1     # item 1 in window 3 of 3


def test_trunk_kernel_hooks_refuse_out_of_range_shapes_before_any_device_work(lib):
    """The hooks of tests/test_emb_conv_kernels_gpu.py check their arguments (E_ARG = -1) and whether the named kernel applies to the
    shape (E_STATE = -3) before they look for a device, so these hold with and without a GPU."""
    f = _lib.fptr
    z = np.zeros(1 << 20, np.float32)
    ran = np.zeros(2, np.int32)

    def conv(dtype, path, B, Fi, Ti, cin, cout, stride, x2=False, Fi2=0, Ti2=0, cin2=0, stride2=2):
        return lib.rvb_test_conv2d(dtype, path, f(z), f(z), f(z), None, f(z), B, Fi, Ti, cin, cout, stride, 9, 1,
                                   f(z) if x2 else None, f(z) if x2 else None, Fi2, Ti2, cin2, stride2, _lib.iptr(ran))
    assert conv(1, 5, 1, 4, 8, 64, 64, 1) == -1                          # no path 5
    assert conv(1, 3, 1, 8, 16, 64, 64, 2) == -3                         # row64 runs stride 1 only
    assert conv(0, 2, 1, 4, 8, 128, 128, 1) == -3                        # the implicit GEMM is bf16 only
    assert conv(1, 4, 1, 4, 8, 128, 128, 1) == -3                        # the stream is 32 / 64 channels only
    assert conv(1, 1, 1, 4, 8, 48, 64, 1) == -1                          # 48 channels: not a whole 64-byte chunk in bf16
    assert conv(0, 1, 1, 4, 8, 24, 64, 1) == -1                          # ... nor 24 in fp32
    assert conv(1, 1, 1, 4, 8, 64, 48, 1) == -1                          # output channels in 32s
    assert conv(1, 2, 1, 20, 250, 128, 128, 1, True, 38, 499, 64) == -1  # x2 of 38 rows gives 19 at stride 2, not 20
    assert conv(1, 2, 1, 20, 250, 128, 128, 1, True, 40, 502, 64) == -1  # ... and 502 columns 251, not 250
    assert conv(1, 1, 1, 20, 250, 128, 128, 1, True, 40, 499, 64) == -3  # the direct kernel has no fused shortcut
    win = np.array([0, 3], np.int64)
    assert lib.rvb_test_emb_stem(0, f(z), 3 * 100 + 997, win.ctypes.data_as(_lib._i64p), 2, 4, 100, 998, 80, 32, f(z), f(z), f(z),
                                 f(z)) == -1                              # window 3 ends one row past the fbank
    assert lib.rvb_test_emb_stem(0, f(z), 3 * 100 + 998, win.ctypes.data_as(_lib._i64p), 2, 3, 100, 998, 80, 32, f(z), f(z), f(z),
                                 f(z)) == -1                              # window 3 of 3
    assert lib.rvb_test_emb_stem(0, f(z), 3 * 100 + 998, win.ctypes.data_as(_lib._i64p), 2, 4, 100, 998, 80, 24, f(z), f(z), f(z),
                                 f(z)) == -1                              # 24 stem channels


def test_attention_hook_refuses_out_of_range_arguments_before_any_device_work(lib):
    """rvb_test_attention_ex (tests/test_attention_kernels_gpu.py) checks every index, stride, offset and kv_index entry against the host
    buffer sizes (E_ARG = -1) before it looks for a device, so these hold with and without a GPU; `out` keeps its sentinel."""
    f, ip = _lib.fptr, _lib.iptr
    heads, dk, rows = 2, 64, 40
    d = heads * dk
    z = np.zeros((rows, 3 * d), np.float32)
    pz = np.zeros((rows, d), np.float32)
    bias = np.zeros(d, np.float32)
    base_i = dict(q_start=[0, 20], q_len=[20, 20], kv_start=[0, 20], kv_len=[20, 20])

    def call(ints=None, with_p=False, **kw):
        a = _lib.AttnTestArgs()
        out = np.full((rows, d), -77.0, np.float32)
        keep = [out]
        a.dtype, a.heads, a.dk, a.nseq = 1, heads, dk, 2
        for n, col in (("q", 0), ("k", d), ("v", 2 * d)):
            setattr(a, n, f(z)); setattr(a, n + "_rows", rows); setattr(a, n + "_stride", 3 * d); setattr(a, n + "_col", col)
        a.out, a.o_rows, a.o_stride, a.o_col = f(out), rows, d, 0
        if with_p:
            a.p, a.p_rows, a.p_stride, a.bias_u, a.bias_v = f(pz), rows, d, f(bias), f(bias)
        for n, val in dict(base_i, **(ints or {})).items():
            arr = np.ascontiguousarray(val, np.int32)
            keep.append(arr)
            setattr(a, n, ip(arr))
        for n, val in kw.items():
            if isinstance(val, (list, np.ndarray)):
                arr = np.ascontiguousarray(val, np.int32)
                keep.append(arr)
                val = ip(arr)
            setattr(a, n, val)
        rc = lib.rvb_test_attention_ex(ctypes.byref(a))
        assert np.all(out == -77.0) and not any(a.ran)
        return rc
    assert call(dict(q_len=[20, 21])) == -1                                   # queries past the last row of q / out
    assert call(dict(kv_len=[20, 21])) == -1                                  # keys past the last row of k / v
    assert call(dict(q_start=[-1, 20])) == -1
    assert call(v_col=2 * d + 8) == -1                                        # the last head's columns past the row
    assert call(k_col=d + 4) == -1                                            # not on a 16-byte boundary (bf16: 8 elements)
    assert call(o_col=2) == -1
    assert call(k_rows=rows - 1) == -1                                        # q and k name one buffer but disagree on its rows
    assert call(kv_index=[0, 1, 2], n_index=3) == -1                          # index list shorter than kv_start + kv_len
    assert call(kv_index=list(range(39)) + [40], n_index=40) == -1            # an entry past the last row
    assert call(kv_index=[-1] + list(range(39)), n_index=40) == -1
    assert call(work=[2, 0], n_work=1) == -1                                  # work item of a sequence that does not exist
    assert call(q_pos0=[0, -1]) == -1
    assert call(with_p=True, p_off=21) == -1                                  # positional rows 21 .. 41 of 40
    assert call(with_p=True, p_col=8) == -1
    assert call(with_p=True, bias_v=None) == -1                               # one bias without the other
    assert call(with_p=True, fold=1, fold_kv_cap=0) == -1                     # the fold's LDS table must cover every kv_len
    assert call(fold=1, fold_kv_cap=64) == -1                                 # fold without positional keys
    assert call(with_p=True, k_prefolded=1) == -1                             # prefolded keys without the fold
    assert call(dtype=2) == -1
    assert lib.rvb_test_attention_ex(None) == -1
    assert lib.rvb_test_attention_pos_bias(f(pz), rows, d, 8, 0, f(bias), f(bias), heads, dk, 1.0, f(pz)) == -1      # columns past the row
    assert lib.rvb_test_attention_pos_bias(f(pz), rows, d, 0, rows, f(bias), f(bias), heads, dk, 1.0, f(pz)) == -1   # no row left


def test_bad_arguments_are_reported_not_crashed(lib):
    cfg = _lib.ModelCfg()
    h = ctypes.c_void_p()
    assert lib.rvb_create(ctypes.byref(cfg), 0, ctypes.byref(h)) == -1      # RVB_E_ARG: all-zero dims
    assert b"unsupported model dimensions" in lib.rvb_last_error() or b"dtype" in lib.rvb_last_error()
    assert lib.rvb_create(None, 0, ctypes.byref(h)) == -1


def test_diarization_header_symbols_and_struct():
    """include/rvd.h (diarization networks): every declared function is exported and bound."""
    from reverb_amd import _lib as L
    lib = L.load()
    text = open(os.path.join(ROOT, "include", "rvd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = sorted(set(re.findall(r"\b(rvd_[a-z0-9_]+)\s*\(", code)))
    assert len(names) >= 14
    for n in names:
        assert hasattr(lib, n), f"librvb.so does not export {n}"
    assert sorted(L.DIAR_SIGNATURES) == names
    body = code[code.index("typedef struct rvd_model_cfg {"):code.index("} rvd_model_cfg;")]
    assert re.findall(r"int32_t\s+([a-z_0-9]+);", body) == [f[0] for f in L.DiarCfg._fields_]


@pytest.mark.skipif(HAVE_GPU, reason="checks the no-GPU failure mode")
def test_diarization_fails_loudly_without_gpu():
    from reverb_amd import synth_diar
    from reverb_amd.diar_engine import DiarEngine
    with pytest.raises(_lib.RvbError, match="no HIP device"):
        DiarEngine(synth_diar.make_diar_config(), {}, dtype="f32")


def test_compute_feats_refuses_what_the_kernel_does_not_cover():
    """host-side argument checks of rvb_compute_feats (no GPU needed for the frame count or the refusals)"""
    lib = _lib.load()
    n = ctypes.c_int64(-1)
    x = np.zeros(16000, np.float32)
    assert lib.rvb_compute_feats(0, _lib.fptr(x), x.size, 23, 25.0, 10.0, None, ctypes.byref(n)) == 0 and n.value == 98
    assert lib.rvb_compute_feats(0, _lib.fptr(x), x.size, 80, 32.0, 8.0, None, ctypes.byref(n)) == 0 and n.value == 1 + (16000 - 512) // 128
    for bins, flen, fshift in ((80, 10.0, 10.0), (80, 40.0, 10.0), (200, 25.0, 10.0), (80, 25.0, 0.0)):
        assert lib.rvb_compute_feats(0, _lib.fptr(x), x.size, bins, flen, fshift, None, ctypes.byref(n)) == -5      # RVB_E_UNSUPPORTED
        assert b"rvb_compute_feats" in lib.rvb_last_error()
