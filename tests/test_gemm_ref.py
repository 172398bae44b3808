"""No GPU: the bound of tests/gemm_ref.py against a float32 numpy emulation of the GEMM kernels' rounding points, on every case
tests/test_gemm_forms_gpu.py runs.  The emulation stays under the bound everywhere; every named mutant of it (a deliberately
broken kernel, gemm_ref.emulate) exceeds the bound by more than the factor 5 the attention tests ask for, on every case where
the mutant changes anything.  Both figures are printed (pytest -s); as committed: emulation 0.986 at worst (bf16 outputs, where
half an ulp of the output is nearly the whole bound; 0.012 with fp32 output), mutants from 62.6 (one dropped 8-element vector out
of K = 1216) upwards: bias_shift >= 1030, alpha_first >= 1107, row_k >= 4043, res_ldc >= 44936, inplace_after >= 335214, store_n
leaves elements unwritten.  Also here: what rvb_test_gemm_ex refuses before it touches
a device, and that the reference of the overlapping-row cases is the Conv1d it stands for."""
import ctypes

import numpy as np
import pytest

import gemm_ref as G
from reverb_amd import _lib
from reverb_amd._lib import fptr

CASES = G.all_cases()
MARGIN = 5.0


_MEASURED = {}


def _measure(case):
    """(emulation's worst err / bound, {mutant: its worst err / bound} for the mutants that apply), computed once per case"""
    key = G.case_id(case)
    if key not in _MEASURED:
        ref, bnd = G.reference(case), G.bound(case)
        assert ref.shape == (case["M"], case["N"]) and bnd.shape == ref.shape and (bnd > 0).all()
        got = G.emulate(case)
        assert np.isnan(got[:, case["N"]:]).all()                  # the emulation stores nothing into the pad columns either
        _MEASURED[key] = (G.ratio(got, ref, bnd), {m: G.ratio(G.emulate(case, m), ref, bnd) for m in G.MUTANTS if G.applies(m, case)})
    return _MEASURED[key]


@pytest.mark.parametrize("case", CASES, ids=[G.case_id(c) for c in CASES])
def test_bound_holds_for_the_emulated_kernel_and_fails_for_every_mutant(case):
    good, muts = _measure(case)
    print("%s: emulation worst err / bound %.3f" % (G.case_id(case), good))
    assert good < 1.0
    for mut, r in muts.items():
        print("%s: mutant '%s' worst err / bound %.1f" % (G.case_id(case), mut, r))
        assert r > MARGIN, "the bound would not notice '%s' on %s (ratio %.2f)" % (mut, G.case_id(case), r)


def test_every_mutant_is_caught_somewhere():
    """every mutant meets at least one case, and the figures of the whole file in one place"""
    res = [_measure(c) for c in CASES]
    good = max(g for g, _ in res)
    print("emulation: worst err / bound over %d cases %.3f" % (len(CASES), good))
    assert 0.0 < good < 1.0
    for mut in G.MUTANTS:
        rs = [m[mut] for _, m in res if mut in m]
        assert rs, "no case exercises mutant '%s'" % mut
        print("mutant '%s': %d cases, err / bound %.1f .. %.1f" % (mut, len(rs), min(rs), max(rs)))
        assert min(rs) > MARGIN


def test_paths_of_the_cases_are_the_ones_their_forms_name():
    """gemm2_applicable's conditions, mirrored in gemm_ref: which kernel family each form reaches (the GPU file asserts the same
    against what the hook reports)"""
    by = {}
    for c in CASES:
        by.setdefault((c["form"], c["dtype"], c["M"], c["N"], c["K"]), G.expected_path(c))
    assert by[("inplace", G.BF16, 512, 512, 128)] == 2 and by[("inplace", G.BF16, 40, 256, 128)] == 1
    assert by[("overlap", G.BF16, 300, 64, 320)] == 2 and by[("overlap", G.BF16, 300, 64, 400)] == 1       # K = 400 is no multiple of 64
    assert by[("lrelu", G.BF16, 200, 128, 256)] == 1                                                       # gemm2 turns LeakyReLU away
    assert by[("cut", G.BF16, 127, 192, 128)] == 1 and by[("cut", G.BF16, 128, 192, 128)] == 2
    assert by[("cut", G.BF16, 256, 63, 128)] == 1 and by[("cut", G.BF16, 256, 64, 128)] == 2
    assert by[("long_k", G.BF16, 300, 128, 1216)] == 2 and by[("logits", G.BF16, 300, 1001, 128)] == 2
    assert all(p == 1 for (f, dt, *_), p in by.items() if dt == G.F32)


@pytest.mark.parametrize("case", G.overlap_cases(), ids=[G.case_id(c) for c in G.overlap_cases()])
def test_overlapping_row_reference_is_conv1d(case):
    """lda = cin, K = 5 cin: row m of A is frames m .. m + 4 of a [frames][cin] tensor, so the GEMM is Conv1d(cin, 64, 5) over it"""
    import torch
    cin = case["lda"]
    frames = case["A"].size // cin
    x = torch.from_numpy(case["A"].astype(np.float64).reshape(frames, cin).T.copy())[None]
    w = torch.from_numpy(case["W"].astype(np.float64).reshape(case["N"], 5, cin).transpose(0, 2, 1).copy())
    b = torch.from_numpy(case["bias"].astype(np.float64)) if case["bias"] is not None else None
    y = torch.nn.functional.conv1d(x, w, b)[0].T.numpy()
    assert y.shape == (case["M"], case["N"])
    np.testing.assert_allclose(G.reference(case), y, rtol=1e-12, atol=1e-12)


def test_hook_refuses_undersized_buffers_before_any_device_work(lib):
    """rvb_test_gemm_ex checks the buffers against the strides first (E_ARG by name), GPU or not"""
    z = np.zeros(64 * 64, np.float32)

    def call(**kw):
        a = _lib.GemmTestArgs()
        a.dtype, a.M, a.N, a.K, a.lda, a.ldw, a.ldc, a.ldres, a.alpha, a.out_f32 = 1, 8, 8, 8, 8, 8, 8, 8, 1.0, 1
        a.a_elems = 64
        a.A, a.W, a.C = fptr(z), fptr(z), fptr(z)
        for k, v in kw.items():
            setattr(a, k, v)
        rc = lib.rvb_test_gemm_ex(ctypes.byref(a))
        return rc, lib.rvb_last_error()

    assert lib.rvb_test_gemm_ex(None) == G.E_ARG
    for kw, word in (({"a_elems": 63}, b"a_elems"), ({"a_row0": 1}, b"a_elems"), ({"lda": 4, "a_elems": 35}, b"a_elems"),
                     ({"ldw": 7}, b"ldw < K"), ({"ldc": 7}, b"ldc < N"), ({"c_rows": 7}, b"c_rows < M"), ({"a_row0": -1}, b"negative"),
                     ({"res": fptr(z), "ldres": 7}, b"ldres < N"), ({"inplace": 1, "out_f32": 0}, b"inplace"),
                     ({"inplace": 1, "res": fptr(z)}, b"inplace"), ({"in_fp8": 1}, b"a_scale"), ({"out_fp8": 1}, b"fp8 output"),
                     ({"dtype": 2}, b"dtype"), ({"A": None}, b"null")):
        rc, msg = call(**kw)
        assert rc == G.E_ARG and msg.startswith(b"rvb_test_gemm_ex: ") and word in msg, (kw, rc, msg)
