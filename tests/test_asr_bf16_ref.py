"""CPU tests of the bf16-storage restatement of the conformer encoder (oracle/asr_bf16_ref.py), of the stage check that the GPU test
runs on the engine's taps (tests/asr_bf16_checks.py) and of the yardstick fixture (tests/golden/asr_bf16_yardstick.json):

  * with storage 'none' the restatement IS the fp32 oracle's network (oracle/model_ref.py), in both GLU forms and both attention forms;
  * on the restatement's own stored tensors the stage check passes at every position, in both sets of forms;
  * deliberately wrong engines (asr_bf16_ref.MUTANTS) are caught by the stage check of the stage they touch; what the end-to-end
    yardstick bound and the older bounds (reference-autocast token edits + 1 %, cos > 0.995) make of each is printed and asserted
    where the measurement allows an assertion (see test_mutants);
  * the yardstick bound accepts every restatement run of every case, and the committed fixture is what the restatement gives.
No GPU."""
import json
import math
import os
import sys

import numpy as np
import pytest

import asr_bf16_checks as C
from oracle import asr_bf16_ref as A

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
import gen_golden_asr_bf16 as G          # noqa: E402

with open(os.path.join(HERE, "golden", "asr_bf16_yardstick.json")) as f:
    YARD = json.load(f)
NAME = "forms64_seed0"
FORMS = [dict(prefold=True, glu_fused=True), dict(prefold=False, glu_fused=False)]
FORM_IDS = ["prefolded-glu_fused", "two_product-glu_unfused"]
# the stage a mutant touches (None: an equivalent mutant, see test_mutants) and the positions checked for it
TOUCHES = {"trunc": "X1 xn0 h_ffm qkv glu dconv xn_cnn y next".split(), "trunc_dconv": ["dconv"], "kp_twice": ["qkv"], "glu_halves": ["glu"],
           "next_from_rounded": ["next"], "p_before_max": None}


@pytest.fixture(scope="module")
def case():
    c = G.make_case(NAME)
    c["W"] = A.load_weights(c["sd"], c["cfg"], C.CAT, 150)
    return c


def test_small_model_selects_the_benchmarks_forms():
    """gemm2 for every GEMM (M = 300 >= 128 rows, K % 64 == 0), GLU in the epilogue, the key pre-folded (32 < dk = 64 <= 64), from the
    engine's own conditions restated on the CPU; a lone chunk (M = 150) selects them too.  The GPU test asserts them on the `forms` tap."""
    cfg = C.small_case(0)[0]
    for lens in (C.LENS, C.LENS[1:]):
        f = C.forms_of(cfg, lens)
        assert f["prefold"] and f["glu_fused"] and all(f["gemm2"].values()), f
    D = A.dims(cfg, C.CHUNK_FRAMES)
    assert (D["T2"], D["dk"], D["blocks"], D["K"]) == (150, 64, 3, 31) and A.enc_lens(C.LENS).tolist() == [150, 83]


@pytest.mark.parametrize("forms", FORMS, ids=FORM_IDS)
def test_without_rounding_the_restatement_is_the_oracles_network(case, forms):
    """storage 'none': fp64 arithmetic of the same network.  The fp32 oracle's own rounding is what separates them: over the valid
    frames 2.5e-6 on encoder_out (values of order 1 after a LayerNorm; 3 blocks of fp32 sums of up to 4864 terms) and 2e-5 on the
    log-probabilities (the CTC head's weights carry a factor 8); held to four times those."""
    enc, logp = A.encoder_bf16(case["sd"], case["cfg"], case["feats"], case["lens"], C.CAT, storage="none", forms=forms)
    valid = np.arange(enc.shape[1])[None, :] < A.enc_lens(case["lens"])[:, None]
    de, dl = np.abs(enc - case["enc"])[valid].max(), np.abs(logp - case["logp"])[valid].max()
    print("storage none, %r: max |encoder_out - oracle| %.3g, max |logp - oracle| %.3g" % (forms, de, dl))
    assert de < 1e-5 and dl < 8e-5


@pytest.mark.parametrize("forms", FORMS, ids=FORM_IDS)
def test_stage_check_passes_on_the_restatements_own_tensors(case, forms):
    taps = {}
    A.encoder_bf16(case["sd"], case["cfg"], case["feats"], case["lens"], C.CAT, taps=taps, forms=forms)
    for block in (3, 0, 1, 2):
        fig, bad = C.check_stages(case["sd"], case["cfg"], case["feats"], case["lens"], taps if block == 3 else taps[block], block, forms, case["W"])
        print("position %d: %s" % (block, json.dumps({k: round(v, 3) for k, v in fig.items()})))
        assert not bad, "\n".join(bad)
        assert set(fig) == set(C.FRONT_STAGES if block == 3 else [n for n in C.BLOCK_STAGES if n != "y" or block != 1])


@pytest.mark.parametrize("mutant", A.MUTANTS)
def test_mutants(case, mutant):
    """Each deliberately wrong engine against (a) the stage check, (b) the end-to-end yardstick bound, (c) the older bounds.

    (a) is asserted for every mutant: the stage it touches falls outside its bound, at a language-specific and at a plain block, and
        no other stage does (truncation everywhere: every bf16 stage it touches).
    (b) Measured (weights seed 0; factor = mutant's enc_rel_l2 / yardstick's): truncation everywhere 2.10, the second norm fed the
        rounded x_out 1.053, GLU rounded as two halves 1.012, k + p rounded twice 1.002, dconv alone truncated 0.998.  A single extra
        rounding among the ~17 stored tensors of a block moves the end-to-end figures by about a percent, which no end-to-end bound
        can tell from another summation order (the seven yardstick runs spread by 0.4 % on enc_rel_l2, by 30 % on the log-prob
        maxima).  So (b) is asserted for the two the bound resolves -- truncation and the mis-fed norm, the latter only through the
        tightened encoder_out factors of asr_bf16_ref.outside_yardstick -- and printed for the others, which the stage check alone
        catches.  That is the reason the GPU test runs the stage check at all.
    (c) is printed only (measured: they notice none: token edits within the reference-autocast's + 1 %, cos > 0.995).
    p_before_max is an EQUIVALENT mutant: rounding exp2(score) before or after the power-of-two-free shift by the row maximum costs
    the same one bf16 rounding per probability; the attention bound carries that rounding (u_p), and nothing can catch it."""
    y = YARD["cases"][NAME]
    taps = {}
    enc, logp = A.encoder_bf16(case["sd"], case["cfg"], case["feats"], case["lens"], C.CAT, taps=taps, mutant=mutant)
    forms = FORMS[0]
    outside = set()
    for block in (3, 0, 1) if mutant == "trunc" else (0, 1):
        fig, _ = C.check_stages(case["sd"], case["cfg"], case["feats"], case["lens"], taps if block == 3 else taps[block], block, forms, case["W"])
        outside |= {k for k, v in fig.items() if v > 1.0}
    m = A.metrics(enc, logp, case["enc"], case["logp"], case["lens"])
    beyond = A.outside_yardstick(m, y["yardstick"])
    edits = G.token_edits(logp, case["tokens"], case["lens"])
    old_edit_bound = y["autocast_greedy_token_edits"] + math.ceil(0.01 * y["reference_tokens"])
    old_notice = edits > old_edit_bound or 1.0 - m["enc_one_minus_cos"] <= 0.995
    print("%s: stages outside their bound %s; beyond the yardstick bound %s (enc_rel_l2 x %.3f of the yardstick); older bounds: %d token "
          "edits (bound %d), cos %.6f (bound 0.995) -> %s" % (mutant, sorted(outside), beyond, m["enc_rel_l2"] / y["yardstick"]["enc_rel_l2"], edits,
                                                             old_edit_bound, 1.0 - m["enc_one_minus_cos"], "noticed" if old_notice else "NOT noticed"))
    if TOUCHES[mutant] is None:
        assert not outside and not beyond, "an equivalent mutant"
        return
    if mutant == "trunc":
        assert set(TOUCHES[mutant]) <= outside
    else:
        assert set(TOUCHES[mutant]) == outside
    if mutant in ("trunc", "next_from_rounded"):
        assert "enc_rel_l2" in beyond


def test_yardstick_bound_accepts_every_restatement_run_and_the_fixture_is_reproducible(case):
    assert YARD["jitters"] == 6 and sorted(YARD["cases"]) == ["forms64_bn", "forms64_seed0", "forms64_seed1", "r640_chunk"]
    for name, c in YARD["cases"].items():
        assert len(c["runs"]) == c["runs_made"] == 7
        for run, m in c["runs"].items():
            assert not A.outside_yardstick(m, c["yardstick"]), (name, run)
    m = G.restatement_metrics(case)
    want = YARD["cases"][NAME]["runs"]["plain"]
    for k in A.COUNTS:
        assert m[k] == want[k]
    for k in A.MEANS:
        assert abs(m[k] - want[k]) <= 1e-9 + 1e-6 * want[k], k
