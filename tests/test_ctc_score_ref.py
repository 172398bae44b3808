"""The fp64 restatement of the CTC forward-backward recursions (tests/ctc_score_ref.py) against the reference's recorded losses, against
torch.nn.functional.ctc_loss, and against the identities of the posteriors; and the C ABI of the score calls."""
import json
import os
import re

import numpy as np
import pytest
import torch

import ctc_score_ref as R
import force_align_ref as A
from conftest import ROOT
from reverb_amd import _lib

GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "ctc_score.json")))
SMALL = [c for c in GOLD["cases"] if c["T"] <= 512]


@pytest.mark.parametrize("case", GOLD["cases"], ids=lambda c: "seed%d" % c["seed"])
def test_restatement_matches_the_references_ctc_loss(case):
    logits, y = R.make_logits(case["seed"], case["T"], case["V"], case["L"], case["scale"], case["repeats_at"])
    ll = R.loglik(R.log_softmax64(logits), y, GOLD["blank"])
    want = -float(case["loss"])
    assert abs(ll - want) <= 1e-10 * abs(want), (ll, want)


@pytest.mark.parametrize("case", GOLD["cases"], ids=lambda c: "seed%d" % c["seed"])
def test_restatement_matches_torch_ctc_loss(case):
    logits, y = R.make_logits(case["seed"], case["T"], case["V"], case["L"], case["scale"], case["repeats_at"])
    lp = torch.from_numpy(logits).double().log_softmax(1)
    loss = torch.nn.functional.ctc_loss(lp[:, None], torch.from_numpy(y.astype(np.int64))[None], torch.tensor([case["T"]]),
                                        torch.tensor([case["L"]]), blank=0, reduction="sum").item()
    ll = R.loglik(lp.numpy(), y, 0)
    assert abs(ll + loss) <= 1e-10 * abs(loss), (ll, -loss)


@pytest.mark.parametrize("case", SMALL, ids=lambda c: "seed%d" % c["seed"])
def test_posteriors_sum_to_one_per_frame_and_occupancies_to_T(case):
    lp, y = R.make_lattice(case["seed"], case["T"], case["V"], case["L"], case["scale"], case["repeats_at"])
    g, ll = R.gamma(lp, y)
    p = np.exp(g)
    assert np.abs(p.sum(1) - 1.0).max() < 1e-9
    assert abs(p.sum() - case["T"]) < 1e-9 * case["T"]
    red = R.reduce_tokens(g)
    assert abs(red["occupancy"].sum() + p[:, 0::2].sum() - case["T"]) < 1e-9 * case["T"]
    assert np.all(red["peak_post"] <= 1.0 + 1e-12) and np.all(red["peak_post"] >= red["second"])
    assert np.all((red["mean_frame"] >= 0) & (red["mean_frame"] <= case["T"] - 1))
    assert abs(R.forward(lp, y)[1] - R.loglik(lp, y)) < 1e-9


@pytest.mark.parametrize("case", SMALL, ids=lambda c: "seed%d" % c["seed"])
def test_loglik_is_at_least_the_viterbi_score(case):
    lp, y = R.make_lattice(case["seed"], case["T"], case["V"], case["L"], case["scale"], case["repeats_at"])
    assert R.loglik(lp, y) >= A.optimum64(lp, y) - 1e-12


@pytest.mark.parametrize("L,rep", [(1, ()), (5, (2,)), (40, (1, 2, 17)), (300, (150,))])
def test_one_feasible_path_makes_loglik_the_viterbi_score(L, rep):
    T = L + len(rep)
    lp, y = R.make_lattice(77, T, 32, L, 1.0, rep)
    assert A.min_frames(y) == T
    ll, red = R.score(lp, y)
    assert abs(ll - A.optimum64(lp, y)) <= 1e-12 * abs(ll)
    assert np.abs(red["occupancy"] - 1.0).max() < 1e-9 and np.abs(red["peak_post"] - 1.0).max() < 1e-9


def _declared(header, pattern):
    text = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(pattern, text, flags=re.S)}


def test_score_calls_are_exported_with_the_documented_arguments():
    pub = _declared(os.path.join(ROOT, "include", "rvb.h"), r"\b(rvb_ctc_score)\s*\(([^)]*)\)")
    assert len(pub["rvb_ctc_score"].split(",")) == 11 == len(_lib.SIGNATURES["rvb_ctc_score"][1])
    lab = _declared(os.path.join(ROOT, "reverb_amd", "csrc", "test_api.h"), r"\b(rvb_test_ctc_score(?:_batch)?)\s*\(([^)]*)\)")
    assert len(lab["rvb_test_ctc_score"].split(",")) == 12 == len(_lib.TEST_SIGNATURES["rvb_test_ctc_score"][1])
    assert len(lab["rvb_test_ctc_score_batch"].split(",")) == 13 == len(_lib.TEST_SIGNATURES["rvb_test_ctc_score_batch"][1])
    product, tlib = _lib.load(), _lib.load_test()
    assert hasattr(product, "rvb_ctc_score") and hasattr(tlib, "rvb_ctc_score")
    assert hasattr(tlib, "rvb_test_ctc_score") and hasattr(tlib, "rvb_test_ctc_score_batch")
    assert not hasattr(product, "rvb_test_ctc_score")


def test_score_refuses_what_the_aligner_refuses_before_any_device_work():
    """the refusals of CtcAligner::plan, in the same words after the caller's name; no GPU is needed to reach them"""
    tlib = _lib.load_test()
    lp = np.zeros((4, 8), np.float32)
    ll = np.zeros(1, np.float64)
    lab = np.zeros(4, np.int32)
    sc = np.zeros(1, np.float32)

    def both(tokens, T=4):
        tok = np.asarray(tokens if len(tokens) else [0], np.int32)
        r1 = tlib.rvb_test_ctc_viterbi(_lib.fptr(lp), T, 8, _lib.iptr(tok), len(tokens), 0, 4, _lib.iptr(lab), _lib.fptr(sc))
        e1 = tlib.rvb_last_error().decode()
        r2 = tlib.rvb_test_ctc_score(_lib.fptr(lp), T, 8, _lib.iptr(tok), len(tokens), 0, 4, _lib.dptr(ll), None, None, None, None)
        e2 = tlib.rvb_last_error().decode()
        return r1, e1, r2, e2

    for tokens, T in (([], 4), ([9], 4), ([0], 4), ([1, 1, 1], 4), ([1, 2, 3, 4, 5], 4), ([1] * 16384, 4), ([1], (1 << 20) + 1)):
        r1, e1, r2, e2 = both(tokens, T)
        assert r1 != 0 and r2 == r1, (tokens[:4], r1, r2)
        assert e1.startswith("rvb_test_ctc_viterbi: ") and e2.startswith("rvb_test_ctc_score: ")
        assert e1[len("rvb_test_ctc_viterbi: "):] == e2[len("rvb_test_ctc_score: "):]
