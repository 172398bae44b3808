"""CPU tests of the bf16-storage restatement of the rescoring decoder (oracle/dec_bf16_ref.py) and of the stage check the GPU test runs
on the engine's taps (tests/dec_bf16_checks.py):

  * the transcripts make the trie non-trivial and send every GEMM of both decoders to gemm2 (the engine's conditions restated);
  * with storage 'none' the restatement on the trie IS oracle/model_ref.py's decoder run one sequence at a time: every sequence reads
    what it would read alone;
  * on the restatement's own stored tensors the stage check passes at every position of both decoders;
  * deliberately wrong decoders (dec_bf16_ref.MUTANTS) are caught at the stage they touch and at no other;
  * on the oracle alone, at most 2 % of the target positions have a top-2 logit gap below the log-prob bound the GPU test holds
    the engine to (1.25 x the restatement's own worst |logp - oracle|), which is what lets the arg-max be compared.
No GPU."""
import json

import numpy as np
import pytest

import asr_bf16_checks as AC
import dec_bf16_checks as C
from oracle import asr_bf16_ref as A
from oracle import dec_bf16_ref as Dc

# the stage(s) a mutant touches, and the positions it is checked at
TOUCHES = {"trunc": "kvmem xn1 qkv xn2 q xn3 y h xn_after".split(), "sibling": ["ao_self"], "causal_plus1": ["ao_self"],
           "q_from_xn1": ["q"], "kv_unrounded_mem": ["kvmem"], "lang_swapped": ["y"], "no_relu": ["h"], "right_unreversed": ["trie"]}


@pytest.fixture(scope="module")
def case():
    cfg, sd, feats, lens = AC.small_case(0)
    taps = {}
    enc, _ = A.encoder_bf16(sd, cfg, feats, lens, AC.CAT, taps=taps)
    nb = A.dims(cfg, feats.shape[1])["blocks"]
    after = (np.asarray(sd["encoder.after_norm.weight"], np.float64), np.asarray(sd["encoder.after_norm.bias"], np.float64))
    raw = A.EW.layer_norm(taps[nb - 1]["x_out"], after[0], after[1], 1e-5).reshape(enc.shape)
    assert np.abs(raw - enc).max() < 2.0 ** -7 * np.abs(raw).max() and not np.array_equal(raw, enc)
    seqs, chunk_of = C.transcripts()
    eos = cfg["output_dim"] - 1
    c = dict(cfg=cfg, sd=sd, mem=enc, mem_raw=raw, enc_lens=A.enc_lens(lens), seqs=seqs, chunk_of=chunk_of, eos=eos, s64=C.sd64(sd), trie={},
             W={}, oracle={}, tg={})
    for side in Dc.SIDES:
        c["trie"][side] = C.build_trie(seqs, chunk_of, 2, eos, eos, side == "right_decoder")
        c["W"][side] = Dc.load_weights(sd, cfg, side, C.CAT)
        c["oracle"][side] = C.oracle_logits(c["s64"], cfg, side, enc, c["enc_lens"], seqs, chunk_of)
        c["tg"][side] = C.targets(seqs, side, eos)
    return c


def test_transcripts_make_the_trie_non_trivial_and_select_gemm2(case):
    """shared prefix, a single token, a hypothesis whose owned rows span three 16-query blocks, a duplicate that owns no row; R >= 128 in
    both directions, so that every GEMM of a layer and the output layer run on gemm2 (M >= 128, N >= 64, K % 64 == 0) -- from the
    engine's own conditions restated on the CPU; the GPU test asserts them on the `forms` tap."""
    t = case["trie"]["left_decoder"]
    lens = [len(s) for s in case["seqs"]]
    assert lens == [40, 28, 28, 28, 1, 30, 30, 35] and case["seqs"][5] == case["seqs"][6]
    assert t["hq_len"].tolist() == [41, 8, 8, 8, 1, 31, 0, 35] and t["hq_pos0"].tolist()[:4] == [0, 21, 21, 21]
    assert len(t["tok"]) == 132 and t["crow_len"].tolist() == [66, 66]
    assert t["work"].reshape(-1, 2).tolist() == [[0, 0], [0, 16], [0, 32], [1, 0], [2, 0], [3, 0], [4, 0], [5, 0], [5, 16], [7, 0], [7, 16], [7, 32]]
    D = Dc.dims(case["cfg"])
    assert (D["d"], D["dk"], D["ff"], D["layers"], D["r_layers"], D["V"], D["Vld"]) == (256, 64, 256, 3, 3, 500, 500)
    for side in Dc.SIDES:
        R = len(case["trie"][side]["tok"])
        assert R >= 128
        for pos in range(4):
            is_lsl = pos < 3 and case["W"][side]["layers"][pos]["is_lsl"]
            assert is_lsl == (pos in (0, 2))
            f = C.decode_forms(Dc.expected_forms(case["cfg"], R, pos, is_lsl), pos, 3, is_lsl)
            assert all(v == 2 for v in f["gemm"].values()), (side, pos, f)
            if pos < 3:
                assert f["attention"] == {"self": [2, 64, 0, 1, 0, 32, 1, 1], "src": [2, 64, 0, 8, 0, 32, 1, 1]}
    assert len(case["trie"]["right_decoder"]["tok"]) > 132       # reversed: the shared prefix is a suffix and shares nothing


@pytest.mark.parametrize("side", Dc.SIDES)
def test_without_rounding_the_restatement_is_the_oracles_decoder_per_sequence(case, side):
    """storage 'none': fp64 arithmetic of the same network on the trie; the oracle runs each sequence alone on its chunk's valid frames.
    Both are fp64: they differ by summation order only (logits of order 1 to 10, sums of 256 terms), held to 1e-9."""
    lg, lp = Dc.decoder_bf16(case["sd"], case["cfg"], side, case["trie"][side], case["mem"], case["enc_lens"], C.CAT, storage="none")
    worst = max(float(np.abs(a - b).max()) for a, b in zip(C.per_sequence(case["trie"][side], lg), case["oracle"][side]))
    m = C.restatement_figures(case["sd"], case["cfg"], side, case["trie"][side], case["mem"], case["enc_lens"], case["oracle"][side],
                              case["tg"][side], storage="none")
    print("%s, storage none: max |logits - oracle| %.3g, figures %s" % (side, worst, json.dumps(m)))
    assert worst < 1e-9 and m["max_dlogp"] < 1e-9 and m["argmax_diff"] == 0


@pytest.mark.parametrize("side", Dc.SIDES)
def test_stage_check_passes_on_the_restatements_own_tensors(case, side):
    taps = {}
    Dc.decoder_bf16(case["sd"], case["cfg"], side, case["trie"][side], case["mem"], case["enc_lens"], C.CAT, taps=taps)
    for pos in range(4):
        T = dict(taps[pos], trie=taps["trie"])
        fig, bad = C.check_stages(case["W"][side], case["cfg"], T, pos, case["mem"], case["enc_lens"], case["trie"][side])
        print("%s position %d: %s" % (side, pos, json.dumps({k: round(v, 3) for k, v in fig.items()})))
        assert not bad, "\n".join(bad)
        want = ("trie",) + (Dc.HEAD_STAGES if pos == 3 else tuple(n for n in Dc.LAYER_STAGES if n != "y" or pos != 1)) + (("x_emb",) if pos == 0 else ())
        assert set(fig) == set(want)


@pytest.mark.parametrize("mutant", Dc.MUTANTS)
def test_mutants_are_caught_at_the_stage_they_touch_and_at_no_other(case, mutant):
    """each wrong decoder's own stored tensors through the stage check, at the language-specific layer 0, the plain layer 1 and the
    head; the batch the check restates is the one the transcripts give (stage 'trie'), which is what notices un-reversed tokens.

    A finding about the bounds: truncation is caught at every GEMM and row-norm output (2 x to 20 x the bound), but NOT reliably at the
    two attention outputs: attention_ref._ref_bound allows the rounding of the probabilities (u) beside the output's (u) relative to
    sum w |v| >= |out|, and a truncated output errs by at most 2 u |out|.  Measured: ao_self 1.09 x / ao_src 1.00 x the bound at layer
    0, inside it at layer 1.  So ao_self / ao_src are not required of the truncation mutant; the wiring mutants of the attentions
    (sibling row, causal mask) are caught there by three orders of magnitude."""
    side = "right_decoder" if mutant == "right_unreversed" else "left_decoder"
    trie = case["trie"]["left_decoder"] if mutant == "right_unreversed" else case["trie"][side]
    taps = {}
    Dc.decoder_bf16(case["sd"], case["cfg"], side, trie, case["mem"], case["enc_lens"], C.CAT, taps=taps,
                    mutant=None if mutant == "right_unreversed" else mutant, memory_raw=case["mem_raw"])
    outside, figs = set(), {}
    for pos in (0, 1, 3):
        fig, _ = C.check_stages(case["W"][side], case["cfg"], dict(taps[pos], trie=taps["trie"]), pos, case["mem"], case["enc_lens"],
                                case["trie"][side])
        outside |= {k for k, v in fig.items() if v > 1.0}
        figs[pos] = {k: round(v, 3) for k, v in fig.items() if v > 1.0}
    print("%s: stages outside their bound %s" % (mutant, json.dumps(figs)))
    if mutant == "trunc":         # the weights are truncated too: every stage with a bf16 output or a bf16 weight moves
        assert set(TOUCHES[mutant]) <= outside, (mutant, sorted(outside))
    else:
        assert outside == set(TOUCHES[mutant]), (mutant, sorted(outside))


def test_oracle_keeps_near_ties_below_two_percent(case):
    """The arg-max of a position may legitimately differ where the oracle's two largest logits are closer than the log-prob bound the
    GPU test holds the engine to: 1.25 x the restatement's own worst |logp - oracle| over the plain and six jittered runs.  Such
    positions may be at most 2 % of the targets; dec_bf16_checks.TOKEN_SEED was chosen for it (measured: left 1, right 0 of 228
    positions; below TWICE the bound 7 and 2).  Oracle and restatement only."""
    for side in Dc.SIDES:
        yard, runs = C.yardstick(case["sd"], case["cfg"], side, case["trie"][side], case["mem"], case["enc_lens"], case["oracle"][side],
                                 case["tg"][side])
        bound = C.FACTOR * yard["max_dlogp"]
        gaps = np.concatenate([np.sort(lg, 1)[:, -1] - np.sort(lg, 1)[:, -2] for lg in case["oracle"][side]])
        near = float((gaps < bound).mean())
        print("%s: yardstick %s, log-prob bound %.3g, positions with a top-2 gap below it: %d of %d (below twice it: %d; median gap %.3g)"
              % (side, json.dumps(yard), bound, int((gaps < bound).sum()), gaps.size, int((gaps < 2 * bound).sum()), float(np.median(gaps))))
        for r in runs:
            assert not C.outside_yardstick(r, yard)
        assert near <= 0.02
