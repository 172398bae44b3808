"""Attention-decoder loss and accuracy through the engine (rvb_attention_score / Engine.score(attention=True) / ReverbASR.score /
bin/get_loss) on the synthetic model: "tiny", f32, two chunks of 30 s of audio, and one short chunk of "tiny_v10k" for the padded
logit stride (V = 10001 in rows of 10004).

Reference: oracle.model_ref.decoder_forward in float64 on the engine's OWN encoder_out()[b, :len], transcript = the chunk's greedy
tokens, so only the decoder is under test; loss and accuracy from tests/att_score_ref.py on the oracle's logits.

ATT_LOGP_BOUND: the per-position bound on att_logp against the oracle's log-softmax at the targets.  It is not known in advance: the
maximum measured on an MI355X is 1.22e-6 (f32; 6.34e-7 over both chunks and both decoders of "tiny", 1.22e-6 on the tiny_v10k chunk,
whose log-probs near -9.8 have a unit in the last place of 9.5e-7), asserted at 4 times that, 4.9e-6, far below the 2e-3 that
tests/test_engine_gpu.py allows the rescoring's per-token confidences.  Every comparison prints its maximum.  loss_att is a sum
over L + 1 positions of terms that are each within the bound (plus the smoothing terms, which move by less: att_score_ref.compose), so
it is held to (L + 1) times the bound.  n_correct equals the oracle's except at positions where the oracle's two largest logits are
closer than the measured log-prob error; those may be at most 2 % of the positions, which the test checks on the oracle alone.

bf16: tests/test_engine_gpu.py bounds no log-prob of its bf16 rescoring (it counts token edits), so the bound is derived here: every
decoder activation is rounded to bf16 (unit roundoff 2^-9) at about 8 places per layer, 3 layers, plus the embedding, the final norm
and the output weights: 27 roundings in sequence, each relative to an O(1) LayerNorm-ed activation, move a logit by at most
27 * 2^-9 of the largest |logit|, and a log-prob (logit minus lse) by twice that (0.22 - 0.25 here; measured 3.3e-3)."""
import json
import os

import numpy as np
import pytest
import torch

import att_score_ref as R
from oracle import model_ref as M
from reverb_amd import synth
from reverb_amd._lib import RvbError
from reverb_amd.engine import Engine

pytestmark = pytest.mark.gpu
CHUNK = 2051
ATT_LOGP_BOUND = 4.9e-6
assert ATT_LOGP_BOUND <= 2e-3
LSM, RW = 0.1, 0.3


def _encode(eng, seconds, seed, beam=4):
    eng.upload_pcm(synth.synth_audio(seconds, seed=seed))
    n = eng.fbank()
    nch = -(-n // CHUNK)
    lens = np.full(nch, CHUNK, np.int32)
    lens[-1] = n - (nch - 1) * CHUNK
    eng.encode(None, lens, beam, 0.0, T0=CHUNK)
    return nch


def _oracle(sd64, cfg, eng, b, y, side):
    """fp64 logits [L + 1, V] of decoder `side` for inputs [sos] + y over chunk b's valid frames, and the targets y + [eos]."""
    sos = eos = cfg["output_dim"] - 1
    n = int(eng.encoder_lens()[b])
    mem = torch.from_numpy(eng.encoder_out()[b, :n]).double()[None]
    seq = list(y) if side == "left_decoder" else list(y)[::-1]
    ys_in = torch.tensor([[sos] + seq])
    out = M.decoder_forward(sd64, cfg, side, mem, torch.ones(1, 1, n, dtype=torch.bool), ys_in, torch.tensor([len(seq) + 1]),
                            torch.tensor([1.0, 0.0], dtype=torch.float64))
    return out[0].numpy(), np.array(seq + [eos])


def _sd64(sd):
    return {k: (v.double() if v.dtype.is_floating_point else v) for k, v in M.to_torch_sd(sd).items()}


@pytest.fixture(scope="module")
def tiny():
    cfg, sd = synth.calibrated_state_dict("tiny")
    eng = Engine(cfg, sd, dtype="f32", device=0, max_chunks=4, chunk_frames=CHUNK)
    assert _encode(eng, 30.0, 21) == 2
    toks = [g.tokens for g in eng.greedy()]
    assert all(toks)
    ref = {(b, side): _oracle(_sd64(sd), cfg, eng, b, toks[b], side) for b in range(2) for side in ("left_decoder", "right_decoder")}
    yield eng, toks, ref, cfg, sd
    eng.close()


def _check_against_oracle(got, ref_l, ref_r, V, bound):
    """One sequence: att_logp, loss sums and n_correct of both decoders against the oracle's logits."""
    worst = 0.0
    for logits, tgt, lp, loss in ((*ref_l, got["logp_l"], got["loss_l"]), (*ref_r, got["logp_r"], got["loss_r"])):
        want = R.log_softmax(logits)[np.arange(len(tgt)), tgt]
        err = float(np.abs(lp - want).max())
        worst = max(worst, err)
        print("V %d L+1 %d: max |att_logp - oracle| %.3g (bound %.3g)" % (V, len(tgt), err, bound))
        assert err <= bound, err
        want_loss = float(R.kl_dense(logits, tgt, LSM).sum())
        assert abs(loss - want_loss) <= len(tgt) * bound, (loss, want_loss)
    logits, tgt = ref_l
    top = np.sort(logits, axis=1)
    near = (top[:, -1] - top[:, -2]) < 2 * bound          # the arg-max may legitimately differ there
    assert near.mean() <= 0.02, "the oracle alone must keep near-ties below 2 % of the positions"
    pred = logits.argmax(axis=1)
    assert np.array_equal(got["top1_l"][~near], pred[~near])
    assert abs(got["n_correct"] - int((pred == tgt).sum())) <= int(near.sum())
    assert got["n_positions"] == len(tgt)
    return worst


def test_logp_loss_and_accuracy_match_the_fp64_decoder_per_chunk(tiny):
    eng, toks, ref, cfg, _ = tiny
    got = eng.attention_score(toks, [0, 1], reverse_weight=RW, lsm_weight=LSM)
    worst = max(_check_against_oracle(got[b], ref[b, "left_decoder"], ref[b, "right_decoder"], cfg["output_dim"], ATT_LOGP_BOUND)
                for b in range(2))
    print("max |att_logp - oracle| %.3g (asserted %.3g), positions %s, n_correct %s"
          % (worst, ATT_LOGP_BOUND, [g["n_positions"] for g in got], [g["n_correct"] for g in got]))
    # without the right decoder: the left results carry the same bits, loss_r is 0
    left = eng.attention_score(toks, [0, 1], reverse_weight=0.0, lsm_weight=LSM)
    for a, b in zip(left, got):
        assert a["loss_l"] == b["loss_l"] and a["loss_r"] == 0.0 and np.array_equal(a["logp_l"], b["logp_l"])
    # smoothing 0: the loss is the negative sum of the log-probs
    plain = eng.attention_score(toks, [0, 1], reverse_weight=0.0, lsm_weight=0.0)
    for a in plain:
        assert abs(a["loss_l"] + float(a["logp_l"].astype(np.float64).sum())) <= 1e-9 * a["n_positions"]


def test_two_candidates_of_one_chunk_share_the_trie_and_keep_their_bits(tiny):
    eng, toks, ref, cfg, sd = tiny
    y = list(toks[0])
    # The synthetic decoder is untrained: it does not prefer the greedy transcript to an arbitrary edit of it.  The wrong candidate is
    # therefore built from the oracle: it keeps the first half (a shared prefix for the trie) and continues with the token the
    # oracle's left decoder finds LEAST likely at each position; the oracle itself must rank it at least 1 nat above the true one.
    base = ref[0, "left_decoder"][0]
    wrong = y[:len(y) // 2] + [int(base[j].argmin()) for j in range(len(y) // 2, len(y))]
    s64 = _sd64(sd)

    def oracle_att(seq):
        l, r = (float(R.kl_dense(*_oracle(s64, cfg, eng, 0, seq, side), LSM).sum()) for side in ("left_decoder", "right_decoder"))
        return (1 - RW) * l + RW * r
    margin = oracle_att(wrong) - oracle_att(y)
    print("oracle: loss_att of the wrong candidate is %.3f nats above the true one" % margin)
    assert margin > 1.0
    both = eng.attention_score([y, wrong, toks[1]], [0, 0, 1], reverse_weight=RW, lsm_weight=LSM)
    alone = [eng.attention_score([s], [c], reverse_weight=RW, lsm_weight=LSM)[0] for s, c in ((y, 0), (wrong, 0), (toks[1], 1))]
    for a, b in zip(both, alone):
        assert a["loss_l"] == b["loss_l"] and a["loss_r"] == b["loss_r"] and a["n_correct"] == b["n_correct"]
        assert np.array_equal(a["logp_l"], b["logp_l"]) and np.array_equal(a["logp_r"], b["logp_r"])
        assert np.array_equal(a["top1_l"], b["top1_l"])
    att = [(1 - RW) * r["loss_l"] + RW * r["loss_r"] for r in both]
    assert att[0] < att[1], "the true transcript must score the lower loss_att"
    assert abs((att[1] - att[0]) - margin) <= 2 * (len(y) + 1) * ATT_LOGP_BOUND
    # the order of the sequences in the call does not matter either
    swapped = eng.attention_score([toks[1], wrong, y], [1, 0, 0], reverse_weight=RW, lsm_weight=LSM)
    assert swapped[2]["loss_l"] == both[0]["loss_l"] and swapped[0]["loss_r"] == both[2]["loss_r"]


def test_scoring_between_search_and_rescoring_leaves_the_rescoring_as_it_was(tiny):
    eng, toks, _, _, _ = tiny

    def run(score_between):
        pref = eng.prefix_beam()
        if score_between:
            eng.attention_score(toks, [0, 1], reverse_weight=RW, lsm_weight=LSM)
        res = eng.rescore(pref, 0.3, RW)
        return pref, res, eng.rescore_stats()
    (p0, r0, s0), (p1, r1, s1) = run(False), run(True)
    assert s0 == s1
    for a, b in zip(p0, p1):
        assert a.nbest == b.nbest and a.nbest_scores == b.nbest_scores
    for a, b in zip(r0, r1):
        assert tuple(a.tokens) == tuple(b.tokens) and a.score == b.score and a.confidence == b.confidence
        assert a.tokens_confidence == b.tokens_confidence


def test_refusals_are_raised_by_name(tiny):
    eng, toks, _, cfg, sd = tiny
    V = cfg["output_dim"]
    with pytest.raises(RvbError, match=r"rvb_attention_score: sequence 1: token id %d outside \[0, %d\)" % (V, V)):
        eng.attention_score([toks[0], [1, V]], [0, 1])
    with pytest.raises(RvbError, match="sequence 0: token id -1 outside"):
        eng.attention_score([[-1]], [0])
    with pytest.raises(RvbError, match="sequence 1: empty transcript"):
        eng.attention_score([toks[0], []], [0, 1])
    with pytest.raises(RvbError, match="sequence 0: chunk 2 outside the encoded batch of 2 chunks"):
        eng.attention_score([toks[0]], [2])
    with pytest.raises(RvbError, match=r"\(-5\).*longer than the positional table"):
        eng.attention_score([[1] * 100000], [0])
    with pytest.raises(RvbError, match="lsm_weight"):
        eng.attention_score([toks[0]], [0], lsm_weight=1.0)
    with pytest.raises(RvbError, match=r"\(-5\).*spans several chunks"):
        eng.score([toks[0] + toks[1]], [(0, 2)], attention=True)
    fresh = Engine(cfg, sd, dtype="f32", device=0, max_chunks=2, chunk_frames=CHUNK)
    with pytest.raises(RvbError, match=r"\(-3\).*rvb_attention_score before rvb_encode"):
        fresh.attention_score([[1, 2]], [0])
    fresh.close()
    # a model without the right-to-left decoder, and one without any decoder (RVB_E_STATE = -3)
    for drop, kw, msg in (("decoder.right_decoder.", dict(reverse_weight=RW), "no right-to-left decoder"),
                          ("decoder.", dict(), "no attention decoder")):
        c2 = json.loads(json.dumps(cfg))
        c2["decoder_conf"]["r_num_blocks"] = 0
        if drop == "decoder.":
            c2["decoder_conf"]["num_blocks"] = 0
        e2 = Engine(c2, {k: v for k, v in sd.items() if not k.startswith(drop)}, dtype="f32", device=0, max_chunks=2, chunk_frames=CHUNK)
        _encode(e2, 5.0, 3)
        with pytest.raises(RvbError, match=r"\(-3\).*" + msg):
            e2.attention_score([[1, 2, 3]], [0], **kw)
        if drop != "decoder.":
            assert e2.attention_score([[1, 2, 3]], [0])[0]["n_positions"] == 4          # the left decoder alone still scores
        e2.close()


def test_engine_score_gains_the_attention_keys_and_combines_the_losses(tiny):
    eng, toks, _, cfg, _ = tiny
    mc = cfg["model_conf"]
    plain = eng.score(toks)
    assert sorted(plain[0]) == ["loglik", "n_frames", "n_tokens"]
    full = eng.score(toks, attention=True)
    raw = eng.attention_score(toks, [0, 1], reverse_weight=mc["reverse_weight"], lsm_weight=mc["lsm_weight"])
    for p, f, r in zip(plain, full, raw):
        assert sorted(f) == sorted(list(p) + ["loss_ctc", "loss_att", "acc_att", "loss", "att_logp"])
        assert f["loglik"] == p["loglik"] and f["loss_ctc"] == -p["loglik"]
        assert f["loss_att"] == (1 - mc["reverse_weight"]) * r["loss_l"] + mc["reverse_weight"] * r["loss_r"]   # batch of one: / 1
        assert f["loss"] == mc["ctc_weight"] * f["loss_ctc"] + (1 - mc["ctc_weight"]) * f["loss_att"]
        assert f["acc_att"] == r["n_correct"] / r["n_positions"] and f["att_logp"] == r["logp_l"].tolist()
    norm = json.loads(json.dumps(cfg))
    norm["model_conf"]["length_normalized_loss"] = True
    eng.configs, keep = norm, eng.configs
    try:
        byl = eng.score(toks, attention=True, reverse_weight=0.0, ctc_weight=0.5)
    finally:
        eng.configs = keep
    for f, r in zip(byl, raw):
        assert f["loss_att"] == r["loss_l"] / r["n_positions"] and f["loss"] == 0.5 * f["loss_ctc"] + 0.5 * f["loss_att"]


def test_reverb_score_and_get_loss(tmp_path):
    from reverb_amd.bin import get_loss
    from reverb_amd.reverb import load_model
    mdir = synth.write_model_dir(str(tmp_path / "m"), "tiny")
    wavs = []
    for i, (sec, seed) in enumerate(((10.0, 21), (8.0, 22))):
        wavs.append(str(tmp_path / ("u%d.wav" % i)))
        synth.write_wav(wavs[-1], synth.synth_audio(sec, seed=seed))
    long_wav = str(tmp_path / "long.wav")
    synth.write_wav(long_wav, synth.synth_audio(30.0, seed=21))
    asr = load_model(mdir, gpu=0, dtype="f32", max_chunks=4)
    texts = [asr.transcribe(w, mode="ctc_greedy_search", format="txt") for w in wavs]
    base = asr.score(wavs[0], transcript=texts[0])
    assert sorted(base) == ["loglik", "loglik_per_token", "n_frames", "n_tokens", "viterbi_score"]           # unchanged without the flag
    out = asr.score(wavs[0], transcript=texts[0], attention=True)
    assert sorted(out) == sorted(list(base) + ["loss_ctc", "loss_att", "acc_att", "loss", "att_logp"])
    assert all(out[k] == base[k] for k in base) and out["loss_ctc"] == -out["loglik"]
    mc = asr.configs["model_conf"]
    assert out["loss"] == mc["ctc_weight"] * out["loss_ctc"] + (1 - mc["ctc_weight"]) * out["loss_att"]
    assert len(out["att_logp"]) == out["n_tokens"] + 1 and 0.0 <= out["acc_att"] <= 1.0
    long_text = asr.transcribe(long_wav, mode="ctc_greedy_search", format="txt")
    with pytest.raises(ValueError, match="encodes to 2 chunks"):
        asr.score(long_wav, transcript=long_text, attention=True)
    asr.engine.close()
    data = str(tmp_path / "utts.jsonl")
    with open(data, "w") as f:
        for w, t in zip(wavs, texts):
            f.write(json.dumps({"wav": w, "txt": t}) + "\n")
        f.write(json.dumps({"wav": long_wav, "txt": long_text}) + "\n")          # longer than one chunk: skipped and reported
    outp = str(tmp_path / "loss.jsonl")
    total = get_loss.main(["--model", mdir, "--data_list", data, "--jsonl_output", outp, "--gpu", "0", "--dtype", "f32",
                           "--batch_size", "2"])
    lines = [json.loads(l) for l in open(outp)]
    assert len(lines) == 3 and lines[-1] == json.loads(json.dumps(total))
    utt, tot = lines[:2], lines[2]
    assert [u["wav"] for u in utt] == wavs and tot["utterances"] == 2 and tot["skipped"] == [long_wav]
    assert tot["dataset"] == "utts.jsonl" and tot["checkpoint"].endswith(".pt") and tot["time_to_process"] > 0
    assert all(tot[k] is None for k in ("loss_tel", "acc_att_tel", "loss_reverb", "acc_att_reverb", "loss_tel_reverb", "acc_att_tel_reverb"))
    assert abs(tot["loss"] - (utt[0]["loss"] + utt[1]["loss"]) / 2) <= 1e-12 * abs(tot["loss"])
    pos = [u["n_tokens"] + 1 for u in utt]
    assert abs(tot["acc_att"] - sum(u["acc_att"] * p for u, p in zip(utt, pos)) / sum(pos)) <= 1e-12


def test_the_padded_logit_stride_of_a_10001_word_vocabulary():
    cfg = synth.make_config("tiny_v10k")
    sd = synth.make_state_dict(cfg, 0, synth.CTC_GAMMA, 12.33)
    eng = Engine(cfg, sd, dtype="f32", device=0, max_chunks=2, chunk_frames=CHUNK)
    assert _encode(eng, 6.0, 5) == 1
    y = eng.greedy()[0].tokens or [17, 4242, 10000, 3]
    y = list(y)[:40]
    got = eng.attention_score([y], [0], reverse_weight=RW, lsm_weight=LSM)[0]
    s64 = _sd64(sd)
    worst = _check_against_oracle(got, _oracle(s64, cfg, eng, 0, y, "left_decoder"), _oracle(s64, cfg, eng, 0, y, "right_decoder"),
                                  cfg["output_dim"], ATT_LOGP_BOUND)
    print("tiny_v10k: L %d max |att_logp - oracle| %.3g" % (len(y), worst))
    eng.close()


def test_bf16_engine_scores_within_the_derived_bound():
    """A coarse check that stays as it was (27 roundings in sequence: about 70 times the measured error).  The real bound of the bf16
    decoder is tests/test_dec_bf16_gpu.py: every stored tensor of every layer against its fp64 stage function, and the log-probs
    against the bf16-storage restatement's own distance from the oracle, on a model with the benchmark's head size and GEMM forms."""
    cfg, sd = synth.calibrated_state_dict("tiny")
    eng = Engine(cfg, sd, dtype="bf16", device=0, max_chunks=2, chunk_frames=CHUNK)
    assert _encode(eng, 10.0, 21) == 1
    y = list(eng.greedy()[0].tokens)
    assert y
    got = eng.attention_score([y], [0], reverse_weight=RW, lsm_weight=LSM)[0]
    s64 = _sd64(sd)
    for side, key in (("left_decoder", "logp_l"), ("right_decoder", "logp_r")):
        logits, tgt = _oracle(s64, cfg, eng, 0, y, side)
        bound = 2 * 27 * 2.0 ** -9 * float(np.abs(logits).max())
        err = float(np.abs(got[key] - R.log_softmax(logits)[np.arange(len(tgt)), tgt]).max())
        print("bf16 %s: max |logp - oracle| %.3g, bound %.3g" % (side, err, bound))
        assert np.all(np.isfinite(got[key])) and err <= bound
    assert np.isfinite(got["loss_l"]) and np.isfinite(got["loss_r"]) and 0 <= got["n_correct"] <= got["n_positions"] == len(y) + 1
    eng.close()
