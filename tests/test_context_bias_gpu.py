"""Hot-word context biasing through the engine (rvb_set_context_graph) on the synthetic small models of tests/test_engine_gpu.py.

The host search is deterministic given the top-k bits, so what the engine returns with a graph must EQUAL tests/context_bias_ref.py
(the plain-Python statement pinned to the reference by tests/test_context_bias.py) run on the engine's own rvb_get_ctc_topk output:
token lists, float64 scores and peak times, exactly.

The hot words are token n-grams of the lower-ranked hypotheses of an unbiased search that its 1-best does not contain
(context_bias_ref.phrases_from).  That these move at least one 1-best on the f32 model was checked without a GPU, by running
context_bias_ref.search on the reference's own top-k of the same cases (tests/golden/tiny_ln.npz, small_ln.npz) -- whose n-best lists
the f32 engine reproduces exactly (test_engine_gpu.py::test_f32_engine_matches_reference_golden): tiny_ln chunk 1 and small_ln chunk 0
change at context scores 3.0 and 6.0."""
import os
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import context_bias_ref as R  # noqa: E402
from golden_util import Case  # noqa: E402
from reverb_amd import synth  # noqa: E402
from reverb_amd.context_graph import ContextGraph  # noqa: E402
from reverb_amd.engine import Engine  # noqa: E402

pytestmark = pytest.mark.gpu
SCORE = 6.0


def _engine(case, max_chunks=4):
    return Engine(case.cfg, case.sd, dtype="f32", device=0, max_chunks=max_chunks, chunk_frames=case.chunk, cat_embs=case.cat)


def _phrases(prefix_results):
    out = []
    for p in prefix_results:
        for ph in R.phrases_from([list(h) for h in p.nbest]):
            if ph not in out:
                out.append(ph)
    assert out, "the unbiased n-best lists offer no hot word"
    return out


def _expected(eng, beam, phrases, score):
    """context_bias_ref.search on the engine's own top-k, per chunk of the current batch"""
    tv, ti = eng.ctc_topk()
    lens = eng.encoder_lens()
    graph = R.Graph(phrases, score) if phrases is not None else None
    return [R.search(tv[b], ti[b], int(lens[b]), beam, 0, graph) for b in range(len(lens))]


def _assert_equal(results, expected):
    for b, (p, want) in enumerate(zip(results, expected)):
        assert [list(h) for h in p.nbest] == want["nbest"], b
        assert p.nbest_times == want["times"], b
        assert list(p.nbest_scores) == want["scores"], b                       # float64, bit for bit
        assert list(p.tokens) == want["nbest"][0] and p.score == want["scores"][0] and list(p.times) == want["times"][0]


def _same(a, b):
    assert len(a) == len(b)
    for p, q in zip(a, b):
        assert list(p.tokens) == list(q.tokens)
        assert (p.nbest is None) == (q.nbest is None)
        if p.nbest is not None:
            assert p.nbest == q.nbest and p.nbest_times == q.nbest_times
            assert np.array(p.nbest_scores).tobytes() == np.array(q.nbest_scores).tobytes()
        assert p.times == q.times and p.score == q.score


@pytest.mark.parametrize("name", ["tiny_ln", "small_ln"])
def test_biased_prefix_beam_equals_the_restatement_on_the_engines_own_topk(name):
    case = Case(name)
    x, lens = case.chunked_feats()
    eng = _engine(case)
    eng.encode(x, lens, case.beam)
    plain = eng.prefix_beam()
    _assert_equal(plain, _expected(eng, case.beam, None, 0.0))
    phrases = _phrases(plain)
    moved = 0
    for score in (SCORE, 3.0):
        eng.set_context_graph(phrases, score)
        biased = eng.prefix_beam()
        _assert_equal(biased, _expected(eng, case.beam, phrases, score))
        moved += sum(list(p.tokens) != list(q.tokens) for p, q in zip(plain, biased)) if score == SCORE else 0
    assert moved >= 1, "no 1-best changed: the fixture no longer exercises the biasing"
    # a ContextGraph object is taken like the lists; its own score is used unless one is given
    eng.set_context_graph(ContextGraph.from_token_ids(phrases, 3.0))
    _same(eng.prefix_beam(), biased)
    # a graph whose score is 0.0 and a cleared graph both give the unbiased result bit for bit
    eng.set_context_graph(phrases, 0.0)
    _same(eng.prefix_beam(), plain)
    eng.set_context_graph(phrases, SCORE)
    eng.set_context_graph(None)
    _same(eng.prefix_beam(), plain)
    eng.close()


def test_bad_phrases_are_refused_by_name_and_leave_the_graph_alone():
    from reverb_amd._lib import RvbError
    case = Case("tiny_ln")
    x, lens = case.chunked_feats()
    eng = _engine(case)
    eng.encode(x, lens, case.beam)
    plain = eng.prefix_beam()
    phrases = _phrases(plain)
    eng.set_context_graph(phrases, SCORE)
    biased = eng.prefix_beam()
    V = case.cfg["output_dim"]
    with pytest.raises(RvbError, match="phrase 1 position 1.*blank"):
        eng.set_context_graph([[3], [4, 0]], SCORE)
    with pytest.raises(RvbError, match=r"phrase 0 position 0.*outside \[0, %d\)" % V):
        eng.set_context_graph([[V]], SCORE)
    _same(eng.prefix_beam(), biased)                   # the refused calls did not touch the graph that was set
    eng.set_context_graph([[], []], SCORE)             # empty phrases: a graph of the root alone
    _same(eng.prefix_beam(), plain)
    eng.close()


def test_attention_rescoring_rescores_the_biased_nbest_with_its_biased_scores():
    """search.py:436-444: final score = attention score + ctc_weight * n-best score, over the n-best of the (biased) prefix beam.
    The oracle's rescoring (oracle/search_ref.py, CPU) is given the restatement's biased n-best and scores and the engine's encoder
    output; tolerance as tests/test_engine_gpu.py has it for unbiased rescoring."""
    import torch
    from oracle import model_ref as M, search_ref as S
    case = Case("tiny_ln")
    x, lens = case.chunked_feats()
    eng = _engine(case)
    eng.encode(x, lens, case.beam)
    phrases = _phrases(eng.prefix_beam())
    unbiased = eng.search(["attention_rescoring"], case.ctc_weight, case.reverse_weight)["attention_rescoring"]
    eng.set_context_graph(phrases, SCORE)
    want_prefix = [S.DecodeResult(tokens=w["nbest"][0], score=w["scores"][0], times=w["times"][0], nbest=[tuple(h) for h in w["nbest"]],
                                  nbest_scores=w["scores"], nbest_times=w["times"]) for w in _expected(eng, case.beam, phrases, SCORE)]
    enc, enc_lens = torch.from_numpy(eng.encoder_out()), eng.encoder_lens()
    want = S.attention_rescoring(M.to_torch_sd(case.sd), case.cfg, want_prefix, enc, enc_lens, case.ctc_weight, case.reverse_weight,
                                 torch.tensor(case.cat))
    # both ways through Engine.search: the bulk path (rescoring alone) and the one that also returns the prefix beam
    alone = eng.search(["attention_rescoring"], case.ctc_weight, case.reverse_weight)["attention_rescoring"]
    both = eng.search(["ctc_prefix_beam_search", "attention_rescoring"], case.ctc_weight, case.reverse_weight)
    _assert_equal(both["ctc_prefix_beam_search"], _expected(eng, case.beam, phrases, SCORE))
    differs = 0
    for b in range(len(lens)):
        for r in (alone[b], both["attention_rescoring"][b]):
            assert list(r.tokens) == list(want[b].tokens), b
            assert list(r.times) == list(want[b].times), b
            assert abs(r.score - want[b].score) <= 2e-2 + 1e-4 * abs(want[b].score), (b, r.score, want[b].score)
        differs += list(alone[b].tokens) != list(unbiased[b].tokens) or abs(alone[b].score - unbiased[b].score) > 1.0
    assert differs >= 1, "rescoring saw the same hypotheses and scores with and without the graph"
    eng.close()


def test_graph_applies_after_stream_finish_and_through_model_decode():
    """RvbASRModel.decode(context_graph=...): the batch branch, the simulate_streaming branch (rvb_stream_finish, then the same
    search), and the per-utterance cat_embs recursion; None clears."""
    import torch
    from reverb_amd.reverb import RvbASRModel
    case = Case("tiny_ln")
    x, lens = case.chunked_feats()
    eng = _engine(case)
    model = RvbASRModel(eng)
    modes = ["ctc_prefix_beam_search"]
    tx, tl = torch.from_numpy(x), torch.from_numpy(lens)
    plain = model.decode(modes, tx, tl, case.beam, cat_embs=case.cat)[modes[0]]
    phrases = _phrases(plain)
    graph = ContextGraph.from_token_ids(phrases, SCORE)
    biased = model.decode(modes, tx, tl, case.beam, cat_embs=case.cat, context_graph=graph)[modes[0]]
    _assert_equal(biased, _expected(eng, case.beam, phrases, SCORE))
    assert any(list(p.tokens) != list(q.tokens) for p, q in zip(plain, biased))
    rows = np.tile(np.asarray(case.cat, np.float32), (len(lens), 1))              # 2-D cat_embs: decoded group by group
    _same(model.decode(modes, tx, tl, case.beam, cat_embs=torch.from_numpy(rows), context_graph=graph)[modes[0]], biased)
    _same(model.decode(modes, tx, tl, case.beam, cat_embs=case.cat)[modes[0]], plain)            # context_graph=None clears
    # one stream (the last item decoded stays on the engine, so its top-k can be read back)
    one = (tx[1:2], tl[1:2])
    s_plain = model.decode(modes, *one, case.beam, 16, -1, 0.0, True, cat_embs=case.cat)[modes[0]]
    _assert_equal(s_plain, _expected(eng, case.beam, None, 0.0))
    s_phrases = phrases + [ph for ph in R.phrases_from([list(h) for h in s_plain[0].nbest]) if ph not in phrases]
    s_biased = model.decode(modes, *one, case.beam, 16, -1, 0.0, True, cat_embs=case.cat,
                            context_graph=ContextGraph.from_token_ids(s_phrases, SCORE))[modes[0]]
    _assert_equal(s_biased, _expected(eng, case.beam, s_phrases, SCORE))
    assert s_biased[0].nbest != s_plain[0].nbest or s_biased[0].nbest_scores != s_plain[0].nbest_scores
    _same(model.decode(modes, *one, case.beam, 16, -1, 0.0, True, cat_embs=case.cat)[modes[0]], s_plain)
    eng.close()


def test_greedy_attention_and_joint_decoding_ignore_the_graph():
    case = Case("tiny_ln")
    x, lens = case.chunked_feats()
    eng = _engine(case)
    modes = ["ctc_greedy_search", "attention", "joint_decoding"]
    from reverb_amd.engine import joint_topk
    topk = joint_topk(modes, case.beam)
    eng.encode(x, lens, case.beam, topk=topk)
    phrases = _phrases(eng.prefix_beam())
    before = eng.search(modes, 0.3, 0.0)
    eng.set_context_graph(phrases, SCORE)
    eng.encode(x, lens, case.beam, topk=topk)           # the same batch again: encoding is deterministic
    after = eng.search(modes, 0.3, 0.0)
    for m in modes:
        assert len(before[m]) == len(after[m]) == len(lens)
        for p, q in zip(before[m], after[m]):
            assert list(p.tokens) == list(q.tokens), m
            assert p.score == q.score and p.times == q.times, m
            assert p.tokens_confidence == q.tokens_confidence, m
    eng.close()


def test_transcribe_takes_the_list_file_end_to_end():
    """load_model(dir, context_path=..., context_score=...) -> ReverbASR.transcribe: the list file is cut with the model's unit table,
    the graph reaches the engine on the resident-features path and on the simulate_streaming path."""
    import reverb_amd
    import wenet
    from reverb_amd.reverb import get_output
    case = Case("tiny_ln")
    kw = dict(verbatimicity=case.cat[0], chunk_size=case.chunk, beam_size=case.beam)
    with tempfile.TemporaryDirectory() as d:
        mdir = synth.write_model_dir(os.path.join(d, "model"), "tiny_ln", sd=case.sd, cfg=case.cfg)
        wav = os.path.join(d, "golden.wav")
        synth.write_wav(wav, case.pcm)
        asr = reverb_amd.load_model(mdir, dtype="f32", max_chunks=4)
        assert asr.context_graph is None
        plain_txt = asr.transcribe(wav, mode="ctc_prefix_beam_search", **kw)
        n_frames = asr.engine.fbank()
        plain = asr.decode_resident(n_frames, ["ctc_prefix_beam_search"], case.chunk, case.beam, 0.1, 0.0)["ctc_prefix_beam_search"]
        phrases = _phrases(plain)
        asr.engine.close()
        units = synth.make_units(case.cfg["output_dim"])
        path = os.path.join(d, "hot.txt")
        with open(path, "w", encoding="utf8") as f:
            for ph in phrases:
                f.write("".join(units[t] for t in ph).replace("▁", " ").strip() + "\n")
            f.write("\n")                                                         # an empty line: an empty phrase, ignored by the engine
        asr = wenet.load_model(mdir, dtype="f32", max_chunks=4, context_path=path, context_score=SCORE)
        assert asr.context_graph.context_list == phrases + [[]] and asr.context_graph.context_score == SCORE
        txt = asr.transcribe(wav, mode="ctc_prefix_beam_search", **kw)
        # the same recording decoded chunk by chunk on the resident features, checked against the restatement
        n_frames = asr.engine.fbank()
        n_chunks = -(-n_frames // case.chunk)
        assert n_chunks <= 4
        biased = asr.decode_resident(n_frames, ["ctc_prefix_beam_search"], case.chunk, case.beam, 0.1, 0.0)["ctc_prefix_beam_search"]
        _assert_equal(biased, _expected(asr.engine, case.beam, phrases, SCORE))
        assert txt == get_output("txt", asr.tokenizer, "golden.wav", biased, 230, case.chunk, asr.input_frame_length, asr.output_frame_length)
        assert txt != plain_txt
        # the simulate_streaming path hands the same graph over: it is the one the engine holds afterwards (the graph is sticky,
        # decode_resident does not touch it), and dropping it from the model clears it there too
        s_kw = dict(kw, decoding_chunk_size=16, simulate_streaming=True)
        assert isinstance(asr.transcribe(wav, mode="ctc_prefix_beam_search", **s_kw), str)
        _same(asr.decode_resident(asr.engine.fbank(), ["ctc_prefix_beam_search"], case.chunk, case.beam, 0.1, 0.0)["ctc_prefix_beam_search"], biased)
        asr.context_graph = None
        assert isinstance(asr.transcribe(wav, mode="ctc_prefix_beam_search", **s_kw), str)
        _same(asr.decode_resident(asr.engine.fbank(), ["ctc_prefix_beam_search"], case.chunk, case.beam, 0.1, 0.0)["ctc_prefix_beam_search"], plain)
        assert asr.transcribe(wav, mode="ctc_prefix_beam_search", **kw) == plain_txt          # and without a graph the engine is unbiased again
        asr.engine.close()
