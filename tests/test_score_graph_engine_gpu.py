"""The full-sum score over token graphs through the engine (rvb_ctc_score_graph / Engine.score_graph / ReverbASR.score(alternatives=True)
/ align(alternatives=True, posteriors=True) / align_wav --graph_score) on the tiny fp32 model and the 25 s of synthetic audio in two
chunks that test_align_graph_engine_gpu.py uses.

The hook runs on rvb_get_ctc_logprobs, which recomputes the CTC head in a launch of its own shape: in f32 the two sets of log-probs
agree to the fp32 rounding of a d_model-long dot product, so loglik is compared at the kernel's own ceiling of 1e-5 nats per frame
plus T * 1e-5 for the log-probs, as tests/test_ctc_score_engine_gpu.py does.  The per-node outputs are compared at the CONDITIONS of
tests/test_ctc_graph_score_gpu.py (1e-3 for peak posterior, occupancy and mean frame, 1e-2 for visit), not at its measured bounds:
those bound the kernel on identical log-prob bits, and here the two sets of log-probs differ by their own rounding, which nobody
has measured separately.  The relative figures are taken on nodes of visit >= 1e-3."""
import json

import numpy as np
import pytest

import graph_align_ref as G
import graph_score_ref as R
from reverb_amd import _lib, synth
from reverb_amd._lib import RvbError, dptr, fptr, iptr, u8ptr
from reverb_amd.ctc_align import WILDCARD
from reverb_amd.engine import Engine
from reverb_amd.token_graph import TokenGraph

pytestmark = pytest.mark.gpu
CHUNK = 2051
LL_PER_FRAME = 2e-5       # the kernel's 1e-5 per frame + 1e-5 per frame for the recomputed log-probs
TOL_POST, TOL_OCC, TOL_MEAN, TOL_VISIT = 1e-3, 1e-3, 1e-3, 1e-2


@pytest.fixture(scope="module")
def enc():
    """the encoded batch of two chunks, its greedy tokens and valid lengths, shared by the tests (none of them changes it)"""
    cfg, sd = synth.calibrated_state_dict("tiny")
    eng = Engine(cfg, sd, dtype="f32", device=0, max_chunks=4, chunk_frames=CHUNK)
    eng.upload_pcm(synth.synth_audio(25.0, seed=41))
    n = eng.fbank()
    nch = -(-n // CHUNK)
    lens = np.full(nch, CHUNK, np.int32)
    lens[-1] = n - (nch - 1) * CHUNK
    assert nch == 2
    eng.encode(None, lens, 2, 0.0, T0=CHUNK)
    greedy = eng.greedy()
    elens = eng.encoder_lens()
    yield eng, [list(g.tokens) for g in greedy], elens
    eng.close()


def corrupted(eng, toks, seed=3):
    """{wrong | right | wrong wrong} at every third token, an optional wrong word before every third: the graph of
    test_align_graph_engine_gpu.py -> (graph, the nodes of the right reading)"""
    V, blank = eng.cfg.vocab, eng.cfg.blank_id
    rng = np.random.default_rng(seed)

    def other(t):
        o = int(rng.integers(0, V))
        while o == t or o == blank:
            o = int(rng.integers(0, V))
        return o

    items, want, n = [], [], 0
    for i, t in enumerate(toks):
        if i % 3 == 1:
            items.append(("choice", [[("tok", other(t))], [("tok", t)], [("tok", other(t)), ("tok", other(t))]]))
            want.append(n + 1); n += 4
        elif i % 3 == 2:
            items += [("choice", [[("tok", other(t))], []]), ("tok", t)]
            want.append(n + 1); n += 2
        else:
            items.append(("tok", t))
            want.append(n); n += 1
    return TokenGraph(*G.build(items)), want


def hook(lp, graph):
    tok, nn, off, prd, fin = R.flat([(graph.tokens, graph.preds, graph.finals)])
    n = len(graph)
    T = np.array([len(lp)], np.int32)
    ll = np.zeros(1, np.float64)
    vis, occ, mean, peak = (np.zeros(n, np.float32) for _ in range(4))
    pf = np.zeros(n, np.int32)
    lib = _lib.load_test()
    rc = lib.rvb_test_ctc_score_graph(fptr(np.ascontiguousarray(lp)), iptr(T), 1, lp.shape[1], iptr(tok), iptr(nn), iptr(off), iptr(prd), u8ptr(fin),
                                      0, len(lp), dptr(ll), fptr(vis), fptr(occ), fptr(mean), fptr(peak), iptr(pf))
    assert rc == 0, lib.rvb_last_error().decode()
    return {"loglik": float(ll[0]), "visit": vis, "occupancy": occ, "mean_frame": mean, "peak_posterior": peak, "peak_frame": pf}


def close(got, want, T):
    """two results of the same lattice on log-probs that differ by rounding"""
    assert abs(got["loglik"] - want["loglik"]) <= LL_PER_FRAME * T
    v, v0 = np.asarray(got["visit"]), np.asarray(want["visit"])
    seen = v0 >= 1e-3
    o, o0 = np.asarray(got["occupancy"]), np.asarray(want["occupancy"])
    m, m0 = np.asarray(got["mean_frame"]), np.asarray(want["mean_frame"])
    assert np.abs(v - v0).max() <= TOL_VISIT
    assert np.abs(np.asarray(got["peak_posterior"]) - np.asarray(want["peak_posterior"])).max() <= TOL_POST
    assert (np.abs(o - o0)[seen] / o0[seen]).max() <= TOL_OCC
    assert (np.abs(m - m0)[seen] / np.maximum(m0[seen], 1.0)).max() <= TOL_MEAN


def test_a_chain_is_score(enc):
    eng, toks, elens = enc
    ranges = [(0, 1), (1, 1)]
    plain = eng.score(toks, ranges, posteriors=True)
    got = eng.score_graph([TokenGraph.chain(t) for t in toks], ranges, posteriors=True)
    fwd = eng.score_graph([TokenGraph.chain(t) for t in toks], ranges)
    for b in range(2):
        assert got[b]["n_nodes"] == len(toks[b]) and got[b]["n_frames"] == int(elens[b]) == plain[b]["n_frames"]
        assert fwd[b]["loglik"] == got[b]["loglik"] and "visit" not in fwd[b]
        assert np.abs(np.asarray(got[b]["visit"]) - 1.0).max() <= TOL_VISIT
        close(dict(got[b]), dict(plain[b], visit=np.ones(len(toks[b]))), got[b]["n_frames"])
        assert np.mean(np.asarray(got[b]["peak_frame"]) != np.asarray(plain[b]["peak_frame"])) <= 0.05


def test_a_graph_agrees_with_the_hook_on_the_engines_logprobs(enc):
    eng, toks, elens = enc
    graph, want = corrupted(eng, toks[0])
    got = eng.score_graph([graph], [(0, 1)], posteriors=True)[0]
    ref = hook(eng.ctc_logprobs(0)[:int(elens[0])], graph)
    close(got, ref, int(elens[0]))
    vis = np.asarray(got["visit"])
    on = np.zeros(len(graph), bool)
    on[want] = True
    assert vis[on].min() > 0.5 > vis[~on].max()              # the greedy reading carries the mass
    plain = eng.score([toks[0]], [(0, 1)])[0]
    assert got["loglik"] >= plain["loglik"] - LL_PER_FRAME * got["n_frames"]      # the sum over all readings holds the right one's


def test_one_graph_over_two_chunks(enc):
    eng, toks, elens = enc
    graph, _ = corrupted(eng, toks[0] + toks[1], seed=4)
    got = eng.score_graph([graph], [(0, 2)], posteriors=True)[0]
    T = int(elens.sum())
    assert got["n_frames"] == T
    lp = np.concatenate([eng.ctc_logprobs(b)[:int(elens[b])] for b in range(2)])
    close(got, hook(lp, graph), T)
    assert got["loglik"] == eng.score_graph([graph], [(0, 2)])[0]["loglik"]


def test_requests_that_are_refused(enc):
    eng, toks, _ = enc
    chain = TokenGraph.chain(toks[0])
    with pytest.raises(RvbError, match="rvb_ctc_score_graph: sequence 0: chunk range outside"):
        eng.score_graph([chain], [(1, 2)])
    with pytest.raises(RvbError, match="sequence 1: node 1: a wildcard has no full-sum score"):
        eng.score_graph([chain, TokenGraph.chain([1, WILDCARD, 2])], [(0, 1), (1, 1)])
    with pytest.raises(RvbError, match="sequence 1: node 2: label %d outside" % eng.cfg.vocab):
        eng.score_graph([chain, TokenGraph.chain([1, 2, eng.cfg.vocab])], [(0, 1), (1, 1)])
    with pytest.raises(RvbError, match="infeasible: no path of"):
        eng.score_graph([TokenGraph.chain([1, 2] * 400)], [(1, 1)])
    fan = TokenGraph([1] + [2 + j % 5 for j in range(65)], [[-1]] + [[0]] * 65, [False] + [True] * 65)
    with pytest.raises(RvbError, match="node 0: out-degree 65 exceeds the cap of 64"):
        eng.score_graph([fan], [(0, 1)], posteriors=True)
    assert np.isfinite(eng.score_graph([fan], [(0, 1)])[0]["loglik"])       # forward only: no cap on the out-degree


def test_alternatives_are_scored_end_to_end(tmp_path):
    from reverb_amd.bin import align_wav
    from reverb_amd.reverb import load_model
    mdir = synth.write_model_dir(str(tmp_path / "m"), "tiny")
    wav = str(tmp_path / "alt.wav")
    synth.write_wav(wav, synth.synth_audio(25.0, seed=41))
    asr = load_model(mdir, gpu=0, dtype="f32", max_chunks=4)
    words = asr.transcribe(wav, mode="ctc_greedy_search", format="txt").split()
    n = len(words)
    assert n >= 9
    wrong = next(w for w in words if w != words[1])
    plain_text = " ".join(words)
    text = "%s {%s|%s} %s [%s] %s" % (words[0], wrong, words[1], " ".join(words[2:n // 2]), words[n // 2], " ".join(words[n // 2 + 1:]))
    fwd = asr.score(wav, transcript=text, alternatives=True)
    assert sorted(fwd) == ["loglik", "n_frames", "text", "viterbi_score"]
    assert fwd["text"] == plain_text and fwd["loglik"] >= fwd["viterbi_score"] - 1e-5 * fwd["n_frames"]
    assert fwd["loglik"] >= asr.score(wav, transcript=plain_text)["loglik"] - 1e-5 * fwd["n_frames"]
    full = asr.score(wav, transcript=text, alternatives=True, posteriors=True)
    assert full["loglik"] == fwd["loglik"] and sorted(full) == sorted(list(fwd) + ["words"])
    ws = full["words"]
    assert [w["text"] for w in ws[:3]] == [words[0], wrong, words[1]] and all(sorted(w) == ["mean_time", "node", "occupancy", "probability", "text"] for w in ws)
    assert ws[2]["probability"] > ws[1]["probability"]        # the spoken word against the planted wrong one
    assert abs(ws[1]["probability"] + ws[2]["probability"] - 1.0) <= 2 * TOL_VISIT      # the two branches of the group
    assert abs(ws[0]["probability"] - 1.0) <= TOL_VISIT
    with pytest.raises(ValueError, match="alternatives"):
        asr.score(wav, transcript=text, alternatives=True, attention=True)
    with pytest.raises(ValueError, match="alternatives"):
        asr.score(wav, tokens=[1, 2], alternatives=True)
    # align carries the chosen path's share of the full sum
    js = asr.align(wav, transcript=text, alternatives=True, posteriors=True, format="json")
    ref = asr.align(wav, transcript=text, alternatives=True, format="json")
    assert js["text"] == plain_text and js["score"] == ref["score"]
    extra = ["mean_time", "occupancy", "peak_posterior", "probability"]
    for a, b in zip(ref["tokens"], js["tokens"]):
        assert sorted(b) == sorted(list(a) + extra) and all(b[k] == a[k] for k in a)
    assert all(t["probability"] > 0.5 for t in js["tokens"])
    asr.engine.close()
    # the command-line tool
    tfile = tmp_path / "alt.txt"
    tfile.write_text(text, encoding="utf-8")
    argv = ["--model", mdir, "--audio_file", wav, "--transcript_file", str(tfile), "--result_dir", str(tmp_path / "out"), "--format", "json",
            "--dtype", "f32", "--max_chunks", "4", "--alternatives", "--graph_score"]
    align_wav.main(argv)
    out = json.loads((tmp_path / "out" / "alt.score.json").read_text(encoding="utf-8"))
    assert out["text"] == plain_text and out["loglik"] == full["loglik"] and [w["node"] for w in out["words"]] == [w["node"] for w in ws]
    with pytest.raises(SystemExit):
        align_wav.get_args(argv[:-2] + ["--graph_score"])                      # needs --alternatives
    with pytest.raises(SystemExit):
        align_wav.get_args(argv + ["--wildcard", "<star>"])
    with pytest.raises(SystemExit):
        align_wav.get_args(argv + ["--attention"])                              # one token sequence only
