"""Long-form full-sum score of a transcript with alternatives through the engine (rvb_ctc_score_graph_long_* /
Engine.score_graph_long_* / ReverbASR.score(alternatives=True, long_form=True) / align_wav --alternatives --long_graph_score) on the
tiny fp32 model and the 50 s of synthetic audio in three chunks that test_align_graph_long_engine_gpu.py uses: max_chunks=2 (two
batches) against max_chunks=3 (one).

With a graph smaller than a window the window never moves, and the long path must give the one-batch path's loglik and words bit
for bit, however the batches cut the file.  With the alternatives_around graph a window of 256 nodes moves; its results are held
against the whole-graph window's (the same kernels with a window that holds the graph) within the bounds of
tests/test_ctc_graph_score_window_gpu.py: loglik within 1e-5 per frame, visit within TOL_VISIT, peak_post within TOL_POST, occupancy
(relative) within TOL_OCC on the nodes of visit >= 1e-3 -- the peaked lattice of the model's own greedy words leaves the band
virtually all of the mass, which the printed figures show."""
import json
import logging

import numpy as np
import pytest

from reverb_amd import synth
from reverb_amd._lib import RvbError
from test_align_engine_gpu import CHUNK, engine, feats_of
from test_align_graph_long_engine_gpu import alternatives_around
from test_ctc_graph_score_window_gpu import LL_PER_FRAME, TOL_OCC, TOL_POST, TOL_VISIT

pytestmark = pytest.mark.gpu


def test_front_end(tmp_path, caplog):
    from reverb_amd.bin import align_wav
    from reverb_amd.reverb import load_model
    mdir = synth.write_model_dir(str(tmp_path / "m"), "tiny")
    wav = str(tmp_path / "three.wav")
    synth.write_wav(wav, synth.synth_audio(50.0, seed=21))
    whole = load_model(mdir, gpu=0, dtype="f32", max_chunks=3)
    words = whole.transcribe(wav, mode="ctc_greedy_search", format="txt").split()
    n = len(words)
    assert n >= 9
    wrong = next(w for w in words if w != words[1])
    plain_text = " ".join(words)
    text = "%s {%s|%s} %s [%s] %s" % (words[0], wrong, words[1], " ".join(words[2:n // 2]), words[n // 2], " ".join(words[n // 2 + 1:]))
    want = whole.score(wav, transcript=text, alternatives=True, posteriors=True)          # three chunks in one batch
    assert "window_nodes" not in want and want["text"] == plain_text
    whole.engine.close()
    two = load_model(mdir, gpu=0, dtype="f32", max_chunks=2)
    with pytest.raises(ValueError, match="long_form=True"):           # never taken silently
        two.score(wav, transcript=text, alternatives=True)
    got = two.score(wav, transcript=text, alternatives=True, posteriors=True, long_form=True)     # two batches: chunks 0-1, then chunk 2
    assert got["loglik"] == want["loglik"], "the long path's loglik differs from the one-batch path's"
    assert got["words"] == want["words"], "the long path's words differ from the one-batch path's"
    assert got["text"] == plain_text and got["n_frames"] == want["n_frames"]
    assert np.float32(got["viterbi_score"]).tobytes() == np.float32(want["viterbi_score"]).tobytes()
    n_nodes = max(w["node"] for w in got["words"]) + 1
    assert got["window_nodes"] % 64 == 0 and n_nodes <= got["window_nodes"] < n_nodes + 64 + 8
    assert got["window_margin"] == got["window_nodes"]                # the window holds the graph: no frame counts
    assert got["loglik"] >= got["viterbi_score"] - 1e-5 * got["n_frames"]
    assert not [r for r in caplog.records if r.levelno >= logging.WARNING and "window_tokens" in r.getMessage()]
    fwd = two.score(wav, transcript=text, alternatives=True, long_form=True)
    assert fwd["loglik"] == want["loglik"] and "words" not in fwd
    with pytest.raises(ValueError, match="one-batch"):                # align keeps its refusal
        two.align(wav, format="json", transcript=text, alternatives=True, posteriors=True, long_form=True)
    two.engine.close()
    # the command-line tool
    tfile = tmp_path / "three.txt"
    tfile.write_text(text, encoding="utf-8")
    argv = ["--model", mdir, "--audio_file", wav, "--transcript_file", str(tfile), "--result_dir", str(tmp_path / "out"), "--format", "json",
            "--dtype", "f32", "--max_chunks", "2", "--alternatives"]
    align_wav.main(argv + ["--long_graph_score", "--window_nodes", "512"])
    out = json.loads((tmp_path / "out" / "three.score.json").read_text(encoding="utf-8"))
    assert out["loglik"] == want["loglik"] and out["text"] == plain_text and out["window_nodes"] == got["window_nodes"]
    assert out["words"] == json.loads(json.dumps(want["words"]))
    ali = json.loads((tmp_path / "out" / "three.json").read_text(encoding="utf-8"))
    assert ali["text"] == plain_text and ali["window_nodes"] == got["window_nodes"]


def test_order_errors_independence_and_a_moving_window():
    eng = engine("tiny", "f32", max_chunks=2)
    with pytest.raises(RvbError, match=r"\(-3\).*rvb_ctc_score_graph_long_feed before rvb_ctc_score_graph_long_begin"):
        eng.score_graph_long_feed()
    lens = feats_of(eng, synth.synth_audio(50.0, seed=21))
    assert len(lens) == 3
    total = sum((int(n) - 7) // 4 + 1 for n in lens)
    tokens = []
    for c0 in (0, 2):
        eng.encode(None, lens[c0:c0 + 2], 2, 0.0, first_chunk=c0, T0=CHUNK)
        tokens += [t for g in eng.greedy() for t in g.tokens]
    graph, want_nodes = alternatives_around(tokens, eng.cfg.vocab, eng.cfg.blank_id)
    with pytest.raises(RvbError, match="window_nodes 8192 must be 0"):
        eng.score_graph_long_begin(graph, total, 8192)
    with pytest.raises(RvbError, match=r"\(-3\).*before rvb_ctc_score_graph_long_begin"):      # a refused begin leaves nothing open
        eng.score_graph_long_feed()
    with pytest.raises(RvbError, match=r"infeasible: the graph's shortest reading needs at least \d+ frames, the lattice has %d" % (len(tokens) - 1)):
        eng.score_graph_long_begin(graph, len(tokens) - 1)

    def whole(window, posteriors=True):
        used = eng.score_graph_long_begin(graph, total, window, posteriors)
        for c0 in (0, 2):
            eng.encode(None, lens[c0:c0 + 2], 2, 0.0, first_chunk=c0, T0=CHUNK)
            eng.score_graph_long_feed()
        ll = eng.score_graph_long_loglik()
        post = None
        if posteriors:
            for c0 in (2, 0):
                eng.encode(None, lens[c0:c0 + 2], 2, 0.0, first_chunk=c0, T0=CHUNK)
                eng.score_graph_long_feed_back()
            post = {k: np.array(v) for k, v in eng.score_graph_long_finish().items()}
        eng.score_graph_long_end()
        return used, ll, post

    used, ll, post = whole(0)
    assert used == (len(graph) + 63) // 64 * 64
    on = np.zeros(len(graph), bool)
    on[want_nodes] = True
    assert post["visit"][on].min() > 0.5, "the model's own reading should carry the mass"
    assert whole(0, posteriors=False)[1] == ll
    assert len(graph) > 256 + 128, "lengthen the audio: the graph must be longer than a window and a half"
    used2, ll2, post2 = whole(256)                                   # the same through a window that has to move
    seen = post["visit"] >= 1e-3
    e_vis = float(np.abs(post2["visit"] - post["visit"]).max())
    e_post = float(np.abs(post2["peak_posterior"] - post["peak_posterior"]).max())
    e_occ = float((np.abs(post2["occupancy"] - post["occupancy"])[seen] / post["occupancy"][seen]).max())
    print("tokens %d nodes %d frames %d: loglik %.9g at %d nodes, %.9g at 256 (diff %.3g); visit %.3g peak_post %.3g occupancy %.3g"
          % (len(tokens), len(graph), total, ll, used, ll2, abs(ll - ll2), e_vis, e_post, e_occ))
    assert used2 == 256 and ll2 <= ll + LL_PER_FRAME * total and abs(ll - ll2) <= LL_PER_FRAME * total
    assert e_vis <= TOL_VISIT and e_post <= TOL_POST and e_occ <= TOL_OCC
    sure = post["visit"] >= 0.5
    assert (post2["peak_frame"][sure] != post["peak_frame"][sure]).mean() <= 0.05
    # the calls out of order, and the one-batch graph scorer in between
    eng.score_graph_long_begin(graph, total, 256, True)
    eng.encode(None, lens[:2], 2, 0.0, first_chunk=0, T0=CHUNK)
    eng.score_graph_long_feed()
    with pytest.raises(RvbError, match=r"\(-3\).*loglik before all %d frames were fed" % total):
        eng.score_graph_long_loglik()
    with pytest.raises(RvbError, match=r"\(-3\).*rvb_ctc_score_graph_long_feed_back before rvb_ctc_score_graph_long_loglik"):
        eng.score_graph_long_feed_back()
    from reverb_amd.token_graph import TokenGraph
    g0 = eng.greedy()
    one = eng.score_graph([TokenGraph.chain(g.tokens) for g in g0 if g.tokens], [(b, 1) for b, g in enumerate(g0) if g.tokens])
    assert all(np.isfinite(r["loglik"]) for r in one)
    with pytest.raises(RvbError, match=r"\(-3\).*frames are used up"):           # both chunks again: more than the lattice has left
        eng.score_graph_long_feed()
    eng.encode(None, lens[2:], 2, 0.0, first_chunk=2, T0=CHUNK)
    eng.score_graph_long_feed()
    assert eng.score_graph_long_loglik() == ll2
    with pytest.raises(RvbError, match=r"\(-3\).*rvb_ctc_score_graph_long_finish|did not reach the first frame"):
        eng.score_graph_long_finish()
    eng.encode(None, lens[:2], 2, 0.0, first_chunk=0, T0=CHUNK)      # the wrong batch: the backward sweep starts with the last one
    with pytest.raises(RvbError, match=r"\(-3\).*descending order: expected batch 1 with the \d+ frames"):
        eng.score_graph_long_feed_back()
    for c0 in (2, 0):
        eng.encode(None, lens[c0:c0 + 2], 2, 0.0, first_chunk=c0, T0=CHUNK)
        eng.score_graph_long_feed_back()
    again = eng.score_graph_long_finish()
    assert np.array_equal(np.array(again["visit"]), post2["visit"]) and np.array_equal(np.array(again["peak_frame"]), post2["peak_frame"])
    eng.score_graph_long_end()
    eng.close()
