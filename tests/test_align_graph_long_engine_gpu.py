"""Long-form alignment of a transcript with alternatives through the engine (rvb_ctc_align_graph_long_* / Engine.align_graph_long_* /
ReverbASR.align(alternatives=True, long_form=True) / align_wav --alternatives --long_graph) on the tiny fp32 model and the 50 s of
synthetic audio in three chunks that test_align_long_engine_gpu.py uses.

The transcript is written around the model's own greedy words, as test_align_graph_engine_gpu.py writes its own: a wrong alternative,
an optional word and an optional wildcard under a bias.  The graph is far smaller than a window, so the window never moves and the
long path must give what the one-batch path gives, bit for bit, however the batches cut the file.  No tolerance is used."""
import json
import logging

import numpy as np
import pytest

import force_align_ref as R
from reverb_amd import synth
from reverb_amd._lib import RvbError
from reverb_amd.token_graph import TokenGraph
from test_align_engine_gpu import CHUNK, engine, feats_of

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
    text = "%s {%s|%s} %s [<star>] [%s] %s [<star>]" % (words[0], wrong, words[1], " ".join(words[2:n // 2]), words[n // 2],
                                                        " ".join(words[n // 2 + 1:]))
    kw = dict(transcript=text, alternatives=True, wildcard="<star>", wildcard_bias=-0.5)
    want = whole.align(wav, format="json", **kw)                      # three chunks in one batch
    assert "window_nodes" not in want and want["text"] == plain_text
    whole.engine.close()
    two = load_model(mdir, gpu=0, dtype="f32", max_chunks=2)
    with pytest.raises(ValueError, match="long_form=True"):           # never taken silently
        two.align(wav, format="json", **kw)
    with pytest.raises(ValueError, match="one-batch"):
        two.align(wav, format="json", transcript=text.replace("[<star>]", ""), alternatives=True, posteriors=True, long_form=True)
    got = two.align(wav, format="json", long_form=True, **kw)         # two batches: chunks 0-1, then chunk 2
    assert got["text"] == want["text"] == plain_text
    assert [(t["id"], t["node"], t["start_ms"], t["end_ms"]) for t in got["tokens"]] == \
           [(t["id"], t["node"], t["start_ms"], t["end_ms"]) for t in want["tokens"]]
    assert np.float32(got["score"]).tobytes() == np.float32(want["score"]).tobytes()
    assert all(0.0 < t["confidence"] <= 1.0 for t in got["tokens"])
    n_nodes = max(t["node"] for t in got["tokens"]) + 1
    assert got["window_nodes"] % 64 == 0 and n_nodes <= got["window_nodes"] < n_nodes + 64 + 8
    assert got["window_margin"] == got["window_nodes"]                # the window holds the graph: no frame counts
    assert not [r for r in caplog.records if r.levelno >= logging.WARNING and "window_tokens" in r.getMessage()]
    two.engine.close()
    # the command-line tool
    tfile = tmp_path / "three.txt"
    tfile.write_text(text, encoding="utf-8")
    argv = ["--model", mdir, "--audio_file", wav, "--transcript_file", str(tfile), "--result_dir", str(tmp_path / "out"), "--format", "json",
            "--dtype", "f32", "--max_chunks", "2", "--alternatives", "--wildcard", "<star>", "--wildcard_bias", "-0.5"]
    align_wav.main(argv + ["--long_graph", "--window_nodes", "512"])
    out = json.loads((tmp_path / "out" / "three.json").read_text(encoding="utf-8"))
    assert out["text"] == plain_text and out["window_nodes"] == got["window_nodes"] and out["window_margin"] == got["window_margin"]
    assert [(t["id"], t["start_ms"], t["end_ms"]) for t in out["tokens"]] == [(t["id"], t["start_ms"], t["end_ms"]) for t in want["tokens"]]
    with pytest.raises(SystemExit):
        align_wav.get_args(argv + ["--long_form"])


def alternatives_around(tokens, V, blank):
    """{wrong | right | wrong wrong | wrong wrong wrong}, two optional wrong tokens, an optional wrong token before the right ones, in
    turn: more than four nodes a token, so that the 50 s fill more than a window of 256 nodes -> (TokenGraph, the nodes of the right reading)"""
    import graph_align_ref as G
    rng = np.random.default_rng(3)

    def other(t):
        o = int(rng.integers(0, V))
        while o == t or o == blank:
            o = int(rng.integers(0, V))
        return o

    items, want_nodes, n = [], [], 0
    for i, t in enumerate(tokens):
        if i % 3 == 1:
            items.append(("choice", [[("tok", other(t))], [("tok", t)], [("tok", other(t))] * 2, [("tok", other(t))] * 3]))
            want_nodes.append(n + 1); n += 7
        elif i % 3 == 2:
            items += [("choice", [[("tok", other(t)), ("tok", other(t))], []]), ("tok", t)]
            want_nodes.append(n + 2); n += 3
        else:
            items += [("choice", [[("tok", other(t))], []]), ("tok", t)]
            want_nodes.append(n + 1); n += 2
    return TokenGraph(*G.build(items), long_form=True), want_nodes


def test_order_errors_independence_and_a_moving_window():
    eng = engine("tiny", "f32", max_chunks=2)
    with pytest.raises(RvbError, match=r"\(-3\).*rvb_ctc_align_graph_long_feed before rvb_ctc_align_graph_long_begin"):
        eng.align_graph_long_feed()
    lens = feats_of(eng, synth.synth_audio(50.0, seed=21))
    assert len(lens) == 3
    total = sum((int(n) - 7) // 4 + 1 for n in lens)
    tokens = []
    for c0 in (0, 2):
        eng.encode(None, lens[c0:c0 + 2], 2, 0.0, first_chunk=c0, T0=CHUNK)
        tokens += [t for g in eng.greedy() for t in g.tokens]
    graph, want_nodes = alternatives_around(tokens, eng.cfg.vocab, eng.cfg.blank_id)
    with pytest.raises(RvbError, match="window_nodes 300 must be 0"):
        eng.align_graph_long_begin(graph, total, 300)
    with pytest.raises(RvbError, match=r"\(-3\).*before rvb_ctc_align_graph_long_begin"):      # a refused begin leaves nothing open
        eng.align_graph_long_feed()
    with pytest.raises(RvbError, match=r"infeasible: the graph's shortest reading needs at least \d+ frames, the lattice has %d" % (len(tokens) - 1)):
        eng.align_graph_long_begin(graph, len(tokens) - 1)

    def whole(window):
        used = eng.align_graph_long_begin(graph, total, window)
        for c0 in (0, 2):
            eng.encode(None, lens[c0:c0 + 2], 2, 0.0, first_chunk=c0, T0=CHUNK)
            eng.align_graph_long_feed()
        out = eng.align_graph_long_finish()
        eng.align_graph_long_end()
        return used, out

    used, (labels, fnode, nodes, begin, end, score, margin) = whole(0)
    assert used == (len(graph) + 63) // 64 * 64 and margin == used
    assert nodes.tolist() == want_nodes and R.collapse(labels, eng.cfg.blank_id).tolist() == tokens
    assert all(fnode[b:e + 1].tolist() == [j] * (e + 1 - b) for j, b, e in zip(nodes, begin, end))
    assert len(graph) > 256 + 128, "lengthen the audio: the graph must be longer than a window and a half"
    used2, small = whole(256)                                        # the same through a window that has to move
    print("tokens", len(tokens), "nodes", len(graph), "margin at 256 nodes:", small[6])
    assert used2 == 256 and 0 <= small[6] < 256
    assert small[0].tolist() == labels.tolist() and small[2].tolist() == want_nodes
    assert np.float32(small[5]).tobytes() == np.float32(score).tobytes()
    # the calls out of order, and the one-batch graph aligner in between
    eng.align_graph_long_begin(graph, total)
    eng.encode(None, lens[:2], 2, 0.0, first_chunk=0, T0=CHUNK)
    eng.align_graph_long_feed()
    with pytest.raises(RvbError, match=r"\(-3\).*finish before all %d frames were fed" % total):
        eng.align_graph_long_finish()
    g0 = eng.greedy()
    one = eng.align_graph([TokenGraph.chain(g.tokens) for g in g0 if g.tokens], [(b, 1) for b, g in enumerate(g0) if g.tokens])
    assert all(R.collapse(r.labels, eng.cfg.blank_id).tolist() == r.tokens for r in one)
    with pytest.raises(RvbError, match=r"\(-3\).*frames are used up"):           # both chunks again: more than the lattice has left
        eng.align_graph_long_feed()
    eng.encode(None, lens[2:], 2, 0.0, first_chunk=2, T0=CHUNK)
    eng.align_graph_long_feed()
    again = eng.align_graph_long_finish()
    assert again[0].tolist() == labels.tolist() and again[2].tolist() == want_nodes
    assert np.float32(again[5]).tobytes() == np.float32(score).tobytes()
    eng.align_graph_long_end()
    eng.close()
