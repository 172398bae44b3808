"""Alignment over token graphs through the engine (rvb_ctc_align_graph / Engine.align_graph / ReverbASR.align(alternatives=True) /
align_wav --alternatives) on the tiny fp32 model and the 25 s of synthetic audio in two chunks that test_align_wild_engine_gpu.py uses.

The transcript is the greedy tokens, so its plain alignment follows the model's best label on every frame and its score is the fp32
sum of the per-frame maxima, which no path of any reading exceeds in any addend.  The graph's score is the largest chain score among
its readings (max and fp32 addition are monotone), hence the greedy reading's; and a path with k >= 1 wildcard frames at bias -0.5
stays 0.5 k below that sum, far above the rounding of the sums, so no optional wildcard is taken.  No tolerance is used."""
import json

import numpy as np
import pytest

import force_align_ref as R
import graph_align_ref as G
from reverb_amd import synth
from reverb_amd._lib import RvbError
from reverb_amd.ctc_align import WILDCARD
from reverb_amd.engine import Engine
from reverb_amd.token_graph import TokenGraph

pytestmark = pytest.mark.gpu
CHUNK = 2051


def feats_of(eng, pcm, chunk=CHUNK):
    eng.upload_pcm(pcm)
    n = eng.fbank()
    nch = -(-n // chunk)
    lens = np.full(nch, chunk, np.int32)
    lens[-1] = n - (nch - 1) * chunk
    return lens


@pytest.fixture(scope="module")
def enc():
    """the encoded batch, its greedy tokens and the plain alignment of chunk 0, shared by the tests (none of them changes it)"""
    cfg, sd = synth.calibrated_state_dict("tiny")
    eng = Engine(cfg, sd, dtype="f32", device=0, max_chunks=4, chunk_frames=CHUNK)
    lens = feats_of(eng, synth.synth_audio(25.0, seed=41))
    assert len(lens) == 2
    eng.encode(None, lens, 2, 0.0, T0=CHUNK)
    greedy = eng.greedy()
    toks = list(greedy[0].tokens)
    assert len(toks) >= 12
    plain = eng.align([toks], [(0, 1)])[0]
    yield eng, greedy, toks, plain
    eng.close()


def fields(r):
    return (r.tokens, r.labels, r.begin, r.end, r.peak, np.array(r.confidence, np.float32).tobytes(), np.float32(r.score).tobytes(),
            r.first_chunk, r.chunk_lens)


def test_a_chain_is_align_and_align_wild_field_for_field(enc):
    eng, greedy, toks, plain = enc
    seqs = [g.tokens for g in greedy if g.tokens]
    ranges = [(b, 1) for b, g in enumerate(greedy) if g.tokens]
    a = eng.align(seqs, ranges)
    g = eng.align_graph([TokenGraph.chain(s) for s in seqs], ranges)
    assert [fields(x) for x in a] == [fields(x) for x in g]
    assert [x.nodes for x in g] == [list(range(len(s))) for s in seqs]
    # with wildcards, one sequence over both chunks
    both = list(greedy[0].tokens) + list(greedy[1].tokens)
    n = len(both)
    ed = [WILDCARD] + both[1:n // 3] + [WILDCARD] + both[2 * n // 3:]
    for bias in (0.0, -0.5):
        w = eng.align_wild([ed], [(0, 2)], bias)[0]
        g = eng.align_graph([TokenGraph.chain(ed)], [(0, 2)], bias)[0]
        assert fields(w) == fields(g) and g.wildcard == w.wildcard


def test_it_picks_the_greedy_reading_among_corrupted_ones(enc):
    eng, _, toks, plain = enc
    V, blank = eng.cfg.vocab, eng.cfg.blank_id
    rng = np.random.default_rng(3)

    def other(t):
        o = int(rng.integers(0, V))
        while o == t or o == blank:
            o = int(rng.integers(0, V))
        return o

    items, want_nodes, n = [], [], 0
    for i, t in enumerate(toks):
        if i % 3 == 1:                                       # {wrong | right | wrong wrong}
            items.append(("choice", [[("tok", other(t))], [("tok", t)], [("tok", other(t)), ("tok", other(t))]]))
            want_nodes.append(n + 1); n += 4
        elif i % 3 == 2:                                     # an optional wrong word before the right one
            items += [("choice", [[("tok", other(t))], []]), ("tok", t)]
            want_nodes.append(n + 1); n += 2
        else:
            items.append(("tok", t))
            want_nodes.append(n); n += 1
    res = eng.align_graph([TokenGraph(*G.build(items))], [(0, 1)])[0]
    assert res.nodes == want_nodes and res.tokens == toks
    assert fields(res) == fields(plain)


def test_optional_wildcards_between_all_tokens_stay_empty_under_a_bias(enc):
    eng, _, toks, plain = enc
    items = []
    for i, t in enumerate(toks):
        if i:
            items.append(("choice", [[("tok", WILDCARD)], []]))
        items.append(("tok", t))
    graph = TokenGraph(*G.build(items))
    res = eng.align_graph([graph], [(0, 1)], -0.5)[0]
    assert WILDCARD not in res.labels and res.nodes == [2 * i for i in range(len(toks))]
    assert fields(res) == fields(plain)
    # without the bias a wildcard ties with the model's best label: still a valid alignment of a reading, never a worse score
    free = eng.align_graph([graph], [(0, 1)], 0.0)[0]
    assert np.float32(free.score) >= np.float32(plain.score)
    assert R.collapse(free.labels, eng.cfg.blank_id).tolist() == [graph.tokens[j] for j in free.nodes]
    assert all(b2 > e1 for e1, b2 in zip(free.end, free.begin[1:]))


def test_requests_that_are_refused(enc):
    eng, _, toks, _ = enc
    chain = TokenGraph.chain(toks)
    with pytest.raises(RvbError, match="sequence 0: chunk range outside"):
        eng.align_graph([chain], [(1, 2)])
    with pytest.raises(RvbError, match="wildcard_bias"):
        eng.align_graph([chain], [(0, 1)], 0.25)
    with pytest.raises(RvbError, match="sequence 1: node 2: label %d outside" % eng.cfg.vocab):
        eng.align_graph([chain, TokenGraph.chain([1, 2, eng.cfg.vocab])], [(0, 1), (1, 1)])
    with pytest.raises(RvbError, match="infeasible"):
        eng.align_graph([TokenGraph.chain([WILDCARD, WILDCARD] * 400)], [(1, 1)])


def test_alternatives_in_the_transcript_end_to_end(tmp_path):
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
    text = "%s {%s|%s} %s [<star>] [%s] %s [<star>]" % (words[0], wrong, words[1], " ".join(words[2:n // 2]), words[n // 2],
                                                        " ".join(words[n // 2 + 1:]))
    kw = dict(transcript=text, alternatives=True, wildcard="<star>", wildcard_bias=-0.5)
    for fmt in ("ctm", "txt", "ali"):
        assert asr.align(wav, format=fmt, **kw) == asr.align(wav, transcript=plain_text, format=fmt)
    js, ref = asr.align(wav, format="json", **kw), asr.align(wav, transcript=plain_text, format="json")
    assert js["text"] == plain_text and js["score"] == ref["score"]
    nodes = [t.pop("node") for t in js["tokens"]]
    assert js["tokens"] == ref["tokens"] and nodes == sorted(set(nodes))
    with pytest.raises(ValueError, match="alternatives"):
        asr.align(wav, format="json", posteriors=True, **kw)
    with pytest.raises(ValueError, match="alternatives"):
        asr.align(wav, tokens=[1, 2], alternatives=True)
    asr.engine.close()
    # the command-line tool
    tfile = tmp_path / "alt.txt"
    tfile.write_text(text, encoding="utf-8")
    argv = ["--model", mdir, "--audio_file", wav, "--transcript_file", str(tfile), "--result_dir", str(tmp_path / "out"), "--format", "json",
            "--dtype", "f32", "--max_chunks", "4", "--alternatives", "--wildcard", "<star>", "--wildcard_bias", "-0.5"]
    align_wav.main(argv)
    out = json.loads((tmp_path / "out" / "alt.json").read_text(encoding="utf-8"))
    assert out["text"] == plain_text and [t["id"] for t in out["tokens"]] == [t["id"] for t in ref["tokens"]]
    for extra in ("--score", "--posteriors"):                # refused for --alternatives itself, without a wildcard
        with pytest.raises(SystemExit):
            align_wav.get_args(argv[:argv.index("--wildcard")] + [extra])
