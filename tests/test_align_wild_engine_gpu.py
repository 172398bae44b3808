"""Forced alignment with wildcards through the engine (rvb_ctc_align_wild / Engine.align_wild / ReverbASR.align(wildcard=...)) on the
tiny fp32 model and the 25 s of synthetic audio in two chunks that test_align_engine_gpu.py uses; the transcript is the greedy tokens.

Where a bound is needed it is derived.  The Viterbi recurrence is max and fp32 addition, both monotone, so by induction over the
frames alpha[t][s] is at least the fp32 left-to-right sum of ANY path that ends in (t, s).  Relabel the plain alignment's path: the
frames of the removed tokens and of the blanks between them become the wildcard, whose emission w[t] is at least every lp[t][v].  That
is a path of the edited transcript whose every addend is at least the plain path's, so score_wild >= score_plain holds exactly, with no
tolerance.  From above nothing beats the per-frame maximum: score_wild <= sum of the top-1 values, up to the rounding bound
T * 2^-24 * |sum| of test_align_engine_gpu.py."""
import numpy as np
import pytest

import force_align_ref as R
from reverb_amd import synth
from reverb_amd._lib import RvbError, check, iptr
from reverb_amd.ctc_align import WILDCARD
from reverb_amd.engine import Engine

pytestmark = pytest.mark.gpu
CHUNK = 2051
EPS = 2.0 ** -24


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
    v, _ = eng.ctc_topk()
    T0 = int(eng.encoder_lens()[0])
    top1 = v[0, :T0, 0].copy()
    toks = list(greedy[0].tokens)
    assert len(toks) >= 12 and T0 >= 500
    plain = eng.align([toks], [(0, 1)])[0]
    yield eng, greedy, toks, plain, top1
    eng.close()


def edits(toks):
    n = len(toks)
    return {"middle": toks[:n // 3] + [WILDCARD] + toks[2 * n // 3:], "first": [WILDCARD] + toks[1:], "last": toks[:-1] + [WILDCARD]}


def test_without_a_wildcard_it_is_align_bit_for_bit(enc):
    eng, greedy, toks, plain, _ = enc
    seqs = [g.tokens for g in greedy if g.tokens]
    ranges = [(b, 1) for b, g in enumerate(greedy) if g.tokens]
    for bias in (0.0, -3.0):
        a, w = eng.align(seqs, ranges), eng.align_wild(seqs, ranges, bias)
        assert a == w                                       # dataclass equality: every field, floats included
        for x, y in zip(a, w):
            assert np.array(x.confidence, np.float32).tobytes() == np.array(y.confidence, np.float32).tobytes()
            assert np.float32(x.score).tobytes() == np.float32(y.score).tobytes() and not any(y.wildcard)
    assert eng.align_wild([toks], [(0, 1)])[0] == plain


@pytest.mark.parametrize("which", ["middle", "first", "last"])
def test_score_lies_between_the_plain_score_and_the_top1_sum(enc, which):
    eng, _, toks, plain, top1 = enc
    ed = edits(toks)[which]
    res = eng.align_wild([ed], [(0, 1)], 0.0)[0]
    assert R.collapse(res.labels, eng.cfg.blank_id).tolist() == ed
    assert res.wildcard == [t == WILDCARD for t in ed]
    want = float(np.sum(top1.astype(np.float64)))
    T = len(top1)
    print("%s: score_wild %.6f score_plain %.6f top-1 sum %.6f bound %.3g" % (which, res.score, plain.score, want, T * EPS * abs(want)))
    assert np.float32(res.score) >= np.float32(plain.score)
    assert res.score <= want + T * EPS * abs(want)
    k = ed.index(WILDCARD)
    b, e = res.begin[k], res.end[k]
    assert res.labels[b:e + 1] == [WILDCARD] * (e - b + 1) and b <= res.peak[k] <= e
    # peak = the frame of the run with the largest top-1 value (first on ties), confidence = exp of it, without the bias
    assert res.peak[k] == b + int(np.argmax(top1[b:e + 1]))
    assert np.isclose(res.confidence[k], np.exp(np.float64(top1[res.peak[k]])), rtol=1e-5)
    assert all(0.0 < c <= 1.0 for c in res.confidence)
    assert all(b2 > e1 for e1, b2 in zip(res.end, res.begin[1:]))
    biased = eng.align_wild([ed], [(0, 1)], -0.5)[0]
    assert np.isclose(biased.confidence[k], np.exp(np.float64(top1[biased.peak[k]])), rtol=1e-5)
    assert np.float32(biased.score) <= np.float32(res.score)


@pytest.mark.parametrize("which", ["middle", "first", "last"])
def test_a_heavy_bias_pushes_the_tokens_back(enc, which):
    """wildcard_bias = -50 with every log-prob above -49: a path with the wildcard on k >= 2 frames loses to the same path with the
    wildcard on its first frame only and the blank state after it on the other k - 1 (valid for every transcript: the blank follows
    the wildcard's state), which gains more than 1 nat per frame, far above the rounding of the sums.  So the run is one frame."""
    eng, _, toks, plain, _ = enc
    lp = eng.ctc_logprobs(0)[:len(plain.labels)]
    assert lp.min() > -49.0, "precondition of the argument: min log-prob %.3f" % lp.min()
    ed = edits(toks)[which]
    res = eng.align_wild([ed], [(0, 1)], -50.0)[0]
    assert R.collapse(res.labels, eng.cfg.blank_id).tolist() == ed
    k = ed.index(WILDCARD)
    assert res.begin[k] == res.end[k] == res.peak[k] and res.labels.count(WILDCARD) == 1


def test_a_spliced_out_stretch_leaves_the_rest_in_place(enc):
    """the transcript misses what was said in frames 200 .. 400 of chunk 0; one wildcard stands there"""
    eng, _, toks, plain, _ = enc
    gone = [i for i, b in enumerate(plain.begin) if 200 <= b <= 400]
    assert gone and gone == list(range(gone[0], gone[-1] + 1)) and 0 < gone[0] and gone[-1] < len(toks) - 1
    ed = toks[:gone[0]] + [WILDCARD] + toks[gone[-1] + 1:]
    res = eng.align_wild([ed], [(0, 1)], 0.0)[0]
    assert R.collapse(res.labels, eng.cfg.blank_id).tolist() == ed
    new_of = {i: (i if i < gone[0] else i - len(gone) + 1) for i in range(len(toks)) if i not in gone}
    far = [i for i in new_of if plain.end[i] < 150 or plain.begin[i] > 450]
    assert len(far) >= 4
    shift = max(max(abs(res.begin[new_of[i]] - plain.begin[i]), abs(res.end[new_of[i]] - plain.end[i])) for i in far)
    k = gone[0]
    print("wildcard run %d .. %d, largest shift of a far token %d frames (%d far tokens)" % (res.begin[k], res.end[k], shift, len(far)))
    assert shift <= 2
    assert res.begin[k] <= 200 + 2 and res.end[k] >= plain.end[gone[-1]] - 2


def test_marker_in_the_transcript_end_to_end(tmp_path):
    from reverb_amd.reverb import load_model
    mdir = synth.write_model_dir(str(tmp_path / "m"), "tiny")
    wav = str(tmp_path / "gap.wav")
    synth.write_wav(wav, synth.synth_audio(25.0, seed=41))
    asr = load_model(mdir, gpu=0, dtype="f32", max_chunks=4)
    words = asr.transcribe(wav, mode="ctc_greedy_search", format="txt").split()
    n = len(words)
    assert n >= 9
    text = " ".join(["<star>"] + words[1:n // 3] + ["<star>", "<star>"] + words[2 * n // 3:])
    ctm = [l.split() for l in asr.align(wav, transcript=text, format="ctm", wildcard="<star>").split("\n")]
    assert [l[4] for l in ctm] == ["<star>"] + words[1:n // 3] + ["<star>"] + words[2 * n // 3:]
    start = [float(l[2]) for l in ctm]
    assert all(b >= a for a, b in zip(start, start[1:])) and start[0] >= 0.0
    marks = [l for l in ctm if l[4] == "<star>"]
    assert len(marks) == 2 and all(float(l[3]) > 0.0 and 0.0 < float(l[5]) <= 1.0 for l in marks)
    js = asr.align(wav, transcript=text, format="json", wildcard="<star>")
    assert [t["piece"] for t in js["tokens"] if t.get("wildcard")] == ["<star>", "<star>"]
    assert all(t["start_ms"] < t["end_ms"] for t in js["tokens"])
    ali = asr.align(wav, transcript=text, format="ali", wildcard="<star>")
    assert ali.startswith("gap.wav [") and "<star>" in ali and len(ali.split(",")) == int(asr.engine.encoder_lens().sum())
    # without the keyword the marker is text like any other, and align() is what it was
    plain_text = " ".join(words)
    assert asr.align(wav, transcript=plain_text, format="ctm", wildcard="<star>") == asr.align(wav, transcript=plain_text, format="ctm")
    with pytest.raises(ValueError, match="posteriors"):
        asr.align(wav, transcript=text, format="json", wildcard="<star>", posteriors=True)
    asr.engine.close()


def test_requests_that_are_refused():
    cfg, sd = synth.calibrated_state_dict("tiny")
    eng = Engine(cfg, sd, dtype="f32", device=0, max_chunks=4, chunk_frames=CHUNK)
    one, zero = np.ones(1, np.int32), np.zeros(1, np.int32)
    rc = eng.lib.rvb_ctc_align_wild(eng.handle, iptr(one), iptr(one), 1, iptr(zero), iptr(one), 0.0, None, None, None, None, None, None)
    assert rc == -3                                         # RVB_E_STATE
    with pytest.raises(RvbError, match="before rvb_encode"):
        check(rc, "rvb_ctc_align_wild")
    lens = feats_of(eng, synth.synth_audio(25.0, seed=41))
    eng.encode(None, lens, 2, 0.0, T0=CHUNK)
    with pytest.raises(RvbError, match="outside"):
        eng.align([[1, WILDCARD, 2]], [(0, 1)])              # rvb_ctc_align knows no wildcard
    with pytest.raises(RvbError, match="outside"):
        eng.align_wild([[1, eng.cfg.vocab, 2]], [(0, 1)])
    with pytest.raises(RvbError, match="wildcard_bias"):
        eng.align_wild([[1, WILDCARD, 2]], [(0, 1)], 0.25)
    with pytest.raises(RvbError, match="wildcard_bias"):
        eng.align_wild([[1, WILDCARD, 2]], [(0, 1)], float("nan"))
    with pytest.raises(RvbError, match="infeasible"):
        eng.align_wild([[WILDCARD, WILDCARD] * 400], [(1, 1)])   # 800 tokens + 799 repeats against the short last chunk
    assert eng.align_wild([[1, WILDCARD, 2]], [(0, 1)])[0].labels.count(WILDCARD) >= 1
    eng.close()
