"""Wildcard alignment without a GPU: properties of the definition itself (the numpy restatement tests/force_align_ref.py on the log-probs
with the column w + bias appended and the wildcard as label V), so that the semantics are pinned independently of the kernel; the
splitting of a transcript at its gap markers; the CTM / label / JSON rendering of a result with wildcards.

The planted case.  Logits are N(0, 1) with +12 on a planted valid path, so the planted label is the strict arg-max of every frame (this
is asserted) and w[t] = lp[t][path[t]].  A middle span of the transcript is replaced by ONE wildcard; "the removed span" is the frames
from the first frame of the first removed token to the last frame of the last removed token.
  * bias = 0.  The labelling "kept tokens as planted, wildcard on the removed span" scores sum(w), which no path can beat, and a path
    reaches it only if every frame carries its arg-max label or the wildcard.  So a kept token can lose frames only to the wildcard,
    at equal score (a tie), and only the two neighbours of the gap can: the tie rule (stay first) lets a state begin as early as it
    can, so the wildcard may take all but the first frame of the token before it; every kept token keeps at least one frame.
  * bias = -0.5.  A wildcard frame is 0.5 worse than the arg-max label and an off-path label at least (12 - spread) worse, so the
    optimum gives the wildcard exactly the removed span and everything else stays as planted, blanks included."""
import numpy as np
import pytest

import force_align_ref as R
from reverb_amd.ctc_align import WILDCARD, AlignResult, align_to_ali, align_to_json, ctc_align, hyps_to_ctm, split_by_chunk, split_transcript

V, BLANK, T, L = 24, 0, 400, 60
LO, HI = 20, 35            # tokens [LO, HI) are left out of the transcript


def planted():
    rng = np.random.default_rng(77)
    y = rng.integers(1, V, L).astype(np.int64)
    for i in range(1, L):                                   # no adjacent repeats: every token of the path is entered by a skip or a blank
        while y[i] == y[i - 1]:
            y[i] = rng.integers(1, V)
    path = R.planted_path(rng, y, T, BLANK)
    logits = rng.standard_normal((T, V)).astype(np.float32)
    logits[np.arange(T), path] += np.float32(12.0)
    m = logits.max(1, keepdims=True)
    lp = (logits - m - np.log(np.exp(logits - m).sum(1, keepdims=True, dtype=np.float32))).astype(np.float32)
    assert np.array_equal(lp.argmax(1), path) and np.all(np.sort(lp, 1)[:, -1] > np.sort(lp, 1)[:, -2])
    # token index of every frame of the planted path (-1 on blank frames)
    starts = np.ones(T, bool)
    starts[1:] = path[1:] != path[:-1]
    tok_of = np.where(path != BLANK, np.cumsum(starts & (path != BLANK)) - 1, -1)
    assert tok_of.max() == L - 1
    return lp, y, path, tok_of


CASE = planted()


def align_edited(bias):
    lp, y, path, tok_of = CASE
    w = lp.max(1)
    ext = np.ascontiguousarray(np.concatenate([lp, (w + np.float32(bias)).astype(np.float32)[:, None]], 1))
    edited = np.concatenate([y[:LO], [V], y[HI:]])
    labels, score = R.force_align(ext, edited, BLANK)
    return labels, score, edited


@pytest.mark.parametrize("bias", [0.0, -0.5])
def test_a_wildcard_takes_the_span_the_transcript_leaves_out(bias):
    lp, y, path, tok_of = CASE
    labels, score, edited = align_edited(bias)
    assert R.collapse(labels, BLANK).tolist() == edited.tolist()
    removed = np.nonzero((tok_of >= LO) & (tok_of < HI))[0]
    r0, r1 = removed[0], removed[-1]
    run = np.nonzero(labels == V)[0]
    assert run.size >= 1 and np.all(np.diff(run) == 1)
    kept = (tok_of >= 0) & ((tok_of < LO) | (tok_of >= HI))
    neighbour = (tok_of == LO - 1) | (tok_of == HI)
    if bias == 0.0:
        assert np.float32(score).tobytes() == R.force_align(lp, y, BLANK)[1].tobytes()      # the same addends in the same order
        strict = kept & ~neighbour
        assert np.all(labels[strict] == path[strict])
        assert np.all((labels[kept] == path[kept]) | (labels[kept] == V))
        for k in (LO - 1, HI):                               # a neighbour of the gap keeps at least one frame
            assert np.any(labels[tok_of == k] == y[k])
        # the run: the removed span, the blanks next to it and the neighbours' tie frames
        ext0 = np.nonzero(tok_of == LO - 1)[0][0] + 1
        ext1 = np.nonzero(tok_of == HI)[0][-1] - 1
        assert ext0 <= run[0] and run[-1] <= ext1 and run[0] <= r0 and r1 <= run[-1]
    else:
        assert np.all((labels[kept] == path[kept]) | (labels[kept] == BLANK))
        assert np.all(labels[kept] == path[kept])            # ... and here not even a blank takes a kept token's frame
        assert run[0] == r0 and run[-1] == r1
        outside = np.ones(T, bool); outside[r0:r1 + 1] = False
        assert np.all(labels[outside] == path[outside])
        assert abs(float(score) - (float(R.force_align(lp, y, BLANK)[1]) + bias * run.size)) < 1e-3


def test_leading_and_trailing_wildcards_give_a_free_start_and_end():
    lp, y, path, tok_of = CASE
    w = lp.max(1)
    ext = np.ascontiguousarray(np.concatenate([lp, (w - np.float32(0.5))[:, None]], 1))
    edited = np.concatenate([[V], y[LO:HI], [V]])
    labels, _ = R.force_align(ext, edited, BLANK)
    assert R.collapse(labels, BLANK).tolist() == edited.tolist()
    inside = (tok_of >= LO) & (tok_of < HI)
    assert np.all(labels[inside] == path[inside])
    first, last = np.nonzero(inside)[0][[0, -1]]
    head, tail = np.nonzero(labels[:first] == V)[0], np.nonzero(labels[last:] == V)[0] + last
    assert head[0] == np.nonzero(tok_of == 0)[0][0] and tail[-1] == np.nonzero(tok_of == L - 1)[0][-1]


# ------------------------------------------------------------------------------------ transcript handling and rendering (host)
def _tokenize(text):
    return [int(x) for x in text.split()]


def test_transcript_is_split_at_the_marker_and_markers_merge():
    S = "<star>"
    assert split_transcript("1 2 3", S, _tokenize) == [1, 2, 3]
    assert split_transcript("1 2 <star> 3", S, _tokenize) == [1, 2, WILDCARD, 3]
    assert split_transcript("<star> 1 2<star>3 <star>", S, _tokenize) == [WILDCARD, 1, 2, WILDCARD, 3, WILDCARD]
    assert split_transcript("1 <star><star>  <star> 2", S, _tokenize) == [1, WILDCARD, 2]
    assert split_transcript("<star>", S, _tokenize) == [WILDCARD]
    assert split_transcript(" <star> <star> ", S, _tokenize) == [WILDCARD]
    assert split_transcript("1 *** 2", "***", _tokenize) == [1, WILDCARD, 2]
    with pytest.raises(ValueError):
        split_transcript("1 2", "", _tokenize)


class _Tok:
    PIECES = {7: "▁he", 8: "llo", 9: "▁world", 10: "▁again"}

    def detokenize(self, ids):
        return None, [self.PIECES[i] for i in ids]


def _result():
    # two chunks of 12 and 6 valid frames; "hello", a gap that runs over the chunk boundary, "world", a one-frame gap, "again"
    labels = [0, 7, 8, 8] + [WILDCARD] * 10 + [9, WILDCARD, 10, 0]
    return AlignResult(tokens=[7, 8, WILDCARD, 9, WILDCARD, 10], labels=labels, begin=[1, 2, 4, 14, 15, 16], end=[1, 3, 13, 14, 15, 16],
                       peak=[1, 2, 6, 14, 15, 16], confidence=[0.5, 0.25, 0.9, 0.75, 0.8, 0.6], score=-3.5, first_chunk=0,
                       chunk_lens=[12, 6])


def test_rendering_of_a_result_with_wildcards():
    res = _result()
    assert res.wildcard == [False, False, True, False, True, False]
    # without ends: the triples align() has always produced
    assert split_by_chunk(res)[0] == ([7, 8, WILDCARD], [1, 2, 4], [0.5, 0.25, 0.9])
    parts = split_by_chunk(res, ends=True)
    assert parts[0] == ([7, 8, WILDCARD], [1, 2, 4], [0.5, 0.25, 0.9], [1, 3, 11])
    assert parts[1] == ([WILDCARD, 9, WILDCARD, 10], [0, 2, 3, 4], [0.9, 0.75, 0.8, 0.6], [1, 2, 3, 4])
    assert align_to_ali("a.wav", res, "<star>") == "a.wav [0, 7, 8, 8, " + "<star>, " * 10 + "9, <star>, 10, 0]"
    js = align_to_json(res, _Tok(), chunk_size=2051, input_frame_ms=10, output_frame_ms=40, wildcard="<star>")
    assert js["tokens"][2] == {"piece": "<star>", "id": WILDCARD, "start_ms": 160, "end_ms": 20510 + 80, "confidence": 0.9, "wildcard": True}
    assert js["tokens"][4]["wildcard"] is True and js["tokens"][4]["end_ms"] - js["tokens"][4]["start_ms"] == 40
    assert [("wildcard" in t) for t in js["tokens"]] == res.wildcard
    # words of the first chunk: the wildcard ends "hello" and is a word of its own over its frames
    toks, times, conf, ends = parts[0]
    words = ctc_align(toks, times, conf, _Tok(), 40, 0, "<star>", ends)
    assert [w["word"] for w in words] == ["hello", "<star>"]
    assert (words[0]["start_time_ms"], words[0]["end_time_ms"]) == (0, 80)           # ends at its last token, not midway to the gap
    assert (words[1]["start_time_ms"], words[1]["end_time_ms"], words[1]["confidence"]) == (160, 480, 0.9)
    toks, times, conf, ends = parts[1]
    words = ctc_align(toks, times, conf, _Tok(), 40, 20510, "<star>", ends)
    assert [w["word"] for w in words] == ["<star>", "world", "<star>", "again"]
    t = [(w["start_time_ms"] - 20510, w["end_time_ms"] - 20510) for w in words]
    assert t[0] == (0, 80) and t[2] == (120, 160)
    assert t[1][0] >= t[0][1] and t[3][0] >= t[2][1]                                  # a word does not start inside the gap before it
    assert all(b <= e for b, e in t) and all(a[1] <= b[0] for a, b in zip(t, t[1:]))
    lines = list(hyps_to_ctm("a.wav", words))
    assert lines[0] == "a.wav 0 20.51 0.08 <star> 0.90" and lines[2].split()[4] == "<star>"
    # a marker that does not look like a tag is a word of its own all the same
    assert [w["word"] for w in ctc_align(toks, times, conf, _Tok(), 40, 0, "***", ends)] == ["***", "world", "***", "again"]
    # and without wildcards the two new arguments change nothing
    assert ctc_align([7, 8, 9], [1, 2, 9], [0.5, 0.25, 0.75], _Tok(), 40, 0) == \
        ctc_align([7, 8, 9], [1, 2, 9], [0.5, 0.25, 0.75], _Tok(), 40, 0, "<star>", [1, 3, 9])
