"""Token -> word merging with CTC-peak timestamps, and the global model time offset.

Host-side integer-millisecond logic with the behaviour of the reference's
`asr/wenet/bin/ctc_align.py` (`ctc_align` :24-113, `adjust_model_time_offset` :116-138), pinned
by the reference-generated known answer C2 of SURVEY.md Appendix C (tests/test_host_format.py):

  * a piece containing the sentencepiece space mark opens a word (its first character is dropped);
    a `<...>` piece is a word of its own;
  * a word starts 100 ms before its first token's frame (clamped at 0) unless the previous token
    is closer than 100 ms, then at the midpoint frame; it ends at its last token's frame, or at the
    midpoint to the next token when that one is closer than 100 ms;
  * word confidence is the maximum of its tokens' confidences (0 when none are given).

Forced alignment with gaps (Engine.align_wild): a token with the id WILDCARD stands for audio the transcript leaves out.  It is a
word of its own with the caller's marker as its text, it ends the word before it, and its times are those of its run of frames.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional, Sequence, Tuple

SPACE_MARK = "▁"
GAP_MS = 100
WILDCARD = -2          # RVB_CTC_WILDCARD of include/rvb.h


def piece_of(token_id: int, tokenizer) -> str:
    return tokenizer.detokenize([token_id])[1][0]


def _looks_special(text: str) -> bool:
    lo, hi = text.find("<"), text.find(">")
    return lo != -1 and hi != -1 and lo < hi


def _blank_word(text: str) -> bool:
    return text in ("", SPACE_MARK)


def ctc_align(hypothesis: Sequence[int], time_stamp: Sequence[int], confidence_scores: Optional[Sequence[float]],
              tokenizer, frame_shift_ms: int, time_shift_ms: int, wildcard: Optional[str] = None,
              end_stamp: Optional[Sequence[int]] = None) -> List[Dict[str, Any]]:
    """`wildcard` (the marker text) and `end_stamp` (last frame of each token's run) are needed only when `hypothesis` holds
    WILDCARD ids: such a token becomes the word `wildcard` from its first frame to the end of its last one, the word before it
    ends at its own last token, and the word after it does not start before the wildcard ends."""
    assert len(hypothesis) == len(time_stamp)
    n = len(hypothesis)
    wild = [t == WILDCARD for t in hypothesis]
    if any(wild):
        assert wildcard and end_stamp is not None and len(end_stamp) == n
    pieces = [wildcard if w else piece_of(t, tokenizer) for t, w in zip(hypothesis, wild)]

    def begin_ms(i: int) -> int:
        if wild[i]:
            return time_stamp[i] * frame_shift_ms
        ms = max(time_stamp[i] * frame_shift_ms - GAP_MS, 0)
        if i > 0 and wild[i - 1]:
            return max(ms, (end_stamp[i - 1] + 1) * frame_shift_ms)
        if i > 0 and (time_stamp[i] - time_stamp[i - 1]) * frame_shift_ms < GAP_MS:
            ms = (time_stamp[i - 1] + time_stamp[i]) // 2 * frame_shift_ms
        return ms

    def finish_ms(i: int) -> int:
        if wild[i]:
            return (end_stamp[i] + 1) * frame_shift_ms
        ms = time_stamp[i] * frame_shift_ms
        if i < n - 1 and not wild[i + 1] and (time_stamp[i + 1] - time_stamp[i]) * frame_shift_ms < GAP_MS:
            ms = (time_stamp[i + 1] + time_stamp[i]) // 2 * frame_shift_ms
        return ms

    def best_conf(first: int, last: int):
        return max(confidence_scores[first:last + 1]) if confidence_scores else 0

    words: List[Dict[str, Any]] = []
    text, ids, t_begin, first_tok = "", [], -1, -1
    for i, piece in enumerate(pieces):
        following = pieces[i + 1] if i + 1 < n else SPACE_MARK
        if wild[i]:                                                 # a word of its own, whatever the marker looks like
            assert text == ""
            words.append({"word": piece, "unit_id": WILDCARD, "start_time_ms": begin_ms(i) + time_shift_ms,
                          "end_time_ms": finish_ms(i) + time_shift_ms, "confidence": best_conf(i, i), "unit_ids": [WILDCARD]})
            continue
        text += piece[len(SPACE_MARK):] if SPACE_MARK in piece else piece
        ids.append(hypothesis[i])
        if t_begin == -1:
            t_begin, first_tok = begin_ms(i), i

        if not _blank_word(text) and _looks_special(text):          # a <tag> closes immediately
            t_end = finish_ms(i)
            assert t_begin < t_end
            assert len(ids) == 1
            words.append({"word": text, "unit_id": ids[0], "start_time_ms": t_begin + time_shift_ms,
                          "end_time_ms": t_end + time_shift_ms, "confidence": best_conf(first_tok, i),
                          "unit_ids": ids})
            text, ids, t_begin, first_tok = "", [], -1, 0

        if SPACE_MARK in following or _looks_special(following) or (i + 1 < n and wild[i + 1]):    # next piece opens a new word
            t_end = finish_ms(i)
            if not _blank_word(text):
                assert len(ids) > 0
                assert t_begin <= t_end
                assert not _looks_special(text)
                words.append({"word": text, "unit_id": -1, "start_time_ms": t_begin + time_shift_ms,
                              "end_time_ms": t_end + time_shift_ms, "confidence": best_conf(first_tok, i),
                              "unit_ids": ids})
            text, ids, t_begin, first_tok = "", [], -1, 0
    return words


def adjust_model_time_offset(hypothesis: List[Dict[str, Any]], adjustment):
    """Shift every word earlier by up to `adjustment` ms without crossing the (already shifted)
    previous word.  Like the reference, an adjustment of 0 returns None."""
    if adjustment == 0:
        return None
    shifted = []
    for i, word in enumerate(hypothesis):
        assert word["start_time_ms"] >= 0
        assert word["start_time_ms"] <= word["end_time_ms"]
        if i == 0:
            move = min(adjustment, word["start_time_ms"])
        else:
            before = hypothesis[i - 1]
            assert word["start_time_ms"] >= before["end_time_ms"], f"ERROR! {word} >= {before}"
            move = min(adjustment, word["start_time_ms"] - before["end_time_ms"])
        assert move >= 0
        word["start_time_ms"] -= move
        word["end_time_ms"] -= move
        shifted.append(word)
    return shifted


def hyps_to_ctm(audio_name: str, path):
    """CTM lines `<audio> 0 <start s> <duration s> <word> <confidence>` (cli/utils.py:4-14)."""
    for w in path:
        start_s = w["start_time_ms"] / 1000
        dur_s = w["end_time_ms"] / 1000 - start_s
        yield f"{audio_name} 0 {start_s:.2f} {dur_s:.2f} {w['word']} {w['confidence']:.2f}"


def hyps_to_txt(path):
    """Plain words (cli/utils.py:16-21)."""
    for w in path:
        yield w["word"]


# ---------------------------------------------------------------- forced alignment of a known transcript (Engine.align)
@dataclass
class AlignResult:
    """One aligned sequence (rvb_ctc_align): frames are numbered within the sequence = the valid encoder frames of its chunks,
    concatenated; `chunk_lens` (valid frames per chunk) and `first_chunk` map a frame back to (chunk, t)."""
    tokens: List[int]
    labels: List[int]                 # per frame: token id or blank id (the reference's force_align output)
    begin: List[int]                  # per token: first / last frame of its run
    end: List[int]
    peak: List[int]                   # per token: the frame of its run where its log-prob is largest
    confidence: List[float]           # per token: exp of that log-prob
    score: float                      # fp32 Viterbi path score
    first_chunk: int = 0
    chunk_lens: List[int] = field(default_factory=list)
    nodes: Optional[List[int]] = None     # Engine.align_graph: the graph node of each entry of `tokens` (the chosen path)

    @property
    def wildcard(self) -> List[bool]:
        """per token: it is a wildcard (Engine.align_wild); its frames carry WILDCARD in `labels`"""
        return [int(t) == WILDCARD for t in self.tokens]

    def chunk_frame(self, frame: int) -> Tuple[int, int]:
        """sequence frame -> (chunk index in the encoded batch, frame inside that chunk)"""
        if frame < 0:
            raise ValueError("negative frame")
        for i, n in enumerate(self.chunk_lens):
            if frame < n:
                return self.first_chunk + i, frame
            frame -= n
        raise ValueError("frame past the end of the sequence")


@dataclass
class Hit:
    """One occurrence of a phrase (Engine.find / rvb_ctc_find): frames are numbered within the searched sequence (the valid encoder
    frames of its chunks, concatenated); `chunk` / `frame_in_chunk` place start_frame in the encoded batch.  score is the fp32 path
    score in nats (<= 0; 0 = the model's greedy labels spell the phrase), score_per_token = score / tokens of the phrase."""
    start_frame: int
    end_frame: int                    # the first frame of the last token
    score: float
    score_per_token: float
    chunk: int
    frame_in_chunk: int


@dataclass
class DecodeLike:
    """What get_output reads of a DecodeResult."""
    tokens: List[int]
    times: List[int]
    tokens_confidence: List[float]
    ctc_frames: Optional[List[int]] = None
    ends: Optional[List[int]] = None          # last frame of each token's run: what a wildcard's word ends at


def split_by_chunk(res: AlignResult, ends: bool = False):
    """The aligned tokens as one (tokens, times, tokens_confidence) triple per chunk of the sequence, a token going to the chunk
    its `begin` frame lies in, times = begin frames relative to that chunk: what `get_output` takes from a DecodeResult per chunk
    (the first frame of a token's run is also what ctc_greedy_search stamps a token with).  ends=True adds a fourth list, the last
    frames alike.  A wildcard whose run crosses into further chunks appears once in each of them, with the frames it has there."""
    parts = [([], [], [], []) for _ in res.chunk_lens]
    for tok, b, e, conf in zip(res.tokens, res.begin, res.end, res.confidence):
        while True:
            c, t = res.chunk_frame(b)
            part = parts[c - res.first_chunk]
            last = t + (e - b)
            room = res.chunk_lens[c - res.first_chunk] - 1
            part[0].append(int(tok)); part[1].append(int(t)); part[2].append(float(conf)); part[3].append(int(min(last, room)))
            if int(tok) != WILDCARD or last <= room:
                break
            b += room - t + 1
    return parts if ends else [p[:3] for p in parts]


def split_transcript(transcript: str, marker: str, tokenize) -> List[int]:
    """Text with gap markers -> token ids: the text is split at `marker`, each piece goes through `tokenize` (text -> ids) as a
    transcript of its own, the pieces are joined with WILDCARD, and markers with nothing but white space between them are one."""
    if not marker:
        raise ValueError("the wildcard marker is empty")
    ids: List[int] = []
    for k, piece in enumerate(transcript.split(marker)):
        if k and (not ids or ids[-1] != WILDCARD):
            ids.append(WILDCARD)
        if piece.strip():
            ids.extend(int(t) for t in tokenize(piece.strip()))
    return ids


def align_to_ali(audio_name: str, res: AlignResult, wildcard: Optional[str] = None) -> str:
    """The reference's result line: `<key> [label, label, ...]` (asr/wenet/bin/alignment.py:242); a wildcard's frames carry the
    marker in place of an id."""
    if wildcard is None or WILDCARD not in res.labels:
        return "{} {}".format(audio_name, [int(x) for x in res.labels])
    return "{} [{}]".format(audio_name, ", ".join(wildcard if int(x) == WILDCARD else str(int(x)) for x in res.labels))


def align_to_json(res: AlignResult, tokenizer, chunk_size: int, input_frame_ms: int, output_frame_ms: int,
                  wildcard: Optional[str] = None) -> Dict[str, Any]:
    """Per token: piece, id, start_ms = chunk shift + begin * frame, end_ms = chunk shift + (end + 1) * frame (both inside the chunk the
    frame lies in), confidence; plus the sequence score.  A wildcard has the marker as its piece and "wildcard": true; a result of
    Engine.align_graph carries the graph node of each token as "node"."""
    def ms(frame: int, extra: int) -> int:
        c, t = res.chunk_frame(frame)
        return c * chunk_size * input_frame_ms + (t + extra) * output_frame_ms

    toks = []
    for tok, b, e, conf in zip(res.tokens, res.begin, res.end, res.confidence):
        wild = int(tok) == WILDCARD
        toks.append({"piece": (wildcard or "") if wild else piece_of(int(tok), tokenizer), "id": int(tok), "start_ms": ms(b, 0),
                     "end_ms": ms(e, 1), "confidence": float(conf)})
        if wild:
            toks[-1]["wildcard"] = True
    for tok, node in zip(toks, res.nodes or []):
        tok["node"] = int(node)
    return {"score": float(res.score), "tokens": toks}


def posteriors_to_json(res: AlignResult, post: Dict[str, Any], chunk_size: int, input_frame_ms: int, output_frame_ms: int) -> List[Dict[str, Any]]:
    """Per token, from Engine.score(..., posteriors=True) of the same sequence: occupancy (expected frames), mean_time (ms; the
    posterior-weighted mean frame through the frame -> ms conversion of align_to_json, the fraction of a frame kept) and
    peak_posterior."""
    def ms(frame: float) -> float:
        whole = min(max(int(frame), 0), sum(res.chunk_lens) - 1)
        c, t = res.chunk_frame(whole)
        return c * chunk_size * input_frame_ms + (t + frame - whole) * output_frame_ms

    return [{"occupancy": float(o), "mean_time": float(ms(float(m))), "peak_posterior": float(p)}
            for o, m, p in zip(post["occupancy"], post["mean_frame"], post["peak_posterior"])]
