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
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional, Sequence, Tuple

SPACE_MARK = "▁"
GAP_MS = 100


def piece_of(token_id: int, tokenizer) -> str:
    return tokenizer.detokenize([token_id])[1][0]


def _looks_special(text: str) -> bool:
    lo, hi = text.find("<"), text.find(">")
    return lo != -1 and hi != -1 and lo < hi


def _blank_word(text: str) -> bool:
    return text in ("", SPACE_MARK)


def ctc_align(hypothesis: Sequence[int], time_stamp: Sequence[int], confidence_scores: Optional[Sequence[float]],
              tokenizer, frame_shift_ms: int, time_shift_ms: int) -> List[Dict[str, Any]]:
    assert len(hypothesis) == len(time_stamp)
    n = len(hypothesis)
    pieces = [piece_of(t, tokenizer) for t in hypothesis]

    def begin_ms(i: int) -> int:
        ms = max(time_stamp[i] * frame_shift_ms - GAP_MS, 0)
        if i > 0 and (time_stamp[i] - time_stamp[i - 1]) * frame_shift_ms < GAP_MS:
            ms = (time_stamp[i - 1] + time_stamp[i]) // 2 * frame_shift_ms
        return ms

    def finish_ms(i: int) -> int:
        ms = time_stamp[i] * frame_shift_ms
        if i < n - 1 and (time_stamp[i + 1] - time_stamp[i]) * frame_shift_ms < GAP_MS:
            ms = (time_stamp[i + 1] + time_stamp[i]) // 2 * frame_shift_ms
        return ms

    def best_conf(first: int, last: int):
        return max(confidence_scores[first:last + 1]) if confidence_scores else 0

    words: List[Dict[str, Any]] = []
    text, ids, t_begin, first_tok = "", [], -1, -1
    for i, piece in enumerate(pieces):
        following = pieces[i + 1] if i + 1 < n else SPACE_MARK
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

        if SPACE_MARK in following or _looks_special(following):    # next piece opens a new word
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
class DecodeLike:
    """What get_output reads of a DecodeResult."""
    tokens: List[int]
    times: List[int]
    tokens_confidence: List[float]
    ctc_frames: Optional[List[int]] = None


def split_by_chunk(res: AlignResult):
    """The aligned tokens as one (tokens, times, tokens_confidence) triple per chunk of the sequence, a token going to the chunk
    its `begin` frame lies in, times = begin frames relative to that chunk: what `get_output` takes from a DecodeResult per chunk
    (the first frame of a token's run is also what ctc_greedy_search stamps a token with)."""
    parts = [([], [], []) for _ in res.chunk_lens]
    for tok, b, conf in zip(res.tokens, res.begin, res.confidence):
        c, t = res.chunk_frame(b)
        part = parts[c - res.first_chunk]
        part[0].append(int(tok)); part[1].append(int(t)); part[2].append(float(conf))
    return parts


def align_to_ali(audio_name: str, res: AlignResult) -> str:
    """The reference's result line: `<key> [label, label, ...]` (asr/wenet/bin/alignment.py:242)."""
    return "{} {}".format(audio_name, [int(x) for x in res.labels])


def align_to_json(res: AlignResult, tokenizer, chunk_size: int, input_frame_ms: int, output_frame_ms: int) -> Dict[str, Any]:
    """Per token: piece, id, start_ms = chunk shift + begin * frame, end_ms = chunk shift + (end + 1) * frame (both inside the chunk the
    frame lies in), confidence; plus the sequence score."""
    def ms(frame: int, extra: int) -> int:
        c, t = res.chunk_frame(frame)
        return c * chunk_size * input_frame_ms + (t + extra) * output_frame_ms

    toks = [{"piece": piece_of(int(tok), tokenizer), "id": int(tok), "start_ms": ms(b, 0), "end_ms": ms(e, 1), "confidence": float(conf)}
            for tok, b, e, conf in zip(res.tokens, res.begin, res.end, res.confidence)]
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
