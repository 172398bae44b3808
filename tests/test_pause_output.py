"""get_output with per-chunk start frames (chunking="pauses") and the keywords of the host layers, on hand-made DecodeResults.  No GPU."""
import pytest

from reverb_amd.bin import recognize_wav
from reverb_amd.ctc_align import GAP_MS
from reverb_amd.engine import _check_chunking
from reverb_amd.reverb import _check_pause_args, get_output
from reverb_amd.search import DecodeResult
from reverb_amd.tokenizer import RevBpeTokenizer

TABLE = {"<blank>": 0, "▁he": 1, "llo": 2, "▁wor": 3, "ld": 4, "<laugh>": 5, "▁a": 6}


def tok():
    return RevBpeTokenizer(None, dict(TABLE))


def _hyps():
    return [DecodeResult([1, 2], times=[3, 5], tokens_confidence=[0.9, 0.8]),
            DecodeResult([], times=[], tokens_confidence=[]),
            DecodeResult([6, 3, 4], times=[10, 30, 31], tokens_confidence=[0.7, 0.6, 0.5]),
            DecodeResult([5], times=[5], tokens_confidence=[0.4])]


def test_every_pieces_first_word_starts_at_its_own_start_frame():
    starts, adjust = [0, 1500, 1987, 3333], 230
    lines = get_output("ctm", tok(), "x.wav", _hyps(), adjust, 2051, 10, 40, chunk_starts=starts).split("\n")
    assert [ln.split()[4] for ln in lines] == ["hello", "a", "world", "<laugh>"]
    first_of_piece = {0: lines[0], 2: lines[1], 3: lines[3]}
    for k, line in first_of_piece.items():
        t = _hyps()[k].times[0]
        begin = starts[k] * 10 + max(t * 40 - GAP_MS, 0)              # ctc_align's word start, shifted by start_k * 10 ms
        want = begin - min(adjust, begin if k == 0 else adjust)          # the existing adjustment: never below the previous word's end
        assert float(line.split()[2]) == pytest.approx(want / 1000.0, abs=0.0051), (k, line)
    assert lines[1] == "x.wav 0 19.94 0.10 a 0.70" and lines[3] == "x.wav 0 33.20 0.10 <laugh> 0.40"


def test_none_keeps_the_fixed_arithmetic():
    fixed = get_output("ctm", tok(), "x.wav", _hyps(), 230, 2051, 10, 40)
    assert fixed == get_output("ctm", tok(), "x.wav", _hyps(), 230, 2051, 10, 40, chunk_starts=None)
    assert fixed == get_output("ctm", tok(), "x.wav", _hyps(), 230, 2051, 10, 40, chunk_starts=[0, 2051, 4102, 6153])
    assert get_output("txt", tok(), "x.wav", _hyps(), 230, 2051, 10, 40, chunk_starts=[0, 7, 20, 90]) == "hello a world <laugh>"
    with pytest.raises(ValueError, match="chunk starts"):
        get_output("ctm", tok(), "x.wav", _hyps(), 230, 2051, 10, 40, chunk_starts=[0, 7])


def test_keywords_are_checked():
    _check_pause_args("fixed", True)
    _check_pause_args("pauses", False)
    with pytest.raises(NotImplementedError, match="simulate_streaming"):
        _check_pause_args("pauses", True)
    for check in (_check_chunking, lambda c: _check_pause_args(c, False)):
        with pytest.raises(ValueError, match="chunking"):
            check("pause")


def test_command_line_flags():
    base = ["--audio_file", "a.wav", "--result_dir", "r"]
    a = recognize_wav.get_args(base)
    assert (a.chunking, a.pause_search_frames, a.pause_smooth_frames) == ("fixed", None, 10)
    a = recognize_wav.get_args(base + ["--chunking", "pauses", "--pause_search_frames", "300", "--pause_smooth_frames", "5"])
    assert (a.chunking, a.pause_search_frames, a.pause_smooth_frames) == ("pauses", 300, 5)
    with pytest.raises(SystemExit):
        recognize_wav.get_args(base + ["--chunking", "silence"])
