"""Forced alignment without a GPU: the numpy restatement (tests/force_align_ref.py) reproduces the labels the unmodified reference's
force_align returned (tests/golden/force_align.json, scripts/gen_golden_force_align.py); refusals; host rendering of AlignResults; argument
validation of rvb_ctc_align / rvb_test_ctc_viterbi before any device work."""
import ctypes
import json
import os

import numpy as np
import pytest

import force_align_ref as R
from conftest import ROOT
from reverb_amd import _lib
from reverb_amd.ctc_align import AlignResult, align_to_ali, align_to_json, split_by_chunk

GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "force_align.json")))


def test_goldens_cover_the_constructions():
    cases = GOLDEN["cases"]
    assert {c["kind"] for c in cases} == set(R.KINDS)
    assert any(c["L"] == 1 for c in cases) and any(c["T"] == 1 for c in cases)
    assert all(c["T"] * (2 * c["L"] + 1) <= 512 * 201 for c in cases)


@pytest.mark.parametrize("case", GOLDEN["cases"], ids=lambda c: "%s-%d" % (c["kind"], c["seed"]))
def test_restatement_reproduces_the_reference(case):
    lp, y, T = R.make_case(case["seed"], case["T"], case["V"], case["L"], case["kind"])
    assert T == case["T"] == len(case["labels"])
    labels, score = R.force_align(lp, y, GOLDEN["blank"])
    assert labels.tolist() == case["labels"]
    assert R.collapse(labels).tolist() == y.tolist()
    if case["kind"] in ("min_t", "min_t_quant"):
        assert T == R.min_frames(y)
    # the fp32 score is the fp32-accumulated score of its own path, and no path beats the fp64 optimum by more than rounding
    assert abs(R.path_score64(lp, labels) - float(score)) <= T * 2.0 ** -24 * abs(float(score)) + 1e-30
    assert R.path_score64(lp, labels) <= R.optimum64(lp, y) + 1e-9


def test_restatement_refuses_what_has_no_answer():
    lp, y, _ = R.make_case(1, 20, 8, 5, "random")
    with pytest.raises(ValueError, match="empty"):
        R.force_align(lp, np.zeros(0, np.int32))
    with pytest.raises(ValueError, match="token id"):
        R.force_align(lp, np.array([1, 8], np.int32))
    with pytest.raises(ValueError, match="token id"):
        R.force_align(lp, np.array([1, 0, 2], np.int32))
    with pytest.raises(ValueError, match="infeasible"):
        R.force_align(lp[:5], np.array([1, 1, 2, 3, 4], np.int32))          # 5 tokens + 1 repeat need 6 frames
    hole = lp.copy()
    hole[7, :] = -np.inf                                                     # a frame nothing can be emitted in
    with pytest.raises(ValueError, match="finite"):
        R.force_align(hole, y)


def _result():
    # two chunks of 5 and 4 valid frames; tokens 7, 8 in the first chunk, 9 in the second
    return AlignResult(tokens=[7, 8, 9], labels=[0, 7, 7, 0, 8, 0, 9, 9, 0], begin=[1, 4, 6], end=[2, 4, 7], peak=[2, 4, 6],
                       confidence=[0.5, 0.25, 0.75], score=-3.5, first_chunk=0, chunk_lens=[5, 4])


class _Tok:
    def detokenize(self, ids):
        return None, ["p%d" % i for i in ids]


def test_rendering_of_hand_made_results():
    res = _result()
    assert [res.chunk_frame(f) for f in (0, 4, 5, 8)] == [(0, 0), (0, 4), (1, 0), (1, 3)]
    with pytest.raises(ValueError):
        res.chunk_frame(9)
    assert split_by_chunk(res) == [([7, 8], [1, 4], [0.5, 0.25]), ([9], [1], [0.75])]
    assert align_to_ali("a.wav", res) == "a.wav [0, 7, 7, 0, 8, 0, 9, 9, 0]"
    js = align_to_json(res, _Tok(), chunk_size=2051, input_frame_ms=10, output_frame_ms=40)
    assert js["score"] == -3.5
    assert js["tokens"][0] == {"piece": "p7", "id": 7, "start_ms": 40, "end_ms": 120, "confidence": 0.5}
    assert js["tokens"][1] == {"piece": "p8", "id": 8, "start_ms": 160, "end_ms": 200, "confidence": 0.25}
    assert js["tokens"][2] == {"piece": "p9", "id": 9, "start_ms": 20510 + 40, "end_ms": 20510 + 120, "confidence": 0.75}
    res.first_chunk = 3                                                       # a sequence that starts at chunk 3 of the batch
    assert res.chunk_frame(5) == (4, 0)


def _hook(lib, lp, y, blank=0, slab=8192, T=None, V=None, L=None):
    lp = np.ascontiguousarray(lp, np.float32)
    y = np.ascontiguousarray(y, np.int32)
    T = lp.shape[0] if T is None else T
    labels = np.full(max(min(T, 1 << 16), 1), -7, np.int32)
    score = np.full(1, 123.0, np.float32)
    rc = lib.rvb_test_ctc_viterbi(_lib.fptr(lp), T, lp.shape[1] if V is None else V, _lib.iptr(y), len(y) if L is None else L, blank, slab,
                                  _lib.iptr(labels), _lib.fptr(score))
    assert rc == 0 or (np.all(labels == -7) and score[0] == 123.0)          # a refusal writes nothing
    return rc, lib.rvb_last_error().decode()


def test_bad_alignment_requests_are_refused_by_name_before_any_device_work(lib):
    """These hold with and without a GPU: the checks come before the first device call."""
    lp, y, _ = R.make_case(1, 20, 8, 5, "random")
    rc, msg = _hook(lib, lp, y, L=0);      assert rc == -1 and "empty transcript" in msg
    rc, msg = _hook(lib, lp, np.array([1, 8, 2], np.int32));  assert rc == -1 and "token id 8 outside [0, 8)" in msg
    rc, msg = _hook(lib, lp, np.array([1, -1, 2], np.int32)); assert rc == -1 and "outside" in msg
    rc, msg = _hook(lib, lp, np.array([1, 0, 2], np.int32));  assert rc == -1 and "blank" in msg
    rc, msg = _hook(lib, lp[:5], np.array([1, 1, 2, 3, 4], np.int32)); assert rc == -1 and "infeasible" in msg and "6 frames" in msg
    rc, msg = _hook(lib, lp, y, blank=8);  assert rc == -1 and "blank" in msg
    rc, msg = _hook(lib, lp, y, slab=0);   assert rc == -1
    big = np.ones(16384, np.int32)
    rc, msg = _hook(lib, lp, big);         assert rc == -5 and "16383 tokens" in msg
    rc, msg = _hook(lib, lp, y, T=(1 << 20) + 1); assert rc == -5 and "1048576 frames" in msg
    assert lib.rvb_test_ctc_viterbi(None, 4, 4, None, 1, 0, 1, None, None) == -1
    mt, mf = ctypes.c_int32(0), ctypes.c_int32(0)
    product = _lib.load()
    assert product.rvb_ctc_align_limits(ctypes.byref(mt), ctypes.byref(mf)) == 0 and (mt.value, mf.value) == (16383, 1 << 20)
    one = np.ones(1, np.int32)
    assert product.rvb_ctc_align(None, _lib.iptr(one), _lib.iptr(one), 1, _lib.iptr(one), _lib.iptr(one), None, None, None, None, None,
                                 None) == -1
    assert b"null engine" in product.rvb_last_error()


def test_cli_and_wenet_reexport_parse():
    from reverb_amd.bin import align_wav
    from wenet.bin import align_wav as w
    assert w.main is align_wav.main
    a = align_wav.get_args(["--model", "m", "--audio_file", "a.wav", "--transcript_file", "t.txt", "--result_dir", "o", "--format", "json"])
    assert (a.format, a.chunk_size, a.verbatimicity) == ("json", 2051, 1.0)


def test_text_is_segmented_against_the_unit_table_when_no_sentencepiece_model_exists():
    """The synthetic model directories carry tk.units.txt only: ReverbASR.align(transcript=...) still needs text -> ids."""
    from reverb_amd import synth
    from reverb_amd.tokenizer import RevBpeTokenizer
    units = synth.make_units(48)
    tk = RevBpeTokenizer("/no/such/tk.model", {u: i for i, u in enumerate(units)})
    ids = [int(x) for x in np.random.default_rng(0).integers(2, 47, 300)]
    text = tk.detokenize(ids)[0]
    pieces, back = tk.tokenize(text)
    assert tk.tokens2text(pieces) == text and all(0 < i < 47 for i in back)
    assert tk.tokenize("zzzz <tag5>") == (["<unk>", "<tag5>"], [1, 5])
    assert tk.tokenize("") == ([], [])
