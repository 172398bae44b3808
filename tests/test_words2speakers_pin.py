"""The word -> speaker join pinned to the reference FUNCTION (VERDICT r4 "missing" #3).

`tests/golden/words2speakers.json` holds what the unmodified reference `diarization/assign_words2speakers.py:24-61`
returned (through `oracle/intervaltree_shim.py`, a stand-in for the two intervaltree methods it calls) on 2 372 seeded
(word, turn set) pairs covering its three branches; the product's per-word function and its vectorised form must give
the same speaker.  Where the reference's own answer depends on set iteration order -- several speakers with EXACTLY the
same overlap or several turns at EXACTLY the same distance -- any of the tied answers is accepted and the product's
documented rule (the earliest turn) is what it must return; such pairs are counted, not skipped.
`tests/golden/words2speakers_live.json` (`python -m oracle.gen_golden_words2speakers --live`) holds what the reference
returned on the real intervaltree 3.1.0 beyond those pairs: 22 further seeded cases, the golden pairs again, digests of
the real tree's overlap sets and distances, and the STM the reference file wrote as a script.
"""
import json
import os
import random
from collections import defaultdict

import pytest

from reverb_amd.bin import assign_words2speakers as A

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "words2speakers.json")
LIVE = os.path.join(os.path.dirname(__file__), "golden", "words2speakers_live.json")


def _turn_list(turns):
    return sorted({(s, e, lab) for s, e, lab in turns})


def _tied_answers(start, dur, turns):
    """Every answer the reference can give, by brute force over the same float expressions."""
    end = start + dur
    hits = [t for t in turns if start < end and t[0] < end and t[1] > start]
    if len(hits) == 1:
        return {hits[0][2]}
    if not hits:
        if not turns:
            return {""}
        dist = [0 if (t[0] < end and t[1] > start) else (t[0] - end if start < t[0] else start - t[1]) for t in turns]
        m = min(dist)
        return {t[2] for t, d in zip(turns, dist) if d == m}
    tot = defaultdict(float)
    for s, e, lab in hits:
        tot[lab] += min(end, e) - max(start, s)
    m = max(tot.values())
    return {lab for lab, v in tot.items() if abs(v - m) <= 1e-12 * max(1.0, abs(m))}     # the sum order is the set's


def _check(turns, words, speakers):
    turns = _turn_list(turns)
    vec = A.speakers_for_words([w[0] for w in words], [w[1] for w in words], turns)
    ties = 0
    for (s, d), want, got_v in zip(words, speakers, vec):
        got = A.speaker_for_segment(s, d, turns)
        ok = _tied_answers(s, d, turns)
        assert want in ok, (s, d, want, ok)            # the brute force agrees with the reference
        if len(ok) == 1:
            assert got == want and got_v == want, (s, d, got, got_v, want)
        else:
            ties += 1
            assert got in ok and got_v == got, (s, d, got, got_v, ok)
    return ties


def test_join_matches_the_reference_function_on_the_golden_pairs():
    doc = json.load(open(GOLDEN))
    assert doc["pairs"] >= 1000 and min(doc["branches"].values()) >= 50, doc["branches"]
    ties = sum(_check(c["turns"], c["words"], c["speakers"]) for c in doc["cases"])
    # exact ties are common in overlapped speech (a word lying inside two speakers' turns gives both the word's whole
    # duration): 358 of the 2 372 pairs; the other 2 014 have one possible answer and must match it
    assert doc["pairs"] - ties >= 1000, ties


def test_join_matches_the_reference_function_live():
    """The reference function's answers, recorded with the real intervaltree 3.1.0, on 22 further seeded cases (Random(7),
    cases 3 .. 24 of the generator)."""
    from oracle.gen_golden_words2speakers import make_case, speaker_code
    fresh = json.load(open(LIVE))["fresh_speakers"]
    assert len(fresh) == 22
    rng = random.Random(7)
    for idx, codes in zip(range(3, 25), fresh):
        c = make_case(rng, idx)
        labels = {speaker_code(lab): lab for _, _, lab in c["turns"]}
        labels[-1] = ""
        _check(c["turns"], c["words"], [labels[k] for k in codes])


def test_golden_pairs_hold_under_the_real_intervaltree_package():
    """The golden speakers were generated through the stand-in; the unmodified reference function was run again over the
    SAME golden pairs on the real `IntervalTree` (words2speakers_live.json: the pairs where it answered differently): every
    answer must be one of the tied-possible answers, and equal to the golden one wherever only one answer is possible.  Also:
    the stand-in answers random overlap / distance queries exactly as the real tree did (digests of its answers), so the
    stand-in is a faithful scan of the same intervals."""
    from oracle import intervaltree_shim as shim
    from oracle.gen_golden_words2speakers import make_tree_queries, tree_digest
    doc = json.load(open(GOLDEN))
    live = json.load(open(LIVE))
    real = {(i, j): got for i, j, got in live["real_tree_differs"]}
    checked = 0
    for i, c in enumerate(doc["cases"]):
        turns = _turn_list(c["turns"])
        for j, ((s, d), want) in enumerate(zip(c["words"], c["speakers"])):
            got = real.get((i, j), want)
            ok = _tied_answers(s, d, turns)
            assert got in ok and (len(ok) > 1 or got == want), (s, d, got, want, ok)
            checked += 1
    assert checked == doc["pairs"]
    assert len(live["tree_digests"]) == 50
    rng = random.Random(3)
    for k, want in enumerate(live["tree_digests"]):
        assert tree_digest(shim.IntervalTree, shim.Interval, *make_tree_queries(rng)) == want, k


def test_script_writes_the_stm_the_reference_script_writes(tmp_path):
    """The reference file run as `__main__`, unmodified (its CTM reader, its tree construction from the annotation, its STM
    line format), wrote the STM recorded in words2speakers_live.json for the seeded RTTM + CTM of make_script_inputs; the
    product's `main` must write the same file.  pyannote's `load_rttm` was stood in for by the product's own reader -- that
    part is shared, not pinned; turn sets without exact ties so both must agree line by line."""
    from oracle.gen_golden_words2speakers import make_script_inputs
    rttm, ctm = make_script_inputs(random.Random(11))
    (tmp_path / "a.rttm").write_text(rttm)
    (tmp_path / "a.ctm").write_text(ctm)
    A.main([str(tmp_path / "a.rttm"), str(tmp_path / "a.ctm"), str(tmp_path / "got.stm")])
    want, got = json.load(open(LIVE))["stm"], (tmp_path / "got.stm").read_text()
    assert len(want.splitlines()) == len(ctm.splitlines()) > 100
    assert got == want


def test_shim_refuses_null_intervals_like_the_package():
    from oracle import intervaltree_shim as shim
    with pytest.raises(ValueError, match="Null Interval"):
        shim.IntervalTree([shim.Interval(1.0, 1.0, "A")])
    t = shim.IntervalTree([shim.Interval(0.0, 1.0, "A"), shim.Interval(0.0, 1.0, "A"), shim.Interval(1.0, 2.0, "B")])
    assert len(t) == 2 and {iv.data for iv in t[0.5:1.0]} == {"A"} and t[1.0:1.0] == set()
    assert shim.Interval(0.0, 1.0).distance_to(shim.Interval(1.0, 2.0)) == 0.0       # touching: gap of zero, not "overlap"
    assert shim.Interval(3.0, 4.0).distance_to(shim.Interval(1.0, 2.0)) == 1.0
