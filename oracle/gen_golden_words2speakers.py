"""TEST INFRASTRUCTURE ONLY.  Golden vectors for the word -> speaker join (BASELINE config 5).

Runs the UNMODIFIED `/root/reference/diarization/assign_words2speakers.py:24-61` (`speaker_for_segment`) through
`oracle/intervaltree_shim.py` on seeded random (word, turn set) pairs and writes
`tests/golden/words2speakers.json`: the turn sets, the words and the speaker the reference returned for each.

    python -m oracle.gen_golden_words2speakers

Turn sets: 0 .. 60 turns of 2 .. 6 speakers, some with heavy overlap, some sparse (gaps of seconds), times either
free floats or rounded to the millisecond grid an RTTM file carries (`{start:.3f} {dur:.3f}`), where exact ties in
overlap / distance do occur.  Words: CTM-like (start on a 10 ms grid or free, duration 0 .. 1.2 s, incl. zero-length
words and words outside every turn).  Every branch of the function is counted in the file's header.
"""
import hashlib
import json
import os
import random

from oracle import intervaltree_shim as shim

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "words2speakers.json")
OUT_LIVE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "words2speakers_live.json")


def make_case(rng, idx):
    grid = idx % 2 == 1                          # odd cases live on the RTTM / CTM grids
    n_turns = [0, 1, 2][idx] if idx < 3 else rng.randint(3, 60)
    n_spk = rng.randint(2, 6)
    dense = rng.random() < 0.5
    t, turns = 0.0, []
    for _ in range(n_turns):
        t += rng.uniform(-2.0, 0.5) if dense else rng.uniform(-0.5, 4.0)
        t = max(t, 0.0)
        dur = rng.uniform(0.05, 6.0)
        s, e = (round(t, 3), round(t + dur, 3)) if grid else (t, t + dur)
        if not s < e:
            e = s + 0.001
        turns.append([s, e, "SPEAKER_%02d" % rng.randrange(n_spk)])
        t += dur * rng.uniform(0.2, 1.0)
    if n_turns > 4:
        turns.append(list(turns[2]))             # an exact duplicate collapses in the tree's set
        turns.append([turns[3][0], turns[3][1], "SPEAKER_%02d" % ((int(turns[3][2][-2:]) + 1) % n_spk)])   # same span, other speaker
    horizon = max([e for _, e, _ in turns], default=10.0) + 5.0
    words = []
    for _ in range(50):
        s = rng.uniform(-1.0, horizon)
        d = rng.choice([0.0, 0.01, 0.05]) if rng.random() < 0.1 else rng.uniform(0.0, 1.2)
        if grid:
            s, d = round(s, 2), round(d, 2)
        words.append([s, d])
    if turns:                                     # words pinned to turn boundaries (half-open interval semantics)
        a = turns[rng.randrange(len(turns))]
        words += [[a[1], 0.3], [a[0] - 0.3, 0.3], [a[0], 0.0], [a[0], a[1] - a[0]]]
    return {"grid": grid, "turns": turns, "words": words}


def main():
    ref = shim.load_reference_module()
    rng = random.Random(20240926)
    cases, branch = [], {"one": 0, "none": 0, "many": 0, "no_turns": 0}
    for idx in range(44):
        c = make_case(rng, idx)
        tree = shim.IntervalTree(shim.Interval(s, e, lab) for s, e, lab in c["turns"])
        c["speakers"] = []
        for s, d in c["words"]:
            k = len(tree[s:s + d])
            branch["no_turns" if not c["turns"] else "one" if k == 1 else "none" if k == 0 else "many"] += 1
            c["speakers"].append(ref.speaker_for_segment(s, d, tree))
        cases.append(c)
    doc = {"made_by": "oracle/gen_golden_words2speakers.py",
           "reference": "diarization/assign_words2speakers.py:24-61 (unmodified) through oracle/intervaltree_shim.py",
           "pairs": sum(len(c["words"]) for c in cases), "branches": branch, "cases": cases}
    with open(OUT, "w") as f:
        json.dump(doc, f)
    print("wrote", os.path.normpath(OUT), doc["pairs"], "pairs", branch)


def make_script_inputs(rng):
    """RTTM + CTM text of one recording for the script-level pin: 40 turns of 4 speakers without exact ties, > 100 words."""
    t, rttm, ctm = 0.0, [], []
    for i in range(40):
        t += rng.uniform(0.1, 3.0)
        d = rng.uniform(0.3, 5.0)
        rttm.append(f"SPEAKER rec1 1 {t:.3f} {d:.3f} <NA> <NA> SPEAKER_{rng.randrange(4):02d} <NA> <NA>")
        t += d * rng.uniform(0.5, 1.0)
    w = 0.0
    while w < t + 3.0:
        d = round(rng.uniform(0.013, 0.7), 2)
        ctm.append(f"rec1.wav 0 {w:.2f} {d:.2f} w{len(ctm)} {rng.random():.2f}")
        w += d + rng.choice([0.0, 0.0, 0.137, 1.731])
    return "\n".join(rttm) + "\n", "\n".join(ctm) + "\n"


def make_tree_queries(rng):
    """One random interval set (1 .. 29 intervals of labels A-D) and 40 queries (a, b) on it."""
    ivs = []
    for _ in range(rng.randrange(1, 30)):
        a = round(rng.uniform(0, 50), 2)
        ivs.append((a, a + round(rng.uniform(0.01, 8), 2), rng.choice("ABCD")))
    queries = []
    for _ in range(40):
        a = round(rng.uniform(-1, 60), 2)
        queries.append((a, a + rng.choice([0.0, 0.01, 1.0, 7.5])))
    return ivs, queries


def tree_digest(IntervalTree, Interval, ivs, queries):
    """SHA-256 (16 hex digits) of what a tree class answers for `queries`: its size, then per query the overlap set (as indices
    into `ivs`) and every interval's distance_to(a, b + 0.01)."""
    tree = IntervalTree(Interval(*iv) for iv in ivs)
    out = [len(tree)]
    for a, b in queries:
        hit = {tuple(iv) for iv in tree[a:b]}
        out.append([[i for i, iv in enumerate(ivs) if iv in hit],
                    [Interval(*iv).distance_to(Interval(a, b + 0.01)) for iv in ivs]])
    return hashlib.sha256(json.dumps(out).encode()).hexdigest()[:16]


def speaker_code(label):
    """"SPEAKER_03" -> 3, "" (no turns at all) -> -1."""
    return int(label[-2:]) if label else -1


def main_live():
    """tests/golden/words2speakers_live.json: what the unmodified reference returned beyond the golden pairs above, so that
    the pin runs without the reference checkout or the intervaltree package.  The inputs are regenerated from their seeds by
    the test; only the answers are stored:
      fresh_speakers    the reference's speakers (speaker_code) on make_case(Random(7), 3 .. 24)
      real_tree_differs [case, word, speaker] where the reference on the REAL intervaltree 3.1.0 answers a pair of
                        words2speakers.json differently from the stand-in (exact ties); every other pair: the same answer
      tree_digests      tree_digest of the real IntervalTree on 50 make_tree_queries(Random(3)) sets
      stm               what the reference file, run as `__main__`, wrote for make_script_inputs(Random(11))"""
    import tempfile

    from reverb_amd.diarization import load_rttm
    real = shim.real_intervaltree()
    if real is None:
        raise SystemExit("needs intervaltree==3.1.0 (oracle/intervaltree_shim.py: REVERB_REAL_INTERVALTREE)")
    ref = shim.load_reference_module()             # on the real package's classes
    rng = random.Random(7)
    fresh = []
    for idx in range(3, 25):
        c = make_case(rng, idx)
        tree = real.IntervalTree(real.Interval(s, e, lab) for s, e, lab in c["turns"])
        fresh.append([speaker_code(ref.speaker_for_segment(s, d, tree)) for s, d in c["words"]])

    with open(OUT) as f:
        golden = json.load(f)
    differs = []
    for i, c in enumerate(golden["cases"]):
        tree = real.IntervalTree(real.Interval(s, e, lab) for s, e, lab in sorted({tuple(t) for t in c["turns"]}))
        for j, ((s, d), want) in enumerate(zip(c["words"], c["speakers"])):
            got = ref.speaker_for_segment(s, d, tree)
            if got != want:
                differs.append([i, j, got])
    rng = random.Random(3)
    digests = [tree_digest(real.IntervalTree, real.Interval, *make_tree_queries(rng)) for _ in range(50)]

    with tempfile.TemporaryDirectory() as d:
        paths = [os.path.join(d, n) for n in ("a.rttm", "a.ctm", "ref.stm")]
        for path, text in zip(paths, make_script_inputs(random.Random(11))):
            open(path, "w").write(text)
        shim.run_reference_script(*paths, load_rttm)
        stm = open(paths[2]).read()

    doc = {"made_by": "oracle/gen_golden_words2speakers.py --live",
           "reference": "diarization/assign_words2speakers.py (unmodified) on " + shim.tree_classes()[2],
           "fresh_speakers": fresh, "real_tree_differs": differs, "tree_digests": digests, "stm": stm}
    with open(OUT_LIVE, "w") as f:             # one line per key, one per fresh case
        f.write("{\n" + ",\n".join(json.dumps(k) + ": " + ("[\n" + ",\n".join(json.dumps(r) for r in v) + "]" if k == "fresh_speakers"
                                                          else json.dumps(v)) for k, v in doc.items()) + "\n}\n")
    print("wrote", os.path.normpath(OUT_LIVE), len(fresh), "fresh cases,", len(differs), "tied pairs answered differently,",
          len(digests), "trees,", len(stm.splitlines()), "STM lines")


if __name__ == "__main__":
    import sys
    main_live() if "--live" in sys.argv else main()
