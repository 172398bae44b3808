"""Writes tests/golden/context_bias.json: what the UNMODIFIED reference's ContextGraph (asr/wenet/utils/context_graph.py) and
ctc_prefix_beam_search (asr/wenet/transformer/search.py:124-248) return on the seeded inputs of tests/context_bias_ref.py.  Only
seeds, shapes, phrase lists and results are stored; the lattices are regenerated from their seeds (a digest pins their bits).

    python scripts/gen_golden_context_bias.py /path/to/reference

Runs on the CPU.  The reference's modules are imported through oracle/ref_shim.py (its `wenet` package shadows this repository's
compatibility package of the same name for the length of the run).

The fixture must not go vacuous: at context_score 6.0, at least half of the searches with beam >= 3 must have a biased 1-best that
differs from the unbiased one.  This is asserted on the reference's results alone; if it fails, change the inputs."""
import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import context_bias_ref as R  # noqa: E402

# graph walks: (phrase set, context_score, stream seed, steps, vocabulary of the stream)
WALKS = [("mixed", 3.0, 1, 32, 6), ("mixed", 0.1, 2, 12, 6), ("nested", 6.0, 3, 20, 3), ("chain", 2.5, 4, 20, 5), ("chain", 0.0, 5, 5, 5)]
# lattices: name -> (seed, T, V, kind); searches: (lattice, beam, context_score).  Phrases: tests/context_bias_ref.phrases_from the
# reference's unbiased n-best at beam 10 of the same lattice.
LATTICES = {"a": (11, 9, 12, "random"), "b": (12, 14, 12, "random"), "c": (13, 7, 11, "random"), "one": (14, 1, 12, "random"),
            "blank": (15, 6, 12, "blank")}
SEARCHES = [("a", 1, 6.0), ("a", 3, 0.0), ("a", 3, 3.0), ("a", 3, 6.0), ("b", 3, 6.0), ("c", 3, 6.0), ("c", 10, 6.0), ("c", 10, 0.0),
            ("one", 3, 6.0), ("blank", 3, 6.0), ("blank", 1, 3.0)]
TOKENIZE_TABLE = {"<blank>": 0, "<unk>": 1, "▁": 2, "a": 3, "b": 4, "c": 5, "d": 6}
TOKENIZE_LINES = ["ab c", "", "  dab  ", "axb", "c"]


def main(ref_root):
    os.environ["REVERB_REFERENCE_ASR"] = os.path.join(ref_root, "asr")
    from oracle import ref_shim
    ref_shim.install()
    from wenet.transformer.search import ctc_prefix_beam_search
    from wenet.utils import context_graph as CG

    def graph_of(phrases, score):
        g = CG.ContextGraph.__new__(CG.ContextGraph)          # the constructor minus the list file
        g.context_score, g.context_list, g.num_nodes = score, phrases, 0
        g.root = CG.ContextState(id=0, token=-1, token_score=0, node_score=0, output_score=0, is_end=False)
        g.root.fail = g.root
        g.build_graph(phrases)
        return g

    walks = []
    for name, score, seed, n, V in WALKS:
        g = graph_of(R.WALK_SETS[name], score)
        state, steps = g.root, []
        for tok in R.stream(seed, n, V):
            sc, state = g.forward_one_step(state, tok)
            steps.append([sc, state.id, g.finalize(state)[0]])
        walks.append({"set": name, "c": score, "seed": seed, "n": n, "V": V, "nodes": g.num_nodes, "steps": steps})

    def run(lp, beam, graph):
        r = ctc_prefix_beam_search(torch.from_numpy(lp).unsqueeze(0), torch.tensor([lp.shape[0]]), beam, graph, 0)[0]
        return {"nbest": [list(x) for x in r.nbest], "scores": [float(s) for s in r.nbest_scores], "times": [list(t) for t in r.nbest_times]}

    lattices, plain = {}, {}
    for name, (seed, T, V, kind) in LATTICES.items():
        lp = R.make_lattice(seed, T, V, kind)
        top = run(lp, min(10, V), None)
        lattices[name] = {"seed": seed, "T": T, "V": V, "kind": kind, "digest": R.digest(lp),
                          "phrases": R.phrases_from(top["nbest"]) or [[1, 2], [3]]}
    searches, changed, eligible = [], 0, 0
    for name, beam, score in SEARCHES:
        seed, T, V, kind = LATTICES[name]
        lp = R.make_lattice(seed, T, V, kind)
        if (name, beam) not in plain:
            plain[(name, beam)] = run(lp, beam, None)
        biased = run(lp, beam, graph_of(lattices[name]["phrases"], score))
        if score == 6.0 and beam >= 3:
            eligible += 1
            changed += biased["nbest"][0] != plain[(name, beam)]["nbest"][0]
        searches.append({"lat": name, "beam": beam, "c": score, "biased": biased})
        print(name, beam, score, plain[(name, beam)]["nbest"][0], "->", biased["nbest"][0])
    assert eligible >= 4 and 2 * changed >= eligible, (changed, eligible)

    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "list.txt")
        with open(path, "w", encoding="utf8") as f:
            f.write("\n".join(TOKENIZE_LINES) + "\n")
        with_unk = CG.tokenize(path, TOKENIZE_TABLE)
        without = CG.tokenize(path, {k: v for k, v in TOKENIZE_TABLE.items() if k != "<unk>"})
    out = {"blank": 0, "walks": walks, "lattices": lattices,
           "plain": [{"lat": k[0], "beam": k[1], **v} for k, v in plain.items()], "searches": searches,
           "tokenize": {"table": TOKENIZE_TABLE, "lines": TOKENIZE_LINES, "ids": with_unk, "ids_no_unk": without}}
    dst = os.path.join(ROOT, "tests", "golden", "context_bias.json")
    with open(dst, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print(os.path.getsize(dst), "bytes; 1-best changed in", changed, "of", eligible)


if __name__ == "__main__":
    main(sys.argv[1])
