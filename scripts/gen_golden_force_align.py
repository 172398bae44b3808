"""Writes tests/golden/force_align.json: the labels the UNMODIFIED reference's force_align (asr/wenet/utils/ctc_utils.py:105-161)
returns on the seeded inputs of tests/force_align_ref.make_case.  Only (seed, T, V, L, kind) and the labels are stored.

    python scripts/gen_golden_force_align.py /path/to/reference

The reference module is loaded by file path (it imports numpy and torch only; as `wenet.utils...` it would collide with this
repository's wenet/ package).  Its loop reads log_alpha[t-1, s-1] for s = 0, which Python resolves to the LAST state: once the whole
transcript can have been emitted, state 0 may be re-entered from there and the result emits the transcript twice -- one more input
class with undefined output.  Where the returned path is a valid one (it collapses to the transcript) it is also the optimum of the
recurrence without that wrap, first-maximum ties included (every value on it is attained by a wrap-free path, and the wrap only
raises other candidates); the generator asserts this for every case instead of filtering cases."""
import importlib.util
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import force_align_ref as R  # noqa: E402

# (seed, T, V, L, kind); T of the min_t kinds is computed
CASES = [(1, 64, 16, 5, "random"), (2, 200, 32, 40, "random"), (3, 512, 48, 100, "random"),
         (4, 64, 8, 10, "quant"), (5, 300, 16, 60, "quant"), (6, 512, 12, 100, "quant"),
         (7, 80, 6, 20, "repeat"), (8, 256, 5, 50, "repeat"),
         (9, 100, 16, 20, "neginf"), (10, 256, 24, 40, "neginf"),
         (11, 0, 16, 30, "min_t"), (15, 0, 4, 25, "min_t_quant"),
         (12, 50, 8, 1, "random"), (13, 30, 8, 1, "quant"), (14, 1, 8, 1, "random"), (16, 3, 4, 2, "quant")]


def main(ref_root):
    path = os.path.join(ref_root, "asr", "wenet", "utils", "ctc_utils.py")
    spec = importlib.util.spec_from_file_location("ref_ctc_utils", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = []
    for seed, T, V, L, kind in CASES:
        lp, y, T = R.make_case(seed, T, V, L, kind)
        labels = [int(x) for x in mod.force_align(torch.from_numpy(lp), torch.from_numpy(y.astype(np.int64)), 0)]
        assert list(R.collapse(labels)) == list(y), (seed, kind, "the reference's path wrapped from the last state into state 0")
        out.append({"seed": seed, "T": T, "V": V, "L": L, "kind": kind, "labels": labels})
        print(seed, kind, T, V, L, "ok")
    with open(os.path.join(ROOT, "tests", "golden", "force_align.json"), "w") as f:
        json.dump({"blank": 0, "cases": out}, f, separators=(",", ":"))


if __name__ == "__main__":
    main(sys.argv[1])
