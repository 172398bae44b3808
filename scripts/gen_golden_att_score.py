"""Writes tests/golden/att_score.json: what the UNMODIFIED reference's LabelSmoothingLoss (asr/wenet/transformer/
label_smoothing_loss.py:68-96) and th_accuracy (asr/wenet/utils/common.py:268-287) return, in float64, on the seeded logits of
tests/att_score_ref.make_case.  Only (seed, lens, V, scale, tie, smoothing, normalize_length) and the expected loss and accuracy are
stored.

    python scripts/gen_golden_att_score.py

The reference is imported through oracle/ref_shim.py."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import att_score_ref as R  # noqa: E402

# (seed, lens, V, scale, tie): a batch of one, a padded batch of 2 (ignore_id rows), a tie for the arg-max
SHAPES = [(1, [7], 5, 2.0, False), (2, [12], 48, 2.0, False), (3, [9, 4], 5, 2.0, False), (4, [6, 11], 48, 2.0, False),
          (5, [5], 5, 2.0, True), (6, [8, 3], 48, 2.0, True)]


def main():
    from oracle import ref_shim
    ref_shim.install()
    from wenet.transformer.label_smoothing_loss import LabelSmoothingLoss
    from wenet.utils.common import th_accuracy
    out = []
    for seed, lens, V, scale, tie in SHAPES:
        x, t = R.make_case(seed, lens, V, scale, tie)
        xt, tt = torch.from_numpy(x).double(), torch.from_numpy(t)
        acc = float(th_accuracy(xt.view(-1, V), tt, ignore_label=R.IGNORE_ID))
        for smoothing in (0.0, 0.1):
            for norm in (False, True):
                crit = LabelSmoothingLoss(size=V, padding_idx=R.IGNORE_ID, smoothing=smoothing, normalize_length=norm)
                loss = float(crit(xt, tt))
                out.append({"seed": seed, "lens": lens, "V": V, "scale": scale, "tie": tie, "smoothing": smoothing,
                            "normalize_length": norm, "loss": repr(loss), "accuracy": repr(acc)})
                print(seed, lens, V, tie, smoothing, norm, loss, acc)
    with open(os.path.join(ROOT, "tests", "golden", "att_score.json"), "w") as f:
        json.dump({"ignore_id": R.IGNORE_ID, "cases": out}, f, indent=0)


if __name__ == "__main__":
    main()
