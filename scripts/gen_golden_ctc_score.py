"""Writes tests/golden/ctc_score.json: the CTC loss the UNMODIFIED reference's CTC.forward (asr/wenet/transformer/ctc.py:65-104:
torch.nn.CTCLoss(blank=blank_id, reduction='sum') over log_softmax(ctc_lo(hs))) returns on the seeded logits of
tests/ctc_score_ref.make_logits, in float64, with ctc_lo set to the identity so that hs ARE the logits.  With a batch of one the loss
is -loglik.  Only (seed, T, V, L, scale, repeats_at) and the loss are stored.

    python scripts/gen_golden_ctc_score.py

The reference is imported through oracle/ref_shim.py."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import ctc_score_ref as R  # noqa: E402

# (seed, T, V, L, scale, repeats_at)
CASES = [(1, 1, 8, 1, 1.0, []), (2, 3, 4, 2, 1.0, [1]), (3, 64, 16, 5, 1.0, []), (4, 200, 32, 40, 1.0, [1, 20]),
         (5, 512, 48, 100, 3.0, [2, 3]), (6, 60, 6, 40, 1.0, [7, 30]), (7, 512, 32, 250, 6.0, [1]), (8, 4096, 32, 300, 6.0, [150]),
         (9, 4096, 64, 1200, 3.0, [2])]


def main():
    from oracle import ref_shim
    ref_shim.install()
    from wenet.transformer.ctc import CTC
    out = []
    for seed, T, V, L, scale, rep in CASES:
        logits, y = R.make_logits(seed, T, V, L, scale, rep)
        ctc = CTC(V, V, blank_id=0).double()
        with torch.no_grad():
            ctc.ctc_lo.weight.copy_(torch.eye(V, dtype=torch.float64))
            ctc.ctc_lo.bias.zero_()
            loss, _ = ctc(torch.from_numpy(logits).double()[None], torch.tensor([T]), torch.from_numpy(y.astype(np.int64))[None],
                          torch.tensor([L]))
        assert np.isfinite(float(loss)) and float(loss) > 0
        out.append({"seed": seed, "T": T, "V": V, "L": L, "scale": scale, "repeats_at": rep, "loss": repr(float(loss))})
        print(seed, T, V, L, scale, float(loss))
    with open(os.path.join(ROOT, "tests", "golden", "ctc_score.json"), "w") as f:
        json.dump({"blank": 0, "cases": out}, f, indent=0)


if __name__ == "__main__":
    main()
