"""TEST INFRASTRUCTURE ONLY.  Writes tests/golden/diar_bf16_yardstick.json (+ .npz): what bf16 STORAGE costs the segmentation
network, measured with oracle/diar_bf16_ref.py (fp64 arithmetic, rounded to bf16 where the bf16 engine stores bf16) against the
fp32 oracle (oracle/diar_ref.py), on the synthetic weights and recordings of tests/test_diar_gpu.py.  CPU only:

    python oracle/gen_golden_diar_bf16.py

Per case -- 14.3 s / 6 windows with weights seed 0 and seed 1, 52.3 s / 44 windows with weights seed 0 -- the six metrics of
diar_bf16_ref.metrics for the plain run and for JITTERS runs in which every value is multiplied by 1 +- 2^-20 before it is rounded
(the size of an fp32 summation-order difference); "yardstick" is the maximum over those runs.  The .npz holds uint8 argmax
arrays only (the oracle's and the plain run's), no log-probabilities.  tests/test_diar_bf16_gpu.py holds the engine to
1.25 x yardstick (+ 4 frames on the counts).

Expectation, from scratch measurements made before this script existed (same oracle, same recordings, weights seed 0):

    case        frames   argmax differs   of which margin > 0.1   mean |dp|   SincNet tap, mean rel.
    6 windows    3 534        27                   4              0.00285       0.0096
    44 windows  25 916       313                  92              0.00300       0.0104
    jittered: 6 windows 27-40 differing frames, 4-6 confident, mean |dp| 0.00285-0.00290; 44 windows 305-318, 86-92 confident.

This script gives 28 / 5 for the plain 6-window run (313 / 92 at 44 windows, as above) and, over its six jitter seeds, 28-37 / 5-11
at 6 windows and 299-331 / 91-98 at 44 (mean |dp| 0.00284-0.00295 / 0.00300-0.00303).  The scratch restatement and this one are two
codes: a value that sits next to a tie falls one way or the other with the order of an fp64 sum, which is the effect the jitter
runs sample, and other seeds draw other signs.  The margin is taken between the oracle's top two LOG-probabilities (that
reading reproduces the 92 above).  Weights seed 1 loses more (64-76 / 18-22, mean |dp| 0.0046): a yardstick holds per model.
The file is what the committed restatement gives.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch                                        # noqa: E402
from oracle import diar_ref as R                    # noqa: E402
from oracle import diar_bf16_ref as B               # noqa: E402
from reverb_amd import synth_diar as SD             # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = {   # name: (seconds, recording seed, weights seed) -- the recordings of tests/test_diar_gpu.py
    "w6_seed0": (14.3, 11, 0),
    "w44_seed0": (52.3, 23, 0),
    "w6_seed1": (14.3, 11, 1),
}
JITTERS = 6


def windows_of(pcm, cfg):
    """pyannote's Inference.slide: the full windows plus one zero-padded tail (as tests/test_diar_gpu.py)"""
    wav = torch.from_numpy(pcm.astype(np.float32) / 32768.0)
    n, win, step = wav.shape[0], cfg["window_samples"], cfg["step_samples"]
    full = (n - win) // step + 1 if n >= win else 0
    W = full + (1 if (n < win or (n - win) % step > 0) else 0)
    x = torch.zeros(W, 1, win)
    for w in range(W):
        seg = wav[w * step:w * step + win]
        x[w, 0, :seg.shape[0]] = seg
    return x


def oracle_run(sd, x):
    """the fp32 oracle on one thread (a fixed summation order) -> (logp, sincnet tap, lstm tap) numpy"""
    taps = {}
    nt = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        with torch.no_grad():
            logp = R.pyannet(R.to_torch_sd(sd), x, taps)
    finally:
        torch.set_num_threads(nt)
    return logp.numpy(), taps["sincnet"].numpy(), taps["lstm"].numpy()


def make_case(name):
    seconds, pcm_seed, w_seed = CASES[name]
    cfg = SD.make_diar_config()
    sd = SD.make_segmentation_sd(cfg, w_seed)
    pcm = SD.synth_conversation(seconds, seed=pcm_seed)
    x = windows_of(pcm, cfg)
    logp, sinc, lstm = oracle_run(sd, x)
    return dict(cfg=cfg, sd=sd, pcm=pcm, x=x, logp=logp, sinc=sinc, lstm=lstm)


def restatement_metrics(case, storage="bf16", jitter_seed=None, hook=None, craw=None, out=None):
    taps = {}
    lp = B.pyannet_bf16(case["sd"], case["x"], taps, storage=storage, jitter_seed=jitter_seed, hook=hook, craw=craw)
    if out is not None:
        out["logp"] = lp
    return B.metrics(lp, taps["sincnet"], case["logp"], case["sinc"])


def raw_sinc(case):
    filt, _ = B.sinc_filter_bank(case["sd"])
    return np.stack([B.sinc_raw(filt, case["x"][w, 0].numpy()) for w in range(case["x"].shape[0])])


def main():
    doc, arrays = {"margin": B.MARGIN, "jitter": B.JITTER, "cases": {}}, {}
    for name, (seconds, pcm_seed, w_seed) in CASES.items():
        case = make_case(name)
        craw = raw_sinc(case)
        runs, out = {}, {}
        runs["plain"] = restatement_metrics(case, craw=craw, out=out)
        for j in range(1, JITTERS + 1):
            runs["jitter%d" % j] = restatement_metrics(case, jitter_seed=j, craw=craw)
        yard = {k: max(r[k] for r in runs.values()) for k in B.COUNTS + B.MEANS}
        plain = runs["plain"]
        doc["cases"][name] = dict(seconds=seconds, pcm_seed=pcm_seed, weights_seed=w_seed, windows=int(case["x"].shape[0]),
                                  frames=plain["frames"], confident=plain["confident"], runs=runs, yardstick=yard)
        arrays[name + "_oracle_argmax"] = case["logp"].argmax(-1).astype(np.uint8)
        arrays[name + "_plain_argmax"] = out["logp"].argmax(-1).astype(np.uint8)
        print(name, json.dumps(yard), flush=True)
    with open(os.path.join(GOLDEN, "diar_bf16_yardstick.json"), "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    np.savez_compressed(os.path.join(GOLDEN, "diar_bf16_yardstick.npz"), **arrays)


if __name__ == "__main__":
    main()
