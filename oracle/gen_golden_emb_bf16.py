"""TEST INFRASTRUCTURE ONLY.  Writes tests/golden/emb_bf16_yardstick.json: what bf16 STORAGE costs the speaker-embedding network,
measured with oracle/emb_bf16_ref.py (fp64 arithmetic, rounded to bf16 where the bf16 engine stores bf16) against the fp32 oracle
(oracle/diar_ref.py), on the synthetic weights, the recording and the items of tests/test_diar_gpu.py's emb_case: windows 0, 2 and
the zero-padded tail window of a 14.3 s recording, each with a contiguous, a scattered and a soft (window 2: an all-zero) mask.
CPU only:

    python oracle/gen_golden_emb_bf16.py

Per metric of emb_bf16_ref.metrics (over the items with a non-empty mask): the plain run and JITTERS runs in which every value is
multiplied by 1 +- 2^-20 before it is rounded (the size of an fp32 summation-order difference); "yardstick" is the maximum over
those runs, and "factor" = max(1.25, 1.06 x widest / median) of them -- 1.25 is what the segmentation test allows for the sample
spread six jitters do not show; the second term widens it only where this network's spread is wider.  tests/test_emb_bf16_gpu.py
holds the engine to factor x yardstick per metric.  The file is numbers only.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch                                        # noqa: E402
from oracle import diar_ref as R                    # noqa: E402
from oracle import emb_bf16_ref as E                # noqa: E402
from oracle.gen_golden_diar_bf16 import windows_of  # noqa: E402
from reverb_amd import synth_diar as SD             # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURE = os.path.join(GOLDEN, "emb_bf16_yardstick.json")
JITTERS = 6
SECONDS, PCM_SEED, WEIGHTS_SEED, MASK_SEED = 14.3, 11, 0, 5


def make_items(W):
    """the items of tests/test_diar_gpu.py's emb_case, drawn the same way from the same seed"""
    rng = np.random.default_rng(MASK_SEED)
    wins, masks = [], []
    for w in (0, 2, W - 1):                       # W - 1 is the zero-padded tail window
        for k in range(3):
            m = np.zeros(R.NUM_FRAMES, np.float32)
            if k == 0:
                m[rng.integers(0, 200):rng.integers(300, 589)] = 1.0
            elif k == 1:
                m[:] = (rng.random(R.NUM_FRAMES) < 0.4)
            elif w == 2:
                pass
            else:
                m[:] = rng.random(R.NUM_FRAMES).astype(np.float32)
            wins.append(w)
            masks.append(m)
    return np.array(wins, np.int64), np.stack(masks)


def make_case(pcm=None):
    """-> dict(cfg, seg_sd, emb_sd, pcm, x windows, wins, masks, active, feats {w: [998][80]}, want [n][256] and trunk {w: [10][125][256]}
    of the fp32 oracle on one thread (a fixed summation order))"""
    cfg = SD.make_diar_config()
    emb_sd = SD.make_embedding_sd(cfg, WEIGHTS_SEED)
    pcm = SD.synth_conversation(SECONDS, seed=PCM_SEED) if pcm is None else pcm
    x = windows_of(pcm, cfg)
    wins, masks = make_items(x.shape[0])
    sd = R.to_torch_sd(emb_sd)
    feats = {w: R.hamming_fbank(x[w, 0].numpy()) for w in sorted(set(wins.tolist()))}
    nt = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        with torch.no_grad():
            trunk = {w: R.resnet34_trunk(sd, torch.from_numpy(f)[None]) for w, f in feats.items()}
            want = torch.cat([F_linear_stats(sd, trunk[int(w)], torch.from_numpy(m)[None]) for w, m in zip(wins, masks)]).numpy()
    finally:
        torch.set_num_threads(nt)
    return dict(cfg=cfg, emb_sd=emb_sd, pcm=pcm, x=x, wins=wins, masks=masks, active=masks.sum(1) > 0, feats=feats, want=want,
                trunk={w: t[0].permute(1, 2, 0).numpy() for w, t in trunk.items()})


def F_linear_stats(sd, trunk, weights):
    return torch.nn.functional.linear(R.tstp(trunk, weights), sd["resnet.seg_1.weight"], sd["resnet.seg_1.bias"])


def want_trunk(case, windows):
    return np.stack([case["trunk"][int(w)] for w in windows])


def run_metrics(case, emb, taps):
    return E.metrics(emb, E.interior(taps["trunk"]), case["want"], want_trunk(case, taps["windows"]), case["active"])


def restatement(case, taps=None, **kw):
    """-> (embeddings, taps, metrics against the fp32 oracle) of one run of the restatement"""
    taps = {} if taps is None else taps
    emb = E.wespeaker_bf16(case["emb_sd"], case["feats"], case["wins"], case["masks"], taps, **kw)
    return emb, taps, run_metrics(case, emb, taps)


def yardstick(runs):
    """runs {name: metrics} -> (yardstick, factor) per metric"""
    yard = {k: max(r[k] for r in runs.values()) for k in E.METRICS}
    fac = {k: max(1.25, 1.06 * yard[k] / float(np.median([r[k] for r in runs.values()]))) for k in E.METRICS}
    return yard, fac


def document(case, runs):
    yard, fac = yardstick(runs)
    return dict(seconds=SECONDS, pcm_seed=PCM_SEED, weights_seed=WEIGHTS_SEED, mask_seed=MASK_SEED, jitter=E._B.JITTER,
                windows=[int(w) for w in sorted(set(case["wins"].tolist()))], items=int(len(case["wins"])),
                active_items=int(case["active"].sum()), runs=runs, yardstick=yard, factor=fac)


def all_runs(case, keep=None):
    runs = {}
    for name, seed in [("plain", None)] + [("jitter%d" % j, j) for j in range(1, JITTERS + 1)]:
        emb, taps, runs[name] = restatement(case, jitter_seed=seed)
        if keep is not None and name == "plain":
            keep["emb"], keep["taps"] = emb, taps
    return runs


def main():
    case = make_case()
    doc = document(case, all_runs(case))
    print(json.dumps(dict(yardstick=doc["yardstick"], factor=doc["factor"]), indent=1))
    with open(FIXTURE, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
