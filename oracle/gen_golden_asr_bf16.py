"""TEST INFRASTRUCTURE ONLY.  Writes tests/golden/asr_bf16_yardstick.json (+ .npz): what bf16 STORAGE costs the conformer encoder and its
CTC head, measured with oracle/asr_bf16_ref.py (fp64 arithmetic, rounded to bf16 where the bf16 engine stores or feeds bf16) against
the fp32 oracle (oracle/model_ref.py) on the same synthetic weights and features.  CPU only, about eleven minutes on 8 cores (ten of them r640_chunk):

    python oracle/gen_golden_asr_bf16.py

Cases: the small model of tests/asr_bf16_checks.py (d 256, 4 heads of 64, 3 blocks, K 31; two chunks of 603 frames, encoder lengths
150 and 83) with weight seed 0, with weight seed 1, and with cnn_module_norm = batch_norm; and r640_chunk, the first two chunks of
the benchmark's model (tests/golden/r640_chunk.json: 2051 and 7 frames, encoder lengths 512 and 1; one fp64 run of its 18 blocks takes
77 s here, the fp32 oracle 5 s), yardstick only.  Per case the six metrics of
asr_bf16_ref.metrics for the plain run and for JITTERS runs in which every value is multiplied by 1 +- 2^-20 before it is rounded
(the size of an fp32 summation-order difference); "yardstick" is the maximum over those runs.  tests/test_asr_bf16_gpu.py holds the
engine to asr_bf16_ref.outside_yardstick: 1.25 x yardstick (+ 4 frames on the two counts) on the log-probability figures, 1.05 x
(and its square) on the two encoder_out figures.  The forms are the ones the engine chooses for these shapes (pre-folded
key, GLU in the GEMM's epilogue); the GPU test asserts through the `forms` tap that they ran.

Also recorded per case, for the comparison with the older, looser bounds (tests/test_asr_bf16_ref.py prints it for every mutant):
the greedy CTC token edits of the fp32 oracle under torch.autocast('cpu', bfloat16) against its fp32 run, and the reference tokens.

The GPU test recomputes the fp32 oracle of the small cases on the host; for r640_chunk what the metrics need of it is stored in
the .npz (asr_bf16_ref.golden_arrays: per frame the top-1 label, its log-probability and the top-2 margin; encoder_out sampled
every 4th frame and 8th channel, over which that case's two encoder_out figures are taken, for the yardstick and the engine alike).
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch                                        # noqa: E402
from oracle import asr_bf16_ref as A                # noqa: E402
from oracle import model_ref as M                   # noqa: E402
import asr_bf16_checks as C                         # noqa: E402
from util import edit_distance                      # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = {   # name: (weights seed, cnn_module_norm)
    "forms64_seed0": (0, "layer_norm"),
    "forms64_seed1": (1, "layer_norm"),
    "forms64_bn": (0, "batch_norm"),
    "r640_chunk": None,          # the long-form golden's model, features and category weights
}
JITTERS = 6
R640_STEPS = (4, 8)              # encoder_out sample of the stored oracle: every 4th frame, every 8th channel


def greedy_tokens(logp, lens):
    """CTC greedy per chunk over its valid frames: collapse repeats, drop blanks (id 0)"""
    out = []
    for b, n in enumerate(A.enc_lens(lens)):
        a = np.asarray(logp[b, :n]).argmax(-1)
        keep = np.concatenate([[True], a[1:] != a[:-1]]) & (a != 0)
        out.append([int(t) for t in a[keep]])
    return out


def token_edits(logp, ref_tokens, lens):
    return int(sum(edit_distance(g, w) for g, w in zip(greedy_tokens(logp, lens), ref_tokens)))


def autocast_logp(sd, cfg, feats, lens, cat=C.CAT):
    """the fp32 oracle under torch.autocast('cpu', bfloat16): the yardstick of the older reduced-precision bounds"""
    tsd = M.to_torch_sd(sd)
    with torch.no_grad(), torch.autocast("cpu", dtype=torch.bfloat16):
        enc, _ = M.encoder_forward(tsd, cfg, torch.as_tensor(feats), torch.as_tensor(lens).long(), torch.tensor(cat))
        logp = M.ctc_logprobs(tsd, enc)
    return enc.float().numpy().astype(np.float64), logp.float().numpy().astype(np.float64)


def r640_inputs():
    """-> (cfg, sd, feats [2][2051][80], lens, cat) of the first two chunks of tests/golden/r640_chunk"""
    from golden_util import LongCase
    lc = LongCase("r640_chunk")
    feats = np.concatenate([lc.chunk_feats(c)[0] for c in range(2)])
    return lc.cfg, lc.sd, feats, np.array(lc.js["lens"][:2], np.int32), tuple(lc.cat)


def make_case(name):
    if name == "r640_chunk":
        cfg, sd, feats, lens, cat = r640_inputs()
        enc, logp = A.oracle_fp32(sd, cfg, feats, lens, cat)
        aenc, alogp = autocast_logp(sd, cfg, feats, lens, cat)
        return dict(cfg=cfg, sd=sd, feats=feats, lens=lens, cat=cat, enc=enc, logp=logp, tokens=greedy_tokens(logp, lens), autocast_enc=aenc,
                    autocast_logp=alogp, g=A.golden_arrays(enc, logp, *R640_STEPS))
    seed, norm = CASES[name]
    cfg, sd, feats, lens = C.small_case(seed, norm)
    nt = torch.get_num_threads()
    torch.set_num_threads(1)            # a fixed summation order
    try:
        enc, logp = A.oracle_fp32(sd, cfg, feats, lens, C.CAT)
        aenc, alogp = autocast_logp(sd, cfg, feats, lens)
    finally:
        torch.set_num_threads(nt)
    return dict(cfg=cfg, sd=sd, feats=feats, lens=lens, cat=C.CAT, enc=enc, logp=logp, tokens=greedy_tokens(logp, lens), autocast_enc=aenc,
                autocast_logp=alogp, g=None)


def case_metrics(case, enc, logp):
    """against the full oracle, or (r640_chunk) against what the fixture stores of it"""
    if case["g"] is not None:
        return A.metrics_golden(enc, logp, case["g"], case["lens"])
    return A.metrics(enc, logp, case["enc"], case["logp"], case["lens"])


def restatement_metrics(case, **kw):
    enc, logp = A.encoder_bf16(case["sd"], case["cfg"], case["feats"], case["lens"], case["cat"], **kw)
    m = case_metrics(case, enc, logp)
    m["greedy_token_edits"] = token_edits(logp, case["tokens"], case["lens"])
    return m


def main():
    doc = {"margin": A.MARGIN, "jitter": 2.0 ** -20, "jitters": JITTERS, "model": C.MODEL, "chunk_frames": C.CHUNK_FRAMES,
           "lens": list(C.LENS), "cases": {}}
    arrays = {}
    for name, spec in CASES.items():
        seed, norm = spec if spec else (0, "layer_norm")
        case = make_case(name)
        if case["g"] is not None:
            arrays.update({"%s_%s" % (name, k): v for k, v in case["g"].items()})
        runs = {"plain": restatement_metrics(case)}
        for j in range(1, JITTERS + 1):
            runs["jitter%d" % j] = restatement_metrics(case, jitter_seed=j)
        yard = {k: max(r[k] for r in runs.values()) for k in A.COUNTS + A.MEANS}
        ac = case_metrics(case, case["autocast_enc"], case["autocast_logp"])
        doc["cases"][name] = dict(weights_seed=seed, cnn_module_norm=norm, runs_made=len(runs), lens=[int(v) for v in case["lens"]], frames=runs["plain"]["frames"], confident=runs["plain"]["confident"],
                                  runs=runs, yardstick=yard, reference_tokens=int(sum(len(t) for t in case["tokens"])),
                                  autocast_greedy_token_edits=token_edits(case["autocast_logp"], case["tokens"], case["lens"]),
                                  autocast_metrics=ac)
        print(name, json.dumps(yard), "autocast edits", doc["cases"][name]["autocast_greedy_token_edits"], flush=True)
    with open(os.path.join(GOLDEN, "asr_bf16_yardstick.json"), "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    np.savez_compressed(os.path.join(GOLDEN, "asr_bf16_yardstick.npz"), **arrays)


if __name__ == "__main__":
    main()
