"""Long-form full-sum scoring beside long-form alignment, synthetic weights, transcript = the engine's own greedy tokens.

    python scripts/score_long_bench.py [--model r640] [--dtype bf16] [--hours 1.0] [--max_chunks 64] [--reps 3] [--warmup 1]
                                       [--window_states 0]

The benchmark recording (--hours of synth.synth_audio, seed 1234) on an engine with --max_chunks, three ways, alternating rep by rep
in one process: "align_long" = encode + Engine.align_long_feed per batch, finish (csrc/ctc_viterbi_window.hip: what
scripts/align_long_bench.py calls "long"); "score_long" = encode + Engine.score_long_feed per batch, loglik (csrc/ctc_fb_window.hip,
forward sweep only); "score_long_post" = the same with posteriors: the forward rows are kept and the batches are encoded a second time
in reverse order for Engine.score_long_feed_back.  Wall seconds (host clock around work that ends in a device synchronise) and, from
one more profiled repetition, the device milliseconds under "ctc_fb_window_forward" / "ctc_fb_window_backward" /
"ctc_viterbi_window".  One JSON line per way at the end."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from align_long_bench import CHUNK, batches, chunk_lens, long_align, timed      # noqa: E402


def long_score(eng, lens, tokens, posteriors, window_states=0):
    total = int(sum((int(n) - 7) // 4 + 1 for n in lens))
    mc = eng.cfg.max_chunks
    used = eng.score_long_begin(tokens, total, window_states, posteriors)
    try:
        for _ in batches(eng, lens):
            eng.score_long_feed()
        ll = eng.score_long_loglik()
        post = None
        if posteriors:
            for c0 in reversed(range(0, len(lens), mc)):
                eng.encode(None, lens[c0:c0 + mc], 1, 0.0, first_chunk=c0, T0=CHUNK)
                eng.score_long_feed_back()
            post = eng.score_long_finish()
    finally:
        eng.score_long_end()
    return ll, post, used, total


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--model", default="r640")
    p.add_argument("--dtype", default="bf16")
    p.add_argument("--hours", type=float, default=1.0)
    p.add_argument("--max_chunks", type=int, default=64)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--window_states", type=int, default=0)
    a = p.parse_args()
    import torch
    from reverb_amd import synth
    from reverb_amd.engine import Engine
    sync = torch.cuda.synchronize
    cfg, sd = synth.calibrated_state_dict(a.model, 0)
    eng = Engine(cfg, sd, dtype=a.dtype, device=0, max_chunks=a.max_chunks, chunk_frames=CHUNK)
    eng.upload_pcm(synth.synth_audio(a.hours * 3600.0, seed=1234))
    lens = chunk_lens(eng.fbank())
    tokens = [t for _ in batches(eng, lens) for g in eng.greedy() for t in g.tokens]
    ways = {"align_long": lambda: long_align(eng, lens, tokens, False, a.window_states),
            "score_long": lambda: long_score(eng, lens, tokens, False, a.window_states),
            "score_long_post": lambda: long_score(eng, lens, tokens, True, a.window_states)}
    wall, out = {k: [] for k in ways}, {}
    for s in range(a.warmup + a.reps):
        for k, fn in ways.items():
            dt, out[k] = timed(fn, sync)
            if s >= a.warmup:
                wall[k].append(dt)
    scopes = ("ctc_viterbi_window", "ctc_fb_window_forward", "ctc_fb_window_backward", "ctc_align_lp")
    for k, fn in ways.items():
        eng.set_profiling(True)
        eng.reset_timings()
        dt, _ = timed(fn, sync)
        w = np.array(wall[k])
        rec = {"workload": "%g h" % a.hours, "way": k, "model": a.model, "dtype": a.dtype, "tokens": len(tokens), "chunks": len(lens),
               "max_chunks": a.max_chunks, "reps": a.reps, "warmup": a.warmup, "wall_s_median": float(np.median(w)),
               "wall_s_min": float(w.min()), "wall_s_max": float(w.max()), "profiled_wall_s": dt}
        for sc in scopes:
            rec[sc + "_ms"] = eng.timing(sc)["ms"]
            rec[sc + "_launches"] = int(eng.timing(sc)["launches"])
        eng.set_profiling(False)
        if k == "align_long":
            rec.update(frames=out[k][4], window_states=out[k][3], viterbi_score=float(out[k][1]))
        else:
            rec.update(frames=out[k][3], window_states=out[k][2], loglik=out[k][0],
                       alpha_row_bytes=out[k][3] * out[k][2] * 4 if k == "score_long_post" else 0)
        out[k] = rec
        print("%-16s wall %.3f s (%.3f .. %.3f)" % (k, rec["wall_s_median"], rec["wall_s_min"], rec["wall_s_max"]), flush=True)
    for rec in out.values():
        print(json.dumps(rec))
    eng.close()


if __name__ == "__main__":
    main()
