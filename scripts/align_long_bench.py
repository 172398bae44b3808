"""Long-form forced alignment against the one-batch aligner, synthetic weights, transcript = the engine's own greedy tokens.

    python scripts/align_long_bench.py [--model r640] [--dtype bf16] [--hours 1.0] [--repeat 3] [--max_chunks 64] [--reps 3] [--warmup 1]

(a) the benchmark recording (--hours of synth.synth_audio, seed 1234) aligned as ONE lattice two ways, alternating rep by rep in one
    process: "one_batch" = an engine whose max_chunks holds the file: one encode, Engine.align (csrc/ctc_viterbi.hip; labels, times and
    the second sweep for the confidences); "long" = an engine with --max_chunks: encode + Engine.align_long_feed per batch, finish
    (csrc/ctc_viterbi_window.hip), and "long_conf" = the same plus the second pass of encodes with Engine.align_long_emissions.  Wall
    seconds (host clock around work that ends in a device synchronise), and from one more profiled repetition the device
    milliseconds under "ctc_viterbi" / "ctc_viterbi_window" and the encoder's share.  The two label sequences are compared.
(b) the recording --repeat times in a row (nothing before the long path aligns it): seconds, back-pointer bytes, window margin.
One JSON line per measurement at the end."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CHUNK = 2051


def chunk_lens(n_frames):
    n = -(-n_frames // CHUNK)
    lens = np.full(n, CHUNK, np.int32)
    lens[-1] = n_frames - (n - 1) * CHUNK
    return lens


def batches(eng, lens):
    mc = eng.cfg.max_chunks
    for c0 in range(0, len(lens), mc):
        eng.encode(None, lens[c0:c0 + mc], 1, 0.0, first_chunk=c0, T0=CHUNK)
        yield int(eng.encoder_lens().sum())


def long_align(eng, lens, tokens, confidences, window_states=0):
    total = int(sum((int(n) - 7) // 4 + 1 for n in lens))
    used = eng.align_long_begin(tokens, total, window_states)
    for _ in batches(eng, lens):
        eng.align_long_feed()
    labels, begin, end, score, margin = eng.align_long_finish()
    if confidences:
        f0 = 0
        for n in batches(eng, lens):
            eng.align_long_emissions(labels[f0:f0 + n])
            f0 += n
    eng.align_long_end()
    return labels, score, margin, used, total


def timed(fn, sync):
    sync()
    t0 = time.perf_counter()
    out = fn()
    sync()
    return time.perf_counter() - t0, out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--model", default="r640")
    p.add_argument("--dtype", default="bf16")
    p.add_argument("--hours", type=float, default=1.0)
    p.add_argument("--repeat", type=int, default=3, help="workload (b): the recording this many times in a row (0: skip)")
    p.add_argument("--max_chunks", type=int, default=64)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--warmup", type=int, default=1)
    a = p.parse_args()
    import torch
    from reverb_amd import synth
    from reverb_amd.engine import Engine
    sync = torch.cuda.synchronize
    cfg, sd = synth.calibrated_state_dict(a.model, 0)
    hour = synth.synth_audio(a.hours * 3600.0, seed=1234)
    n_chunks = -(-(1 + (len(hour) - 400) // 160) // CHUNK)
    big = Engine(cfg, sd, dtype=a.dtype, device=0, max_chunks=n_chunks, chunk_frames=CHUNK)
    small = Engine(cfg, sd, dtype=a.dtype, device=0, max_chunks=a.max_chunks, chunk_frames=CHUNK)
    for eng in (big, small):
        eng.upload_pcm(hour)
    lens = chunk_lens(big.fbank())
    assert len(chunk_lens(small.fbank())) == len(lens) == n_chunks
    big.encode(None, lens, 1, 0.0, T0=CHUNK)
    tokens = [t for g in big.greedy() for t in g.tokens]
    T = int(big.encoder_lens().sum())

    def one_batch():
        big.encode(None, lens, 1, 0.0, T0=CHUNK)
        return big.align([tokens], [(0, n_chunks)])[0]

    ways = {"one_batch": one_batch, "long": lambda: long_align(small, lens, tokens, False),
            "long_conf": lambda: long_align(small, lens, tokens, True)}
    wall = {k: [] for k in ways}
    out = {}
    for s in range(a.warmup + a.reps):
        for k, fn in ways.items():
            dt, out[k] = timed(fn, sync)
            if s >= a.warmup:
                wall[k].append(dt)
    same = out["one_batch"].labels == out["long"][0].tolist()
    prof = {}
    for k, eng, scope in (("one_batch", big, "ctc_viterbi"), ("long", small, "ctc_viterbi_window"), ("long_conf", small, "ctc_viterbi_window")):
        eng.set_profiling(True)
        eng.reset_timings()
        dt, _ = timed(ways[k], sync)
        prof[k] = {"scope": scope, "scope_ms": eng.timing(scope)["ms"], "scope_launches": int(eng.timing(scope)["launches"]),
                   "ctc_align_lp_ms": eng.timing("ctc_align_lp")["ms"], "profiled_wall_s": dt}
        eng.set_profiling(False)
    records = []
    for k in ways:
        w = np.array(wall[k])
        rec = {"workload": "hour", "way": k, "model": a.model, "dtype": a.dtype, "frames": T, "tokens": len(tokens), "chunks": n_chunks,
               "max_chunks": big.cfg.max_chunks if k == "one_batch" else a.max_chunks, "reps": a.reps, "warmup": a.warmup,
               "wall_s_median": float(np.median(w)), "wall_s_min": float(w.min()), "wall_s_max": float(w.max()),
               "viterbi_scope": prof[k]["scope"], "viterbi_ms": prof[k]["scope_ms"], "viterbi_launches": prof[k]["scope_launches"],
               "viterbi_us_per_frame": 1e3 * prof[k]["scope_ms"] / T, "viterbi_share_of_wall": 1e-3 * prof[k]["scope_ms"] / float(np.median(w)),
               "ctc_align_lp_ms": prof[k]["ctc_align_lp_ms"], "labels_equal_one_batch": bool(same)}
        if k != "one_batch":
            rec.update(window_states=out[k][3], window_margin=out[k][2], back_pointer_bytes=out[k][4] * (out[k][3] // 4))
        records.append(rec)
        print("%-10s wall %.3f s (%.3f .. %.3f)  %s %.1f ms in %d launches = %.2f us/frame, %.1f %% of the wall" % (
            k, rec["wall_s_median"], rec["wall_s_min"], rec["wall_s_max"], rec["viterbi_scope"], rec["viterbi_ms"], rec["viterbi_launches"],
            rec["viterbi_us_per_frame"], 100 * rec["viterbi_share_of_wall"]), flush=True)
    big.close()
    if a.repeat > 0:
        pcm = np.concatenate([hour] * a.repeat)
        small.upload_pcm(pcm)
        lens3 = chunk_lens(small.fbank())
        toks3 = [t for _ in batches(small, lens3) for g in small.greedy() for t in g.tokens]
        w3 = []
        for s in range(a.warmup + a.reps):
            dt, res = timed(lambda: long_align(small, lens3, toks3, False), sync)
            if s >= a.warmup:
                w3.append(dt)
        small.set_profiling(True)
        small.reset_timings()
        timed(lambda: long_align(small, lens3, toks3, False), sync)
        vit = small.timing("ctc_viterbi_window")
        rec = {"workload": "%d x hour" % a.repeat, "way": "long", "model": a.model, "dtype": a.dtype, "frames": res[4], "tokens": len(toks3),
               "chunks": len(lens3), "max_chunks": a.max_chunks, "reps": a.reps, "warmup": a.warmup, "wall_s_median": float(np.median(w3)),
               "wall_s_min": float(min(w3)), "wall_s_max": float(max(w3)), "viterbi_ms": vit["ms"], "viterbi_launches": int(vit["launches"]),
               "viterbi_us_per_frame": 1e3 * vit["ms"] / res[4], "window_states": res[3], "window_margin": res[2],
               "back_pointer_bytes": res[4] * (res[3] // 4), "score": res[1]}
        records.append(rec)
        print("%d x hour: %d tokens, %d frames: wall %.3f s, back-pointers %.2f GB, window margin %d" % (
            a.repeat, len(toks3), res[4], rec["wall_s_median"], rec["back_pointer_bytes"] / 1e9, rec["window_margin"]), flush=True)
    for rec in records:
        print(json.dumps(rec))
    small.close()


if __name__ == "__main__":
    main()
