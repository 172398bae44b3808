"""Phrase search over the benched hour: synthetic weights, the recording encoded once, phrases of 4 tokens cut from the engine's own
greedy tokens (so they do occur).  Prints one JSON line: per case (1 / 100 / 1000 phrases as ONE sequence over the hour; 100 phrases
as one sequence per chunk) the wall time of Engine.find (host clock, median of --reps) and the "ctc_find" / "ctc_align_lp" device
times of rvb_get_timing (HIP events; a profiled run of its own), and the yardstick: Engine.align_wild of `<star> phrase <star>` over
the same hour, one call per phrase, for --wild phrases.

    python scripts/find_bench.py [--model r640] [--dtype bf16] [--seconds 3600] [--reps 3] [--wild 4]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--model", default="r640")
    p.add_argument("--dtype", default="bf16")
    p.add_argument("--seconds", type=float, default=3600.0)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--wild", type=int, default=4, help="phrases timed through align_wild, one call each")
    a = p.parse_args()
    from reverb_amd import synth
    from reverb_amd.ctc_align import WILDCARD
    from reverb_amd.engine import Engine
    chunk = 2051
    cfg, sd = synth.calibrated_state_dict(a.model, 0)
    pcm = synth.synth_audio(a.seconds, seed=1234)
    n_chunks = -(-int((len(pcm) - 400) // 160 + 1) // chunk)
    eng = Engine(cfg, sd, dtype=a.dtype, device=0, max_chunks=n_chunks, chunk_frames=chunk)
    eng.upload_pcm(pcm)
    n = eng.fbank()
    lens = np.full(n_chunks, chunk, np.int32)
    lens[-1] = n - (n_chunks - 1) * chunk
    eng.encode(None, lens, 1, 0.0, T0=chunk)
    tokens = [t for g in eng.greedy() for t in g.tokens]
    T = int(eng.encoder_lens().sum())
    rng = np.random.default_rng(0)
    starts = rng.integers(0, len(tokens) - 4, size=1000)
    phrases = [tokens[s:s + 4] for s in starts]
    out = {"model": a.model, "dtype": a.dtype, "frames": T, "chunks": n_chunks, "cases": []}
    for name, n_phr, ranges in (("1 phrase, one sequence", 1, [(0, n_chunks)]), ("100 phrases, one sequence", 100, [(0, n_chunks)]),
                                ("1000 phrases, one sequence", 1000, [(0, n_chunks)]),
                                ("100 phrases, one sequence per chunk", 100, [(c, 1) for c in range(n_chunks)])):
        ph = phrases[:n_phr]
        eng.set_profiling(False)
        found = eng.find(ph, ranges)                            # warm-up: buffers allocated
        wall = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            found = eng.find(ph, ranges)
            wall.append((time.perf_counter() - t0) * 1e3)
        eng.set_profiling(True)
        eng.reset_timings()
        for _ in range(a.reps):
            eng.find(ph, ranges)
        k, lp = eng.timing("ctc_find"), eng.timing("ctc_align_lp")
        out["cases"].append({"case": name, "pairs": n_phr * len(ranges), "find_wall_ms": [round(w, 2) for w in wall],
                             "find_wall_ms_median": round(float(np.median(wall)), 2), "ctc_find_ms": round(k["ms"] / a.reps, 3),
                             "ctc_find_launches": k["launches"] // a.reps, "ctc_align_lp_ms": round(lp["ms"] / a.reps, 3),
                             "ctc_find_us_per_frame": round(k["ms"] / a.reps * 1e3 / T, 4), "hits": sum(len(s) for per in found for s in per),
                             "calls": eng.last_find["calls"]})
    eng.set_profiling(False)
    wild_wall = []
    for ph in phrases[:a.wild + 1]:                             # the first call warms up
        t0 = time.perf_counter()
        eng.align_wild([[WILDCARD] + ph + [WILDCARD]], [(0, n_chunks)], 0.0)
        wild_wall.append((time.perf_counter() - t0) * 1e3)
    eng.set_profiling(True)
    eng.reset_timings()
    for ph in phrases[:a.wild]:
        eng.align_wild([[WILDCARD] + ph + [WILDCARD]], [(0, n_chunks)], 0.0)
    vit, lp = eng.timing("ctc_viterbi"), eng.timing("ctc_align_lp")
    out["align_wild"] = {"phrases": a.wild, "wall_ms_per_phrase": [round(w, 2) for w in wild_wall[1:]],
                         "wall_ms_per_phrase_median": round(float(np.median(wild_wall[1:])), 2),
                         "ctc_viterbi_ms_per_phrase": round(vit["ms"] / a.wild, 3), "ctc_align_lp_ms_per_phrase": round(lp["ms"] / a.wild, 3)}
    print(json.dumps(out))
    eng.close()


if __name__ == "__main__":
    main()
