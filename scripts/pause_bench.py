"""chunking="pauses" against chunking="fixed" on the same engine: what the moved cuts cost.

    python scripts/pause_bench.py [--model r640] [--dtype bf16] [--steps 3] [--warmup 1] [--hours 1.0] [--many 64x30]

Two workloads with the synthetic weights bench.py uses, attention_rescoring, chunk_size 2051, the defaults of the two pause parameters
(search = chunk_size // 4, smooth = 10): (a) the benchmark hour of synth.synth_audio as one recording (fbank + decode_resident, the
samples resident before the timed region, max_chunks = the fixed chunk count as in bench.py, so the extra pieces of "pauses" cost a
second, small encode), (b) recordings cut from that hour through upload_batch + decode_batch.  The two ways alternate within one
process, step by step.  Per workload and way: the chunk count, the step time (median and range over the timed steps) and, from one
more step with the stage timer on, the milliseconds under "pause_chunks" (the three kernels and the table copy between them).
Pause cuts make more and shorter chunks, every one padded to chunk_size: the slowdown is mostly padding.  One JSON line per
(workload, way) at the end.  No word error rate can be measured here: the weights are synthetic."""
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
    p.add_argument("--steps", type=int, default=3)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--hours", type=float, default=1.0)
    p.add_argument("--many", default="64x30", help="COUNTxSECONDS of the recordings of workload (b)")
    p.add_argument("--beam", type=int, default=10)
    a = p.parse_args()
    import torch
    from reverb_amd import synth
    from reverb_amd.engine import Engine

    chunk, modes = 2051, ["attention_rescoring"]
    n_samples = int(round(a.hours * 3600.0 * 16000))
    n_chunks = -(-(1 + (n_samples - 400) // 160) // chunk)
    cfg, sd = synth.calibrated_state_dict(a.model, 0)
    eng = Engine(cfg, sd, dtype=a.dtype, device=0, max_chunks=n_chunks, chunk_frames=chunk)
    hour = synth.synth_audio(a.hours * 3600.0, seed=1234)
    count, sec = a.many.split("x")
    count, ns = int(count), int(float(sec) * 16000)
    stride = max((len(hour) - ns) // max(count - 1, 1), 1)
    items = [(np.ascontiguousarray(hour[(i * stride) % (len(hour) - ns + 1):][:ns]), 16000) for i in range(count)]
    pieces = {}

    def one_hour(way):
        out = eng.decode_resident(eng.fbank(), modes, chunk, a.beam, 0.1, 0.0, chunking=way)
        pieces["hour", way] = len((out[0] if way == "pauses" else out)[modes[0]])

    def many(way):
        out = eng.decode_batch(modes, chunk, a.beam, 0.1, 0.0, chunking=way)
        pieces["many", way] = sum(len(r[modes[0]]) for r in (out[0] if way == "pauses" else out))

    records = []
    for label, setup, run, audio_s in (("hour", lambda: eng.upload_pcm(hour), one_hour, a.hours * 3600.0),
                                       ("many " + a.many, lambda: None, many, count * float(sec))):
        key = label.split()[0]
        times = {"fixed": [], "pauses": []}
        setup()
        for s in range(a.warmup + a.steps + 1):
            profiled = s == a.warmup + a.steps           # the last step: stage timer on, not among the timed ones
            for way in ("fixed", "pauses"):
                if key == "many":
                    eng.upload_batch(items)              # a batch is uploaded per call (transcribe_modes_many does); not timed
                eng.set_profiling(profiled)
                eng.reset_timings()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(way)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                if profiled:
                    times[way + "_stage_ms"] = eng.timing("pause_chunks")["ms"]
                    times[way + "_stage_launches"] = int(eng.timing("pause_chunks")["launches"])
                elif s >= a.warmup:
                    times[way].append(dt)
        eng.set_profiling(False)
        med = {w: float(np.median(times[w])) for w in ("fixed", "pauses")}
        for way in ("fixed", "pauses"):
            t = np.array(times[way])
            rec = {"workload": label, "chunking": way, "model": a.model, "dtype": a.dtype, "steps": a.steps, "warmup": a.warmup,
                   "chunks": pieces[key, way], "step_ms_median": 1e3 * med[way], "step_ms_min": 1e3 * float(t.min()),
                   "step_ms_max": 1e3 * float(t.max()), "rtfx": audio_s / med[way], "slowdown_vs_fixed": med[way] / med["fixed"],
                   "pause_chunks_ms": times[way + "_stage_ms"], "pause_chunks_launches": times[way + "_stage_launches"],
                   "pause_chunks_share_of_step": times[way + "_stage_ms"] / (1e3 * med[way])}
            records.append(rec)
            print("%-12s %-6s %4d chunks  step %8.2f ms (%.2f .. %.2f)  RTFx %7.0f  x%.3f of fixed  pause_chunks %.3f ms (%.2f %% of a step)" % (
                label, way, rec["chunks"], rec["step_ms_median"], rec["step_ms_min"], rec["step_ms_max"], rec["rtfx"],
                rec["slowdown_vs_fixed"], rec["pause_chunks_ms"], 100.0 * rec["pause_chunks_share_of_step"]), flush=True)
    for rec in records:
        print(json.dumps(rec))
    eng.close()


if __name__ == "__main__":
    main()
