"""Many short recordings: a loop of single-recording ReverbASR.transcribe_modes calls against one transcribe_modes_many call.

    python scripts/batch_bench.py [--model r640] [--dtype bf16] [--steps 3] [--warmup 1] [--short 256x30] [--long 64x180]

Synthetic weights as bench.py uses them, attention_rescoring.  The recordings (256 of 30 s and 64 of 180 s by default) are cut from
one hour of synth.synth_audio and held in memory as (waveform, rate), so that the engine is measured and not the disk: leg (a) hands
transcribe_modes a name that a replaced _load_pcm looks up, leg (b) hands transcribe_modes_many the pairs.  Each step ends with a
device synchronise.  Per set and leg: recordings per second and RTFx as the median over the timed steps with their range, and the
"fbank" launches and rvb_encode calls of one step.  One JSON line per (set, leg) at the end."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--model", default="r640")
    p.add_argument("--dtype", default="bf16")
    p.add_argument("--steps", type=int, default=3)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--short", default="256x30", help="COUNTxSECONDS of the short set")
    p.add_argument("--long", default="64x180", help="COUNTxSECONDS of the long set")
    p.add_argument("--max_chunks", type=int, default=64)
    a = p.parse_args()
    import torch
    import reverb_amd
    from reverb_amd import synth
    hour = synth.synth_audio(3600.0, seed=1234)

    def cut(spec):
        n, sec = spec.split("x")
        n, ns = int(n), int(float(sec) * 16000)
        step = max((len(hour) - ns) // max(n - 1, 1), 1)
        return [(np.ascontiguousarray(hour[(i * step) % (len(hour) - ns + 1):][:ns]), 16000) for i in range(n)], float(sec)

    with tempfile.TemporaryDirectory() as d:
        cfg, sd = synth.calibrated_state_dict(a.model, 0)
        synth.write_model_dir(d, a.model, sd=sd, cfg=cfg)
        del sd
        asr = reverb_amd.load_model(d, dtype=a.dtype, max_chunks=a.max_chunks)
    eng = asr.engine
    store = {}
    asr._load_pcm = lambda name, rate: store[name]          # leg (a): transcribe_modes itself is untouched
    encodes = [0]
    encode = eng.encode

    def counted(*args, **kw):
        encodes[0] += 1
        return encode(*args, **kw)
    eng.encode = counted
    modes = ["attention_rescoring"]
    records = []
    for label, spec in (("short", a.short), ("long", a.long)):
        items, sec = cut(spec)
        store.clear()
        store.update({"rec%05d.wav" % i: it for i, it in enumerate(items)})
        names = sorted(store)
        legs = {"a: loop of transcribe_modes": lambda: [asr.transcribe_modes(n, modes, format="ctm") for n in names],
                "b: transcribe_modes_many": lambda: asr.transcribe_modes_many(items, modes, format="ctm")}
        outs = {}
        for leg, run in legs.items():
            times = []
            for s in range(a.warmup + a.steps):
                eng.reset_timings()
                encodes[0] = 0
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                outs[leg] = run()
                torch.cuda.synchronize()
                if s >= a.warmup:
                    times.append(time.perf_counter() - t0)
            t = np.array(times)
            audio = len(items) * sec
            rec = {"set": spec, "leg": leg, "model": a.model, "dtype": a.dtype, "steps": a.steps, "warmup": a.warmup,
                   "seconds_median": float(np.median(t)), "seconds_min": float(t.min()), "seconds_max": float(t.max()),
                   "recordings_per_s": len(items) / float(np.median(t)), "rtfx": audio / float(np.median(t)),
                   "rtfx_range": [audio / float(t.max()), audio / float(t.min())],
                   "fbank_launches": int(eng.timing("fbank")["launches"]), "encodes": encodes[0]}
            records.append(rec)
            print("%-6s %-32s %8.3f s (%.3f .. %.3f)  %8.1f rec/s  RTFx %8.0f (%.0f .. %.0f)  fbank launches %d, encodes %d" % (
                spec, leg, rec["seconds_median"], rec["seconds_min"], rec["seconds_max"], rec["recordings_per_s"], rec["rtfx"],
                rec["rtfx_range"][0], rec["rtfx_range"][1], rec["fbank_launches"], rec["encodes"]), flush=True)
        la, lb = list(legs)
        same = [x[0].replace(n, str(i)) == y[0] for i, (n, x, y) in enumerate(zip(names, outs[la], outs[lb]))]
        print("%-6s CTM of (b) equal to (a) up to the recording's name: %d of %d" % (spec, sum(same), len(same)), flush=True)
    for rec in records:
        print(json.dumps(rec))


if __name__ == "__main__":
    main()
