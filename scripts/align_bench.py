"""Forced alignment of the benched hour: synthetic weights, transcript = the engine's own greedy tokens of the whole recording,
ONE lattice over all chunks.  Prints one JSON line: wall time of Engine.align per repetition (host clock around a call that ends in a
device synchronise) and the "ctc_align_lp" / "ctc_viterbi" device times of rvb_get_timing (HIP events; a profiled run of its own).

    python scripts/align_bench.py [--model r640] [--dtype bf16] [--seconds 3600] [--reps 5] [--warmup 2] [--score [--attention]] [--graph] [--graph_score]

--graph also times Engine.align_graph on the same transcript as a chain graph (csrc/ctc_graph.hip against csrc/ctc_viterbi.hip on the
same log-probs; the "ctc_graph" device time).  A graph holds at most 8192 nodes: choose --seconds so that the tokens fit.

--graph_score times Engine.score_graph on the same transcript as a chain graph (csrc/ctc_graph_score.hip against
csrc/ctc_forward_backward.hip on the same log-probs): the "ctc_graph_forward" / "ctc_graph_backward" device times beside
"ctc_forward" / "ctc_backward" of Engine.score, both with posteriors.  The same cap of 8192 nodes holds.

--score --attention also times Engine.attention_score: every chunk's own greedy tokens against that chunk, all chunks in one call,
both decoders (reverse_weight 0.3): the wall time per call and the "lse_gather" device time, which is the row_xent kernel there.
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
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--score", action="store_true", help="also time Engine.score of the same lattice: ctc_forward / ctc_backward")
    p.add_argument("--graph", action="store_true", help="also time Engine.align_graph of the transcript as a chain graph: ctc_graph")
    p.add_argument("--graph_score", action="store_true",
                   help="also time Engine.score_graph of the transcript as a chain graph against Engine.score: ctc_graph_forward / _backward")
    p.add_argument("--attention", action="store_true", help="with --score: also time Engine.attention_score, one sequence per chunk")
    a = p.parse_args()
    from reverb_amd import synth
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
    for _ in range(a.warmup):
        res = eng.align([tokens], [(0, n_chunks)])[0]
    wall = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        res = eng.align([tokens], [(0, n_chunks)])[0]
        wall.append((time.perf_counter() - t0) * 1e3)
    eng.set_profiling(True)
    eng.reset_timings()
    for _ in range(a.reps):
        eng.align([tokens], [(0, n_chunks)])
    lp, vit = eng.timing("ctc_align_lp"), eng.timing("ctc_viterbi")
    extra = {}
    if a.score:
        # full-sum score of the same lattice: forward only (wall), then with posteriors under the profiler
        for _ in range(a.warmup):
            sc = eng.score([tokens], [(0, n_chunks)], posteriors=True)[0]
        eng.set_profiling(False)
        swall = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            eng.score([tokens], [(0, n_chunks)])
            swall.append((time.perf_counter() - t0) * 1e3)
        eng.set_profiling(True)
        eng.reset_timings()
        for _ in range(a.reps):
            sc = eng.score([tokens], [(0, n_chunks)], posteriors=True)[0]
        fw, bw = eng.timing("ctc_forward"), eng.timing("ctc_backward")
        extra = {"score_forward_wall_ms_median": round(float(np.median(swall)), 2), "ctc_forward_ms": round(fw["ms"] / a.reps, 3),
                 "ctc_backward_ms": round(bw["ms"] / a.reps, 3), "forward_us_per_frame": round(fw["ms"] / a.reps * 1e3 / T, 3),
                 "backward_us_per_frame": round(bw["ms"] / a.reps * 1e3 / T, 3), "loglik": sc["loglik"],
                 "alpha_rows_bytes": 4 * T * ((2 * len(tokens) + 1 + 31) // 32 * 32)}
    if a.score and a.attention:
        per_chunk = [g.tokens for g in eng.greedy()]
        keep = [b for b, t in enumerate(per_chunk) if t]
        seqs = [per_chunk[b] for b in keep]
        eng.set_profiling(False)
        for _ in range(a.warmup):
            att = eng.attention_score(seqs, keep, reverse_weight=0.3, lsm_weight=0.1)
        awall = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            eng.attention_score(seqs, keep, reverse_weight=0.3, lsm_weight=0.1)
            awall.append((time.perf_counter() - t0) * 1e3)
        eng.set_profiling(True)
        eng.reset_timings()
        for _ in range(a.reps):
            eng.attention_score(seqs, keep, reverse_weight=0.3, lsm_weight=0.1)
        rx = eng.timing("lse_gather")
        npos = sum(r["n_positions"] for r in att)
        extra.update({"attention_score_wall_ms_median": round(float(np.median(awall)), 2), "attention_positions": npos,
                      "row_xent_ms": round(rx["ms"] / a.reps, 3), "row_xent_launches": rx["launches"] // a.reps,
                      "acc_att": sum(r["n_correct"] for r in att) / npos})
    if a.graph:
        from reverb_amd.token_graph import TokenGraph
        chain = TokenGraph.chain(tokens)
        eng.set_profiling(False)
        for _ in range(a.warmup):
            gres = eng.align_graph([chain], [(0, n_chunks)])[0]
        gwall = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            gres = eng.align_graph([chain], [(0, n_chunks)])[0]
            gwall.append((time.perf_counter() - t0) * 1e3)
        eng.set_profiling(True)
        eng.reset_timings()
        for _ in range(a.reps):
            eng.align_graph([chain], [(0, n_chunks)])
        gr = eng.timing("ctc_graph")
        extra.update({"align_graph_wall_ms_median": round(float(np.median(gwall)), 2), "ctc_graph_ms": round(gr["ms"] / a.reps, 3),
                      "graph_us_per_frame": round(gr["ms"] / a.reps * 1e3 / T, 3),
                      "graph_equals_chain": gres.labels == res.labels and gres.score == res.score})
    if a.graph_score:
        from reverb_amd.token_graph import TokenGraph
        chain = TokenGraph.chain(tokens)
        for _ in range(a.warmup):
            gs = eng.score_graph([chain], [(0, n_chunks)], posteriors=True)[0]
            cs = eng.score([tokens], [(0, n_chunks)], posteriors=True)[0]
        eng.set_profiling(False)
        gswall = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            eng.score_graph([chain], [(0, n_chunks)])
            gswall.append((time.perf_counter() - t0) * 1e3)
        eng.set_profiling(True)
        eng.reset_timings()
        for _ in range(a.reps):
            gs = eng.score_graph([chain], [(0, n_chunks)], posteriors=True)[0]
            cs = eng.score([tokens], [(0, n_chunks)], posteriors=True)[0]
        t = {k: eng.timing(k)["ms"] / a.reps for k in ("ctc_graph_forward", "ctc_graph_backward", "ctc_forward", "ctc_backward")}
        extra.update({"score_graph_forward_wall_ms_median": round(float(np.median(gswall)), 2),
                      **{k + "_ms": round(v, 3) for k, v in t.items()},
                      **{k + "_us_per_frame": round(v * 1e3 / T, 3) for k, v in t.items()},
                      "graph_loglik": gs["loglik"], "chain_loglik": cs["loglik"],
                      "graph_alpha_rows_bytes": 4 * T * ((len(tokens) + 63) // 64 * 64)})
    print(json.dumps({"model": a.model, "dtype": a.dtype, "frames": T, "tokens": len(tokens), "states": 2 * len(tokens) + 1,
                      "align_wall_ms": [round(w, 2) for w in wall], "align_wall_ms_median": round(float(np.median(wall)), 2),
                      "ctc_align_lp_ms": round(lp["ms"] / a.reps, 3), "ctc_viterbi_ms": round(vit["ms"] / a.reps, 3),
                      "viterbi_us_per_frame": round(vit["ms"] / a.reps * 1e3 / T, 3), "score": res.score, **extra}))
    eng.close()


if __name__ == "__main__":
    main()
