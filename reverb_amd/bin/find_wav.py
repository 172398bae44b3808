"""Phrase search: where in an audio file are the phrases of a list spoken?  Every occurrence of every phrase (ReverbASR.find:
rvb_ctc_find on the CTC log-probs, one wave of the device per phrase) is written to `<result_dir>/<audio>.find.<json|ctm>`.
json: one record per phrase with its hits (start / end in seconds, frames, score, score_per_token, confidence).
ctm: one line per hit, `<audio> 0 <start s> <duration s> <phrase> <confidence>`, the phrase standing where a CTM has its word (blanks
inside it become `_`) and confidence = exp(score / tokens of the phrase); lines in order of start time."""
from __future__ import annotations

import argparse
import json
import logging
import os
from pathlib import Path


def get_args(argv=None):
    p = argparse.ArgumentParser(description="find every occurrence of the phrases of a list in an audio file")
    p.add_argument("--model", default=None, help="reverb model name or a directory with config.yaml and a .pt file")
    p.add_argument("--config", default=None, help="config file")
    p.add_argument("--checkpoint", default=None, help="checkpoint model")
    p.add_argument("--audio_file", required=True, help="audio to search")
    p.add_argument("--phrase_list", required=True, help="text file, one phrase (a name, a term) per line")
    p.add_argument("--result_dir", required=True, help="directory of the result file")
    p.add_argument("--min_score", type=float, default=-1.0,
                   help="lowest score per token (nats, <= 0) of a reported occurrence; 0 = the model's own best labels spell the phrase")
    p.add_argument("--max_hits", type=int, default=64, help="most occurrences reported per phrase and encoded batch")
    p.add_argument("--format", default="json", choices=["json", "ctm"], help="per-phrase JSON, or one CTM line per hit")
    p.add_argument("--gpu", type=int, default=-1, help="gpu id for this rank, -1 means device 0")
    p.add_argument("--chunk_size", type=int, default=2051, help="Chunk size")
    p.add_argument("--verbatimicity", type=float, default=1.0, help="the level of verbatimicity to run the model")
    p.add_argument("--timings_adjustment", type=float, default=230, help="time shift applied to all timings (ms)")
    p.add_argument("--log_level", default="INFO", help="log level")
    p.add_argument("--dtype", default="bf16", choices=["bf16", "f32"], help="device compute mode")
    p.add_argument("--max_chunks", type=int, default=64, help="chunks per device batch; an occurrence across two batches is not found")
    args = p.parse_args(argv)
    if not args.min_score <= 0:
        p.error("--min_score must be <= 0")
    if args.max_hits < 1:
        p.error("--max_hits must be >= 1")
    return args


def to_ctm(audio_name: str, found) -> str:
    lines = []
    for rec in found:
        word = "_".join(rec["phrase"].split())
        for h in rec["hits"]:
            lines.append((h["start"], f"{audio_name} 0 {h['start']:.2f} {h['end'] - h['start']:.2f} {word} {h['confidence']:.2f}"))
    return "\n".join(line for _, line in sorted(lines, key=lambda x: x[0]))


def main(argv=None):
    args = get_args(argv)
    logging.basicConfig(level=getattr(logging, str(args.log_level).upper(), logging.INFO),
                        format="%(asctime)s %(levelname)s %(message)s")
    from reverb_amd.reverb import ReverbASR, load_model
    if (args.model is not None) == (args.checkpoint is not None and args.config is not None):
        raise RuntimeError("One of either --model or (--checkpoint and --config) must be set.")
    if args.model:
        reverb = load_model(args.model, gpu=args.gpu, dtype=args.dtype, max_chunks=args.max_chunks)
    else:
        reverb = ReverbASR(args.config, args.checkpoint, gpu=args.gpu, dtype=args.dtype, max_chunks=args.max_chunks)
    found = reverb.find(args.audio_file, phrase_file=args.phrase_list, min_score=args.min_score, max_hits=args.max_hits,
                        verbatimicity=args.verbatimicity, chunk_size=args.chunk_size, timings_adjustment=args.timings_adjustment)
    name = Path(args.audio_file).name
    out = to_ctm(name, found) if args.format == "ctm" else json.dumps(found, ensure_ascii=False, indent=1)
    os.makedirs(args.result_dir, exist_ok=True)
    path = os.path.join(args.result_dir, Path(args.audio_file).with_suffix(".find." + args.format).name)
    with open(path, "w", encoding="utf-8") as f:
        f.write(out)
    logging.info("wrote %s (%d hits of %d phrases)", path, sum(len(r["hits"]) for r in found), len(found))


if __name__ == "__main__":
    main()
