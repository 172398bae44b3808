"""Forced alignment of a known transcript: the job of the reference's `asr/wenet/bin/alignment.py` (:221-242: encoder, CTC
log-softmax, force_align, one `<key> [labels]` line per utterance) for one audio file and its transcript, written as
`<result_dir>/<audio>.<ctm|ali|json>`.  --score also writes `<result_dir>/<audio>.score.json`: the full-sum CTC log-likelihood of
the transcript (the reference's bin/get_loss.py reports its negative as loss_ctc); with --attention that file also carries the
attention decoders' loss_att and acc_att and the combined loss.  --wildcard TOKEN marks, in the transcript, audio that nobody
transcribed: the aligner gives each marker the frames the rest of the transcript does not explain (at least one), and the marker
shows up in the result as a word / label / token of its own.  --alternatives reads choices and optional words in the transcript,
`it is {twenty|two zero} [um] goodbye`, and aligns the reading that was spoken; with --graph_score, `<audio>.score.json` holds the
full-sum log-likelihood over ALL readings and the probability of every word run of the transcript.  A file of more than --max_chunks
chunks, or a transcript of more than 16 383 tokens, is aligned over several device batches with a windowed lattice (--long_form forces
it, --window_tokens N sets the window; ReverbASR.align).  --score and --posteriors go with the long form too: the score file then
holds the windowed full-sum score (ReverbASR.score's long path) with the per-token posteriors, and the alignment file is written
without them; --graph_score and --attention stay within one device batch, and so does --alternatives unless --long_graph asks for
the windowed graph alignment (--window_nodes N sets its window; any number of chunks and graph nodes); --long_graph_score does
that and also writes the windowed full-sum score over all readings to `<audio>.score.json` (ReverbASR.score's long graph path).  Praat .lab / TextGrid output (--gen_praat there) is not written."""
from __future__ import annotations

import argparse
import json
import logging
import os
from pathlib import Path


def get_args(argv=None, long_score=False):
    """long_score=False is the parser's contract for its callers since the long form exists: --long_form / --window_tokens go with
    the alignment alone.  The tool itself (main) passes True: --score and --posteriors then go with them too (ReverbASR.score's long
    path); --alternatives, --graph_score and --attention stay within one device batch either way."""
    p = argparse.ArgumentParser(description="align a transcript with your model")
    p.add_argument("--model", default=None, help="reverb model name or a directory with config.yaml and a .pt file")
    p.add_argument("--config", default=None, help="config file")
    p.add_argument("--checkpoint", default=None, help="checkpoint model")
    p.add_argument("--audio_file", required=True, help="audio the transcript belongs to")
    p.add_argument("--transcript_file", required=True, help="text file with the transcript of the whole audio")
    p.add_argument("--result_dir", required=True, help="directory of the result file")
    p.add_argument("--format", default="ctm", choices=["ctm", "ali", "json"], help="word CTM, the reference's label line, or per-token JSON")
    p.add_argument("--gpu", type=int, default=-1, help="gpu id for this rank, -1 means device 0")
    p.add_argument("--chunk_size", type=int, default=2051, help="Chunk size")
    p.add_argument("--verbatimicity", type=float, default=1.0, help="the level of verbatimicity to run the model")
    p.add_argument("--timings_adjustment", type=float, default=230, help="time shift applied to all timings (ms)")
    p.add_argument("--log_level", default="INFO", help="log level")
    p.add_argument("--dtype", default="bf16", choices=["bf16", "f32"], help="device compute mode")
    p.add_argument("--max_chunks", type=int, default=64, help="chunks per device batch: at least the chunks of the file")
    p.add_argument("--score", action="store_true", help="also write <audio>.score.json: full-sum CTC log-likelihood of the transcript")
    p.add_argument("--posteriors", action="store_true",
                   help="per-token occupancy, mean_time and peak_posterior in --format json and in the --score file")
    p.add_argument("--attention", action="store_true",
                   help="with --score: also loss_ctc, loss_att, acc_att, loss and att_logp of the attention decoders (audio of one chunk)")
    p.add_argument("--wildcard", default=None, metavar="TOKEN",
                   help="a marker in the transcript, such as '<star>', that stands for audio left untranscribed")
    p.add_argument("--wildcard_bias", type=float, default=0.0,
                   help="penalty (<= 0, nats per frame) on wildcard frames: the misfit above which a marker is preferred to the transcript")
    p.add_argument("--alternatives", action="store_true",
                   help="the transcript holds choices {a|b c|} and optional words [x]: align the reading that was spoken")
    p.add_argument("--graph_score", action="store_true",
                   help="with --alternatives (no --wildcard): also write <audio>.score.json, the full-sum score over all readings and "
                        "the probability, occupancy and mean_time of every word run")
    p.add_argument("--reverse_weight", type=float, default=None, help="weight of the right-to-left decoder in loss_att (default: the config's)")
    p.add_argument("--long_form", action="store_true",
                   help="align over several device batches with a windowed lattice (taken by itself when the file has more than "
                        "--max_chunks chunks or more than 16383 tokens)")
    p.add_argument("--window_tokens", type=int, default=None, metavar="N",
                   help="long form: tokens of the transcript alive at a frame (default and most: 16384); the json result carries "
                        "window_margin, how close the path came to the window's edge")
    p.add_argument("--long_graph", action="store_true",
                   help="with --alternatives: align over several device batches with a windowed graph lattice (never taken by itself)")
    p.add_argument("--window_nodes", type=int, default=None, metavar="N",
                   help="with --long_graph: graph nodes alive at a frame (default and most: 8192); the json result carries "
                        "window_margin, how close the path came to the window's edge")
    p.add_argument("--long_graph_score", action="store_true",
                   help="with --alternatives (no --wildcard): the windowed graph alignment of --long_graph, and <audio>.score.json with "
                        "the windowed full-sum score over all readings and the probability, occupancy and mean_time of every word run "
                        "(--window_nodes: at most 4096 here; the file is encoded three times)")
    args = p.parse_args(argv)
    if (args.long_form or args.window_tokens is not None) and (args.alternatives or args.graph_score or args.attention):
        p.error("--long_form / --window_tokens: --alternatives, --graph_score and --attention stay within one device batch "
                "(a transcript with alternatives is aligned over several batches by --long_graph)")
    if args.long_graph and not args.alternatives:
        p.error("--long_graph aligns a transcript with alternatives: it needs --alternatives")
    if args.long_graph and (args.graph_score or args.score or args.posteriors or args.attention):
        p.error("--long_graph: --graph_score, --score, --posteriors and --attention stay within one device batch")
    if args.long_graph_score and not args.alternatives:
        p.error("--long_graph_score scores a transcript with alternatives: it needs --alternatives")
    if args.long_graph_score and (args.wildcard is not None or args.attention or args.score or args.graph_score):
        p.error("--long_graph_score: the windowed full sum over a graph has no gaps (--wildcard) and no attention loss (--attention), "
                "and is neither --score nor --graph_score")
    if args.window_nodes is not None and not (args.long_graph or args.long_graph_score):
        p.error("--window_nodes goes with --long_graph")
    if args.window_nodes is not None and args.window_nodes < 1:
        p.error("--window_nodes must be at least 1")
    if (args.long_form or args.window_tokens is not None) and (args.score or args.posteriors) and not long_score:
        p.error("--long_form / --window_tokens: --score, --posteriors and --alternatives stay within one device batch")
    if args.window_tokens is not None and args.window_tokens < 1:
        p.error("--window_tokens must be at least 1")
    if args.wildcard is not None and (args.score or args.posteriors):
        p.error("--wildcard: the full-sum score (--score, --posteriors) is not defined for a transcript with gaps")
    if args.alternatives and (args.score or args.posteriors):
        p.error("--alternatives: the full-sum score (--score, --posteriors) is not defined for a transcript with alternatives")
    if args.graph_score and not args.alternatives:
        p.error("--graph_score scores a transcript with alternatives: it needs --alternatives")
    if args.graph_score and args.wildcard is not None:
        p.error("--graph_score: the full-sum score is not defined for a transcript with gaps (--wildcard)")
    if args.graph_score and args.attention:
        p.error("--graph_score: the attention decoders' loss (--attention) is defined for one token sequence, not for alternatives")
    if not args.wildcard_bias <= 0:
        p.error("--wildcard_bias must be <= 0")
    return args


def main(argv=None):
    args = get_args(argv, long_score=True)
    logging.basicConfig(level=getattr(logging, str(args.log_level).upper(), logging.INFO),
                        format="%(asctime)s %(levelname)s %(message)s")
    from reverb_amd.reverb import ReverbASR, load_model
    if (args.model is not None) == (args.checkpoint is not None and args.config is not None):
        raise RuntimeError("One of either --model or (--checkpoint and --config) must be set.")
    if args.model:
        reverb = load_model(args.model, gpu=args.gpu, dtype=args.dtype, max_chunks=args.max_chunks)
    else:
        reverb = ReverbASR(args.config, args.checkpoint, gpu=args.gpu, dtype=args.dtype, max_chunks=args.max_chunks)
    with open(args.transcript_file, encoding="utf-8") as f:
        transcript = " ".join(f.read().split())
    long_graph = args.long_graph or args.long_graph_score
    long_form = True if args.long_form or args.window_tokens is not None or long_graph else None
    out = reverb.align(args.audio_file, transcript=transcript, format=args.format, verbatimicity=args.verbatimicity,
                       chunk_size=args.chunk_size, timings_adjustment=args.timings_adjustment,
                       posteriors=args.posteriors and args.format == "json" and not long_form, wildcard=args.wildcard,
                       wildcard_bias=args.wildcard_bias, alternatives=args.alternatives,
                       window_tokens=args.window_nodes if long_graph else args.window_tokens, long_form=long_form)
    if args.format == "json":
        out = json.dumps(out, ensure_ascii=False, indent=1)
    os.makedirs(args.result_dir, exist_ok=True)
    path = os.path.join(args.result_dir, Path(args.audio_file).with_suffix("." + args.format).name)
    with open(path, "w", encoding="utf-8") as f:
        f.write(out)
    logging.info("wrote %s", path)
    if args.score or args.graph_score or args.long_graph_score:
        graph_score = args.graph_score or args.long_graph_score
        sc = reverb.score(args.audio_file, transcript=transcript, verbatimicity=args.verbatimicity, chunk_size=args.chunk_size,
                          posteriors=args.posteriors or graph_score, attention=args.attention, reverse_weight=args.reverse_weight,
                          alternatives=graph_score, window_tokens=args.window_nodes if args.long_graph_score else args.window_tokens,
                          long_form=long_form)
        path = os.path.join(args.result_dir, Path(args.audio_file).with_suffix(".score.json").name)
        with open(path, "w", encoding="utf-8") as f:
            f.write(json.dumps(sc, ensure_ascii=False, indent=1))
        logging.info("wrote %s", path)


if __name__ == "__main__":
    main()
