"""Loss and attention accuracy of a checkpoint on a list of utterances: what the reference's `asr/wenet/bin/get_loss.py` reports
(:186-305: `Executor.cv` over a data set, one LossStatistics line per data set and checkpoint appended to --jsonl_output), computed
by the engine: loss_ctc from the full-sum CTC score (rvb_ctc_score), loss_att and acc_att from the teacher-forced attention decoders
(rvb_attention_score), loss = ctc_weight loss_ctc + (1 - ctc_weight) loss_att with the weights of the config's model_conf.

    python -m reverb_amd.bin.get_loss --model <dir> --data_list utts.jsonl --jsonl_output out.jsonl [--gpu 0] [--reverse_weight W]
                                      [--batch_size N]

--data_list: one JSON object per line with `wav` (path) and `txt` (transcript), and optionally `key`.  Every utterance is encoded as
a chunk of its own, up to `max_chunks` (--batch_size) per encode, and scored against that chunk.  The decoder attends to one chunk's
frames, so an utterance longer than one chunk (--chunk_size frames) is skipped; skipped utterances (also: no tokens, fewer than 7
frames, a transcript the frames cannot emit) are counted and named in the final line.

Output, appended to --jsonl_output: one line per utterance (key, wav, n_tokens, n_frames, loss_ctc, loss_att, acc_att, loss) and a
final line with the reference's LossStatistics fields: dataset (base name of --data_list), checkpoint, loss, acc_att,
time_to_process, the six augmentation fields None, plus utterances / skipped.

How the totals differ from `Executor.cv` (utils/executor.py): that loop starts its utterance count at 1, so its loss is
sum(loss_b * batch_b) / (1 + utterances), and it averages acc_att per BATCH, whatever the batches' sizes.  Here `loss` is the plain
mean of the per-utterance losses (each the reference's loss for a batch of one) and `acc_att` is correct positions / positions over
the whole list, which does not depend on how the list is batched."""
from __future__ import annotations

import argparse
import json
import logging
import os
import time

import numpy as np


def get_args(argv=None):
    p = argparse.ArgumentParser(description="loss and attention accuracy of a model on a list of utterances")
    p.add_argument("--model", required=True, help="reverb model name or a directory with config.yaml and a .pt file")
    p.add_argument("--data_list", required=True, help="jsonl: one {\"wav\": path, \"txt\": transcript} per line")
    p.add_argument("--jsonl_output", required=True, help="output file, jsonl; appended to if it exists")
    p.add_argument("--gpu", type=int, default=-1, help="gpu id, -1 means device 0")
    p.add_argument("--reverse_weight", type=float, default=None, help="weight of the right-to-left decoder (default: the config's)")
    p.add_argument("--batch_size", type=int, default=16, help="utterances per encode (the engine's max_chunks)")
    p.add_argument("--chunk_size", type=int, default=2051, help="longest utterance in input frames")
    p.add_argument("--verbatimicity", type=float, default=1.0, help="the level of verbatimicity to run the model")
    p.add_argument("--dtype", default="bf16", choices=["bf16", "f32"], help="device compute mode")
    p.add_argument("--log_level", default="INFO", help="log level")
    return p.parse_args(argv)


def score_batch(asr, eng, batch, reverse_weight):
    """batch: [(entry, ids, feats)] -> per-utterance dicts (None where the engine refuses the transcript)."""
    T0 = max(f.shape[0] for _, _, f in batch)
    x = np.zeros((len(batch), T0, eng.cfg.input_dim), np.float32)
    lens = np.zeros(len(batch), np.int32)
    for b, (_, _, f) in enumerate(batch):
        x[b, :f.shape[0]] = f
        lens[b] = f.shape[0]
    eng.encode(x, lens, 1, 0.0)
    out = []
    for b, (entry, ids, _) in enumerate(batch):          # one call per utterance: a refusal concerns that utterance alone
        try:
            r = eng.score([ids], [(b, 1)], attention=True, reverse_weight=reverse_weight)[0]
        except Exception as exc:                          # RvbError by name: the frames cannot emit the transcript, ...
            logging.warning("skipped %s: %s", entry.get("key", entry["wav"]), exc)
            out.append(None)
            continue
        out.append({"key": entry.get("key", os.path.basename(entry["wav"])), "wav": entry["wav"], "n_tokens": r["n_tokens"],
                    "n_frames": r["n_frames"], "loss_ctc": r["loss_ctc"], "loss_att": r["loss_att"], "acc_att": r["acc_att"],
                    "loss": r["loss"]})
    return out


def main(argv=None):
    args = get_args(argv)
    logging.basicConfig(level=getattr(logging, str(args.log_level).upper(), logging.INFO),
                        format="%(asctime)s %(levelname)s %(message)s")
    from reverb_amd.reverb import load_model
    asr = load_model(args.model, gpu=args.gpu, dtype=args.dtype, max_chunks=max(1, args.batch_size))
    eng = asr._engine_for_chunk(args.chunk_size)
    eng.set_cat_embs([args.verbatimicity, 1.0 - args.verbatimicity])
    eng.apply_decoding_chunk(-1, -1)
    with open(args.data_list, encoding="utf-8") as f:
        entries = [json.loads(line) for line in f if line.strip()]
    t0 = time.perf_counter()
    rows, skipped, batch = [], [], []

    def flush():
        for entry, r in zip([b[0] for b in batch], score_batch(asr, eng, batch, args.reverse_weight)):
            if r is None:
                skipped.append(entry.get("key", entry["wav"]))
            else:
                rows.append(r)
        batch.clear()

    for entry in entries:
        ids = list(asr.tokenizer.tokenize(" ".join(entry["txt"].split()))[1])
        eng.upload_pcm(*asr._load_pcm(entry["wav"], 16000))
        n, feats = eng.fbank(return_feats=True)
        if not ids or n < 7 or n > args.chunk_size:
            logging.warning("skipped %s: %d tokens, %d frames (one chunk holds 7 .. %d)", entry.get("key", entry["wav"]), len(ids), n,
                            args.chunk_size)
            skipped.append(entry.get("key", entry["wav"]))
            continue
        batch.append((entry, ids, feats[:n].copy()))
        if len(batch) == eng.cfg.max_chunks:
            flush()
    if batch:
        flush()
    npos = sum(r["n_tokens"] + 1 for r in rows)
    correct = sum(round(r["acc_att"] * (r["n_tokens"] + 1)) for r in rows)
    total = {"dataset": os.path.basename(args.data_list), "checkpoint": str(asr.checkpoint),
             "loss": float(np.mean([r["loss"] for r in rows])) if rows else None, "acc_att": correct / npos if npos else None,
             "time_to_process": time.perf_counter() - t0, "loss_tel": None, "acc_att_tel": None, "loss_reverb": None,
             "acc_att_reverb": None, "loss_tel_reverb": None, "acc_att_tel_reverb": None, "utterances": len(rows), "skipped": skipped}
    os.makedirs(os.path.dirname(os.path.abspath(args.jsonl_output)), exist_ok=True)
    with open(args.jsonl_output, "a", encoding="utf-8") as f:
        for r in rows:
            f.write(json.dumps(r, ensure_ascii=False) + "\n")
        f.write(json.dumps(total, ensure_ascii=False) + "\n")
    logging.info("%s: loss %s acc_att %s over %d utterances (%d skipped) in %.2fs", total["dataset"], total["loss"], total["acc_att"],
                 len(rows), len(skipped), total["time_to_process"])
    return total


if __name__ == "__main__":
    main()
