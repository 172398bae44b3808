"""Drop-in for the reference's Python API of the recognize_wav hot path
(`asr/wenet/cli/reverb.py`): `load_model`, `ReverbASR`, `get_available_models`, `download_model`
with the same signatures, keyword names and defaults -- compute goes to librvb's HIP kernels.

Differences a caller can observe (all supersets):
  * `ReverbASR(..., gpu=N)` / `load_model(model, gpu=N, dtype=...)`: the engine always runs on an
    MI355X (there is no CPU path); `gpu < 0` means device 0.
  * `transcribe(mode="ctc_greedy_search")` returns text/CTM (the reference raises, A1).
  * chunks are batched on the device; `batch_size` keeps its meaning for `feats_batcher` but does
    not limit the device batch (chunks are independent, reverb.py:148-180, so results are equal).
"""
from __future__ import annotations

import logging
import os
import shutil
from functools import partial
from itertools import chain
from math import ceil
from pathlib import Path
from typing import Generator, List, Optional, Tuple

import numpy as np

from .ctc_align import adjust_model_time_offset, ctc_align, hyps_to_ctm, hyps_to_txt
from .engine import Engine, SUPPORTED_MODES, joint_topk
from .search import DecodeResult
from .tokenizer import RevBpeTokenizer
from . import audio

ALIGN_MAX_TOKENS = 16383          # RVB_CTC_ALIGN_MAX_TOKENS: what one workgroup's lattice holds; above it align() takes the long path
_FRAME_DOWNSAMPLING_FACTOR = {"linear": 1, "conv2d": 4, "conv2d6": 6, "conv2d8": 8}
CACHED_MODELS_DIR = Path.home() / ".cache/reverb"
_MODELS = {"reverb_asr_v1": "https://huggingface.co/Revai/reverb-asr"}


def _torch():
    import torch
    return torch


class RvbASRModel:
    """Stands where the reference keeps `ASRModel` (`ReverbASR.model`): same `decode` seam
    (asr/wenet/transformer/asr_model.py:331-350), backed by the device engine."""

    def __init__(self, engine: Engine):
        self.engine = engine
        self.lsl_enc = self.lsl_dec = engine.cfg.num_langs > 0

    def eval(self):
        return self

    def to(self, *_a, **_k):
        return self

    def sos_symbol(self):
        return self.engine.cfg.sos_id

    def eos_symbol(self):
        return self.engine.cfg.eos_id

    def decode(self, methods: List[str], speech, speech_lengths, beam_size: int, decoding_chunk_size: int = -1,
               num_decoding_left_chunks: int = -1, ctc_weight: float = 0.0, simulate_streaming: bool = False,
               reverse_weight: float = 0.0, context_graph=None, blank_id: int = 0, blank_penalty: float = 0.0,
               length_penalty: float = 0.0, infos=None, cat_embs=None, cv=None, cv_lengths=None):
        assert speech.shape[0] == speech_lengths.shape[0]
        assert decoding_chunk_size != 0
        # search.py:124-248: the graph biases ctc_prefix_beam_search and what attention_rescoring rescores; None decodes unbiased
        self.engine.set_context_graph(context_graph)
        if blank_id != self.engine.cfg.blank_id:
            raise ValueError("blank_id differs from the model's ctc_blank_id")
        feats = speech.detach().cpu().numpy() if hasattr(speech, "detach") else np.asarray(speech)
        lens = speech_lengths.detach().cpu().numpy() if hasattr(speech_lengths, "detach") else np.asarray(speech_lengths)
        if cat_embs is not None:
            cat = cat_embs.detach().cpu().numpy() if hasattr(cat_embs, "detach") else np.asarray(cat_embs)
            cat = np.asarray(cat, dtype=np.float32)
            if cat.ndim == 2:
                # per-utterance language weights (encoder_layer.py:378-390, decoder_layer.py: `cat_embs[:, i]` scales layer i's output
                # of batch item b): the engine folds ONE weight vector into its language-specific layers (W = sum_i c_i W_i), so the
                # batch is decoded group by group, one group per distinct row, and the results go back in the caller's order
                if cat.shape[0] != feats.shape[0]:
                    raise ValueError(f"cat_embs has {cat.shape[0]} rows for a batch of {feats.shape[0]}")
                kw = dict(decoding_chunk_size=decoding_chunk_size, num_decoding_left_chunks=num_decoding_left_chunks, ctc_weight=ctc_weight,
                          simulate_streaming=simulate_streaming, reverse_weight=reverse_weight, context_graph=context_graph, blank_id=blank_id,
                          blank_penalty=blank_penalty, length_penalty=length_penalty)
                rows, groups = {}, []
                for b in range(cat.shape[0]):
                    key = cat[b].tobytes()
                    if key not in rows:
                        rows[key] = len(groups)
                        groups.append([])
                    groups[rows[key]].append(b)
                merged = {}
                for idx in groups:
                    part = self.decode(methods, feats[idx], lens[idx], beam_size, cat_embs=cat[idx[0]], **kw)
                    for m, res in part.items():
                        slot = merged.setdefault(m, [None] * cat.shape[0])
                        for b, r in zip(idx, res):
                            slot[b] = r
                return merged
            self.engine.set_cat_embs(cat)
        results = {}
        if simulate_streaming and decoding_chunk_size > 0:
            # asr_model.py:301-306: the encoder runs chunk by chunk with attention caches (encoder.py:343-402) on the whole
            # (zero padded) input, lengths are not consulted and every output frame is valid.  The reference's call leaves
            # cat_embs out, which its language-specific layers refuse (encoder_layer.py:379); here the embeddings set on
            # the engine apply, and each item of the batch is its own stream (the reference asserts batch 1).
            for b in range(feats.shape[0]):
                self.engine.forward_chunk_by_chunk(feats[b], decoding_chunk_size, num_decoding_left_chunks, return_output=False)
                self.engine.stream_finish(beam_size, blank_penalty, topk=joint_topk(methods, beam_size))
                part = self.engine.search(methods, ctc_weight, reverse_weight, length_penalty)
                for k, v in part.items():
                    results.setdefault(k, []).extend(v)
            return results
        self.engine.apply_decoding_chunk(decoding_chunk_size, num_decoding_left_chunks)
        mc = self.engine.cfg.max_chunks
        for s in range(0, feats.shape[0], mc):
            self.engine.encode(feats[s:s + mc], lens[s:s + mc], beam_size, blank_penalty, topk=joint_topk(methods, beam_size))
            part = self.engine.search(methods, ctc_weight, reverse_weight, length_penalty)
            for k, v in part.items():
                results.setdefault(k, []).extend(v)
        return results


class ReverbASR:
    def __init__(self, config, checkpoint, cmvn_path: str | None = None, tokenizer_symbols: str | None = None,
                 bpe_path: str | None = None, gpu: int = -1, overwrite_cmvn: bool = False, dtype: str = "bf16",
                 max_chunks: int = 64, context_path: str | None = None, context_score: float = 6.0):
        import yaml
        torch = _torch()
        self.jit = False
        self.device = torch.device("cuda", max(gpu, 0))
        self.checkpoint = checkpoint
        with open(config, "r") as fin:
            self.configs = yaml.load(fin, Loader=yaml.FullLoader)
        self.configs["cmvn_conf"]["cmvn_file"] = self._make_path_absolute(
            self.configs["cmvn_conf"]["cmvn_file"], cmvn_path)
        tc = self.configs["tokenizer_conf"]
        tc["symbol_table_path"] = self._make_path_absolute(tc["symbol_table_path"], tokenizer_symbols)
        tc["bpe_path"] = self._make_path_absolute(tc["bpe_path"], bpe_path)
        if self.configs.get("tokenizer", "rev_bpe") not in ("rev_bpe", "char", "bpe"):
            raise NotImplementedError(f"tokenizer {self.configs.get('tokenizer')!r} is not supported")
        self.tokenizer = RevBpeTokenizer(tc["bpe_path"], tc["symbol_table_path"], tc.get("non_lang_syms_path"),
                                         split_with_space=tc.get("split_with_space", False), full_config=tc)
        self.blank_id = self._blank_id()
        # cli/model.py:51-56: a list file of hot words, one phrase per line; cut with the model's own tokenizer
        self.context_graph = None
        if context_path is not None:
            from .context_graph import ContextGraph
            char = self.configs.get("tokenizer", "rev_bpe") == "char"
            self.context_graph = ContextGraph(context_path, self.tokenizer.symbol_table, None if char else tc["bpe_path"] or "",
                                              context_score)
        self.configs["output_dim"] = len(self.tokenizer.symbol_table)

        # weights: the checkpoint as torch.load reads it (utils/checkpoint.py:29-46, strict=False)
        sd = torch.load(checkpoint, map_location="cpu", mmap=False)
        if "model0" in sd and isinstance(sd["model0"], dict):
            sd = sd["model0"]
        if overwrite_cmvn or "encoder.global_cmvn.mean" not in sd:
            mean, istd = load_cmvn(self.configs["cmvn_conf"]["cmvn_file"], self.configs["cmvn_conf"]["is_json_cmvn"])
            sd = dict(sd)
            sd["encoder.global_cmvn.mean"] = torch.from_numpy(mean).float()
            sd["encoder.global_cmvn.istd"] = torch.from_numpy(istd).float()
        self._sd, self._dtype, self._gpu, self._max_chunks = sd, dtype, max(gpu, 0), max_chunks
        self.engine = Engine(self.configs, sd, dtype=dtype, device=max(gpu, 0), max_chunks=max_chunks)
        self.model = RvbASRModel(self.engine)
        self.test_conf = self.configs["dataset_conf"]
        self.input_frame_length = self.test_conf["fbank_conf"]["frame_shift"]
        self.output_frame_length = self.input_frame_length * _FRAME_DOWNSAMPLING_FACTOR.get(
            self.configs["encoder_conf"]["input_layer"], 4)

    # ------------------------------------------------------------------ helpers
    def _blank_id(self) -> int:
        cc = self.configs.setdefault("ctc_conf", {})
        table = self.tokenizer.symbol_table
        if "<blank>" in table:
            if "ctc_blank_id" in cc:
                assert cc["ctc_blank_id"] == table["<blank>"]
            else:
                cc["ctc_blank_id"] = table["<blank>"]
        else:
            assert "ctc_blank_id" in cc, "PLZ set ctc_blank_id in yaml"
        return cc["ctc_blank_id"]

    def _make_path_absolute(self, config_path, alternate_path: str | None = None) -> str:
        if alternate_path:
            return alternate_path
        if config_path is None:
            return None
        p = Path(config_path)
        if not p.is_absolute():
            p = Path(self.checkpoint).parent / p       # assumed adjacent to the checkpoint
        return p.as_posix()

    # ------------------------------------------------------------------ front end
    def _load_pcm(self, audio_file: str, resample_rate: int):
        """-> (channel 0 in the native sample format -- int16, or float32 holding `.to(torch.float)` of anything else --, its
        sample rate); WAVE and FLAC are decoded by librvb on the host, the engine resamples to 16 kHz on the device."""
        wave, rate = audio.load(audio_file, channel=0)
        logging.info(f"detected sample rate: {rate}")
        if resample_rate != 16000:
            raise NotImplementedError("the device front end is built for a 16 kHz model (resample_rate=16000)")
        return wave[0], rate                              # kaldi.fbank uses channel 0 (Appendix A8)

    def compute_feats(self, audio_file: str, resample_rate: int = 16000, num_mel_bins=23, frame_length=25,
                      frame_shift=10, dither=0.0):
        """(1, frames, num_mel_bins) float32 tensor.  With the model's own settings (80 / 25 / 10) the same features stay resident
        in HBM for the decode that follows; any other setting (the reference passes them straight to kaldi.fbank, and its own
        default is 23 bins) goes through the stand-alone `rvb_compute_feats`."""
        if dither != 0.0:
            raise NotImplementedError("dither is random noise: the device fbank computes dither = 0.0 (what the Reverb recipe uses)")
        self.engine.upload_pcm(*self._load_pcm(audio_file, resample_rate))
        if (num_mel_bins, frame_length, frame_shift) == (80, 25, 10):
            _, feats = self.engine.fbank(return_feats=True)
            return _torch().from_numpy(feats).unsqueeze(0)
        import ctypes as C
        from ._lib import check, fptr
        wave = np.ascontiguousarray(self.engine.waveform(), np.float32)       # 16 kHz, int16 scale (resampled on the device if needed)
        n = C.c_int64(0)
        lib, dev = self.engine.lib, int(getattr(self.engine, "device_index", 0) or 0)
        check(lib.rvb_compute_feats(dev, fptr(wave), wave.size, int(num_mel_bins), float(frame_length), float(frame_shift), None, C.byref(n)),
              "rvb_compute_feats")
        feats = np.empty((n.value, int(num_mel_bins)), np.float32)
        if n.value:
            check(lib.rvb_compute_feats(dev, fptr(wave), wave.size, int(num_mel_bins), float(frame_length), float(frame_shift), fptr(feats),
                                        C.byref(n)), "rvb_compute_feats")
        return _torch().from_numpy(feats).unsqueeze(0)

    def feats_batcher(self, infeats, chunk_size: int, batch_size: int) -> Generator[Tuple, None, None]:
        """Fixed-length, non-overlapping chunks; the last one is zero padded and length-masked."""
        torch = _torch()
        nbins = self.test_conf["fbank_conf"]["num_mel_bins"]
        per_batch = chunk_size * batch_size
        total = infeats.shape[1]
        for b in range(ceil(total / per_batch)):
            piece = infeats[:, b * per_batch: (b + 1) * per_batch, :]
            nchunks = ceil(piece.shape[1] / chunk_size)
            lens = torch.full((nchunks,), chunk_size, dtype=torch.int32)
            short = nchunks * chunk_size - piece.shape[1]
            if short > 0:
                lens[-1] -= short
                piece = torch.nn.functional.pad(piece, (0, 0, 0, short, 0, 0), mode="constant", value=0)
            yield piece.reshape(-1, chunk_size, nbins), lens

    # ------------------------------------------------------------------ transcription
    def transcribe_modes(self, audio_file, modes: List[str], format: str = "txt", verbatimicity: float = 1.0,
                         chunk_size: int = 2051, batch_size: int = 1, beam_size: int = 10,
                         decoding_chunk_size: int = -1, num_decoding_left_chunks: int = -1, ctc_weight: float = 0.1,
                         simulate_streaming: bool = False, reverse_weight: float = 0.0, blank_penalty: float = 0.0,
                         length_penalty: float = 0.0, timings_adjustment: float = 230, chunking: str = "fixed",
                         pause_search: Optional[int] = None, pause_smooth: int = 10) -> list[str]:
        """chunking="pauses": instead of every chunk_size frames the recording is cut where it is quietest within the pause_search
        frames (default chunk_size // 4) before each such boundary, the loudness smoothed over 2 * pause_smooth frames
        (Engine.pause_chunks; both defaults are unmeasured), and CTM times follow the pieces' own start frames."""
        _check_pause_args(chunking, simulate_streaming)
        fc = self.test_conf["fbank_conf"]
        if (fc["num_mel_bins"], fc["frame_length"], fc["frame_shift"]) != (80, 25, 10):
            raise NotImplementedError("the device fbank is built for 80 bins / 25 ms / 10 ms")
        if chunk_size < 7:
            raise ValueError("chunk_size must be at least 7 frames (Conv2dSubsampling4 needs 7 input frames, subsampling.py:201-226)")
        eng = self._engine_for_chunk(chunk_size)
        eng.upload_pcm(*self._load_pcm(audio_file, 16000))
        eng.set_cat_embs([verbatimicity, 1.0 - verbatimicity])
        eng.set_context_graph(self.context_graph)
        if simulate_streaming and decoding_chunk_size > 0:
            # the reference's loop (cli/reverb.py:220-253) with the encoder run chunk by chunk inside model.decode
            _, feats = eng.fbank(return_feats=True)
            hyps = {m: [] for m in modes}
            for x, lens in self.feats_batcher(_torch().from_numpy(feats).unsqueeze(0), chunk_size, batch_size):
                part = self.model.decode(modes, x, lens, beam_size, decoding_chunk_size, num_decoding_left_chunks, ctc_weight,
                                         True, reverse_weight, context_graph=self.context_graph, blank_id=self.blank_id,
                                         blank_penalty=blank_penalty, length_penalty=length_penalty)
                for m in modes:
                    hyps[m].extend(part[m])
            return [get_output(format, self.tokenizer, Path(audio_file).name, hyps[mode], timings_adjustment, chunk_size,
                               self.input_frame_length, self.output_frame_length) for mode in modes]
        eng.apply_decoding_chunk(decoding_chunk_size, num_decoding_left_chunks)
        n_frames = eng.fbank()
        hyps = self.decode_resident(n_frames, modes, chunk_size, beam_size, ctc_weight, reverse_weight, blank_penalty, length_penalty,
                                    chunking, pause_search, pause_smooth)
        hyps, starts = hyps if chunking == "pauses" else (hyps, None)
        return [get_output(format, self.tokenizer, Path(audio_file).name, hyps[mode], timings_adjustment, chunk_size,
                           self.input_frame_length, self.output_frame_length, chunk_starts=starts) for mode in modes]

    def align(self, audio_file, transcript: Optional[str] = None, tokens=None, format: str = "ctm", verbatimicity: float = 1.0,
              chunk_size: int = 2051, timings_adjustment: float = 230, posteriors: bool = False, wildcard: Optional[str] = None,
              wildcard_bias: float = 0.0, alternatives: bool = False, window_tokens: Optional[int] = None,
              long_form: Optional[bool] = None):
        """Forced alignment of a KNOWN transcript (the reference's bin/alignment.py -> force_align, utils/ctc_utils.py:105-161): exactly
        one of `transcript` (text, tokenised with the model's tokenizer) or `tokens` (ids).  The whole file is encoded as
        transcribe_modes does and the transcript aligned as ONE sequence over all chunks.  format: "ctm" / "txt" (through get_output,
        a token going to the chunk its first frame lies in), "ali" (the reference's `<audio> [labels]` line), "json" (dict: per-token
        times + score; with posteriors=True each token also carries occupancy, mean_time and peak_posterior of the full-sum
        posteriors, see score()).
        wildcard: a marker such as "<star>" that stands in `transcript` for audio nobody transcribed (hold music, cross-talk, a
        preamble before the first word).  The text is split at the marker, the pieces are tokenised as usual and joined with the
        wildcard label (consecutive markers are one); with tokens= the ids may hold ctc_align.WILDCARD.  A wildcard takes at least
        one frame and costs what the model's own best label costs there + wildcard_bias (<= 0) per frame; its run appears in every
        format with the marker as its text ("wildcard": true in json).  Full-sum posteriors do not exist for such a transcript.
        alternatives=True: `transcript` holds choices and optional words in the syntax of token_graph.parse_alternatives --
        "it is {twenty|two zero} [um] [<star>] goodbye" -- and ONE pass over the graph of all readings (Engine.align_graph) picks the
        reading that was spoken and aligns it.  [<star>] (with wildcard="<star>") is a gap marker that may be empty.  Every format
        shows the chosen reading; json adds "text" (that reading) and "node" (the graph node) per token.  tokens= is refused: a
        graph is written as text.  With posteriors=True (json, no wildcard in the text: the full-sum score has none) each token of the
        chosen path also carries its node's probability (Engine.score_graph's visit: the posterior of the readings through that
        node), occupancy, mean_time and peak_posterior of the full sum over ALL readings.
        Recordings of any length.  A file of at most max_chunks chunks and 16 383 tokens is aligned as one encoded batch, exactly.
        A longer one (long_form=None), or any file with long_form=True, takes the LONG path: the file is encoded batch by batch and
        ONE lattice continues over the batches (Engine.align_long_*), in which only a window of 2 window_tokens states (rounded up to
        256; default and most: 16 384 tokens = 32 768 states) is alive and follows the best partial path.  A window that holds
        the whole transcript gives the exact alignment; otherwise the result is the best path inside the windows, json carries
        "window_states" and "window_margin" (the path's smallest distance to a window edge, in states), and a margin below 64 logs
        a warning: align again with a larger window_tokens.  ctm and json encode the file a second time for the confidences.
        wildcard= works on the long path; posteriors=True stays one-batch (ValueError on a file that needs the long path).
        long_form=False insists on the one-batch path.
        alternatives=True with long_form=True takes the long GRAPH path (Engine.align_graph_long_*: a windowed graph Viterbi,
        csrc/ctc_graph_window.hip): a graph of any number of nodes, of which a window of window_tokens NODES (rounded up to 256;
        default and most: 8192) is alive.  json then carries "window_nodes", "window_margin" (in nodes) and "text".  It is never
        chosen silently: with long_form=None a file or a graph that does not fit one batch raises ValueError, which names
        long_form=True.  An arc that jumps over more than window / 2 - 64 nodes (a very long alternative) is refused by the engine:
        ask for a wider window."""
        from .ctc_align import WILDCARD, DecodeLike, align_to_ali, align_to_json, posteriors_to_json, split_by_chunk, split_transcript
        if (transcript is None) == (tokens is None):
            raise ValueError("align: give exactly one of transcript= (text) or tokens= (ids)")
        if format not in ("ctm", "txt", "ali", "json"):
            raise ValueError("Invalid output format.")
        fc = self.test_conf["fbank_conf"]
        if (fc["num_mel_bins"], fc["frame_length"], fc["frame_shift"]) != (80, 25, 10):
            raise NotImplementedError("the device fbank is built for 80 bins / 25 ms / 10 ms")
        if chunk_size < 7:
            raise ValueError("chunk_size must be at least 7 frames (Conv2dSubsampling4 needs 7 input frames, subsampling.py:201-226)")
        graph = None
        if alternatives:
            from .token_graph import parse_alternatives
            if tokens is not None:
                raise ValueError("align: alternatives=True takes transcript= (text)")
            try:
                graph = parse_alternatives(transcript, lambda text: self.tokenizer.tokenize(text)[1], wildcard, long_form=bool(long_form))
            except ValueError as e:
                if long_form is None and ("MAX_NODES" in str(e) or "MAX_ARCS" in str(e)):
                    raise ValueError(f"{e}: long_form=True aligns a graph of any size inside a moving window") from None
                raise
            if posteriors and WILDCARD in graph.tokens:
                raise ValueError("align: alternatives=True with a wildcard has no posteriors: the full-sum score has no wildcards")
            tokens = []                                       # nothing to tokenise below
        elif wildcard is not None:
            if posteriors:
                raise ValueError("align: posteriors come from the full-sum score, which has no wildcards")
            if tokens is None:
                tokens = split_transcript(transcript, wildcard, lambda text: self.tokenizer.tokenize(text)[1])
        if window_tokens is not None and int(window_tokens) < 1:
            raise ValueError("align: window_tokens must be at least 1")
        eng, ids, n_frames, n_chunks = self._prepare_for_align(audio_file, transcript, tokens, verbatimicity, chunk_size)
        fits = n_chunks <= eng.cfg.max_chunks and len(ids) <= ALIGN_MAX_TOKENS
        if long_form or (long_form is None and not fits):
            if posteriors or (alternatives and not long_form):
                raise ValueError("align: posteriors=True stays one-batch (full-sum scores do not span encoded batches) and "
                                 "alternatives=True takes the long path only when asked to: "
                                 f"the file has {n_chunks} chunks of {chunk_size} frames and {len(ids)} tokens, one "
                                 f"batch holds {eng.cfg.max_chunks} chunks and {ALIGN_MAX_TOKENS} tokens"
                                 + (" -- or drop long_form=True" if fits else " -- load the model with a larger max_chunks")
                                 + ("" if posteriors else ", or pass long_form=True for the windowed graph alignment"))
            if graph is not None:
                res, window, margin = self._align_graph_long(eng, graph, n_frames, n_chunks, chunk_size, window_tokens, wildcard_bias,
                                                             format in ("ctm", "json"))
                name = Path(audio_file).name
                if format == "ali":
                    return align_to_ali(name, res, wildcard)
                if format == "json":
                    out = align_to_json(res, self.tokenizer, chunk_size, self.input_frame_length, self.output_frame_length, wildcard)
                    out["text"] = graph.text_of(res.nodes)
                    out["window_nodes"], out["window_margin"] = window, margin
                    return out
                hyps = [DecodeLike(t, fr, cf, ends=en) for t, fr, cf, en in split_by_chunk(res, ends=True)]
                return get_output(format, self.tokenizer, name, hyps, timings_adjustment, chunk_size, self.input_frame_length,
                                  self.output_frame_length, wildcard=wildcard)
            res, window, margin = self._align_long(eng, ids, n_frames, n_chunks, chunk_size, window_tokens,
                                                   wildcard_bias if wildcard is not None else 0.0, format in ("ctm", "json"))
            name = Path(audio_file).name
            if format == "ali":
                return align_to_ali(name, res, wildcard)
            if format == "json":
                out = align_to_json(res, self.tokenizer, chunk_size, self.input_frame_length, self.output_frame_length, wildcard)
                out["window_states"], out["window_margin"] = window, margin
                return out
            hyps = [DecodeLike(t, fr, cf, ends=en) for t, fr, cf, en in split_by_chunk(res, ends=True)]
            return get_output(format, self.tokenizer, name, hyps, timings_adjustment, chunk_size, self.input_frame_length,
                              self.output_frame_length, wildcard=wildcard)
        n_chunks = self._encode_prepared("align", eng, n_frames, n_chunks, chunk_size)
        if graph is not None:
            res = eng.align_graph([graph], [(0, n_chunks)], wildcard_bias)[0]
        elif wildcard is None:
            res = eng.align([ids], [(0, n_chunks)])[0]
        else:
            res = eng.align_wild([ids], [(0, n_chunks)], wildcard_bias)[0]
        name = Path(audio_file).name
        if format == "ali":
            return align_to_ali(name, res, wildcard)
        if format == "json":
            out = align_to_json(res, self.tokenizer, chunk_size, self.input_frame_length, self.output_frame_length, wildcard)
            if graph is not None:
                out["text"] = graph.text_of(res.nodes)
            if posteriors and graph is not None:
                sg = eng.score_graph([graph], [(0, n_chunks)], posteriors=True)[0]
                on_path = {key: [sg[key][j] for j in res.nodes] for key in ("visit", "occupancy", "mean_frame", "peak_posterior")}
                for tok, extra, p in zip(out["tokens"], posteriors_to_json(res, on_path, chunk_size, self.input_frame_length,
                                                                           self.output_frame_length), on_path["visit"]):
                    tok.update(extra, probability=float(p))
            elif posteriors:
                post = eng.score([ids], [(0, n_chunks)], posteriors=True)[0]
                for tok, extra in zip(out["tokens"], posteriors_to_json(res, post, chunk_size, self.input_frame_length,
                                                                        self.output_frame_length)):
                    tok.update(extra)
            return out
        hyps = [DecodeLike(t, fr, cf, ends=en) for t, fr, cf, en in split_by_chunk(res, ends=True)]
        return get_output(format, self.tokenizer, name, hyps, timings_adjustment, chunk_size, self.input_frame_length,
                          self.output_frame_length, wildcard=wildcard)

    def _align_graph_long(self, eng: Engine, graph, n_frames: int, n_chunks: int, chunk_size: int, window_tokens, wildcard_bias: float,
                          need_emissions: bool):
        """The long path of align(alternatives=True): _align_long() for a token graph (Engine.align_graph_long_*: a windowed graph
        Viterbi, csrc/ctc_graph_window.hip) -> (AlignResult of the chosen reading over all chunks, window nodes, window margin)."""
        from .ctc_align import AlignResult
        mc = eng.cfg.max_chunks
        lens_all = np.full(n_chunks, chunk_size, np.int32)
        lens_all[-1] = n_frames - (n_chunks - 1) * chunk_size
        enc_all = np.where(lens_all > 6, (lens_all - 7) // 4 + 1, 0).astype(np.int32)      # Conv2dSubsampling4: frames 6 + 4j < len
        window = 0 if window_tokens is None else min(8192, -(-int(window_tokens) // 256) * 256)
        used = eng.align_graph_long_begin(graph, int(enc_all.sum()), window, wildcard_bias)

        def batches():
            for c0 in range(0, n_chunks, mc):
                eng.encode(None, lens_all[c0:c0 + mc], 1, 0.0, first_chunk=c0, T0=chunk_size)
                assert eng.encoder_lens().tolist() == enc_all[c0:c0 + mc].tolist(), "encoder frames differ from the subsampling arithmetic"
                yield int(enc_all[c0:c0 + mc].sum())

        try:
            for _ in batches():
                eng.align_graph_long_feed()
            labels, _, nodes, begin, end, score, margin = eng.align_graph_long_finish()
            peak, conf = begin.copy(), np.zeros(len(begin), np.float32)
            if need_emissions:
                f0, parts = 0, []
                for n in batches():
                    parts.append(eng.align_long_emissions(labels[f0:f0 + n]))
                    f0 += n
                emit = np.concatenate(parts)
                for k, (b, e) in enumerate(zip(begin, end)):                             # per run, as rvb_ctc_align_graph does: first maximum
                    peak[k] = b + int(np.argmax(emit[b:e + 1]))
                    conf[k] = np.exp(emit[peak[k]])
        finally:
            eng.align_graph_long_end()
        if margin < 64 and margin < used:
            logging.getLogger(__name__).warning(
                "align: the path came within %d nodes of the edge of its window of %d nodes; a better path may lie outside: "
                "align again with a larger window_tokens (now %d)", margin, used, used)
        nodes = nodes.tolist()
        res = AlignResult([graph.tokens[j] for j in nodes], labels.tolist(), begin.tolist(), end.tolist(), peak.tolist(), conf.tolist(),
                          score, 0, enc_all.tolist(), nodes)
        return res, used, margin

    def _align_long(self, eng: Engine, ids, n_frames: int, n_chunks: int, chunk_size: int, window_tokens, wildcard_bias: float,
                    need_emissions: bool):
        """The long path of align(): ONE lattice over the whole file, encoded batch by batch as find() does (Engine.align_long_*: a
        windowed Viterbi, csrc/ctc_viterbi_window.hip) -> (AlignResult over all chunks, window states, window margin).  Peaks and
        confidences need the log-prob of the chosen label at every frame, known only after the back-trace: the batches are then
        encoded a second time (need_emissions); without them peak = begin and confidence = 0."""
        from .ctc_align import AlignResult
        mc = eng.cfg.max_chunks
        lens_all = np.full(n_chunks, chunk_size, np.int32)
        lens_all[-1] = n_frames - (n_chunks - 1) * chunk_size
        enc_all = np.where(lens_all > 6, (lens_all - 7) // 4 + 1, 0).astype(np.int32)      # Conv2dSubsampling4: frames 6 + 4j < len
        window = 0 if window_tokens is None else min(32768, -(-2 * int(window_tokens) // 256) * 256)
        used = eng.align_long_begin(ids, int(enc_all.sum()), window, wildcard_bias)

        def batches():
            for c0 in range(0, n_chunks, mc):
                eng.encode(None, lens_all[c0:c0 + mc], 1, 0.0, first_chunk=c0, T0=chunk_size)
                assert eng.encoder_lens().tolist() == enc_all[c0:c0 + mc].tolist(), "encoder frames differ from the subsampling arithmetic"
                yield int(enc_all[c0:c0 + mc].sum())

        try:
            for _ in batches():
                eng.align_long_feed()
            labels, begin, end, score, margin = eng.align_long_finish()
            peak, conf = begin.copy(), np.zeros(len(begin), np.float32)
            if need_emissions:
                f0, parts = 0, []
                for n in batches():
                    parts.append(eng.align_long_emissions(labels[f0:f0 + n]))
                    f0 += n
                emit = np.concatenate(parts)
                for k, (b, e) in enumerate(zip(begin, end)):                             # per run, as rvb_ctc_align does: first maximum
                    peak[k] = b + int(np.argmax(emit[b:e + 1]))
                    conf[k] = np.exp(emit[peak[k]])
        finally:
            eng.align_long_end()
        if margin < 64 and margin < used:
            logging.getLogger(__name__).warning(
                "align: the path came within %d states of the edge of its window of %d states; a better path may lie outside: "
                "align again with a larger window_tokens (now %d)", margin, used, used // 2)
        res = AlignResult([int(t) for t in ids], labels.tolist(), begin.tolist(), end.tolist(), peak.tolist(), conf.tolist(), score, 0,
                          enc_all.tolist())
        return res, used, margin

    def _prepare_for_align(self, audio_file, transcript, tokens, verbatimicity: float, chunk_size: int):
        """Tokenise, upload and run the fbank -> (engine, ids, n_frames, n_chunks)."""
        ids = list(self.tokenizer.tokenize(transcript)[1]) if tokens is None else [int(t) for t in tokens]
        eng = self._engine_for_chunk(chunk_size)
        eng.upload_pcm(*self._load_pcm(audio_file, 16000))
        eng.set_cat_embs([verbatimicity, 1.0 - verbatimicity])
        eng.apply_decoding_chunk(-1, -1)
        n_frames = eng.fbank()
        return eng, ids, n_frames, -(-n_frames // chunk_size)

    def _encode_for_align(self, who: str, audio_file, transcript, tokens, verbatimicity: float, chunk_size: int):
        """Tokenise and encode the whole file as ONE batch, as align() and score() need it -> (engine, ids, n_chunks)."""
        eng, ids, n_frames, n_chunks = self._prepare_for_align(audio_file, transcript, tokens, verbatimicity, chunk_size)
        return eng, ids, self._encode_prepared(who, eng, n_frames, n_chunks, chunk_size)

    def _encode_prepared(self, who: str, eng: Engine, n_frames: int, n_chunks: int, chunk_size: int) -> int:
        if n_chunks > eng.cfg.max_chunks:
            raise ValueError(f"{who}: the file has {n_chunks} chunks of {chunk_size} frames, the engine batches {eng.cfg.max_chunks}: "
                             "one lattice spans one encoded batch -- load the model with max_chunks >= the file's chunks")
        lens = np.full(n_chunks, chunk_size, np.int32)
        lens[-1] = n_frames - (n_chunks - 1) * chunk_size
        eng.encode(None, lens, 1, 0.0, first_chunk=0, T0=chunk_size)
        return n_chunks

    def score(self, audio_file, transcript: Optional[str] = None, tokens=None, verbatimicity: float = 1.0, chunk_size: int = 2051,
              posteriors: bool = False, attention: bool = False, reverse_weight: Optional[float] = None, alternatives: bool = False,
              window_tokens: Optional[int] = None, long_form: Optional[bool] = None):
        """How likely a KNOWN transcript is under the model: the full-sum CTC log-likelihood, the negative of what the reference
        calls loss_ctc (CTC.forward, transformer/ctc.py:65-104; bin/get_loss.py), of the transcript as ONE sequence over the whole
        file, tokenised and encoded exactly as align() does.  -> dict: loglik, n_tokens, n_frames, loglik_per_token, viterbi_score
        (the best single path, from the align call: loglik >= viterbi_score) and, with posteriors=True, per token occupancy
        (expected frames), mean_time (ms, the frame -> ms conversion of align's json) and peak_posterior.  A transcript the frames
        cannot emit is refused, as by align(); the reference's zero_infinity would report loss 0.
        attention=True adds the other half of the reference's bin/get_loss.py: loss_ctc (= -loglik), loss_att and acc_att of the
        attention decoders (ASRModel._calc_att_loss, asr_model.py:248-286; reverse_weight defaults to the config's), loss =
        ctc_weight loss_ctc + (1 - ctc_weight) loss_att and att_logp (left decoder, per target, <eos> last) -- see Engine.score.  The
        decoder attends to ONE chunk's frames: audio that encodes to more than one chunk raises ValueError.
        alternatives=True: `transcript` holds choices and optional words in the syntax of token_graph.parse_alternatives (no wildcard)
        and ONE pass scores the graph of all readings (Engine.score_graph): loglik is the log of the summed likelihood of the
        readings -- "how well does this transcript fit, whichever way the numerals were read" -- where two readings that spell the
        same tokens both count.  -> dict: loglik, n_frames, viterbi_score and text (the best reading, from align(alternatives=True))
        and, with posteriors=True, words: one entry per node that opens a run of text, with text, node, probability (the posterior of
        the readings through that node; the branches of a choice, plus the skip of an optional one, sum to 1), occupancy and
        mean_time (None where the node holds no mass).  tokens= and attention=True are refused.
        A file of more chunks than the engine batches, or a transcript of more than 16 383 tokens, takes the LONG path (long_form=None:
        only then; True: always; False: never, such a file is refused): the file is encoded batch by batch and ONE full-sum lattice
        continues over the batches inside a window of 2 window_tokens states, as align()'s long path does (Engine.score_long_*,
        csrc/ctc_fb_window.hip); with posteriors=True the batches are encoded a second time, in reverse order, for the backward
        sweep.  The result then also holds window_states and window_margin (align's); loglik is the sum over the paths inside the
        windows, and a loglik below viterbi_score logs a warning: score again with a larger window_tokens.  attention=True is
        refused there.
        alternatives=True with long_form=True takes the long GRAPH path (Engine.score_graph_long_*: a windowed full sum over the
        graph, csrc/ctc_graph_fb_window.hip): a graph of any number of nodes, of which a window of window_tokens NODES (rounded up to
        256; default and most: 4096) is alive; pass 1 also runs the windowed graph Viterbi, and posteriors=True encodes the batches a
        second time in reverse order.  -> loglik, n_frames, viterbi_score, text, window_nodes, window_margin and, with posteriors,
        words as above.  It is never chosen silently: with long_form=None a file or a graph that does not fit one batch raises
        ValueError, which names long_form=True."""
        from .ctc_align import posteriors_to_json
        if window_tokens is not None and int(window_tokens) < 1:
            raise ValueError("score: window_tokens must be at least 1")
        if alternatives and (tokens is not None or attention):
            raise ValueError("score: alternatives=True takes transcript= (text) and has no attention loss")
        if (transcript is None) == (tokens is None):
            raise ValueError("score: give exactly one of transcript= (text) or tokens= (ids)")
        fc = self.test_conf["fbank_conf"]
        if (fc["num_mel_bins"], fc["frame_length"], fc["frame_shift"]) != (80, 25, 10):
            raise NotImplementedError("the device fbank is built for 80 bins / 25 ms / 10 ms")
        if chunk_size < 7:
            raise ValueError("chunk_size must be at least 7 frames (Conv2dSubsampling4 needs 7 input frames, subsampling.py:201-226)")
        if alternatives:
            from .token_graph import parse_alternatives
            try:
                graph = parse_alternatives(transcript, lambda text: self.tokenizer.tokenize(text)[1], None, long_form=bool(long_form))
            except ValueError as e:
                if long_form is None and ("MAX_NODES" in str(e) or "MAX_ARCS" in str(e)):
                    raise ValueError(f"{e}: long_form=True scores a graph of any size inside a moving window") from None
                raise
            eng, _, n_frames, n_chunks = self._prepare_for_align(audio_file, transcript, [], verbatimicity, chunk_size)
            if long_form:
                return self._score_graph_long(eng, graph, n_frames, n_chunks, chunk_size, window_tokens, posteriors)
            if long_form is None and n_chunks > eng.cfg.max_chunks:
                raise ValueError(f"score: alternatives=True takes the long path only when asked to: the file has {n_chunks} chunks of "
                                 f"{chunk_size} frames, one batch holds {eng.cfg.max_chunks} -- pass long_form=True for the windowed "
                                 "full sum over the graph, or load the model with a larger max_chunks")
            n_chunks = self._encode_prepared("score", eng, n_frames, n_chunks, chunk_size)
            res = eng.align_graph([graph], [(0, n_chunks)])[0]
            sg = eng.score_graph([graph], [(0, n_chunks)], posteriors=posteriors)[0]
            out = {"loglik": sg["loglik"], "n_frames": sg["n_frames"], "viterbi_score": float(res.score), "text": graph.text_of(res.nodes)}
            if posteriors:
                opens = [j for j in range(len(graph)) if graph.words[j] != ""]
                picked = {key: [sg[key][j] for j in opens] for key in ("occupancy", "mean_frame", "peak_posterior")}
                per = posteriors_to_json(res, picked, chunk_size, self.input_frame_length, self.output_frame_length)
                out["words"] = [{"text": graph.words[j], "node": j, "probability": float(sg["visit"][j]), "occupancy": p["occupancy"],
                                 "mean_time": p["mean_time"] if p["occupancy"] > 0 else None} for j, p in zip(opens, per)]
            return out
        eng, ids, n_frames, n_chunks = self._prepare_for_align(audio_file, transcript, tokens, verbatimicity, chunk_size)
        fits = n_chunks <= eng.cfg.max_chunks and len(ids) <= ALIGN_MAX_TOKENS
        if long_form or (long_form is None and not fits):
            if attention:
                raise ValueError("score: attention=True stays one-batch (the attention decoder's memory is one chunk): the long path "
                                 f"scores {n_chunks} chunks of {chunk_size} frames batch by batch"
                                 + (" -- drop long_form=True" if fits else ""))
            return self._score_long(eng, ids, n_frames, n_chunks, chunk_size, window_tokens, posteriors)
        if long_form is False and len(ids) > ALIGN_MAX_TOKENS:
            raise ValueError(f"score: long_form=False, but the transcript has {len(ids)} tokens and one batch's lattice holds {ALIGN_MAX_TOKENS}")
        n_chunks = self._encode_prepared("score", eng, n_frames, n_chunks, chunk_size)
        res = eng.align([ids], [(0, n_chunks)])[0]
        sc = eng.score([ids], [(0, n_chunks)], posteriors=posteriors)[0]
        out = {"loglik": sc["loglik"], "n_tokens": sc["n_tokens"], "n_frames": sc["n_frames"],
               "loglik_per_token": sc["loglik"] / sc["n_tokens"], "viterbi_score": float(res.score)}
        if posteriors:
            per = posteriors_to_json(res, sc, chunk_size, self.input_frame_length, self.output_frame_length)
            for key in ("occupancy", "mean_time", "peak_posterior"):
                out[key] = [p[key] for p in per]
        if attention:
            if n_chunks != 1:
                raise ValueError(f"score(attention=True): the audio encodes to {n_chunks} chunks of {chunk_size} frames; the attention "
                                 "decoder's memory is one chunk -- score shorter audio or raise chunk_size")
            att = eng.score([ids], [(0, 1)], attention=True, reverse_weight=reverse_weight)[0]
            for key in ("loss_ctc", "loss_att", "acc_att", "loss", "att_logp"):
                out[key] = att[key]
        return out

    def _score_graph_long(self, eng: Engine, graph, n_frames: int, n_chunks: int, chunk_size: int, window_tokens, posteriors: bool):
        """The long path of score(alternatives=True): pass 1 encodes the batches in order and feeds both the windowed graph Viterbi
        (viterbi_score, text and window_margin) and the windowed forward sweep over the graph (Engine.score_graph_long_*,
        csrc/ctc_graph_fb_window.hip); pass 2 (posteriors only) encodes them in reverse order for the backward sweep."""
        from .ctc_align import AlignResult, posteriors_to_json
        mc = eng.cfg.max_chunks
        lens_all = np.full(n_chunks, chunk_size, np.int32)
        lens_all[-1] = n_frames - (n_chunks - 1) * chunk_size
        enc_all = np.where(lens_all > 6, (lens_all - 7) // 4 + 1, 0).astype(np.int32)      # Conv2dSubsampling4: frames 6 + 4j < len
        window = 0 if window_tokens is None else min(4096, -(-int(window_tokens) // 256) * 256)
        total = int(enc_all.sum())

        def encode(c0):
            eng.encode(None, lens_all[c0:c0 + mc], 1, 0.0, first_chunk=c0, T0=chunk_size)
            assert eng.encoder_lens().tolist() == enc_all[c0:c0 + mc].tolist(), "encoder frames differ from the subsampling arithmetic"

        starts = list(range(0, n_chunks, mc))
        eng.align_graph_long_begin(graph, total, window or 4096, 0.0)      # the scorer's default window, not the aligner's own
        try:
            used = eng.score_graph_long_begin(graph, total, window, posteriors)
            for c0 in starts:
                encode(c0)
                eng.align_graph_long_feed()
                eng.score_graph_long_feed()
            labels, _, nodes, begin, end, vit, margin = eng.align_graph_long_finish()
            loglik = eng.score_graph_long_loglik()
            sg = None
            if posteriors:
                for c0 in reversed(starts):
                    encode(c0)
                    eng.score_graph_long_feed_back()
                sg = eng.score_graph_long_finish()
        finally:
            eng.align_graph_long_end()
            eng.score_graph_long_end()
        if loglik < vit - 1e-5 * total:
            logging.getLogger(__name__).warning(
                "score: loglik %.3f lies below viterbi_score %.3f: the scoring window of %d nodes lost the best path; "
                "score again with a larger window_tokens (now %d)", loglik, vit, used, used)
        nodes = nodes.tolist()
        out = {"loglik": loglik, "n_frames": total, "viterbi_score": float(vit), "text": graph.text_of(nodes), "window_nodes": used,
               "window_margin": margin}
        if sg is not None:
            res = AlignResult([graph.tokens[j] for j in nodes], labels.tolist(), begin.tolist(), end.tolist(), begin.tolist(),
                              [0.0] * len(begin), vit, 0, enc_all.tolist(), nodes)
            opens = [j for j in range(len(graph)) if graph.words[j] != ""]
            picked = {key: [sg[key][j] for j in opens] for key in ("occupancy", "mean_frame", "peak_posterior")}
            per = posteriors_to_json(res, picked, chunk_size, self.input_frame_length, self.output_frame_length)
            out["words"] = [{"text": graph.words[j], "node": j, "probability": float(sg["visit"][j]), "occupancy": p["occupancy"],
                             "mean_time": p["mean_time"] if p["occupancy"] > 0 else None} for j, p in zip(opens, per)]
        return out

    def _score_long(self, eng: Engine, ids, n_frames: int, n_chunks: int, chunk_size: int, window_tokens, posteriors: bool):
        """The long path of score(): pass 1 encodes the batches in order and feeds both the windowed Viterbi (viterbi_score and
        window_margin) and the windowed forward sweep; pass 2 (posteriors only) encodes them in reverse order for the backward sweep."""
        from .ctc_align import AlignResult, posteriors_to_json
        mc = eng.cfg.max_chunks
        lens_all = np.full(n_chunks, chunk_size, np.int32)
        lens_all[-1] = n_frames - (n_chunks - 1) * chunk_size
        enc_all = np.where(lens_all > 6, (lens_all - 7) // 4 + 1, 0).astype(np.int32)      # Conv2dSubsampling4: frames 6 + 4j < len
        window = 0 if window_tokens is None else min(32768, -(-2 * int(window_tokens) // 256) * 256)
        total = int(enc_all.sum())

        def encode(c0):
            eng.encode(None, lens_all[c0:c0 + mc], 1, 0.0, first_chunk=c0, T0=chunk_size)
            assert eng.encoder_lens().tolist() == enc_all[c0:c0 + mc].tolist(), "encoder frames differ from the subsampling arithmetic"

        starts = list(range(0, n_chunks, mc))
        eng.align_long_begin(ids, total, window, 0.0)
        try:
            used = eng.score_long_begin(ids, total, window, posteriors)
            for c0 in starts:
                encode(c0)
                eng.align_long_feed()
                eng.score_long_feed()
            labels, begin, end, vit, margin = eng.align_long_finish()
            loglik = eng.score_long_loglik()
            post = None
            if posteriors:
                for c0 in reversed(starts):
                    encode(c0)
                    eng.score_long_feed_back()
                post = eng.score_long_finish()
        finally:
            eng.align_long_end()
            eng.score_long_end()
        if loglik < vit - 1e-5 * total:
            logging.getLogger(__name__).warning(
                "score: loglik %.3f lies below viterbi_score %.3f: the scoring window of %d states lost the best path; "
                "score again with a larger window_tokens (now %d)", loglik, vit, used, used // 2)
        out = {"loglik": loglik, "n_tokens": len(ids), "n_frames": total, "loglik_per_token": loglik / len(ids),
               "viterbi_score": float(vit), "window_states": used, "window_margin": margin}
        if post is not None:
            res = AlignResult([int(t) for t in ids], labels.tolist(), begin.tolist(), end.tolist(), begin.tolist(),
                              [0.0] * len(begin), vit, 0, enc_all.tolist())
            per = posteriors_to_json(res, post, chunk_size, self.input_frame_length, self.output_frame_length)
            for key in ("occupancy", "mean_time", "peak_posterior"):
                out[key] = [p[key] for p in per]
        return out

    def find(self, audio_file, phrases: Optional[List[str]] = None, phrase_file: Optional[str] = None, min_score: float = -1.0,
             max_hits: int = 64, verbatimicity: float = 1.0, chunk_size: int = 2051, timings_adjustment: float = 230):
        """Where in the audio are these phrases spoken?  Exactly one of `phrases` (texts) or `phrase_file` (one phrase per line, empty
        lines skipped); each is cut into tokens as the hot words of a context list are (context_graph.tokenize_lines) and searched
        with Engine.find: every occurrence whose score per token is at least min_score (nats; 0 = the model's own best labels
        spell the phrase), overlapping occurrences of a phrase suppressed best first, at most max_hits per phrase and batch.
        The file is encoded batch by batch (the engine's max_chunks) and each batch searched as ONE sequence, its frames offset by
        the batches before it: a hit may straddle chunks, but an occurrence that straddles two BATCHES is not found.
        -> one dict per phrase: phrase, tokens, hits = [{start, end (seconds: start_frame and end_frame + 1 through the frame -> ms
        conversion of align's json, shifted earlier by up to timings_adjustment ms), start_frame, end_frame (within the file),
        score, score_per_token, confidence = exp(score_per_token)}] in order of time.  end is the end of the FIRST frame of the
        last token (token times inside a hit are not computed)."""
        from .context_graph import tokenize_lines
        if (phrases is None) == (phrase_file is None):
            raise ValueError("find: give exactly one of phrases= (texts) or phrase_file=")
        if phrase_file is not None:
            with open(phrase_file, encoding="utf-8") as f:
                phrases = [line.strip() for line in f if line.strip()]
        if not phrases:
            raise ValueError("find: no phrase given")
        fc = self.test_conf["fbank_conf"]
        if (fc["num_mel_bins"], fc["frame_length"], fc["frame_shift"]) != (80, 25, 10):
            raise NotImplementedError("the device fbank is built for 80 bins / 25 ms / 10 ms")
        if chunk_size < 7:
            raise ValueError("chunk_size must be at least 7 frames (Conv2dSubsampling4 needs 7 input frames, subsampling.py:201-226)")
        tc = self.configs["tokenizer_conf"]
        char = self.configs.get("tokenizer", "rev_bpe") == "char"
        ids = tokenize_lines(phrases, self.tokenizer.symbol_table, None if char else tc["bpe_path"] or "")
        for text, t in zip(phrases, ids):
            if not t:
                raise ValueError(f"find: the phrase {text!r} has no token in the model's table")
        eng = self._engine_for_chunk(chunk_size)
        eng.upload_pcm(*self._load_pcm(audio_file, 16000))
        eng.set_cat_embs([verbatimicity, 1.0 - verbatimicity])
        eng.apply_decoding_chunk(-1, -1)
        n_frames = eng.fbank()
        n_chunks = -(-n_frames // chunk_size)
        out = [{"phrase": text, "tokens": [int(x) for x in t], "hits": []} for text, t in zip(phrases, ids)]
        frame0 = 0                                            # encoder frames of the batches before this one
        for c0 in range(0, n_chunks, eng.cfg.max_chunks):
            nb = min(eng.cfg.max_chunks, n_chunks - c0)
            lens = np.full(nb, chunk_size, np.int32)
            if c0 + nb == n_chunks:
                lens[-1] = n_frames - (n_chunks - 1) * chunk_size
            eng.encode(None, lens, 1, 0.0, first_chunk=c0, T0=chunk_size)
            found = eng.find(ids, [(0, nb)], min_score, max_hits)
            for rec, t, per_seq in zip(out, ids, found):
                for h in per_seq[0]:
                    ec, et = self._chunk_frame(eng, h.end_frame)
                    start_ms = (c0 + h.chunk) * chunk_size * self.input_frame_length + h.frame_in_chunk * self.output_frame_length
                    end_ms = (c0 + ec) * chunk_size * self.input_frame_length + (et + 1) * self.output_frame_length
                    move = min(timings_adjustment, start_ms)
                    rec["hits"].append({"start": (start_ms - move) / 1000.0, "end": (end_ms - move) / 1000.0,
                                        "start_frame": frame0 + h.start_frame, "end_frame": frame0 + h.end_frame, "score": h.score,
                                        "score_per_token": h.score_per_token, "confidence": float(np.exp(h.score_per_token))})
            frame0 += int(eng.encoder_lens().sum())
        return out

    @staticmethod
    def _chunk_frame(eng: Engine, frame: int):
        """frame of the one sequence over the encoded batch -> (chunk, frame inside it)"""
        ends = np.cumsum(eng.encoder_lens())
        c = int(np.searchsorted(ends, frame, side="right"))
        return c, frame - (int(ends[c - 1]) if c else 0)

    def _engine_for_chunk(self, chunk_size: int) -> Engine:
        """The reference accepts any --chunk_size (cli/reverb.py:188, recognize_wav.py:66-70).  The engine sizes its
        positional tables and workspace for `chunk_frames` input frames per chunk: smaller chunks run on the same
        engine, a larger one rebuilds it once (weights are re-packed from the kept state dict)."""
        if chunk_size > self.engine.cfg.chunk_frames:
            cat = self.engine._cat
            chunks = max(1, self._max_chunks * self.engine.cfg.chunk_frames // chunk_size)     # same workspace budget
            self.engine.close()
            self.engine = Engine(self.configs, self._sd, dtype=self._dtype, device=self._gpu, max_chunks=chunks,
                                 chunk_frames=chunk_size, cat_embs=cat)
            self.model = RvbASRModel(self.engine)
        return self.engine

    def decode_resident(self, n_frames: int, modes, chunk_size: int, beam_size: int, ctc_weight: float,
                        reverse_weight: float, blank_penalty: float = 0.0, length_penalty: float = 0.0, chunking: str = "fixed",
                        pause_search: Optional[int] = None, pause_smooth: int = 10):
        return self.engine.decode_resident(n_frames, modes, chunk_size, beam_size, ctc_weight, reverse_weight,
                                           blank_penalty, length_penalty, chunking, pause_search, pause_smooth)

    def _item_duration(self, item) -> float:
        """seconds of one transcribe_modes_many item, from the file's header or the waveform's length"""
        if isinstance(item, (tuple, list)):
            return np.asarray(item[0]).size / float(item[1])
        with open(item, "rb") as f:                       # the whole file: a clipped image would probe as a shorter recording
            info = audio.probe_bytes(f.read())
        return info.frames / float(max(info.sample_rate, 1))

    def _load_item(self, item):
        if isinstance(item, (tuple, list)):
            wave = np.asarray(item[0])
            return (wave[0] if wave.ndim == 2 else wave), int(item[1])
        return self._load_pcm(item, 16000)

    def transcribe_modes_many(self, audio_files, modes: List[str], format: str = "txt", verbatimicity: float = 1.0,
                              chunk_size: int = 2051, batch_size: int = 1, beam_size: int = 10, decoding_chunk_size: int = -1,
                              num_decoding_left_chunks: int = -1, ctc_weight: float = 0.1, simulate_streaming: bool = False,
                              reverse_weight: float = 0.0, blank_penalty: float = 0.0, length_penalty: float = 0.0,
                              timings_adjustment: float = 230, group_seconds: float = 3600.0, load_threads: int = 8,
                              errors: str = "raise", chunking: str = "fixed", pause_search: Optional[int] = None,
                              pause_smooth: int = 10) -> list:
        """transcribe_modes for many recordings in one pass (the reference's bin/recognize.py decodes a data set in batches through
        the same model.decode): -> list[list[str]] indexed [recording][mode].  Items are paths or (waveform, sample_rate) pairs
        (mono int16, or float32 at int16 scale; the CTM name of a pair is its index in the list).  Output i is string-equal to
        transcribe_modes(audio_files[i], ...): every recording keeps its own frames, chunks and padding, so a recording without a
        frame gives "".  verbatimicity, the context graph and decoding_chunk_size apply to the whole call.
        Recordings are taken in order into groups of at most group_seconds of audio (plan_groups); a group costs one upload, one
        fbank launch and ceil(chunks / max_chunks) encodes, and while it decodes the next group's files are read and decoded on
        load_threads host threads (at most 16).  errors="raise": a file that cannot be read raises, naming it, before any decode of
        its group; "skip": its place in the result holds None and its name is logged.
        fp8 engines are allowed but outside the identity promise: their activation scales come from the first batch they see.
        chunking, pause_search, pause_smooth: as in transcribe_modes; every recording is cut on its own frames."""
        from concurrent.futures import ThreadPoolExecutor
        _check_pause_args(chunking, simulate_streaming)
        if simulate_streaming:
            raise NotImplementedError("transcribe_modes_many does not simulate streaming: use transcribe / transcribe_modes per file")
        if errors not in ("raise", "skip"):
            raise ValueError("errors must be 'raise' or 'skip'")
        fc = self.test_conf["fbank_conf"]
        if (fc["num_mel_bins"], fc["frame_length"], fc["frame_shift"]) != (80, 25, 10):
            raise NotImplementedError("the device fbank is built for 80 bins / 25 ms / 10 ms")
        if chunk_size < 7:
            raise ValueError("chunk_size must be at least 7 frames (Conv2dSubsampling4 needs 7 input frames, subsampling.py:201-226)")
        items = list(audio_files)
        out: list = [None] * len(items)
        if not items:
            return out
        eng = self._engine_for_chunk(chunk_size)
        eng.set_cat_embs([verbatimicity, 1.0 - verbatimicity])
        eng.set_context_graph(self.context_graph)
        eng.apply_decoding_chunk(decoding_chunk_size, num_decoding_left_chunks)

        def duration(item):
            try:
                return self._item_duration(item)
            except (OSError, ValueError, NotImplementedError) as e:
                return e
        with ThreadPoolExecutor(max_workers=max(1, min(int(load_threads), 16))) as pool:
            durations, bad = list(pool.map(duration, items)), set()
            for i, d in enumerate(durations):
                if isinstance(d, Exception):
                    if errors == "raise":
                        raise type(d)(f"{items[i]}: {d}") from None
                    logging.warning("skipping %s: %s", items[i], d)
                    bad.add(i)
                    durations[i] = 0.0
            groups = [[i for i in g if i not in bad] for g in plan_groups(durations, group_seconds)]
            groups = [g for g in groups if g]
            submit = lambda g: [pool.submit(self._load_item, items[i]) for i in g]
            pending = submit(groups[0]) if groups else []
            for k, g in enumerate(groups):
                futures, pending = pending, (submit(groups[k + 1]) if k + 1 < len(groups) else [])
                loaded = []
                for i, fut in zip(g, futures):
                    try:
                        loaded.append((i, fut.result()))
                    except (OSError, ValueError, NotImplementedError) as e:
                        if errors == "raise":
                            for p in pending:
                                p.cancel()
                            raise type(e)(f"{items[i]}: {e}") from None
                        logging.warning("skipping %s: %s", items[i], e)
                if not loaded:
                    continue
                eng.upload_batch([w for _, w in loaded])
                hyps = eng.decode_batch(modes, chunk_size, beam_size, ctc_weight, reverse_weight, blank_penalty, length_penalty,
                                        chunking, pause_search, pause_smooth)
                hyps, starts = hyps if chunking == "pauses" else (hyps, [None] * len(hyps))
                for (i, _), h, st in zip(loaded, hyps, starts):
                    name = str(i) if isinstance(items[i], (tuple, list)) else Path(items[i]).name
                    out[i] = [get_output(format, self.tokenizer, name, h[mode], timings_adjustment, chunk_size,
                                         self.input_frame_length, self.output_frame_length, chunk_starts=st) for mode in modes]
        return out

    def transcribe_many(self, audio_files, mode: str = "ctc_prefix_beam_search", **kwargs) -> list:
        """transcribe for many recordings in one pass -> list[str] (None for a skipped file): transcribe_modes_many with one mode."""
        return [None if r is None else r[0] for r in self.transcribe_modes_many(audio_files, [mode], **kwargs)]

    def transcribe(self, audio_file, mode: str = "ctc_prefix_beam_search", format: str = "txt",
                   verbatimicity: float = 1.0, chunk_size: int = 2051, batch_size: int = 1, beam_size: int = 10,
                   decoding_chunk_size: int = -1, num_decoding_left_chunks: int = -1, ctc_weight: float = 0.1,
                   simulate_streaming: bool = False, reverse_weight: float = 0.0, blank_penalty: float = 0.0,
                   length_penalty: float = 0.0, timings_adjustment: float = 230, chunking: str = "fixed",
                   pause_search: Optional[int] = None, pause_smooth: int = 10) -> str:
        return self.transcribe_modes(
            audio_file, modes=[mode], format=format, verbatimicity=verbatimicity, chunk_size=chunk_size,
            batch_size=batch_size, beam_size=beam_size, decoding_chunk_size=decoding_chunk_size,
            num_decoding_left_chunks=num_decoding_left_chunks, ctc_weight=ctc_weight,
            simulate_streaming=simulate_streaming, reverse_weight=reverse_weight, blank_penalty=blank_penalty,
            length_penalty=length_penalty, timings_adjustment=timings_adjustment, chunking=chunking, pause_search=pause_search,
            pause_smooth=pause_smooth)[0]


def _check_pause_args(chunking: str, simulate_streaming: bool):
    if chunking not in ("fixed", "pauses"):
        raise ValueError(f"chunking must be 'fixed' or 'pauses', not {chunking!r}")
    if chunking == "pauses" and simulate_streaming:
        raise NotImplementedError("chunking='pauses' cuts the whole recording's features: it does not go with simulate_streaming")


def plan_groups(durations, group_seconds: float) -> List[List[int]]:
    """Recordings, in order, into groups of at most group_seconds of audio: -> lists of indices, each index exactly once, order kept.
    A recording longer than the budget is a group of its own."""
    groups, cur, total = [], [], 0.0
    for i, d in enumerate(durations):
        d = float(d)
        if cur and total + d > group_seconds:
            groups.append(cur)
            cur, total = [], 0.0
        cur.append(i)
        total += d
    if cur:
        groups.append(cur)
    return groups


def load_cmvn(cmvn_file: str, is_json: bool):
    """mean / inverse std from accumulated statistics (asr/wenet/utils/cmvn.py:21-93)."""
    import json
    import math
    if is_json:
        with open(cmvn_file) as f:
            st = json.load(f)
        sums, sqs, count = st["mean_stat"], st["var_stat"], st["frame_num"]
    else:
        with open(cmvn_file) as f:
            arr = f.read().split()
        assert arr[0] == "[" and arr[-2] == "0" and arr[-1] == "]"
        dim = int((len(arr) - 4) / 2)
        sums = [float(x) for x in arr[1:dim + 1]]
        count = float(arr[dim + 1])
        sqs = [float(x) for x in arr[dim + 2:2 * dim + 2]]
    mean, istd = [], []
    for s, q in zip(sums, sqs):
        m = s / count
        var = max(q / count - m * m, 1.0e-20)
        mean.append(m)
        istd.append(1.0 / math.sqrt(var))
    return np.array(mean), np.array(istd)


def get_output(format: str, tokenizer, audio_name: str, hyps: List[DecodeResult], timings_adjustment_ms,
               chunk_size: int, input_frame_length: int, output_frame_length: int, wildcard: Optional[str] = None,
               chunk_starts: Optional[List[int]] = None) -> str:
    """DecodeResults of consecutive chunks -> one TXT / CTM string (cli/reverb.py:298-327).  wildcard: the marker that the words of
    wildcard tokens carry (forced alignment with gaps; such hyps also give `ends`).  chunk_starts: the first input frame of every
    chunk (chunking="pauses"): chunk k is shifted by chunk_starts[k] * input_frame_length ms; None: by k * chunk_size frames."""
    if chunk_starts is not None and len(chunk_starts) != len(hyps):
        raise ValueError(f"get_output: {len(chunk_starts)} chunk starts for {len(hyps)} chunks")
    if format == "txt":
        render, sep = hyps_to_txt, " "
    elif format == "ctm":
        render, sep = partial(hyps_to_ctm, audio_name), "\n"
    else:
        raise ValueError("Invalid output format.")
    lines, shift_ms = [], 0
    for k, hyp in enumerate(hyps):
        if chunk_starts is not None:
            shift_ms = int(chunk_starts[k]) * input_frame_length
        times = hyp.times if hyp.times is not None else hyp.ctc_frames
        if times is None:
            # `attention` mode carries no timestamps (search.py:357-360: DecodeResult(hyp.tolist())); the reference's
            # get_output then fails in ctc_align on len(None).  Text output does not need times; CTM cannot be written.
            if format != "txt":
                raise ValueError("this decoding mode produces no timestamps: use format='txt'")
            times = [0] * len(hyp.tokens)
        words = ctc_align(hyp.tokens, times, hyp.tokens_confidence, tokenizer, output_frame_length, shift_ms, wildcard,
                          getattr(hyp, "ends", None))
        words = adjust_model_time_offset(words, timings_adjustment_ms)
        shift_ms += chunk_size * input_frame_length
        lines.extend(list(render(words)))
    return sep.join(lines)


def load_model(model: str, gpu: int = -1, dtype: str = "bf16", max_chunks: int = 64, context_path: str | None = None,
               context_score: float = 6.0):
    """Loads a reverb model from a directory (config.yaml + *.pt) or by name (cli/reverb.py:330-363).  context_path: a list of hot
    words, one phrase per line, that ctc_prefix_beam_search / attention_rescoring are biased towards (context_score per token)."""
    if Path(model).exists():
        model_dir = Path(model)
        config_path = model_dir / "config.yaml"
        checkpoint_path = list(model_dir.glob("*.pt"))[0]
    elif model in _MODELS:
        model_dir = CACHED_MODELS_DIR / model
        config_path = model_dir / "config.yaml"
        checkpoint_path = model_dir / f"{model}.pt"
        if not (model_dir.exists() and config_path.exists() and checkpoint_path.exists()):
            CACHED_MODELS_DIR.parent.mkdir(exist_ok=True, parents=True)
            shutil.rmtree(model_dir, ignore_errors=True)
            download_model(_MODELS[model], model_dir)
    else:
        raise ValueError("Please specify a local path to a model or one of our pretrained models: "
                         f"{','.join(get_available_models())}")
    config_path, checkpoint_path = config_path.resolve(), checkpoint_path.resolve()
    logging.info(f"Loading the model with {config_path = } and {checkpoint_path = }")
    return ReverbASR(str(config_path), str(checkpoint_path), gpu=gpu, dtype=dtype, max_chunks=max_chunks, context_path=context_path,
                     context_score=context_score)


def get_available_models():
    return list(_MODELS.keys())


def download_model(url: str, root: str):
    """Clones the model repository at `url` into `root` (needs GitPython and network)."""
    from git import Repo
    Repo.clone_from(url, root)
