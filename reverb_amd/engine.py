"""Python host of the librvb engine: loads a Reverb-ASR state dict into HBM through the C ABI
and exposes `ASRModel.decode`-shaped decoding (asr/wenet/transformer/asr_model.py:331-432).

PyTorch is used only to read `.pt` checkpoints; all compute is in librvb's HIP kernels."""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import _lib
from ._lib import ModelCfg, RvbError, check, dptr, fptr, iptr
from .search import DecodeResult

DTYPES = {"f32": _lib.RVB_F32, "fp32": _lib.RVB_F32, "float32": _lib.RVB_F32,
          "bf16": _lib.RVB_BF16, "bfloat16": _lib.RVB_BF16, "fp8": _lib.RVB_FP8}
SUPPORTED_MODES = ("attention", "ctc_greedy_search", "ctc_prefix_beam_search", "attention_rescoring", "joint_decoding")
JOINT_PRE_BEAM_RATIO = 1.5      # transformer/search.py:458


def model_cfg_from_configs(configs: dict, dtype: str, max_chunks: int, chunk_frames: int) -> ModelCfg:
    """config.yaml -> rvb_model_cfg; refuses the model families / options the hot path does not cover
     instead of silently computing something else."""
    ec, dc = configs["encoder_conf"], configs.get("decoder_conf", {})
    if configs.get("encoder", "conformer") != "conformer":
        raise RvbError(f"encoder {configs.get('encoder')!r} is not supported (Reverb-ASR is a conformer)")
    want = dict(input_layer="conv2d", pos_enc_layer_type="rel_pos", selfattention_layer_type="rel_selfattn",
                activation_type="swish", normalize_before=True, use_cnn_module=True, macaron_style=True)
    defaults = dict(input_layer="conv2d", pos_enc_layer_type="rel_pos", selfattention_layer_type="rel_selfattn",
                    activation_type="swish", normalize_before=True, use_cnn_module=True, macaron_style=True)
    for k, v in want.items():
        if ec.get(k, defaults[k]) != v:
            raise RvbError(f"encoder_conf.{k}={ec.get(k)!r} is not supported (need {v!r})")
    ds = configs.get("dataset_conf", {})
    lsl = bool(ds.get("pass_cat_emb", False))
    if ds.get("add_cat_emb", False):
        raise RvbError("dataset_conf.add_cat_emb is not supported")
    nlang = int(ds["cat_emb_conf"]["emb_len"]) if lsl else 0
    vocab = int(configs["output_dim"])
    blank = int(configs.get("ctc_conf", {}).get("ctc_blank_id", 0))
    cfg = ModelCfg()
    cfg.dtype = DTYPES[dtype]
    cfg.input_dim = int(configs["input_dim"])
    cfg.vocab = vocab
    cfg.d_model = int(ec["output_size"])
    cfg.heads = int(ec["attention_heads"])
    cfg.ffn_dim = int(ec["linear_units"])
    cfg.num_blocks = int(ec["num_blocks"])
    cfg.cnn_kernel = int(ec.get("cnn_module_kernel", 15))
    cfg.cnn_norm = 0 if ec.get("cnn_module_norm", "batch_norm") == "layer_norm" else 1
    cfg.cnn_causal = 1 if ec.get("causal", False) else 0          # convolution.py:55-57: left padding cnn_kernel-1 only
    cfg.num_langs = nlang
    cfg.dec_heads = int(dc.get("attention_heads", 4))
    cfg.dec_ffn_dim = int(dc.get("linear_units", 2048))
    cfg.dec_blocks = int(dc.get("num_blocks", 0))
    cfg.dec_r_blocks = int(dc.get("r_num_blocks", 0))
    cfg.blank_id = blank
    cfg.sos_id = vocab - 1
    cfg.eos_id = vocab - 1
    cfg.max_chunks = int(max_chunks)
    cfg.chunk_frames = int(chunk_frames)
    return cfg


def _check_chunking(chunking: str):
    if chunking not in ("fixed", "pauses"):
        raise ValueError(f"chunking must be 'fixed' or 'pauses', not {chunking!r}")


def joint_topk(methods, beam_size: int) -> Optional[int]:
    """CTC log-probs to keep per frame when `joint_decoding` is among the modes (its pre-beam), else None."""
    if "joint_decoding" not in methods:
        return None
    # the pre-beam itself + 8 more: log-probs that tie exactly with the pre-beam threshold are candidates too (the reference
    # compares the whole row, search.py / beam_search_timesync.py:268-270); the kernel keeps at most 64
    return min(int(JOINT_PRE_BEAM_RATIO * beam_size) + 8, 64)


def _as_numpy_f32(v) -> Optional[np.ndarray]:
    if hasattr(v, "detach"):          # torch tensor
        if not v.dtype.is_floating_point:
            return None
        v = v.detach().cpu().float().numpy()
    v = np.asarray(v)
    if v.dtype.kind != "f":
        return None
    return np.ascontiguousarray(v, dtype=np.float32)


class _PinnedBlock:
    """Owner of one rvb_host_alloc block: frees it when the last numpy view over it is garbage-collected."""

    def __init__(self, lib, ptr):
        self._free, self._ptr = lib.rvb_host_free, ptr

    def __del__(self):
        try:
            self._free(self._ptr)
        except Exception:
            pass


class Engine:
    """One librvb engine = one MI355X.  Not thread-safe (use one engine per thread/GPU)."""

    def __init__(self, configs: dict, state_dict, dtype: str = "bf16", device: int = 0, max_chunks: int = 64,
                 chunk_frames: int = 2051, cat_embs: Sequence[float] = (1.0, 0.0)):
        self.lib = _lib.load()
        self.configs = configs
        self.dtype = dtype
        self.cfg = model_cfg_from_configs(configs, dtype, max_chunks, chunk_frames)
        self.handle = C.c_void_p()
        self.device_index = int(device)
        check(self.lib.rvb_create(C.byref(self.cfg), int(device), C.byref(self.handle)), "rvb_create")
        if "model0" in state_dict and isinstance(state_dict["model0"], dict):     # checkpoint.py:38-41
            state_dict = state_dict["model0"]
        for name, value in state_dict.items():
            arr = _as_numpy_f32(value)
            if arr is None:
                continue                # e.g. BatchNorm num_batches_tracked
            shape = (C.c_int64 * max(arr.ndim, 1))(*arr.shape)
            check(self.lib.rvb_load_tensor(self.handle, name.encode(), fptr(arr), shape, arr.ndim), f"load {name}")
        self._cat = None
        self.set_cat_embs(cat_embs)
        self.batch = 0
        self.enc_frames = 0

    # -------------------------------------------------------------------------------- lifecycle
    def close(self):
        if getattr(self, "handle", None) is not None and self.handle:
            self.lib.rvb_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_cat_embs(self, cat_embs: Sequence[float]):
        """[verbatimicity, 1-verbatimicity] (cli/reverb.py:215-217): refolds the language-specific layers."""
        cat = np.ascontiguousarray(np.asarray(cat_embs, dtype=np.float32).reshape(-1))
        if self._cat is not None and np.array_equal(cat, self._cat):
            return
        n = self.cfg.num_langs
        if n and len(cat) != n:
            raise RvbError(f"cat_embs must have {n} entries")
        check(self.lib.rvb_finalize(self.handle, fptr(cat), len(cat) if n else 0), "rvb_finalize")
        self._cat = cat

    def set_context_graph(self, graph=None, context_score: Optional[float] = None):
        """Hot-word biasing of every later ctc_prefix_beam_search (and, through its n-best, attention_rescoring): `graph` is a
        reverb_amd.context_graph.ContextGraph or a list of token-id lists (then `context_score`, default 6.0, is the bonus per
        matched token); None clears it.  The graph stays on the engine until replaced (rvb_set_context_graph)."""
        if graph is None:
            check(self.lib.rvb_set_context_graph(self.handle, None, None, 0, 0.0), "rvb_set_context_graph")
            return
        if not hasattr(graph, "context_list"):
            from .context_graph import ContextGraph
            graph = ContextGraph.from_token_ids(graph, 6.0 if context_score is None else context_score)
        toks, lens = graph.flat()
        score = float(graph.context_score if context_score is None else context_score)
        check(self.lib.rvb_set_context_graph(self.handle, iptr(toks), iptr(lens), len(lens), score), "rvb_set_context_graph")

    # -------------------------------------------------------------------------------- front end
    def pinned_pcm(self, n_samples: int) -> np.ndarray:
        """int16 array of page-locked host memory (rvb_host_alloc) for the audio reader to fill: upload_pcm from it runs
        at the PCIe rate.  The memory lives exactly as long as the array (or any view of it): it is owned by the
        array's base object and released when the last view dies -- not by close(), so an array that outlives its
        engine (ReverbASR re-creates the engine for a larger chunk_size) stays valid."""
        p = C.c_void_p()
        check(self.lib.rvb_host_alloc(C.byref(p), int(n_samples) * 2), "rvb_host_alloc")
        buf = (C.c_int16 * max(int(n_samples), 1)).from_address(p.value)
        buf._rvb_owner = _PinnedBlock(self.lib, p)        # numpy keeps `buf` alive as the base of every view
        return np.ctypeslib.as_array(buf)[:int(n_samples)]

    def upload_pcm(self, pcm: np.ndarray, sample_rate: int = 16000):
        """Mono waveform -> HBM; other rates than 16 kHz are resampled on the device (reverb.py:128-134).  int16 PCM stays
        int16; a float32 array (the `.to(torch.float)` of a source whose native format is not int16) is uploaded as it is."""
        self._n_samples_next = None             # a synchronous upload replaces a pending upload_pcm_async
        self._batch_n = self._batch_plan = None # ... and a batch
        self._packed = False                    # ... and the pieces of pause_chunks
        if isinstance(pcm, np.ndarray) and pcm.dtype.kind == "f":
            wave = np.ascontiguousarray(pcm, dtype=np.float32).reshape(-1)
            check(self.lib.rvb_upload_wave_f32(self.handle, wave.ctypes.data_as(_lib._f32p), len(wave), int(sample_rate)),
                  "rvb_upload_wave_f32")
            n = C.c_int64(0)
            check(self.lib.rvb_get_waveform(self.handle, None, C.byref(n)), "rvb_get_waveform")
            self._n_samples = int(n.value)
            return
        pcm = np.ascontiguousarray(pcm, dtype=np.int16).reshape(-1)
        if sample_rate == 16000:
            check(self.lib.rvb_upload_pcm(self.handle, pcm.ctypes.data_as(_lib._i16p), len(pcm)), "rvb_upload_pcm")
            self._n_samples = len(pcm)
        else:
            check(self.lib.rvb_upload_pcm_rate(self.handle, pcm.ctypes.data_as(_lib._i16p), len(pcm), int(sample_rate)),
                  "rvb_upload_pcm_rate")
            n = C.c_int64(0)
            check(self.lib.rvb_get_waveform(self.handle, None, C.byref(n)), "rvb_get_waveform")
            self._n_samples = int(n.value)

    def upload_pcm_async(self, pcm: np.ndarray):
        """Double-buffered upload of the NEXT recording (16 kHz int16, ideally a pinned_pcm() array): returns at once, the copy
        runs underneath the decoding in progress, and the samples become the engine's audio at the next fbank().  `pcm` must
        not change until then."""
        assert isinstance(pcm, np.ndarray) and pcm.dtype == np.int16 and pcm.flags["C_CONTIGUOUS"]
        pcm = pcm.reshape(-1)
        check(self.lib.rvb_upload_pcm_async(self.handle, pcm.ctypes.data_as(_lib._i16p), len(pcm)), "rvb_upload_pcm_async")
        self._pending_pcm = pcm                 # keeps the host buffer alive until the copy has been consumed
        self._n_samples_next = len(pcm)

    def set_decoding_chunk(self, chunk_size: int = -1, num_left_chunks: int = -1):
        """Chunk mask of the encoder self-attention for the next encode() calls (<= 0: full context)."""
        check(self.lib.rvb_set_decoding_chunk(self.handle, int(chunk_size), int(num_left_chunks)), "rvb_set_decoding_chunk")

    FP8_GROUPS = {"ffn_macaron": 1, "qkv": 2, "pointwise_conv1": 4, "pointwise_conv2": 8, "ffn": 16, "subsample_conv2": 32}

    def set_fp8_policy(self, groups=None, first_block: int = 0, last_block: int = -1):
        """fp8 engines: the GEMM groups (names of FP8_GROUPS, or a bit mask) of blocks first_block..last_block that run on
        the fp8 MFMA path; None = the default (both feed-forward modules of every block)."""
        if groups is None:
            mask = -1
        elif isinstance(groups, int):
            mask = groups
        else:
            mask = sum(self.FP8_GROUPS[g] for g in set(groups))
        check(self.lib.rvb_set_fp8_policy(self.handle, int(mask), int(first_block), int(last_block)), "rvb_set_fp8_policy")

    def fp8_saturation(self, reset: bool = False) -> np.ndarray:
        """fp8 engines: values clipped at +-448 per (block, activation slot) -- [blocks, 7] in the order of fp8_scales() -- since
        the scales were calibrated / installed / last reset.  All zeros = the scales cover what was decoded."""
        n = C.c_int32(0)
        check(self.lib.rvb_get_fp8_saturation(self.handle, None, C.byref(n), 0), "rvb_get_fp8_saturation")
        out = np.zeros(max(n.value, 1), np.uint32)
        check(self.lib.rvb_get_fp8_saturation(self.handle, out.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(n), 1 if reset else 0),
              "rvb_get_fp8_saturation")
        return out[:n.value].reshape(-1, 7)

    def fp8_subsample(self, reset: bool = False):
        """fp8 engines with "subsample_conv2" in the policy: (scale of conv1's fp8 output -- 0.0 before the calibration batch --,
        values of it clipped at 448 * scale since the last reset)."""
        sc, cl = C.c_float(0.0), C.c_uint32(0)
        check(self.lib.rvb_get_fp8_subsample(self.handle, C.byref(sc), C.byref(cl), 1 if reset else 0), "rvb_get_fp8_subsample")
        return float(sc.value), int(cl.value)

    def fp8_scale_vector(self) -> Optional[np.ndarray]:
        """fp8 engines: EVERY calibrated activation scale as rvb_get_fp8_scales returns them -- 7 per conformer block, then the
        scale of conv1's fp8 output (policy group "subsample_conv2"; 0.0 = not measured) -- or None before the calibration
        batch.  This is the vector ranks of a sharded run exchange (dist.share_fp8_scales) and set_fp8_scales() installs."""
        n = C.c_int32(0)
        check(self.lib.rvb_get_fp8_scales(self.handle, None, C.byref(n)), "rvb_get_fp8_scales")
        if n.value == 0:
            return None
        out = np.empty(n.value, np.float32)
        check(self.lib.rvb_get_fp8_scales(self.handle, fptr(out), C.byref(n)), "rvb_get_fp8_scales")
        return out

    def fp8_scales(self) -> Optional[np.ndarray]:
        """fp8 engines: the calibrated activation scales of the conformer blocks [blocks, 7], or None before the calibration batch."""
        v = self.fp8_scale_vector()
        return None if v is None else v[:(v.size // 7) * 7].reshape(-1, 7)

    def set_fp8_scales(self, scales):
        """Install activation scales (e.g. the element-wise maximum over the ranks of a sharded run, or scales measured
        once): the engine counts as calibrated, the next encode runs in fp8.  Accepts [blocks, 7] (the subsampling scale is
        left as it is) or the whole fp8_scale_vector()."""
        a = np.ascontiguousarray(scales, dtype=np.float32).reshape(-1)
        check(self.lib.rvb_set_fp8_scales(self.handle, fptr(a), len(a)), "rvb_set_fp8_scales")

    def apply_decoding_chunk(self, decoding_chunk_size: int = -1, num_decoding_left_chunks: int = -1):
        """What BaseEncoder.forward does with these two arguments (encoder.py:140-145 -> add_optional_chunk_mask,
        utils/mask.py:126-197): they select a chunk mask only for models configured with use_dynamic_chunk, a
        static_chunk_size model is always chunk-masked, any other model ignores them."""
        ec = self.configs.get("encoder_conf", {})
        if ec.get("use_dynamic_chunk", False):
            if decoding_chunk_size > 0:
                self.set_decoding_chunk(decoding_chunk_size, num_decoding_left_chunks)
            else:
                self.set_decoding_chunk(-1, -1)
        elif int(ec.get("static_chunk_size", 0)) > 0:
            self.set_decoding_chunk(int(ec["static_chunk_size"]), num_decoding_left_chunks)
        else:
            self.set_decoding_chunk(-1, -1)

    def waveform(self) -> np.ndarray:
        """The waveform the fbank reads (float32, int16 scale; after resampling if any)."""
        out = np.empty(max(self._n_samples, 1), np.float32)
        n = C.c_int64(0)
        check(self.lib.rvb_get_waveform(self.handle, fptr(out), C.byref(n)), "rvb_get_waveform")
        return out[:int(n.value)]

    def fbank(self, return_feats: bool = False):
        """Kaldi fbank of the uploaded PCM; features stay resident in HBM.  Returns n_frames
        (and the (n_frames, 80) float32 array when asked)."""
        n = C.c_int64(0)
        out = None
        if getattr(self, "_n_samples_next", None) is not None:      # upload_pcm_async: this call makes those samples the audio
            self._n_samples, self._n_samples_next = self._n_samples_next, None
        if return_feats:
            out = np.empty((int(self.lib.rvb_num_frames(self._n_samples)), 80), np.float32)
        check(self.lib.rvb_fbank(self.handle, fptr(out), C.byref(n)), "rvb_fbank")
        self.n_frames = int(n.value)
        self._resident = [self.n_frames]        # frames per recording of the resident features (pause_chunks)
        self._packed = False
        return (self.n_frames, out) if return_feats else self.n_frames

    # -------------------------------------------------------------------------------- several recordings at once
    def upload_batch(self, items):
        """Several recordings resident together (rvb_upload_batch): items = [(waveform, sample_rate)], each mono int16 PCM or float32
        at int16 scale, at any rate upload_pcm takes.  Replaces whatever was uploaded before; fbank_batch() / decode_batch() follow.
        -> the 16 kHz lengths (after resampling)."""
        items = list(items)
        if not items:
            raise RvbError("upload_batch: at least one recording")
        waves = []
        for w, _ in items:
            w = np.asarray(w)
            waves.append(np.ascontiguousarray(w, np.float32 if w.dtype.kind == "f" else np.int16).reshape(-1))
        n = len(waves)
        data = (C.c_void_p * n)(*[w.ctypes.data for w in waves])
        fmt = np.array([4 if w.dtype == np.float32 else 2 for w in waves], np.int32)          # RVB_SAMPLE_F32 / RVB_SAMPLE_I16
        ns = np.array([len(w) for w in waves], np.int64)
        rate = np.array([int(r) for _, r in items], np.int32)
        self._n_samples_next = None
        self._batch_n = self._batch_plan = None
        self._packed = False
        check(self.lib.rvb_upload_batch(self.handle, data, iptr(fmt), ns.ctypes.data_as(_lib._i64p), iptr(rate), n), "rvb_upload_batch")
        out = np.empty(n, np.int64)
        check(self.lib.rvb_batch_n_samples(self.handle, out.ctypes.data_as(_lib._i64p)), "rvb_batch_n_samples")
        self._batch_n = out
        return out

    def batch_plan(self, n_samples, chunk_size: int):
        """rvb_batch_plan (host only): 16 kHz lengths -> (n_frames [n], first_chunk [n + 1], lens [chunks])."""
        ns = np.ascontiguousarray(n_samples, np.int64).reshape(-1)
        p64 = lambda a: a.ctypes.data_as(_lib._i64p)
        nf, first = np.empty(len(ns), np.int64), np.empty(len(ns) + 1, np.int64)
        check(self.lib.rvb_batch_plan(p64(ns), len(ns), int(chunk_size), p64(nf), p64(first), None), "rvb_batch_plan")
        lens = np.empty(int(first[-1]), np.int32)
        check(self.lib.rvb_batch_plan(p64(ns), len(ns), int(chunk_size), p64(nf), p64(first), iptr(lens)), "rvb_batch_plan")
        return nf, first, lens

    def fbank_batch(self, chunk_size: int, return_feats: bool = False):
        """Kaldi fbank of every recording of upload_batch() in one launch; recording r's frames start at row first_chunk[r] *
        chunk_size of the resident features and stop at its own last sample, the rest of its last chunk is zero.  -> (n_frames [n],
        first_chunk [n + 1]) and, when asked, the (first_chunk[n] * chunk_size, 80) float32 rows."""
        if getattr(self, "_batch_n", None) is None:
            n, ff = C.c_int64(0), C.c_int64(0)              # no batch: the library says which call is missing
            check(self.lib.rvb_fbank_batch(self.handle, int(chunk_size), None, C.byref(n), C.byref(ff)), "rvb_fbank_batch")
        p64 = lambda a: a.ctypes.data_as(_lib._i64p)
        nf, first, lens = self.batch_plan(self._batch_n, chunk_size)
        out = np.empty((int(first[-1]) * int(chunk_size), 80), np.float32) if return_feats else None
        check(self.lib.rvb_fbank_batch(self.handle, int(chunk_size), fptr(out), p64(nf), p64(first)), "rvb_fbank_batch")
        self._batch_plan = (int(chunk_size), nf, first, lens)
        self._resident = [int(x) for x in nf]
        self._packed = False
        return (nf, first, out) if return_feats else (nf, first)

    def pause_chunks(self, chunk_size: int, search: Optional[int] = None, smooth: int = 10, return_feats: bool = False):
        """Cut the resident features (after fbank() or fbank_batch()) at pauses instead of every chunk_size frames (rvb_pause_chunks;
        the definition is in include/rvb.h): each cut falls in the `search` frames before the fixed boundary (default chunk_size // 4),
        where the loudness summed over 2 * smooth frames is smallest.  -> (first_chunk [n_rec + 1], starts [chunks], lens [chunks])
        and, when asked, the packed (chunks * chunk_size, 80) rows: piece k of recording r is chunk first_chunk[r] + k, starts at
        frame starts[k] of its recording and has lens[k] frames.  encode(None, lens[a:b], ..., first_chunk=a, T0=chunk_size) reads the
        pieces until the next upload or fbank call.  Both defaults are unmeasured (docs/tuning-log.md)."""
        search = int(chunk_size) // 4 if search is None else int(search)
        res = getattr(self, "_resident", None) or [0]
        gap = max(int(chunk_size) - search, 1)
        cap = sum(-(-n // gap) for n in res) + 1
        first = np.zeros(len(res) + 1, np.int64)
        starts, lens = np.zeros(cap, np.int32), np.zeros(cap, np.int32)
        n = C.c_int64(0)
        p64 = lambda a: a.ctypes.data_as(_lib._i64p)
        out = None
        if return_feats:        # sized by a first call: the piece count is not known before the cuts are
            check(self.lib.rvb_pause_chunks(self.handle, int(chunk_size), search, int(smooth), p64(first), iptr(starts), iptr(lens), cap,
                                            C.byref(n), None), "rvb_pause_chunks")
            out = np.empty((int(n.value) * int(chunk_size), 80), np.float32)
        check(self.lib.rvb_pause_chunks(self.handle, int(chunk_size), search, int(smooth), p64(first), iptr(starts), iptr(lens), cap,
                                        C.byref(n), fptr(out)), "rvb_pause_chunks")
        k = int(n.value)
        self._packed = True
        return (first, starts[:k].copy(), lens[:k].copy()) + ((out,) if return_feats else ())

    def fixed_chunks(self):
        """Undo pause_chunks(): encode(None, ...) reads the frame-ordered features again (every upload and fbank call does the same)."""
        if getattr(self, "_packed", False):
            check(self.lib.rvb_fixed_chunks(self.handle), "rvb_fixed_chunks")
            self._packed = False

    def decode_batch(self, modes, chunk_size: int, beam_size: int, ctc_weight: float, reverse_weight: float,
                     blank_penalty: float = 0.0, length_penalty: float = 0.0, chunking: str = "fixed",
                     pause_search: Optional[int] = None, pause_smooth: int = 10):
        """decode_resident() over every chunk of the batch, `max_chunks` chunks per encode whichever recordings they belong to (a
        recording whose chunks fall into two encodes is the normal case) -> per recording {mode: [DecodeResult per chunk]}.
        chunking="pauses": the chunks are the pieces of pause_chunks(chunk_size, pause_search, pause_smooth), and the result is
        (that list, per recording the start frame of each of its pieces)."""
        if not 7 <= chunk_size <= self.cfg.chunk_frames:
            raise RvbError(f"resident decoding needs 7 <= chunk_size <= engine chunk_frames ({self.cfg.chunk_frames}); "
                           "ReverbASR rebuilds the engine for larger chunks")
        _check_chunking(chunking)
        plan = getattr(self, "_batch_plan", None)
        if plan is None or plan[0] != int(chunk_size):
            self.fbank_batch(chunk_size)
        self.fixed_chunks()
        _, _, first, lens = self._batch_plan
        starts = None
        if chunking == "pauses":
            first, starts, lens = self.pause_chunks(chunk_size, pause_search, pause_smooth)
        flat: Dict[str, List[DecodeResult]] = {m: [] for m in modes}
        for s in range(0, len(lens), self.cfg.max_chunks):
            e = min(len(lens), s + self.cfg.max_chunks)
            self.encode(None, lens[s:e], beam_size, blank_penalty, first_chunk=s, T0=chunk_size, topk=joint_topk(modes, beam_size))
            part = self.search(modes, ctc_weight, reverse_weight, length_penalty)
            for m in modes:
                flat[m].extend(part[m])
        per_rec = [{m: flat[m][int(first[r]):int(first[r + 1])] for m in modes} for r in range(len(first) - 1)]
        if starts is None:
            return per_rec
        return per_rec, [starts[int(first[r]):int(first[r + 1])].tolist() for r in range(len(first) - 1)]

    # -------------------------------------------------------------------------------- decode
    def encode(self, feats: Optional[np.ndarray], lens, beam: int, blank_penalty: float = 0.0, first_chunk: int = 0,
               T0: Optional[int] = None, topk: Optional[int] = None):
        """`beam`: the search beam of the modes that follow; `topk` (>= beam): CTC log-probs kept per frame, when a mode needs
        more than the beam (joint_decoding's pre-beam = int(1.5 * beam))."""
        lens = np.ascontiguousarray(np.asarray(lens, dtype=np.int32).reshape(-1))
        B = len(lens)
        if feats is not None:
            feats = np.ascontiguousarray(feats, dtype=np.float32)
            assert feats.ndim == 3 and feats.shape[0] == B and feats.shape[2] == self.cfg.input_dim
            T0 = feats.shape[1]
        elif T0 is None:
            T0 = self.cfg.chunk_frames
        k = max(int(beam), int(topk or 0))
        if k > 64:
            raise RvbError(f"the CTC kernel keeps at most 64 log-probs per frame; beam {beam}" +
                           (f" with joint_decoding's pre-beam {topk}" if topk else "") + " needs more")
        check(self.lib.rvb_encode(self.handle, fptr(feats), int(first_chunk), iptr(lens), B, int(T0), k,
                                  float(blank_penalty)), "rvb_encode")
        t = C.c_int32(0)
        check(self.lib.rvb_encoder_frames(self.handle, C.byref(t)))
        self.batch, self.enc_frames, self.beam, self.topk = B, int(t.value), int(beam), k
        self._last_T0 = int(T0)
        # joint_decode's tie retry encodes the batch again; only an encode that asked for joint decoding's pre-beam (topk) and
        # so may be followed by joint_decode keeps its arguments, and joint_decode drops them when it is done (every encode pinned
        # hundreds of MB of features for the engine's lifetime)
        self._last_encode = ((feats, lens, int(beam), float(blank_penalty), int(first_chunk), int(T0))
                             if topk and k < 64 else None)      # feats None: the resident features (valid until the next upload)

    # -------------------------------------------------------------------------------- streaming encoder
    def stream_begin(self):
        """Empty the attention cache: the next forward_chunk starts a new stream (encoder.py:385-388)."""
        check(self.lib.rvb_stream_begin(self.handle), "rvb_stream_begin")

    def forward_chunk(self, xs: np.ndarray, required_cache_size: int = -1, return_output: bool = True):
        """BaseEncoder.forward_chunk (encoder.py:231-341) on the engine's stream state: xs (time, 80) raw log-mel of one
        chunk -> (chunk_frames_out, d) encoder output; `offset` and the attention cache are kept by the engine
        (stream_state())."""
        xs = np.ascontiguousarray(xs, dtype=np.float32).reshape(-1, self.cfg.input_dim)
        cap = max((xs.shape[0] - 3) // 2 + 1, 1)
        out = np.empty((cap, self.cfg.d_model), np.float32) if return_output else None
        n = C.c_int32(0)
        check(self.lib.rvb_stream_chunk(self.handle, fptr(xs), xs.shape[0], int(required_cache_size), fptr(out), C.byref(n)),
              "rvb_stream_chunk")
        return out[:n.value] if return_output else n.value

    def stream_state(self):
        """(offset, cached frames): encoder frames produced so far / frames in the attention cache (att_cache.size(2))."""
        o, c = C.c_int32(0), C.c_int32(0)
        check(self.lib.rvb_stream_state(self.handle, C.byref(o), C.byref(c)))
        return int(o.value), int(c.value)

    def forward_chunk_by_chunk(self, xs: np.ndarray, decoding_chunk_size: int, num_decoding_left_chunks: int = -1,
                               return_output: bool = True):
        """BaseEncoder.forward_chunk_by_chunk (encoder.py:343-402): overlapping input windows of (chunk-1)*4 + 7 frames every
        4*chunk frames, attention cache of chunk * left frames.  xs (T, 80) -> (T', d)."""
        assert decoding_chunk_size > 0
        xs = np.ascontiguousarray(xs, dtype=np.float32).reshape(-1, self.cfg.input_dim)
        subsampling, context = 4, 7                       # Conv2dSubsampling4: rate 4, right_context 6 (+ current frame)
        stride = subsampling * decoding_chunk_size
        window = (decoding_chunk_size - 1) * subsampling + context
        required = decoding_chunk_size * num_decoding_left_chunks
        self.stream_begin()
        outs = []
        for cur in range(0, xs.shape[0] - context + 1, stride):
            y = self.forward_chunk(xs[cur:min(cur + window, xs.shape[0])], required, return_output)
            if return_output:
                outs.append(y)
        if not return_output:
            return None
        return np.concatenate(outs) if outs else np.zeros((0, self.cfg.d_model), np.float32)

    def stream_finish(self, beam: int, blank_penalty: float = 0.0, topk: Optional[int] = None):
        """CTC head + top-k over the streamed frames; greedy() / prefix_beam() / rescore() / encoder_out() then see the
        stream as one chunk."""
        k = max(int(beam), int(topk or 0))
        check(self.lib.rvb_stream_finish(self.handle, k, float(blank_penalty)), "rvb_stream_finish")
        t = C.c_int32(0)
        check(self.lib.rvb_encoder_frames(self.handle, C.byref(t)))
        self.batch, self.enc_frames, self.beam, self.topk = 1, int(t.value), int(beam), k

    def encoder_lens(self) -> np.ndarray:
        out = np.empty(self.batch, np.int32)
        check(self.lib.rvb_get_encoder_lens(self.handle, iptr(out)))
        return out

    def encoder_out(self) -> np.ndarray:
        out = np.empty((self.batch, self.enc_frames, self.cfg.d_model), np.float32)
        check(self.lib.rvb_get_encoder_out(self.handle, fptr(out)))
        return out

    def set_encoder_tap(self, block: int = -1):
        """Parity taps of one position of the offline encoder (include/rvb.h rvb_set_encoder_tap): block 0 .. blocks - 1, `blocks`
        for the front end before block 0, -1 for off.  The following encode() calls keep that position's stored tensors."""
        check(self.lib.rvb_set_encoder_tap(self.handle, int(block)), "rvb_set_encoder_tap")

    def encoder_tap(self, name: str) -> np.ndarray:
        """One tensor the last tapped encode() kept, as float32 (bf16 widened bit for bit): [B * T, width] for a block's tensors,
        X1 [B, T1, F1, d], X2 [B, T, F2, d], pos_keys [T, d], pos_bias [heads, T], forms: a list of ints (see rvb_get_encoder_tap)."""
        c, B, T = self.cfg, self.batch, self.enc_frames
        d, ff = c.d_model, c.ffn_dim
        if name == "forms":
            out = np.zeros(32, np.float32)
            check(self.lib.rvb_get_encoder_tap(self.handle, b"forms", fptr(out), out.size), "rvb_get_encoder_tap")
            return [int(v) for v in out[1:1 + int(out[0])]]
        T0 = self._last_T0
        T1, F1 = (T0 - 3) // 2 + 1, (c.input_dim - 3) // 2 + 1
        F2 = (F1 - 3) // 2 + 1
        if name == "glu":
            shape = (B * T, d if self.encoder_tap("forms")[1] else 2 * d)
        else:
            shape = {"X1": (B, T1, F1, d), "X2": (B, T, F2, d), "pos_keys": (T, d), "pos_bias": (c.heads, T), "h_ffm": (B * T, ff),
                     "h_ff": (B * T, ff), "qkv": (B * T, 3 * d)}.get(name, (B * T, d))
        out = np.empty(shape, np.float32)
        check(self.lib.rvb_get_encoder_tap(self.handle, name.encode(), fptr(out), out.size), "rvb_get_encoder_tap")
        return out

    TRIE_ARRAYS = ("tok", "pos", "path", "hq_start", "hq_len", "hq_pos0", "hkv_start", "hkv_len", "crow_start", "crow_len", "tgt_ptr",
                   "tgt", "work")

    def set_decoder_tap(self, side: int = 0, position: int = -1):
        """Parity taps of one position of a rescoring decoder (include/rvb.h rvb_set_decoder_tap): side 0 left / 1 right; position
        0 .. layers - 1 a decoder layer, `layers` the head, -1 off.  The following rescore() / attention_score() calls keep that
        position's stored tensors."""
        check(self.lib.rvb_set_decoder_tap(self.handle, int(side), int(position)), "rvb_set_decoder_tap")

    def decoder_tap(self, name: str):
        """One tensor the last tapped decoder pass kept, as float32 (bf16 widened bit for bit), [rows, width]; `forms`: a list of
        ints; `trie`: dict of the int32 arrays TRIE_ARRAYS (see rvb_get_decoder_tap)."""
        c = self.cfg
        d = c.d_model
        if name == "forms":
            out = np.zeros(256, np.float32)
            check(self.lib.rvb_get_decoder_tap(self.handle, b"forms", fptr(out), out.size), "rvb_get_decoder_tap")
            return [int(v) for v in out[1:1 + int(out[0])]]
        if name == "trie":
            head = np.zeros(1 + len(self.TRIE_ARRAYS), np.float32)
            check(self.lib.rvb_get_decoder_tap(self.handle, b"trie_dims", fptr(head), head.size), "rvb_get_decoder_tap")
            out = np.zeros(head.size + int(head[1:].sum()), np.float32)
            check(self.lib.rvb_get_decoder_tap(self.handle, b"trie", fptr(out), out.size), "rvb_get_decoder_tap")
            n = out[1:1 + len(self.TRIE_ARRAYS)].astype(np.int64)
            assert int(out[0]) == len(self.TRIE_ARRAYS) and out.size == 1 + len(n) + int(n.sum())
            off = np.concatenate([[0], np.cumsum(n)]) + 1 + len(n)
            return {k: out[off[i]:off[i + 1]].astype(np.int32) for i, k in enumerate(self.TRIE_ARRAYS)}
        trie = self.decoder_tap("trie")
        R, P = len(trie["tok"]), len(trie["tgt"])
        shape = {"qkv": (R, 3 * d), "h": (R, c.dec_ffn_dim), "kvmem": (self.batch * self.enc_frames, 2 * d),
                 "logits": (R, (c.vocab + 3) & ~3), "logp": (P,)}.get(name, (R, d))
        out = np.empty(shape, np.float32)
        check(self.lib.rvb_get_decoder_tap(self.handle, name.encode(), fptr(out), out.size), "rvb_get_decoder_tap")
        return out

    def ctc_logprobs(self, chunk: int) -> np.ndarray:
        out = np.empty((self.enc_frames, self.cfg.vocab), np.float32)
        check(self.lib.rvb_get_ctc_logprobs(self.handle, int(chunk), fptr(out)))
        return out

    def ctc_topk(self):
        k = getattr(self, "topk", self.beam)
        v = np.empty((self.batch, self.enc_frames, k), np.float32)
        i = np.empty((self.batch, self.enc_frames, k), np.int32)
        check(self.lib.rvb_get_ctc_topk(self.handle, fptr(v), iptr(i)))
        return v, i

    def greedy(self) -> List[DecodeResult]:
        T = self.enc_frames
        tok = np.empty((self.batch, T), np.int32); n = np.empty(self.batch, np.int32); fr = np.empty((self.batch, T), np.int32)
        check(self.lib.rvb_ctc_greedy(self.handle, iptr(tok), iptr(n), iptr(fr)), "rvb_ctc_greedy")
        res = []
        for b in range(self.batch):
            r = DecodeResult(tok[b, :n[b]].tolist())
            r.ctc_frames = fr[b, :n[b]].tolist()
            res.append(r)
        return res

    def _chunk_spans(self, n, chunk_ranges, default, mismatch=None):
        """The chunks behind the n sequences of an align / score / find call: chunk_ranges[i] = (first, count), None -> default.
        -> (lens, first, count, frames): the batch's valid encoder frames per chunk, and per sequence its first chunk, its chunk
        count and its frames (0 for a range outside the batch, which the library refuses by name).  mismatch: the RvbError text
        when there is not one range per sequence, or no sequence at all."""
        if chunk_ranges is None:
            chunk_ranges = default
        if mismatch is not None and (len(chunk_ranges) != n or not n):
            raise RvbError(mismatch)
        lens = self.encoder_lens()
        first = np.array([r[0] for r in chunk_ranges], np.int32)
        count = np.array([r[1] for r in chunk_ranges], np.int32)
        frames = [int(lens[f:f + c].sum()) if 0 <= f and c >= 1 and f + c <= self.batch else 0 for f, c in zip(first, count)]
        return lens, first, count, frames

    @staticmethod
    def _pack_tokens(seqs):
        """int32 id sequences -> (their ids concatenated, one zero if there is none; their lengths), as the C ABI takes them."""
        tok = np.ascontiguousarray(np.concatenate(seqs) if sum(map(len, seqs)) else np.zeros(1, np.int32), np.int32)
        return tok, np.array([len(t) for t in seqs], np.int32)

    def align(self, token_seqs, chunk_ranges=None):
        """Forced alignment (rvb_ctc_align; reference: force_align, utils/ctc_utils.py:105-161) of known token sequences against the
        chunks of the last encode(): sequence i covers the chunks chunk_ranges[i] = (first, count), default one sequence per chunk
        in order (utterance by utterance); ONE sequence with (0, batch) aligns the transcript of the whole batch.  -> List[AlignResult]."""
        return self._align(token_seqs, chunk_ranges, None)

    def align_wild(self, token_seqs, chunk_ranges=None, wildcard_bias=0.0):
        """align() for transcripts with gaps (rvb_ctc_align_wild): a token ctc_align.WILDCARD (-2) stands for audio that was not
        transcribed.  It is a CTC label of its own that takes at least one frame and emits the frame's largest log-prob (blank
        included) + wildcard_bias (<= 0, nats per frame: the misfit above which the aligner prefers the wildcard to the
        transcript).  Its frames carry WILDCARD in `labels`, AlignResult.wildcard marks the tokens, its confidence is the largest
        top-1 probability of its run.  Without a wildcard the results are those of align(), bit for bit."""
        return self._align(token_seqs, chunk_ranges, float(wildcard_bias))

    def _align(self, token_seqs, chunk_ranges, wildcard_bias):
        from .ctc_align import AlignResult
        seqs = [np.ascontiguousarray(t, np.int32).reshape(-1) for t in token_seqs]
        lens, first, count, frames = self._chunk_spans(len(seqs), chunk_ranges, [(i, 1) for i in range(len(seqs))],
                                                       "align: one chunk range per token sequence, at least one sequence")
        tok, tl = self._pack_tokens(seqs)
        labels = np.empty(max(sum(frames), 1), np.int32)
        nt = max(int(tl.sum()), 1)
        begin, end, peak = (np.empty(nt, np.int32) for _ in range(3))
        conf, score = np.empty(nt, np.float32), np.empty(len(seqs), np.float32)
        if wildcard_bias is None:
            check(self.lib.rvb_ctc_align(self.handle, iptr(tok), iptr(tl), len(seqs), iptr(first), iptr(count), iptr(labels), iptr(begin),
                                         iptr(end), iptr(peak), fptr(conf), fptr(score)), "rvb_ctc_align")
        else:
            check(self.lib.rvb_ctc_align_wild(self.handle, iptr(tok), iptr(tl), len(seqs), iptr(first), iptr(count), wildcard_bias,
                                              iptr(labels), iptr(begin), iptr(end), iptr(peak), fptr(conf), fptr(score)),
                  "rvb_ctc_align_wild")
        out, t0, f0 = [], 0, 0
        for i, t in enumerate(seqs):
            n = len(t)
            out.append(AlignResult(t.tolist(), labels[f0:f0 + frames[i]].tolist(), begin[t0:t0 + n].tolist(), end[t0:t0 + n].tolist(),
                                   peak[t0:t0 + n].tolist(), conf[t0:t0 + n].tolist(), float(score[i]), int(first[i]),
                                   lens[first[i]:first[i] + count[i]].tolist()))
            t0 += n; f0 += frames[i]
        return out

    # ---- long-form alignment (rvb_ctc_align_long_*, csrc/ctc_viterbi_window.hip): one transcript over several encoded batches
    def align_long_begin(self, tokens, total_frames, window_states=0, wildcard_bias=0.0):
        """Open ONE lattice of `tokens` (ids; ctc_align.WILDCARD allowed) over total_frames valid encoder frames, which the encoded
        batches to come deliver through align_long_feed().  window_states: 0 (the default, 32 768) or a multiple of 256 in
        [256, 32768]: the states alive at a frame.  -> the window in use (reduced to the lattice rounded up to 32 states)."""
        tok = np.ascontiguousarray(tokens, np.int32).reshape(-1)
        self._long_tokens = tok.tolist()
        self._long_frames = int(total_frames)
        check(self.lib.rvb_ctc_align_long_begin(self.handle, iptr(tok if tok.size else np.zeros(1, np.int32)), int(tok.size),
                                                int(total_frames), int(window_states), float(wildcard_bias)), "rvb_ctc_align_long_begin")
        return min(int(window_states) or 32768, (2 * tok.size + 1 + 31) // 32 * 32)

    def align_long_feed(self):
        """After encode(): every valid frame of the encoded batch, in chunk order, continues the lattice."""
        check(self.lib.rvb_ctc_align_long_feed(self.handle), "rvb_ctc_align_long_feed")

    def align_long_finish(self):
        """-> (labels [total_frames], begin [tokens], end [tokens], score, min_margin) once every frame was fed; min_margin is the
        path's smallest distance, in states, to a window edge that is not the lattice's own (the window when no frame counts)."""
        n = getattr(self, "_long_frames", 0)
        nt = len(getattr(self, "_long_tokens", []))
        labels = np.empty(max(n, 1), np.int32)
        begin, end = np.empty(max(nt, 1), np.int32), np.empty(max(nt, 1), np.int32)
        score, margin = np.empty(1, np.float32), np.empty(1, np.int32)
        check(self.lib.rvb_ctc_align_long_finish(self.handle, iptr(labels), iptr(begin), iptr(end), fptr(score), iptr(margin)),
              "rvb_ctc_align_long_finish")
        return labels[:n], begin[:nt], end[:nt], float(score[0]), int(margin[0])

    def align_long_emissions(self, labels):
        """lp[t][labels[t]] of the valid frames of the encoded batch (a WILDCARD frame: the row maximum) -> fp32 [frames]"""
        lab = np.ascontiguousarray(labels, np.int32).reshape(-1)
        out = np.empty(max(lab.size, 1), np.float32)
        check(self.lib.rvb_ctc_align_long_emissions(self.handle, iptr(lab), int(lab.size), fptr(out)), "rvb_ctc_align_long_emissions")
        return out[:lab.size]

    def align_long_end(self):
        check(self.lib.rvb_ctc_align_long_end(self.handle), "rvb_ctc_align_long_end")

    # ---- long-form full-sum score (rvb_ctc_score_long_*, csrc/ctc_fb_window.hip): score() of one transcript over several batches
    def score_long_begin(self, tokens, total_frames, window_states=0, posteriors=False):
        """Open ONE full-sum lattice of `tokens` over total_frames valid encoder frames; window_states as align_long_begin's.
        posteriors=True keeps the forward rows (total_frames x window x 4 bytes) for the backward sweep.  -> the window in use."""
        tok = np.ascontiguousarray(tokens, np.int32).reshape(-1)
        self._score_long_tokens = int(tok.size)
        check(self.lib.rvb_ctc_score_long_begin(self.handle, iptr(tok if tok.size else np.zeros(1, np.int32)), int(tok.size),
                                                int(total_frames), int(window_states), int(bool(posteriors))), "rvb_ctc_score_long_begin")
        return min(int(window_states) or 32768, (2 * tok.size + 1 + 31) // 32 * 32)

    def score_long_feed(self):
        """After encode(), batches in ascending order: every valid frame of the encoded batch continues the forward sweep."""
        check(self.lib.rvb_ctc_score_long_feed(self.handle), "rvb_ctc_score_long_feed")

    def score_long_loglik(self):
        """-> loglik (fp64) once every frame was fed."""
        ll = np.empty(1, np.float64)
        check(self.lib.rvb_ctc_score_long_loglik(self.handle, dptr(ll)), "rvb_ctc_score_long_loglik")
        return float(ll[0])

    def score_long_feed_back(self):
        """After score_long_loglik() and encode(), the same batches in DESCENDING order: the backward sweep (needs posteriors)."""
        check(self.lib.rvb_ctc_score_long_feed_back(self.handle), "rvb_ctc_score_long_feed_back")

    def score_long_finish(self):
        """-> dict of per-token occupancy, mean_frame, peak_posterior, peak_frame (frames within the lattice), as score()'s."""
        n = getattr(self, "_score_long_tokens", 0)
        occ, mean, peak = (np.empty(max(n, 1), np.float32) for _ in range(3))
        pkf = np.empty(max(n, 1), np.int32)
        check(self.lib.rvb_ctc_score_long_finish(self.handle, fptr(occ), fptr(mean), fptr(peak), iptr(pkf)), "rvb_ctc_score_long_finish")
        return {"occupancy": occ[:n].tolist(), "mean_frame": mean[:n].tolist(), "peak_posterior": peak[:n].tolist(),
                "peak_frame": pkf[:n].tolist()}

    def score_long_end(self):
        check(self.lib.rvb_ctc_score_long_end(self.handle), "rvb_ctc_score_long_end")

    def align_graph(self, graphs, chunk_ranges=None, wildcard_bias=0.0):
        """align_wild() for transcripts with alternatives and optional words (rvb_ctc_align_graph, csrc/ctc_graph.hip): each sequence
        is a token_graph.TokenGraph, and one Viterbi pass picks the reading that was spoken and aligns it.  -> List[AlignResult]
        whose `nodes` is the chosen path and whose `tokens` / begin / end / peak / confidence describe the nodes on it, so everything
        that reads an align() result reads this one.  On TokenGraph.chain(ids) the result is that of align_wild(ids), bit for bit."""
        from .ctc_align import AlignResult
        from ._lib import u8ptr
        graphs = list(graphs)
        lens, first, count, frames = self._chunk_spans(len(graphs), chunk_ranges, [(i, 1) for i in range(len(graphs))],
                                                       "align_graph: one chunk range per graph, at least one graph")
        arrs = [g.arrays() for g in graphs]
        tok, off, prd, fin = (np.ascontiguousarray(np.concatenate([a[k] for a in arrs])) for k in range(4))
        nn = np.array([len(g) for g in graphs], np.int32)
        labels, fnode = (np.empty(max(sum(frames), 1), np.int32) for _ in range(2))
        nt = int(nn.sum())
        path, begin, end, peak = (np.empty(nt, np.int32) for _ in range(4))
        plen, conf, score = np.empty(len(graphs), np.int32), np.empty(nt, np.float32), np.empty(len(graphs), np.float32)
        check(self.lib.rvb_ctc_align_graph(self.handle, iptr(tok), iptr(nn), iptr(off), iptr(prd), u8ptr(fin), len(graphs), iptr(first),
                                           iptr(count), float(wildcard_bias), iptr(labels), iptr(fnode), iptr(plen), iptr(path),
                                           iptr(begin), iptr(end), iptr(peak), fptr(conf), fptr(score)), "rvb_ctc_align_graph")
        out, t0, f0 = [], 0, 0
        for i, g in enumerate(graphs):
            n = int(plen[i])
            nodes = path[t0:t0 + n].tolist()
            out.append(AlignResult([g.tokens[j] for j in nodes], labels[f0:f0 + frames[i]].tolist(), begin[t0:t0 + n].tolist(),
                                   end[t0:t0 + n].tolist(), peak[t0:t0 + n].tolist(), conf[t0:t0 + n].tolist(), float(score[i]),
                                   int(first[i]), lens[first[i]:first[i] + count[i]].tolist(), nodes))
            t0 += len(g); f0 += frames[i]
        return out

    # ---- long-form graph alignment (rvb_ctc_align_graph_long_*, csrc/ctc_graph_window.hip): one graph over several encoded batches
    def align_graph_long_begin(self, graph, total_frames, window_nodes=0, wildcard_bias=0.0):
        """Open ONE lattice of `graph` (a token_graph.TokenGraph of any number of nodes) over total_frames valid encoder frames, which
        the encoded batches to come deliver through align_graph_long_feed().  window_nodes: 0 (the default, 8192) or a multiple of
        256 in [256, 8192]: the nodes alive at a frame.  -> the window in use (reduced to the graph rounded up to 64 nodes)."""
        from ._lib import u8ptr
        tok, off, prd, fin = (np.ascontiguousarray(a) for a in graph.arrays())
        self._long_graph = graph
        self._long_graph_frames = int(total_frames)
        check(self.lib.rvb_ctc_align_graph_long_begin(self.handle, iptr(tok), int(tok.size), iptr(off), iptr(prd), u8ptr(fin),
                                                      int(total_frames), int(window_nodes), float(wildcard_bias)),
              "rvb_ctc_align_graph_long_begin")
        return min(int(window_nodes) or 8192, (len(graph) + 63) // 64 * 64)

    def align_graph_long_feed(self):
        """After encode(): every valid frame of the encoded batch, in chunk order, continues the lattice."""
        check(self.lib.rvb_ctc_align_graph_long_feed(self.handle), "rvb_ctc_align_graph_long_feed")

    def align_graph_long_finish(self):
        """-> (labels [total_frames], frame_node [total_frames], path nodes, begin, end (per path position), score, min_margin) once
        every frame was fed; min_margin is the path's smallest distance, in nodes, to a window edge that is not the graph's own."""
        graph = getattr(self, "_long_graph", None)
        n, nn = getattr(self, "_long_graph_frames", 0), len(graph) if graph is not None else 0
        labels, fnode = np.empty(max(n, 1), np.int32), np.empty(max(n, 1), np.int32)
        path, begin, end = (np.empty(max(nn, 1), np.int32) for _ in range(3))
        plen, score, margin = np.zeros(1, np.int32), np.empty(1, np.float32), np.empty(1, np.int32)
        check(self.lib.rvb_ctc_align_graph_long_finish(self.handle, iptr(labels), iptr(fnode), iptr(plen), iptr(path), iptr(begin),
                                                       iptr(end), fptr(score), iptr(margin)), "rvb_ctc_align_graph_long_finish")
        k = int(plen[0])
        return labels[:n], fnode[:n], path[:k], begin[:k], end[:k], float(score[0]), int(margin[0])

    def align_graph_long_end(self):
        check(self.lib.rvb_ctc_align_graph_long_end(self.handle), "rvb_ctc_align_graph_long_end")
        self._long_graph = None

    # ---- long-form graph full sum (rvb_ctc_score_graph_long_*, csrc/ctc_graph_fb_window.hip): one graph over several encoded batches
    def score_graph_long_begin(self, graph, total_frames, window_nodes=0, posteriors=False):
        """Open ONE full-sum lattice of `graph` (a token_graph.TokenGraph of any number of nodes, no wildcards) over total_frames valid
        encoder frames.  window_nodes: 0 (the default, 4096) or a multiple of 256 in [256, 4096].  posteriors=True keeps the forward
        rows (total_frames x window x 4 bytes) for the backward sweep.  -> the window in use (reduced to the graph rounded up to 64)."""
        from ._lib import u8ptr
        tok, off, prd, fin = (np.ascontiguousarray(a) for a in graph.arrays())
        self._score_long_graph_nodes = len(graph)
        check(self.lib.rvb_ctc_score_graph_long_begin(self.handle, iptr(tok), int(tok.size), iptr(off), iptr(prd), u8ptr(fin),
                                                      int(total_frames), int(window_nodes), int(bool(posteriors))),
              "rvb_ctc_score_graph_long_begin")
        return min(int(window_nodes) or 4096, (len(graph) + 63) // 64 * 64)

    def score_graph_long_feed(self):
        """After encode(), batches in ascending order: every valid frame of the encoded batch continues the forward sweep."""
        check(self.lib.rvb_ctc_score_graph_long_feed(self.handle), "rvb_ctc_score_graph_long_feed")

    def score_graph_long_loglik(self):
        """-> loglik (fp64) once every frame was fed."""
        ll = np.empty(1, np.float64)
        check(self.lib.rvb_ctc_score_graph_long_loglik(self.handle, dptr(ll)), "rvb_ctc_score_graph_long_loglik")
        return float(ll[0])

    def score_graph_long_feed_back(self):
        """After score_graph_long_loglik() and encode(), the same batches in DESCENDING order: the backward sweep (needs posteriors)."""
        check(self.lib.rvb_ctc_score_graph_long_feed_back(self.handle), "rvb_ctc_score_graph_long_feed_back")

    def score_graph_long_finish(self):
        """-> dict of per-node visit, occupancy, mean_frame, peak_posterior, peak_frame (frames within the lattice), as score_graph()'s."""
        n = getattr(self, "_score_long_graph_nodes", 0)
        vis, occ, mean, peak = (np.empty(max(n, 1), np.float32) for _ in range(4))
        pkf = np.empty(max(n, 1), np.int32)
        check(self.lib.rvb_ctc_score_graph_long_finish(self.handle, fptr(vis), fptr(occ), fptr(mean), fptr(peak), iptr(pkf)),
              "rvb_ctc_score_graph_long_finish")
        return {"visit": vis[:n].tolist(), "occupancy": occ[:n].tolist(), "mean_frame": mean[:n].tolist(),
                "peak_posterior": peak[:n].tolist(), "peak_frame": pkf[:n].tolist()}

    def score_graph_long_end(self):
        check(self.lib.rvb_ctc_score_graph_long_end(self.handle), "rvb_ctc_score_graph_long_end")

    def find(self, phrases, chunk_ranges=None, min_score=-1.0, max_hits=64, max_candidates=None):
        """Phrase search (rvb_ctc_find, csrc/ctc_find.hip): EVERY occurrence of each token phrase (1 .. 32 ids, none the blank) in the
        chunks of the last encode().  Sequence i covers the chunks chunk_ranges[i] = (first, count); the default is ONE sequence
        over the whole batch, so a hit may straddle a chunk boundary.  A frame costs what the phrase's label loses against the
        model's own best label there, so a score of 0 means the greedy labels spell the phrase.  min_score is in nats PER TOKEN:
        a phrase of L tokens keeps the occurrences with score >= float32(min_score * L) (-inf: every arrival).  Overlapping
        occurrences of one phrase in one sequence are suppressed, best first; at most max_hits per phrase and sequence.
        -> hits[phrase][sequence] = List[Hit], in order of end_frame; frames are numbered within the sequence.
        The device keeps max_candidates candidates per phrase and sequence (default: 4 max_hits, at least 256); if more arrive the
        call is repeated ONCE with the largest count reported, and RvbError is raised if that still overflows."""
        from .ctc_align import Hit
        seqs = [np.ascontiguousarray(t, np.int32).reshape(-1) for t in phrases]
        if not seqs:
            raise RvbError("find: at least one phrase")
        lens, first, count, _ = self._chunk_spans(None, chunk_ranges, [(0, self.batch)])
        tok, tl = self._pack_tokens(seqs)
        thr = np.array([np.float32(min_score * len(t)) for t in seqs], np.float32)
        thr[np.isnan(thr) & (tl == 0)] = 0.0                 # -inf * 0: the empty phrase is refused below, by its own name
        n_p, n_s, max_hits = len(seqs), len(first), int(max_hits)
        cap = int(max_candidates) if max_candidates is not None else max(4 * max_hits, 256)
        n_hits = np.zeros(max(n_p * n_s, 1), np.int32)
        start, end = (np.zeros(max(n_p * n_s * max(max_hits, 1), 1), np.int32) for _ in range(2))
        score = np.zeros(start.size, np.float32)
        n_cand = np.zeros(n_hits.size, np.int64)
        self.last_find = {"calls": 0, "max_candidates": cap}
        for attempt in range(2):
            check(self.lib.rvb_ctc_find(self.handle, iptr(tok), iptr(tl), n_p, fptr(thr), iptr(first), iptr(count), n_s, cap, max_hits,
                                        iptr(n_hits), iptr(start), iptr(end), fptr(score), n_cand.ctypes.data_as(_lib._i64p)), "rvb_ctc_find")
            self.last_find = {"calls": attempt + 1, "max_candidates": cap}
            worst = int(n_cand.max())
            if worst <= cap:
                break
            if attempt == 1:
                raise RvbError(f"find: {worst} candidates of one phrase and sequence still exceed the cap of {cap} after one retry")
            cap = worst
        out = []
        for p, t in enumerate(seqs):
            per_seq = []
            for i in range(n_s):
                k = p * n_s + i
                ends = np.cumsum(lens[first[i]:first[i] + count[i]])
                hits = []
                for j in range(int(n_hits[k])):
                    b, e, v = int(start[k * max_hits + j]), int(end[k * max_hits + j]), float(score[k * max_hits + j])
                    c = int(np.searchsorted(ends, b, side="right"))
                    hits.append(Hit(b, e, v, v / len(t), int(first[i]) + c, b - (int(ends[c - 1]) if c else 0)))
                per_seq.append(hits)
            out.append(per_seq)
        return out

    def score(self, token_seqs, chunk_ranges=None, posteriors=False, attention=False, reverse_weight=None, lsm_weight=None,
              ctc_weight=None):
        """Full-sum CTC score (rvb_ctc_score; reference: CTC.forward, transformer/ctc.py:65-104 = -CTCLoss(reduction='sum')) of known
        token sequences against the chunks of the last encode(); sequences and chunk_ranges as in align(), and several sequences
        over the SAME chunks compare candidate transcripts in one launch.  -> List[dict]: loglik (fp64), n_tokens, n_frames and, with
        posteriors=True, per token occupancy (expected frames), mean_frame, peak_posterior, peak_frame (frames within the sequence).
        attention=True adds what the reference's bin/get_loss.py reports for the transcript (ASRModel.forward, asr_model.py:105-151,
        with a batch of one): loss_ctc (= -loglik), loss_att (the decoders' label-smoothed KL, (1 - reverse_weight) left +
        reverse_weight right, divided by L + 1 when the config's length_normalized_loss is true, else by the batch size 1), acc_att
        (th_accuracy of the left decoder over the L + 1 positions), loss = ctc_weight loss_ctc + (1 - ctc_weight) loss_att, att_logp
        (left decoder, log p of each target, <eos> last).  lsm_weight, ctc_weight and reverse_weight
        default to the config's model_conf.  The decoder's memory is ONE chunk: a sequence over several chunks is refused."""
        seqs = [np.ascontiguousarray(t, np.int32).reshape(-1) for t in token_seqs]
        _, first, count, frames = self._chunk_spans(len(seqs), chunk_ranges, [(i, 1) for i in range(len(seqs))],
                                                    "score: one chunk range per token sequence, at least one sequence")
        tok, tl = self._pack_tokens(seqs)
        nt = max(int(tl.sum()), 1)
        loglik = np.empty(len(seqs), np.float64)
        occ, mean, peak = (np.empty(nt, np.float32) for _ in range(3))
        pkf = np.empty(nt, np.int32)
        none_f, none_i = C.POINTER(C.c_float)(), C.POINTER(C.c_int32)()
        check(self.lib.rvb_ctc_score(self.handle, iptr(tok), iptr(tl), len(seqs), iptr(first), iptr(count), dptr(loglik),
                                     fptr(occ) if posteriors else none_f, fptr(mean) if posteriors else none_f,
                                     fptr(peak) if posteriors else none_f, iptr(pkf) if posteriors else none_i), "rvb_ctc_score")
        out, t0 = [], 0
        for i, t in enumerate(seqs):
            n = len(t)
            r = {"loglik": float(loglik[i]), "n_tokens": n, "n_frames": frames[i]}
            if posteriors:
                r.update(occupancy=occ[t0:t0 + n].tolist(), mean_frame=mean[t0:t0 + n].tolist(), peak_posterior=peak[t0:t0 + n].tolist(),
                         peak_frame=pkf[t0:t0 + n].tolist())
            out.append(r)
            t0 += n
        if attention:
            self._attention_score(seqs, first, count, out, reverse_weight, lsm_weight, ctc_weight)
        return out

    def score_graph(self, graphs, chunk_ranges=None, posteriors=False):
        """score() for transcripts with alternatives and optional words (rvb_ctc_score_graph, csrc/ctc_graph_score.hip): each sequence
        is a token_graph.TokenGraph without wildcards, graphs and chunk_ranges as in align_graph().  loglik is the log of the SUM
        over the graph's node paths of the CTC likelihood of the path's labels; two paths that spell the same tokens are two paths
        and both count ({a|a} scores loglik(a) + log 2), nothing is deduplicated.  -> List[dict]: loglik (fp64), n_nodes, n_frames
        and, with posteriors=True, per node visit (the probability that the path passes through the node = the posterior of the
        readings that contain it), occupancy, mean_frame (-1 where no mass), peak_posterior, peak_frame.  On TokenGraph.chain(ids)
        loglik and the per-node outputs are those of score(ids) within rounding, and every visit is 1."""
        from ._lib import u8ptr
        graphs = list(graphs)
        _, first, count, frames = self._chunk_spans(len(graphs), chunk_ranges, [(i, 1) for i in range(len(graphs))],
                                                    "score_graph: one chunk range per graph, at least one graph")
        arrs = [g.arrays() for g in graphs]
        tok, off, prd, fin = (np.ascontiguousarray(np.concatenate([a[k] for a in arrs])) for k in range(4))
        nn = np.array([len(g) for g in graphs], np.int32)
        nt = max(int(nn.sum()), 1)
        loglik = np.empty(len(graphs), np.float64)
        vis, occ, mean, peak = (np.empty(nt, np.float32) for _ in range(4))
        pkf = np.empty(nt, np.int32)
        none_f, none_i = C.POINTER(C.c_float)(), C.POINTER(C.c_int32)()
        check(self.lib.rvb_ctc_score_graph(self.handle, iptr(tok), iptr(nn), iptr(off), iptr(prd), u8ptr(fin), len(graphs), iptr(first),
                                           iptr(count), dptr(loglik), *[fptr(a) if posteriors else none_f for a in (vis, occ, mean, peak)],
                                           iptr(pkf) if posteriors else none_i), "rvb_ctc_score_graph")
        out, t0 = [], 0
        for i, g in enumerate(graphs):
            n = len(g)
            r = {"loglik": float(loglik[i]), "n_nodes": n, "n_frames": frames[i]}
            if posteriors:
                r.update(visit=vis[t0:t0 + n].tolist(), occupancy=occ[t0:t0 + n].tolist(), mean_frame=mean[t0:t0 + n].tolist(),
                         peak_posterior=peak[t0:t0 + n].tolist(), peak_frame=pkf[t0:t0 + n].tolist())
            out.append(r)
            t0 += n
        return out

    def _attention_score(self, seqs, first, count, out, reverse_weight, lsm_weight, ctc_weight):
        """rvb_attention_score of the sequences of score(); fills the attention keys into the dicts of `out`."""
        mc = self.configs.get("model_conf", {})
        rw = float(mc.get("reverse_weight", 0.0) if reverse_weight is None else reverse_weight)
        lsm = float(mc.get("lsm_weight", 0.0) if lsm_weight is None else lsm_weight)
        cw = float(mc.get("ctc_weight", 0.5) if ctc_weight is None else ctc_weight)
        if np.any(count != 1):
            raise RvbError("score(attention=True) failed (-5): RVB_E_UNSUPPORTED: a sequence spans several chunks; the attention "
                           "decoder's memory is one chunk (score each chunk's transcript against its own chunk)")
        tok, tl = self._pack_tokens(seqs)
        n, npos = len(seqs), int(tl.sum()) + len(seqs)
        loss_l, loss_r = np.zeros(n, np.float64), np.zeros(n, np.float64)
        ncor, nposn = np.zeros(n, np.int32), np.zeros(n, np.int32)
        logp = np.zeros(npos, np.float32)
        check(self.lib.rvb_attention_score(self.handle, iptr(tok), iptr(tl), n, iptr(np.ascontiguousarray(first, np.int32)), rw, lsm,
                                           dptr(loss_l), dptr(loss_r), iptr(ncor), iptr(nposn), fptr(logp), None, None),
              "rvb_attention_score")
        norm_len = bool(mc.get("length_normalized_loss", False))
        p0 = 0
        for i, r in enumerate(out):
            k = int(nposn[i])
            att = ((1.0 - rw) * float(loss_l[i]) + rw * float(loss_r[i])) / (k if norm_len else 1)
            r["loss_ctc"] = -r["loglik"]
            r["loss_att"] = att
            r["acc_att"] = int(ncor[i]) / k
            r["loss"] = cw * r["loss_ctc"] + (1.0 - cw) * att
            r["att_logp"] = logp[p0:p0 + k].tolist()
            p0 += k

    def attention_score(self, token_seqs, chunk_of, reverse_weight: float = 0.0, lsm_weight: float = 0.0):
        """rvb_attention_score as it is: per sequence the un-normalised loss sums of both decoders, the correct / total positions and
        the per-position log-probs (right decoder in its own order) and arg-max.  -> List[dict]."""
        seqs = [np.ascontiguousarray(t, np.int32).reshape(-1) for t in token_seqs]
        if not seqs or len(chunk_of) != len(seqs):
            raise RvbError("attention_score: one chunk per token sequence, at least one sequence")
        tok, tl = self._pack_tokens(seqs)
        ch = np.ascontiguousarray(chunk_of, np.int32)
        n, npos = len(seqs), max(int(np.maximum(tl, 0).sum()) + len(seqs), 1)
        loss_l, loss_r = np.zeros(n, np.float64), np.zeros(n, np.float64)
        ncor, nposn = np.zeros(n, np.int32), np.zeros(n, np.int32)
        lp_l, lp_r, top = np.zeros(npos, np.float32), np.zeros(npos, np.float32), np.zeros(npos, np.int32)
        check(self.lib.rvb_attention_score(self.handle, iptr(tok), iptr(tl), n, iptr(ch), float(reverse_weight), float(lsm_weight),
                                           dptr(loss_l), dptr(loss_r), iptr(ncor), iptr(nposn), fptr(lp_l), fptr(lp_r), iptr(top)),
              "rvb_attention_score")
        out, p0 = [], 0
        for i in range(n):
            k = int(nposn[i])
            out.append({"loss_l": float(loss_l[i]), "loss_r": float(loss_r[i]), "n_correct": int(ncor[i]), "n_positions": k,
                        "logp_l": lp_l[p0:p0 + k].copy(), "logp_r": lp_r[p0:p0 + k].copy(), "top1_l": top[p0:p0 + k].copy()})
            p0 += k
        return out

    def _nbest(self, chunk: int):
        nh, ml = C.c_int32(0), C.c_int32(0)
        check(self.lib.rvb_get_nbest_count(self.handle, chunk, C.byref(nh), C.byref(ml)))
        nh, ml = nh.value, max(ml.value, 1)
        tok = np.empty((nh, ml), np.int32); lens = np.empty(nh, np.int32)
        tim = np.empty((nh, ml), np.int32); tl = np.empty(nh, np.int32); sc = np.empty(nh, np.float64)
        check(self.lib.rvb_get_nbest(self.handle, chunk, iptr(tok), iptr(lens), iptr(tim), iptr(tl), dptr(sc)))
        nbest = [tuple(tok[i, :lens[i]].tolist()) for i in range(nh)]
        times = [tim[i, :tl[i]].tolist() for i in range(nh)]
        return nbest, sc.tolist(), times

    def prefix_beam(self) -> List[DecodeResult]:
        check(self.lib.rvb_ctc_prefix_beam(self.handle, self.beam), "rvb_ctc_prefix_beam")
        res = []
        for b in range(self.batch):
            nbest, scores, times = self._nbest(b)
            res.append(DecodeResult(tokens=nbest[0], score=scores[0], times=times[0], nbest=nbest, nbest_scores=scores,
                                    nbest_times=times))
        return res

    def rescore(self, prefix_results: List[DecodeResult], ctc_weight: float, reverse_weight: float) -> List[DecodeResult]:
        check(self.lib.rvb_attention_rescore(self.handle, float(ctc_weight), float(reverse_weight)), "rvb_attention_rescore")
        res = []
        for b, pr in enumerate(prefix_results):
            bi, sc, cf = C.c_int32(0), C.c_float(0), C.c_double(0)
            check(self.lib.rvb_get_rescored(self.handle, b, C.byref(bi), C.byref(sc), C.byref(cf), None))
            tc = np.empty(max(len(pr.nbest[bi.value]), 1), np.float64)
            check(self.lib.rvb_get_rescored(self.handle, b, None, None, None, dptr(tc)))
            res.append(DecodeResult(pr.nbest[bi.value], float(sc.value), confidence=float(cf.value),
                                    times=pr.nbest_times[bi.value],
                                    tokens_confidence=tc[:len(pr.nbest[bi.value])].tolist()))
        return res

    def _rescore_bulk(self, ctc_weight: float, reverse_weight: float) -> List[DecodeResult]:
        check(self.lib.rvb_attention_rescore(self.handle, float(ctc_weight), float(reverse_weight)), "rvb_attention_rescore")
        return self._rescore_fetch()

    def _rescore_fetch(self) -> List[DecodeResult]:
        """The winners of the last rvb_attention_rescore in one bulk read."""
        B, T = self.batch, self.enc_frames
        lens = np.empty(B, np.int32); tok = np.empty((B, T), np.int32); tl = np.empty(B, np.int32)
        tim = np.empty((B, T), np.int32); sc = np.empty(B, np.float32); cf = np.empty(B, np.float64)
        tc = np.empty((B, T), np.float64)
        check(self.lib.rvb_get_rescored_batch(self.handle, iptr(lens), iptr(tok), iptr(tl), iptr(tim), fptr(sc), dptr(cf),
                                              dptr(tc)), "rvb_get_rescored_batch")
        return [DecodeResult(tuple(tok[b, :lens[b]].tolist()), float(sc[b]), confidence=float(cf[b]),
                             times=tim[b, :tl[b]].tolist(), tokens_confidence=tc[b, :lens[b]].tolist()) for b in range(B)]

    def rescore_stats(self):
        """(decoder rows computed, (hypothesis, position) pairs served) of the last rescoring: distinct prefixes vs the
        padded batch the reference runs."""
        r, p = C.c_int64(0), C.c_int64(0)
        check(self.lib.rvb_get_rescore_stats(self.handle, C.byref(r), C.byref(p)))
        return int(r.value), int(p.value)

    def rescore_logp(self, chunk: int, hyp: int, length: int, right: bool = False) -> np.ndarray:
        out = np.empty(length + 1, np.float32)
        check(self.lib.rvb_get_rescore_logp(self.handle, chunk, hyp, 1 if right else 0, fptr(out)))
        return out

    def attention_beam(self, length_penalty: float = 0.0) -> List[DecodeResult]:
        """`attention` mode (search.py:251-360): tokens only, like the reference's DecodeResult(hyp.tolist())."""
        check(self.lib.rvb_attention_decode(self.handle, self.beam, float(length_penalty)), "rvb_attention_decode")
        tok = np.empty(max(self.enc_frames, 1), np.int32)
        res = []
        for b in range(self.batch):
            n, sc = C.c_int32(0), C.c_float(0)
            check(self.lib.rvb_get_attention_result(self.handle, b, iptr(tok), C.byref(n), C.byref(sc)), "rvb_get_attention_result")
            res.append(DecodeResult(tok[:n.value].tolist()))
        return res

    def joint_decode(self, ctc_weight: float, length_bonus: float = 0.0, pre_beam_ratio: float = JOINT_PRE_BEAM_RATIO
                     ) -> List[DecodeResult]:
        """`joint_decoding` (search.py:450-496): time-synchronous joint CTC / attention beam search of the last encoded batch
        (encode(..., topk=int(pre_beam_ratio * beam)) first).  DecodeResult: tokens, joint score, start frame and confidence
        per token -- the fields the reference fills -- plus `end_times`."""
        rc = self.lib.rvb_joint_decode(self.handle, self.beam, float(ctc_weight), float(pre_beam_ratio), float(length_bonus))
        if (rc == -5 and self.topk < 64 and getattr(self, "_last_encode", None) is not None
                and b"tie exactly" in self.lib.rvb_last_error()):
            # RVB_E_UNSUPPORTED here = a frame holds a longer run of log-probs that tie EXACTLY with the pre-beam threshold than
            # the kept top-k covers (the reference compares the whole row, beam_search_timesync.py:268-270).  Rather than fail
            # the decode after all the work is done, encode the batch again keeping the kernel's maximum of 64
            # log-probs per frame and search once more; only a run longer than that is refused.
            feats, lens, beam, blank_penalty, first_chunk, T0 = self._last_encode
            self.encode(feats, lens, beam, blank_penalty, first_chunk, T0, topk=64)
            rc = self.lib.rvb_joint_decode(self.handle, self.beam, float(ctc_weight), float(pre_beam_ratio), float(length_bonus))
        self._last_encode = None
        check(rc, "rvb_joint_decode")
        T = max(self.enc_frames, 1)
        tok = np.empty(T, np.int32); st = np.empty(T, np.int32); en = np.empty(T, np.int32); cf = np.empty(T, np.float64)
        res = []
        for b in range(self.batch):
            n, sc = C.c_int32(0), C.c_double(0)
            check(self.lib.rvb_get_joint_result(self.handle, b, iptr(tok), iptr(st), iptr(en), dptr(cf), C.byref(n), C.byref(sc)),
                  "rvb_get_joint_result")
            k = n.value
            r = DecodeResult(tok[:k].tolist(), float(sc.value), times=st[:k].tolist(), tokens_confidence=cf[:k].tolist())
            r.end_times = en[:k].tolist()
            res.append(r)
        return res

    def joint_stats(self):
        """(decoder rows computed, batched decoder steps) of the last joint_decode."""
        r, p = C.c_int64(0), C.c_int64(0)
        check(self.lib.rvb_get_joint_stats(self.handle, C.byref(r), C.byref(p)))
        return int(r.value), int(p.value)

    def search(self, methods: Sequence[str], ctc_weight: float, reverse_weight: float, length_penalty: float = 0.0
               ) -> Dict[str, List[DecodeResult]]:
        """Search stages of ASRModel.decode (asr_model.py:391-432) on the last encoded batch."""
        results: Dict[str, List[DecodeResult]] = {}
        for m in methods:
            if m not in SUPPORTED_MODES:
                raise RvbError(f"decoding mode {m!r} is not built yet (supported: {', '.join(SUPPORTED_MODES)})")
        if "attention" in methods:
            results["attention"] = self.attention_beam(length_penalty)
        if "joint_decoding" in methods:          # asr_model.py:427-431: length_bonus = length_penalty
            results["joint_decoding"] = self.joint_decode(ctc_weight, length_penalty)
        if "ctc_greedy_search" in methods:
            results["ctc_greedy_search"] = self.greedy()
        if "attention_rescoring" in methods and "ctc_prefix_beam_search" not in methods:
            # fast path: n-best lists stay in the engine, one bulk read of the winners; the decoders' memory keys / values are
            # enqueued first so that the device has work while the host searches the last slice
            check(self.lib.rvb_prepare_rescoring(self.handle, 1 if reverse_weight > 0 else 0), "rvb_prepare_rescoring")
            check(self.lib.rvb_ctc_prefix_beam(self.handle, self.beam), "rvb_ctc_prefix_beam")
            results["attention_rescoring"] = self._rescore_bulk(ctc_weight, reverse_weight)
        elif "ctc_prefix_beam_search" in methods or "attention_rescoring" in methods:
            pref = self.prefix_beam()
            if "ctc_prefix_beam_search" in methods:
                results["ctc_prefix_beam_search"] = pref
            if "attention_rescoring" in methods:
                results["attention_rescoring"] = self.rescore(pref, ctc_weight, reverse_weight)
        return results

    def decode_resident(self, n_frames: int, modes, chunk_size: int, beam_size: int, ctc_weight: float,
                        reverse_weight: float, blank_penalty: float = 0.0, length_penalty: float = 0.0, chunking: str = "fixed",
                        pause_search: Optional[int] = None, pause_smooth: int = 10):
        """Decode the device-resident features of the last fbank() call: fixed, non-overlapping
        chunks with a length-masked zero-padded tail (feats_batcher, cli/reverb.py:148-180),
        `max_chunks` chunks per launch, results concatenated in chunk order -> {mode: [DecodeResult per chunk]}.
        chunking="pauses": the chunks are the pieces of pause_chunks(chunk_size, pause_search, pause_smooth), of at most chunk_size
        frames each, and the result is (that dict, the start frame of each piece)."""
        if not 7 <= chunk_size <= self.cfg.chunk_frames:
            raise RvbError(f"resident decoding needs 7 <= chunk_size <= engine chunk_frames ({self.cfg.chunk_frames}); "
                           "ReverbASR rebuilds the engine for larger chunks")
        _check_chunking(chunking)
        starts = None
        if chunking == "pauses":
            _, starts, lens = self.pause_chunks(chunk_size, pause_search, pause_smooth)
            if int(lens.sum()) != int(n_frames):
                raise RvbError(f"decode_resident: n_frames = {n_frames}, the resident features hold {int(lens.sum())}")
            n_chunks = len(lens)
        else:
            self.fixed_chunks()
            n_chunks = -(-n_frames // chunk_size)
            lens = np.full(n_chunks, chunk_size, np.int32)
            if n_chunks:
                lens[-1] = n_frames - (n_chunks - 1) * chunk_size
        out: Dict[str, List[DecodeResult]] = {m: [] for m in modes}
        for s in range(0, n_chunks, self.cfg.max_chunks):
            e = min(n_chunks, s + self.cfg.max_chunks)
            self.encode(None, lens[s:e], beam_size, blank_penalty, first_chunk=s, T0=chunk_size, topk=joint_topk(modes, beam_size))
            part = self.search(modes, ctc_weight, reverse_weight, length_penalty)
            for m in modes:
                out[m].extend(part[m])
        return out if starts is None else (out, starts.tolist())

    # -------------------------------------------------------------------------------- timings
    def set_profiling(self, on, gemm_only: bool = False):
        """HIP-event stage timing: every stage, or (gemm_only) just the GEMM launches the roofline figure needs."""
        check(self.lib.rvb_set_profiling(self.handle, 0 if not on else 2 if gemm_only else 1))

    def reset_timings(self):
        check(self.lib.rvb_reset_timings(self.handle))

    def timing(self, name: str):
        ms, fl, n = C.c_double(0), C.c_double(0), C.c_int64(0)
        check(self.lib.rvb_get_timing(self.handle, name.encode(), C.byref(ms), C.byref(fl), C.byref(n)))
        by = C.c_double(0)
        check(self.lib.rvb_get_timing_bytes(self.handle, name.encode(), C.byref(by)))
        return {"ms": ms.value, "flops": fl.value, "launches": n.value, "bytes": by.value}
