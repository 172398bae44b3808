"""Python host of the rvd_* C ABI (include/rvd.h): the two neural networks of the pyannote
diarization pipeline on one MI355X.  All compute is in librvb.so's HIP kernels; without the
library or without a GPU construction fails (no CPU fallback)."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import numpy as np

from . import _lib
from ._lib import DiarCfg, RvbError, fptr

DTYPES = {"f32": _lib.RVB_F32, "fp32": _lib.RVB_F32, "float32": _lib.RVB_F32, "bf16": _lib.RVB_BF16, "bfloat16": _lib.RVB_BF16, "fp8": _lib.RVB_FP8}


def _check(rc: int, what: str):
    if rc != 0:
        msg = _lib.load().rvd_last_error()
        raise RvbError(f"{what} failed ({rc}): {msg.decode('utf8', 'replace') if msg else ''}")


def _np32(v) -> Optional[np.ndarray]:
    if hasattr(v, "detach"):
        if not v.dtype.is_floating_point:
            return None
        v = v.detach().cpu().float().numpy()
    v = np.asarray(v)
    if v.dtype.kind != "f":
        return None
    return np.ascontiguousarray(v, dtype=np.float32)


def window_count(n_samples: int, window: int, step: int) -> int:
    """rvd_num_windows without the library: the full windows of n_samples samples plus one zero-padded tail."""
    n, window, step = int(n_samples), int(window), int(step)
    if n <= 0:
        return 0
    full = (n - window) // step + 1 if n >= window else 0
    tail = n < window or (n - window) % step > 0
    return full + (1 if tail else 0)


def window_layout(n_samples, window: int, step: int) -> np.ndarray:
    """The packed layout of rvd_upload_pcm_many, stated once more without the library: -> first_window int64 [n_rec].
    Recording r of n_samples[r] samples has W_r = window_count(n_samples[r]) windows and takes (W_r + window // step - 1) * step
    samples -- its own zero-padded length -- from sample first_window[r] * step on, so that its window w is global window
    first_window[r] + w and the window // step - 1 global indices between two recordings belong to nobody.  A recording of
    0 samples has no windows and takes no space (its entry is where the next recording starts).  One past the last valid global
    index -- the `total` of DiarEngine.upload_many -- is max(first_window[r] + W_r) over the recordings that have windows, else 0."""
    first, nxt = [], 0
    for n in n_samples:
        if int(n) < 0:
            raise ValueError("window_layout: negative length")
        W = window_count(n, window, step)
        first.append(nxt)
        if W > 0:
            nxt += W + int(window) // int(step) - 1
    return np.array(first, np.int64)


CPAD = 64            # padded width of the sinc_channels-wide activation tensors (csrc/diar_engine.hip rvd_create: cpad)


class DiarEngine:
    """segmentation (PyanNet) + embedding (WeSpeaker ResNet34) networks resident on one GPU."""

    def __init__(self, cfg: dict, segmentation_sd: Dict, embedding_sd: Optional[Dict] = None, dtype: str = "bf16",
                 device: int = 0):
        self.lib = _lib.load()
        self.cfg = dict(cfg)
        c = DiarCfg()
        c.dtype = DTYPES[dtype]
        for k in ("sample_rate", "window_samples", "step_samples", "sinc_filters", "sinc_channels", "lstm_hidden",
                  "lstm_layers", "linear_dim", "linear_layers", "num_classes", "emb_dim"):
            setattr(c, k, int(cfg[k]))
        c.emb_channels = int(cfg["emb_channels"]) if embedding_sd is not None else 0
        self.dtype = dtype
        self._h = C.c_void_p()
        self.device_index = int(device)
        _check(self.lib.rvd_create(C.byref(c), device, C.byref(self._h)), "rvd_create")
        for prefix, sd in (("segmentation.", segmentation_sd), ("embedding.", embedding_sd or {})):
            for name, v in sd.items():
                a = _np32(v)
                if a is None:
                    continue
                shape = (C.c_int64 * max(a.ndim, 1))(*a.shape)
                _check(self.lib.rvd_load_tensor(self._h, (prefix + name).encode(), fptr(a), shape, a.ndim), f"rvd_load_tensor({name})")
        _check(self.lib.rvd_finalize(self._h), "rvd_finalize")
        self.frames = self.lib.rvd_frames_per_window(self._h)
        self.num_classes = int(cfg["num_classes"])
        self.n_windows = 0
        self._last_W = 0                 # windows of the last rvd_segment / rvd_segment_windows call (what the taps hold)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self.lib.rvd_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ audio
    def num_windows(self, n_samples: int) -> int:
        return int(self.lib.rvd_num_windows(self._h, int(n_samples)))

    def resample(self, pcm: np.ndarray, sample_rate: int) -> np.ndarray:
        """int16 mono PCM at `sample_rate` -> int16 at the model's rate (torchaudio.functional.resample's kernel, on the device)."""
        pcm = np.ascontiguousarray(pcm, dtype=np.int16).reshape(-1)
        n = C.c_int64(0)
        _check(self.lib.rvd_resample_pcm(self._h, pcm.ctypes.data_as(C.POINTER(C.c_int16)), pcm.shape[0], int(sample_rate), None,
                                         C.byref(n)), "rvd_resample_pcm")
        out = np.empty(int(n.value), np.int16)
        _check(self.lib.rvd_resample_pcm(self._h, pcm.ctypes.data_as(C.POINTER(C.c_int16)), pcm.shape[0], int(sample_rate),
                                         out.ctypes.data_as(C.POINTER(C.c_int16)), C.byref(n)), "rvd_resample_pcm")
        return out[:int(n.value)]

    def upload(self, pcm: np.ndarray) -> int:
        pcm = np.ascontiguousarray(pcm, dtype=np.int16)
        _check(self.lib.rvd_upload_pcm(self._h, pcm.ctypes.data_as(C.POINTER(C.c_int16)), pcm.shape[0]), "rvd_upload_pcm")
        self.n_windows = self.num_windows(pcm.shape[0])
        return self.n_windows

    def upload_many(self, pcms):
        """Several recordings (int16 at the model's rate) in one upload and one front-end pass, packed as window_layout() states:
        -> (first_window int64 [n_rec], total).  Window w of recording r is global window first_window[r] + w for segment_windows,
        embed and emb_fbank; self.n_windows becomes `total`.  upload() afterwards returns to a single recording."""
        pcms = [np.ascontiguousarray(p, dtype=np.int16).reshape(-1) for p in pcms]
        n = len(pcms)
        ptrs = (C.POINTER(C.c_int16) * max(n, 1))(*[p.ctypes.data_as(C.POINTER(C.c_int16)) for p in pcms])
        lens = (C.c_int64 * max(n, 1))(*[p.shape[0] for p in pcms])
        first = np.zeros(max(n, 1), np.int64)
        total = C.c_int64(0)
        _check(self.lib.rvd_upload_pcm_many(self._h, ptrs, lens, n, first.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(total)),
               "rvd_upload_pcm_many")
        self.n_windows = int(total.value)
        return first[:n], self.n_windows

    def rerun_resident(self) -> int:
        """The recording of the last upload() is still in HBM: its front end again (what upload() does behind the copy)."""
        _check(self.lib.rvd_rerun_resident(self._h), "rvd_rerun_resident")
        return self.n_windows

    # ------------------------------------------------------------------ networks
    def segment(self, first: int = 0, n: Optional[int] = None, batch: int = 4096) -> np.ndarray:
        """log-probabilities over the powerset classes, [n, frames, classes]."""
        n = self.n_windows - first if n is None else n
        out = np.empty((n, self.frames, self.num_classes), np.float32)
        for b0 in range(0, n, batch):
            nb = min(batch, n - b0)
            _check(self.lib.rvd_segment(self._h, first + b0, nb, fptr(out[b0:b0 + nb])), "rvd_segment")
            self._last_W = nb
        return out

    def segment_classes(self, first: int = 0, n: Optional[int] = None, batch: int = 4096) -> np.ndarray:
        """argmax powerset class per frame, uint8 [n, frames] (the log-probabilities stay on the device)."""
        n = self.n_windows - first if n is None else n
        out = np.empty((n, self.frames), np.uint8)
        for b0 in range(0, n, batch):
            nb = min(batch, n - b0)
            _check(self.lib.rvd_segment(self._h, first + b0, nb, None), "rvd_segment")
            self._last_W = nb
            _check(self.lib.rvd_get_classes(self._h, out[b0:b0 + nb].ctypes.data_as(C.POINTER(C.c_uint8))), "rvd_get_classes")
        return out

    def segment_windows(self, windows, batch: int = 4096) -> np.ndarray:
        """segment() over a window list (after upload_many: global indices): [len(windows), frames, classes]."""
        windows = np.ascontiguousarray(windows, dtype=np.int64).reshape(-1)
        n = windows.shape[0]
        out = np.empty((n, self.frames, self.num_classes), np.float32)
        for b0 in range(0, n, batch):
            nb = min(batch, n - b0)
            _check(self.lib.rvd_segment_windows(self._h, windows[b0:].ctypes.data_as(C.POINTER(C.c_int64)), nb, fptr(out[b0:b0 + nb])),
                   "rvd_segment_windows")
            self._last_W = nb
        return out

    def segment_classes_windows(self, windows, batch: int = 4096) -> np.ndarray:
        """segment_classes() over a window list: uint8 [len(windows), frames]."""
        windows = np.ascontiguousarray(windows, dtype=np.int64).reshape(-1)
        n = windows.shape[0]
        out = np.empty((n, self.frames), np.uint8)
        for b0 in range(0, n, batch):
            nb = min(batch, n - b0)
            _check(self.lib.rvd_segment_windows(self._h, windows[b0:].ctypes.data_as(C.POINTER(C.c_int64)), nb, None), "rvd_segment_windows")
            self._last_W = nb
            _check(self.lib.rvd_get_classes(self._h, out[b0:b0 + nb].ctypes.data_as(C.POINTER(C.c_uint8))), "rvd_get_classes")
        return out

    def tap(self, name: str, n: int) -> np.ndarray:
        """debug taps of the last segment call (include/rvd.h rvd_get_tap): [n, rows per window, width] with the pad columns of the
        stored tensor; "stats" [n, 2]; "fsum" [sinc_filters]; "craw" [frames of the whole upload, sinc_filters].  n must be the window
        count of that call (its last batch): the engine copies that many windows."""
        c = self.cfg
        if self._last_W and n != self._last_W:
            raise ValueError("tap: the last segment call ran %d windows, not %d" % (self._last_W, n))
        p1 = ((c["window_samples"] - 251) // 10 + 1) // 3
        p2 = (p1 - 4) // 3
        H2, nf = 2 * c["lstm_hidden"], c["sinc_filters"]
        if name == "craw":
            n_pad = (self.n_windows - 1) * c["step_samples"] + c["window_samples"]
            shape = ((n_pad - 251) // 10 + 1, nf)
        elif name == "fsum":
            shape = (nf,)
        elif name == "stats":
            shape = (n, 2)
        else:
            rows, width = {"sincnet": (self.frames, c["sinc_channels"]), "lstm": (self.frames, H2), "a1": (p1, nf), "c2": (p1, CPAD),
                           "a2": (p2, CPAD), "c3": (p2, CPAD), "a3": (self.frames, CPAD), "lstm_prev": (self.frames, H2),
                           "linear0": (self.frames, c["linear_dim"]), "linear1": (self.frames, c["linear_dim"])}[name]
            shape = (n, rows, width)
        out = np.empty(shape, np.float32)
        _check(self.lib.rvd_get_tap(self._h, name.encode(), fptr(out)), "rvd_get_tap")
        return out

    def embed(self, windows: np.ndarray, masks: np.ndarray, batch: int = 1 << 20) -> np.ndarray:
        """one embedding per (window, mask) item: windows int64 [n], masks float32 [n, frames] -> [n, emb_dim]."""
        windows = np.ascontiguousarray(windows, dtype=np.int64)
        masks = np.ascontiguousarray(masks, dtype=np.float32)
        n = windows.shape[0]
        out = np.empty((n, int(self.cfg["emb_dim"])), np.float32)
        for b0 in range(0, n, batch):
            nb = min(batch, n - b0)
            _check(self.lib.rvd_embed(self._h, windows[b0:].ctypes.data_as(C.POINTER(C.c_int64)), fptr(masks[b0:b0 + nb]), nb,
                                      fptr(out[b0:b0 + nb])), "rvd_embed")
        return out

    def emb_fbank(self, window: int) -> np.ndarray:
        """80-bin hamming log-mel frames of one window as the ResNet sees them before mean subtraction."""
        out = np.empty((1200, 80), np.float32)
        n = C.c_int32()
        _check(self.lib.rvd_get_emb_fbank(self._h, int(window), fptr(out), C.byref(n)), "rvd_get_emb_fbank")
        return out[:n.value].copy()

    # ------------------------------------------------------------------ parity taps of the embedding pass
    EMB_BLOCKS = (3, 4, 6, 3)

    def set_emb_tap(self, on: bool = True):
        """Parity taps of the embedding trunk (include/rvd.h rvd_set_emb_tap): while on, every trunk pass of embed() keeps its stored
        tensors (at most 4 windows per pass); off releases them."""
        _check(self.lib.rvd_set_emb_tap(self._h, 1 if on else 0), "rvd_set_emb_tap")

    def emb_forms(self) -> dict:
        """-> dict(B, first_item, items, blocks=[(stage, block, kernel of conv 1, kernel of conv 2, shortcut form), ...]) of the last pass"""
        f = np.zeros(3 + 3 * 16, np.float32)
        _check(self.lib.rvd_get_emb_tap(self._h, b"forms", fptr(f), f.size), "rvd_get_emb_tap")
        f = f.astype(np.int64)
        blocks, k = [], 3
        for s, nb in enumerate(self.EMB_BLOCKS, start=1):
            for b in range(nb):
                blocks.append((s, b, int(f[k]), int(f[k + 1]), int(f[k + 2])))
                k += 3
        return dict(B=int(f[0]), first_item=int(f[1]), items=int(f[2]), blocks=blocks)

    def emb_tap(self, name: str) -> np.ndarray:
        """One stored tensor of the last trunk pass by name (rvd_get_emb_tap): padded tensors [B, F + 2, T + 2, C], "feats" [B, T, 80],
        "mean" [B, 80], "stats" [items, 2 C F], "windows" [B] and "item_b" [items] as int64."""
        fm = self.emb_forms()
        B, ni = fm["B"], fm["items"]
        nfr = (int(self.cfg["window_samples"]) - 400) // 160 + 1
        m = int(self.cfg["emb_channels"])
        dims = [(80, nfr, m)]
        for _ in range(3):
            F, T, Cc = dims[-1]
            dims.append(((F - 1) // 2 + 1, (T - 1) // 2 + 1, Cc * 2))
        pad = lambda s: (B, dims[s][0] + 2, dims[s][1] + 2, dims[s][2])
        if name in ("windows", "item_b"):
            out = np.zeros(B if name == "windows" else ni, np.float32)
            _check(self.lib.rvd_get_emb_tap(self._h, name.encode(), fptr(out), out.size), "rvd_get_emb_tap")
            return out.astype(np.int64)
        if name == "feats":
            shape = (B, nfr, 80)
        elif name == "mean":
            shape = (B, 80)
        elif name == "stem":
            shape = pad(0)
        elif name == "trunk":
            shape = pad(3)
        elif name == "stats":
            shape = (ni, 2 * dims[3][2] * dims[3][0])
        else:
            s, b = int(name[1]) - 1, int(name[3:name.index(".")])
            what = name[name.index(".") + 1:]
            shape = pad(s - 1 if (what == "x" and b == 0 and s > 0) else s)
        out = np.empty(shape, np.float32)
        _check(self.lib.rvd_get_emb_tap(self._h, name.encode(), fptr(out), out.size), "rvd_get_emb_tap")
        return out

    def set_linkage_workgroups(self, workgroups: int = 0):
        """Workgroups the clustering's merge loop may take (0 default = 16, 1, 2, 4, 8, 16).  The dendrogram does not depend on the count
        from 2 up; 1 selects another loop, which gives the same dendrogram bit for bit on input without tied distances and an equally
        valid one (every merge joins a closest pair) when distances tie -- there the two loops may take tied merges in another order."""
        _check(self.lib.rvd_set_linkage_workgroups(self._h, int(workgroups)), "rvd_set_linkage_workgroups")

    def emb_windows_per_pass(self) -> int:
        """distinct windows one pass of the embedding trunk takes (rvd_emb_windows_per_pass)"""
        n = self.lib.rvd_emb_windows_per_pass(self._h)
        if n < 0:
            _check(n, "rvd_emb_windows_per_pass")
        return int(n)

    def emb_fp8(self):
        """dtype="fp8" engines (ResNet34 stages 3-4 on e4m3 operands): (state 0 off / not calibrated, 1 calibrating, 2 active;
        activation scales [32]; values clipped at +-448 so far)."""
        st, n, cl = C.c_int32(0), C.c_int32(32), C.c_uint32(0)
        sc = np.zeros(32, np.float32)
        _check(self.lib.rvd_get_emb_fp8(self._h, C.byref(st), fptr(sc), C.byref(n), C.byref(cl)), "rvd_get_emb_fp8")
        return int(st.value), sc, int(cl.value)

    def set_emb_fp8_scales(self, scales: np.ndarray) -> None:
        """install the 32 activation scales and activate the fp8 trunk (rvd_set_emb_fp8_scales): no calibration pass follows"""
        sc = np.ascontiguousarray(scales, np.float32).reshape(-1)
        _check(self.lib.rvd_set_emb_fp8_scales(self._h, fptr(sc), len(sc)), "rvd_set_emb_fp8_scales")

    def centroid_linkage(self, X: np.ndarray) -> np.ndarray:
        """scipy.cluster.hierarchy.linkage(X, method="centroid", metric="euclidean") on the GPU (fp64)."""
        X = np.ascontiguousarray(X, dtype=np.float64)
        n, d = X.shape
        Z = np.zeros((max(n - 1, 0), 4), np.float64)
        f64 = C.POINTER(C.c_double)
        _check(self.lib.rvd_centroid_linkage(self._h, X.ctypes.data_as(f64), n, d, Z.ctypes.data_as(f64)), "rvd_centroid_linkage")
        return Z

    def centroid_linkage_many(self, Xs):
        """centroid_linkage for a list of point sets [n_p, d] in one call (rvd_centroid_linkage_many): -> list of Z [max(n_p - 1, 0), 4].
        Sets of fewer than 3 000 points are clustered together, one workgroup each, in one launch per stage; every dendrogram equals
        centroid_linkage's with set_linkage_workgroups(1), bit for bit."""
        Xs = [np.ascontiguousarray(X, dtype=np.float64) for X in Xs]
        if not Xs:
            return []
        for X in Xs:
            if X.ndim != 2:
                raise ValueError("centroid_linkage_many: every point set is [n, d]")
        ds = {X.shape[1] for X in Xs if X.shape[0] > 0}
        if len(ds) > 1:
            raise ValueError(f"centroid_linkage_many: point sets of different dimensions {sorted(ds)}")
        d = ds.pop() if ds else max(Xs[0].shape[1], 1)
        ns = np.array([X.shape[0] for X in Xs], np.int32)
        rows = np.maximum(ns.astype(np.int64) - 1, 0)
        allX = np.ascontiguousarray(np.concatenate([X.reshape(-1, d) for X in Xs], axis=0)) if ns.sum() else np.zeros((0, d))
        Z = np.zeros((int(rows.sum()), 4), np.float64)
        f64 = C.POINTER(C.c_double)
        _check(self.lib.rvd_centroid_linkage_many(self._h, allX.ctypes.data_as(f64), ns.ctypes.data_as(C.POINTER(C.c_int32)), len(Xs), int(d),
                                                  Z.ctypes.data_as(f64)), "rvd_centroid_linkage_many")
        ends = np.cumsum(rows)
        return [Z[e - r:e] for r, e in zip(rows, ends)]

    # ------------------------------------------------------------------ profiling
    def set_profiling(self, on: bool):
        _check(self.lib.rvd_set_profiling(self._h, 1 if on else 0), "rvd_set_profiling")

    def reset_timings(self):
        _check(self.lib.rvd_reset_timings(self._h), "rvd_reset_timings")

    def timing(self, name: str):
        ms, fl, n = C.c_double(), C.c_double(), C.c_int64()
        _check(self.lib.rvd_get_timing(self._h, name.encode(), C.byref(ms), C.byref(fl), C.byref(n)), "rvd_get_timing")
        return ms.value, fl.value, n.value
