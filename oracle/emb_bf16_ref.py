"""TEST INFRASTRUCTURE ONLY (oracle) -- never imported by the product path.

A restatement of oracle/diar_ref.py's speaker-embedding network (resnet34_trunk, tstp, seg_1 on hamming_fbank features) in fp64
arithmetic that rounds to bf16 (round to nearest even, tests/util.py bf16_round: fp64 -> fp32 -> bf16, the engine's accumulators
being fp32) exactly where the bf16 engine stores bf16, and nowhere else.  It is the yardstick of what bf16 STORAGE costs: the
engine's distance from the fp32 oracle is held to this restatement's distance from it (tests/test_emb_bf16_gpu.py, fixture
tests/golden/emb_bf16_yardstick.json written by oracle/gen_golden_emb_bf16.py).

Storage points (reverb_amd/csrc/..., read from run_trunk, diar_engine.hip:604-736, embed_impl, :738-835, and finalize_embedding /
pack_conv_bn / pack_fused_shortcut, :423-549):

  tensor                                      stored by                                            read by
  stem output   act[0][0] [B][82][1000][32]   resnet.hip:98-105 (emb_conv1_kernel, pack2_bf16),     first block of stage 1
                                              called at diar_engine.hip:609
  tmp           first convolution of a block  resnet.hip:343 (direct), conv_stream.hip:291,        the block's second convolution (:713 / :725)
                after bias and ReLU           conv_row64.hip:202, conv_gemm.hip:289-290 -- through
                                              run_conv, diar_engine.hip:696; conv_s2.hip:179 (:693)
  tmp of a      the same value, rounded in    conv_block.hip:185 (the intermediate goes to LDS      the same kernel's second convolution
  one-kernel    LDS instead of HBM            through pack2_bf16), called at diar_engine.hip:640
  block
  sc            the 1x1 / stride-2 projection conv_s2.hip:180 (stage 2's opener, :693) or           the second convolution's residual (:725)
                shortcut, where it is a       run_conv(Bk.sc), diar_engine.hip:721
                launch of its own
  (no sc)       stages 3 and 4: the shortcut  -- (conv_gemm.hip:110-119 reads x through              --
                rides in the second           ConvArgs::in2, diar_engine.hip:700-713: its
                convolution's K loop          products join the fp32 accumulator unrounded)
  out           every block's output after    the same store lines as tmp; conv_block.hip:211       next block, or tstp_pool (:821)
                bias, residual and ReLU
  stats         TSTP mean and std             resnet.hip:486-487 (Cvt<T>::from_f32), :821          seg_1 GEMM (:823-829)
  weights       every 3x3 and 1x1 convolution: w * (gamma / sqrt(var + eps)) multiplied in fp32 (resnet.hip:418 / :426 / :436) and
                rounded once by pack_T (diar_engine.hip:154-161, convert_f32, RNE) at :440 (direct layout), :448 (implicit-GEMM layout)
                and :495 (rows [9 cout | cin_sc] with the shortcut's weights); seg_1.weight at :543

Not rounded: the fbank features and the per-window means (fp32: diar_engine.hip:1065 / :1068, subtracted in fp32 at resnet.hip:65);
the stem's folded weights and bias (up_f32, :519-520); every folded bias (:466; b_2 + b_sc summed in fp32, :492 / :496); the masks
and the TSTP sums (fp64 in the kernel, resnet.hip:475-484, with fp32 v1 / den, :466-469, and sqrtf, :487: modelled as stated
there); the embedding (fp32 output of the GEMM, g.out_f32 = 1, :827).

Forms.  One dispatch choice changes values: per block, whether the projection shortcut is fused into the second convolution's K
loop (stages 3 and 4 by default; lab switch RVD_CONV_SC_FUSE=0 stores it).  Everything else -- direct / stream / row64 / implicit
GEMM narrow or wide, the one-kernel block, the stride-2 opener -- is a summation order; the jitter of Storage stands for it.

The stage functions below are what the network function is made of; each can be run on given inputs (the engine's own stored
tensors, exact in bf16) and returns the fp64 result BEFORE the output rounding together with the stage's derived bound, which
they share with the kernel tests (tests/emb_conv_ref.py, tests/gemm_ref.py).  Tensors are NHWC with their zero border of one
pixel, [B][F + 2][T + 2][C], under the names of rvd_get_emb_tap (include/rvd.h).
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch
import torch.nn.functional as F

from . import diar_ref as R
from .diar_bf16_ref import Storage, _np          # noqa: F401  (Storage: the rounding of every stored tensor, with jitter and mutants)
from . import diar_bf16_ref as _B                 # puts tests/ on sys.path

import emb_conv_ref as CR            # noqa: E402  (tests/: the fp64 stage references and bounds shared with the kernel tests)
import gemm_ref as GR                # noqa: E402

BLOCKS = (3, 4, 6, 3)
EPS = np.float32(1e-5)
# blocks (stage, block), 0-based, whose projection shortcut rides in the second convolution's K loop by default
DEFAULT_FUSED = frozenset({(2, 0), (3, 0)})


def f32(a):
    return np.asarray(a, np.float32)


def tname(li, bi, what):
    return "s%db%d.%s" % (li + 1, bi, what)


def block_list():
    return [(li, bi) for li, n in enumerate(BLOCKS) for bi in range(n)]


def stage_dims(nfr=998, m=32):
    """-> [(F, T, C)] of the four stages (80 x 998 x 32, 40 x 499 x 64, 20 x 250 x 128, 10 x 125 x 256)"""
    d = [(80, nfr, m)]
    for _ in range(3):
        d.append(((d[-1][0] - 1) // 2 + 1, (d[-1][1] - 1) // 2 + 1, d[-1][2] * 2))
    return d


# ------------------------------------------------------------------------------------ weights
def fold(sd, conv, bn):
    """Conv2d weight + eval-mode BatchNorm folded as pack_conv_bn does, in fp32: -> (w * sc [cout][cin][k][k] fp32, bias fp32)"""
    w = f32(_np(sd, conv + ".weight"))
    g, b, m, v = (f32(_np(sd, bn + s)) for s in (".weight", ".bias", ".running_mean", ".running_var"))
    sc = f32(g / np.sqrt(f32(v + EPS)))
    return f32(w * sc[:, None, None, None]), f32(b - f32(m * sc))


def weights(sd, st: Optional[Storage] = None):
    """-> dict(stem=(w fp32 [32][1][3][3], bias), blocks={(li, bi): dict(w1, b1, w2, b2, wsc, bsc, b2sc, stride)}, seg1=(w, bias)):
    convolution weights and seg_1.weight as stored (st.weight: rounded once after the fp32 fold), the stem's and every bias fp32"""
    st = st or Storage("bf16")
    out = dict(stem=fold(sd, "resnet.conv1", "resnet.bn1"), blocks={})
    for li, bi in block_list():
        p = "resnet.layer%d.%d" % (li + 1, bi)
        w1, b1 = fold(sd, p + ".conv1", p + ".bn1")
        w2, b2 = fold(sd, p + ".conv2", p + ".bn2")
        blk = dict(w1=st.weight(w1), b1=b1, w2=st.weight(w2), b2=b2, wsc=None, bsc=None, b2sc=None, stride=2 if (bi == 0 and li > 0) else 1)
        if (p + ".shortcut.0.weight") in sd:
            ws, bs = fold(sd, p + ".shortcut.0", p + ".shortcut.1")
            blk.update(wsc=st.weight(ws), bsc=bs, b2sc=f32(b2 + bs))
        out["blocks"][(li, bi)] = blk
    out["seg1"] = (st.weight(f32(_np(sd, "resnet.seg_1.weight"))), f32(_np(sd, "resnet.seg_1.bias")))
    return out


# ------------------------------------------------------------------------------------ stages (on stored tensors)
def interior(P):
    return P[:, 1:-1, 1:-1, :]


def padded(x):
    return np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))


def stem_stage(Wt, feats, mean):
    """The stem from the stored fbank frames feats [B][T][80] and per-window means [B][80] (both fp32; the subtraction is the fp32
    one the kernel makes) -> (fp64 [B][80][T][32] before rounding, bound)"""
    w, b = Wt["stem"]
    plane = f32(f32(feats) - f32(mean)[:, None, :])
    refs, tols = zip(*[CR.stem_ref(plane[i].T, w, b) for i in range(plane.shape[0])])
    ref, tol = np.stack(refs), np.stack(tols)
    return ref, CR.conv_bound(CR.BF16, ref, tol)


def conv_stage(x, w, bias, stride=1, relu=True, res=None, x2=None, w2=None):
    """One convolution from its stored input x [B][Fi][Ti][Cin] (interior), weights as stored, bias fp32, the stored residual res
    [B][Fo][To][Cout] and / or the fused 1x1 / stride-2 shortcut (x2 [B][Fi2][Ti2][Cin2], w2 [Cout][Cin2][1][1]; K then counts its
    channels) -> (fp64 before rounding, bound (K + 2) u sum|terms| + half a bf16 ulp)"""
    op = dict(x=x, w=w, bias=f32(bias), res=res, x2=x2, w2=None if w2 is None else np.asarray(w2).reshape(w2.shape[0], -1), stride=stride,
              stride2=2)
    ref, tol = CR.conv_ref(op, relu)
    return ref, CR.conv_bound(CR.BF16, ref, tol)


def frame_weights(masks, TT):
    """masks [n][589] -> [n][TT]: nearest resampling, the map taken from torch itself"""
    masks = np.asarray(masks)
    return masks[:, CR.nearest_map(masks.shape[1], TT)]


def tstp_stage(trunk, item_b, masks):
    """TSTP from the stored stage-4 output trunk [B][F][TT][C] (interior) and the items' masks -> (fp64 [n][2 C F] before rounding,
    bound), feature index = channel * F + f, mean | std, at the TSTP kernel test's bound"""
    B_, Fq, TT, C = trunk.shape
    w = frame_weights(masks, TT)
    ref, tol = [], []
    for it, b in enumerate(item_b):
        mean, std, mt, stl = CR.tstp_ref(CR.BF16, np.asarray(trunk[b], np.float64).transpose(2, 0, 1), w[it])
        ref.append(np.concatenate([mean.reshape(-1), std.reshape(-1)]))
        tol.append(np.concatenate([np.broadcast_to(mt, mean.shape).reshape(-1), np.broadcast_to(stl, std.shape).reshape(-1)]))
    return np.stack(ref), np.stack(tol)


def seg1_stage(stats, w, bias):
    """stats [n][2 C F] as stored, seg_1.weight as stored, bias fp32 -> (fp64 embedding [n][256], bound of the GEMM with fp32 output)"""
    M, K = stats.shape
    case = dict(form="seg_1", dtype=GR.BF16, M=M, N=w.shape[0], K=K, lda=K, ldw=K, ldc=w.shape[0], a_row0=0, alpha=1.0, act=GR.ACT_NONE,
                out="f32", in_fp8=False, inplace=False, A=np.ascontiguousarray(stats).reshape(-1), W=np.asarray(w), bias=f32(bias), res=None,
                ldres=0)
    return GR.reference(case), GR.bound(case)


# ------------------------------------------------------------------------------------ the network
def _conv_t(P, w, stride, k):
    """fp64 convolution with torch: P padded NHWC; 3x3 reads the border as its padding (whatever it holds), 1x1 the interior"""
    x = torch.from_numpy(np.ascontiguousarray((P if k == 3 else interior(P)).transpose(0, 3, 1, 2)))
    y = F.conv2d(x, torch.from_numpy(np.asarray(w, np.float64)), stride=stride)
    return y.numpy().transpose(0, 2, 3, 1)


def tstp_kernel_model(trunk, item_b, masks):
    """TSTP with the kernel's fp32 steps (resnet.hip:466-487): fp32 s1, s2, v1 = s1 + 1e-8f, den = v1 - s2 / v1 + 1e-8f; fp64 sums
    a1 = sum w x, a2 = sum w x^2; mean = (float)(a1 / v1), std = sqrtf((float)(max(a2 - 2 m a1 + m^2 s1, 0) / den)) -> [n][2 C F]"""
    B_, Fq, TT, C = trunk.shape
    w = f32(frame_weights(masks, TT))
    out = np.zeros((len(item_b), 2 * C * Fq))
    for it, b in enumerate(item_b):
        s1, s2 = np.float32(w[it].sum(dtype=np.float32)), np.float32((w[it] * w[it]).sum(dtype=np.float32))
        v1 = np.float32(s1 + np.float32(1e-8))
        den = np.float32(np.float32(v1 - np.float32(s2 / v1)) + np.float32(1e-8))
        xv = np.asarray(trunk[b], np.float64).transpose(2, 0, 1)              # [C][F][TT]
        wv = w[it].astype(np.float64)
        a1, a2 = (xv * wv).sum(-1), (xv * xv * wv).sum(-1)
        m = a1 / np.float64(v1)
        q = np.maximum(a2 - 2.0 * m * a1 + m * m * np.float64(s1), 0.0)
        mean = f32(m).astype(np.float64)
        std = np.sqrt(f32(q / np.float64(den))).astype(np.float32).astype(np.float64)
        out[it] = np.concatenate([mean.reshape(-1), std.reshape(-1)])
    return out


def wespeaker_bf16(sd, feats, wins, masks, taps: Optional[dict] = None, storage: str = "bf16", jitter_seed: Optional[int] = None,
                   fused=DEFAULT_FUSED, mutant: Optional[dict] = None):
    """The embedding network as the bf16 engine stores it.  feats {window: [T][80] fp32, mean-subtracted (diar_ref.hamming_fbank)},
    wins int [n] and masks [n][589]: the items -> embeddings fp64 [n][256].  storage 'none' is the fp64 oracle, 'trunc' truncates
    at the same points (a mutant); jitter_seed: see Storage.  fused: the blocks whose shortcut rides in the K loop.
    taps (dict): every stored tensor under rvd_get_emb_tap's names, plus 'windows' and 'item_b'.
    mutant (dict, optional), deliberately wrong networks for tests/test_emb_bf16_ref.py:
      stale_residual=(li, bi)     that block adds the output of the block BEFORE LAST instead of its input (the stale rotating buffer)
      dirty_border=(name, values) the stored tensor `name` keeps `values` [B][F + 2][C] in its last border column instead of zeros
      round_fused_sc=True         a fused shortcut is rounded to bf16 before it is added (one rounding too many)"""
    st = Storage(storage, jitter_seed)
    mutant = mutant or {}
    T = {} if taps is None else taps
    Wt = weights(sd, st)
    uniq = sorted(set(int(w) for w in wins))
    item_b = np.array([uniq.index(int(w)) for w in wins])
    T["windows"], T["item_b"] = np.array(uniq, np.int64), item_b
    x = np.stack([np.asarray(feats[w], np.float64) for w in uniq])            # [B][T][80]

    def keep(name, y):
        """store: round the interior, restore the zero border (or the mutant's)"""
        P = padded(st(name, y))
        if mutant.get("dirty_border") and mutant["dirty_border"][0] == name:
            P[:, :, -1, :] = mutant["dirty_border"][1]
        T[name] = P
        return P

    w, b = Wt["stem"]
    plane = padded(x.transpose(0, 2, 1)[..., None])                           # [B][82][T + 2][1]
    P = keep("stem", np.maximum(_conv_t(plane, w, 1, 3) + b.astype(np.float64), 0.0))
    outs = []
    for li, bi in block_list():
        k = Wt["blocks"][(li, bi)]
        T[tname(li, bi, "x")] = P
        tmp = keep(tname(li, bi, "tmp"), np.maximum(_conv_t(P, k["w1"], k["stride"], 3) + k["b1"].astype(np.float64), 0.0))
        acc = _conv_t(tmp, k["w2"], 1, 3)
        if k["wsc"] is None:
            res = interior(P)
            if mutant.get("stale_residual") == (li, bi):
                res = interior(outs[-2])
            acc = acc + k["b2"].astype(np.float64) + res
        elif (li, bi) in fused:
            sc = _conv_t(P, k["wsc"], k["stride"], 1)
            if mutant.get("round_fused_sc"):
                sc = st(tname(li, bi, "sc"), sc + k["bsc"].astype(np.float64)) - k["bsc"].astype(np.float64)
            acc = acc + sc + k["b2sc"].astype(np.float64)
        else:
            sc = keep(tname(li, bi, "sc"), _conv_t(P, k["wsc"], k["stride"], 1) + k["bsc"].astype(np.float64))
            acc = acc + k["b2"].astype(np.float64) + interior(sc)
        P = keep(tname(li, bi, "out"), np.maximum(acc, 0.0))
        outs.append(P)
    T["trunk"] = P
    T["stats"] = stats = st("stats", tstp_kernel_model(interior(P), item_b, masks))
    ws, bs = Wt["seg1"]
    return stats @ np.asarray(ws, np.float64).T + bs.astype(np.float64)


def forms_of(fused=DEFAULT_FUSED):
    """the shortcut form per block as rvd_get_emb_tap 'forms' reports it: 0 identity, 1 stored, 3 in the K loop"""
    return {(li, bi): (0 if not (bi == 0 and li > 0) else 3 if (li, bi) in fused else 1) for li, bi in block_list()}


# ------------------------------------------------------------------------------------ metrics
METRICS = ("one_minus_cos_max", "one_minus_cos_mean", "emb_rel_l2_max", "emb_rel_l2_mean", "trunk_rel_l2_max", "trunk_rel_l2_mean")


def metrics(got_emb, got_trunk, want_emb, want_trunk, active=None) -> Dict[str, float]:
    """A run against the fp32 oracle's, over the items with a non-empty mask (`active`, default all): 1 - cos of the embeddings
    (max, mean), their relative L2 error (max, mean), and the relative L2 error of the stage-4 output per window (max, mean).
    got_trunk / want_trunk [B][10][125][256] (interior, NHWC)."""
    g, w = np.asarray(got_emb, np.float64), np.asarray(want_emb, np.float64)
    if active is not None:
        g, w = g[active], w[active]
    cos = (g * w).sum(1) / (np.linalg.norm(g, axis=1) * np.linalg.norm(w, axis=1))
    rel = np.linalg.norm(g - w, axis=1) / np.linalg.norm(w, axis=1)
    gt, wt = np.asarray(got_trunk, np.float64), np.asarray(want_trunk, np.float64)
    B_ = gt.shape[0]
    tr = np.linalg.norm((gt - wt).reshape(B_, -1), axis=1) / np.linalg.norm(wt.reshape(B_, -1), axis=1)
    return dict(one_minus_cos_max=float((1.0 - cos).max()), one_minus_cos_mean=float((1.0 - cos).mean()),
                emb_rel_l2_max=float(rel.max()), emb_rel_l2_mean=float(rel.mean()),
                trunk_rel_l2_max=float(tr.max()), trunk_rel_l2_mean=float(tr.mean()))


def outside_yardstick(m, yard, factor):
    """-> list of the metrics of m that exceed factor[k] x yardstick[k]"""
    return [k for k in METRICS if m[k] > factor[k] * yard[k]]
