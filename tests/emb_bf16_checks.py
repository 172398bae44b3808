"""Stage-by-stage and structural check of a bf16 run of the speaker-embedding network on its OWN stored tensors: every stage's
stored input, exact in bf16, goes through the fp64 stage function of oracle/emb_bf16_ref.py, and the stored output must lie inside
that stage's derived bound (the kernel tests' bound, tests/emb_conv_ref.py and tests/gemm_ref.py, which already contains the
output's bf16 half ulp) -- every element, no fraction may fail.  Used on the engine's tensors (tests/test_emb_bf16_gpu.py, through
DiarEngine.emb_tap) and, without a GPU, on the restatement's own and on mutants of them (tests/test_emb_bf16_ref.py).  Nothing here
needs a GPU.

Tensors T by the names of rvd_get_emb_tap (include/rvd.h): padded NHWC [B][F + 2][T + 2][C].  A block whose "tmp" is missing ran as
one kernel (conv_block.hip): it has no stored intermediate and is listed in the figures' "unchecked" for the caller, who checks it
through the run that stores it.  The structure checks need no bound: zero borders, every block's input bit-equal to what the block
before it stored, the pooling's input bit-equal to the last block's output."""
import numpy as np

from oracle import emb_bf16_ref as E


def _ratio(got, ref, tol):
    return np.abs(np.asarray(got, np.float64) - ref) / tol


def check_structure(T):
    """-> list of messages: a border row or column that is not zero, a block input that is not the previous block's stored output"""
    bad = []
    for name, P in T.items():
        if isinstance(P, np.ndarray) and P.ndim == 4 and (name in ("stem", "trunk") or name.startswith("s")):
            for what, sl in (("first row", P[:, 0]), ("last row", P[:, -1]), ("first column", P[:, :, 0]), ("last column", P[:, :, -1])):
                if np.any(sl != 0):
                    bad.append("%s: %s of the border is not zero (%d values)" % (name, what, int((sl != 0).sum())))
    prev, prev_name = T.get("stem"), "stem"
    for li, bi in E.block_list():
        x = T.get(E.tname(li, bi, "x"))
        if x is not None and prev is not None and not np.array_equal(x, prev):
            bad.append("%s is not %s bit for bit" % (E.tname(li, bi, "x"), prev_name))
        prev, prev_name = T.get(E.tname(li, bi, "out")), E.tname(li, bi, "out")
    if "trunk" in T and prev is not None and not np.array_equal(T["trunk"], prev):
        bad.append("trunk is not %s bit for bit" % prev_name)
    return bad


def check_stages(sd, T, masks=None, emb=None, feats=None, mean=None, blocks=None, Wt=None, structure=True):
    """sd: the embedding state dict; T: the stored tensors of one pass; masks [n][589] and emb [n][256]: the pass's items and their
    embeddings (None: pooling and seg_1 are not checked); feats [B][T][80], mean [B][80] (default T's own "feats" / "mean"; None:
    the stem is not checked); blocks: the (stage, block) pairs to check (default all).
    -> (figures, failures): per stage the worst |err| / bound ratio, "unchecked": the blocks without a stored intermediate; and a
    list of messages, one per stage outside its bound or structure fault.  Callers assert that the list is empty."""
    Wt = Wt or E.weights(sd)
    fig, bad, unchecked = {}, [], []

    def within(name, got, ref, tol):
        r = _ratio(got, ref, tol)
        fig[name] = float(r.max())
        if not r.max() <= 1.0:
            bad.append("%s: %d of %d elements outside the bound, worst %.3g x the bound" % (name, int((~(r <= 1)).sum()), r.size, r.max()))

    feats = T.get("feats") if feats is None else feats
    mean = T.get("mean") if mean is None else mean
    if feats is not None and mean is not None and "stem" in T:
        within("stem", E.interior(T["stem"]), *E.stem_stage(Wt, feats, mean))
    for li, bi in (E.block_list() if blocks is None else blocks):
        k = Wt["blocks"][(li, bi)]
        x, tmp, sc, out = (T.get(E.tname(li, bi, w)) for w in ("x", "tmp", "sc", "out"))
        if x is None or out is None:
            continue
        if tmp is None:
            unchecked.append([li, bi])
            continue
        xi = E.interior(x)
        within(E.tname(li, bi, "conv1"), E.interior(tmp), *E.conv_stage(xi, k["w1"], k["b1"], stride=k["stride"]))
        if sc is not None:
            within(E.tname(li, bi, "shortcut"), E.interior(sc), *E.conv_stage(xi, k["wsc"], k["bsc"], stride=k["stride"], relu=False))
            ref = E.conv_stage(E.interior(tmp), k["w2"], k["b2"], res=E.interior(sc))
        elif k["wsc"] is not None:           # the shortcut in the K loop: K counts its channels, the bias is b_2 + b_sc
            ref = E.conv_stage(E.interior(tmp), k["w2"], k["b2sc"], x2=xi, w2=k["wsc"])
        else:
            ref = E.conv_stage(E.interior(tmp), k["w2"], k["b2"], res=xi)
        within(E.tname(li, bi, "conv2"), E.interior(out), *ref)
    if masks is not None and "trunk" in T and "stats" in T:
        within("tstp", T["stats"], *E.tstp_stage(E.interior(T["trunk"]), T["item_b"], masks))
        if emb is not None:
            within("seg_1", emb, *E.seg1_stage(np.asarray(T["stats"], np.float32), *Wt["seg1"]))
    if structure:
        bad += check_structure(T)
    fig["unchecked"] = unchecked
    return fig, bad


def summary(fig):
    """the worst ratio per kind of stage, for _record and the logs"""
    out = {}
    for k, v in fig.items():
        if k == "unchecked":
            continue
        kind = k.split(".")[1] if "." in k else k
        key = ("stage%s_%s" % (k[1], kind)) if "." in k else kind
        out[key] = max(out.get(key, 0.0), v)
    return out
