"""Without a GPU: the bf16-storage restatement of the speaker-embedding network (oracle/emb_bf16_ref.py), its fixture
(tests/golden/emb_bf16_yardstick.json) and the proof that the bounds of tests/test_emb_bf16_gpu.py bite -- mutant restatements on
the same case, each of which at least one new check rejects, with the old bar (cos > 0.999, tests/test_diar_gpu.py
test_embedding_bf16_close_to_oracle) beside it:

  mutant                                           end-to-end bound   stage / structure checks                        old cos > 0.999
  truncation instead of RNE at every store         rejects, all six   reject: the stem and every convolution (35      accepts
                                                   (rel. L2 x 14,     stages)                                         (1 - cos 3.4e-5)
                                                   1 - cos x 2.6)
  stage 3, block 2 adds the output of the block    rejects, all six   reject: s3b2.conv2, and only it (the stored     rejects
    before last (the stale rotating buffer)        (rel. L2 0.16)       residual is not what was added)               (1 - cos 1.0e-2)
  one border column of a stage-1 buffer holds      at the edge: one   reject: structure (s1b0.out's last column) and  accepts
    the previous pass's values                     metric at 1.25 x     s1b1.conv1 at the pixels that read it
                                                   (not relied on)
  the fused shortcut rounded to bf16 before the    accepts            reject: s3b0.conv2 and s4b0.conv2 (two half     accepts
    add                                                                 ulps where the bound holds one)

The old bar lets three of the four through; the end-to-end bound alone lets the last one (and, but for a hair, the third) through:
those are what the stage and structure checks are for."""
import json

import numpy as np
import pytest

from oracle import emb_bf16_ref as E
from oracle import gen_golden_emb_bf16 as G
import emb_bf16_checks as CK


@pytest.fixture(scope="module")
def yard():
    with open(G.FIXTURE) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def case():
    return G.make_case()


@pytest.fixture(scope="module")
def runs(case):
    """the plain run and the six jittered ones, as the generator makes them; the plain run's embeddings and tensors are kept"""
    keep = {}
    return G.all_runs(case, keep), keep


def _old_bar_accepts(case, emb):
    a = case["active"]
    g, w = emb[a], case["want"][a].astype(np.float64)
    cos = (g * w).sum(1) / (np.linalg.norm(g, axis=1) * np.linalg.norm(w, axis=1))
    return bool(cos.min() > 0.999)


def _stages(case, emb, T, **kw):
    B = len(T["windows"])
    feats = np.stack([case["feats"][int(w)] for w in T["windows"]])
    return CK.check_stages(case["emb_sd"], T, case["masks"], emb, feats=feats, mean=np.zeros((B, 80), np.float32), **kw)


def test_storage_none_is_the_oracle(case):
    """fp64 without rounding against the fp32 oracle: the embedding at the f32 engine test's bound (2e-3 of the largest value), the
    all-zero mask gives seg_1's bias"""
    emb, T, m = G.restatement(case, storage="none")
    assert np.abs(emb - case["want"]).max() < 2e-3 * np.abs(case["want"]).max()
    assert m["one_minus_cos_max"] < 1e-9 and m["trunk_rel_l2_max"] < 1e-5, m
    idx = int(np.where(~case["active"])[0][0])
    assert np.abs(emb[idx] - case["emb_sd"]["resnet.seg_1.bias"]).max() < 1e-5


def test_regenerating_the_runs_reproduces_the_fixture(case, runs, yard):
    """Figures may move by 1e-3 of their value on another machine (another build of torch may order the fp32 oracle's sums
    differently); on the machine that wrote the fixture they are reproduced exactly.  The factor is the stated rule."""
    doc = G.document(case, runs[0])
    assert sorted(doc["runs"]) == sorted(yard["runs"]) and len(doc["runs"]) == 1 + G.JITTERS
    for name, r in doc["runs"].items():
        for k in E.METRICS:
            assert r[k] == pytest.approx(yard["runs"][name][k], rel=1e-3), (name, k)
    for k in E.METRICS:
        vals = [r[k] for r in yard["runs"].values()]
        assert yard["yardstick"][k] == max(vals)
        assert yard["factor"][k] == pytest.approx(max(1.25, 1.06 * max(vals) / float(np.median(vals))), rel=1e-12)
    assert yard["active_items"] == int(case["active"].sum()) == 8 and yard["items"] == 9


def test_the_restatement_against_itself_meets_every_bound(runs, yard):
    """plain and each jittered run inside factor x yardstick, per metric; and a jitter seed the fixture has not seen"""
    for name, m in runs[0].items():
        assert not E.outside_yardstick(m, yard["yardstick"], yard["factor"]), (name, m)


def test_a_fresh_jitter_run_meets_the_end_to_end_bound_and_every_stage_bound(case, yard):
    emb, T, m = G.restatement(case, jitter_seed=1001)
    assert not E.outside_yardstick(m, yard["yardstick"], yard["factor"]), m
    fig, bad = _stages(case, emb, T)
    print("jittered run, worst ratios:", json.dumps(CK.summary(fig)))
    assert not bad, bad
    assert fig["unchecked"] == []
    assert _old_bar_accepts(case, emb)


def _verdict(case, yard, emb, T, m, **kw):
    e2e = E.outside_yardstick(m, yard["yardstick"], yard["factor"])
    fig, bad = _stages(case, emb, T, **kw)
    return e2e, bad, _old_bar_accepts(case, emb)


def test_truncation_is_rejected_end_to_end_and_by_every_stage(case, yard):
    """storage='trunc': bf16 by dropping bits at every storage point, a classic kernel slip.  Rejected by every end-to-end metric and
    by the stage check of every convolution; accepted by the old bar."""
    emb, T, m = G.restatement(case, storage="trunc")
    e2e, bad, old = _verdict(case, yard, emb, T, m, Wt=E.weights(case["emb_sd"]))
    print("truncation:", json.dumps(m), "old bar accepts:", old, "stage failures:", len(bad))
    assert sorted(e2e) == sorted(E.METRICS), (e2e, m)
    assert any(b.startswith("stem:") for b in bad) and any(b.startswith("s4b2.conv2:") for b in bad), bad
    assert old


def test_a_residual_from_the_stale_rotating_buffer_is_rejected(case, yard):
    """block 2 of stage 3 adds the output of the block before last -- what act[2][oi] held before this block overwrote it, the
    buffer a wrong `xi` rotation would hand it.  The stage check of that block's second convolution names it; the old bar accepts."""
    emb, T, m = G.restatement(case, mutant=dict(stale_residual=(2, 2)))
    e2e, bad, old = _verdict(case, yard, emb, T, m)
    print("stale residual:", json.dumps(m), "end-to-end rejects:", e2e, "old bar accepts:", old)
    assert [b.split(":")[0] for b in bad] == ["s3b2.conv2"], bad
    assert sorted(e2e) == sorted(E.METRICS), m
    assert not old                   # 1 - cos 1e-2: the one mutant of the four that the old bar notices too


def test_a_border_column_with_the_previous_pass_values_is_rejected(case, runs, yard):
    """the last border column of stage 1's first block output keeps values (here: the stem's last column) instead of zeros, as after a
    partial tile that wrote one pixel too far.  The structure check names the tensor, the stage check the convolution that read it."""
    vals = runs[1]["taps"]["stem"][:, :, -2, :]
    emb, T, m = G.restatement(case, mutant=dict(dirty_border=("s1b0.out", vals)))
    e2e, bad, old = _verdict(case, yard, emb, T, m, blocks=[(0, 0), (0, 1), (0, 2)])
    print("dirty border:", json.dumps(m), "end-to-end rejects:", e2e, "old bar accepts:", old)
    heads = [b.split(":")[0] for b in bad]
    assert "s1b1.conv1" in heads and any(h in ("s1b0.out", "s1b1.x") and "last column" in b for h, b in zip(heads, bad)), bad
    assert old


def test_a_fused_shortcut_rounded_once_too_often_is_rejected(case, yard):
    """the projection shortcut of stages 3 and 4 rounded to bf16 before it joins the second convolution's sum, as it was before it
    moved into the K loop: two half ulps where the bound of 9 C + C_sc terms holds one.  Only the stage checks of those two
    convolutions see it."""
    emb, T, m = G.restatement(case, mutant=dict(round_fused_sc=True))
    e2e, bad, old = _verdict(case, yard, emb, T, m, blocks=[(2, 0), (3, 0)], structure=False)
    print("fused shortcut rounded:", json.dumps(m), "end-to-end rejects:", e2e, "old bar accepts:", old)
    assert sorted(b.split(":")[0] for b in bad) == ["s3b0.conv2", "s4b0.conv2"], bad
    assert old


def test_structure_check_names_a_block_that_read_the_wrong_buffer(runs):
    """a block input that is not the previous block's stored output, and a pooling input that is not the last block's"""
    T = dict(runs[1]["taps"])
    T["s3b3.x"] = T["s3b1.out"]
    T["trunk"] = T["s4b1.out"]
    bad = CK.check_structure(T)
    assert bad == ["s3b3.x is not s3b2.out bit for bit", "trunk is not s4b2.out bit for bit"], bad
    assert CK.check_structure(runs[1]["taps"]) == []
