"""The bf16 speaker-embedding network as run_trunk / embed_impl (csrc/diar_engine.hip) chain their kernels, held to what bf16 STORAGE
costs.

End to end: the engine's distance from the fp32 oracle (six metrics, oracle/emb_bf16_ref.py metrics, over the items with a
non-empty mask) must stay within factor x the distance of the bf16-storage restatement (fp64 arithmetic, rounded where the engine
stores bf16; yardstick = tests/golden/emb_bf16_yardstick.json, the maximum over a plain and six jittered runs; factor =
max(1.25, 1.06 x widest / median) of those runs = 1.25 for every metric).  tests/test_emb_bf16_ref.py shows without a GPU which
wrong networks this bound, the stage checks and the structure checks reject, and that the old bar (cos > 0.999) accepts most.

Stage by stage: every stored tensor of a trunk pass is read back (rvd_set_emb_tap / rvd_get_emb_tap), each stage's stored input --
exact in bf16 -- goes through the fp64 stage function, and every element of the stored output must lie inside that stage's
kernel-test bound (tests/emb_bf16_checks.py).  The blocks that run as one kernel store no intermediate: they, and the stride-2
opener, are checked in their two-launch forms (lab switches RVD_CONV_BLOCK=0, RVD_CONV_S2SC=0), whose outputs the default run must
equal bit for bit.  Structure, which no bound shows: zero borders, every block's input bit-equal to the previous block's output,
the documented dispatch.  The same through permuted items, several passes, the out-of-memory retry and a two-recording pack, whose
results must also equal the plain run's bit for bit."""
import json

import numpy as np
import pytest

from oracle import emb_bf16_ref as E
from oracle import gen_golden_emb_bf16 as G
from reverb_amd import synth_diar as SD
import emb_bf16_checks as CK
from test_diar_gpu import _record

pytestmark = pytest.mark.gpu

DIRECT, IGEMM, ROW64, STREAM, IGEMM_WIDE, BLOCK32, S2SC = 1, 2, 3, 4, 5, 6, 7
SC_NONE, SC_OWN, SC_OPENER, SC_K_LOOP = 0, 1, 2, 3
PROF = ("emb_stem", "emb_conv_32", "emb_conv_64", "emb_conv_128", "emb_conv_256", "emb_conv_s2_64", "emb_conv_s2_128", "emb_conv_s2_256",
        "emb_conv_sc", "emb_pool", "emb_linear", "emb_conv_igemm", "emb_conv_igemm_wide", "emb_conv_row64", "emb_conv_stream",
        "emb_conv_block", "emb_conv_s2sc", "emb_conv_sc_fused")


@pytest.fixture(scope="module")
def yard():
    with open(G.FIXTURE) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def case():
    c = G.make_case()
    c["seg_sd"] = SD.make_segmentation_sd(c["cfg"], 0)
    return c


def _engine(case, dtype="bf16"):
    from reverb_amd.diar_engine import DiarEngine
    return DiarEngine(case["cfg"], case["seg_sd"], case["emb_sd"], dtype=dtype)


def _read(eng, blocks=None):
    """every tensor the last trunk pass kept -> (T, forms)"""
    fm = eng.emb_forms()
    T = {k: eng.emb_tap(k) for k in ("feats", "mean", "stem", "trunk", "stats", "windows", "item_b")}
    for li, bi, k1, k2, sc in fm["blocks"]:
        if blocks is not None and (li - 1, bi) not in blocks:
            continue
        for what in ("x", "out") + (("tmp",) if k1 != BLOCK32 else ()) + (("sc",) if sc in (SC_OWN, SC_OPENER) else ()):
            T[E.tname(li - 1, bi, what)] = eng.emb_tap(E.tname(li - 1, bi, what))
    return T, fm


def _run(case, wins=None, masks=None, upload=None, blocks=None):
    """a fresh engine with the taps on: upload, embed -> (embeddings, T, forms)"""
    eng = _engine(case)
    (upload or (lambda e: e.upload(case["pcm"])))(eng)
    eng.set_emb_tap(True)
    emb = eng.embed(case["wins"] if wins is None else wins, case["masks"] if masks is None else masks)
    T, fm = _read(eng, blocks)
    eng.close()
    return emb, T, fm


@pytest.fixture(scope="module")
def plain(case):
    return _run(case)


def _same_bits(T, ref, rows=None, ref_rows=None, skip=("windows", "item_b", "stats")):
    """every tensor of T equals ref's bit for bit; rows / ref_rows: the windows of each that correspond"""
    for k, v in T.items():
        if k in skip:
            continue
        a = v if rows is None else v[rows]
        b = ref[k] if ref_rows is None else ref[k][ref_rows]
        assert np.array_equal(a, b), k


def _checked(case, emb, T, fm, what, expect_unchecked=(), masks=None):
    """the stage and structure checks on what the last pass left: its items are first_item .. first_item + items of the call"""
    i0, n = fm["first_item"], fm["items"]
    fig, bad = CK.check_stages(case["emb_sd"], T, (case["masks"] if masks is None else masks)[i0:i0 + n], emb[i0:i0 + n])
    s = CK.summary(fig)
    print("stages, %s: %s" % (what, json.dumps(s)))
    _record(test="emb_bf16_stages", case=what, **s)
    assert not bad, bad
    assert [tuple(u) for u in fig["unchecked"]] == list(expect_unchecked), fig["unchecked"]
    return s


# ------------------------------------------------------------------------------------ end to end
# measured on MI355X, engine against the fp32 oracle (yardstick; bound = 1.25 x yardstick), 3 windows, 8 items with a non-empty mask:
#   1 - cos            max 1.188e-5 (1.310e-5; 1.638e-5)   mean 8.557e-6 (8.507e-6; 1.063e-5)
#   embedding rel. L2  max 4.882e-3 (5.129e-3; 6.412e-3)   mean 4.128e-3 (4.125e-3; 5.156e-3)
#   stage-4 rel. L2    max 6.576e-3 (6.757e-3; 8.446e-3)   mean 6.451e-3 (6.469e-3; 8.087e-3)
# The engine sits inside the restatement's own spread; these figures are never used to set the bound (docs/tuning-log.md section 23).
def test_bf16_engine_within_the_storage_yardstick(case, yard, plain):
    emb, T, fm = plain
    assert list(T["windows"]) == yard["windows"] and fm["B"] == 3 and fm["items"] == yard["items"]
    m = G.run_metrics(case, emb.astype(np.float64), T)
    print("bf16 engine: %s; yardstick %s" % (json.dumps(m), json.dumps(yard["yardstick"])))
    _record(test="emb_bf16_engine_within_the_storage_yardstick", **m)
    for k in E.METRICS:
        assert m[k] <= yard["factor"][k] * yard["yardstick"][k], (k, m[k], yard["yardstick"][k])
    idx = int(np.where(~case["active"])[0][0])
    assert np.abs(emb[idx] - case["emb_sd"]["resnet.seg_1.bias"]).max() < 1e-5      # an all-zero mask pools to zero statistics


# ------------------------------------------------------------------------------------ stage by stage, structure
# measured on MI355X, worst |err| / bound per stage (plain run of 3 windows; the 1-window pass after it): stem 0.996; 0.996, stage 1
# (two-launch forms) 0.985 / 0.989, stage 2 opener 0.979 and its stored shortcut 0.995; 0.978, 0.995, stage 2 second convolutions
# 0.983; 0.979, stage 3 0.957 / 0.965; 0.965 / 0.963, stage 4 0.905 / 0.918; 0.876 / 0.895 (each within the output's half ulp, which
# is nearly all of these bounds), TSTP 0.980; 0.980, seg_1 1.1e-4; 1.2e-4 (fp32 output)
def test_every_stage_of_the_engine_is_inside_its_kernel_bound(case, plain):
    """the stem from the tapped features and means, every convolution from its stored input (first convolution, the opener's stored
    shortcut, the second convolution with its stored residual or with the shortcut in its K loop), TSTP from the stored stage-4
    output, seg_1 from the stored statistics; zero borders; every block's input is the previous block's output.  Stage 1's three
    blocks run as one kernel each and store no intermediate: the next test checks them."""
    emb, T, fm = plain
    _checked(case, emb, T, fm, "plain", expect_unchecked=[(0, 0), (0, 1), (0, 2)])


def test_dispatch_at_the_product_shape_is_the_documented_one(plain):
    """a silent fall-back to the direct kernel (or a block that stopped fusing) is noticed here, not in a benchmark"""
    want = ([(1, b, BLOCK32, BLOCK32, SC_NONE) for b in range(3)] +
            [(2, 0, S2SC, ROW64, SC_OPENER)] + [(2, b, ROW64, ROW64, SC_NONE) for b in range(1, 4)] +
            [(3, 0, IGEMM, IGEMM, SC_K_LOOP)] + [(3, b, IGEMM, IGEMM, SC_NONE) for b in range(1, 6)] +
            [(4, 0, IGEMM, IGEMM, SC_K_LOOP)] + [(4, b, IGEMM, IGEMM, SC_NONE) for b in range(1, 3)])
    assert plain[2]["blocks"] == want, plain[2]["blocks"]


def test_one_kernel_blocks_and_the_opener_equal_their_two_launch_forms(case, plain, monkeypatch, lab):
    """RVD_CONV_BLOCK=0 and RVD_CONV_S2SC=0: stage 1's blocks and stage 2's opener as two (three) launches of the single-convolution
    kernels.  Both convolutions of each are inside their bounds there, and the default run's stored tensors of those blocks -- and
    everything after them -- equal this run's bit for bit: the kernel tests claim that identity for the kernels, this for the engine."""
    monkeypatch.setenv("RVD_CONV_BLOCK", "0")
    monkeypatch.setenv("RVD_CONV_S2SC", "0")
    blocks = [(0, 0), (0, 1), (0, 2), (1, 0)]
    emb, T, fm = _run(case, blocks=blocks)
    assert [b[2:] for b in fm["blocks"][:4]] == [(STREAM, STREAM, SC_NONE)] * 3 + [(DIRECT, ROW64, SC_OWN)], fm["blocks"][:4]
    fig, bad = CK.check_stages(case["emb_sd"], T, blocks=blocks)
    s = CK.summary(fig)
    print("stages, two-launch forms: %s" % json.dumps(s))
    _record(test="emb_bf16_stages", case="two_launch_forms", **s)
    assert not bad, bad
    assert fig["unchecked"] == []
    assert np.array_equal(emb, plain[0])
    _same_bits({k: v for k, v in T.items() if not k.endswith(".tmp") or k == "s2b0.tmp"}, plain[1])


def test_borders_stay_zero_when_a_smaller_pass_follows_a_larger_one(case, plain):
    """three windows, then one OTHER window through the same buffers (their interiors stale, their borders never written again):
    zero borders, the chain of inputs and outputs, and every stage bound on what the second pass left"""
    eng = _engine(case)
    eng.upload(case["pcm"])
    eng.set_emb_tap(True)
    eng.embed(case["wins"], case["masks"])
    wins, masks = np.array([4, 4], np.int64), case["masks"][[0, 1]]
    emb = eng.embed(wins, masks)
    T, fm = _read(eng)
    eng.close()
    assert list(T["windows"]) == [4] and fm["items"] == 2
    fig, bad = CK.check_stages(case["emb_sd"], T, masks, emb)
    print("stages, smaller pass after a larger: %s" % json.dumps(CK.summary(fig)))
    assert not bad, bad


# ------------------------------------------------------------------------------------ other ways in
# Every embedding and every stored tensor must equal the plain run's bit for bit, and every stage is checked again on what these
# calls left behind.
def test_items_permuted_and_regrouped_give_the_same_bits(case, plain):
    perm = np.array([7, 3, 4, 5, 0, 6, 1, 2, 8])          # windows 5, 2, 2, 2, 0, 5, 0, 0, 5: window 5's and 0's items split up
    emb, T, fm = _run(case, case["wins"][perm], case["masks"][perm])
    assert np.array_equal(emb, plain[0][perm])
    order = [list(plain[1]["windows"]).index(w) for w in T["windows"]]
    assert list(T["windows"]) == [5, 2, 0]
    _same_bits(T, plain[1], ref_rows=order)
    assert np.array_equal(T["stats"], plain[1]["stats"][perm])
    _checked(case, emb, T, fm, "permuted", expect_unchecked=[(0, 0), (0, 1), (0, 2)], masks=case["masks"][perm])


def test_several_trunk_passes_give_the_same_bits(case, plain, monkeypatch, lab):
    """RVD_EMB_BATCH=2: windows 0 and 2 in one pass, the tail window in a second, which is what the taps hold"""
    monkeypatch.setenv("RVD_EMB_BATCH", "2")
    emb, T, fm = _run(case)
    assert np.array_equal(emb, plain[0])
    assert list(T["windows"]) == [int(case["wins"][-1])] and (fm["first_item"], fm["items"]) == (6, 3)
    _same_bits(T, plain[1], ref_rows=[2])
    assert np.array_equal(T["stats"], plain[1]["stats"][6:9])
    _checked(case, emb, T, fm, "two_passes", expect_unchecked=[(0, 0), (0, 1), (0, 2)])


def test_the_out_of_memory_retry_gives_the_same_bits(case, plain, monkeypatch, lab):
    """RVD_FAKE_NOMEM_ABOVE=1: the workspace of more than one window is refused, the engine halves its batch, releases and regroups"""
    monkeypatch.setenv("RVD_FAKE_NOMEM_ABOVE", "1")
    emb, T, fm = _run(case)
    assert np.array_equal(emb, plain[0])
    assert list(T["windows"]) == [int(case["wins"][-1])] and (fm["first_item"], fm["items"]) == (6, 3)
    _same_bits(T, plain[1], ref_rows=[2])
    _checked(case, emb, T, fm, "nomem_retry", expect_unchecked=[(0, 0), (0, 1), (0, 2)])


def test_the_second_recording_of_a_pack_gives_the_same_bits(case, plain):
    """rvd_upload_pcm_many([a short recording, the case's]): the case's windows are global windows 10 + w"""
    first = {}

    def upload(eng):
        f, total = eng.upload_many([case["pcm"][:52345], case["pcm"]])
        first["w"] = int(f[1])
        assert list(f) == [0, 10] and total == 16
    emb, T, fm = _run(case, case["wins"] + 10, upload=upload)
    assert np.array_equal(emb, plain[0])
    assert list(T["windows"]) == [int(w) + 10 for w in plain[1]["windows"]]
    _same_bits(T, plain[1])
    assert np.array_equal(T["stats"], plain[1]["stats"])
    _checked(case, emb, T, fm, "pack", expect_unchecked=[(0, 0), (0, 1), (0, 2)])


# ------------------------------------------------------------------------------------ the switch
def test_taps_are_off_by_default_and_change_nothing_that_is_enqueued(case, plain):
    """launch counts of every embedding kernel (e->prof) with the taps never touched, on, and off again: equal; the copies are
    counted under a name of their own, which stays at zero unless the switch is on.  The embeddings do not depend on the switch."""
    eng = _engine(case)
    eng.upload(case["pcm"])
    counts = []
    for on in (None, True, False):
        if on is not None:
            eng.set_emb_tap(on)
        eng.reset_timings()
        emb = eng.embed(case["wins"], case["masks"])
        assert np.array_equal(emb, plain[0])
        counts.append(({k: eng.timing(k)[2] for k in PROF}, eng.timing("emb_tap_copy")[2]))
    eng.close()
    assert counts[0][0] == counts[1][0] == counts[2][0], counts
    assert counts[0][0]["emb_stem"] == 1 and counts[0][0]["emb_conv_block"] == 3 and counts[0][0]["emb_conv_sc_fused"] == 2
    assert counts[0][1] == 0 and counts[2][1] == 0 and counts[1][1] > 40, [c[1] for c in counts]


def test_refusals_by_name_with_nothing_written(case, monkeypatch, lab):
    from reverb_amd._lib import RvbError, fptr
    sentinel = np.full(64, -77.0, np.float32)
    eng = _engine(case)
    eng.upload(case["pcm"])
    assert eng.lib.rvd_get_emb_tap(eng._h, b"stem", fptr(sentinel), sentinel.size) != 0 and np.all(sentinel == -77.0)      # no pass yet
    assert b"rvd_get_emb_tap" in eng.lib.rvd_last_error()
    eng.set_emb_tap(True)
    assert eng.lib.rvd_get_emb_tap(eng._h, b"forms", fptr(sentinel), sentinel.size) != 0 and np.all(sentinel == -77.0)     # on, still no pass
    out = np.full((5, 256), -77.0, np.float32)
    wins5 = np.arange(5, dtype=np.int64)
    rc = eng.lib.rvd_embed(eng._h, wins5.ctypes.data_as(eng.lib.rvd_embed.argtypes[1]), fptr(np.ascontiguousarray(case["masks"][:5])), 5,
                           fptr(out))                                              # five windows in one pass: more than the taps keep
    assert rc != 0 and np.all(out == -77.0) and b"rvd_set_emb_tap is on" in eng.lib.rvd_last_error()
    eng.embed(case["wins"][:1], case["masks"][:1])
    for name in (b"s1b0.tmp", b"s3b0.sc", b"s2b1.sc", b"no_such_tap"):             # a fused block's tmp, a K-loop / identity shortcut
        assert eng.lib.rvd_get_emb_tap(eng._h, name, fptr(sentinel), sentinel.size) != 0 and np.all(sentinel == -77.0), name
        assert name in eng.lib.rvd_last_error()
    assert eng.lib.rvd_get_emb_tap(eng._h, b"stem", fptr(sentinel), sentinel.size) != 0 and np.all(sentinel == -77.0)      # buffer too small
    eng.close()
    e8 = _engine(case, dtype="fp8")
    with pytest.raises(RvbError, match="rvd_set_emb_tap"):
        e8.set_emb_tap(True)
    e8.close()
    monkeypatch.setenv("RVD_EMB_FP8", "1")
    e8 = _engine(case)
    with pytest.raises(RvbError, match="rvd_set_emb_tap"):
        e8.set_emb_tap(True)
    e8.close()
