"""The bf16 segmentation network as segment_impl (csrc/diar_engine.hip) chains its kernels, held to what bf16 STORAGE costs.

End to end: the engine's distance from the fp32 oracle (six metrics, oracle/diar_bf16_ref.py metrics) must stay within
1.25 x the distance of the bf16-storage restatement (fp64 arithmetic, rounded where the engine stores bf16; yardstick =
tests/golden/diar_bf16_yardstick.json, the maximum over a plain and six jittered runs), + 4 frames on the counts (the floor
tests/test_longform_gpu.py uses for small cases).  1.25 covers the sample spread six jitters do not show (widest run seen
1.18 x the median).  tests/test_diar_bf16_ref.py shows without a GPU that a network that truncates instead of rounding, or
chains its LSTM layers wrongly, is outside this bound while the bounds of tests/test_diar_gpu.py accept it.

Stage by stage: every tensor that survives rvd_segment is read back (rvd_get_tap), each stage's stored input -- exact in bf16 --
goes through the fp64 stage function, and the stored output must lie inside that stage's kernel-test bound
(tests/diar_bf16_checks.py).  The same through rvd_segment_windows on a list out of order and through a two-recording
rvd_upload_pcm_many pack, whose results must also equal the plain run's bit for bit."""
import json
import os

import numpy as np
import pytest

from conftest import ROOT
from oracle import diar_bf16_ref as B
from oracle import gen_golden_diar_bf16 as G
import diar_bf16_checks as CK
from test_diar_gpu import _record

pytestmark = pytest.mark.gpu

NOT_LSTM = tuple(s for s in CK.STAGES if s != "lstm_last")
TAPS = ("craw", "fsum", "stats", "a1", "c2", "a2", "c3", "a3", "lstm_prev", "lstm", "linear0", "linear1")
PER_WINDOW = TAPS[2:]                  # [n][...]: row i belongs to window i of the call


@pytest.fixture(scope="module")
def yard():
    with open(os.path.join(ROOT, "tests", "golden", "diar_bf16_yardstick.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def cases():
    """the recordings of tests/test_diar_gpu.py with the fp32 oracle's output, made on demand; 'short' is the single zero-padded
    window of test_short_audio_single_padded_window (no oracle run: the stage checks need none)"""
    made = {}

    def get(name):
        if name not in made:
            if name == "short":
                c6 = get("w6_seed0")
                pcm = c6["pcm"][:52345]
                made[name] = dict(cfg=c6["cfg"], sd=c6["sd"], pcm=pcm, x=G.windows_of(pcm, c6["cfg"]))
            else:
                made[name] = G.make_case(name)
        return made[name]
    return get


def _engine(case):
    from reverb_amd.diar_engine import DiarEngine
    return DiarEngine(case["cfg"], case["sd"], dtype="bf16")


def _tensors(eng, logp):
    T = {k: eng.tap(k, logp.shape[0]) for k in TAPS}
    T["logp"] = logp
    return T


def _valid(k, t):
    """the rows of a tapped tensor that the network reads: the last 4 conv rows of a window run on into the next window's frames
    (or the buffer's slack) and are never pooled"""
    d = B.dims()
    return t[:, :d["f2"]] if k == "c2" else t[:, :d["f3"]] if k == "c3" else t


@pytest.fixture(scope="module")
def plain(cases):
    """the 6-window recording and the single padded window through upload + segment: log-probabilities and every tap"""
    out = {}
    for name in ("w6_seed0", "short"):
        case = cases(name)
        eng = _engine(case)
        assert eng.upload(case["pcm"]) == case["x"].shape[0]
        logp = eng.segment()
        out[name] = _tensors(eng, logp)
        eng.close()
    return out


# ------------------------------------------------------------------------------------ end to end
# measured on MI355X, engine against the fp32 oracle (yardstick; bound):
#   6 windows,  3 534 frames (3 452 confident): argmax differs on 34 (37; 50), on confident frames 6 (11; 17),
#                                               mean |dp| 0.002830 (0.002953; 0.003692), SincNet tap 0.009628 (0.009638; 0.012048)
#   44 windows, 25 916 frames (25 250 confident): argmax differs on 301 (331; 417), on confident frames 83 (98; 126),
#                                               mean |dp| 0.002992 (0.003030; 0.003788), SincNet tap 0.010422 (0.010423; 0.013029)
#   6 windows, weights seed 1 (3 394 confident): argmax differs on 67 (76; 99), on confident frames 20 (22; 31),
#                                               mean |dp| 0.004576 (0.004630; 0.005788), SincNet tap 0.009974 (0.009993; 0.012491)
# The engine sits at or below the restatement's own spread: the fast exp2 / rcp sigmoid and tanh of GateMath<bf16_t>, which the
# restatement does not model, cost nothing that these metrics see.
@pytest.mark.parametrize("name", ["w6_seed0", "w44_seed0", "w6_seed1"])
def test_bf16_engine_within_the_storage_yardstick(cases, yard, name):
    case = cases(name)
    eng = _engine(case)
    W = eng.upload(case["pcm"])
    assert W == case["x"].shape[0] == yard["cases"][name]["windows"]
    logp = eng.segment()
    sinc = eng.tap("sincnet", W)
    eng.close()
    m = B.metrics(logp, sinc, case["logp"], case["sinc"])
    y = yard["cases"][name]["yardstick"]
    print("bf16 engine, %s: %s; yardstick %s" % (name, json.dumps(m), json.dumps(y)))
    _record(test="bf16_engine_within_the_storage_yardstick", case=name, **m)
    assert m["frames"] == yard["cases"][name]["frames"]
    assert abs(m["confident"] - yard["cases"][name]["confident"]) <= 2       # the oracle's own margin: the fixture's, to fp32 ties
    for k in B.COUNTS:
        assert m[k] <= 1.25 * y[k] + 4, (k, m[k], y[k])
    for k in B.MEANS:
        assert m[k] <= 1.25 * y[k], (k, m[k], y[k])


# ------------------------------------------------------------------------------------ stage by stage
# measured on MI355X, worst |err| / bound per stage (6 windows; single padded window): first block 0.993; 0.994, conv 2 0.972; 0.962,
# pool-norm 2 0.990; 0.979, conv 3 0.985; 0.958, pool-norm 3 0.989; 0.987, linear 0 0.953; 0.952, linear 1 0.990; 0.988 (each within
# the output's half ulp, which is nearly all of these bounds), classifier 0.019; 0.021 (fp32 output)
@pytest.mark.parametrize("name", ["w6_seed0", "short"])
def test_every_stage_of_the_engine_is_inside_its_kernel_bound(cases, plain, name):
    """first block (from the stored sinc convolution and the engine's own fp32 window statistics and filter sums), conv 2, pool-norm 2, conv 3, pool-norm 3, linear 0,
    linear 1, classifier -- and zero pad columns in every tapped tensor"""
    case, T = cases(name), plain[name]
    fig, bad = CK.check_stages(case["sd"], case["x"][:, 0].numpy(), T, fstep=1600, stages=NOT_LSTM)
    print("stages, %s: %s" % (name, json.dumps(fig)))
    _record(test="every_stage_inside_its_kernel_bound", case=name, **fig)
    assert not bad, bad


# measured on MI355X (forward; reverse): 6 windows max 2.0e-3; 3.9e-3 (one bf16 ulp), mean 3.6e-8; 4.5e-8 -- single padded window
# max 4.9e-4; 2.4e-4, mean 1.3e-8; 9.6e-9.  'free' figures: 6 windows mean 9.7e-5; 8.2e-5, single window 5.2e-5; 1.29e-4, max 3.9e-3.
@pytest.mark.parametrize("name", ["w6_seed0", "short"])
def test_last_lstm_layer_of_the_engine_is_inside_the_layer_tests_bound(cases, plain, name):
    """the last LSTM layer (T = 589, in = 256) from its stored inputs -- the output of the layer before it and, at every step, the
    h_{t-1} the kernel itself stored and read back -- at test_lstm_layer's measured bf16 bound (max 4e-2, mean 5e-5 per direction).

    Reported with it and not asserted ('free' figures): the same fp64 layer fed its OWN h_{t-1}.  One rounding that falls the other
    way is then carried on by this model's recurrence (W_hh ~ U(+-3 / sqrt(H)): three times the variance of test_lstm_layer's), on
    reference and kernel alike: the fp64 restatement, every value moved by 1 +- 2^-20 and no kernel involved, is at mean 1.1e-4
    against itself in that form (tests/test_diar_bf16_ref.py), the MI355X at 5e-5 .. 1.3e-4, both at max 3.9e-3 = one bf16 ulp."""
    case, T = cases(name), plain[name]
    fig, bad = CK.check_stages(case["sd"], case["x"][:, 0].numpy(), T, fstep=1600, stages=("lstm_last",))
    print("last LSTM layer, %s: %s" % (name, json.dumps(fig)))
    _record(test="last_lstm_layer_inside_the_layer_tests_bound", case=name, **fig)
    assert not bad, bad
    # Fed the stored h_{t-1}, a difference cannot outlive its step: what is left is the roundings that fall the other way, which the
    # 2^-20 jitter model puts at mean 4e-7 (tests/test_diar_bf16_ref.py).  A tenth of the layer bound leaves that model a factor 10
    # and is a tenth of what h truncated instead of rounded gives (5.4e-4 there).
    assert max(fig["lstm_last_forward_mean"], fig["lstm_last_reverse_mean"]) < 0.1 * CK.SR.LSTM_BF16_MEAN


# ------------------------------------------------------------------------------------ other ways in
# Every tap must equal the plain run's bit for bit, and every stage is checked again on what these calls left behind.
def test_window_list_out_of_order_gives_the_same_bits_and_passes_the_stage_checks(cases, plain):
    case = cases("w6_seed0")
    win = np.array([4, 0, 5, 2], np.int64)
    eng = _engine(case)
    eng.upload(case["pcm"])
    logp = eng.segment_windows(win)
    T = _tensors(eng, logp)
    eng.close()
    assert np.array_equal(logp, plain["w6_seed0"]["logp"][win])
    for k in PER_WINDOW:
        assert np.array_equal(_valid(k, T[k]), _valid(k, plain["w6_seed0"][k][win])), k
    fig, bad = CK.check_stages(case["sd"], case["x"][win, 0].numpy(), T, fstep=1600, win=win)
    print("stages, window list: %s" % json.dumps(fig))
    assert not bad, bad


def test_two_recording_pack_gives_the_same_bits_and_passes_the_stage_checks(cases, plain):
    a, b = cases("w6_seed0"), cases("short")
    eng = _engine(a)
    first, total = eng.upload_many([a["pcm"], b["pcm"]])
    assert list(first) == [0, 15] and total == 16
    win = np.array([0, 1, 2, 3, 4, 5, 15], np.int64)
    logp = eng.segment_windows(win)
    T = _tensors(eng, logp)
    eng.close()
    assert np.array_equal(logp[:6], plain["w6_seed0"]["logp"]) and np.array_equal(logp[6:], plain["short"]["logp"])
    for k in PER_WINDOW:
        assert np.array_equal(_valid(k, T[k][:6]), _valid(k, plain["w6_seed0"][k])), k
        assert np.array_equal(_valid(k, T[k][6:]), _valid(k, plain["short"][k])), k
    wav = np.concatenate([a["x"][:, 0].numpy(), b["x"][:, 0].numpy()])
    fig, bad = CK.check_stages(a["sd"], wav, T, fstep=1600, win=win)
    print("stages, two-recording pack: %s" % json.dumps(fig))
    assert not bad, bad


def test_a_tap_that_does_not_survive_the_call_is_refused(cases):
    """lstm_prev is the other ping-pong buffer: a one-layer model has none, and the engine says so instead of returning stale memory"""
    from reverb_amd import synth_diar as SD
    from reverb_amd._lib import RvbError
    from reverb_amd.diar_engine import DiarEngine
    cfg = SD.make_diar_config(lstm_layers=1)
    eng = DiarEngine(cfg, SD.make_segmentation_sd(cfg, 0), dtype="bf16")
    with pytest.raises(RvbError):
        eng.tap("a1", 1)                      # nothing segmented yet
    assert eng.upload(cases("short")["pcm"]) == 1
    eng.segment()
    assert eng.tap("lstm", 1).shape == (1, 589, 256) and eng.tap("linear1", 1).shape == (1, 589, 128)
    with pytest.raises(RvbError):
        eng.tap("lstm_prev", 1)
    eng.close()
