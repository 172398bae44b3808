"""The three kernels of csrc/pause_chunks.hip through their lab hooks (rvb_test_pause_cuts: loudness + cut search,
rvb_test_gather_chunks) against tests/pause_ref.py.  Integer-valued features make every fp32 sum exact, so the kernel's cuts must equal
the definition's with ==; on real log-mel features the order of the additions is the kernel's own, and its cuts are checked with the
replay check (each cut inside its window and within the rounding bound of the window's fp64 minimum).

Shapes: chunk_size 16 / 64 / 256, search 7 / chunk_size // 4 / chunk_size - 7, h 1 / 10 / 64.  chunk_size 16 with search = 16 // 4 = 4
lies below the 7 frames a piece needs: that one combination must be refused, by name."""
import numpy as np
import pytest

import pause_ref as P
from oracle import fbank_ref
from reverb_amd import _lib, synth

pytestmark = pytest.mark.gpu
SHAPES = [(cs, s, h) for cs in (16, 64, 256) for s in sorted({7, cs // 4, cs - 7}) for h in (1, 10, 64)]
VALID = [(cs, s, h) for cs, s, h in SHAPES if 7 <= s <= cs - 7]
POISON = np.float32(-3.0e38)           # finite and huge: a neighbour's row read by mistake would win every minimum


def gpu_cuts(lib, rows, recs, cs, search, h):
    """rows [n_rows, 80]; recs = [(row0, n_frames)] -> per recording its piece starts"""
    rows = np.ascontiguousarray(rows, np.float32)
    r0 = np.array([r[0] for r in recs], np.int64)
    nf = np.array([r[1] for r in recs], np.int64)
    cap = sum(-(-int(n) // (cs - search)) for n in nf) + 1
    starts, counts = np.full(cap, -7, np.int32), np.full(len(recs), -7, np.int32)
    _lib.check(lib.rvb_test_pause_cuts(_lib.fptr(rows), len(rows), r0.ctypes.data_as(_lib._i64p), nf.ctypes.data_as(_lib._i64p), len(recs),
                                       cs, search, h, _lib.iptr(starts), cap, _lib.iptr(counts)), "rvb_test_pause_cuts")
    out, k = [], 0
    for c in counts:
        out.append(starts[k:k + c].tolist())
        k += c
    return out


def one(lib, x, cs, search, h):
    rows = x if len(x) else np.zeros((1, 80), np.float32)
    return gpu_cuts(lib, rows, [(0, len(x))], cs, search, h)[0]


@pytest.fixture(scope="module")
def real_feats():
    return {"speech": fbank_ref.fbank(synth.synth_audio(30.0)), "bursts": fbank_ref.fbank(P.burst_audio(30.0, 0))}


def test_the_refused_shape(lib):
    assert sorted(set(SHAPES) - set(VALID)) == [(16, 4, 1), (16, 4, 10), (16, 4, 64)]
    with pytest.raises(_lib.RvbError, match="search = 4"):
        one(lib, np.zeros((40, 80), np.float32), 16, 4, 10)


@pytest.mark.parametrize("cs,search,h", VALID)
def test_integer_features_equal_the_definition(lib, cs, search, h):
    ns = (0, 1, 6, cs, cs + 1, cs + 7, 3000)
    xs = [np.random.default_rng(n).integers(-20, 21, size=(n, 80)).astype(np.float32) for n in ns]
    # every length as a launch of its own and all of them as the recordings of one launch
    alone = [one(lib, x, cs, search, h) for x in xs]
    rows = np.concatenate([x for x in xs if len(x)])
    recs, r = [], 0
    for x in xs:
        recs.append((min(r, len(rows) - 1), len(x)))
        r += len(x)
    together = gpu_cuts(lib, rows, recs, cs, search, h)
    for n, x, a, t in zip(ns, xs, alone, together):
        want = P.cuts(x, cs, search, h)
        assert a == want and t == want, n
        P.check_tiling(a, n, cs)
    assert len(alone[4]) == 2 and alone[3] == [0] and alone[0] == []


@pytest.mark.parametrize("cs,search,h", VALID)
def test_constant_features_cut_at_hi(lib, cs, search, h):
    n = 5 * cs + 3
    st = one(lib, np.full((n, 80), P.FLOOR, np.float32), cs, search, h)
    want = [0]
    while n - want[-1] > cs:
        want.append(min(want[-1] + cs, n - 7))
    assert st == want


@pytest.mark.parametrize("cs,search,h", VALID)
def test_real_features_pass_the_replay_check(lib, real_feats, cs, search, h):
    for name, x in real_feats.items():
        st = one(lib, x, cs, search, h)
        P.replay_check(x, st, cs, search, h)


@pytest.mark.parametrize("seed", range(5))
def test_burst_cuts_land_in_silence(lib, real_feats, seed):
    x = real_feats["bursts"] if seed == 0 else fbank_ref.fbank(P.burst_audio(30.0, seed))
    st = one(lib, x, 256, 96, 10)
    P.replay_check(x, st, 256, 96, 10)
    assert len(st) > 4
    for c in st[1:]:
        assert np.all(x[c - 10:c + 10] == P.FLOOR), "cut %d does not lie in silence" % c


def test_recordings_do_not_read_their_neighbours(lib, real_feats):
    """five recordings at scattered row0 with poison rows between them: each recording's starts are those of the same recording alone"""
    sp, bu = real_feats["speech"], real_feats["bursts"]
    parts = [sp[:700], bu[100:1500], sp[:0], bu[:257], sp[1000:2990]]
    gaps = [3, 1, 70, 2, 5, 9]
    rows, recs = [np.full((gaps[0], 80), POISON, np.float32)], []
    r = gaps[0]
    for p, g in zip(parts, gaps[1:]):
        recs.append((r, len(p)))
        rows += [p, np.full((g, 80), POISON, np.float32)]
        r += len(p) + g
    rows = np.concatenate(rows)
    for cs, search, h in ((256, 96, 10), (64, 57, 64), (16, 7, 1)):
        got = gpu_cuts(lib, rows, recs, cs, search, h)
        for p, g in zip(parts, got):
            assert g == one(lib, p, cs, search, h)
            P.replay_check(p, g, cs, search, h)
    assert len(got[2]) == 0 and len(got[3]) > 1


@pytest.mark.parametrize("cs,search,h", [(64, 16, 10), (256, 96, 10), (16, 9, 64)])
def test_a_nan_stretch_wider_than_a_window(lib, real_feats, cs, search, h):
    x = real_feats["speech"][:1500].copy()
    a, b = cs - search - h - 5, 3 * cs + 2 * h          # every candidate of the first cuts is NaN; later windows are partly NaN
    x[max(a, 1):b] = np.nan
    st = one(lib, x, cs, search, h)
    assert st[1] == cs and st[2] == 2 * cs
    P.replay_check(x, st, cs, search, h)
    s = P.smoothed(P.loudness(x), h)
    later = [c for c in st[1:] if c > b + h]
    assert later and not np.isnan(s[st[1:]][np.array(st[1:]) > b + h]).any()


def test_gather(lib, real_feats):
    x = np.ascontiguousarray(real_feats["speech"][:700])
    cs = 64
    src = np.array([0, 64, 71, 300, 636, 699], np.int64)
    lens = np.array([64, 7, 33, 1, 64, 0], np.int32)                      # a full slot, 7 rows, the last rows of the source, an empty piece
    out = np.empty((len(src) * cs + 1, 80), np.float32)
    _lib.check(lib.rvb_test_gather_chunks(_lib.fptr(x), len(x), src.ctypes.data_as(_lib._i64p), _lib.iptr(lens), len(src), cs, _lib.fptr(out)),
               "rvb_test_gather_chunks")
    bits = out.view(np.uint32)
    for k, (s, n) in enumerate(zip(src, lens)):
        assert np.array_equal(bits[k * cs:k * cs + n], x[s:s + n].view(np.uint32)), k
        assert np.all(bits[k * cs + n:(k + 1) * cs] == 0), k
    assert np.all(bits[-1] == 0xFFFFFFFF)                                 # the row behind the last slot is untouched
    # a chunk_size whose float4 count is no multiple of the workgroup
    cs = 23
    src, lens = np.array([5, 100], np.int64), np.array([23, 7], np.int32)
    out = np.empty((2 * cs + 1, 80), np.float32)
    _lib.check(lib.rvb_test_gather_chunks(_lib.fptr(x), len(x), src.ctypes.data_as(_lib._i64p), _lib.iptr(lens), 2, cs, _lib.fptr(out)),
               "rvb_test_gather_chunks")
    bits = out.view(np.uint32)
    assert np.array_equal(bits[:23], x[5:28].view(np.uint32)) and np.array_equal(bits[23:30], x[100:107].view(np.uint32))
    assert np.all(bits[30:46] == 0) and np.all(bits[-1] == 0xFFFFFFFF)
