"""Kernel-level parity of the speaker-embedding trunk's convolutions (csrc/resnet.hip conv_kernel, conv_gemm.hip conv_igemm_kernel,
conv_row64.hip, conv_stream.hip, conv_block.hip, conv_s2.hip) and of its stem (resnet.hip emb_mean_kernel + emb_conv1_kernel), each
called through its rvb_test_* hook, against a plain fp64 numpy reference on the same rounded operands.

Bounds follow the rounding model and hold for every element (no fraction may fail): an fp32 sum of K products plus the bias (and
the residual) is off by at most (K + 2) u sum|terms| (u = 2^-24); K counts the fused shortcut's channels when it rides in the K loop.
A bf16 output adds half a bf16 ulp, at most 2^-8 of the value.  Kernels that claim the direct kernel's accumulation order and rounding
points (row64, stream, the fused block, the stride-2 opener, the wide implicit-GEMM tile against the narrow one) must also be
bit-identical to it.  Every test names a subtle fault it catches.  The worst error-to-bound ratio of each kernel is recorded with
tests/test_diar_gpu.py's _record, beside that file's parity numbers."""
import numpy as np
import pytest

from reverb_amd import _lib
from reverb_amd._lib import fptr
from test_diar_gpu import _record
from util import bf16_round, f32

pytestmark = pytest.mark.gpu
# the fp64 references and derived bounds live in tests/emb_conv_ref.py, shared with the bf16-storage restatement of the network
from emb_conv_ref import (F32, BF16, U32, check_within as _check_within, conv_ref as _ref, conv_ref_pixels as _ref_pixels,
                          conv_bound as _bound, stem_ref as _stem_ref)
DIRECT, IGEMM, ROW64, STREAM = 1, 2, 3, 4


def _rnd(dtype, a):
    return bf16_round(f32(a)) if dtype == BF16 else f32(a)


def _operands(rng, dtype, B, Fi, Ti, Cin, Cout, taps=9, res=False, stride=1, Cin2=0, plane2=None, stride2=2):
    """seeded operands, rounded to the compute dtype (bias stays fp32, as the kernels read it); x2 [B][plane2][Cin2] / w2 for a
    fused shortcut"""
    k = 3 if taps == 9 else 1
    Fo, To = (Fi - 1) // stride + 1, (Ti - 1) // stride + 1
    op = dict(x=_rnd(dtype, rng.standard_normal((B, Fi, Ti, Cin), dtype=np.float32)),
              w=_rnd(dtype, rng.standard_normal((Cout, Cin, k, k), dtype=np.float32) / np.sqrt(taps * Cin)),
              bias=f32(rng.standard_normal(Cout) * 0.5), res=None, x2=None, w2=None, stride=stride, stride2=stride2)
    if res:
        op["res"] = _rnd(dtype, rng.standard_normal((B, Fo, To, Cout), dtype=np.float32))
    if Cin2:
        op["x2"] = _rnd(dtype, rng.standard_normal((B,) + tuple(plane2) + (Cin2,), dtype=np.float32))
        op["w2"] = _rnd(dtype, rng.standard_normal((Cout, Cin2), dtype=np.float32) / np.sqrt(Cin2))
    return op


def _conv(lib, dtype, path, op, relu):
    """one convolution through rvb_test_conv2d -> (out [B][Fo][To][Cout], (kernel that ran, its tile))"""
    x, w, s = op["x"], op["w"], op["stride"]
    B, Fi, Ti, Cin = x.shape
    Cout, k = w.shape[0], w.shape[2]
    Fo, To = (Fi - 1) // s + 1, (Ti - 1) // s + 1
    out = np.full((B, Fo, To, Cout), np.nan, np.float32)
    ran = np.zeros(2, np.int32)
    x2 = op["x2"]
    Fi2, Ti2, Cin2 = x2.shape[1:] if x2 is not None else (0, 0, 0)
    rc = lib.rvb_test_conv2d(dtype, path, fptr(x), fptr(w), fptr(op["bias"]), fptr(op["res"]), fptr(out), B, Fi, Ti, Cin, Cout, s,
                             k * k, int(relu), fptr(x2), fptr(op["w2"]), Fi2, Ti2, Cin2, op["stride2"], _lib.iptr(ran))
    _lib.check(rc, "rvb_test_conv2d(path %d)" % path)
    return out, (int(ran[0]), int(ran[1]))


def _check_conv(dtype, got, op, relu, what):
    ref, tol = _ref(op, relu)
    return _check_within(got, ref, _bound(dtype, ref, tol), what)


# ------------------------------------------------------------------------------------ direct kernel (resnet.hip conv_kernel)
# every instantiation (dtype x NT 32 / 64 / 128 x stride 1 / 2 x 3x3 / 1x1) on planes whose Fo is not a multiple of CV_TF = 4 and
# whose To is not a multiple of CV_TT = 64, To < 64, Fi = 1, Ti = 1, odd and even planes at stride 2, several windows
_PLANES = [(2, 6, 70), (2, 5, 33), (1, 8, 130), (3, 1, 65), (2, 7, 1), (1, 9, 129), (2, 2, 64), (1, 1, 1), (2, 10, 200), (2, 3, 2)]
DIRECT_CASES = []
for _dt in (F32, BF16):
    _i = 0
    for _cout, _cin in ((32, 32), (64, 32), (96, 64), (128, 64), (256, 128)):       # NT 32, 64, 32 x 3 tiles, 128, 128 x 2 tiles
        for _stride in (1, 2):
            for _taps in (9, 1):
                _B, _Fi, _Ti = _PLANES[_i % len(_PLANES)]
                DIRECT_CASES.append((_dt, _cin, _cout, _stride, _taps, _B, _Fi, _Ti, _i % 2 == 0, _i % 3 != 1))
                _i += 1


@pytest.mark.parametrize("dtype,cin,cout,stride,taps,B,Fi,Ti,res,relu", DIRECT_CASES)
def test_direct_kernel_against_fp64(lib, dtype, cin, cout, stride, taps, B, Fi, Ti, res, relu):
    """resnet.hip's conv_kernel through path 1, whatever the lab switches say.  Catches: the last partial row tile (Fo % 4) or
    time tile (To % 64) dropped or written twice, a patch column of the stride-2 form read one pixel late (odd / even Fi, Ti), the
    weights of channel tile n0 > 0 taken from tile 0 (Cout 96 / 256), the window base of b > 0 wrong, a 1x1 tap read at (0, 0) instead
    of the centre, the residual added to the wrong pixel, ReLU applied when off."""
    rng = np.random.default_rng(hash((dtype, cin, cout, stride, taps, B, Fi, Ti)) % 2 ** 32)
    op = _operands(rng, dtype, B, Fi, Ti, cin, cout, taps=taps, res=res, stride=stride)
    got, ran = _conv(lib, dtype, DIRECT, op, relu)
    assert ran == (DIRECT, 128 if cout % 128 == 0 else 64 if cout % 64 == 0 else 32), ran
    r = _check_conv(dtype, got, op, relu, "direct")
    _record(test="emb_conv_kernels", kernel="direct", dtype=dtype, shape=[B, Fi, Ti, cin, cout, stride, taps], ratio=r)


# ------------------------------------------------------------------------------------ implicit GEMM (conv_gemm.hip), bf16
IGEMM_CASES = [
    # cin, cout, stride, res, relu, B, Fi, Ti      M = B Fo To: never a multiple of 256 / 512, tiles straddle windows
    (64, 128, 2, False, True, 2, 40, 37),          # 2 x 20 x 19 = 760
    (128, 128, 1, True, True, 3, 7, 45),           # 945
    (128, 128, 1, False, False, 2, 11, 50),        # 1100
    (128, 256, 2, False, True, 2, 19, 33),         # 2 x 10 x 17 = 340
    (256, 256, 1, True, False, 2, 5, 29),          # 290
    (128, 128, 1, True, True, 1, 1, 1),            # a single pixel
    (256, 256, 1, False, True, 1, 1, 1),
    (64, 128, 2, True, True, 1, 1, 2),             # stride 2 onto one pixel
    (128, 128, 2, False, True, 3, 3, 3),
]


@pytest.mark.parametrize("cin,cout,stride,res,relu,B,Fi,Ti", IGEMM_CASES)
def test_implicit_gemm_against_fp64_narrow_and_wide(lib, monkeypatch, lab, cin, cout, stride, res, relu, B, Fi, Ti):
    """conv_igemm_kernel through path 2 on 256-pixel tiles and (128 output channels) on 512-pixel tiles (RVD_IGEMM_BM), each within
    the fp64 bound, and the wide tile bit-identical to the narrow one (same K order per output).  Catches: a clamped row m >= M
    stored (it would overwrite the last pixel of the next window), a tile that straddles two windows reading the second window's
    patch from the first's base, tap (kh, kw) of the stride-2 gather off by one pixel, the residual of the wrong pixel, the weights
    of the second 128-channel tile read from the first."""
    rng = np.random.default_rng(hash((cin, cout, stride, B, Fi, Ti)) % 2 ** 32)
    op = _operands(rng, BF16, B, Fi, Ti, cin, cout, res=res, stride=stride)
    outs = {}
    for bm in ("256", "512"):
        monkeypatch.setenv("RVD_IGEMM_BM", bm)
        outs[bm], ran = _conv(lib, BF16, IGEMM, op, relu)
        assert ran == (IGEMM, 512 if bm == "512" and cout % 256 else 256), (bm, ran)
        r = _check_conv(BF16, outs[bm], op, relu, "igemm BM %s" % bm)
        _record(test="emb_conv_kernels", kernel="igemm" + ("_wide" if ran[1] == 512 else ""), dtype=BF16,
                shape=[B, Fi, Ti, cin, cout, stride, 9], ratio=r)
    assert np.array_equal(outs["256"], outs["512"])


SHORTCUT_CASES = [
    # x2 plane (B, Fi2, Ti2, Cin2) -> block output (Cin = Cout, stride 1 on x; 1x1 / stride 2 on x2)
    (2, 40, 499, 64, 128),             # the opener of the 128-channel stage: 64 ch @ 40 x 499 -> 128 ch @ 20 x 250
    (2, 20, 250, 128, 256),            # the opener of the 256-channel stage
    (2, 9, 37, 64, 128),               # odd openers: 5 x 19, ragged tiles
    (3, 4, 3, 128, 256),               # 2 x 2
    (1, 1, 1, 64, 128),                # one pixel
]


@pytest.mark.parametrize("B,Fi2,Ti2,cin2,cout", SHORTCUT_CASES)
def test_fused_projection_shortcut_against_fp64(lib, B, Fi2, Ti2, cin2, cout):
    """The block's second convolution with the 1x1 / stride-2 projection shortcut in its K loop (ConvArgs::in2, rows
    [Cout][9 Cin + Cin2] as pack_fused_shortcut packs them), through path 2 and through conv2d's own dispatch (path 0), within the
    fp64 bound of 9 Cin + Cin2 terms.  Catches: the last shortcut K step skipped (Cin2 = 128: 64 channels of the shortcut missing),
    the shortcut pixel taken at (s fo, s to) of the BORDERED plane (one row / column off), the shortcut weights read from the 3x3
    block's columns, the summed bias counted once."""
    Fo, To = (Fi2 - 1) // 2 + 1, (Ti2 - 1) // 2 + 1
    rng = np.random.default_rng(Fi2 * 1000 + Ti2 + cin2)
    op = _operands(rng, BF16, B, Fo, To, cout, cout, Cin2=cin2, plane2=(Fi2, Ti2), stride2=2)
    for path in (IGEMM, 0):
        got, ran = _conv(lib, BF16, path, op, True)
        assert ran == (IGEMM, 256), (path, ran)
        r = _check_conv(BF16, got, op, True, "fused shortcut path %d" % path)
    _record(test="emb_conv_kernels", kernel="igemm_shortcut", dtype=BF16, shape=[B, Fi2, Ti2, cin2, cout], ratio=r)


def test_auto_dispatch_takes_the_wide_tile_at_512_ki_pixels(lib, monkeypatch, lab):
    """conv2d's own dispatch (path 0) on 105 windows of the 128-channel stage (525 000 >= 512 Ki pixels) runs the 512-pixel tile
    without any lab switch, and its output equals the narrow tile's bit for bit.  The fp64 reference covers whole windows at the
    batch's start, middle and end and a seeded sample of 4 096 pixels.  Catches: a tile index that overflows or wraps past window
    64, the last partial tile (525 000 % 512 = 200 pixels) dropped, the size rule inverted."""
    monkeypatch.delenv("RVD_IGEMM_BM", raising=False)
    monkeypatch.delenv("RVD_CONV_IGEMM", raising=False)
    rng = np.random.default_rng(105)
    B, F, T, C = 105, 20, 250, 128
    op = _operands(rng, BF16, B, F, T, C, C, res=True)
    got, ran = _conv(lib, BF16, 0, op, True)
    assert ran == (IGEMM, 512), ran
    ref, tol = _ref(op, True, batches=[0, B // 2, B - 1])
    r = _check_within(got[[0, B // 2, B - 1]], ref, _bound(BF16, ref, tol), "wide auto, whole windows")
    pix = np.stack([rng.integers(0, B, 4096), rng.integers(0, F, 4096), rng.integers(0, T, 4096)], 1)
    refp, tolp = _ref_pixels(op, True, pix)
    r = max(r, _check_within(got[pix[:, 0], pix[:, 1], pix[:, 2]], refp, _bound(BF16, refp, tolp), "wide auto, sampled pixels"))
    _record(test="emb_conv_kernels", kernel="igemm_wide_auto", dtype=BF16, shape=[B, F, T, C, C, 1, 9], ratio=r)
    monkeypatch.setenv("RVD_IGEMM_BM", "256")
    narrow, ran = _conv(lib, BF16, 0, op, True)
    assert ran == (IGEMM, 256), ran
    assert np.array_equal(got, narrow)


# ------------------------------------------------------------------------------------ row64 and stream, vs fp64 and bit-identical to the direct kernel
ROW64_PLANES = [(2, 6, 61, True, True), (1, 9, 31, False, True), (1, 1, 5, True, False), (1, 3, 29, False, False),
                (2, 5, 91, True, True), (1, 2, 1, True, True)]     # Fo % 4 != 0, To % 30 != 0


@pytest.mark.parametrize("B,F,T,res,relu", ROW64_PLANES)
def test_row64_against_fp64_and_the_direct_kernel(lib, monkeypatch, lab, B, F, T, res, relu):
    """conv_row64.hip (path 3) within the fp64 bound and bit-identical to the direct kernel (path 1): the file's header claims the
    same accumulation order and rounding points.  Catches: a partial last 30-frame tile or 4-row band stored from stale
    accumulators, the bias or residual of channel group 7 off by one ulp (only the identity check sees that), the spill pad read
    as data."""
    monkeypatch.delenv("RVD_CONV_ROW64", raising=False)
    rng = np.random.default_rng(F * 100 + T)
    op = _operands(rng, BF16, B, F, T, 64, 64, res=res)
    got, ran = _conv(lib, BF16, ROW64, op, relu)
    assert ran == (ROW64, 0), ran
    r = _check_conv(BF16, got, op, relu, "row64")
    _record(test="emb_conv_kernels", kernel="row64", dtype=BF16, shape=[B, F, T, 64, 64, 1, 9], ratio=r)
    direct, _ = _conv(lib, BF16, DIRECT, op, relu)
    assert np.array_equal(got, direct)


STREAM_PLANES = [(2, 6, 63), (1, 5, 125), (1, 1, 7), (2, 9, 200), (1, 3, 62)]     # To % 62 != 0 (but one), Fo % 4 != 0


@pytest.mark.parametrize("C", [32, 64])
@pytest.mark.parametrize("B,F,T", STREAM_PLANES)
def test_stream_against_fp64_and_the_direct_kernel(lib, monkeypatch, lab, C, B, F, T):
    """conv_stream.hip (path 4) at splits 1, 2, 3, 17 and 40 of the time axis (40 > the tiles in any of these rows: capped to one
    tile per workgroup) within the fp64 bound and bit-identical to the direct kernel at every split.  Catches: the two positions
    62 / 63 of an m-tile stored, a workgroup of a split walking its neighbour's first tile too (or skipping its own last one),
    clamped patch rows feeding a stored output, the residual of the previous tile."""
    monkeypatch.setenv("RVD_CONV_STREAM64", "1")
    rng = np.random.default_rng(C * 1000 + F * 100 + T)
    op = _operands(rng, BF16, B, F, T, C, C, res=T % 2 == 1)
    relu = T % 3 != 0
    direct, _ = _conv(lib, BF16, DIRECT, op, relu)
    r = _check_conv(BF16, direct, op, relu, "direct (stream shapes)")
    tiles = -(-T // 62)
    for split in (1, 2, 3, 17, 40):
        monkeypatch.setenv("RVD_CONV_STREAM", str(split))
        got, ran = _conv(lib, BF16, STREAM, op, relu)
        assert ran == (STREAM, min(split, tiles)), (split, ran)
        assert np.array_equal(got, direct), split
    _record(test="emb_conv_kernels", kernel="stream", dtype=BF16, shape=[B, F, T, C, C, 1, 9], ratio=r)


# ------------------------------------------------------------------------------------ fused block and stride-2 opener vs the direct kernel
def test_fused_basic_block_is_bit_identical_to_two_direct_launches(lib):
    """rvb_test_conv_block32 on the ragged shapes of test_fused_basic_block_on_ragged_shapes against the same block as two direct
    launches (path 1; the intermediate is rounded to bf16 by the first): conv_block.hip claims identical results.  Catches: a mid row
    of a band computed from the clamped (wrong) input row, the residual taken from the patch one pixel off, any reordering of the
    taps."""
    rng = np.random.default_rng(5)
    for B, F, T in ((2, 6, 61), (1, 9, 130), (1, 3, 17), (1, 4, 60), (1, 1, 5), (1, 2, 64), (1, 7, 121)):
        x = bf16_round(f32(np.abs(rng.standard_normal((B, F, T, 32)))))
        wa = bf16_round(f32(rng.standard_normal((32, 32, 3, 3)) / 12.0))
        wb = bf16_round(f32(rng.standard_normal((32, 32, 3, 3)) / 12.0))
        ba, bb = f32(rng.standard_normal(32) * 0.1), f32(rng.standard_normal(32) * 0.1)
        got = np.zeros((B, F, T, 32), np.float32)
        _lib.check(lib.rvb_test_conv_block32(fptr(x), fptr(wa), fptr(ba), fptr(wb), fptr(bb), fptr(got), B, F, T))
        mid, _ = _conv(lib, BF16, DIRECT, dict(x=x, w=wa, bias=ba, res=None, x2=None, w2=None, stride=1, stride2=1), True)
        want, _ = _conv(lib, BF16, DIRECT, dict(x=mid, w=wb, bias=bb, res=x, x2=None, w2=None, stride=1, stride2=1), True)
        assert np.array_equal(got, want), (B, F, T, float(np.abs(got - want).max()))


def test_stride2_opener_is_bit_identical_to_two_direct_launches(lib):
    """rvb_test_conv_s2sc on the ragged shapes of test_stride2_opener_on_ragged_shapes against the 3x3 / stride-2 convolution (ReLU)
    and the 1x1 / stride-2 shortcut as two direct launches (path 1): conv_s2.hip claims identical results.  Catches: a de-interleaved
    patch plane off by one pixel at odd Ti, the shortcut read from the 3x3 patch's corner instead of its centre, a partial last tile."""
    rng = np.random.default_rng(6)
    for B, Fi, Ti in ((2, 8, 62), (1, 9, 125), (1, 3, 17), (1, 1, 2), (1, 16, 63), (1, 5, 130)):
        Fo, To = (Fi - 1) // 2 + 1, (Ti - 1) // 2 + 1
        x = bf16_round(f32(rng.standard_normal((B, Fi, Ti, 32))))
        w = bf16_round(f32(rng.standard_normal((64, 32, 3, 3)) / 12.0))
        wsc = bf16_round(f32(rng.standard_normal((64, 32)) / 4.0))
        b, bsc = f32(rng.standard_normal(64) * 0.1), f32(rng.standard_normal(64) * 0.1)
        out, sc = np.zeros((B, Fo, To, 64), np.float32), np.zeros((B, Fo, To, 64), np.float32)
        _lib.check(lib.rvb_test_conv_s2sc(fptr(x), fptr(w), fptr(b), fptr(wsc), fptr(bsc), fptr(out), fptr(sc), B, Fi, Ti))
        want, _ = _conv(lib, BF16, DIRECT, dict(x=x, w=w, bias=b, res=None, x2=None, w2=None, stride=2, stride2=1), True)
        want_sc, _ = _conv(lib, BF16, DIRECT, dict(x=x, w=f32(wsc[:, :, None, None]), bias=bsc, res=None, x2=None, w2=None, stride=2,
                                                    stride2=1), False)
        assert np.array_equal(out, want), (B, Fi, Ti, float(np.abs(out - want).max()))
        assert np.array_equal(sc, want_sc), (B, Fi, Ti, float(np.abs(sc - want_sc).max()))


# ------------------------------------------------------------------------------------ the stage shapes at product size, every path the engine can route them to
PRODUCT_CASES = [
    # name, (Fi, Ti, Cin, Cout, stride, taps, res), paths besides the direct kernel (0 = conv2d's dispatch)
    ("stage1", (80, 998, 32, 32, 1, 9, True), (0, STREAM)),
    ("stage2", (40, 499, 64, 64, 1, 9, True), (0, ROW64, STREAM)),
    ("stage3", (20, 250, 128, 128, 1, 9, True), (0, IGEMM)),
    ("stage4", (10, 125, 256, 256, 1, 9, True), (0, IGEMM)),
    ("open2", (80, 998, 32, 64, 2, 9, False), (0,)),
    ("open2_sc", (80, 998, 32, 64, 2, 1, False), (0,)),
    ("open3", (40, 499, 64, 128, 2, 9, False), (0, IGEMM)),
    ("open4", (20, 250, 128, 256, 2, 9, False), (0, IGEMM)),
]
# what conv2d's dispatch picks at these shapes by default (path 0): stream for 32 channels, row64 for 64, the implicit GEMM from 128 up
_AUTO = {"stage1": STREAM, "stage2": ROW64, "stage3": IGEMM, "stage4": IGEMM, "open2": DIRECT, "open2_sc": DIRECT, "open3": IGEMM,
         "open4": IGEMM}
_IDENTICAL_TO_DIRECT = (DIRECT, ROW64, STREAM)


@pytest.mark.parametrize("name,shape,paths", PRODUCT_CASES, ids=[c[0] for c in PRODUCT_CASES])
def test_stage_shapes_at_product_size_on_every_path(lib, monkeypatch, lab, name, shape, paths):
    """The four stage shapes (80x998x32, 40x499x64, 20x250x128, 10x125x256) and the stride-2 openers with B = 2, on the direct kernel
    and on every path the engine can route them to, each within the fp64 bound; row64 and stream bit-identical to the direct kernel.
    Catches what only the product's plane sizes reach: 998 = 16 tiles of 62 + 6 and 499 = 16 tiles of 30 + 19, 80 rows = 20 bands of
    4, M = 2 x 5 000 pixels in 256-pixel tiles that straddle the two windows."""
    for k in ("RVD_CONV_STREAM", "RVD_CONV_ROW64", "RVD_IGEMM_BM", "RVD_CONV_IGEMM"):
        monkeypatch.delenv(k, raising=False)
    Fi, Ti, cin, cout, stride, taps, res = shape
    rng = np.random.default_rng(Fi + cin)
    op = _operands(rng, BF16, 2, Fi, Ti, cin, cout, taps=taps, res=res, stride=stride)
    ref, tol = _ref(op, True)
    bound = _bound(BF16, ref, tol)
    direct, ran = _conv(lib, BF16, DIRECT, op, True)
    assert ran[0] == DIRECT
    worst = {"direct": _check_within(direct, ref, bound, name + " direct")}
    for path in paths:
        if path == STREAM and cin == 64:
            monkeypatch.setenv("RVD_CONV_STREAM64", "1")
        got, ran = _conv(lib, BF16, path, op, True)
        monkeypatch.delenv("RVD_CONV_STREAM64", raising=False)
        if path == 0:
            assert ran[0] == _AUTO[name], ran
        kern = {DIRECT: "direct", IGEMM: "igemm", ROW64: "row64", STREAM: "stream"}[ran[0]] + ("_wide" if ran == (IGEMM, 512) else "")
        worst[kern] = max(worst.get(kern, 0.0), _check_within(got, ref, bound, "%s path %d" % (name, path)))
        if ran[0] in _IDENTICAL_TO_DIRECT:
            assert np.array_equal(got, direct), (name, path)
    for kern, r in worst.items():
        _record(test="emb_conv_kernels", kernel=kern, dtype=BF16, shape=[2, Fi, Ti, cin, cout, stride, taps], ratio=r)


# ------------------------------------------------------------------------------------ stem: per-window CMN + Conv2d(1, C, 3) + BN + ReLU
STEM_CASES = [
    # dtype, C, nfr, F, frames_per_step, n_windows, window list, dc
    (F32, 32, 998, 80, 100, 4, [3, 0, 3, 1], True),      # 62 full 16-frame tiles + 6; overlapping windows; out of order, repeats
    (BF16, 32, 998, 80, 100, 4, [3, 0, 3, 1], True),
    (F32, 16, 998, 80, 400, 3, [2, 1], False),
    (BF16, 16, 998, 80, 400, 3, [2, 1], True),
    (F32, 8, 11, 37, 5, 6, [5, 0, 2, 2, 4], False),      # nfr < 16: one partial tile; F < 80
    (BF16, 8, 11, 37, 5, 6, [5, 0, 2, 2, 4], True),
    (BF16, 32, 40, 64, 16, 2, [1], False),
]


@pytest.mark.parametrize("dtype,C,nfr,F,fps,nwin,win,dc", STEM_CASES)
def test_emb_stem_against_fp64(lib, dtype, C, nfr, F, fps, nwin, win, dc):
    """emb_window_mean over every window, then emb_conv1 on a window list, against fp64: the means within (nfr + 4) u mean|x| of the
    fp64 means, and the stem output, on the kernel's own means (fb - mean rounded to fp32 as the kernel does), within 11 u sum|terms|
    (+ half a bf16 ulp).  A DC offset of 100 sigma in one mel bin must vanish (CMN).  Catches: the mean of window b used for window
    win[b] (the list is out of order, with repeats), the mean divided by 3 slots' counts instead of nfr, the last partial 16-frame
    tile or the row t = nfr read as data instead of zero padding, mel bin F read as data when F < 80, the taps' kh / kw swapped."""
    rng = np.random.default_rng(nfr * 10 + C + dtype)
    n_rows = (nwin - 1) * fps + nfr + 3
    fb = f32(rng.standard_normal((n_rows, 80)) * 2.0 + rng.standard_normal(80) * 3.0)
    if dc:
        fb[:, 7] += f32(100.0 * fb[:, 7].std())
    w = f32(rng.standard_normal((C, 1, 3, 3)) / 3.0)
    bias = f32(rng.standard_normal(C) * 0.3)
    wl = np.array(win, np.int64)
    B = len(wl)
    mean = np.empty((nwin, 80), np.float32)
    out = np.full((B, F, nfr, C), np.nan, np.float32)
    _lib.check(lib.rvb_test_emb_stem(dtype, fptr(fb), n_rows, wl.ctypes.data_as(_lib._i64p), B, nwin, fps, nfr, F, C, fptr(w), fptr(bias),
                                     fptr(mean), fptr(out)))
    fb64 = fb.astype(np.float64)
    for v in range(nwin):
        rows = fb64[v * fps:v * fps + nfr]
        m = rows.mean(0)
        assert np.all(np.abs(mean[v] - m) <= (nfr + 4) * U32 * np.abs(rows).mean(0) + 1e-30), (v, np.abs(mean[v] - m).max())
    r = 0.0
    for b, v in enumerate(wl):
        plane = (fb[v * fps:v * fps + nfr, :F] - mean[v, :F]).T.astype(np.float64)      # [F][nfr], fp32 subtraction as the kernel's
        ref, tol = _stem_ref(plane, w, bias)
        r = max(r, _check_within(out[b], ref, _bound(dtype, ref, tol), "stem window %d" % v))
        if dc:
            assert np.abs(plane[7]).max() < 10.0         # the 100-sigma offset is gone: the bin is centred like the others
    _record(test="emb_conv_kernels", kernel="stem", dtype=dtype, shape=[B, F, nfr, C], ratio=r)
