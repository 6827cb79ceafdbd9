"""Element-wise float64 parity of every compiled convolution instantiation the three older suites do not reach.

tests/test_conv_tiles_gpu.py, tests/test_conv_small_tiles_gpu.py and tests/test_wgrad_parity_gpu.py pin the instantiations the round-6
traces launched: 56 of the 138 conv_igemm / conv_igemm_s3 / conv_wgrad kernels of the production library.  conv_route() and
wgrad_route() pick the instantiation from the launch size, so another batch size, one image in the Tester or a K = 80 class head lands
on one of the other 82.  This file holds one case (a few have two) for each of them, in the form of those suites and with their
runners and references: (id, route, runner, features); the case asserts its route from the library's own name through
ops.KERNEL_EVENTS, prefills outputs with NaN (dw / db and accumulated outputs with values, workspaces with NaN), and compares every
element — outputs, pad lanes, tile statistics, the fused bias gradient — with a float64 reference of the operand values the kernel
sees under helpers.check_elementwise.  tests/test_conv_all_routes_cpu.py pins every route on the host, counts the library's kernels
against the four GPU files (138 of 138) and shows what the one new reference rejects.

Shapes, from pick_tc / conv_uses_s3 / conv_needs_ext / pick_tile / wgrad_uses_dma / wgrad_lin_ok:

  * 256-row tile: 16-bit, Cout_store >= 256, pixel tiles x ceil(Cout_store / 256) >= 400, >= 16 k-steps — B3 67x65 (103 pixel tiles, tail
    9; images end inside tiles) with Cout 1000 / 1024, or B2 115x113 (204 tiles, tail 6) with 1x1 512 -> 512 / 1000;
  * 128-row tile: pixel tiles x ceil(Cout_store / 128) >= 200 with the 256-row rule not met (fewer than 16 k-steps, or Cout_store 224);
  * 64-row tile: fewer workgroups (B3 29x27: 19 tiles, tail 45); 32-row tile: Cout_store 32;
  * EXT: residual + accumulate on the plain kernel, the virtual concatenation on the shared-tile 3x3 kernel;
  * OUTF32 without GENERAL: f32 output, no bias / activation, Cout a multiple of the tile height.

The register-staged generic weight gradient conv_wgrad_kernel<T, TM, TN>.  mpn_conv_wgrad refuses a Cin that is not a multiple of 8
(MPN_E_BADARG, whatever mpn_conv_wgrad_kernel_name says for such a block), its f32 blocks with nseg > 0 or kseg_n > 0 likewise (both
forms require the LDS-DMA kernel), so through the C ABI the generic kernel runs for one reason only: an operand whose extent passes the
2^31 - 1 bytes of a buffer descriptor.  _generic_case gets there without a 2 GB tensor: x is a strided view — B small images whose batch
stride x_sB is 2^31 / B bytes, inside one allocation of (B - 1) x_sB plus one image, of which only the images are ever written or read.
wgrad_uses_dma() sees B x_sB = 2 GiB and routes the launch to the generic kernel; everything else about the launch is small.  The
dense > 2 GB blocks of tests/test_kernel_names_cpu.py are not launched; their names stay pinned on the host.

Bound of the generic kernel, from its own loop (conv_wgrad.hip: conv_wgrad_kernel): one f32 accumulator per element over the pixels of
a slice, advanced by one 16x16x32 MFMA per 32-pixel step (16-bit) or four 16x16x4 MFMAs per 16-pixel step (f32: k_step 4), then the
slices added in order by the reduction kernels and into the prefilled dw — K = the pixels of one slice and slices + 1 extra terms,
the DMA kernels' bound (their ring changes how tiles arrive, not the summation order)."""
from types import SimpleNamespace

import pytest
import torch

import test_conv_small_tiles_gpu as st
import test_conv_tiles_gpu as ct
import test_wgrad_parity_gpu as wt
from helpers import check_elementwise, report, rng_normal, round_up
from test_conv_tiles_gpu import BF, F32, H16, _inst, _need_gpu  # noqa: F401  (the module fixture: GPU present, host threads capped at 16)

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------- the generic weight gradient: reference (CPU)
def _generic_ref(cid, f):
    """Operands (rounded through the storage type, float64), prefill and the float64 gradient of one single-tensor launch."""
    dt, B, H, W, Cin, Cout, k = f["dtype"], f["B"], f["H"], f["W"], f["Cin"], f["Cout"], f["k"]
    stride, pad = f.get("stride", 1), f.get("pad", (k - 1) // 2)
    seed = 7000 + sum(ord(c) for c in cid)
    R = SimpleNamespace(dt=dt, k=k, stride=stride, pad=pad, k_step=4 if dt == F32 else 32, kp=16 if dt == F32 else 32)
    R.Ho, R.Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    R.P = B * R.Ho * R.Wo
    R.x = wt._q(dt, rng_normal(seed, B, Cin, H, W))
    R.dy = wt._q(dt, rng_normal(seed + 1, B, Cout, R.Ho, R.Wo))
    R.dw0 = wt._prefill(seed + 2, Cout, k, k, Cin)
    R.db0 = wt._prefill(seed + 3, Cout) if f.get("bias") else None
    R.ref, R.mag = wt._ref_wgrad(R.x, R.dy, k, k, stride, pad)
    return R


def _slice_len(R, chunks):
    """launch_wgrad: ceil(P / chunks) rounded up to the k-step's pixels."""
    return R.P if chunks == 1 else round_up((R.P + chunks - 1) // chunks, R.kp)


def _check_generic(cid, route, R, dw, chunks):
    K = min(_slice_len(R, chunks), R.P)
    return check_elementwise(cid + " dw", dw.double(), R.ref + R.dw0.double(), R.mag + R.dw0.double().abs(), F32, R.k_step, K, chunks + 1,
                             route=route, names="orsc")


# ------------------------------------------------------------------------------------- the generic weight gradient: launch (GPU)
IMAGE_ELEMS = 1 << 22          # room for the last image behind the last batch stride (every case's image is far smaller)


def _spread_act(x, dt):
    """x [B, C, H, W] on the device as a strided view whose B images lie 2^31 / B bytes apart (the file's docstring): (Act, x_geom)."""
    from multiposenet.pytorch_amd.ops import Act
    B, C, H, W = x.shape
    Cs = round_up(C, 32)
    es = 4 if dt == F32 else 2
    sB = round_up(((1 << 31) + B * es - 1) // (B * es), 32)
    assert H * W * Cs <= IMAGE_ELEMS and B * sB * es >= (1 << 31) - 1
    flat = torch.empty((B - 1) * sB + IMAGE_ELEMS, dtype=dt, device="cuda")
    view = flat.as_strided((B, H, W, Cs), (sB, W * Cs, Cs, 1))
    img = torch.zeros((B, H, W, Cs), dtype=torch.float32)
    img[..., :C] = x.permute(0, 2, 3, 1).float()
    view.copy_(img.to(dt))
    return Act(view, C), (H, W, sB, W * Cs, Cs)


def _generic_case(cid, route, f):
    ops = wt._ops()
    R = _generic_ref(cid, f)
    dt, Cin, Cout, k = R.dt, f["Cin"], f["Cout"], R.k
    xa, geom = _spread_act(R.x, dt)
    dya = wt._act(R.dy, dt)
    dw, db, fused, names, p = wt._three_runs(
        cid, lambda dw, db: ops.conv_wgrad(xa, dya, dw, Cout, k, k, R.stride, R.pad, cin=Cin, x_geom=geom, db=db), R.dw0, R.db0)
    wt._assert_route(cid, names, route)
    # the generic kernel has no bias column: the wrapper reports db unserved and leaves it alone (the engine then calls ops.bias_grad)
    assert fused is False, "%s: the generic kernel does not fuse the bias gradient" % cid
    assert p.db is None and (db is None or torch.equal(wt._bits(db), wt._bits(R.db0))), "%s: db touched by a launch that does not serve it" % cid
    assert p.chunks == f["chunks"], "%s: %d slices, expected %d" % (cid, p.chunks, f["chunks"])
    last = R.P - (p.chunks - 1) * _slice_len(R, p.chunks)
    assert last == f["last_slice"], "%s: last slice %d pixels, expected %d" % (cid, last, f["last_slice"])
    _check_generic(cid, route, R, dw, p.chunks)


# ------------------------------------------------------------------------------------- conv_igemm_kernel / conv_igemm_s3_kernel
C, KS, PY = st._conv_case, ct._kseg_case, st._pyramid_case
S = st.S                                  # B3 29x27: P = 2349, 19 pixel tiles, tail 45
M = dict(B=4, H=30, W=30)                 # P = 3600: 29 tiles, tail 16
L = dict(B=2, H=115, W=113)               # P = 25 990: 204 tiles, tail 6
Q = dict(B=3, H=67, W=65)                 # P = 13 065: 103 tiles, tail 9; an image is 34.02 tiles
RA = dict(bias=True, acc=True)            # + res=(H, W): residual with accumulate, the extended epilogue of the plain kernel


def _plain(dt, name, tc):
    """The conv_igemm_kernel rows of one 16-bit type: <tc | OUTF32 GENERAL EXT> in the comments."""
    big = tc if tc != 32 else 32
    rows = []
    if tc == 128:        # 1x1 256 -> 1024 / 1000 at B4 30x30: 29 x 8 = 232 workgroups, 8 k-steps (< 16: not the 256-row tile)
        g = dict(dtype=dt, Cin=256, k=1, **M)
        rows = [("F F F", "1x1 256->1024 B4 30x30 stats", dict(Cout=1024, stats=True)),
                ("F T T", "1x1 256->1000 B4 30x30 bias res+acc", dict(Cout=1000, res=(30, 30), **RA)),            # last channel tile: 104 rows live
                ("T F F", "1x1 256->1024 B4 30x30 f32out", dict(Cout=1024, out_f32=True)),
                ("T T F", "1x1 256->1000 B4 30x30 bias f32out", dict(Cout=1000, bias=True, out_f32=True))]
    elif tc == 256:      # 1x1 512 -> 512 / 1000 at B2 115x113: 204 x 2 = 408 / 204 x 4 workgroups, 16 k-steps
        g = dict(dtype=dt, Cin=512, k=1, **L)
        rows = [("F F F", "1x1 512->512 B2 115x113 stats", dict(Cout=512, stats=True)),
                ("F T T", "1x1 512->1000 B2 115x113 bias res+acc", dict(Cout=1000, res=(115, 113), **RA)),        # last channel tile: 232 rows live
                ("T F F", "1x1 512->512 B2 115x113 f32out", dict(Cout=512, out_f32=True)),
                ("T T F", "1x1 512->1000 B2 115x113 bias f32out", dict(Cout=1000, bias=True, out_f32=True))]
    elif tc == 64:       # B3 29x27: 19 pixel tiles
        g = dict(dtype=dt, Cin=256, k=1, **S)
        rows = [("F F F", "1x1 256->64 stats", dict(Cout=64, stats=True)),
                ("F T T", "1x1 64->200 bias res+acc", dict(Cin=64, Cout=200, res=(29, 27), **RA)),                # 4 channel tiles, the last 8 rows live
                ("T F F", "1x1 256->128 f32out", dict(Cout=128, out_f32=True)),                                   # 2 channel tiles by workgroup count
                ("T T F", "1x1 256->100 bias f32out", dict(Cout=100, bias=True, out_f32=True))]                   # Cout_store 128, 36 of 64 rows live
    else:                # Cout_store 32
        g = dict(dtype=dt, Cin=256, **S)
        rows = [("F F F", "1x1 256->32 stats", dict(Cout=32, k=1, stats=True)),
                ("F T F", "3x3 256->17 bias", dict(Cout=17, k=3, bias=True)),                                     # 17 of 32 rows live, the 3x3 gather
                ("F T T", "1x1 256->24 bias res+acc", dict(Cout=24, k=1, res=(29, 27), **RA)),
                ("T F F", "3x3 s2 256->32 f32out", dict(Cout=32, k=3, stride=2, out_f32=True))]
    out = []
    for flags, what, extra in rows:
        o, gen, ext = [c == "T" for c in flags.split()]
        out.append(("%s %s" % (name, what), _inst(dt, big, out_f32=o, general=gen, ext=ext), C, dict(g, **extra)))
    return out


def _only(rows, keep):
    """The rows whose route's <OUTF32, GENERAL, EXT> is in `keep` ('T F F' ...)."""
    def flags(route):
        return " ".join("T" if a == "true" else "F" for a in route[:-1].split(", ")[3:])
    got = [r for r in rows if flags(r[1]) in keep]
    assert len(got) == len(keep), (keep, [r[0] for r in got])
    return got


IGEMM = (
    _only(_plain(BF, "bf16", 128), ("T F F", "T T F")) + _only(_plain(BF, "bf16", 256), ("T F F", "T T F")) + _only(_plain(BF, "bf16", 64), ("T T F",))
    + _plain(BF, "bf16", 32)
    + _only(_plain(H16, "f16", 128), ("F F F", "F T T", "T F F")) + _plain(H16, "f16", 256) + _plain(H16, "f16", 64) + _plain(H16, "f16", 32)
    + [("f32 3x3 256->32 stats", _inst(F32, 32), C, dict(dtype=F32, Cin=256, Cout=32, k=3, stats=True, **S)),
       ("f32 1x1 256->24 bias res+acc", _inst(F32, 32, ext=True), C, dict(dtype=F32, Cin=256, Cout=24, k=1, res=(29, 27), **RA, **S))]
)
assert len(IGEMM) == 26


def _s3(dt, name):
    """The conv_igemm_s3_kernel rows both 16-bit types need."""
    return [
        # 128 rows: 3x3 32 -> 256 / 200 at B3 67x65: 103 x 2 = 206 workgroups, 9 k-steps (< 16: not the 256-row tile)
        ("%s s3 3x3 32->256 B3 67x65 f32out" % name, _inst(dt, 128, s3=True, out_f32=True), C, dict(dtype=dt, Cin=32, Cout=256, k=3, out_f32=True, **Q)),
        # the class head over the pyramid at B2: levels 40, 20, 10, 5, 3 = 25 + 7 + 2 + 1 + 1 = 36 tiles x 6 channel tiles of Cout_store 736
        ("%s s3 pyramid 64->720 B2 bias sigmoid f32out" % name, _inst(dt, 128, s3=True, out_f32=True, general=True), PY,
         dict(dtype=dt, B=2, Cin=64, Cout=720, levels=(40, 20, 10, 5, 3), act=2, out_f32=True)),
        # the virtual concatenation below the 256-row rule: Cout_store 224 (72 of the second 128 rows live), B3 72x72 = 122 tiles (tail 64)
        ("%s s3 kseg 4x128->200 B3 72x72" % name, _inst(dt, 128, s3=True, ext=True), KS, dict(dtype=dt, B=3, H=72, W=72, Cout=200, kseg=True)),
        # ... and on the 64-row tile: B3 24x24 = 14 tiles (tail 64, an image is 4.5 tiles), 4 channel tiles, the last 8 rows live
        ("%s s3 kseg 4x128->200 B3 24x24" % name, _inst(dt, 64, s3=True, ext=True), KS, dict(dtype=dt, B=3, H=24, W=24, Cout=200, kseg=True)),
        ("%s s3 3x3 64->128 f32out" % name, _inst(dt, 64, s3=True, out_f32=True), C, dict(dtype=dt, Cin=64, Cout=128, k=3, out_f32=True, **S)),
    ]


S3 = _s3(BF, "bf16") + [
    # 256 rows: the class head over the pyramid at B4: levels 60, 30, 15, 8, 4 = 113 + 29 + 8 + 2 + 1 = 153 tiles x 3 channel tiles, 18 k-steps
    ("bf16 s3 pyramid 64->720 B4 bias sigmoid f32out", _inst(BF, 256, s3=True, out_f32=True, general=True), PY,
     dict(dtype=BF, B=4, Cin=64, Cout=720, levels=(60, 30, 15, 8, 4), act=2, out_f32=True)),
] + _s3(H16, "f16") + [
    ("f16 s3 3x3 32->256 B3 67x65 stats", _inst(H16, 128, s3=True), C, dict(dtype=H16, Cin=32, Cout=256, k=3, stats=True, **Q)),
    # 256 rows: 3x3 64 -> 1024 / 1000 at B3 67x65: 103 x 4 = 412 workgroups, 18 k-steps
    ("f16 s3 3x3 64->1024 B3 67x65 stats", _inst(H16, 256, s3=True), C, dict(dtype=H16, Cin=64, Cout=1024, k=3, stats=True, **Q)),
    ("f16 s3 3x3 64->1000 B3 67x65 bias sigmoid f32out", _inst(H16, 256, s3=True, out_f32=True, general=True), C,
     dict(dtype=H16, Cin=64, Cout=1000, k=3, bias=True, act=2, out_f32=True, **Q)),
    ("f16 s3 3x3 64->64 stats", _inst(H16, 64, s3=True), C, dict(dtype=H16, Cin=64, Cout=64, k=3, stats=True, **S)),
]
assert len(S3) == 15


# ------------------------------------------------------------------------------------- LDS-DMA weight gradients
W_, SEG = wt._conv_case, wt._seg_case
_lin, _dma, _seg = wt._lin, wt._dma, wt._seg
# Slice counts are mpn_conv_wgrad_chunks' (512 workgroups / tiles, at most one slice per 512 pixels).  Every family has a single-slice
# case (the kernel adds into dw / db itself) and one of several slices with a short last one; cin / cout tiles are ragged throughout.
WGRAD_DMA = [
    # bf16 gather <64, 128>: 3x3 / stride 2, odd extents
    ("bf16 dma 3x3 s2 40->200 B2 61x59", _dma(BF, 64, 128), W_,                          # 31 x 30 out, P = 1860: 4 slices of 480, last 420
     dict(dtype=BF, B=2, H=61, W=59, Cin=40, Cout=200, k=3, stride=2, chunks=4, last_slice=420)),
    ("bf16 dma 3x3 valid 40->72 B3 9x11 one slice", _dma(BF, 64, 128), W_,               # 7 x 9 out, P = 189
     dict(dtype=BF, B=3, H=9, W=11, Cin=40, Cout=72, k=3, pad=0, chunks=1)),
    # f16 gather
    ("f16 dma 3x3 s2 200->36 B2 61x59", _dma(H16, 128, 64), W_,
     dict(dtype=H16, B=2, H=61, W=59, Cin=200, Cout=36, k=3, stride=2, chunks=4, last_slice=420)),
    ("f16 dma 3x3 valid 40->72 B3 9x11 one slice", _dma(H16, 64, 128), W_,
     dict(dtype=H16, B=3, H=9, W=11, Cin=40, Cout=72, k=3, pad=0, chunks=1)),
    ("f16 dma 1x1 s2 40->19 B2 61x59", _dma(H16, 64, 64), W_,
     dict(dtype=H16, B=2, H=61, W=59, Cin=40, Cout=19, k=1, stride=2, chunks=4, last_slice=420)),
    # f32 gather
    ("f32 dma 3x3 s2 200->36 B2 61x59", _dma(F32, 128, 64), W_,                          # 4 slices of 480 (k-step 16), last 420
     dict(dtype=F32, B=2, H=61, W=59, Cin=200, Cout=36, k=3, stride=2, chunks=4, last_slice=420)),
    ("f32 dma 3x3 valid 40->72 B3 9x11 one slice", _dma(F32, 64, 128), W_,
     dict(dtype=F32, B=3, H=9, W=11, Cin=40, Cout=72, k=3, pad=0, chunks=1)),
    # f16 linear addressing
    ("f16 lin 3x3 200->36 B2 33x31", _lin(H16, 128, 64), W_,                             # P = 2046: 4 slices of 512, last 510
     dict(dtype=H16, B=2, H=33, W=31, Cin=200, Cout=36, k=3, chunks=4, last_slice=510)),
    ("f16 lin 3x3 64->200 B3 7x9 one slice", _lin(H16, 64, 128), W_,
     dict(dtype=H16, B=3, H=7, W=9, Cin=64, Cout=200, k=3, chunks=1)),
    ("f16 lin 1x1 40->19 B2 33x31", _lin(H16, 64, 64), W_,
     dict(dtype=H16, B=2, H=33, W=31, Cin=40, Cout=19, k=1, chunks=4, last_slice=510)),
    # pyramid, bf16
    ("bf16 seg 3x3 40->200 B2 p3..p7 bias", _seg(BF, 64, 128), SEG,
     dict(dtype=BF, B=2, Cin=40, Cout=200, k=3, levels=wt.P3P7, bias=True)),
    ("bf16 seg 3x3 40->19 B2 15,8,4,2,1 bias", _seg(BF, 64, 64), SEG,                    # one slice per level
     dict(dtype=BF, B=2, Cin=40, Cout=19, k=3, levels=(15, 8, 4, 2, 1), bias=True)),
    ("bf16 seg 3x3 40->19 B2 one level 15x15 one slice bias", _seg(BF, 64, 64), SEG,      # 450 pixels: the pyramid kernel's own add into dw / db
     dict(dtype=BF, B=2, Cin=40, Cout=19, k=3, levels=(15,), bias=True, slices=(1, 1))),
    # pyramid, f16
    ("f16 seg 3x3 256->36 B2 p3..p7 bias", _seg(H16, 128, 64), SEG,
     dict(dtype=H16, B=2, Cin=256, Cout=36, k=3, levels=wt.P3P7, bias=True)),
    ("f16 seg 1x1 40->200 B2 45,23,12,6,3", _seg(H16, 64, 128), SEG,
     dict(dtype=H16, B=2, Cin=40, Cout=200, k=1, levels=(45, 23, 12, 6, 3))),
    ("f16 seg 3x3 40->19 B2 15,8,4,2,1 bias", _seg(H16, 64, 64), SEG,
     dict(dtype=H16, B=2, Cin=40, Cout=19, k=3, levels=(15, 8, 4, 2, 1), bias=True)),
    ("f16 seg 3x3 40->200 B2 one level 15x15 one slice bias", _seg(H16, 64, 128), SEG,
     dict(dtype=H16, B=2, Cin=40, Cout=200, k=3, levels=(15,), bias=True, slices=(1, 1))),
]


# ------------------------------------------------------------------------------------- the generic weight gradient
# One geometry per <TM, TN>, the same for the three element types.  Cin 24 / 40 / 200 and Cout 19 / 36 / 200 give pick_tile's 32, 64
# and 128 with a ragged tile each (200 = a full 128-channel tile and 72 of the next).  Slices: tiles = cin tiles x cout tiles x taps,
# 512 / tiles of them for the 16-bit types and 768 / tiles for f32, at most one per 512 pixels; `slices` = (16-bit, f32) as
# (chunks, last slice).  B2 19x17: P = 646; B2 33x31: P = 2046; B2 29x27 / stride 2: 15 x 14, P = 420; B2 20x22 valid: 18 x 20, P = 720;
# B2 30x30: P = 1800.
GEOM = {
    (32, 32): ("3x3 24->19 B2 19x17", dict(B=2, H=19, W=17, Cin=24, Cout=19, k=3), ((2, 294), (2, 310))),
    (32, 64): ("1x1 24->36 B2 33x31 db", dict(B=2, H=33, W=31, Cin=24, Cout=36, k=1, bias=True), ((4, 510), (4, 510))),
    (32, 128): ("3x3 s2 24->200 B2 29x27 one slice", dict(B=2, H=29, W=27, Cin=24, Cout=200, k=3, stride=2), ((1, 420), (1, 420))),
    (64, 32): ("3x3 valid 40->19 B2 20x22", dict(B=2, H=20, W=22, Cin=40, Cout=19, k=3, pad=0), ((2, 336), (2, 352))),
    (64, 64): ("3x3 40->36 B2 7x9 one slice db", dict(B=2, H=7, W=9, Cin=40, Cout=36, k=3, bias=True), ((1, 126), (1, 126))),
    (64, 128): ("1x1 s2 64->200 B2 61x59", dict(B=2, H=61, W=59, Cin=64, Cout=200, k=1, stride=2), ((4, 420), (4, 420))),
    (128, 32): ("3x3 200->19 B2 19x17", dict(B=2, H=19, W=17, Cin=200, Cout=19, k=3), ((2, 294), (2, 310))),
    (128, 64): ("3x3 s2 72->36 B2 61x59 db", dict(B=2, H=61, W=59, Cin=72, Cout=36, k=3, stride=2, bias=True), ((4, 420), (4, 420))),
    (128, 128): ("3x3 200->200 B2 30x30", dict(B=2, H=30, W=30, Cin=200, Cout=200, k=3), ((4, 360), (4, 408))),
}
TNAME = {BF: "bf16", H16: "_Float16", F32: "float"}
WGRAD_GENERIC = []
for _dt, _nm in ((BF, "bf16"), (H16, "f16"), (F32, "f32")):
    for (_tm, _tn), (_what, _g, _sl) in GEOM.items():
        _c, _last = _sl[1 if _dt == F32 else 0]
        WGRAD_GENERIC.append(("%s generic %s" % (_nm, _what), "conv_wgrad_kernel<%s, %d, %d>" % (TNAME[_dt], _tm, _tn), _generic_case,
                              dict(dtype=_dt, chunks=_c, last_slice=_last, **_g)))
assert len(WGRAD_GENERIC) == 27

CASES = IGEMM + S3 + WGRAD_DMA + WGRAD_GENERIC


@pytest.mark.parametrize("case", CASES, ids=[c[0].replace(" ", "_") for c in CASES])
def test_conv_all_routes_parity(case):
    cid, route, runner, f = case
    runner(cid, route, f)


def test_narrow_channel_counts_are_refused_not_routed_to_the_generic_kernel():
    """mpn_conv_wgrad_kernel_name spells conv_wgrad_kernel<bf16, 64, 64> for Cin = 36, but mpn_conv_wgrad refuses the block (Cin % 8): the
    channel count is no way into the generic kernel, and nothing is written."""
    from multiposenet.pytorch_amd import _lib
    ops = wt._ops()
    for Cin in (36, 20):
        xa, dya = wt._act(rng_normal(1, 2, Cin, 9, 7), BF), wt._act(rng_normal(2, 2, 19, 9, 7), BF)
        dw0 = wt._prefill(3, 19, 3, 3, Cin)
        dw = dw0.clone().cuda()
        with wt._Launch(events=True) as L:
            with pytest.raises(_lib.MpnError, match="mpn_conv_wgrad failed with status"):
                ops.conv_wgrad(xa, dya, dw, 19, 3, 3, 1, 1)
        assert L.names == [] and torch.equal(wt._bits(dw), wt._bits(dw0)), Cin
        report("%-58s %-52s refused, dw untouched  OK" % ("bf16 wgrad 3x3 %d->19 B2 9x7" % Cin, "mpn_conv_wgrad: MPN_E_BADARG"))


def test_every_route_is_new_and_named_once_per_family():
    """The 82 instantiations of this file are exactly those the three older suites do not name."""
    older = set(c[1] for c in ct.CASES + st.CASES + wt.CASES)
    mine = set(c[1] for c in CASES)
    assert len(mine) == 82 and not (mine & older), sorted(mine & older)
    assert len(set(c[0] for c in CASES)) == len(CASES)
    for r in sorted(mine):
        report("all-routes coverage %-64s %d case(s)" % (r, sum(1 for c in CASES if c[1] == r)))
