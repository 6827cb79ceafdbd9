"""Element-wise parity of the weight-gradient kernels (csrc/conv_wgrad.hip) against float64.

launch_wgrad() picks its instantiation from the launch: wgrad_tiles() the cin / cout tile (64 or 128), wgrad_uses_dma() and
wgrad_lin_ok() the LDS-DMA kernel with linear or gathered x addressing, nseg / kseg_n the pyramid and virtual-concatenation forms, and
mpn_conv_wgrad_chunks() / mpn_conv_wgrad_seg_plan() the split-K slices.  Every case of CASES names the instantiation it must reach and
asserts it from ops.KERNEL_EVENTS before comparing anything.  Each case then

  * prefills dw and db with non-zero values (both are accumulated into) and gives every launch workspaces (ws, db_ws) full of NaN, so a
    slice that leaves its partial unwritten fails;
  * runs the plain path (mpn_conv_wgrad: slices and reduction in one call), the profiler-bracketed path (KERNEL_EVENTS on:
    mpn_conv_wgrad_partials + mpn_conv_wgrad_reduce) and the plain path again, and requires the same bits from all three;
  * compares every element of dw and of the fused db with the float64 gradient of the same operand values under
    helpers.check_elementwise, with K = the pixels of one slice and slices + 1 extra terms (tests/test_wgrad_parity_cpu.py shows
    that bound rejects a lost k-step, slice, halo tap, level or shift).

The slice plan of a launch is read from the parameter block the wrapper passed to the library (ops.call is wrapped for that), so the
bound uses the slices that actually ran.  The reduction kernels are held bit for bit to a NumPy float32 replica of their own order.

test_required_wgrad_routes_are_covered pins the weight-gradient and reduction instantiations of the round-6 traces."""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch.nn.grad import conv2d_weight

from helpers import check_elementwise, report, rng_normal, round_up

pytestmark = pytest.mark.gpu

BF, H16, F32 = torch.bfloat16, torch.float16, torch.float32


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests selected but no GPU is visible"
    from multiposenet.pytorch_amd import _lib
    _lib.lib()
    n = torch.get_num_threads()
    torch.set_num_threads(min(n, 16))
    yield
    torch.set_num_threads(n)


def _ops():
    from multiposenet.pytorch_amd import ops
    return ops


def _q(dtype, t):
    return t.to(dtype).double()


def _act(x_nchw, dtype):
    from multiposenet.pytorch_amd.ops import Act
    B, C, H, W = x_nchw.shape
    t = torch.zeros((B, H, W, round_up(C, 32)), dtype=torch.float32)
    t[..., :C] = x_nchw.permute(0, 2, 3, 1).float()
    return Act(t.to(dtype).cuda(), C)


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


class _Launch(object):
    """Runs a wrapper call with NaN-filled workspaces and records the MpnWgradParams blocks it passed to the library."""

    def __init__(self, events=False):
        self.events = events

    def __enter__(self):
        from multiposenet.pytorch_amd._lib import WgradParams
        ops = _ops()
        self.ops, self.params, self.calls, self.bufs = ops, [], [], []
        self._call, self._ws = ops.call, ops.workspace

        def call(name, *args):
            self.calls.append(name)
            if name in ("mpn_conv_wgrad", "mpn_conv_wgrad_partials"):
                self.params.append(WgradParams.from_buffer_copy(args[0]._obj))
            return self._call(name, *args)

        def workspace(nbytes, device, slot=0):
            t = torch.full(((int(nbytes) + 3) // 4 + 64,), float("nan"), dtype=torch.float32, device=device)
            self.bufs.append(t)
            return t.view(torch.uint8)
        ops.call, ops.workspace = call, workspace
        if self.events:
            ops.KERNEL_EVENTS.enable()
        return self

    def __exit__(self, *exc):
        ops = self.ops
        try:
            torch.cuda.synchronize()
            self.names = [r[0] for r in ops.KERNEL_EVENTS.rec] if self.events else []
        finally:
            ops.call, ops.workspace = self._call, self._ws
            ops.KERNEL_EVENTS.disable()
        return False


def _three_runs(cid, launch, dw0, db0):
    """Plain, bracketed, plain again.  Returns (dw, db, ret, names, params): all three give the same bits."""
    outs = []
    for events in (False, True, False):
        dw = dw0.clone().cuda()
        db = db0.clone().cuda() if db0 is not None else None
        with _Launch(events=events) as L:
            ret = launch(dw, db)
        outs.append((dw.cpu(), db.cpu() if db is not None else None, ret, L))
    (dw, db, ret, L0), (dwe, dbe, rete, Le), (dw2, db2, ret2, _) = outs
    assert ret == rete == ret2, (cid, ret, rete, ret2)
    assert torch.equal(_bits(dw), _bits(dw2)), "%s: a second plain run gave different dw bits" % cid
    assert torch.equal(_bits(dw), _bits(dwe)), "%s: dw of the profiler-bracketed path differs from the plain path" % cid
    if db is not None:
        assert torch.equal(_bits(db), _bits(db2)), "%s: a second plain run gave different db bits" % cid
        assert torch.equal(_bits(db), _bits(dbe)), "%s: db of the profiler-bracketed path differs from the plain path (%d slices)" % (
            cid, L0.params[0].chunks if L0.params else -1)
    assert len(L0.params) == 1, (cid, L0.calls)
    return dw, db, ret, Le.names, L0.params[0]


def _assert_route(cid, names, route):
    got = sorted(set(names))
    assert got == [route], "%s: launched %s, expected the route %s" % (cid, got, route)


def _slice_pixels(p, P, kp):
    """Pixels per slice of the launch p (launch_wgrad: ceil(P / chunks) rounded up to the k-step; pyramid: seg_chunk_pixels)."""
    if p.nseg > 0:
        return p.seg_chunk_pixels
    if p.chunks == 1:
        return P
    return round_up((P + p.chunks - 1) // p.chunks, kp)


def _prefill(seed, *shape):
    return (0.5 * rng_normal(seed, *shape)).float()


def _compare(cid, route, dw, db, ref, mag, dbref, dbmag, dw0, db0, k_step, K, slices):
    extra = slices + 1
    check_elementwise(cid + " dw", dw.double(), ref + dw0.double(), mag + dw0.double().abs(), F32, k_step, K, extra, route=route, names="orsc")
    if db is not None:
        check_elementwise(cid + " db", db.double(), dbref + db0.double(), dbmag + db0.double().abs(), F32, k_step, K, extra, route=route, names="o")


def _ref_wgrad(x, dy, R, S, stride, pad):
    """float64 weight gradient [Cout][R][S][Cin] and its magnitude sum |dy| |x|."""
    shape = (dy.shape[1], x.shape[1], R, S)
    g = conv2d_weight(x, shape, dy, stride=stride, padding=pad).permute(0, 2, 3, 1)
    m = conv2d_weight(x.abs(), shape, dy.abs(), stride=stride, padding=pad).permute(0, 2, 3, 1)
    return g, m


# ----------------------------------------------------------------------------------------------------- single-tensor launches
def _conv_case(cid, route, f):
    ops = _ops()
    dt, B, H, W, Cin, Cout, k = f["dtype"], f["B"], f["H"], f["W"], f["Cin"], f["Cout"], f["k"]
    stride, pad = f.get("stride", 1), f.get("pad", (k - 1) // 2)
    Ho, Wo = ops.conv_out_hw(H, W, k, k, stride, pad)
    seed = 3000 + sum(ord(c) for c in cid)
    x = _q(dt, rng_normal(seed, B, Cin, H, W))
    dy = _q(dt, rng_normal(seed + 1, B, Cout, Ho, Wo) * f.get("dy_scale", 1.0))
    if f.get("subnormal"):
        t = dy.abs()
        frac = float(((t > 0) & (t < 2.0 ** -14)).double().mean())
        assert frac > 0.5, "%s: only %.2f of dy is f16-subnormal" % (cid, frac)
        report("%-58s dy f16-subnormal fraction %.3f" % (cid, frac))
    if f.get("nonfinite"):
        p, o, v = f["nonfinite"]
        b, rem = divmod(p, Ho * Wo)
        dy[b, o, rem // Wo, rem % Wo] = v
    xa, dya = _act(x, dt), _act(dy, dt)
    dw0 = _prefill(seed + 2, Cout, k, k, Cin)
    db0 = _prefill(seed + 3, Cout) if f.get("bias", True) else None
    dw, db, fused, names, p = _three_runs(cid, lambda dw, db: ops.conv_wgrad(xa, dya, dw, Cout, k, k, stride, pad, db=db), dw0, db0)
    _assert_route(cid, names, route)
    if db0 is not None:
        assert fused is True, "%s: the LDS-DMA route must fuse the bias gradient" % cid
    if "chunks" in f:
        assert p.chunks == f["chunks"], "%s: %d slices, expected %d" % (cid, p.chunks, f["chunks"])
    if "slices" in f:
        lo, hi = f["slices"]
        assert lo <= p.chunks <= hi, "%s: %d slices, expected %d..%d" % (cid, p.chunks, lo, hi)
    P = B * Ho * Wo
    kp = 16 if dt == F32 else 32
    K = min(_slice_pixels(p, P, kp), P)
    if "last_slice" in f:
        last = max(0, P - (p.chunks - 1) * _slice_pixels(p, P, kp))
        assert last == f["last_slice"], "%s: last slice %d pixels, expected %d" % (cid, last, f["last_slice"])
    k_step = 4 if dt == F32 else 32
    fin = torch.isfinite(dy)
    ref, mag = _ref_wgrad(x, dy, k, k, stride, pad)
    dbref, dbmag = dy.sum((0, 2, 3)), dy.abs().sum((0, 2, 3))
    if f.get("nonfinite"):
        # exactly the elements the float64 reference makes NaN (or non-finite, for an Inf) are; the rest stay within the bound
        dz = torch.where(fin, dy, torch.zeros_like(dy))
        _, mag = _ref_wgrad(x, dz, k, k, stride, pad)
        dbmag = dz.abs().sum((0, 2, 3))
        isbad = torch.isnan if math.isnan(f["nonfinite"][2]) else (lambda t: ~torch.isfinite(t))
        for what, got, r in (("dw", dw, ref), ("db", db, dbref)):
            exp = isbad(r)
            assert bool(exp.any())
            assert torch.equal(isbad(got.double()), exp), "%s %s: non-finite at %d elements, float64 reference at %d (first mismatch %s)" % (
                cid, what, int(isbad(got.double()).sum()), int(exp.sum()), torch.nonzero(isbad(got.double()) != exp)[:1].tolist())
        bad_dw, bad_db = isbad(ref), isbad(dbref)
        dw, ref, dw0 = dw.masked_fill(bad_dw, 0.0), ref.masked_fill(bad_dw, 0.0), dw0.masked_fill(bad_dw, 0.0)
        db, dbref, db0 = db.masked_fill(bad_db, 0.0), dbref.masked_fill(bad_db, 0.0), db0.masked_fill(bad_db, 0.0)
    _compare(cid, route, dw, db, ref, mag, dbref, dbmag, dw0, db0, k_step, K, p.chunks)


def _stem_case(cid, route, f):
    """The stem as engine.py runs it: the 7x7x3 / stride 2 image convolution as a packed R=7, S=1, stride 2 convolution of 32
    'channels' (8 pixels x 4 slots of the NHWC4 image, x_sW = 4), then mpn_stem_unpack_wgrad into the [64][7][7][3] gradient."""
    ops = _ops()
    from multiposenet.pytorch_amd._lib import call
    from multiposenet.pytorch_amd.ops import Act
    dt, B, H, W = f["dtype"], f["B"], f["H"], f["W"]
    Hp, Wp = H + 6, W + 8
    Ho, Wo = ops.conv_out_hw(H, W, 7, 7, 2, 3)
    img = rng_normal(71, B, 3, H, W).cuda()
    packed = torch.empty((B, Hp, Wp, 4), dtype=dt, device="cuda")
    call("mpn_stem_pack_image", ops.ptr(img), img.stride(0), img.stride(1), img.stride(2), img.stride(3), ops.ptr(packed), B, H, W,
         ops.dtype_code(dt), ops.stream_ptr())
    xa = Act(packed, 4)
    geom = (Hp, Wp, Hp * Wp * 4, Wp * 4, 4)
    dy = _q(dt, rng_normal(72, B, 64, Ho, Wo))
    dya = _act(dy, dt)
    dwp0 = _prefill(73, 64, 7, 1, 32)
    dwp, _, _, names, p = _three_runs(cid, lambda dw, db: ops.conv_wgrad(xa, dya, dw, 64, 7, 1, 2, 0, cin=32, x_geom=geom), dwp0, None)
    _assert_route(cid, names, route)
    # float64 reference of the packed launch: channel j of output column wo reads element 8 wo + j of the packed image row
    X = packed.double().cpu().reshape(B, 1, Hp, Wp * 4)
    cols = F.unfold(X, (7, 32), stride=(2, 8))
    Lw = (Wp * 4 - 32) // 8 + 1
    cols = cols.view(B, 7 * 32, -1, Lw)[:, :, :Ho, :Wo].reshape(B, 7 * 32, Ho * Wo)
    d = dy.reshape(B, 64, Ho * Wo)
    g = torch.einsum("bol,bjl->oj", d, cols).view(64, 7, 1, 32)
    m = torch.einsum("bol,bjl->oj", d.abs(), cols.abs()).view(64, 7, 1, 32)
    P = B * Ho * Wo
    K = min(_slice_pixels(p, P, 32), P)
    _compare(cid, route, dwp, None, g, m, None, None, dwp0, None, 32, K, p.chunks)
    # unpack into a prefilled [64][7][7][3] gradient: against the float64 gradient of the 7x7x3 / stride 2 / pad 3 convolution
    img64 = _q(dt, img.cpu())
    g7, m7 = _ref_wgrad(img64, dy, 7, 7, 2, 3)
    gp = g.view(64, 7, 32)[:, :, :28].reshape(64, 7, 7, 4)
    assert torch.allclose(gp[..., 3], torch.zeros(()).double()), "slot 3 of the packed image is not zero"
    torch.testing.assert_close(gp[..., :3], g7, rtol=1e-12, atol=1e-9)          # the packing is exact: same sums, same terms
    dw0 = _prefill(74, 64, 7, 7, 3)
    dwr = dw0.clone().cuda()
    dwp_dev = dwp.cuda()
    call("mpn_stem_unpack_wgrad", ops.ptr(dwp_dev), ops.ptr(dwr), 64, ops.stream_ptr())
    torch.cuda.synchronize()
    dwp0_u = dwp0.view(64, 7, 32)[:, :, :28].reshape(64, 7, 7, 4)[..., :3].double()
    check_elementwise(cid + " unpacked 7x7x3", dwr.cpu().double(), g7 + dwp0_u + dw0.double(), m7 + dwp0_u.abs() + dw0.double().abs(), F32, 32,
                      K, p.chunks + 2, route="mpn_stem_unpack_wgrad", names="orsc")


# ----------------------------------------------------------------------------------------------------------------- pyramid
def _seg_case(cid, route, f):
    ops = _ops()
    from multiposenet.pytorch_amd._lib import WgradParams, call
    dt, B, Cin, Cout, k = f["dtype"], f["B"], f["Cin"], f["Cout"], f["k"]
    pad = (k - 1) // 2
    seed = 5000 + sum(ord(c) for c in cid)
    xs = [_q(dt, rng_normal(seed + 2 * i, B, Cin, s, s)) for i, s in enumerate(f["levels"])]
    dys = [_q(dt, rng_normal(seed + 2 * i + 1, B, Cout, s, s)) for i, s in enumerate(f["levels"])]
    xa, dya = [_act(x, dt) for x in xs], [_act(d, dt) for d in dys]
    dw0 = _prefill(seed + 20, Cout, k, k, Cin)
    db0 = _prefill(seed + 21, Cout) if f.get("bias") else None
    if dt == F32:
        # no f32 pyramid instantiation: the wrapper reports the launch unhandled and touches nothing (the engine then runs the levels
        # one by one)
        dw, db = dw0.clone().cuda(), db0.clone().cuda() if db0 is not None else None
        with _Launch() as L:
            r = ops.conv_wgrad_seg(xa, dya, dw, Cout, k, k, pad, db=db)
        assert r == (False, False) and not any(n.startswith("mpn_conv_wgrad") and n != "mpn_conv_wgrad_kernel_id" for n in L.calls), (r, L.calls)
        assert torch.equal(_bits(dw), _bits(dw0)) and (db is None or torch.equal(_bits(db), _bits(db0)))
        report("%-58s %-52s handled=False, dw/db untouched  OK" % (cid, route))
        return
    dw, db, ret, names, p = _three_runs(cid, lambda dw, db: ops.conv_wgrad_seg(xa, dya, dw, Cout, k, k, pad, db=db), dw0, db0)
    assert ret == (True, db0 is not None), (cid, ret)
    _assert_route(cid, names, route)
    # the slice plan the launch ran is mpn_conv_wgrad_seg_plan's
    q = WgradParams.from_buffer_copy(p)
    q.chunks, q.seg_chunk_pixels = 1, 0
    for i in range(6):
        q.seg_chunk0[i] = 0
    c = call("mpn_conv_wgrad_seg_plan", ctypes.byref(q))
    assert c == p.chunks and list(q.seg_chunk0) == list(p.seg_chunk0) and q.seg_chunk_pixels == p.seg_chunk_pixels, (
        c, list(q.seg_chunk0), list(p.seg_chunk0))
    cp, sizes = p.seg_chunk_pixels, [B * s * s for s in f["levels"]]
    assert list(p.seg_chunk0)[: len(sizes) + 1] == [0] + list(np.cumsum([(n + cp - 1) // cp for n in sizes]))
    report("%-58s slice plan: %d x %d pixels, seg_chunk0 %s, level pixels %s" % (cid, p.chunks, cp, list(p.seg_chunk0), sizes))
    if "slices" in f:
        lo, hi = f["slices"]
        assert lo <= p.chunks <= hi, "%s: %d slices, expected %d..%d" % (cid, p.chunks, lo, hi)
    ref = torch.zeros(Cout, k, k, Cin, dtype=torch.float64)
    mag = torch.zeros_like(ref)
    for x, d in zip(xs, dys):
        g, m = _ref_wgrad(x, d, k, k, 1, pad)
        ref, mag = ref + g, mag + m
    dbref = sum(d.sum((0, 2, 3)) for d in dys)
    dbmag = sum(d.abs().sum((0, 2, 3)) for d in dys)
    _compare(cid, route, dw, db, ref, mag, dbref, dbmag, dw0, db0, 32, cp, p.chunks)


# --------------------------------------------------------------------------------------------------- virtual concatenation
def _cat_case(cid, route, f):
    ops = _ops()
    dt, B, H, W, Cout, shifts = f["dtype"], f["B"], f["H"], f["W"], f["Cout"], f["shifts"]
    seed = 6000 + sum(ord(c) for c in cid)
    mem = [_q(dt, rng_normal(seed + s, B, 128, H >> s, W >> s)) for s in shifts]
    dy = _q(dt, rng_normal(seed + 9, B, Cout, H, W))
    srcs, dya = [_act(m, dt) for m in mem], _act(dy, dt)
    Cin = 128 * len(shifts)
    dw0 = _prefill(seed + 10, Cout, 3, 3, Cin)
    db0 = _prefill(seed + 11, Cout) if f.get("bias") else None
    dw, db, fused, names, p = _three_runs(cid, lambda dw, db: ops.conv_wgrad_cat(srcs, H, W, dya, dw, Cout, db=db), dw0, db0)
    assert fused is (db0 is not None)
    _assert_route(cid, names, route)
    assert p.kseg_n == len(shifts) and list(p.kseg_shift)[: len(shifts)] == list(shifts), (p.kseg_n, list(p.kseg_shift))
    if "slices" in f:
        lo, hi = f["slices"]
        assert lo <= p.chunks <= hi, "%s: %d slices, expected %d..%d" % (cid, p.chunks, lo, hi)
    x = torch.cat([m.repeat_interleave(1 << s, 2).repeat_interleave(1 << s, 3) for m, s in zip(mem, shifts)], 1)
    ref, mag = _ref_wgrad(x, dy, 3, 3, 1, 1)
    del x
    P = B * H * W
    _compare(cid, route, dw, db, ref, mag, dy.sum((0, 2, 3)), dy.abs().sum((0, 2, 3)), dw0, db0, 32, min(_slice_pixels(p, P, 32), P), p.chunks)


def _lin(dt, tm, tn):
    return "conv_wgrad_dma_lin%s_kernel<%d, %d>" % ({BF: "", H16: "_f16", F32: "_f32"}[dt], tm, tn)


def _dma(dt, tm, tn):
    return "conv_wgrad_dma%s_kernel<%d, %d>" % ({BF: "", H16: "_f16", F32: "_f32"}[dt], tm, tn)


def _seg(dt, tm, tn):
    return "conv_wgrad_dma_seg%s_kernel<%d, %d>" % ({BF: "", H16: "_f16"}[dt], tm, tn)


C, SEG, CAT = _conv_case, _seg_case, _cat_case
P3P7 = (60, 30, 15, 8, 4)          # p3..p7 of a 480 x 480 image
# (id, route, runner, features).  Slice counts are mpn_conv_wgrad_chunks' (target 512 workgroups / tiles, at most one slice per 512
# pixels, at most 256) and are asserted where a case exists for them.
CASES = [
    # bf16, linear addressing
    ("bf16 lin 3x3 200->72 B2 30x30", _lin(BF, 128, 128), C,                     # ragged cin tile (72 of 128 live) and cout (72 of 128)
     dict(dtype=BF, B=2, H=30, W=30, Cin=200, Cout=72, k=3, chunks=4)),
    ("bf16 lin 1x1 256->1024 B4 50x82 empty last slice", _lin(BF, 128, 128), C,   # 32 slices of 544 pixels: slice 31 empty, slice 30 80
     dict(dtype=BF, B=4, H=50, W=82, Cin=256, Cout=1024, k=1, chunks=32, last_slice=0)),
    ("bf16 lin 1x1 640->640 B2 45x115 short last slice", _lin(BF, 128, 128), C,   # 20 slices of 544: the last one 14 pixels (< a k-step)
     dict(dtype=BF, B=2, H=45, W=115, Cin=640, Cout=640, k=1, chunks=20, last_slice=14)),
    ("bf16 lin 3x3 256->256 B1 16x16 one slice", _lin(BF, 128, 128), C,           # chunks == 1: the kernel adds into dw / db itself
     dict(dtype=BF, B=1, H=16, W=16, Cin=256, Cout=256, k=3, chunks=1)),
    ("bf16 lin 1x1 128->128 B3 5x5 tiny images", _lin(BF, 128, 128), C,           # 25-pixel images, 75 pixels: one slice
     dict(dtype=BF, B=3, H=5, W=5, Cin=128, Cout=128, k=1, chunks=1)),
    ("bf16 lin 3x3 256->36 B2 90x90 head 28 slices", _lin(BF, 128, 64), C,
     dict(dtype=BF, B=2, H=90, W=90, Cin=256, Cout=36, k=3, chunks=28)),
    ("bf16 lin 3x3 256->9 B2 90x90 head 28 slices", _lin(BF, 128, 64), C,
     dict(dtype=BF, B=2, H=90, W=90, Cin=256, Cout=9, k=3, chunks=28)),
    ("bf16 lin 1x1 256->36 B2 60x100 24 slices", _lin(BF, 128, 64), C,
     dict(dtype=BF, B=2, H=60, W=100, Cin=256, Cout=36, k=1, chunks=24)),
    ("bf16 lin 1x1 256->36 B4 50x82 33 slices", _lin(BF, 128, 64), C,
     dict(dtype=BF, B=4, H=50, W=82, Cin=256, Cout=36, k=1, chunks=33)),
    ("bf16 lin 3x3 64->200 B2 40x40", _lin(BF, 64, 128), C,
     dict(dtype=BF, B=2, H=40, W=40, Cin=64, Cout=200, k=3)),
    ("bf16 lin 3x3 40->19 B3 7x9", _lin(BF, 64, 64), C,                           # 63-pixel images; cin 40 and cout 19 in 64-wide tiles
     dict(dtype=BF, B=3, H=7, W=9, Cin=40, Cout=19, k=3, chunks=1)),
    ("bf16 lin 1x1 40->19 B2 33x31", _lin(BF, 64, 64), C,
     dict(dtype=BF, B=2, H=33, W=31, Cin=40, Cout=19, k=1)),
    # bf16, general gather
    ("bf16 dma 3x3 s2 128->128 B2 61x59", _dma(BF, 128, 128), C,                  # first bottleneck of layer2: odd extents, 31 x 30 out
     dict(dtype=BF, B=2, H=61, W=59, Cin=128, Cout=128, k=3, stride=2)),
    ("bf16 dma 3x3 s2 256->256 B2 30x30", _dma(BF, 128, 128), C,                  # layer3
     dict(dtype=BF, B=2, H=30, W=30, Cin=256, Cout=256, k=3, stride=2)),
    ("bf16 dma 3x3 valid 64->64 B2 34x34", _dma(BF, 64, 64), C,
     dict(dtype=BF, B=2, H=34, W=34, Cin=64, Cout=64, k=3, pad=0)),
    ("bf16 dma stem 7x7x3 s2 B2 64x60", _dma(BF, 64, 64), _stem_case,
     dict(dtype=BF, B=2, H=64, W=60)),
    # pyramid
    ("bf16 seg 3x3 256->256 B2 p3..p7", _seg(BF, 128, 128), SEG,
     dict(dtype=BF, B=2, Cin=256, Cout=256, k=3, levels=P3P7)),
    ("bf16 seg 3x3 256->256 B2 15,8,4,2,1", _seg(BF, 128, 128), SEG,              # levels of 8 and 2 pixels (< a k-step)
     dict(dtype=BF, B=2, Cin=256, Cout=256, k=3, levels=(15, 8, 4, 2, 1))),
    ("bf16 seg 3x3 256->9 B2 p3..p7 bias", _seg(BF, 128, 64), SEG,               # 22 slices of 512
     dict(dtype=BF, B=2, Cin=256, Cout=9, k=3, levels=P3P7, bias=True, slices=(17, 31))),
    ("bf16 seg 3x3 256->36 B2 45,23,12,6,3 bias", _seg(BF, 128, 64), SEG,
     dict(dtype=BF, B=2, Cin=256, Cout=36, k=3, levels=(45, 23, 12, 6, 3), bias=True)),
    ("bf16 seg 1x1 256->36 B4 p3..p7 bias", _seg(BF, 128, 64), SEG,              # >= 32 slices
     dict(dtype=BF, B=4, Cin=256, Cout=36, k=1, levels=P3P7, bias=True, slices=(32, 256))),
    ("f32 seg 3x3 256->36 B2 p3..p7 unhandled", "per-level fallback", SEG,
     dict(dtype=F32, B=2, Cin=256, Cout=36, k=3, levels=P3P7, bias=True)),
    # virtual concatenation
    ("bf16 cat 4x128 (3,2,1,0)->128 B2 32x32 bias", _dma(BF, 128, 128), CAT,
     dict(dtype=BF, B=2, H=32, W=32, Cout=128, shifts=(3, 2, 1, 0), bias=True)),
    ("bf16 cat [q3,q2] 2x128 (1,0)->36 B2 96x96 bias", _dma(BF, 128, 64), CAT,    # 28 slices
     dict(dtype=BF, B=2, H=96, W=96, Cout=36, shifts=(1, 0), bias=True, slices=(17, 31))),
    # f16
    ("f16 lin 3x3 256->256 B2 30x30", _lin(H16, 128, 128), C,
     dict(dtype=H16, B=2, H=30, W=30, Cin=256, Cout=256, k=3)),
    ("f16 lin 1x1 128->128 B2 40x40 subnormal dy", _lin(H16, 128, 128), C,        # dy in 2^-24 .. 2^-14
     dict(dtype=H16, B=2, H=40, W=40, Cin=128, Cout=128, k=1, dy_scale=2.0 ** -17, subnormal=True)),
    ("f16 dma 3x3 s2 128->128 B2 61x59", _dma(H16, 128, 128), C,
     dict(dtype=H16, B=2, H=61, W=59, Cin=128, Cout=128, k=3, stride=2)),
    ("f16 seg 3x3 256->256 B2 p3..p7", _seg(H16, 128, 128), SEG,
     dict(dtype=H16, B=2, Cin=256, Cout=256, k=3, levels=P3P7)),
    # f32 (exact-fp32 MFMA, k-step 4)
    ("f32 lin 3x3 200->72 B2 30x30", _lin(F32, 128, 128), C,
     dict(dtype=F32, B=2, H=30, W=30, Cin=200, Cout=72, k=3)),
    ("f32 lin 1x1 128->36 B2 45x43", _lin(F32, 128, 64), C,
     dict(dtype=F32, B=2, H=45, W=43, Cin=128, Cout=36, k=1)),
    ("f32 lin 3x3 64->200 B2 40x40", _lin(F32, 64, 128), C,
     dict(dtype=F32, B=2, H=40, W=40, Cin=64, Cout=200, k=3)),
    ("f32 lin 3x3 32->16 B3 7x9", _lin(F32, 64, 64), C,
     dict(dtype=F32, B=3, H=7, W=9, Cin=32, Cout=16, k=3)),
    ("f32 dma 3x3 s2 128->128 B2 61x59", _dma(F32, 128, 128), C,
     dict(dtype=F32, B=2, H=61, W=59, Cin=128, Cout=128, k=3, stride=2)),
    ("f32 dma 3x3 valid 64->64 B2 34x34", _dma(F32, 64, 64), C,
     dict(dtype=F32, B=2, H=34, W=34, Cin=64, Cout=64, k=3, pad=0)),
    # non-finite dy: one NaN / one Inf at (pixel, output channel)
    ("bf16 lin 3x3 128->36 B2 40x40 NaN in dy", _lin(BF, 128, 64), C,
     dict(dtype=BF, B=2, H=40, W=40, Cin=128, Cout=36, k=3, nonfinite=(1234, 7, float("nan")))),
    ("bf16 lin 3x3 128->36 B2 40x40 Inf in dy", _lin(BF, 128, 64), C,
     dict(dtype=BF, B=2, H=40, W=40, Cin=128, Cout=36, k=3, nonfinite=(3199, 35, float("inf")))),
    ("f32 lin 1x1 128->36 B2 45x43 NaN in dy", _lin(F32, 128, 64), C,
     dict(dtype=F32, B=2, H=45, W=43, Cin=128, Cout=36, k=1, nonfinite=(0, 0, float("nan")))),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0].replace(" ", "_") for c in CASES])
def test_wgrad_route_parity(case):
    cid, route, runner, f = case
    runner(cid, route, f)


def test_empty_last_slice_through_the_c_abi():
    """1x1 256->1024 over 16 400 pixels: mpn_conv_wgrad_chunks gives 32 slices; launch_wgrad's slice length is 544 pixels, so
    slice 31 starts at 16 864 > 16 400 and is empty (its partial must still be written: the workspace is NaN in the parity case)."""
    from multiposenet.pytorch_amd._lib import BF16, WgradParams, call
    p = WgradParams()
    p.B, p.H, p.W, p.Ho, p.Wo, p.Cin, p.Cout = 4, 50, 82, 50, 82, 256, 1024
    p.x_sW, p.x_sH, p.x_sB, p.dy_sP = 256, 82 * 256, 50 * 82 * 256, 1024
    p.R, p.S, p.stride, p.pad, p.dtype, p.chunks = 1, 1, 1, 0, BF16, 1
    c = call("mpn_conv_wgrad_chunks", ctypes.byref(p))
    assert c == 32
    cp = round_up((16400 + c - 1) // c, 32)
    assert cp == 544 and (c - 1) * cp >= 16400 > (c - 2) * cp
    kid = call("mpn_conv_wgrad_kernel_id", ctypes.byref(p))
    assert (kid >> 16, (kid >> 4) & 0xfff, kid & 3) == (128, 128, 3)


# ------------------------------------------------------------------------------------------------------------------ reductions
def _replica(kernel, ws, dst, accumulate):
    """NumPy float32 replica of a reduction kernel's own order.  reduce_partials_kernel: dst (or 0) + ws[0] + ws[1] + ... in index
    order.  reduce_partials_small_kernel: 16 strided groups g = ws[s] + ws[s + 16] + ... (from 0), then dst (or 0) + g[0] + ... + g[15]."""
    chunks, n = ws.shape
    a = dst.copy() if accumulate else np.zeros(n, np.float32)
    if kernel == "reduce_partials_kernel":
        for c in range(chunks):
            a = (a + ws[c]).astype(np.float32)
        return a
    g = np.zeros((16, n), np.float32)
    for s in range(16):
        for c in range(s, chunks, 16):
            g[s] = (g[s] + ws[c]).astype(np.float32)
    for s in range(16):
        a = (a + g[s]).astype(np.float32)
    return a


def _reduce_kernel(chunks, n):
    """mpn_reduce_partials' dispatch rule."""
    return "reduce_partials_small_kernel" if (n <= 8192 and chunks >= 32) else "reduce_partials_kernel"


REDUCE_N = [1, 3, 5, 19, 36, 8191, 8192, 8193, 1000003]
REDUCE_CHUNKS = [1, 2, 16, 17, 31, 32, 33, 256]


@pytest.mark.parametrize("n", REDUCE_N)
def test_reduce_partials_bit_exact(n):
    ops = _ops()
    from multiposenet.pytorch_amd._lib import call
    rng = np.random.default_rng(n)
    for chunks in REDUCE_CHUNKS:
        if n > 10 ** 6 and chunks > 33:
            continue                     # 256 slices of 10^6 floats: a gigabyte for nothing the 33-slice case does not reach
        # magnitudes spread over 2^-10 .. 2^10 so that the order of the additions shows in the bits
        ws = (rng.standard_normal((chunks, n)) * np.exp2(rng.integers(-10, 11, (chunks, n)))).astype(np.float32)
        dst0 = rng.standard_normal(n).astype(np.float32)
        kernel = _reduce_kernel(chunks, n)
        wsd = torch.from_numpy(ws).cuda()
        for acc in (0, 1):
            dst = torch.from_numpy(dst0.copy()).cuda()
            call("mpn_reduce_partials", ops.ptr(wsd), chunks, n, ops.ptr(dst), acc, ops.stream_ptr())
            got = dst.cpu().numpy()
            exp = _replica(kernel, ws, dst0, acc)
            same = got.view(np.uint32) == exp.view(np.uint32)
            if not same.all():
                i = int(np.nonzero(~same)[0][0])
                raise AssertionError("%s chunks=%d n=%d accumulate=%d: element %d got %r, replica %r (%d elements differ)" % (
                    kernel, chunks, n, acc, i, float(got[i]), float(exp[i]), int((~same).sum())))
        report("%-58s %-52s chunks=%d n=%d bit-exact  OK" % ("reduce_partials", kernel, chunks, n))


def test_bias_grad_both_routes():
    """ops.bias_grad: mpn_colsum_rows (few rows, or a channel storage whose 16-byte groups are not a power of two) and
    mpn_channel_sum + mpn_reduce_partials, each against float64 column sums into a prefilled db."""
    ops = _ops()
    from multiposenet.pytorch_amd._lib import call
    from multiposenet.pytorch_amd.ops import Act
    cases = [  # (dtype, P, C, Cs, route by bias_grad's rule)
        (BF, 200, 36, 64, "mpn_colsum_rows"), (BF, 5000, 72, 96, "mpn_colsum_rows"), (BF, 16400, 36, 64, "mpn_channel_sum"),
        (BF, 300, 19, 32, "mpn_channel_sum"), (F32, 256, 200, 224, "mpn_colsum_rows"), (F32, 9000, 9, 32, "mpn_channel_sum"),
        (H16, 70000, 256, 256, "mpn_channel_sum"),
    ]
    for i, (dt, P, Cc, Cs, route) in enumerate(cases):
        v = 4 if dt == F32 else 8
        g = Cs // v
        rule = "mpn_colsum_rows" if (P <= 256 or Cs % v != 0 or (g & (g - 1)) != 0) else "mpn_channel_sum"
        assert rule == route, (dt, P, Cs, rule)
        t = torch.zeros(P, Cs)
        t[:, :Cc] = rng_normal(900 + i, P, Cc)
        t = t.to(dt)
        dy = Act(t.view(1, 1, P, Cs).cuda(), Cc)
        db0 = _prefill(950 + i, Cc)
        db = db0.clone().cuda()
        with _Launch() as L:
            ops.bias_grad(dy, db, Cc)
        assert route in L.calls, (route, L.calls)
        d64 = t[:, :Cc].double()
        if route == "mpn_colsum_rows":
            K, extra = P, 1                         # one sequential sum per channel, then the add into db
        else:
            # channel_sum_kernel: slices of `chunk` pixels (resample.hip cs_chunk), each summed by `lanes` strided lanes and then across
            # them — at most `chunk` sequential additions — then the slices added into db in order
            lanes = 256 // min(g, 256)
            chunk = min(max(P // 512, lanes * 4), 4096)
            chunk = (chunk + lanes - 1) // lanes * lanes
            chunks = call("mpn_channel_sum_chunks", P, Cs, ops.dtype_code(dt))
            assert chunks == (P + chunk - 1) // chunk
            K, extra = min(chunk, P), chunks + 1
        check_elementwise("bias_grad %s P=%d C=%d Cs=%d" % (str(dt), P, Cc, Cs), db.cpu().double(), db0.double() + d64.sum(0),
                          db0.double().abs() + d64.abs().sum(0), F32, 1, K, extra, route=route, names="c")


# Every weight-gradient and reduction instantiation of the round-6 traces (profiles/r06_kernel_trace_stats_serial.txt: cfg3, R101
# 480x480 B=32 bf16 training; profiles/r06_cfg4_kernel_trace_serial.txt: cfg4; profiles/r06_cfg2_kernel_trace_serial.txt: cfg2, R50
# 480x480 B=16 fp32).
REQUIRED_ROUTES = [
    # cfg3 / cfg4 (bf16)
    "conv_wgrad_dma_lin_kernel<128, 128>",
    "conv_wgrad_dma_lin_kernel<128, 64>",
    "conv_wgrad_dma_lin_kernel<64, 128>",
    "conv_wgrad_dma_lin_kernel<64, 64>",
    "conv_wgrad_dma_kernel<128, 128>",
    "conv_wgrad_dma_kernel<64, 64>",
    "conv_wgrad_dma_seg_kernel<128, 128>",
    "conv_wgrad_dma_seg_kernel<128, 64>",
    "reduce_partials_kernel",
    "reduce_partials_small_kernel",
    # cfg2 (fp32)
    "conv_wgrad_dma_lin_f32_kernel<128, 128>",
    "conv_wgrad_dma_lin_f32_kernel<128, 64>",
    "conv_wgrad_dma_lin_f32_kernel<64, 128>",
    "conv_wgrad_dma_lin_f32_kernel<64, 64>",
    "conv_wgrad_dma_f32_kernel<128, 128>",
    "conv_wgrad_dma_f32_kernel<64, 64>",
]


def test_required_wgrad_routes_are_covered():
    assert len(REQUIRED_ROUTES) == len(set(REQUIRED_ROUTES)) == 16
    reached = set(c[1] for c in CASES)
    reached |= set(_reduce_kernel(c, n) for n in REDUCE_N for c in REDUCE_CHUNKS)
    missing = [r for r in REQUIRED_ROUTES if r not in reached]
    for r in REQUIRED_ROUTES:
        report("wgrad route coverage %-56s %s" % (r, "reached" if r in reached else "MISSING"))
    assert not missing, "instantiations of the round-6 traces without a parity case: %s" % missing
