"""Element-wise parity of the 128- and 256-row conv_igemm tiles against float64.

conv_igemm.hip picks its instantiation from the launch size: pick_tc() the output-channel tile height, conv_uses_s3() the
shared-pixel-tile 3x3 kernel, launch_conv() the plain / general / extended epilogue.  A test reaches a route only through the
shape it launches, so every case of CASES names the route it must take, asserts it first (from the library's own
mpn_conv_kernel_name through ops.KERNEL_EVENTS, plus `ext` by conv_needs_ext()'s rule) and then compares
every element — outputs, pad lanes, per-tile statistics, BatchNorm-backward partials, the in-launch finalize — with a float64
reference of the same operand values under helpers.check_elementwise's bound (half an output spacing plus the linear
worst-case bound of the fp32 blocked summation).  Shapes carry the ragged edges: P not a multiple of 128, images that end
inside a pixel tile, Cout_store > Cout, a second channel tile that is only partly live.

test_required_routes_are_covered pins the set of 128/256-row instantiations the round-6 traces ran; a change of pick_tc that
moves a route fails a case's route assertion or needs a deliberate edit of that set."""
import math

import pytest
import torch
import torch.nn.functional as F

from helpers import U24, check_elementwise, report, rng_normal, round_up, ulp_out, w_krsc

pytestmark = pytest.mark.gpu

BF, H16, F32 = torch.bfloat16, torch.float16, torch.float32
TP = 128


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


def _route(name, ext):
    """KERNEL_EVENTS name -> the instantiation as the traces spell it (without the profiling flag): the extended epilogue is a
    general one, and its flag is appended."""
    base, args = name[:-1].split("<")
    a = [s.strip() for s in args.split(",")]
    if ext:
        a[4] = "true"
    return "%s<%s, %s>" % (base, ", ".join(a), "true" if ext else "false")


def _needs_ext(f):
    """conv_needs_ext(): BatchNorm-backward statistics with relu + z and no mask bits, a residual together with accumulate, the
    virtual concatenation (kseg) or a parity-class output (y_step)."""
    return bool((f.get("bnb") == "z") or (f.get("res") and f.get("acc")) or f.get("kseg") or f.get("ystep"))


def _launch(fn):
    ops = _ops()
    ops.KERNEL_EVENTS.enable()
    try:
        r = fn()
        torch.cuda.synchronize()
        names = [e[0] for e in ops.KERNEL_EVENTS.rec]
    finally:
        ops.KERNEL_EVENTS.disable()
    return r, names


def _assert_route(cid, names, ext, route):
    got = sorted(set(_route(n, ext) for n in names))
    assert got == [route], "%s: launched %s, expected the route %s" % (cid, got, route)


def _act(x_nchw, dtype, fill=0.0):
    """NHWC activation with 32-aligned channel storage; pad lanes hold `fill`."""
    from multiposenet.pytorch_amd.ops import Act
    B, C, H, W = x_nchw.shape
    t = torch.full((B, H, W, round_up(C, 32)), fill, dtype=torch.float32)
    t[..., :C] = x_nchw.permute(0, 2, 3, 1)
    return Act(t.to(dtype).cuda(), C)


def _nan_out(B, H, W, C, dtype):
    from multiposenet.pytorch_amd.ops import Act
    return Act(torch.full((B, H, W, round_up(C, 32)), float("nan"), dtype=dtype, device="cuda"), C)


def _nchw(a):
    return a.t[..., : a.C].double().cpu().permute(0, 3, 1, 2)


def _pad_lanes_zero(cid, a):
    if a.Cs > a.C:
        pad = a.t[..., a.C:].float()
        assert bool((pad == 0).all()), "%s: pad lanes [%d, %d) not zero (max |v| %r)" % (cid, a.C, a.Cs, float(pad.abs().nan_to_num(1e30).max()))


def _q(dtype, t):
    """Round f32 values through `dtype`, returned as float64 (the operand values the kernel sees)."""
    return t.to(dtype).double()


def _upsample(r, Ho, Wo):
    """The epilogue's nearest up-sampling: output (ho, wo) reads (ho * rH / Ho, wo * rW / Wo)."""
    rh = torch.arange(Ho) * r.shape[2] // Ho
    rw = torch.arange(Wo) * r.shape[3] // Wo
    return r[:, :, rh][:, :, :, rw]


def _tile_sums(v, terms):
    """[B, C, H, W] float64 -> per 128-pixel tile (pixel order b, h, w) sums of each term: [tiles, C, len(terms)] and their
    magnitudes Σ|term|."""
    B, C, H, W = v.shape
    P = B * H * W
    tiles = (P + TP - 1) // TP
    flat = [t.permute(0, 2, 3, 1).reshape(P, C) for t in terms]
    out, mag = [], []
    for f in flat:
        g = torch.zeros(tiles * TP, C, dtype=torch.float64)
        g[:P] = f
        g = g.view(tiles, TP, C)
        out.append(g.sum(1))
        mag.append(g.abs().sum(1))
    return torch.stack(out, 2), torch.stack(mag, 2)


def _check_stats(cid, route, y, stats, extra=(0, 0)):
    """Per-tile (Σy, Σy²) partials [tiles][Cout][2] against float64 sums of the STORED output y over each tile's pixels."""
    ref, mag = _tile_sums(y, [y, y * y])
    got = stats.double().cpu()
    for i, what in enumerate(("sum", "sum of squares")):
        check_elementwise("%s tile %s" % (cid, what), got[..., i], ref[..., i], mag[..., i], F32, 1, TP, extra[i], route=route, names="tc")


# ----------------------------------------------------------------------------------------------------------------- plain conv launches
def _conv_case(cid, route, f):
    ops = _ops()
    dt = f["dtype"]
    B, H, W, Cin, Cout, k = f["B"], f["H"], f["W"], f["Cin"], f["Cout"], f["k"]
    pad, mode = (k - 1) // 2, f.get("mode", 0)
    out_f32 = f.get("out_f32", False)
    odt = F32 if (out_f32 or dt == F32) else dt
    seed = 1000 + sum(ord(c) for c in cid)
    x = _q(dt, rng_normal(seed, B, Cin, H, W))
    wv = _q(dt, rng_normal(seed + 1, Cout, Cin, k, k) / math.sqrt(Cin * k * k))      # [Cout][Cin]: the GEMM the launch runs
    scale = (0.5 + torch.rand(Cout, generator=torch.Generator().manual_seed(seed + 2))) if f.get("scale") else None
    bias = 0.5 * rng_normal(seed + 3, Cout) if f.get("bias") else None
    act = f.get("act", 0)
    res = None
    if f.get("res"):
        rh, rw = f["res"]
        res = _q(odt, rng_normal(seed + 4, B, Cout, rh, rw))
    prev = _q(odt, rng_normal(seed + 5, B, Cout, H, W)) if f.get("acc") else None

    kw = dict(bias=bias.cuda() if bias is not None else None, scale=scale.cuda() if scale is not None else None, act=act, out_f32=out_f32,
              want_stats=f.get("stats", False))
    if prev is not None:
        kw["out"], kw["accumulate"] = _act(prev, odt), True
    else:
        kw["out"] = _nan_out(B, H, W, Cout, odt)
    if res is not None:
        kw["res"], kw["res_mode"] = _act(res, odt), (1 if res.shape[2:] == (H, W) else 2)
    bn = None
    if f.get("fin"):
        g = torch.Generator().manual_seed(seed + 6)
        gamma, beta = 0.5 + torch.rand(Cout, generator=g), 0.3 * torch.randn(Cout, generator=g)
        rm, rv = 0.1 * torch.randn(Cout, generator=g), 0.5 + torch.rand(Cout, generator=g)
        bn = (gamma, beta, rm, rv, 0.1, 1e-5)
        kw["bn_fin"] = ops.BNFinalize(gamma.cuda(), beta.cuda(), rm.cuda(), rv.cuda(), 0.1, 1e-5)
    if f.get("bnb"):
        g = torch.Generator().manual_seed(seed + 7)
        st = ops.BNState(Cout, "cuda")
        mean, invstd = 0.3 * torch.randn(Cout, generator=g), 0.5 + 1.5 * torch.rand(Cout, generator=g)
        st.mean.copy_(mean); st.invstd.copy_(invstd)
        st.scale.copy_(torch.randn(Cout, generator=g)); st.shift.copy_(0.3 * torch.randn(Cout, generator=g))
        yb = _q(dt, rng_normal(seed + 8, B, Cout, H, W))
        zb = _q(dt, rng_normal(seed + 9, B, Cout, H, W))
        ya, za = _act(yb, dt), _act(zb, dt)
        if f["bnb"] == "mask":          # the ReLU mask as bits (bn_act(want_mask=True) layout): one byte per 8 channels, bit e = z > 0
            bits = (za.t.float() > 0).view(B * H * W, za.Cs // 8, 8).to(torch.int32)
            za.mask = (bits << torch.arange(8, device="cuda", dtype=torch.int32)).sum(2).to(torch.uint8).contiguous()
        kw["bnb"] = ops.BNBackward(ya, za, st, True)

    if mode == 0:
        w_dev = w_krsc(wv.float(), dt)
        ref = F.conv2d(x, wv, padding=pad)
        mag = F.conv2d(x.abs(), wv.abs(), padding=pad)
        cin = None
    else:
        # input gradient: the launch's weight is the transpose of a forward filter wf [Cin][Cout] (forward conv Cout -> Cin)
        wf = wv.transpose(0, 1).contiguous()
        cin = round_up(Cin, 32)
        w_dev = torch.empty((Cout, k, k, cin), dtype=dt, device="cuda")
        ops.weight_transpose(wf.float().permute(0, 2, 3, 1).contiguous().cuda(), w_dev, Cin, k * k, Cout, cin)
        ref = F.conv_transpose2d(x, wf, padding=pad)
        mag = F.conv_transpose2d(x.abs(), wf.abs(), padding=pad)
        kw["mode"], kw["out_hw"], kw["cin"] = 1, (H, W), cin
    (out, stats), names = _launch(lambda: ops.conv_forward(_act(x, dt), w_dev, Cout, k, k, 1, pad, **kw))
    _assert_route(cid, names, _needs_ext(f), route)

    # float64 epilogue in mpn.h order: scale, bias, act 1 | then the residual stage (res, accumulate), act 3
    K = Cin * k * k
    k_step = 4 if dt == F32 else 32
    acc_bound = (K / k_step + k_step + 2) * U24 * mag
    if scale is not None:
        ref, mag, acc_bound = ref * scale.double().view(1, -1, 1, 1), mag * scale.double().view(1, -1, 1, 1), acc_bound * scale.double().view(1, -1, 1, 1)
    if bias is not None:
        ref, mag = ref + bias.double().view(1, -1, 1, 1), mag + bias.double().abs().view(1, -1, 1, 1)
    if act == 1:
        ref = ref.clamp(min=0)
    extra_abs = None
    if res is not None or prev is not None:
        # the staged value is stored in the output type before the residual stage reads it back: half a spacing at most
        extra_abs = 0.5 * ulp_out(ref.abs() + acc_bound, odt)
        if res is not None:
            r = _upsample(res, H, W)
            ref, mag = ref + r, mag + r.abs()
        if prev is not None:
            ref, mag = ref + prev, mag + prev.abs()
    if act == 3:
        ref = ref.clamp(min=0)
    got = _nchw(out)
    check_elementwise(cid, got, ref, mag, odt, k_step, K, extra_abs=extra_abs, route=route)
    _pad_lanes_zero(cid, out)

    if f.get("stats") and not f.get("fin"):
        _check_stats(cid, route, got, stats)
    if f.get("fin"):
        _check_fin(cid, route, got, stats, bn, kw["bn_fin"])
    if f.get("bnb"):
        # per-tile (Σg, Σg·x̂) with g = the stored dz where z > 0, x̂ = (y - mean) * invstd in fp32 (two roundings: extra terms)
        xh = (yb - mean.double().view(1, -1, 1, 1)) * invstd.double().view(1, -1, 1, 1)
        gz = got * (zb > 0)
        ref_p, mag_p = _tile_sums(gz, [gz, gz * xh])
        assert stats.coef is None and not stats.frozen, (cid, stats)          # no finalize asked for: the partial table comes back
        gp = stats.partial.double().cpu()
        check_elementwise("%s bnb sum g" % cid, gp[..., 0], ref_p[..., 0], mag_p[..., 0], F32, 1, TP, route=route, names="tc")
        check_elementwise("%s bnb sum g*xhat" % cid, gp[..., 1], ref_p[..., 1], mag_p[..., 1], F32, 1, TP, 3, route=route, names="tc")


def _check_fin(cid, route, y, st, bn, bn_dev):
    """In-launch finalize (the last workgroup of every channel tile): mean / invstd / scale / shift and the running statistics against
    float64 from the stored output, each within the bound the fp32 tile partials (K = 128 pixels each) propagate into it plus the
    fp32 roundings of its own formula."""
    ops = _ops()
    gamma, beta, rm0, rv0, mom, eps = [t.double() if torch.is_tensor(t) else t for t in bn]
    B, C, H, W = y.shape
    n = float(B * H * W)
    s1, s2 = y.sum((0, 2, 3)), (y * y).sum((0, 2, 3))
    e1 = (TP + 3) * U24 * y.abs().sum((0, 2, 3)) + 1e-15 * s1.abs()
    e2 = (TP + 3) * U24 * (y * y).sum((0, 2, 3)) + 1e-15 * s2
    mu = s1 / n
    var = (s2 / n - mu * mu).clamp(min=0)
    is64 = 1.0 / torch.sqrt(var + eps)
    sc64 = gamma * is64
    sh64 = beta - mu * sc64
    d_mu = e1 / n + U24 * mu.abs()
    d_var = e2 / n + 2 * mu.abs() * e1 / n + (e1 / n) ** 2
    d_is = is64 * (0.5 * d_var / (var + eps)) * 1.01 + U24 * is64
    d_sc = gamma.abs() * d_is + U24 * sc64.abs()
    d_sh = mu.abs() * d_sc + sc64.abs() * d_mu + 2 * U24 * ((mu * sc64).abs() + sh64.abs())
    rm64 = (1 - mom) * rm0 + mom * mu
    unb = var * n / (n - 1)
    rv64 = (1 - mom) * rv0 + mom * unb
    d_rm = mom * d_mu + 3 * U24 * (((1 - mom) * rm0).abs() + (mom * mu).abs())
    d_rv = mom * d_var * n / (n - 1) + 3 * U24 * (((1 - mom) * rv0).abs() + (mom * unb).abs())
    z = torch.zeros(C, dtype=torch.float64)
    for tag, gotv, refv, bound in (("mean", st.mean, mu, d_mu), ("invstd", st.invstd, is64, d_is), ("scale", st.scale, sc64, d_sc),
                                   ("shift", st.shift, sh64, d_sh), ("running mean", bn_dev.running_mean, rm64, d_rm),
                                   ("running var", bn_dev.running_var, rv64, d_rv)):
        check_elementwise("%s finalize %s" % (cid, tag), gotv.cpu(), refv, z, F32, 1, 0, extra_abs=bound, route=route, names="c")
    cnt = ops.fin_counters(torch.device("cuda", torch.cuda.current_device()))
    assert int(cnt.abs().sum()) == 0, "%s: fin_counters not back at zero: %s" % (cid, cnt.tolist())


# ----------------------------------------------------------------------------------------------------------------- special launches
def _ystep_case(cid, route, f):
    """Input gradient of a stride-2 3x3 convolution as four parity-class launches (mpn.h: y_step): every class, odd extents."""
    ops = _ops()
    dt, B, Hx, Wx, Cx, Cy = f["dtype"], f["B"], f["H"], f["W"], f["Cout"], f["Cin"]
    Hy, Wy = (Hx - 1) // 2 + 1, (Wx - 1) // 2 + 1
    dy = _q(dt, rng_normal(41, B, Cy, Hy, Wy))
    wf = _q(dt, rng_normal(42, Cy, Cx, 3, 3) / math.sqrt(Cx * 9))                       # forward conv Cx -> Cy, stride 2
    cin = round_up(Cy, 32)
    wt = torch.empty((Cx, 3, 3, cin), dtype=dt, device="cuda")
    ops.weight_transpose(wf.float().permute(0, 2, 3, 1).contiguous().cuda(), wt, Cy, 9, Cx, cin)
    out = _nan_out(B, Hx, Wx, Cx, dt)
    (o, _), names = _launch(lambda: ops.conv_forward(_act(dy, dt), wt, Cx, 3, 3, 2, 1, mode=1, out_hw=(Hx, Wx), cin=cin, out=out))
    assert len(names) == 4, names
    _assert_route(cid, names, _needs_ext(f), route)
    ref = F.conv_transpose2d(dy, wf, stride=2, padding=1)
    mag = F.conv_transpose2d(dy.abs(), wf.abs(), stride=2, padding=1)
    assert ref.shape[2:] == (Hx, Wx)
    got = _nchw(o)
    for a in (0, 1):
        for c in (0, 1):
            check_elementwise("%s class (%d,%d)" % (cid, a, c), got[:, :, a::2, c::2], ref[:, :, a::2, c::2], mag[:, :, a::2, c::2], dt, 32, 4 * Cy, route=route)
    _pad_lanes_zero(cid, o)


def _kseg_case(cid, route, f):
    """conv2 of the keypoint head: 3x3 over the virtual concatenation of four 128-channel members up-sampled by 8, 4, 2, 1."""
    ops = _ops()
    from multiposenet.pytorch_amd.ops import Act
    dt, B, H, W, Cout = f["dtype"], f["B"], f["H"], f["W"], f["Cout"]
    mem = [_q(dt, rng_normal(61 + s, B, 128, H >> s, W >> s)) for s in (3, 2, 1, 0)]
    w = _q(dt, rng_normal(66, Cout, 512, 3, 3) / math.sqrt(512 * 9))
    bias = 0.5 * rng_normal(67, Cout)
    srcs = [_act(m, dt) for m in mem]
    out, names = _launch(lambda: ops.conv_forward_cat(srcs, H, W, w_krsc(w.float(), dt), Cout, bias=bias.cuda(), act=1))
    _assert_route(cid, names, _needs_ext(f), route)
    x = torch.cat([m.repeat_interleave(H // m.shape[2], 2).repeat_interleave(W // m.shape[3], 3) for m in mem], 1)
    ref = F.conv2d(x, w, padding=1) + bias.double().view(1, -1, 1, 1)
    mag = F.conv2d(x.abs(), w.abs(), padding=1) + bias.double().abs().view(1, -1, 1, 1)
    del x
    check_elementwise(cid, _nchw(out), ref.clamp(min=0), mag, dt, 32, 9 * 512, route=route)
    _pad_lanes_zero(cid, out)
    assert isinstance(out, Act)


def _pyramid_case(cid, route, f):
    """The RetinaNet tower: one launch over every level of the pyramid (conv_forward_seg), each level compared on its own."""
    ops = _ops()
    dt, B, Cin, Cout = f["dtype"], f["B"], f["Cin"], f["Cout"]
    xs = [_q(dt, rng_normal(80 + i, B, Cin, s, s)) for i, s in enumerate(f["levels"])]
    w = _q(dt, rng_normal(88, Cout, Cin, 3, 3) / math.sqrt(Cin * 9))
    bias = 0.5 * rng_normal(89, Cout)
    acts = [_act(x, dt) for x in xs]
    outs, names = _launch(lambda: ops.conv_forward_seg(acts, w_krsc(w.float(), dt), Cout, 3, 3, 1, bias=bias.cuda(), act=1))
    _assert_route(cid, names, _needs_ext(f), route)
    for s, x, o in zip(f["levels"], xs, outs):
        ref = (F.conv2d(x, w, padding=1) + bias.double().view(1, -1, 1, 1)).clamp(min=0)
        mag = F.conv2d(x.abs(), w.abs(), padding=1) + bias.double().abs().view(1, -1, 1, 1)
        check_elementwise("%s level %dx%d" % (cid, s, s), _nchw(o), ref, mag, dt, 32, 9 * Cin, route=route)
        _pad_lanes_zero(cid, o)


def _inst(dt, tc, s3=False, out_f32=False, general=False, ext=False):
    return "%s<%s, %d, 128, %s, %s, %s>" % ("conv_igemm_s3_kernel" if s3 else "conv_igemm_kernel", {BF: "bf16", H16: "_Float16", F32: "float"}[dt],
                                            tc, str(out_f32).lower(), str(general or ext).lower(), str(ext).lower())


C = _conv_case
# (id, route, runner, features).  Pixel tiles / tail of the last tile and the channel tiles are in the comments; each route was
# derived by hand from pick_tc and is asserted by the case itself.
CASES = [
    # bf16, 256-row tile
    ("bf16 s3 3x3 64->300 B4 91x91 bias relu", _inst(BF, 256, s3=True, general=True), C,        # 259 tiles (tail 100) x 2 channel tiles, Cout_store 320
     dict(dtype=BF, B=4, H=91, W=91, Cin=64, Cout=300, k=3, bias=True, act=1)),
    ("bf16 s3 3x3 256->256 B4 115x113 fwd f32out", _inst(BF, 256, s3=True, out_f32=True), C,      # 407 tiles (tail 12), images end inside tiles
     dict(dtype=BF, B=4, H=115, W=113, Cin=256, Cout=256, k=3, out_f32=True)),
    ("bf16 s3 3x3 256->256 B4 115x113 dgrad f32out", _inst(BF, 256, s3=True, out_f32=True), C,
     dict(dtype=BF, B=4, H=115, W=113, Cin=256, Cout=256, k=3, out_f32=True, mode=1)),
    ("bf16 s3 3x3 256->256 B4 115x113 stats", _inst(BF, 256, s3=True), C,
     dict(dtype=BF, B=4, H=115, W=113, Cin=256, Cout=256, k=3, stats=True)),
    ("bf16 s3 kseg 4x128->256 B5 120x104", _inst(BF, 256, s3=True, ext=True), _kseg_case,         # 488 tiles (tail 64)
     dict(dtype=BF, B=5, H=120, W=104, Cout=256, kseg=True)),
    ("bf16 1x1 512->512 B2 115x113 stats", _inst(BF, 256), C,                                     # 204 tiles (tail 6) x 2
     dict(dtype=BF, B=2, H=115, W=113, Cin=512, Cout=512, k=1, stats=True)),
    ("bf16 1x1 512->1000 B2 115x113 bias", _inst(BF, 256, general=True), C,                       # x 4 channel tiles, the last 232 rows live
     dict(dtype=BF, B=2, H=115, W=113, Cin=512, Cout=1000, k=1, bias=True)),
    ("bf16 1x1 512->1000 B2 115x113 res+acc", _inst(BF, 256, ext=True), C,
     dict(dtype=BF, B=2, H=115, W=113, Cin=512, Cout=1000, k=1, bias=True, res=(115, 113), acc=True)),
    # bf16, 128-row tile
    ("bf16 1x1 256->1024 B4 30x30", _inst(BF, 128), C,                                            # 29 tiles (tail 16) x 8
     dict(dtype=BF, B=4, H=30, W=30, Cin=256, Cout=1024, k=1)),
    ("bf16 1x1 256->1024 B4 30x30 res2 15x15", _inst(BF, 128, general=True), C,
     dict(dtype=BF, B=4, H=30, W=30, Cin=256, Cout=1024, k=1, res=(15, 15))),
    ("bf16 1x1 dgrad 1024->256 B16 30x30", _inst(BF, 128), C,                                     # 113 tiles (tail 64) x 2
     dict(dtype=BF, B=16, H=30, W=30, Cin=1024, Cout=256, k=1, mode=1)),
    ("bf16 1x1 256->1024 B8 25x21 res2 13x11 bias", _inst(BF, 128, general=True), C,              # 33 tiles (tail 104) x 8; non-2x ratio
     dict(dtype=BF, B=8, H=25, W=21, Cin=256, Cout=1024, k=1, res=(13, 11), bias=True)),
    ("bf16 1x1 dgrad 256->1024 B8 30x30 bnb z", _inst(BF, 128, ext=True), C,                      # 57 tiles (tail 32) x 8
     dict(dtype=BF, B=8, H=30, W=30, Cin=256, Cout=1024, k=1, mode=1, bnb="z")),
    ("bf16 1x1 dgrad 256->1024 B8 30x30 bnb mask", _inst(BF, 128, general=True), C,
     dict(dtype=BF, B=8, H=30, W=30, Cin=256, Cout=1024, k=1, mode=1, bnb="mask")),
    ("bf16 1x1 256->1024 B1 60x60 stats finalize", _inst(BF, 128), C,                             # 29 tiles (<= 64: in-launch) x 8
     dict(dtype=BF, B=1, H=60, W=60, Cin=256, Cout=1024, k=1, stats=True, fin=True)),
    ("bf16 s3 3x3 256->256 B31 30x30", _inst(BF, 128, s3=True), C,                                # 218 tiles (tail 124) x 2
     dict(dtype=BF, B=31, H=30, W=30, Cin=256, Cout=256, k=3)),
    ("bf16 s3 3x3 256->256 B31 30x30 bias relu", _inst(BF, 128, s3=True, general=True), C,
     dict(dtype=BF, B=31, H=30, W=30, Cin=256, Cout=256, k=3, bias=True, act=1)),
    ("bf16 dgrad s2 classes 128->256 B4 121x119", _inst(BF, 128, ext=True), _ystep_case,          # classes of 115, 113, 113, 111 tiles x 2
     dict(dtype=BF, B=4, H=121, W=119, Cin=128, Cout=256, ystep=True)),
    # f16 (folded-BN inference: act 3 = scale + shift + residual, then ReLU)
    ("f16 s3 3x3 256->256 B2 163x161 act3", _inst(H16, 256, s3=True, general=True), C,            # 411 tiles (tail 6)
     dict(dtype=H16, B=2, H=163, W=161, Cin=256, Cout=256, k=3, scale=True, bias=True, res=(163, 161), act=3)),
    ("f16 1x1 1024->256 B2 163x161 act3", _inst(H16, 256, general=True), C,
     dict(dtype=H16, B=2, H=163, W=161, Cin=1024, Cout=256, k=1, scale=True, bias=True, res=(163, 161), act=3)),
    ("f16 s3 3x3 256->256 B2 163x161 f32out", _inst(H16, 256, s3=True, out_f32=True), C,
     dict(dtype=H16, B=2, H=163, W=161, Cin=256, Cout=256, k=3, out_f32=True)),
    ("f16 s3 kseg 4x128->256 B5 120x104", _inst(H16, 256, s3=True, ext=True), _kseg_case,
     dict(dtype=H16, B=5, H=120, W=104, Cout=256, kseg=True)),
    ("f16 s3 3x3 256->256 B8 45x43 act3", _inst(H16, 128, s3=True, general=True), C,              # 121 tiles (tail 120) x 2
     dict(dtype=H16, B=8, H=45, W=43, Cin=256, Cout=256, k=3, scale=True, bias=True, res=(45, 43), act=3)),
    ("f16 1x1 256->1024 B8 45x43 act3", _inst(H16, 128, general=True), C,                         # x 8 (k-steps 8 < 16: not 256 rows)
     dict(dtype=H16, B=8, H=45, W=43, Cin=256, Cout=1024, k=1, scale=True, bias=True, res=(45, 43), act=3)),
    ("f16 1x1 256->1024 B8 45x43 bias", _inst(H16, 128, general=True), C,
     dict(dtype=H16, B=8, H=45, W=43, Cin=256, Cout=1024, k=1, bias=True)),
    ("f16 1x1 256->1024 B8 45x43 bias f32out", _inst(H16, 128, out_f32=True, general=True), C,
     dict(dtype=H16, B=8, H=45, W=43, Cin=256, Cout=1024, k=1, bias=True, out_f32=True)),
    # pyramid: RetinaNet tower, levels 60, 30, 15, 8, 4 (338 + 85 + 22 + 6 + 2 = 453 tiles)
    ("bf16 s3 pyramid 256->256 B12", _inst(BF, 256, s3=True, general=True), _pyramid_case,
     dict(dtype=BF, B=12, Cin=256, Cout=256, levels=(60, 30, 15, 8, 4))),
    # f32 (exact-fp32 MFMA, k_step 4): 104 tiles (tail 16) x 2
    ("f32 1x1 256->256 B1 120x110", _inst(F32, 128), C,
     dict(dtype=F32, B=1, H=120, W=110, Cin=256, Cout=256, k=1)),
    ("f32 1x1 256->200 B1 120x110 bias", _inst(F32, 128, general=True), C,
     dict(dtype=F32, B=1, H=120, W=110, Cin=256, Cout=200, k=1, bias=True)),
    ("f32 1x1 256->200 B1 120x110 res+acc", _inst(F32, 128, ext=True), C,
     dict(dtype=F32, B=1, H=120, W=110, Cin=256, Cout=200, k=1, bias=True, res=(120, 110), acc=True)),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0].replace(" ", "_") for c in CASES])
def test_conv_tile_route_parity(case):
    cid, route, runner, f = case
    runner(cid, route, f)


# Every conv_igemm instantiation with a 128- or 256-row tile in the round-6 traces (profiles/r06_kernel_trace_stats_serial.txt: cfg3,
# R101 480x480 B=32 bf16 training; profiles/r06_cfg5_kernel_trace.txt: cfg5, R101 640x640 B=64 f16 inference, mangled names there;
# profiles/r06_cfg2_kernel_trace_serial.txt: cfg2, R50 480x480 B=16 fp32).  Template arguments: <T, TC, TP, OUTF32, GENERAL, EXT>
# (the trailing profiling flag dropped).
REQUIRED_ROUTES = [
    # bf16 (cfg3): 12
    "conv_igemm_kernel<bf16, 128, 128, false, false, false>",
    "conv_igemm_kernel<bf16, 128, 128, false, true, false>",
    "conv_igemm_kernel<bf16, 128, 128, false, true, true>",
    "conv_igemm_kernel<bf16, 256, 128, false, false, false>",
    "conv_igemm_kernel<bf16, 256, 128, false, true, false>",
    "conv_igemm_kernel<bf16, 256, 128, false, true, true>",
    "conv_igemm_s3_kernel<bf16, 128, 128, false, false, false>",
    "conv_igemm_s3_kernel<bf16, 128, 128, false, true, false>",
    "conv_igemm_s3_kernel<bf16, 256, 128, false, false, false>",
    "conv_igemm_s3_kernel<bf16, 256, 128, false, true, false>",
    "conv_igemm_s3_kernel<bf16, 256, 128, false, true, true>",
    "conv_igemm_s3_kernel<bf16, 256, 128, true, false, false>",
    # f16 (cfg5): 7
    "conv_igemm_s3_kernel<_Float16, 256, 128, false, true, false>",
    "conv_igemm_kernel<_Float16, 128, 128, false, true, false>",
    "conv_igemm_kernel<_Float16, 256, 128, false, true, false>",
    "conv_igemm_s3_kernel<_Float16, 128, 128, false, true, false>",
    "conv_igemm_s3_kernel<_Float16, 256, 128, false, true, true>",
    "conv_igemm_s3_kernel<_Float16, 256, 128, true, false, false>",
    "conv_igemm_kernel<_Float16, 128, 128, true, true, false>",
    # f32 (cfg2): 3
    "conv_igemm_kernel<float, 128, 128, false, false, false>",
    "conv_igemm_kernel<float, 128, 128, false, true, false>",
    "conv_igemm_kernel<float, 128, 128, false, true, true>",
]


def test_required_routes_are_covered():
    assert len(REQUIRED_ROUTES) == len(set(REQUIRED_ROUTES)) == 22
    asserted = set(c[1] for c in CASES)
    missing = [r for r in REQUIRED_ROUTES if r not in asserted]
    for r in REQUIRED_ROUTES:
        report("route coverage %-64s %s" % (r, "reached" if r in asserted else "MISSING"))
    assert not missing, "instantiations of the round-6 traces without a parity case: %s" % missing
