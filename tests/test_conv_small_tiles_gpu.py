"""Element-wise parity of the 64- and 32-row conv_igemm tiles, the strided gathers and the loaded dgrad epilogue against float64.

Same construction as tests/test_conv_tiles_gpu.py (whose helpers this file imports): every case of CASES names the route it must
take, asserts it from the library's own name, and then compares every element with a float64 reference of the operand values the
kernel sees under helpers.check_elementwise.  What this tier adds:

* ConvCfg<T, 64 | 32, 128>: the tiles of every launch with Cout_store <= 64 and of every launch with fewer than 200 128-row
  workgroups — other WTC / LPP / PPI / NIT, another store-group size and other row arithmetic in both statistics reductions;
* the gathers: forward stride 2, the non-shared-tile 3x3 of the 16-bit types, every f32 3x3, the plain mode 1 / stride 2 gather,
  the one-tap parity class, the stem's 7x1 / stride 2 row convolution through x_geom;
* the loaded dgrad epilogue: the residual through res_mask bits, BatchNorm-backward partials with the mask recomputed from
  y * scale + shift, without ReLU, on parity-class launches that share one table, and with the in-launch backward finalize;
* act = 2 (sigmoid).

The references and checks are plain CPU functions of the operands (`_ref`, `_check_out`, `_check_bnb`, `_check_classes`,
`_check_onetap`): tests/test_conv_small_tiles_cpu.py feeds them modelled results to show what they accept and what they reject, and
pins every case's route without a GPU.  Shapes: 29x27 B=3 is P = 2349 = 19 pixel tiles (tail 45), its stride-2 image 15x14 is
P = 630 = 5 tiles (tail 118); images end inside tiles in both."""
import contextlib
import math
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

import loss_ref
import stream_ref
from helpers import U24, check_elementwise, report, rng_normal, round_up, ulp_out, w_krsc
from test_conv_tiles_gpu import (BF, F32, H16, TP, _act, _assert_route, _check_fin, _check_stats, _inst, _launch, _nan_out, _nchw, _need_gpu,  # noqa: F401
                                 _needs_ext, _ops, _pad_lanes_zero, _q, _tile_sums, _upsample)

pytestmark = pytest.mark.gpu


def _vec(dt):
    return 4 if dt == F32 else 8


def _k_step(dt):
    return 4 if dt == F32 else 32


def _hw_out(H, W, k, stride, pad):
    return (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1


def _pc(t):
    """[B, C, H, W] -> [P, C] in pixel order (b, h, w)."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def _unpc(t, like):
    B, C, H, W = like.shape
    return t.reshape(B, H, W, C).permute(0, 3, 1, 2)


def _c(v):
    return v.double().view(1, -1, 1, 1)


def pack_bits(z_store, dt):
    """bn_act(want_mask=True) layout from the stored tensor [B, H, W, Cs]: one byte per 16-byte chunk, bit e = z > 0 (built as
    test_conv_tiles_gpu._conv_case builds za.mask)."""
    V = _vec(dt)
    B, H, W, Cs = z_store.shape
    bits = (z_store.float() > 0).view(B * H * W, Cs // V, V).to(torch.int32)
    return (bits << torch.arange(V, device=z_store.device, dtype=torch.int32)).sum(2).to(torch.uint8).contiguous()


# ----------------------------------------------------------------------------------------------------------------- references (CPU)
def _ref(cid, f):
    """Operands (rounded through their storage types, float64) and the float64 reference of one plain launch: forward or input
    gradient, any stride, the stem, with the epilogue in mpn.h order — scale, bias, act 1 | 2, then the residual stage (res through
    optional mask bits, accumulate), act 3."""
    dt = f["dtype"]
    B, H, W, Cin, Cout, k = f["B"], f["H"], f["W"], f["Cin"], f["Cout"], f["k"]
    stride, mode, pad = f.get("stride", 1), f.get("mode", 0), (f["k"] - 1) // 2
    odt = F32 if (f.get("out_f32") or dt == F32) else dt
    seed = 2000 + sum(ord(c) for c in cid)
    R = SimpleNamespace(dt=dt, odt=odt, seed=seed, pad=pad, k_step=_k_step(dt))
    if f.get("stem"):
        # 7x7 / stride 2 / pad 3 over 3 channels; the launch contracts 7 rows x 32 packed slots (8 columns x 4 channels, zeros included)
        R.x = _q(dt, rng_normal(seed, B, 3, H, W))
        R.wv = _q(dt, rng_normal(seed + 1, 64, 3, 7, 7) / 12.0)
        R.Ho, R.Wo = _hw_out(H, W, 7, 2, 3)
        ref, mag, R.K = F.conv2d(R.x, R.wv, stride=2, padding=3), F.conv2d(R.x.abs(), R.wv.abs(), stride=2, padding=3), 7 * 32
    else:
        R.x = _q(dt, rng_normal(seed, B, Cin, H, W))
        R.wv = _q(dt, rng_normal(seed + 1, Cout, Cin, k, k) / math.sqrt(Cin * k * k))     # [Cout][Cin]: the GEMM the launch runs
        R.K = Cin * k * k
        if mode == 0:
            R.Ho, R.Wo = _hw_out(H, W, k, stride, pad)
            ref, mag = F.conv2d(R.x, R.wv, stride=stride, padding=pad), F.conv2d(R.x.abs(), R.wv.abs(), stride=stride, padding=pad)
        else:
            # input gradient: the launch's weight is the transpose of a forward filter wf [Cin][Cout] (forward conv Cout -> Cin)
            R.Ho, R.Wo = f.get("out_hw", (H, W))
            R.wf = R.wv.transpose(0, 1).contiguous()
            op = (R.Ho - ((H - 1) * stride - 2 * pad + k), R.Wo - ((W - 1) * stride - 2 * pad + k))
            ref = F.conv_transpose2d(R.x, R.wf, stride=stride, padding=pad, output_padding=op)
            mag = F.conv_transpose2d(R.x.abs(), R.wf.abs(), stride=stride, padding=pad, output_padding=op)
    assert tuple(ref.shape) == (B, Cout, R.Ho, R.Wo), (cid, ref.shape)
    Ho, Wo = R.Ho, R.Wo
    R.scale = (0.5 + torch.rand(Cout, generator=torch.Generator().manual_seed(seed + 2))) if f.get("scale") else None
    R.bias = 0.5 * rng_normal(seed + 3, Cout) if f.get("bias") else None
    R.res = _q(odt, rng_normal(seed + 4, B, Cout, *f["res"])) if f.get("res") else None
    R.prev = _q(odt, rng_normal(seed + 5, B, Cout, Ho, Wo)) if f.get("acc") else None
    R.zr = _q(odt, rng_normal(seed + 10, B, Cout, Ho, Wo)) if f.get("res_mask") else None
    act = f.get("act", 0)

    acc_bound = (R.K / R.k_step + R.k_step + 2) * U24 * mag
    if R.scale is not None:
        ref, mag, acc_bound = ref * _c(R.scale), mag * _c(R.scale), acc_bound * _c(R.scale)
    if R.bias is not None:
        ref, mag = ref + _c(R.bias), mag + _c(R.bias).abs()
        acc_bound = acc_bound + (R.K / R.k_step + R.k_step + 2) * U24 * _c(R.bias).abs()
    R.pre, R.pre_bound = ref, acc_bound                  # the float64 pre-activation and the accumulation bound of it
    if act == 1:
        ref = ref.clamp(min=0)
    if act == 2:
        ref = torch.sigmoid(ref)
    R.staged = ref
    R.extra_abs = None
    if R.res is not None or R.prev is not None:
        # the staged value is stored in the output type before the residual stage reads it back: half a spacing at most
        R.extra_abs = 0.5 * ulp_out(ref.abs() + acc_bound, odt)
        if R.res is not None:
            r = _upsample(R.res, Ho, Wo)
            if R.zr is not None:
                r = r * (R.zr > 0)
            ref, mag = ref + r, mag + r.abs()
        if R.prev is not None:
            ref, mag = ref + R.prev, mag + R.prev.abs()
    if act == 3:
        ref = ref.clamp(min=0)
    R.ref, R.mag = ref, mag
    if f.get("bnb"):
        _bnb_operands(R, f, seed, B, Cout, Ho, Wo)
    return R


def _bnb_operands(R, f, seed, B, C, Ho, Wo):
    """The BatchNorm whose dz the launch completes: mean / invstd / scale / shift (f32), its input y and output z (storage type), and for
    the in-launch finalize gamma and the prefilled dgamma / dbeta."""
    g = torch.Generator().manual_seed(seed + 7)
    R.mean, R.invstd = 0.3 * torch.randn(C, generator=g), 0.5 + 1.5 * torch.rand(C, generator=g)
    R.bscale, R.bshift = torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g)
    R.yb = _q(R.odt, rng_normal(seed + 8, B, C, Ho, Wo))
    R.zb = _q(R.odt, rng_normal(seed + 9, B, C, Ho, Wo))
    R.gamma, R.dg0, R.db0 = 0.5 + torch.rand(C, generator=g), torch.randn(C, generator=g), torch.randn(C, generator=g)


def relu_mask(how, R):
    """(float64 0/1 mask of g over [B, C, H, W], ambiguity mask or None) of the launch's bnb mode: 'z' / 'mask' the stored z > 0, 're' the
    sign of y * scale + shift recomputed in the epilogue (stream_ref.relu_pos: either sign accepted within 3 roundings of zero), 'norelu'
    none."""
    C = R.yb.shape[1]
    mode = {"z": "z", "mask": "bits", "re": "remask", "norelu": "none"}[how]
    pos, amb = stream_ref.relu_pos(mode, _pc(R.zb), _pc(R.yb), R.bscale, R.bshift, C)
    return (None if pos is None else _unpc(pos, R.yb)), (None if amb is None else _unpc(amb, R.yb))


# ----------------------------------------------------------------------------------------------------------------- checks (CPU)
def _check_out(cid, route, f, R, got):
    """Every output element.  act 2: ref = sigmoid(a); the allowance is the accumulation bound of a times the largest sigmoid' over
    [a - bound, a + bound] (at most 1/4) plus (R_EXP + 2) 2^-24 ref for expf, the addition and the division (loss_ref.check_sigmoid's
    terms); f32 output, so no output rounding."""
    if f.get("act") == 2:
        assert R.odt == F32 and R.extra_abs is None
        t = (R.pre.abs() - R.pre_bound).clamp(min=0)          # the point of the interval nearest 0, where sigmoid' is largest
        s = torch.sigmoid(t)
        return check_elementwise(cid, got, R.ref, R.ref, F32, extra_abs=R.pre_bound * s * (1 - s) + loss_ref.TINY, route=route,
                                 **stream_ref.roundings(loss_ref.R_EXP + 2))
    return check_elementwise(cid, got, R.ref, R.mag, R.odt, R.k_step, R.K, extra_abs=R.extra_abs, route=route)


AMBIGUOUS_MAX = 1e-3          # share of live elements whose recomputed ReLU sign may be ambiguous


def _bnb_sums(cid, how, R, got, sel=None):
    """Reference per-tile (sum g, sum g * xhat) of the STORED dx `got` with g masked: (ref [tiles, C, 2], mag, extra_abs or None, ambiguous
    share).  sel: the class slice (a, c) of a parity-class launch, tiles over the class's pixels in class order."""
    pos, amb = relu_mask(how, R)
    xh = (R.yb - _c(R.mean)) * _c(R.invstd)
    cut = (lambda t: t) if sel is None else (lambda t: t[:, :, sel[0]::2, sel[1]::2])
    g = cut(got)
    gz = g if pos is None else g * cut(pos)
    xh = cut(xh)
    ref_p, mag_p = _tile_sums(gz, [gz, gz * xh])
    extra, share = None, 0.0
    if amb is not None:
        a = cut(amb)
        share = float(a.mean())
        _, extra = _tile_sums(g, [g * a, g * a * xh])           # sum |g| and sum |g xhat| of the tile's ambiguous elements
    return ref_p, mag_p, extra, share


def _check_partials(cid, route, part, ref_p, mag_p, extra):
    gp = part.double().cpu()
    for i, (what, terms) in enumerate((("bnb sum g", 0), ("bnb sum g*xhat", 3))):
        check_elementwise("%s %s" % (cid, what), gp[..., i], ref_p[..., i], mag_p[..., i], F32, 1, TP, terms,
                          extra_abs=None if extra is None else extra[..., i], route=route, names="tc")


def _check_bnb(cid, route, f, R, got, part):
    """part: the launch's [tiles][C][2] table."""
    ref_p, mag_p, extra, share = _bnb_sums(cid, f["bnb"], R, got)
    assert share <= AMBIGUOUS_MAX, "%s: %.4f of the elements have an ambiguous recomputed ReLU sign" % (cid, share)
    _check_partials(cid, route, part, ref_p, mag_p, extra)


def _check_bnb_fin(cid, route, f, R, part, dgamma, dbeta, fused, count):
    """In-launch backward finalize (fused: the launch's ops.BNBackwardResult) against the device's own partial table `part`: dgamma /
    dbeta accumulated onto their prefill, and (train) the [3][C] k1 / k2 / k3 of dy = k1 g + k2 y + k3."""
    train = f["bnb_fin"] == "train"
    assert fused.partial is None, (cid, fused)          # a finalized launch keeps its partial table to itself
    if train:
        assert not fused.frozen and torch.is_tensor(fused.coef) and tuple(fused.coef.shape) == (3, R.yb.shape[1]), (cid, fused)
    else:
        assert fused.frozen is True and fused.coef is None, (cid, fused)
    stream_ref.check_bwd_finalize(cid + " finalize ", part.cpu(), count, R.gamma, R.mean, R.invstd, R.dg0, R.db0, train, dgamma, dbeta,
                                  fused.coef if train else None, route)


def _class_ref(cid, f):
    """Input gradient of a 3x3 (taps 9) or 1x1 (taps 1) / stride 2 convolution: dx [B, Cout, H, W] from dy [B, Cin, Hy, Wy]."""
    dt, B, Hx, Wx, Cx, Cy, k = f["dtype"], f["B"], f["H"], f["W"], f["Cout"], f["Cin"], f.get("k", 3)
    pad = (k - 1) // 2
    Hy, Wy = (Hx - 1) // 2 + 1, (Wx - 1) // 2 + 1
    seed = 3000 + sum(ord(c) for c in cid)
    R = SimpleNamespace(dt=dt, odt=dt, k=k, pad=pad, k_step=_k_step(dt), Hy=Hy, Wy=Wy)
    R.dy = _q(dt, rng_normal(seed, B, Cy, Hy, Wy))
    R.wf = _q(dt, rng_normal(seed + 1, Cy, Cx, k, k) / math.sqrt(Cx * k * k))              # forward conv Cx -> Cy, stride 2
    op = (Hx - ((Hy - 1) * 2 - 2 * pad + k), Wx - ((Wy - 1) * 2 - 2 * pad + k))
    R.ref = F.conv_transpose2d(R.dy, R.wf, stride=2, padding=pad, output_padding=op)
    R.mag = F.conv_transpose2d(R.dy.abs(), R.wf.abs(), stride=2, padding=pad, output_padding=op)
    assert tuple(R.ref.shape) == (B, Cx, Hx, Wx)
    R.prev = _q(dt, rng_normal(seed + 5, B, Cx, Hx, Wx)) if f.get("acc") else None
    if f.get("bnb"):
        _bnb_operands(R, f, seed, B, Cx, Hx, Wx)
    return R


def _check_classes(cid, route, f, R, got, part=None):
    """Four parity classes: class (a, c) owns the pixels (2 i + a, 2 j + c) and contracts (1 + a)(1 + c) taps; the shared partial table's
    row ranges follow ops.dgrad_s2_class_plan."""
    from multiposenet.pytorch_amd.ops import dgrad_s2_class_plan
    B, Cx, Hx, Wx = R.ref.shape
    Cy = R.dy.shape[1]
    plan = dgrad_s2_class_plan(B, Hx, Wx)
    if part is not None:
        assert tuple(part.shape) == (sum(t for _, _, _, _, t, _ in plan), Cx, 2), (cid, part.shape)
    amb_n = 0.0
    for a, c, ho, wo, t, tile0 in plan:
        s = (slice(None), slice(None), slice(a, None, 2), slice(c, None, 2))
        ref, mag, extra_abs = R.ref[s], R.mag[s], None
        K = (1 + a) * (1 + c) * Cy
        assert tuple(ref.shape[2:]) == (ho, wo)
        if R.prev is not None:
            extra_abs = 0.5 * ulp_out(ref.abs() + (K / R.k_step + R.k_step + 2) * U24 * mag, R.odt)
            ref, mag = ref + R.prev[s], mag + R.prev[s].abs()
        check_elementwise("%s class (%d,%d)" % (cid, a, c), got[s], ref, mag, R.odt, R.k_step, K, extra_abs=extra_abs, route=route)
        if part is not None:
            ref_p, mag_p, extra, share = _bnb_sums(cid, f["bnb"], R, got, sel=(a, c))
            amb_n += share * ref.numel()
            assert ref_p.shape[0] == t
            _check_partials("%s class (%d,%d)" % (cid, a, c), route, part[tile0: tile0 + t], ref_p, mag_p, extra)
    assert amb_n <= AMBIGUOUS_MAX * R.ref.numel(), "%s: %d elements have an ambiguous recomputed ReLU sign" % (cid, amb_n)


def _check_onetap(cid, route, f, R, got_raw, prefill_raw):
    """1x1 / stride 2 input gradient into an existing dx: class (0, 0) receives its one tap on top of the prefill; every other pixel keeps
    the prefill bit for bit (raw storage tensors [B, H, W, Cs], pad lanes included)."""
    keep = torch.ones(got_raw.shape[1:3], dtype=torch.bool)
    keep[::2, ::2] = False
    same = torch.equal(got_raw[:, keep], prefill_raw[:, keep])
    report("%-58s %-52s pixels outside class (0,0) keep the prefill  %s" % (cid, route, "OK" if same else "FAIL"))
    assert same, "%s: a pixel outside class (0, 0) changed" % cid
    C = R.ref.shape[1]
    got = got_raw[..., :C].double().permute(0, 3, 1, 2)
    s = (slice(None), slice(None), slice(0, None, 2), slice(0, None, 2))
    K = R.dy.shape[1]
    extra_abs = 0.5 * ulp_out(R.ref[s].abs() + (K / R.k_step + R.k_step + 2) * U24 * R.mag[s], R.odt)
    check_elementwise("%s class (0,0)" % cid, got[s], R.ref[s] + R.prev[s], R.mag[s] + R.prev[s].abs(), R.odt, R.k_step, K, extra_abs=extra_abs,
                      route=route)


def _gather_zeros(cid, route, got):
    """A 1x1 / stride 2 gather into a fresh output: every pixel with an odd row or column is exactly 0."""
    z = got.clone()
    z[:, :, ::2, ::2] = 0
    ok = bool((z == 0).all())
    report("%-58s %-52s odd rows / columns exactly zero  %s" % (cid, route, "OK" if ok else "FAIL"))
    assert ok, "%s: a pixel with an odd row or column is not exactly 0" % cid


# ----------------------------------------------------------------------------------------------------------------- launches (GPU)
@contextlib.contextmanager
def _tables(shape):
    """ops.conv_forward keeps the partial table of an in-launch finalize to itself (its `keep`): record every f32 tensor of the table's
    shape allocated while the launch is set up, so the finalize can be checked against the device's own partials."""
    real, seen = torch.empty, []

    def empty(*a, **k):
        t = real(*a, **k)
        if tuple(t.shape) == tuple(shape) and t.dtype == F32:
            seen.append(t)
        return t
    torch.empty = empty
    try:
        yield seen
    finally:
        torch.empty = real


def _dgrad_weight(wf, dt, k):
    """The launch's weight [Cx][k][k][cin] from the forward filter wf [Cy][Cx][k][k] through ops.weight_transpose."""
    ops = _ops()
    Cy, Cx = wf.shape[:2]
    cin = round_up(Cy, 32)
    wt = torch.empty((Cx, k, k, cin), dtype=dt, device="cuda")
    ops.weight_transpose(wf.float().permute(0, 2, 3, 1).contiguous().cuda(), wt, Cy, k * k, Cx, cin)
    return wt, cin


def _bnb_device(R, f):
    """The ops.BNBackward (ya, za | None, BNState, relu; no finalize) that ops.conv_forward takes."""
    ops = _ops()
    C = R.yb.shape[1]
    st = ops.BNState(C, "cuda")
    st.mean.copy_(R.mean); st.invstd.copy_(R.invstd); st.scale.copy_(R.bscale); st.shift.copy_(R.bshift)
    ya, za, how = _act(R.yb, R.odt), None, f["bnb"]
    if how in ("z", "mask"):
        za = _act(R.zb, R.odt)
        if how == "mask":
            za.mask = pack_bits(za.t, R.odt)
    return ops.BNBackward(ya, za, st, how != "norelu")


def _conv_case(cid, route, f):
    ops = _ops()
    from multiposenet.pytorch_amd import _lib
    R = _ref(cid, f)
    dt, odt = R.dt, R.odt
    B, H, W, Cin, Cout, k = f["B"], f["H"], f["W"], f["Cin"], f["Cout"], f["k"]
    Ho, Wo = R.Ho, R.Wo
    kw = dict(bias=R.bias.cuda() if R.bias is not None else None, scale=R.scale.cuda() if R.scale is not None else None, act=f.get("act", 0),
              out_f32=f.get("out_f32", False), want_stats=f.get("stats", False))
    if R.prev is not None:
        kw["out"], kw["accumulate"] = _act(R.prev, odt), True
    else:
        kw["out"] = _nan_out(B, Ho, Wo, Cout, odt)
    if R.res is not None:
        kw["res"], kw["res_mode"] = _act(R.res, odt), (1 if tuple(R.res.shape[2:]) == (Ho, Wo) else 2)
        if R.zr is not None:
            kw["res_mask"] = pack_bits(_act(R.zr, odt).t, odt)
    bn = None
    if f.get("fin"):
        g = torch.Generator().manual_seed(R.seed + 6)
        gamma, beta = 0.5 + torch.rand(Cout, generator=g), 0.3 * torch.randn(Cout, generator=g)
        rm, rv = 0.1 * torch.randn(Cout, generator=g), 0.5 + torch.rand(Cout, generator=g)
        bn = (gamma, beta, rm, rv, 0.1, 1e-5)
        kw["bn_fin"] = ops.BNFinalize(gamma.cuda(), beta.cuda(), rm.cuda(), rv.cuda(), 0.1, 1e-5)
    tiles = (B * Ho * Wo + TP - 1) // TP
    dgamma = dbeta = None
    if f.get("bnb"):
        kw["bnb"] = _bnb_device(R, f)
        if f.get("bnb_fin"):
            dgamma, dbeta = R.dg0.cuda(), R.db0.cuda()
            kw["bnb"] = kw["bnb"]._replace(fin=ops.BNBackwardFinalize(R.gamma.cuda(), f["bnb_fin"] == "train", dgamma, dbeta))

    if f.get("stem"):
        Hp, Wp = H + 6, W + 8
        xg = R.x.float().cuda()
        packed = torch.empty((B, Hp, Wp, 4), dtype=dt, device="cuda")
        _lib.call("mpn_stem_pack_image", ops.ptr(xg), xg.stride(0), xg.stride(1), xg.stride(2), xg.stride(3), ops.ptr(packed), B, H, W,
                  ops.dtype_code(dt), ops.stream_ptr())
        wk = R.wv.float().permute(0, 2, 3, 1).contiguous().cuda()                              # master layout [64][7][7][3] f32
        wp = torch.empty((64, 7, 32), dtype=dt, device="cuda")
        _lib.call("mpn_stem_pack_weight", ops.ptr(wk), ops.ptr(wp), 64, ops.dtype_code(dt), ops.stream_ptr())
        xa = ops.Act(packed, 4)

        def run():
            return ops.conv_forward(xa, wp, 64, 7, 1, 2, 0, cin=32, x_geom=(Hp, Wp, Hp * Wp * 4, Wp * 4, 4), out_hw=(Ho, Wo), **kw)
    elif f.get("mode", 0) == 0:
        w_dev = w_krsc(R.wv.float(), dt)

        def run():
            return ops.conv_forward(_act(R.x, dt), w_dev, Cout, k, k, f.get("stride", 1), R.pad, **kw)
    else:
        w_dev, cin = _dgrad_weight(R.wf, dt, k)

        def run():
            return ops.conv_forward(_act(R.x, dt), w_dev, Cout, k, k, f.get("stride", 1), R.pad, mode=1, out_hw=(Ho, Wo), cin=cin, **kw)
    with _tables((tiles, Cout, 2)) as seen:
        (out, stats), names = _launch(run)
    assert len(names) == 1, names
    _assert_route(cid, names, _needs_ext(f), route)

    got = _nchw(out)
    _check_out(cid, route, f, R, got)
    _pad_lanes_zero(cid, out)
    if f.get("mode", 0) == 1 and f.get("stride", 1) == 2 and k == 1:
        _gather_zeros(cid, route, got)
    if f.get("stats") and not f.get("fin"):
        _check_stats(cid, route, got, stats)
    if f.get("fin"):
        _check_fin(cid, route, got, stats, bn, kw["bn_fin"])
    if f.get("bnb"):
        assert isinstance(stats, ops.BNBackwardResult), (cid, stats)
        part = stats.partial
        if f.get("bnb_fin") and ops.fin_in_launch(tiles, Cout):
            assert len(seen) == 1, "%s: %d partial tables allocated" % (cid, len(seen))
            part = seen[0]
            _check_bnb_fin(cid, route, f, R, part, dgamma, dbeta, stats, float(B * Ho * Wo))
        elif f.get("bnb_fin"):
            # more pixel tiles than one workgroup finishes: the table comes back, dgamma / dbeta are left to the finalize launch
            assert torch.is_tensor(part) and tuple(part.shape) == (tiles, Cout, 2) and stats.coef is None and not stats.frozen, (cid, stats)
            assert torch.equal(dgamma.cpu(), R.dg0) and torch.equal(dbeta.cpu(), R.db0), "%s: dgamma / dbeta touched without a finalize" % cid
        _check_bnb(cid, route, f, R, got, part)
        cnt = ops.fin_counters(torch.device("cuda", torch.cuda.current_device()))
        assert int(cnt.abs().sum()) == 0, "%s: fin_counters not back at zero: %s" % (cid, cnt.tolist())


def _class_case(cid, route, f):
    """3x3 / stride 2 input gradient as four parity-class launches: fresh or accumulated dx, BatchNorm-backward partials in one table."""
    ops = _ops()
    R = _class_ref(cid, f)
    dt = R.dt
    B, Cx, Hx, Wx = R.ref.shape
    wt, cin = _dgrad_weight(R.wf, dt, 3)
    out = _act(R.prev, dt) if R.prev is not None else _nan_out(B, Hx, Wx, Cx, dt)
    bnb = _bnb_device(R, f) if f.get("bnb") else None
    (o, fused), names = _launch(lambda: ops.conv_forward(_act(R.dy, dt), wt, Cx, 3, 3, 2, 1, mode=1, out_hw=(Hx, Wx), cin=cin, out=out,
                                                         accumulate=R.prev is not None, bnb=bnb))
    assert len(names) == 4, names
    _assert_route(cid, names, _needs_ext(f), route)
    assert (fused is not None) == bool(f.get("bnb"))
    part = None
    if fused is not None:          # the four classes share one table; class launches never finalize
        assert fused.partial is not None and fused.coef is None and not fused.frozen, (cid, fused)
        part = fused.partial
    _check_classes(cid, route, f, R, _nchw(o), part)
    _pad_lanes_zero(cid, o)


def _onetap_case(cid, route, f):
    """1x1 / stride 2 input gradient into an existing dx: one launch of the one-tap class."""
    ops = _ops()
    R = _class_ref(cid, f)
    dt = R.dt
    B, Cx, Hx, Wx = R.ref.shape
    wt, cin = _dgrad_weight(R.wf, dt, 1)
    out = _act(R.prev, dt, fill=0.25)                     # pad lanes of the prefill carry a value: they must come back unchanged, too
    prefill = out.t.cpu().clone()
    (o, _), names = _launch(lambda: ops.conv_forward(_act(R.dy, dt), wt, Cx, 1, 1, 2, 0, mode=1, out_hw=(Hx, Wx), cin=cin, out=out, accumulate=True))
    assert len(names) == 1, names
    _assert_route(cid, names, _needs_ext(f), route)
    assert o is out
    _check_onetap(cid, route, f, R, o.t.cpu(), prefill)


def _pyramid_ref(cid, f):
    dt, B, Cin, Cout = f["dtype"], f["B"], f["Cin"], f["Cout"]
    seed = 4000 + sum(ord(c) for c in cid)
    w = _q(dt, rng_normal(seed + 8, Cout, Cin, 3, 3) / math.sqrt(Cin * 9))
    bias = 0.5 * rng_normal(seed + 9, Cout)
    levels = []
    for i, s in enumerate(f["levels"]):
        R = SimpleNamespace(dt=dt, odt=F32 if f.get("out_f32") else dt, k_step=32, K=9 * Cin, extra_abs=None, wv=w, bias=bias)
        R.x = _q(dt, rng_normal(seed + i, B, Cin, s, s))
        R.pre = F.conv2d(R.x, w, padding=1) + _c(bias)
        R.mag = F.conv2d(R.x.abs(), w.abs(), padding=1) + _c(bias).abs()
        R.pre_bound = (R.K / 32.0 + 32 + 2) * U24 * R.mag
        R.ref = R.pre.clamp(min=0) if f["act"] == 1 else torch.sigmoid(R.pre)
        levels.append(R)
    return levels


def _pyramid_case(cid, route, f):
    """conv_forward_seg: one launch over every level, each level compared on its own; three of the five pixel tiles are nearly empty."""
    ops = _ops()
    dt, Cout = f["dtype"], f["Cout"]
    levels = _pyramid_ref(cid, f)
    acts = [_act(R.x, dt) for R in levels]
    outs = ops.alloc_seg(acts, Cout, levels[0].odt)
    for o in outs:
        o.t.fill_(float("nan"))
    outs, names = _launch(lambda: ops.conv_forward_seg(acts, w_krsc(levels[0].wv.float(), dt), Cout, 3, 3, 1, bias=levels[0].bias.cuda(), act=f["act"],
                                                       out_f32=f.get("out_f32", False), outs=outs))
    assert len(names) == 1, names
    _assert_route(cid, names, _needs_ext(f), route)
    for s, R, o in zip(f["levels"], levels, outs):
        _check_out("%s level %dx%d" % (cid, s, s), route, f, R, _nchw(o))
        _pad_lanes_zero(cid, o)


C, K4, K1, PY = _conv_case, _class_case, _onetap_case, _pyramid_case
S = dict(B=3, H=29, W=27)               # P = 2349: 19 pixel tiles, tail 45
S2 = dict(B=3, H=15, W=14)              # its stride-2 image, P = 630: 5 tiles, tail 118
STEM = dict(B=2, H=58, W=54, Cin=3, Cout=64, k=7, stem=True)        # output 29x27: P = 1566, 13 tiles, tail 30
# (id, route, runner, features).  Routes: mpn_conv_kernel_name for exactly these parameter blocks (tests/test_conv_small_tiles_cpu.py pins
# them without a GPU); each case asserts its own from the launch.
CASES = [
    # ---- bf16 forward
    ("bf16 1x1 256->64 stats", _inst(BF, 64), C, dict(dtype=BF, Cin=256, Cout=64, k=1, stats=True, **S)),
    ("bf16 1x1 256->64 stats finalize", _inst(BF, 64), C, dict(dtype=BF, Cin=256, Cout=64, k=1, stats=True, fin=True, **S)),
    ("bf16 1x1 s2 256->512 stats", _inst(BF, 64), C, dict(dtype=BF, Cin=256, Cout=512, k=1, stride=2, stats=True, **S)),
    ("bf16 3x3 s2 128->128 stats", _inst(BF, 64), C, dict(dtype=BF, Cin=128, Cout=128, k=3, stride=2, stats=True, **S)),
    ("bf16 1x1 s2 256->500 bias", _inst(BF, 64, general=True), C,                                   # last channel tile: 52 rows live
     dict(dtype=BF, Cin=256, Cout=500, k=1, stride=2, bias=True, **S)),
    ("bf16 3x3 s2 256->256 bias", _inst(BF, 64, general=True), C, dict(dtype=BF, Cin=256, Cout=256, k=3, stride=2, bias=True, **S)),      # P6
    ("bf16 3x3 256->17 bias f32out", _inst(BF, 32, out_f32=True, general=True), C,                  # non-s3 3x3, 17 of 32 rows live
     dict(dtype=BF, Cin=256, Cout=17, k=3, bias=True, out_f32=True, **S)),
    ("bf16 1x1 256->24 bias f32out", _inst(BF, 32, out_f32=True, general=True), C, dict(dtype=BF, Cin=256, Cout=24, k=1, bias=True, out_f32=True, **S)),
    ("bf16 s3 3x3 64->64 stats", _inst(BF, 64, s3=True), C, dict(dtype=BF, Cin=64, Cout=64, k=3, stats=True, **S)),
    ("bf16 s3 3x3 64->64 bias relu", _inst(BF, 64, s3=True, general=True), C, dict(dtype=BF, Cin=64, Cout=64, k=3, bias=True, act=1, **S)),
    ("bf16 s3 3x3 256->256 B3 13x11 bias relu", _inst(BF, 64, s3=True, general=True), C,             # 64 rows by workgroup count; 4 tiles
     dict(dtype=BF, B=3, H=13, W=11, Cin=256, Cout=256, k=3, bias=True, act=1)),
    ("bf16 s3 pyramid 256->256 B3 bias relu", _inst(BF, 64, s3=True, general=True), PY,              # 2 + 1 + 1 + 1 tiles
     dict(dtype=BF, B=3, Cin=256, Cout=256, levels=(8, 4, 2, 1), act=1)),
    ("bf16 s3 3x3 256->36 bias f32out", _inst(BF, 64, s3=True, out_f32=True, general=True), C,
     dict(dtype=BF, Cin=256, Cout=36, k=3, bias=True, out_f32=True, **S)),
    ("bf16 s3 3x3 256->36 bias sigmoid f32out", _inst(BF, 64, s3=True, out_f32=True, general=True), C,
     dict(dtype=BF, Cin=256, Cout=36, k=3, bias=True, act=2, out_f32=True, **S)),
    ("bf16 s3 pyramid 256->36 B3 bias sigmoid f32out", _inst(BF, 64, s3=True, out_f32=True, general=True), PY,
     dict(dtype=BF, B=3, Cin=256, Cout=36, levels=(8, 4, 2, 1), act=2, out_f32=True)),
    # ---- the stem: 7x1 / stride 2 row convolution over the packed image (x_geom)
    ("bf16 stem B2 58x54 stats", _inst(BF, 64), C, dict(dtype=BF, stats=True, **STEM)),
    ("f16 stem B2 58x54 scale bias relu", _inst(H16, 64, general=True), C, dict(dtype=H16, scale=True, bias=True, act=1, **STEM)),
    ("f32 stem B2 58x54 stats", _inst(F32, 64), C, dict(dtype=F32, stats=True, **STEM)),
    # ---- f32 forward
    ("f32 3x3 64->64 stats", _inst(F32, 64), C, dict(dtype=F32, Cin=64, Cout=64, k=3, stats=True, **S)),
    ("f32 1x1 48->64 stats", _inst(F32, 64), C, dict(dtype=F32, Cin=48, Cout=64, k=1, stats=True, **S)),       # Cin a multiple of 16 only
    ("f32 3x3 s2 128->128 bias", _inst(F32, 64, general=True), C, dict(dtype=F32, Cin=128, Cout=128, k=3, stride=2, bias=True, **S)),
    ("f32 3x3 256->17 bias", _inst(F32, 32, general=True), C, dict(dtype=F32, Cin=256, Cout=17, k=3, bias=True, **S)),
    # ---- f16 forward (folded-BN inference)
    ("f16 1x1 256->64 scale bias relu", _inst(H16, 64, general=True), C, dict(dtype=H16, Cin=256, Cout=64, k=1, scale=True, bias=True, act=1, **S)),
    ("f16 1x1 s2 256->512 scale bias", _inst(H16, 64, general=True), C, dict(dtype=H16, Cin=256, Cout=512, k=1, stride=2, scale=True, bias=True, **S)),
    ("f16 1x1 64->256 scale bias res act3", _inst(H16, 64, general=True), C,
     dict(dtype=H16, Cin=64, Cout=256, k=1, scale=True, bias=True, res=(29, 27), act=3, **S)),
    ("f16 1x1 256->128 bias res2 from 15x14", _inst(H16, 64, general=True), C, dict(dtype=H16, Cin=256, Cout=128, k=1, bias=True, res=(15, 14), **S)),
    ("f16 s3 3x3 64->64 scale bias relu", _inst(H16, 64, s3=True, general=True), C, dict(dtype=H16, Cin=64, Cout=64, k=3, scale=True, bias=True, act=1, **S)),
    ("f16 3x3 256->17 bias f32out", _inst(H16, 32, out_f32=True, general=True), C, dict(dtype=H16, Cin=256, Cout=17, k=3, bias=True, out_f32=True, **S)),
    ("f16 s3 3x3 256->36 bias sigmoid f32out", _inst(H16, 64, s3=True, out_f32=True, general=True), C,
     dict(dtype=H16, Cin=256, Cout=36, k=3, bias=True, act=2, out_f32=True, **S)),
    # ---- the loaded dgrad epilogue (weights through ops.weight_transpose)
    ("bf16 dgrad 1x1 64->256 res mask bnb mask", _inst(BF, 64, general=True), C,
     dict(dtype=BF, Cin=64, Cout=256, k=1, mode=1, res=(29, 27), res_mask=True, bnb="mask", **S)),
    ("bf16 dgrad 1x1 64->256 res mask bnb mask finalize train", _inst(BF, 64, general=True), C,
     dict(dtype=BF, Cin=64, Cout=256, k=1, mode=1, res=(29, 27), res_mask=True, bnb="mask", bnb_fin="train", **S)),
    ("bf16 dgrad 1x1 64->256 res mask bnb mask finalize frozen", _inst(BF, 64, general=True), C,
     dict(dtype=BF, Cin=64, Cout=256, k=1, mode=1, res=(29, 27), res_mask=True, bnb="mask", bnb_fin="frozen", **S)),
    ("bf16 dgrad 1x1 64->256 B24 res mask bnb mask", _inst(BF, 128, general=True), C,             # 147 tiles (tail 104): no in-launch finalize
     dict(dtype=BF, B=24, H=29, W=27, Cin=64, Cout=256, k=1, mode=1, res=(29, 27), res_mask=True, bnb="mask", bnb_fin="train")),
    ("bf16 dgrad 1x1 256->64 bnb recompute", _inst(BF, 64, general=True), C, dict(dtype=BF, Cin=256, Cout=64, k=1, mode=1, bnb="re", **S)),
    ("bf16 dgrad s3 3x3 64->64 bnb recompute finalize train", _inst(BF, 64, s3=True, general=True), C,
     dict(dtype=BF, Cin=64, Cout=64, k=3, mode=1, bnb="re", bnb_fin="train", **S)),
    ("bf16 dgrad 1x1 512->256 B3 15x14 bnb norelu", _inst(BF, 64, general=True), C, dict(dtype=BF, Cin=512, Cout=256, k=1, mode=1, bnb="norelu", **S2)),
    ("bf16 dgrad 1x1 64->256 acc bnb mask", _inst(BF, 64, general=True), C, dict(dtype=BF, Cin=64, Cout=256, k=1, mode=1, acc=True, bnb="mask", **S)),
    ("bf16 dgrad 1x1 64->256 acc bnb z", _inst(BF, 64, ext=True), C, dict(dtype=BF, Cin=64, Cout=256, k=1, mode=1, acc=True, bnb="z", **S)),
    ("f32 dgrad 1x1 64->256 acc bnb z", _inst(F32, 64, ext=True), C, dict(dtype=F32, Cin=64, Cout=256, k=1, mode=1, acc=True, bnb="z", **S)),
    ("f32 dgrad 1x1 256->64 bnb recompute finalize train", _inst(F32, 64, general=True), C,
     dict(dtype=F32, Cin=256, Cout=64, k=1, mode=1, bnb="re", bnb_fin="train", **S)),
    # ---- strided input gradients: the plain gather, the one-tap class, the four classes
    ("bf16 dgrad 1x1 s2 gather 512->256 fresh", _inst(BF, 64), C, dict(dtype=BF, Cin=512, Cout=256, k=1, mode=1, stride=2, out_hw=(29, 27), **S2)),
    ("bf16 dgrad 3x3 s2 gather 128->128 f32out", _inst(BF, 64, out_f32=True), C,                   # out_f32 keeps it off the class path
     dict(dtype=BF, Cin=128, Cout=128, k=3, mode=1, stride=2, out_hw=(29, 27), out_f32=True, **S2)),
    ("bf16 dgrad 1x1 s2 one-tap class 512->256 existing dx", _inst(BF, 64, ext=True), K1, dict(dtype=BF, Cin=512, Cout=256, k=1, acc=True, ystep=True, **S)),
    ("bf16 dgrad s2 classes 128->128 bnb recompute fresh", _inst(BF, 64, ext=True), K4, dict(dtype=BF, Cin=128, Cout=128, bnb="re", ystep=True, **S)),
    ("bf16 dgrad s2 classes 128->128 acc bnb mask", _inst(BF, 64, ext=True), K4, dict(dtype=BF, Cin=128, Cout=128, acc=True, bnb="mask", ystep=True, **S)),
    ("f32 dgrad s2 classes 128->128", _inst(F32, 64, ext=True), K4, dict(dtype=F32, Cin=128, Cout=128, ystep=True, **S)),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0].replace(" ", "_") for c in CASES])
def test_conv_small_tile_route_parity(case):
    cid, route, runner, f = case
    runner(cid, route, f)


# Every conv_igemm instantiation with a 64- or 32-row tile in the round-6 traces (profiles/r06_kernel_trace_stats_serial.txt,
# r06_cfg4_kernel_trace_serial.txt, r06_cfg2_kernel_trace_serial.txt, r06_cfg5_kernel_trace.txt — mangled names there).  Template
# arguments <T, TC, TP, OUTF32, GENERAL, EXT> (the trailing profiling flag dropped).
REQUIRED_ROUTES = [
    # bf16: 7
    "conv_igemm_kernel<bf16, 64, 128, false, false, false>",
    "conv_igemm_kernel<bf16, 64, 128, false, true, false>",
    "conv_igemm_kernel<bf16, 64, 128, false, true, true>",
    "conv_igemm_kernel<bf16, 32, 128, true, true, false>",
    "conv_igemm_s3_kernel<bf16, 64, 128, false, false, false>",
    "conv_igemm_s3_kernel<bf16, 64, 128, false, true, false>",
    "conv_igemm_s3_kernel<bf16, 64, 128, true, true, false>",
    # float: 4
    "conv_igemm_kernel<float, 64, 128, false, false, false>",
    "conv_igemm_kernel<float, 64, 128, false, true, false>",
    "conv_igemm_kernel<float, 64, 128, false, true, true>",
    "conv_igemm_kernel<float, 32, 128, false, true, false>",
    # _Float16: 4
    "conv_igemm_kernel<_Float16, 64, 128, false, true, false>",
    "conv_igemm_kernel<_Float16, 32, 128, true, true, false>",
    "conv_igemm_s3_kernel<_Float16, 64, 128, false, true, false>",
    "conv_igemm_s3_kernel<_Float16, 64, 128, true, true, false>",
]


def test_required_small_routes_are_covered():
    assert len(REQUIRED_ROUTES) == len(set(REQUIRED_ROUTES)) == 15
    asserted = set(c[1] for c in CASES)
    missing = [r for r in REQUIRED_ROUTES if r not in asserted]
    for r in REQUIRED_ROUTES:
        report("route coverage %-64s %s" % (r, "reached" if r in asserted else "MISSING"))
    assert not missing, "small-tile instantiations of the round-6 traces without a parity case: %s" % missing
