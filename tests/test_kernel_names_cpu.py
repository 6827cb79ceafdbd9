"""Kernel names come from the launchers' own routing decision (mpn_conv_kernel_name, mpn_conv_wgrad_kernel_name): host only, no GPU.

The table below holds parameter blocks as the ops.py wrappers fill them, built as plain ctypes structs from the shapes of the two
float64 parity suites (tests/test_conv_tiles_gpu.py and tests/test_wgrad_parity_gpu.py: their CASES and the routes those name), plus a
32- and a 64-row tile, the non-DMA weight-gradient fallback and a plain parity-class launch.  For every block the library must return
exactly the instantiation the case names; the table must reach each of the 22 + 14 kernel routes the suites pin from the round-6 traces.

tests/golden/g19_kernel_names.json holds, for the same table, the five-argument names ops.py derived with its own formulas before the
library named its kernels.  The KERNEL_EVENTS spelling (the library's name without its last argument) must equal it — bench.py keys
per-kernel HBM traffic on that spelling — except for the entries of OLD_NAME_WRONG."""
import ctypes
import json
import os

import pytest
import torch

import test_conv_tiles_gpu as ct
import test_wgrad_parity_gpu as wt
from helpers import ROOT, round_up

BF, H16, F32 = torch.bfloat16, torch.float16, torch.float32
DT = {F32: 0, BF: 1, H16: 2}
PTR = 0x1000            # stands for a device tensor: routing only asks whether a pointer is set


def _hw(H, W, k, stride, pad):
    return (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1


# ------------------------------------------------------------------------------------------- forward / input-gradient blocks
def conv_block(dtype, B, H, W, Cin, Cout, k, mode=0, out_f32=False, bias=False, scale=False, act=0, res=None, acc=False, stats=False,
               fin=False, bnb=None, stride=1, out_hw=None, stem=False, res_mask=False, bnb_fin=None, **_):
    """ops.conv_forward as tests/test_conv_tiles_gpu.py::_conv_case (stride 1, 'same') and tests/test_conv_small_tiles_gpu.py::_conv_case
    (any stride, the strided mode 1 gather into out_hw, the stem's packed row convolution through x_geom, the loaded dgrad epilogue) call it."""
    from multiposenet.pytorch_amd import ops
    from multiposenet.pytorch_amd._lib import ConvParams
    p = ConvParams()
    pad = (k - 1) // 2
    if stem:        # 7x7 / stride 2 / pad 3 over the NHWC4 zero-bordered image: R = 7, S = 1 over 32 'channels' (engine.stem)
        Ho, Wo = _hw(H, W, 7, 2, 3)
        H, W, xs, Cin, Cout, R, S, stride, pad, cin = H + 6, W + 8, 4, 32, 64, 7, 1, 2, 0, 32
    else:
        Ho, Wo = _hw(H, W, k, stride, pad) if mode == 0 else (out_hw or (H, W))
        xs, R, S = round_up(Cin, 32), k, k
        cin = round_up(Cin, 32 if (mode == 1 or dtype != F32) else 16)
    ys = round_up(Cout, 32)
    p.x, p.w, p.y = PTR, PTR, PTR
    p.B, p.H, p.W, p.Ho, p.Wo = B, H, W, Ho, Wo
    p.Cin = cin
    p.Cout, p.Cout_store = Cout, ys
    p.x_sW, p.x_sH, p.x_sB = xs, W * xs, H * W * xs
    p.y_sP, p.y_sB = ys, Ho * Wo * ys
    p.R, p.S, p.stride, p.pad = R, S, stride, pad
    p.mode, p.act, p.accumulate, p.dtype = mode, act, 1 if acc else 0, DT[dtype]
    p.out_f32 = 1 if (out_f32 and dtype != F32) else 0
    p.bias, p.scale = (PTR if bias else None), (PTR if scale else None)
    if res:
        p.res, p.res_mode, p.res_H, p.res_W = PTR, (1 if tuple(res) == (Ho, Wo) else 2), res[0], res[1]
        p.res_sP, p.res_sB = ys, res[0] * res[1] * ys
        if res_mask:
            p.res_mask = PTR
    tiles = (B * Ho * Wo + 127) // 128
    if stats:
        p.stats = PTR
    if fin and ops.fin_in_launch(tiles, Cout):
        p.fin_counters, p.fin_gamma, p.fin_beta, p.fin_out, p.fin_count = PTR, PTR, PTR, PTR, float(B * Ho * Wo)
    if bnb:
        _bnb_fields(p, bnb)
        if bnb_fin and ops.fin_in_launch(tiles, Cout):
            p.fin_counters, p.fin_gamma, p.fin_dgamma, p.fin_dbeta, p.fin_count = PTR, PTR, PTR, PTR, float(B * Ho * Wo)
            p.fin_train = 1 if bnb_fin == "train" else 0
            p.fin_out = PTR if bnb_fin == "train" else None
    return p


def _bnb_fields(p, bnb):
    """BatchNorm-backward statistics in the epilogue: the ReLU mask from z ('z'), from its sign bits ('mask'), recomputed from
    y * scale + shift ('re'), or none ('norelu')."""
    p.bnb_partial, p.bnb_y, p.bnb_mean, p.bnb_invstd, p.bnb_scale, p.bnb_shift = PTR, PTR, PTR, PTR, PTR, PTR
    p.bnb_relu = 0 if bnb == "norelu" else 1
    if bnb == "mask":
        p.bnb_mask = PTR
    elif bnb == "z":
        p.bnb_z = PTR


def class_block(dtype, B, H, W, Cin, Cout, a=1, c=1, acc=False, k=3, bnb=None, **_):
    """Parity class (a, c) of the 3x3 / stride 2 / pad 1 input gradient of _ystep_case (ops._conv_dgrad_s2_classes): dx [B, H, W, Cout] from
    dy with Cin channels.  k = 1: the one-tap class (0, 0) of a 1x1 / stride 2 input gradient into an existing dx."""
    from multiposenet.pytorch_amd._lib import ConvParams
    p = ConvParams()
    if k == 1:
        a = c = 0
    Hy, Wy = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xs, ys = round_up(Cin, 32), round_up(Cout, 32)
    p.x, p.w, p.y = PTR, PTR, PTR
    p.B, p.H, p.W, p.Ho, p.Wo = B, Hy, Wy, (H - a + 1) // 2, (W - c + 1) // 2
    p.Cin, p.Cout, p.Cout_store = xs, Cout, ys
    p.x_sW, p.x_sH, p.x_sB = xs, Wy * xs, Hy * Wy * xs
    p.y_sP, p.y_sB, p.y_H, p.y_W = ys, H * W * ys, H, W
    p.R, p.S, p.stride, p.pad, p.dtype, p.accumulate = 1 + a, 1 + c, 1, 0, DT[dtype], 1 if acc else 0
    p.y_step, p.y_oh, p.y_ow = 2, a, c
    if k == 1:
        p.w_taps, p.wtap0, p.wtap_dr, p.wtap_ds = 1, 0, 0, 0
    else:
        p.w_taps, p.wtap0, p.wtap_dr, p.wtap_ds = 9, (a + 1) * 3 + (c + 1), -6, -2
    if bnb:
        _bnb_fields(p, bnb)
    return p


def kseg_block(dtype, B, H, W, Cout, **_):
    """ops.conv_forward_cat over four 128-channel members, bias + ReLU (_kseg_case)."""
    from multiposenet.pytorch_amd._lib import ConvParams
    p = ConvParams()
    ys = round_up(Cout, 32)
    p.kseg_n, p.kseg_c = 4, 128
    for i, sh in enumerate((3, 2, 1, 0)):
        p.kseg_shift[i], p.kseg_x[i] = sh, PTR
    p.w, p.y, p.bias = PTR, PTR, PTR
    p.B, p.H, p.W, p.Ho, p.Wo = B, H, W, H, W
    p.Cin, p.Cout, p.Cout_store = 512, Cout, ys
    p.x_sW, p.x_sH, p.x_sB = 512, W * 512, H * W * 512
    p.y_sP, p.y_sB = ys, H * W * ys
    p.R, p.S, p.stride, p.pad, p.act, p.dtype = 3, 3, 1, 1, 1, DT[dtype]
    return p


def pyramid_block(dtype, B, Cin, Cout, levels, act=1, out_f32=False, **_):
    """ops.conv_forward_seg: 3x3 tower over the pyramid levels, bias + ReLU (_pyramid_case) or bias + sigmoid into f32 (the class head)."""
    from multiposenet.pytorch_amd._lib import ConvParams
    p = ConvParams()
    p.w, p.bias = PTR, PTR
    p.B, p.Cin, p.Cout, p.Cout_store = B, round_up(Cin, 32), Cout, round_up(Cout, 32)
    p.x_sW, p.y_sP = round_up(Cin, 32), round_up(Cout, 32)
    p.R, p.S, p.stride, p.pad, p.act, p.dtype = 3, 3, 1, 1, act, DT[dtype]
    p.out_f32 = 1 if (out_f32 and dtype != F32) else 0
    p.nseg = len(levels)
    tile0 = 0
    for l, s in enumerate(levels):
        p.seg_x[l], p.seg_y[l], p.seg_H[l], p.seg_W[l], p.seg_tile0[l] = PTR, PTR, s, s, tile0
        tile0 += (B * s * s + 127) // 128
    p.seg_tile0[len(levels)] = tile0
    return p


def conv_table():
    """(id, block, expected six-argument name)."""
    build = {ct._conv_case: conv_block, ct._kseg_case: kseg_block, ct._pyramid_case: pyramid_block}
    rows = []
    for cid, route, runner, f in ct.CASES:
        if runner is ct._ystep_case:
            # the case launches its four classes into a fresh output; the training step's class launches mostly accumulate into an
            # existing dx — that block reaches the same instantiation (the plain one is the last entry of this table)
            rows.append((cid + " class(1,1) accumulate", class_block(acc=True, **f), route))
        else:
            rows.append((cid, build[runner](**f), route))
    rows += [
        ("bf16 1x1 256->24 B2 30x30 32-row tile", conv_block(BF, 2, 30, 30, 256, 24, 1), ct._inst(BF, 32, general=True)),
        ("bf16 s3 3x3 64->64 B2 30x30 64-row tile", conv_block(BF, 2, 30, 30, 64, 64, 3), ct._inst(BF, 64, s3=True)),
        ("f32 3x3 64->128 B1 20x20 64-row tile by workgroup count", conv_block(F32, 1, 20, 20, 64, 128, 3, bias=True), ct._inst(F32, 64, general=True)),
        ("bf16 dgrad s2 class(1,1) 128->64 B4 121x119 plain", class_block(BF, 4, 121, 119, 128, 64), ct._inst(BF, 64, ext=True)),
    ]
    return rows


# An extended-epilogue launch is instantiated <..., GENERAL=true, EXT=true> whatever else it asks for (launch_conv in conv_igemm.hip), but
# ops.py used to derive GENERAL from its argument list alone and reported false for these: the old name was wrong, the new one is the
# kernel that runs.  Their new five-argument name must be the old one with the flag corrected.
OLD_NAME_WRONG = {"bf16 dgrad s2 class(1,1) 128->64 B4 121x119 plain"}


# ------------------------------------------------------------------------------------------------------ weight-gradient blocks
def wgrad_block(dtype, B, H, W, Cin, Cout, k, stride=1, pad=None, **_):
    """ops.conv_wgrad as tests/test_wgrad_parity_gpu.py::_conv_case calls it."""
    from multiposenet.pytorch_amd._lib import WgradParams
    p = WgradParams()
    pad = (k - 1) // 2 if pad is None else pad
    xs = round_up(Cin, 32)
    p.x, p.dy, p.dw = PTR, PTR, PTR
    p.x_sW, p.x_sH, p.x_sB, p.dy_sP = xs, W * xs, H * W * xs, round_up(Cout, 32)
    p.B, p.H, p.W, p.Cin, p.Cout = B, H, W, Cin, Cout
    p.Ho, p.Wo = _hw(H, W, k, stride, pad)
    p.R, p.S, p.stride, p.pad, p.dtype = k, k, stride, pad, DT[dtype]
    return p


def stem_block(dtype, B, H, W, **_):
    """The packed 7x7x3 / stride 2 stem (_stem_case): R = 7, S = 1 over 32 'channels' of the NHWC4 image."""
    from multiposenet.pytorch_amd._lib import WgradParams
    p = WgradParams()
    Hp, Wp = H + 6, W + 8
    p.x, p.dy, p.dw = PTR, PTR, PTR
    p.x_sW, p.x_sH, p.x_sB, p.dy_sP = 4, Wp * 4, Hp * Wp * 4, 64
    p.B, p.H, p.W, p.Cin, p.Cout = B, Hp, Wp, 32, 64
    p.Ho, p.Wo = _hw(H, W, 7, 2, 3)
    p.R, p.S, p.stride, p.pad, p.dtype = 7, 1, 2, 0, DT[dtype]
    return p


def wseg_block(dtype, B, Cin, Cout, k, levels, **_):
    """ops.conv_wgrad_seg (_seg_case)."""
    from multiposenet.pytorch_amd._lib import WgradParams
    p = WgradParams()
    p.dw = PTR
    p.x_sW, p.dy_sP = round_up(Cin, 32), round_up(Cout, 32)
    p.B, p.Cin, p.Cout = B, Cin, Cout
    p.R, p.S, p.stride, p.pad, p.dtype = k, k, 1, (k - 1) // 2, DT[dtype]
    p.nseg = len(levels)
    for l, s in enumerate(levels):
        p.seg_x[l], p.seg_dy[l], p.seg_H[l], p.seg_W[l] = PTR, PTR, s, s
    return p


def wcat_block(dtype, B, H, W, Cout, shifts, **_):
    """ops.conv_wgrad_cat (_cat_case)."""
    from multiposenet.pytorch_amd._lib import WgradParams
    p = WgradParams()
    Cin = 128 * len(shifts)
    p.kseg_n, p.kseg_c = len(shifts), 128
    for i, sh in enumerate(shifts):
        p.kseg_shift[i], p.kseg_x[i] = sh, PTR
    p.dy, p.dw, p.dy_sP = PTR, PTR, round_up(Cout, 32)
    p.x_sW, p.x_sH, p.x_sB = Cin, W * Cin, H * W * Cin
    p.B, p.H, p.W, p.Cin, p.Ho, p.Wo, p.Cout = B, H, W, Cin, H, W, Cout
    p.R, p.S, p.stride, p.pad, p.dtype = 3, 3, 1, 1, DT[dtype]
    return p


def wgrad_table():
    """(id, block, expected name)."""
    build = {wt._conv_case: wgrad_block, wt._stem_case: stem_block, wt._seg_case: wseg_block, wt._cat_case: wcat_block}
    rows = [(cid, build[runner](**f), route) for cid, route, runner, f in wt.CASES if route != "per-level fallback"]
    rows += [
        # operands past the 2^31 - 1 bytes a buffer descriptor addresses: the register-staged generic kernel
        ("bf16 3x3 64->128 B64 512x512 x over 2 GB", wgrad_block(BF, 64, 512, 512, 64, 128, 3), "conv_wgrad_kernel<bf16, 64, 128>"),
        ("f32 1x1 32->16 B64 512x512 x over 2 GB", wgrad_block(F32, 64, 512, 512, 32, 16, 1), "conv_wgrad_kernel<float, 32, 32>"),
        ("f16 3x3 128->40 B40 512x512 x over 2 GB", wgrad_block(H16, 40, 512, 512, 128, 40, 3), "conv_wgrad_kernel<_Float16, 128, 64>"),
    ]
    return rows


# ---------------------------------------------------------------------------------------------------------------------- tests
def _name(query, p):
    from multiposenet.pytorch_amd import _lib
    buf = ctypes.create_string_buffer(128)
    n = getattr(_lib.lib(), query)(ctypes.byref(p), buf, len(buf))
    assert n > 0, "%s returned %d" % (query, n)
    name = buf.value.decode()
    assert len(name) == n
    return name


def _five(name):
    """The KERNEL_EVENTS class of a forward launch: the library's name without its last (EXT) argument (ops._launch_conv)."""
    return name.rsplit(", ", 1)[0] + ">"


def _golden():
    with open(os.path.join(ROOT, "tests", "golden", "g19_kernel_names.json")) as f:
        return json.load(f)


CONV, WGRAD = conv_table(), wgrad_table()


@pytest.mark.parametrize("row", CONV, ids=[r[0].replace(" ", "_") for r in CONV])
def test_conv_kernel_name(row):
    cid, p, route = row
    assert _name("mpn_conv_kernel_name", p) == route, cid


@pytest.mark.parametrize("row", WGRAD, ids=[r[0].replace(" ", "_") for r in WGRAD])
def test_wgrad_kernel_name(row):
    cid, p, route = row
    assert _name("mpn_conv_wgrad_kernel_name", p) == route, cid
    # the id the production path reads for the fused bias gradient is the same decision
    from multiposenet.pytorch_amd import _lib
    kid = _lib.lib().mpn_conv_wgrad_kernel_id(ctypes.byref(p))
    tm, tn = route[route.index("<") + 1: -1].split(", ")[-2:]
    assert (kid >> 16, (kid >> 4) & 0xfff, bool(kid & 2), bool(kid & 1)) == (int(tm), int(tn), "_lin" in route, route.startswith("conv_wgrad_dma")), (cid, hex(kid))


def test_tables_reach_every_required_route():
    conv = set(r[2] for r in CONV if r[0] not in OLD_NAME_WRONG)
    wgrad = set(r[2] for r in WGRAD)
    kernels = [r for r in wt.REQUIRED_ROUTES if not r.startswith("reduce_partials")]
    assert len(ct.REQUIRED_ROUTES) == 22 and len(kernels) == 14
    assert not [r for r in ct.REQUIRED_ROUTES if r not in conv], [r for r in ct.REQUIRED_ROUTES if r not in conv]
    assert not [r for r in kernels if r not in wgrad], [r for r in kernels if r not in wgrad]
    tiles = set(r[2].split(", ")[1] for r in CONV)
    assert {"32", "64", "128", "256"} <= tiles, tiles
    assert any(r[2].startswith("conv_wgrad_kernel<") for r in WGRAD)
    assert [r[2] for r in CONV if r[0].endswith("plain")][0].endswith("true, true>")


def test_event_names_equal_the_names_ops_used_to_derive():
    gold = _golden()
    assert sorted(gold) == sorted(r[0] for r in CONV + WGRAD), "fixture and table differ"
    required = set(ct.REQUIRED_ROUTES) | set(wt.REQUIRED_ROUTES)
    for cid, p, route in CONV:
        new = _five(_name("mpn_conv_kernel_name", p))
        if cid in OLD_NAME_WRONG:
            assert route.endswith("true, true>") and route not in required, cid
            assert gold[cid].endswith(", false>") and new == gold[cid][: -len("false>")] + "true>", (cid, gold[cid], new)
        else:
            assert new == gold[cid], (cid, gold[cid], new)
    for cid, p, route in WGRAD:
        assert _name("mpn_conv_wgrad_kernel_name", p) == gold[cid], cid
    assert 2 * len(OLD_NAME_WRONG) < len(CONV) and OLD_NAME_WRONG <= set(r[0] for r in CONV)

