"""GPU parity of the inference post-processing arithmetic against independent float64 references: `resize_kernel` and the refinement
half of `peaks_refine_kernel` (csrc/peaks.hip), `box_decode_clip_kernel` / `clip_boxes_kernel` (csrc/nms.hip) and
`bn_finalize_eval_kernel` (csrc/bn.hip).  The references, the derivation of every bound and the peak rules are in
tests/postproc_ref.py; tests/test_postproc_parity_cpu.py holds the oracle to the same references and shows that the bounds reject
modelled faults.  Every comparison writes one line to the parity report (worst error over bound and where).  The bit-equality tests
against oracle/joint_oracle.py stay in tests/test_peaks_gpu.py."""
import os
import re

import numpy as np
import pytest
import torch

import postproc_ref as pr
from helpers import ROOT, report

pytestmark = pytest.mark.gpu
NAN = float("nan")


def _ops():
    from multiposenet.pytorch_amd import ops
    return ops


def _tester():
    from multiposenet.pytorch_amd.evaluate import tester
    return tester


def _ju():
    from multiposenet.pytorch_amd.network import joint_utils
    return joint_utils


def _resize_prefilled(img, out_hw, cubic, inv_scale):
    """tester.resize's launch into an output prefilled with NaN (tester.resize allocates its own)."""
    from multiposenet.pytorch_amd._lib import call
    ops = _ops()
    H, W, C = img.shape
    out = torch.full((int(out_hw[0]), int(out_hw[1]), C), NAN, dtype=torch.float32, device=img.device)
    sy, sx = (0.0, 0.0) if inv_scale is None else (float(inv_scale[0]), float(inv_scale[1]))
    call("mpn_resize", ops.ptr(img), img.stride(0), img.stride(1), img.stride(2), H, W, C, ops.ptr(out), out.shape[0], out.shape[1],
         1 if cubic else 0, sy, sx, ops.stream_ptr())
    return out


def _check_resize(name, img_np, img_dev, out_hw, cubic, inv_scale=None):
    got = _tester().resize(img_dev, out_hw, cubic, inv_scale)
    pre = _resize_prefilled(img_dev, out_hw, cubic, inv_scale)
    assert tuple(got.shape) == (int(out_hw[0]), int(out_hw[1]), img_np.shape[2])
    assert not bool(torch.isnan(pre).any()), "%s: an element of the output was not written" % name
    assert torch.equal(got, pre), name
    pr.check_resize(name, pre.cpu().numpy(), img_np, out_hw, cubic, inv_scale, route="mpn_resize vs torch float64")
    return pre


# ------------------------------------------------------------------------------------------------ resize
@pytest.mark.parametrize("cubic", [True, False], ids=["cubic", "linear"])
@pytest.mark.parametrize("case", pr.RESIZE_CASES, ids=lambda c: "%dx%dx%d-%dx%d" % c)
def test_resize_case_table(case, cubic):
    Hs, Ws, C, Hd, Wd = case
    img = pr.resize_input(Hs, Ws, C)
    assert img.size < 25 or (img.min() < -1 and img.max() > 1)                # mixed sign: the magnitude array matters
    got = _check_resize("resize %dx%dx%d->%dx%d %s" % (case + ("cubic" if cubic else "linear",)), img, torch.from_numpy(img).cuda(), (Hd, Wd), cubic)
    if (Hs, Ws) == (Hd, Wd):
        assert np.array_equal(got.cpu().numpy(), img), "identity resize changed the image"


@pytest.mark.parametrize("cubic", [True, False], ids=["cubic", "linear"])
@pytest.mark.parametrize("f", pr.FX_FACTORS)
def test_resize_fx_fy_form(f, cubic):
    img, hw, inv = pr.fx_case(f)
    assert hw == (int(np.rint(37 * f)), int(np.rint(53 * f)))
    _check_resize("resize fx=fy=%g 37x53x3->%dx%d %s" % (f, hw[0], hw[1], "cubic" if cubic else "linear"), img, torch.from_numpy(img).cuda(), hw,
                  cubic, inv)


@pytest.mark.parametrize("cubic", [True, False], ids=["cubic", "linear"])
def test_resize_generic_strides(cubic):
    """A channel-first tensor viewed as [H, W, C], cut out of a larger one: no stride is 1 times the next extent."""
    img = pr.resize_input(19, 23, 5, seed=7)
    big = torch.full((7, 21, 26), NAN, device="cuda")
    big[1:6, 1:20, 2:25] = torch.from_numpy(img).cuda().permute(2, 0, 1)
    view = big[1:6, 1:20, 2:25].permute(1, 2, 0)
    assert tuple(view.shape) == (19, 23, 5) and view.stride() == (26, 1, 21 * 26)
    _check_resize("resize 19x23x5->45x31 %s channel-first view" % ("cubic" if cubic else "linear"), img, view, (45, 31), cubic)
    _check_resize("resize 19x23x5 fx=fy=0.6 %s channel-first view" % ("cubic" if cubic else "linear"), img, view, (11, 14), cubic, (1 / 0.6, 1 / 0.6))


# ------------------------------------------------------------------------------------------------ peak refinement
def _row_width():
    src = open(os.path.join(ROOT, "multiposenet", "pytorch_amd", "csrc", "peaks.hip")).read()
    return int(re.search(r"constexpr\s+int\s+PK_ROW_W\s*=\s*(\d+)\s*;", src).group(1))


def _views(heat_np):
    t = torch.from_numpy(heat_np).cuda()
    B, J, H, W = t.shape
    big = torch.zeros((B, J + 1, H + 2, W + 3), device="cuda")
    big[:, 1:, 1:-1, 2:-1] = t
    cl = t.contiguous(memory_format=torch.channels_last)
    if J > 1:
        assert cl.stride(1) == 1 and cl.stride(3) == J
    return {"planar": t, "channels_last": cl, "strided": big[:, 1:, 1:-1, 2:-1]}


@pytest.mark.parametrize("f", pr.PEAK_FACTORS)
@pytest.mark.parametrize("name", pr.PEAK_MAPS)
def test_peak_refinement_vs_float64(name, f):
    heat, thre, expect = pr.peak_case(name, f)
    for b in range(heat.shape[0]):                                            # the cap, from the reference alone
        share, n = pr.undecided_share(expect[b])
        assert n > 0 and share <= 0.05, (name, f, b, n, share)
    widths = [p["dw"] for e in expect for r in e for p in r]
    row_w = _row_width()
    staged, direct = sum(1 for w in widths if w <= row_w), sum(1 for w in widths if w > row_w)
    report("%-58s %-52s patches staged (dw <= %d)=%d direct=%d" % ("peaks %s f=%g" % (name, f), "peaks_refine_kernel branches", row_w, staged, direct))
    if f == 13.0:
        assert pr.dsize(5, f) == 65 and direct > 0, "no patch takes the direct branch at f = 13 (PK_ROW_W = %d)" % row_w
        assert staged > 0 and min(widths) == pr.dsize(3, f) == 39, "no border patch takes the staged branch at f = 13 (PK_ROW_W = %d)" % row_w
        if name == "noise":
            assert max(w for w in widths if w <= row_w) == pr.dsize(4, f) == 52
    else:
        assert direct == 0
    for vname, v in _views(heat).items():
        got = _ju().NMS_batch({"thre1": thre}, v, f)
        for b in range(heat.shape[0]):
            pr.check_peak_rows("peaks %s f=%g image %d" % (name, f, b), got[b], expect[b], f, route="NMS_batch %s vs torch float64" % vname)


def test_peak_refinement_exact_tie():
    """tie_map: every operation is exact in float32 at f = 4, so the device equals the float64 reference bit for bit and resolves the
    four-way tie to the first cell in row-major order."""
    heat, thre, expect = pr.peak_case("tie", 4.0)
    (p,) = [q for r in expect[0] for q in r]
    assert p["gap"] == 0.0 and p["am"] == (9, 9)
    for vname, v in _views(heat).items():
        got = _ju().NMS_batch({"thre1": thre}, v, 4.0)
        pr.check_peak_rows("peaks tie f=4", got[0], expect[0], 4.0, route="NMS_batch %s vs torch float64, exact" % vname, exact_scores=True)


# ------------------------------------------------------------------------------------------------ box decode / clip
@pytest.mark.parametrize("clip", [True, False], ids=["clip", "noclip"])
@pytest.mark.parametrize("mean_std", [None, pr.NONDEFAULT_MEAN_STD], ids=["default", "nondefault"])
def test_box_decode_vs_float64(mean_std, clip):
    ops = _ops()
    an, d = pr.decode_inputs(mean_std)                                        # B = 3, A = 257
    assert d.shape == (3, 257, 4) and len(np.unique(an, axis=0)) == 257
    boxes = ops.box_decode_clip(torch.from_numpy(an).cuda(), torch.from_numpy(d).cuda(), pr.IMG_W, pr.IMG_H, clip=clip, mean_std=mean_std)
    name = "box_decode_clip B=3 A=257 %s %s" % ("clip" if clip else "noclip", "default" if mean_std is None else "mean_std")
    report("%-58s %-52s expf measured %.4f ulp on [-10, 10], allowance %.4f ulp (twice the measured worst)" % (
        name, "stand-alone expf sweep, MI355X", pr.EXPF_ULP_MEASURED, pr.EXPF_ULP_ALLOWED))
    pr.check_decode(name, boxes.cpu().numpy(), an, d, mean_std, pr.IMG_W, pr.IMG_H, clip, route="vs float64 network/utils.py formulas")


def test_box_decode_saturating_ends_of_exp():
    ops = _ops()
    an, d = pr.decode_inputs(None, B=1, A=4)
    d[0, :, 2] = [500.0, -500.0, 500.0, -500.0]                               # dw * std = +-100 with the default std 0.2
    t = d[0, :, 2].astype(np.float64) * float(np.float32(pr.DEFAULT_MEAN_STD[6]))
    assert np.abs(np.abs(t) - 100.0).max() < 1e-5 and 0.0 < np.exp(-100.0) < pr.TINY < pr.F32_MAX < np.exp(100.0)   # subnormal / overflow
    up, down = [0, 2], [1, 3]
    for clip in (True, False):
        got = ops.box_decode_clip(torch.from_numpy(an).cuda(), torch.from_numpy(d).cuda(), pr.IMG_W, pr.IMG_H, clip=clip).cpu().numpy().astype(np.float64)
        ref, un, bd = pr.decode_ref(an, d, None, pr.IMG_W, pr.IMG_H, clip)
        x = got[0][:, [0, 2]]
        if clip:
            assert np.array_equal(x[up], np.array([[0.0, pr.IMG_W]] * 2)), x[up]
        else:
            assert np.array_equal(x[up], np.array([[-np.inf, np.inf]] * 2)), x[up]
        assert np.array_equal(un[0, down, 0], un[0, down, 2])                  # float64: width 0, the box is its centre
        pr.check_bound("box_decode_clip exp(-100) %s" % ("clip" if clip else "noclip"), got[:, down], ref[:, down], bd[:, down],
                       "vs float64, box collapsed to its centre", "bak")
        pr.check_bound("box_decode_clip exp(+100) y %s" % ("clip" if clip else "noclip"), got[:, up][:, :, [1, 3]], ref[:, up][:, :, [1, 3]],
                       bd[:, up][:, :, [1, 3]], "vs float64, the finite coordinates", "bak")


def test_clip_boxes_in_place_equals_clamp():
    ops = _ops()
    n = 1000003                                                               # not a multiple of the 256-thread block
    g = torch.Generator().manual_seed(11)
    boxes = ((torch.rand(1, n, 4, generator=g) - 0.3) * 900.0)
    boxes[0, :7] = torch.tensor([[0.0, 0.0, pr.IMG_W, pr.IMG_H], [-0.0, -1e-30, 1e30, 3e38], [float("-inf"), float("inf"), float("inf"), float("-inf")],
                                 [640.0, 480.0, 640.5, 480.5], [-5.0, 7.0, 9.0, -11.0], [1e-30, -1e-30, 639.99994, 479.99997], [639.0, 479.0, 0.0, 0.0]])
    assert not bool(torch.isnan(boxes).any())
    ref = boxes.clone()
    ref[..., 0].clamp_(min=0.0); ref[..., 1].clamp_(min=0.0); ref[..., 2].clamp_(max=pr.IMG_W); ref[..., 3].clamp_(max=pr.IMG_H)
    dev = boxes.cuda()
    out = ops.clip_boxes_(dev, pr.IMG_W, pr.IMG_H)
    assert out.data_ptr() == dev.data_ptr()
    pr.exact("clip_boxes_ n=1000003", dev.cpu(), ref, route="in place vs torch.clamp")


# ------------------------------------------------------------------------------------------------ eval BN finalize
@pytest.mark.parametrize("C", [1, 63, 64, 257, 2048])
def test_bn_finalize_eval_vs_float64(C):
    ops = _ops()
    gamma, beta, rm, rv = pr.bn_inputs(C)
    if C > 2:
        assert bool((rv < 1e-5).any()) and bool((rm.abs() > 100).any()) and gamma[0] == 0 and gamma[1] < 0
    st = ops.bn_finalize_eval(gamma.cuda(), beta.cuda(), rm.cuda(), rv.cuda())
    pr.check_bn_eval("bn_finalize_eval C=%d" % C, st, gamma, beta, rm, rv, route="vs float64")
