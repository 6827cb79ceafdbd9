"""Person masks at inference on the device (csrc/seg_infer.hip, Tester return_masks / person_masks / seg_eval): the two mask kernels
bit for bit against the numpy restatement (tests/seg_infer_ref.py) and against the composed chain of existing launches, the counting
kernel against numpy, the Tester paths against each other byte for byte, the launches made, and seg_eval against numpy."""
import sys

import numpy as np
import pytest
import torch

from helpers import report
import seg_infer_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests selected but no GPU is visible"
    from multiposenet.pytorch_amd import _lib
    _lib.lib()


def _tester_mod():
    from multiposenet.pytorch_amd.evaluate import tester
    return tester


def _same(tag, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (tag, got.shape, want.shape, got.dtype, want.dtype)
    bad = int((got.view(np.uint8) != want.view(np.uint8)).sum()) if got.dtype != np.uint8 else int((got != want).sum())
    assert bad == 0, "%s: %d of %d bytes differ" % (tag, bad, want.nbytes)


# ------------------------------------------------------------------------------------------------ mpn_seg_masks
def _heat19(qs, layout):
    """[B, 19, hq, hq] maps whose channel 18 holds qs, the other channels noise; ``nhwc``: channels-last strides."""
    B, hq = len(qs), qs[0].shape[0]
    heat = torch.rand((B, 19, hq, hq), generator=torch.Generator().manual_seed(hq)).cuda()
    for b, q in enumerate(qs):
        heat[b, 18] = torch.from_numpy(q).cuda()
    if layout == "nhwc":
        heat = heat.contiguous(memory_format=torch.channels_last)
        assert heat.stride(1) == 1 and heat.stride(3) == 19
    return heat


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("H,W,hq", ref.SINGLE_CASES)
def test_seg_masks_equal_the_restatement_and_the_device_chain(H, W, hq, layout):
    T = _tester_mod()
    q, P, M = ref.single_case(H, W, hq)
    heat = _heat19([q], layout)
    masks, planes = T.seg_masks(heat, [(H, W)], ref.THR, planes=True)
    D = max(H, W)
    chain = T.resize(heat[0, 18][:, :, None], (D, D), cubic=True)[:H, :W, 0]
    _same("plane vs device chain", planes[0].cpu().numpy(), chain.contiguous().cpu().numpy())
    _same("plane vs restatement", planes[0].cpu().numpy(), P)
    _same("mask vs restatement", masks[0].cpu().numpy(), M)
    assert masks[0].data_ptr() % 16 == 0 and masks[0].stride() == (W, 1) and masks[0].dtype == torch.uint8
    only = T.seg_masks(heat, [(H, W)], ref.THR)
    _same("mask without planes", only[0].cpu().numpy(), M)


@pytest.mark.parametrize("odd", [False, True], ids=["aligned", "odd-offsets"])
def test_seg_masks_one_launch_over_three_images_writes_every_plane_and_nothing_between(odd):
    """Three images of different sizes on one 32 x 32 map size, pitch W + 3 (aligned form: W rounded up to a multiple of 4, plus 4), the
    buffer pre-filled with 0xA5; a fourth row names a plane outside the buffer and must be skipped."""
    from multiposenet.pytorch_amd import ops
    from multiposenet.pytorch_amd._lib import call
    sizes = [(64, 65), (130, 70), (37, 53)]
    cases = [ref.single_case(H, W, 32) for H, W in sizes]
    heat = _heat19([c[0] for c in cases], "nchw")
    pitches = [W + 3 if odd else (W + 3) // 4 * 4 + 4 for _, W in sizes]
    offs, n = [], 5 if odd else 16
    for (H, W), p in zip(sizes, pitches):
        offs.append(n)
        n += H * p + (7 if odd else 0)
        n = n if odd else (n + 15) // 16 * 16
    nbytes = n + 11
    table = np.zeros((4, 7), dtype=np.int64)
    poff = 0
    for b, ((H, W), p, o) in enumerate(zip(sizes, pitches, offs)):
        table[b] = (b * heat.stride(0), max(H, W), H, W, o, p, poff)
        poff += H * W
    table[3] = (0, 40, 40, 40, nbytes - 100, 40, 0)                                      # 40 x 40 bytes do not fit: skipped
    d_table = torch.from_numpy(table).cuda()
    span = 2 * heat.stride(0) + 31 * 32 + 31 + 1
    runs = []
    for _ in range(2):
        buf = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device="cuda")
        pl = torch.full((poff,), -7.0, dtype=torch.float32, device="cuda")
        call("mpn_seg_masks", ops.ptr(heat[:, 18]), heat.stride(2), heat.stride(3), 32, 32, span, ops.ptr(d_table), 4, 70, 130, float(np.float32(ref.THR)),
             ops.ptr(buf), nbytes, ops.ptr(pl), poff, ops.stream_ptr())
        runs.append((buf.cpu().numpy(), pl.cpu().numpy()))
    want = np.full((nbytes,), 0xA5, dtype=np.uint8)
    want_pl = np.empty((poff,), dtype=np.float32)
    poff = 0
    for (H, W), p, o, (_, P, M) in zip(sizes, pitches, offs, cases):
        for y in range(H):
            want[o + y * p: o + y * p + W] = M[y]
        want_pl[poff: poff + H * W] = P.ravel()
        poff += H * W
    _same("masks and the bytes between them", runs[0][0], want)
    _same("planes", runs[0][1], want_pl)
    _same("second run", runs[1][0], runs[0][0])
    _same("second run planes", runs[1][1], runs[0][1])


# ------------------------------------------------------------------------------------------------ mpn_tta_merge_mask
def _device_chain_plane(heats, geo, H, W):
    """The unfused op sequence on one channel, without a swap: _get_outputs' loop body per pass, the mirror, the halving, .float()."""
    T = _tester_mod()
    acc = []
    for p in range(2):
        a = torch.zeros((H, W, 1), dtype=torch.float64, device="cuda")
        for heat, (h, w) in zip(heats, geo):
            sm = heat[p, 18:19].permute(1, 2, 0)
            sm = T.resize(sm, (sm.shape[0] * 4, sm.shape[1] * 4), cubic=True)
            sm = sm[0:h, 0:w, :]
            sm = T.resize(sm, (H, W), cubic=True)
            a = a + sm / len(heats)
        acc.append(a)
    return ((acc[0] + acc[1].flip(1)) / 2.).float()[:, :, 0].contiguous()


@pytest.mark.parametrize("H,W,scales", ref.MERGE_CASES)
def test_merge_mask_equals_the_device_chain_and_the_restatement(H, W, scales):
    T = _tester_mod()
    qs, geo, host_maps, P, M = ref.merge_case(H, W, scales)
    heats, maps = [], []
    for q, (h, w) in zip(qs, geo):
        heat = torch.rand((2, 19, q.shape[1], q.shape[2]), generator=torch.Generator().manual_seed(h)).cuda()
        heat[:, 18] = torch.from_numpy(q).cuda()
        heats.append(heat)
        maps.append(T.tta_seg_upsample(heat, min(h, 4 * q.shape[1]), min(w, 4 * q.shape[2])))
    assert scales == 1 or any(h < 4 * q.shape[1] or w < 4 * q.shape[2] for q, (h, w) in zip(qs, geo)), "no scale crops the x4 map"
    for u, hu in zip(maps, host_maps):
        _same("seg pair map", u.cpu().numpy(), hu)
    mask, plane = T.tta_merge_mask(maps, H, W, ref.THR, plane=True)
    chain = _device_chain_plane(heats, geo, H, W)
    _same("plane vs device chain", plane.cpu().numpy(), chain.cpu().numpy())
    _same("plane vs restatement", plane.cpu().numpy(), P)
    _same("mask vs restatement", mask.cpu().numpy(), M)
    _same("mask vs the chain's compare", mask.cpu().numpy(), ((chain > float(np.float32(ref.THR))).to(torch.uint8) * 255).cpu().numpy())
    big = torch.full((H, W + 5), 0xA5, dtype=torch.uint8, device="cuda")                 # pitch > W, mask only
    T.tta_merge_mask(maps, H, W, ref.THR, out=big[:, :W])
    got = big.cpu().numpy()
    _same("mask with pitch W + 5", np.ascontiguousarray(got[:, :W]), M)
    assert (got[:, W:] == 0xA5).all(), "bytes beyond the row were written"


# ------------------------------------------------------------------------------------------------ mpn_mask_iou
IOU_SIZES = [(5, 6), (37, 53), (64, 65), (130, 70)]


def _iou_layout(planes, mode):
    """planes: list of uint8 [H, W] -> (buffer, offsets, pitches): ``v16`` / ``v8``: starts and pitches multiples of 16 / of 8 but not
    16; ``bytes``: odd starts and pitches."""
    step = {"v16": 16, "v8": 8, "bytes": 1}[mode]
    offs, pitches, n = [], [], {"v16": 16, "v8": 8, "bytes": 3}[mode]
    for pl in planes:
        H, W = pl.shape
        p = (W + step - 1) // step * step
        if mode == "v8" and p % 16 == 0:
            p += 8
        if mode == "bytes" and p % 2 == 0:
            p += 1
        offs.append(n)
        pitches.append(p)
        n += H * p
        n = (n + step - 1) // step * step
        if mode == "v8" and n % 16 == 0:
            n += 8
        if mode == "bytes" and n % 2 == 0:
            n += 1
    host = np.full((n + 16,), 0x5A, dtype=np.uint8)                  # non-zero between planes: a read outside a row would count
    for pl, o, p in zip(planes, offs, pitches):
        for y in range(pl.shape[0]):
            host[o + y * p: o + y * p + pl.shape[1]] = pl[y]
    return torch.from_numpy(host).cuda(), offs, pitches


@pytest.mark.parametrize("mode", ["v16", "v8", "bytes"])
def test_mask_iou_counts_equal_numpy(mode):
    from multiposenet.pytorch_amd.evaluate.seg_eval import mask_iou_counts
    groups = [[s] for s in IOU_SIZES] + [[(64, 65), (130, 70), (37, 53)]]
    for sizes in groups:
        preds, gts = [ref.iou_case(H, W)[0] for H, W in sizes], [ref.iou_case(H, W)[1] for H, W in sizes]
        pbuf, poffs, ppit = _iou_layout(preds, mode)
        gbuf, goffs, gpit = _iou_layout(gts, mode)
        assert pbuf.data_ptr() % 16 == 0 and gbuf.data_ptr() % 16 == 0
        table = np.array([(H, W, po, pp, go, gp) for (H, W), po, pp, go, gp in zip(sizes, poffs, ppit, goffs, gpit)], dtype=np.int64)
        want = np.stack([ref.iou_counts_ref(p, g) for p, g in zip(preds, gts)])
        got = mask_iou_counts(pbuf, gbuf, table)
        again = mask_iou_counts(pbuf, gbuf, table, out=torch.full((len(sizes), 3), -1, dtype=torch.int64, device="cuda"))
        assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), want), (mode, sizes, got.cpu().numpy().tolist(), want.tolist())
        assert np.array_equal(again.cpu().numpy(), want), "second run"
        assert (want[:, 0] > 0).all() and (want[:, 0] < want[:, 1]).all(), "a case without intersection or without a prediction outside it"


def test_mask_iou_all_zero_all_on_and_a_skipped_row():
    from multiposenet.pytorch_amd.evaluate.seg_eval import mask_iou_counts
    H, W = 37, 53
    zero, on, mixed = np.zeros((H, W), np.uint8), np.full((H, W), 255, np.uint8), ref.iou_case(H, W)[0]
    pbuf, poffs, ppit = _iou_layout([zero, on, on, mixed], "v16")
    gbuf, goffs, gpit = _iou_layout([zero, on, zero, on], "v8")
    table = np.array([(H, W, po, pp, go, gp) for po, pp, go, gp in zip(poffs, ppit, goffs, gpit)] +
                     [(H, W, pbuf.numel() - 10, W, 0, W)], dtype=np.int64)                  # the last row leaves the buffer: skipped
    got = mask_iou_counts(pbuf, gbuf, table).cpu().numpy()
    n_on = int((mixed != 0).sum())
    assert got.tolist() == [[0, 0, 0], [H * W, H * W, H * W], [0, H * W, 0], [n_on, n_on, H * W], [0, 0, 0]], got.tolist()


# ------------------------------------------------------------------------------------------------ the Tester
@pytest.fixture(scope="module", params=[torch.float32, torch.float16], ids=["fp32", "fp16"])
def rig(request):
    """The rig of test_tester_results_of_a_person_seg_model_equal_the_plain_model_s: R50, inp_size 128, the 96 x 128 stand-in image,
    seeded weights (detector bias shifted so that people are found, seeded PRN weights), a random convfin row 18."""
    import tta_standin
    from multiposenet.pytorch_amd import synthetic as weightgen
    from multiposenet.pytorch_amd.network.posenet import poseNet
    from test_model_gpu import load_he, t
    T = _tester_mod()
    m = poseNet(50, compute_dtype=request.param, person_seg=True).cuda()
    load_he(m)
    sd = weightgen.gen_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items() if k.startswith("prn.")}, seed=3, flavour="he")
    m.load_state_dict({k: t(v) for k, v in sd.items()}, strict=False)
    m.eval()
    S = 128
    with torch.no_grad():
        _, (cls, _, _) = m([torch.randn((2, 3, S, S), generator=torch.Generator().manual_seed(2)).cuda(), "detection_subnet"])
        s_ = cls.float().flatten().clamp(1e-6, 1 - 1e-6)
        qt = torch.quantile(s_, 1.0 - 40.0 / float(cls.shape[1]))
        m.classificationModel.output.bias.data += float(-torch.log(qt / (1 - qt)))
        g = torch.Generator().manual_seed(18)
        m.convfin.weight.data[18].copy_((torch.randn(tuple(m.convfin.weight.shape[1:]), generator=g) * 0.05).to(m.convfin.weight))
        m.convfin.bias.data[18] = 0.3
    tp = T.TestParams()
    tp.ckpt, tp.inp_size = None, S
    tester = T.Tester(m, tp)
    img = tta_standin.synth_image(5, 96, 128)
    yield {"tester": tester, "img": img, "dtype": request.param, "model": m}
    del tester, m
    torch.cuda.empty_cache()


def _single_plane(tester, img):
    """The unfused single-scale plane of one image, by infer_image's own steps."""
    T = _tester_mod()
    H, W, S = img.shape[0], img.shape[1], tester.params.inp_size
    dimg = T._to_device_image(img, tester.dev)
    D = max(H, W)
    sq = torch.zeros((D, D, 3), dtype=torch.float32, device=tester.dev)
    sq[:H, :W] = dimg
    with torch.no_grad():
        heatmaps = tester.model([T.resnet_preprocess(T.resize(sq, (S, S), cubic=False))[None], 'both'])[0]
    assert heatmaps.shape[1] == 19
    return T.resize(heatmaps[0, 18][:, :, None], (D, D), cubic=True)[:H, :W, 0]


def _multi_plane(tester, img):
    """The unfused multi-scale + flip plane of one image, by infer_image_multiscale's own steps."""
    T = _tester_mod()
    dimg = T._to_device_image(img, tester.dev)
    mult = tester._get_multiplier(dimg)
    _, _, seg_o = tester._get_outputs(mult, dimg, seg=True)
    _, _, seg_f = tester._get_outputs(mult, dimg.flip(1).contiguous(), seg=True)
    return ((seg_o + seg_f.flip(1)) / 2.).float()[:, :, 0]


def _median_threshold(tester, plane):
    thr = float(torch.sort(plane.flatten())[0][plane.numel() // 2])
    tester.params.mask_thresh = thr
    return thr


def _share(mask):
    return float((mask != 0).float().mean())


def test_tester_single_scale_masks(rig):
    T = _tester_mod()
    tester, img = rig["tester"], rig["img"]
    H, W = img.shape[0], img.shape[1]
    plane = _single_plane(tester, img)
    thr = _median_threshold(tester, plane)
    plain_res = tester.infer_image(img, "a.jpg", 7)
    res, masks = tester.infer_image(img, "a.jpg", 7, return_masks=True)
    assert res == plain_res and len(masks) == 1
    m0 = masks[0]
    assert m0.dtype == torch.uint8 and tuple(m0.shape) == (H, W) and m0.is_cuda and m0.data_ptr() % 16 == 0
    assert set(torch.unique(m0).tolist()) <= {0, 255} and 0.25 <= _share(m0) <= 0.75, _share(m0)
    assert torch.equal(m0, (plane > float(np.float32(thr))).to(torch.uint8) * 255)
    small = np.ascontiguousarray(img[:80, :64])                       # a second size in the same batch: H > W
    want_small = tester.infer_image(small, "b.jpg", 8, return_masks=True)
    for pipeline in (True, False):
        bres, bmasks = tester.infer_images_batched([img, small], ["a.jpg", "b.jpg"], [7, 8], pipeline=pipeline, return_masks=True)
        assert bres == tester.infer_images_batched([img, small], ["a.jpg", "b.jpg"], [7, 8], pipeline=pipeline)
        assert bres[0] == plain_res and bres[1] == want_small[0]
        assert torch.equal(bmasks[0], m0), "pipeline=%s: %d bytes differ" % (pipeline, int((bmasks[0] != m0).sum()))
        assert torch.equal(bmasks[1], want_small[1][0]), "pipeline=%s, 80 x 64: %d bytes differ" % (pipeline, int((bmasks[1] != want_small[1][0]).sum()))
        assert bmasks[0].untyped_storage().data_ptr() == bmasks[1].untyped_storage().data_ptr() and bmasks[1].data_ptr() % 16 == 0
    assert torch.equal(tester.person_masks([img, small])[1], want_small[1][0])
    report("single-scale person mask (R50 %s): thr %.6f, ON share %.3f, batched == unfused byte for byte" % (rig["dtype"], thr, _share(m0)))


def test_tester_multi_scale_masks(rig):
    T = _tester_mod()
    tester, img = rig["tester"], rig["img"]
    H, W = img.shape[0], img.shape[1]
    dimg = T._to_device_image(img, tester.dev)
    mult = tester._get_multiplier(dimg)
    plane = _multi_plane(tester, img)
    thr = _median_threshold(tester, plane)
    plain_res = tester.infer_image_multiscale(img, "a.jpg", 7)
    res, masks = tester.infer_image_multiscale(img, "a.jpg", 7, return_masks=True)
    m0 = masks[0]
    assert res == plain_res and m0.dtype == torch.uint8 and tuple(m0.shape) == (H, W)
    assert torch.equal(m0, (plane > float(np.float32(thr))).to(torch.uint8) * 255) and 0.25 <= _share(m0) <= 0.75, _share(m0)
    # pair=False: always checked
    fres, fmasks = tester.infer_image_multiscale_fused(img, "a.jpg", 7, pair=False, return_masks=True)
    assert fres == plain_res == tester.infer_image_multiscale_fused(img, "a.jpg", 7, pair=False)
    assert torch.equal(fmasks[0], m0), "fused, pair=False: %d bytes differ" % int((fmasks[0] != m0).sum())
    for pipeline in (True, False):
        r2, m2 = tester.infer_images_multiscale([img, img], ["a.jpg", "a.jpg"], [7, 7], pipeline=pipeline, pair=False, return_masks=True)
        assert r2 == [plain_res, plain_res] and torch.equal(m2[0], m0) and torch.equal(m2[1], m0), "pair=False, pipeline=%s" % pipeline
        assert m2[0].untyped_storage().data_ptr() == m2[1].untyped_storage().data_ptr() and m2[1].data_ptr() % 16 == 0
    # pair=True: byte for byte only if the paired forward is bit-equal to the per-image forward — that equality first
    with torch.no_grad():
        for scale in mult:
            im_scale, h, w, hp, wp = T.scale_geometry(H, W, scale * H, 32)
            x = T.tta_input(dimg, h, w, hp, wp, 1.0 / im_scale)
            both, keep = tester.model.forward_heat(x)
            one = torch.cat([tester.model.forward_heat(x[:1])[0], tester.model.forward_heat(x[1:])[0]])
            assert both.shape[1] == 19 and torch.equal(both, one), "scale %.3f: the paired forward differs from the per-image one" % scale
            del keep
    pres, pmasks = tester.infer_image_multiscale_fused(img, "a.jpg", 7, return_masks=True)
    assert pres == plain_res and torch.equal(pmasks[0], m0), "fused, pair=True: %d bytes differ" % int((pmasks[0] != m0).sum())
    for pipeline in (True, False):
        r2, m2 = tester.infer_images_multiscale([img, img], pipeline=pipeline, return_masks=True)
        assert r2 == tester.infer_images_multiscale([img, img], pipeline=pipeline)
        assert torch.equal(m2[0], m0) and torch.equal(m2[1], m0), "pair=True, pipeline=%s" % pipeline
    assert torch.equal(tester.person_masks([img], multiscale=True)[0], m0)
    report("multi-scale person mask (R50 %s): thr %.6f, ON share %.3f, fused == unfused byte for byte (pair, unpaired, serial, pipelined)"
           % (rig["dtype"], thr, _share(m0)))


def test_a_plain_model_raises_before_any_device_work(monkeypatch):
    from multiposenet.pytorch_amd._lib import MpnError
    from test_model_gpu import get_model
    T = _tester_mod()
    tp = T.TestParams()
    tp.ckpt, tp.inp_size = None, 128
    tester = T.Tester(get_model(50, torch.float32).eval(), tp)
    seen = _spy(monkeypatch)
    img = np.zeros((96, 128, 3), dtype=np.float32)
    for fn in (lambda: tester.infer_image(img, return_masks=True), lambda: tester.infer_images_batched([img], return_masks=True),
               lambda: tester.infer_image_multiscale(img, return_masks=True), lambda: tester.infer_image_multiscale_fused(img, return_masks=True),
               lambda: tester.infer_images_multiscale([img], return_masks=True), lambda: tester.person_masks([img]),
               lambda: tester.seg_eval([(1, "a.jpg", img)], [])):
        with pytest.raises(MpnError):
            fn()
    assert seen == [], "launches before the refusal: %s" % seen


# ------------------------------------------------------------------------------------------------ launches
def _spy(monkeypatch):
    """The spy of tests/test_tta_fused_gpu.py: every module of the package that took ``call`` from _lib records the names it invokes."""
    from multiposenet.pytorch_amd import _lib
    import multiposenet.pytorch_amd.evaluate.seg_eval  # noqa: F401
    seen = []
    real = _lib.call

    def spy(name, *a):
        seen.append(name)
        return real(name, *a)
    for modname, mod in list(sys.modules.items()):
        if modname.startswith("multiposenet.pytorch_amd") and mod is not None and getattr(mod, "call", None) is real:
            monkeypatch.setattr(mod, "call", spy)
    return seen


def test_launch_accounting_with_and_without_masks(rig, monkeypatch):
    tester, img = rig["tester"], rig["img"]
    seen = _spy(monkeypatch)
    new = ("mpn_seg_masks", "mpn_tta_merge_mask", "mpn_mask_iou")
    tester.infer_image_multiscale_fused(img, "a.jpg", 7)
    plain = list(seen)
    assert (plain.count("mpn_tta_input"), plain.count("mpn_resize"), plain.count("mpn_tta_merge")) == (5, 5, 1)
    assert not any(s in plain for s in new)
    del seen[:]
    tester.infer_image_multiscale_fused(img, "a.jpg", 7, return_masks=True)
    with_masks = list(seen)
    extra = list(with_masks)
    for s in plain:
        extra.remove(s)                                             # ValueError if a launch of the plain path is missing
    assert sorted(extra) == ["mpn_resize"] * 5 + ["mpn_tta_merge_mask"], extra
    del seen[:]
    tester.infer_images_batched([img], ["a.jpg"], [7])
    plain = list(seen)
    assert not any(s in plain for s in new)
    del seen[:]
    tester.infer_images_batched([img], ["a.jpg"], [7], return_masks=True)
    extra = list(seen)
    for s in plain:
        extra.remove(s)
    assert extra == ["mpn_seg_masks"], extra


# ------------------------------------------------------------------------------------------------ seg_eval
@pytest.mark.parametrize("multiscale", [False, True], ids=["single-scale", "multi-scale"])
def test_seg_eval_equals_numpy(rig, multiscale):
    import person_seg_ref
    tester = rig["tester"]
    sizes = [(64, 65), (37, 53)]
    rs = np.random.RandomState(4)
    images = [(11 + i, "f%d.jpg" % i, rs.uniform(0, 255, (h, w, 3)).astype(np.float32)) for i, (h, w) in enumerate(sizes)]
    anns = []
    for (image_id, _, _), (h, w) in reversed(list(zip(images, sizes))):         # the json lists the second image's annotations first
        anns += [dict(a, image_id=image_id, category_id=1) for a in person_seg_ref.case_annotations(h, w)[0]]
    anns.append(dict(anns[0], image_id=999))                                    # an image that is not evaluated
    # the median of both images' unfused planes: neither mask is then all 0 or all 255 unless the two planes do not overlap in value
    planes = [(_multi_plane if multiscale else _single_plane)(tester, arr) for _, _, arr in images]
    _median_threshold(tester, torch.cat([p.flatten() for p in planes]))
    masks = [m.cpu().numpy() for m in tester.person_masks([arr for _, _, arr in images], multiscale=multiscale)]
    shares = [float((m != 0).mean()) for m in masks]
    assert all(0.0 < s < 1.0 for s in shares), "a predicted mask is all 0 or all 255 and would hide every fault: %s" % shares
    for batch in (64, 1):
        ev = tester.seg_eval(images, anns, multiscale=multiscale, batch=batch)
        assert ev is tester.last_seg_eval
        want = np.stack([ref.iou_counts_ref(m, person_seg_ref.mask_all(person_seg_ref.case_annotations(h, w)[0], h, w))
                         for m, (h, w) in zip(masks, sizes)])
        got = np.stack([ev["inter"], ev["pred"], ev["gt"]], 1)
        assert got.dtype == np.int64 and np.array_equal(got, want), (got.tolist(), want.tolist())
        summary = ref.summary_ref(want, [h * w for h, w in sizes])
        for k, v in summary.items():
            assert ev[k] == v, (k, ev[k], v)
        assert ev["image_ids"] == [11, 12] and ev["pixels"].tolist() == [h * w for h, w in sizes]
        assert (want[:, 0] > 0).all() and (want[:, 2] > 0).all()
    report("seg_eval (%s, R50 %s): iou %.4f, mean_iou %.4f, precision %.4f, recall %.4f, pixel_acc %.4f" % (
        "multi-scale" if multiscale else "single scale", rig["dtype"], ev["iou"], ev["mean_iou"], ev["precision"], ev["recall"], ev["pixel_acc"]))
