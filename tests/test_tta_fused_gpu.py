"""Fused, flip-paired multi-scale test-time augmentation (csrc/tta.hip, Tester.infer_image_multiscale_fused / infer_images_multiscale)
against the unfused path it must reproduce value for value: the two kernels bit for bit (G1, G2), the keypoint-only paired forward
(G3), the driver against the recorded run of the real reference Tester (G4), whole results end to end (G5) and the launches made (G6)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from helpers import GOLD, gold, report

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests selected but no GPU is visible"
    from multiposenet.pytorch_amd import _lib
    _lib.lib()


def _tester_mod():
    from multiposenet.pytorch_amd.evaluate import tester
    return tester


# ------------------------------------------------------------------------------------------------ G1: the input kernel
G1_SIZES = [(37, 53), (64, 48), (96, 128)]
G1_MULT = [0.5, 1.0, 2.5]


@pytest.mark.parametrize("strided", [False, True], ids=["dense", "strided"])
def test_g1_input_kernel_equals_crop_and_preprocess_bit_for_bit(strided):
    """mpn_tta_input against resnet_preprocess(crop_with_factor(x, s * H, 32, pad_val=128)[0]) for x = img and x = img.flip(1), 3 sizes
    x 3 multipliers: (96, 128) at 1.0 needs no padding, (37, 53) at 1.0 pads both axes, 0.5 shrinks, 2.5 enlarges.  ``strided``: the
    source is a view with gaps on every axis."""
    T = _tester_mod()
    rs = np.random.RandomState(3)
    pads = set()
    for H, W in G1_SIZES:
        if strided:
            big = torch.from_numpy(rs.uniform(0, 255, (2 * H, W + 5, 4)).astype(np.float32)).cuda()
            img = big[::2, 3:3 + W, :3]
            assert not img.is_contiguous()
        else:
            img = torch.from_numpy(rs.uniform(0, 255, (H, W, 3)).astype(np.float32)).cuda()
        for s in G1_MULT:
            im_scale, h, w, hp, wp = T.scale_geometry(H, W, s * H, 32)
            pads.add((hp > h, wp > w))
            got = T.tta_input(img, h, w, hp, wp, 1.0 / im_scale)
            for k, x in enumerate((img, img.flip(1).contiguous())):
                want = T.resnet_preprocess(T.crop_with_factor(x, s * H, 32, pad_val=128)[0])
                assert got[k].shape == want.shape, (H, W, s, k)
                bad = int((got[k] != want).sum())
                assert torch.equal(got[k], want), "%dx%d x%.1f image %d: %d of %d values differ, max %.3e" % (
                    H, W, s, k, bad, want.numel(), float((got[k] - want).abs().max()))
    assert (False, False) in pads and (True, True) in pads


# ------------------------------------------------------------------------------------------------ G2: the merge kernel
def _device_chain(heats, geo, H, W, n_div):
    """The unfused op sequence on the device for given heat-maps: _get_outputs' loop body per pass, _handle_heat, .float()."""
    T = _tester_mod()
    acc = []
    for p in range(2):
        a = torch.zeros((H, W, 18), dtype=torch.float64, device="cuda")
        for heat, (h, w) in zip(heats, geo):
            hm = heat[p].permute(1, 2, 0)
            hm = T.resize(hm, (hm.shape[0] * 4, hm.shape[1] * 4), cubic=True)
            hm = hm[0:h, 0:w, :]
            hm = T.resize(hm, (H, W), cubic=True)
            a = a + hm / n_div
        acc.append(a)
    return T.Tester._handle_heat(acc[0], acc[1])[:, :, :18].float().contiguous()


@pytest.mark.parametrize("H,W,scales", [(37, 53, 5), (64, 48, 5), (37, 53, 1)], ids=["37x53", "64x48", "single-scale"])
def test_g2_merge_kernel_equals_the_device_chain_and_the_restatement_bit_for_bit(H, W, scales):
    import tta_merge_ref as ref
    T = _tester_mod()
    g = torch.Generator().manual_seed(H * 100 + scales)
    mult = [x * 48 / float(H) for x in [0.5, 1., 1.5, 2, 2.5]][:scales] if scales > 1 else [1.5 * 48 / float(H)]
    heats, geo, maps = [], [], []
    for m in mult:
        _, h, w, hp, wp = T.scale_geometry(H, W, m * H, 32)
        heat = torch.rand((2, 18, hp // 4, wp // 4), generator=g).cuda()
        heats.append(heat)
        geo.append((h, w))
        maps.append(T.tta_upsample(heat, h, w))
    assert any(h < 4 * heat.shape[2] or w < 4 * heat.shape[3] for (h, w), heat in zip(geo, heats)), "no scale crops the x4 map"
    got = T.tta_merge(maps, H, W)
    want = _device_chain(heats, geo, H, W, len(mult))
    bad = int((got != want).sum())
    assert torch.equal(got, want), "%d of %d values differ from the device chain, max %.3e" % (bad, want.numel(), float((got - want).abs().max()))
    host_maps = [ref.upsample_crop_ref(heat.cpu().numpy(), h, w) for heat, (h, w) in zip(heats, geo)]
    for u, hu in zip(maps, host_maps):
        assert np.array_equal(u.cpu().numpy(), hu), "the 36-channel cropped up-sampling differs from the restatement"
    assert np.array_equal(got.cpu().numpy(), ref.merge_ref(host_maps, H, W)), "merge kernel differs from tests/tta_merge_ref.py"


# ------------------------------------------------------------------------------------------------ the network rig of G3, G5, G6
IMG_SIZES = [(96, 128), (80, 64), (77, 111), (128, 128)]


@pytest.fixture(scope="module", params=[torch.float32, torch.float16], ids=["fp32", "fp16"])
def rig(request):
    """R50, inp_size 128, random weights with the detector bias shifted so that people are found, seeded PRN weights (the setup of
    test_pipelined_batched_inference_equals_the_serial_one); the unfused results of the four images, computed once."""
    from multiposenet.pytorch_amd import synthetic as weightgen
    from test_model_gpu import get_model, t
    T = _tester_mod()
    m = get_model(50, request.param)
    sd = weightgen.gen_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items() if k.startswith("prn.")}, seed=3, flavour="he")
    m.load_state_dict({k: t(v) for k, v in sd.items()}, strict=False)
    m.eval()
    S = 128
    tp = T.TestParams()
    tp.ckpt, tp.inp_size = None, S
    tester = T.Tester(m, tp)
    rs = np.random.RandomState(11)
    images = [rs.uniform(0, 255, (h, w, 3)).astype(np.float32) for h, w in IMG_SIZES]
    names, ids = ["f%d.jpg" % i for i in range(len(images))], list(range(10, 10 + len(images)))
    with torch.no_grad():
        _, (cls, _, _) = m([torch.zeros(2, 3, S, S, device="cuda").normal_(), "detection_subnet"])
        s_ = cls.float().flatten().clamp(1e-6, 1 - 1e-6)
        q = torch.quantile(s_, 1.0 - 40.0 / float(cls.shape[1]))
        old_bias = m.classificationModel.output.bias.data.clone()
        m.classificationModel.output.bias.data += float(-torch.log(q / (1 - q)))
    try:
        unfused = [tester.infer_image_multiscale(images[i], names[i], ids[i]) for i in range(len(images))]
        yield {"model": m, "tester": tester, "images": images, "names": names, "ids": ids, "unfused": unfused, "dtype": request.param}
    finally:
        m.classificationModel.output.bias.data.copy_(old_bias)


@pytest.mark.parametrize("shape", [(2, 3, 96, 128), (2, 3, 64, 160)], ids=["96x128", "64x160"])
def test_g3_forward_heat_on_a_pair_equals_the_whole_network_image_by_image(rig, shape):
    m = rig["model"]
    x = torch.randn(shape, generator=torch.Generator().manual_seed(shape[3])).cuda()
    with torch.no_grad():
        heat, keep = m.forward_heat(x)
        assert heat.shape == (2, 18, shape[2] // 4, shape[3] // 4) and heat.dtype == torch.float32
        for i in range(2):
            want = m([x[i:i + 1], 'both'])[0]
            bad = int((heat[i:i + 1] != want).sum())
            assert torch.equal(heat[i:i + 1], want), "image %d of the pair: %d of %d values differ, max %.3e" % (
                i, bad, want.numel(), float((heat[i:i + 1] - want).abs().max()))
    del keep


def test_g5_fused_results_equal_the_unfused_ones(rig, tmp_path):
    tester, images, names, ids, unfused = rig["tester"], rig["images"], rig["names"], rig["ids"], rig["unfused"]
    people = sum(len(r) for r in unfused)
    assert people >= 4, "the unfused path finds %d people: the comparison would be empty" % people
    for pair in (True, False):
        for i in range(len(images)):
            got = tester.infer_image_multiscale_fused(images[i], names[i], ids[i], pair=pair)
            assert got == unfused[i], "image %d (%s), pair=%s" % (i, IMG_SIZES[i], pair)
    serial = tester.infer_images_multiscale(images, names, ids, pipeline=False)
    piped = tester.infer_images_multiscale(images, names, ids, pipeline=True)
    assert serial == unfused and piped == unfused
    triples = [(ids[i], names[i], images[i]) for i in (0, 2)]
    tester.params.coco_result_filename = str(tmp_path / "results.json")
    tester.params.testresult_write_json = True
    try:
        assert tester.params.tta_fused is False
        plain = tester.coco_eval(triples)
        plain_disk = json.load(open(tester.params.coco_result_filename))
        os.remove(tester.params.coco_result_filename)
        tester.params.tta_fused = True
        fused = tester.coco_eval(triples)
        fused_disk = json.load(open(tester.params.coco_result_filename))
    finally:
        tester.params.tta_fused = False
        tester.params.testresult_write_json = False
    assert plain == unfused[0] + unfused[2] and fused == plain and fused_disk == plain_disk and len(fused_disk) == len(fused)
    report("fused TTA (R50 %s, inp_size 128, 4 images): %d people, result dicts identical to infer_image_multiscale (pair, unpaired, serial, pipelined, coco_eval)"
           % (rig["dtype"], people))


def _spy(monkeypatch):
    """Every module of the package that took ``call`` from _lib records the entry point names it invokes."""
    from multiposenet.pytorch_amd import _lib
    seen = []
    real = _lib.call

    def spy(name, *a):
        seen.append(name)
        return real(name, *a)
    for modname, mod in list(sys.modules.items()):
        if modname.startswith("multiposenet.pytorch_amd") and mod is not None and getattr(mod, "call", None) is real:
            monkeypatch.setattr(mod, "call", spy)
    return seen


def test_g6_launch_accounting(rig, monkeypatch):
    tester, images, names, ids = rig["tester"], rig["images"], rig["names"], rig["ids"]
    seen = _spy(monkeypatch)
    n = len(images)
    new = ("mpn_tta_input", "mpn_tta_merge")

    def detections():
        return sum(1 for s in seen if s.startswith("mpn_score_filter")), sum(1 for s in seen if s.startswith("mpn_box_decode_clip"))
    tester.infer_images_multiscale(images, names, ids)
    assert seen.count("mpn_tta_input") == 5 * n and seen.count("mpn_resize") == 5 * n and seen.count("mpn_tta_merge") == n
    assert detections() == (n, n), "the detection head runs once per image"
    del seen[:]
    tester.infer_image_multiscale_fused(images[0], names[0], ids[0])
    assert (seen.count("mpn_tta_input"), seen.count("mpn_resize"), seen.count("mpn_tta_merge")) == (5, 5, 1) and detections() == (1, 1)
    del seen[:]
    assert tester.params.tta_fused is False
    tester.params.coco_result_filename = os.devnull
    tester.coco_eval([(ids[0], names[0], images[0])])
    assert not any(s in seen for s in new) and detections() == (10, 10) and seen.count("mpn_resize") == 30


# ------------------------------------------------------------------------------------------------ G4: the driver vs the real Tester
class _PairStandin(object):
    """tests/tta_standin.py behind the three methods the fused path calls.  Rows of image 1 of a pair (the mirrored pass) are shifted by
    7 pixels: the stand-in's boxes depend on the padded shape only, and a driver that took them would otherwise go unnoticed."""

    def __init__(self):
        self.shapes = []

    def _both(self, x):
        import tta_standin
        assert x.is_cuda and x.dtype == torch.float32
        self.shapes.append(tuple(int(v) for v in x.shape))
        return [tta_standin.standin_outputs(x[i:i + 1]) for i in range(x.shape[0])]

    def forward_heat(self, x):
        return torch.cat([o[0] for o in self._both(x)]), None

    def forward_padded_begin(self, x):
        outs = self._both(x)
        boxes = torch.stack([o[1][2] + 7.0 * i for i, o in enumerate(outs)])
        cls = torch.zeros((len(outs), boxes.shape[1], 2), dtype=torch.float32, device=x.device)
        for i, o in enumerate(outs):
            cls[i].scatter_(1, o[1][1].long()[:, None], o[1][0][:, None])
        return torch.cat([o[0] for o in outs]), boxes, cls, None

    @staticmethod
    def detect_padded(anchors, cls, pre_nms_top_n=None, return_class=False, class_wise=False):
        score, cid = cls.max(-1)
        order = torch.argsort(score, dim=1, descending=True, stable=True)
        out = (torch.gather(anchors, 1, order[:, :, None].expand(-1, -1, 4)), torch.gather(score, 1, order), [anchors.shape[1]] * anchors.shape[0])
        return out + (torch.gather(cid, 1, order),) if return_class else out


def test_g4_fused_driver_matches_the_real_reference_tester(tmp_path):
    """The checks of test_tta_driver_matches_the_real_reference_tester on the fused path: the same keypoints, scores and ids as the
    recorded result file, boxes within 1e-3; the joints and boxes handed to prn_process as recorded."""
    import tta_standin
    T = _tester_mod()
    g = gold("g15_tta.npz")
    fixture = json.load(open(os.path.join(GOLD, "g15_tta_results.json")))
    prn_args = []
    t = T.Tester.__new__(T.Tester)
    t.params = T.TestParams()
    t.params.inp_size = 48
    t.params.tta_fused = True
    t.params.coco_result_filename = str(tmp_path / "results.json")
    t.params.testresult_write_json = True
    t.dev = torch.device("cuda", 0)
    t.model = _PairStandin()
    t.prn_process = lambda kps, boxes, name, image_id=0: (prn_args.append((kps, boxes, name, image_id)) or
                                                         tta_standin.fake_prn_results(kps, boxes, name, image_id))
    images = [(11, "img11.jpg", g["img_a"]), (22, "img22.jpg", g["img_b"])]
    results = t.coco_eval(images)
    want_shapes = [(2,) + tuple(r[1:]) for tag in ("a", "b") for r in g["shapes_" + tag].tolist()]
    assert t.model.shapes == want_shapes, "pair input shapes %s != reference %s" % (t.model.shapes, want_shapes)
    assert len(prn_args) == int(g["n_images"])
    for i, (kps, boxes, name, image_id) in enumerate(prn_args):
        ref_k, ref_b = g["prn_kps_%d" % i], g["prn_boxes_%d" % i]
        assert image_id == int(g["prn_id_%d" % i]) and name == images[i][1]
        got_b = np.array(boxes, dtype=np.float64).reshape(-1, 4)
        assert got_b.shape == ref_b.shape and np.abs(got_b - ref_b).max() <= 1e-3, "prn_process got another scale's or the mirrored pass's boxes"
        got_k = np.array(kps, dtype=np.float64).reshape(-1, 5)
        assert got_k.shape == ref_k.shape, "image %d: %d joints, reference %d" % (i, got_k.shape[0], ref_k.shape[0])
        assert np.array_equal(got_k[:, 3:], ref_k[:, 3:]), "joint ids / types differ"
        assert np.abs(got_k[:, 2] - ref_k[:, 2]).max() <= 1e-4, "peak scores differ"
        assert np.abs(got_k[:, :2] - ref_k[:, :2]).max() <= 1.0, "peak coordinates differ by more than a pixel"
    ref_res = fixture["results"]
    on_disk = json.load(open(t.params.coco_result_filename))
    assert len(results) == len(ref_res) == len(on_disk)
    for r, q, o in zip(results, ref_res, on_disk):
        assert r["image_id"] == q["image_id"] and r["file_name"] == q["file_name"] and r["category_id"] == q["category_id"]
        assert r["keypoints"] == q["keypoints"] == o["keypoints"], "COCO keypoint order differs"
        assert r["score"] == q["score"] and np.abs(np.array(r["bbox"]) - np.array(q["bbox"])).max() <= 1e-3
