"""GPU side of the smoothed peak refinement: ``NMS(..., bool_gaussian_filt=True)`` (mpn_heatmap_peaks_smooth, csrc/peaks.hip:
peaks_refine_smooth_kernel) against the recorded run of the reference's own NMS with real scipy (tests/golden/g20_peaks_gauss.npz)
and against the numpy restatement (tests/peaks_gauss_ref.py) — exactly: coordinates, ids, and scores as float32 bits widened to double.
tests/test_peaks_gauss_cpu.py shows on the golden alone that the flag changes every score, so a kernel ignoring it cannot pass."""
import numpy as np
import pytest
import torch

import peaks_gauss_ref as pg
from helpers import gold, report

pytestmark = pytest.mark.gpu

CASES = ("c1", "c2", "c3", "c4", "c5", "c6", "c7", "c8")
PARAM = {"thre1": 0.1}
_g = {}


def g20():
    if "g" not in _g:
        _g["g"] = gold("g20_peaks_gauss.npz")
    return _g["g"]


def ju():
    from multiposenet.pytorch_amd.network import joint_utils
    return joint_utils


def assert_rows(got, want, what):
    assert got.shape == want.shape, "%s: %d rows, want %d" % (what, len(got), len(want))
    assert np.array_equal(got[:, [0, 1, 3, 4]], want[:, [0, 1, 3, 4]]), "%s: coordinates / ids differ" % what
    assert np.array_equal(got[:, 2].view(np.uint64), want[:, 2].view(np.uint64)), "%s: score bits differ" % what
    assert np.array_equal(got[:, 2], got[:, 2].astype(np.float32).astype(np.float64)), "%s: a score is no widened float32" % what


@pytest.mark.parametrize("case", CASES)
def test_smoothed_nms_equals_reference_golden_and_restatement(case):
    g = g20()
    heat, f = g["heat_" + case], float(g["f_" + case])
    dev = torch.from_numpy(heat).cuda()
    got = pg.rows(ju().NMS(PARAM, dev, f, True, True))
    assert_rows(got, g["on_" + case], "%s flag on vs golden" % case)
    assert_rows(got, pg.rows(pg.nms_peaks_smooth(0.1, heat, f)), "%s flag on vs restatement" % case)
    # the plain path is untouched, and the flag is ignored without the refinement (joint_utils.py:101-116)
    assert_rows(pg.rows(ju().NMS(PARAM, dev, f, True, False)), g["off_" + case], "%s flag off vs golden" % case)
    assert_rows(pg.rows(ju().NMS(PARAM, dev, f, False, True)), g["plain_" + case], "%s no refinement, flag on" % case)
    report("smoothed peak refinement %s (f = %g, %d peaks): rows identical to the reference's NMS with scipy's gaussian_filter" % (case, f, len(got)))


def test_layouts_and_batches_give_the_same_rows():
    """Channels-last and planar [B, J, H, W], a strided view, and a 2-image batch through NMS_batch / NMS_batch_arrays; ids run per image."""
    g = g20()
    a, b = g["heat_c1"], g["heat_c1"][::-1, ::-1].copy()                     # same map size, factor 4
    want = [g["on_c1"], pg.rows(pg.nms_peaks_smooth(0.1, b, 4.0))]
    planar = torch.from_numpy(np.stack([a, b]).transpose(0, 3, 1, 2).copy()).cuda()          # [2, 18, H, W] contiguous
    cl = planar.contiguous(memory_format=torch.channels_last)
    wide = torch.zeros((2, 18, a.shape[0] + 3, 2 * a.shape[1] + 5), device="cuda")
    view = wide[:, :, 2:2 + a.shape[0], 1:1 + 2 * a.shape[1]:2]                                  # x stride 2, padded rows
    view.copy_(planar)
    assert cl.stride(1) == 1 and planar.stride(3) == 1 and view.stride(3) == 2
    for name, t in (("channels-last", cl), ("planar", planar), ("strided view", view)):
        per_image = ju().NMS_batch(PARAM, t, 4.0, True, None, bool_gaussian_filt=True)
        assert len(per_image) == 2
        for i in range(2):
            assert_rows(pg.rows(per_image[i]), want[i], "%s image %d" % (name, i))
        pk, cnt = ju().NMS_batch_arrays(PARAM, t, 4.0, bool_gaussian_filt=True)
        for i in range(2):
            again = pg.rows([pk[i, j, :cnt[i, j]] for j in range(18)])
            assert_rows(again, want[i], "%s image %d (arrays)" % (name, i))
        assert want[1][0, 3] == 0.0                                                              # ids restart with every image
    plain = ju().NMS_batch(PARAM, cl, 4.0)                                                      # positional callers: the flag stays off
    assert_rows(pg.rows(plain[0]), g["off_c1"], "NMS_batch default")


def test_get_joint_list_with_the_flag():
    g = g20()
    heat = g["heat_c1"]
    dev = torch.from_numpy(heat).cuda()
    img = np.zeros((heat.shape[0] * 4, heat.shape[1] * 4, 3), dtype=np.float32)                  # shape[0] / heat rows = 4
    got = ju().get_joint_list(img, PARAM, dev, 1.5, bool_gaussian_filt=True)
    want = g["on_c1"].copy()
    want[:, :2] *= 1.5
    assert_rows(np.asarray(got), want, "get_joint_list")
    off = g["off_c1"].copy()
    off[:, :2] *= 1.5
    assert_rows(np.asarray(ju().get_joint_list(img, PARAM, dev, 1.5)), off, "get_joint_list default")


def test_widest_supported_factor_and_the_refusal_beyond():
    from multiposenet.pytorch_amd._lib import MpnError
    g = g20()
    dev = torch.from_numpy(g["heat_c5"]).cuda()
    assert float(g["f_c5"]) == 12.8
    assert len(pg.rows(ju().NMS(PARAM, dev, 12.8, True, True))) == len(g["on_c5"])             # rint(64.0) = 64: the largest patch
    with pytest.raises(MpnError, match=r"rint\(5 \* upsampFactor\) <= 64"):
        ju().NMS(PARAM, dev, 13.0, True, True)
    assert len(pg.rows(ju().NMS(PARAM, dev, 13.0, False, True))) == len(g["on_c5"])            # no refinement: nothing to smooth, no limit
    assert len(pg.rows(ju().NMS(PARAM, dev, 13.0, True, False))) == len(g["on_c5"])            # the plain path has its direct form


def test_explicit_capacity_is_a_hard_limit_as_on_the_plain_path():
    from multiposenet.pytorch_amd._lib import MpnError
    g = g20()
    dev = torch.from_numpy(g["heat_c7"]).cuda()                                                 # ridge planes: 16 peaks in one plane
    most = int(np.bincount(g["on_c7"][:, 4].astype(int)).max())
    assert most > 8
    for flag in (False, True):
        with pytest.raises(MpnError, match="raise `cap`"):
            ju().NMS(PARAM, dev, 1.0, True, flag, cap=8)
    assert_rows(pg.rows(ju().NMS(PARAM, dev, 1.0, True, True, cap=most)), g["on_c7"], "cap == most")
    assert_rows(pg.rows(ju().NMS(PARAM, dev, 1.0, True, True, cap=None)), g["on_c7"], "growing capacity")


def test_tester_batched_equals_per_image_with_the_flag(monkeypatch):
    """Tester on a toy model (R50, fp16, 128 x 128 input): infer_images_batched with gaussian_filt=True equals per-image infer_image with
    the same flag, and both go through the smoothed entry point."""
    from multiposenet.pytorch_amd.evaluate.tester import Tester, TestParams
    from multiposenet.pytorch_amd import synthetic as weightgen
    from test_model_gpu import get_model, t
    m = get_model(50, torch.float16)
    sd = weightgen.gen_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items() if k.startswith("prn.")}, seed=3, flavour="he")
    m.load_state_dict({k: t(v) for k, v in sd.items()}, strict=False)
    m.eval()
    S = 128
    rs = np.random.RandomState(13)
    images = [rs.uniform(0, 255, hw + (3,)).astype(np.float32) for hw in ((S, S), (100, 128), (128, 90), (77, 111))]
    assert TestParams.gaussian_filt is False
    tp = TestParams()
    tp.ckpt, tp.inp_size, tp.gaussian_filt = None, S, True
    tester = Tester(m, tp)
    seen = []
    real = ju().call
    monkeypatch.setattr(ju(), "call", lambda name, *a: (seen.append(name), real(name, *a))[1])
    with torch.no_grad():
        _, (cls, _, _) = m([torch.zeros(2, 3, S, S, device="cuda").normal_(), "detection_subnet"])
        s_ = cls.float().flatten().clamp(1e-6, 1 - 1e-6)
        q = torch.quantile(s_, 1.0 - 30.0 / float(cls.shape[1]))
        old_bias = m.classificationModel.output.bias.data.clone()
        m.classificationModel.output.bias.data += float(-torch.log(q / (1 - q)))
    try:
        names, ids = ["f%d.jpg" % i for i in range(len(images))], list(range(len(images)))
        batched = tester.infer_images_batched(images, names, ids, batch=4)
        assert seen.count("mpn_heatmap_peaks_smooth") >= 1 and "mpn_heatmap_peaks" not in seen
        for i in range(len(images)):
            assert tester.infer_image(images[i], names[i], i) == batched[i], i
        assert "mpn_heatmap_peaks" not in seen
        people = sum(len(r) for r in batched)
        tp.gaussian_filt = False
        del seen[:]
        tester.infer_images_batched(images, names, ids, batch=4)
        assert "mpn_heatmap_peaks_smooth" not in seen and "mpn_heatmap_peaks" in seen                # the default launches what it did
    finally:
        m.classificationModel.output.bias.data.copy_(old_bias)
    report("Tester with gaussian_filt (R50 f16 128x128, 4 images): %d people, batched results identical to per-image inference" % people)
