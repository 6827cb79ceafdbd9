"""GPU tests of the device augmentation (csrc/augment.hip through datasets/augment.py: mpn_augment_image, mpn_augment_mask,
DeviceAugmenter).

PARITY.  Image and mask kernels against the float64 one-pass restatement tests/augment_ref.py on the cases of
tests/golden/g17_augment.npz (geometry recorded from the reference's real functions) with seeded synthetic sources.  Per element,
no element left out:
    |got - ref| <= C_SUM u mag + W_ABS u wabs,    u = 2^-24
with mag the same sum over absolute values carried through the normalisation and wabs the largest of the 16 taps on the same
scale.  Both constants come from operation counts, written out in augment_ref's docstring and not tuned to any observed error:
  C_SUM = 12 (image) / 10 (mask): 8 float32 roundings on the longest path of the 16-term sum (product, three additions, product,
          three additions), 3 (image: / 255, - mean, / std) or 1 (mask: / 255) after it, 1 for second-order terms;
  W_ABS = 2 * 1.375 * 136 = 374: the four float32 weights of an axis are off by at most 136 u in total against the float64
          polynomial at the same float32 fraction (40 + 12 + 14 + 70 by the count of interpolateCubic's operations), the other
          axis contributes sum |w| <= 1.375, two axes.
The inside/outside decisions are float64 in the same operation order on both sides, so they agree exactly; elements outside are
required to be EXACTLY the normalised 128 / 1.0.  test_augment_cpu.py shows that this bound is violated by a wrong cubic constant,
shifted taps, a missing channel swap, a flip over the wrong width and a half-pixel offset.
"""
import numpy as np
import pytest
import torch

import augment_ref as ar
from helpers import report

pytestmark = pytest.mark.gpu

CASES, INP, STRIDE = ar.golden_cases()
GRID = INP // STRIDE


def _sample(i, c, with_mask=True):
    img, mask = ar.synth_sources(40 + i, int(c["hw"][0]), int(c["hw"][1]))
    return {"img": torch.from_numpy(img), "mask_miss": torch.from_numpy(mask) if with_mask else None, "objpos": c["objpos_in"],
            "scale_provided": float(c["scale_provided"]), "joint_self": c["joint_self_in"], "joint_others": c["joint_others_in"],
            "objpos_other": c["objpos_other_in"]}


def _ref_geo(c):
    o = (int(c["center"][0]) + INP // 2 - INP, int(c["center"][1]) + INP // 2 - INP)
    return ar.geometry(c["M"], c["scale"], c["stage_shapes"][0][:2], c["stage_shapes"][1][:2], o, int(c["flip"]))


def _pad_values():
    mean, std = np.array(ar.MEANS, dtype=np.float32), np.array(ar.STDS, dtype=np.float32)
    return ((np.float32(128.0) / np.float32(255.0) - mean) / std).astype(np.float32)


def _run_case(i, with_mask=True):
    from multiposenet.pytorch_amd.datasets.augment import DeviceAugmenter
    c = CASES[i]
    da = DeviceAugmenter(INP, STRIDE, ar.case_params(c))
    img, heat, hm, meta = da([_sample(i, c, with_mask)], dice=c["dice"][None])
    torch.cuda.synchronize()
    return c, img, heat, hm, meta


@pytest.mark.parametrize("i", range(len(CASES)))
def test_image_and_mask_kernels_vs_float64_restatement(i):
    c, img, heat, hm, meta = _run_case(i)
    assert img.dtype == torch.float32 and img.is_contiguous() and tuple(img.shape) == (1, 3, INP, INP)
    assert hm.dtype == torch.float32 and hm.is_contiguous() and tuple(hm.shape) == (1, 18, GRID, GRID)
    geo = _ref_geo(c)
    src_img, src_mask = ar.synth_sources(40 + i, int(c["hw"][0]), int(c["hw"][1]))
    got = img[0].cpu().numpy().astype(np.float64)
    ref, mag, wabs = ar.image_ref(src_img, geo, INP, INP)
    r = ar.ratio(got, ref, mag, wabs, ar.C_SUM_IMAGE)
    w = np.unravel_index(int(np.argmax(r)), r.shape)
    report("%-58s %-52s worst err/bound=%.3f at (c=%d, y=%d, x=%d)  %s" % ("augment_image golden case %d" % i, "one-pass cubic, f32",
                                                                            r.max(), w[0], w[1], w[2], "OK" if r.max() <= 1 else "FAIL"))
    print("image case %d: worst err/bound %.4f, max abs err %.3e, pad fraction %.3f" % (i, r.max(), np.abs(got - ref).max(), (wabs[0] == 0).mean()))
    # outside the canvas / the scaled image (found with a constant source: wabs is 0 exactly there): exactly the normalised 128
    pad = np.broadcast_to(_pad_values()[:, None, None], got.shape)
    outside = ar.image_ref(np.full_like(src_img, 7), geo, INP, INP)[2] == 0
    assert np.array_equal(img[0].cpu().numpy()[outside], pad[outside])
    assert r.max() <= 1.0, "image case %d: element %s got %r ref %r, err/bound %.3f" % (i, w, got[w], ref[w], r.max())

    gm = hm[0].cpu().numpy()
    for k in range(1, 18):
        assert np.array_equal(gm[k], gm[0]), "mask channel %d differs from channel 0" % k
    ref, mag, wabs = ar.mask_ref(src_mask, geo, GRID, GRID, STRIDE, INP)
    r = ar.ratio(gm[0].astype(np.float64), ref, mag, wabs, ar.C_SUM_MASK)
    w = np.unravel_index(int(np.argmax(r)), r.shape)
    report("%-58s %-52s worst err/bound=%.3f at (y=%d, x=%d)  %s" % ("augment_mask golden case %d" % i, "one-pass cubic, f32", r.max(), w[0], w[1],
                                                                     "OK" if r.max() <= 1 else "FAIL"))
    print("mask case %d: worst err/bound %.4f, max abs err %.3e" % (i, r.max(), np.abs(gm[0] - ref).max()))
    outside = ar.mask_ref(np.full_like(src_mask, 7), geo, GRID, GRID, STRIDE, INP)[2] == 0
    assert np.all(gm[0][outside] == np.float32(1.0))
    assert r.max() <= 1.0, "mask case %d: element %s got %r ref %r, err/bound %.3f" % (i, w, gm[0][w], ref[w], r.max())
    assert gm.min() >= 0.0 and gm.max() <= 1.0


def test_ragged_blocks_of_the_image_and_mask_kernels_in_a_batch_of_two():
    """The kernels called directly at output shapes that end inside a block: an image of 5 x 65 (one full wave plus one lane, a
    4-row block plus one row) and a mask grid of 3 x 87 = 261 cells (one full 256-lane workgroup plus five lanes), two samples per
    launch so blockIdx.z selects the table row and the source.  Geometry of one unflipped and one flipped golden case from the
    recorded values, the crop origin moved so that the small window lies in the middle of the recorded crop.  Same bound as above."""
    from multiposenet.pytorch_amd.datasets import augment as aug
    pair = [next(i for i, c in enumerate(CASES) if int(c["flip"]) == f) for f in (0, 1)]
    CY, CX, GH, GW = 5, 65, 3, 87
    srcs = [ar.synth_sources(40 + i, int(CASES[i]["hw"][0]), int(CASES[i]["hw"][1])) for i in pair]
    ioff, moff = ([0, (srcs[0][k].size + 15) // 16 * 16] for k in (0, 1))       # every source on a 16-byte boundary
    buf_i, buf_m = (np.zeros(off[1] + srcs[1][k].size, dtype=np.uint8) for k, off in ((0, ioff), (1, moff)))
    geos = {"image": [], "mask": []}
    rows = {"image": [], "mask": []}
    for b, i in enumerate(pair):
        c, (H, W) = CASES[i], srcs[b][0].shape[:2]
        buf_i[ioff[b]: ioff[b] + srcs[b][0].size] = srcs[b][0].reshape(-1)
        buf_m[moff[b]: moff[b] + srcs[b][1].size] = srcs[b][1].reshape(-1)
        ox, oy = int(c["center"][0]) + INP // 2 - INP, int(c["center"][1]) + INP // 2 - INP
        for kind, o in (("image", (ox + (INP - CX) // 2, oy + (INP - CY) // 2)),
                        ("mask", (ox + (INP - GW * STRIDE) // 2, oy + (INP - GH * STRIDE) // 2))):
            g = ar.geometry(c["M"], c["scale"], c["stage_shapes"][0][:2], c["stage_shapes"][1][:2], o, int(c["flip"]))
            geos[kind].append(g)
            rows[kind].append(aug.table_row(g, H, W, ioff[b], W * 3, moff[b], W))
    img = aug.augment_image(torch.from_numpy(buf_i).cuda(), torch.from_numpy(np.stack(rows["image"])).cuda(), CY, CX)
    hm = aug.augment_mask(torch.from_numpy(buf_m).cuda(), torch.from_numpy(np.stack(rows["mask"])).cuda(), GH, GW, STRIDE, GW * STRIDE)
    torch.cuda.synchronize()
    assert tuple(img.shape) == (2, 3, CY, CX) and tuple(hm.shape) == (2, 18, GH, GW)
    for b in range(2):
        ref, mag, wabs = ar.image_ref(srcs[b][0], geos["image"][b], CY, CX)
        assert (wabs[0] > 0).mean() > 0.25                             # the window shows the source, not only pad
        r = ar.ratio(img[b].cpu().numpy().astype(np.float64), ref, mag, wabs, ar.C_SUM_IMAGE)
        print("ragged image sample %d: worst err/bound %.4f" % (b, r.max()))
        assert r.max() <= 1.0, (b, np.unravel_index(int(np.argmax(r)), r.shape), r.max())
        gm = hm[b].cpu().numpy()
        assert all(np.array_equal(gm[k], gm[0]) for k in range(1, 18))
        ref, mag, wabs = ar.mask_ref(srcs[b][1], geos["mask"][b], GH, GW, STRIDE, GW * STRIDE)
        assert (wabs > 0).mean() > 0.25
        r = ar.ratio(gm[0].astype(np.float64), ref, mag, wabs, ar.C_SUM_MASK)
        print("ragged mask sample %d: worst err/bound %.4f" % (b, r.max()))
        assert r.max() <= 1.0, (b, np.unravel_index(int(np.argmax(r)), r.shape), r.max())


def test_exact_case_identity_transform_returns_the_source_pixels():
    """Even-sized source, scale 1 (scale_provided = target_dist, scale_prob 0), 0 degrees (dice 0.5), no flip, crop inside the image:
    every fraction is 0, the cubic weights are exactly (0, 1, 0, 0), so the image must EQUAL (src / 255 - mean) / std computed in
    float32 and the mask src / 255 at the sampled cells.  Independent of augment_ref.  The mask is checked at stride 1 (cells on
    pixels) and at stride 4 on a mask that is constant over aligned 4 x 4 blocks (fraction 0.5, weights (-3, 19, 19, -3) / 32: the
    products and sums of a constant are exact)."""
    from multiposenet.pytorch_amd.datasets.augment import DeviceAugmenter, DEFAULT_PARAMS
    H, W, S = 600, 640, 128
    rs = np.random.RandomState(2)
    src = rs.randint(0, 256, size=(H, W, 3)).astype(np.uint8)
    m1 = rs.randint(0, 256, size=(H, W)).astype(np.uint8)
    m4 = np.repeat(np.repeat(rs.randint(0, 256, size=(H // 4, W // 4)), 4, 0), 4, 1).astype(np.uint8)
    mean, std = np.array(ar.MEANS, dtype=np.float32), np.array(ar.STDS, dtype=np.float32)
    dice = np.array([[0.7, np.nan, 0.5, 0.5, 0.5, 0.9]])
    for stride, mask in ((1, m1), (4, m4)):
        da = DeviceAugmenter(S, stride, dict(DEFAULT_PARAMS, scale_prob=0.0))
        s = {"img": torch.from_numpy(src), "mask_miss": torch.from_numpy(mask), "objpos": (320.0, 300.0), "scale_provided": 0.6,
             "joint_self": np.ones((18, 3))}
        img, heat, hm, meta = da([s], dice=dice)
        g = meta[0]
        assert g["scale"] == 1.0 and g["degree"] == 0.0 and not g["flip"] and (g["ox"], g["oy"]) == (320 - S // 2, 300 - S // 2)
        assert g["ox"] % 4 == 0 and g["oy"] % 4 == 0
        crop = src[g["oy"]:g["oy"] + S, g["ox"]:g["ox"] + S, ::-1].astype(np.float32).transpose(2, 0, 1)
        want = ((crop / np.float32(255.0) - mean[:, None, None]) / std[:, None, None]).astype(np.float32)
        assert np.array_equal(img[0].cpu().numpy(), want)
        mc = mask[g["oy"]:g["oy"] + S, g["ox"]:g["ox"] + S].astype(np.float32)
        cells = mc if stride == 1 else mc[1::4, 1::4]                  # cell j samples crop coordinate 4 j + 1.5: inside block j
        wantm = (cells / np.float32(255.0)).astype(np.float32)
        assert np.array_equal(hm[0, 0].cpu().numpy(), wantm) and np.array_equal(hm[0, 17].cpu().numpy(), wantm)


def test_pad_regions_are_exactly_the_normalised_border_values():
    """A person in the image corner (golden cases 4 and 5): a large part of the crop lies outside the rotated canvas.  Those
    elements are exactly (128 / 255 - mean) / std in float32 and exactly 1.0 in the mask, and they are many."""
    for i in (4, 5):
        c, img, heat, hm, meta = _run_case(i)
        geo = _ref_geo(c)
        src_img, src_mask = ar.synth_sources(40 + i, int(c["hw"][0]), int(c["hw"][1]))
        _, _, wabs = ar.image_ref(np.full_like(src_img, 7), geo, INP, INP)          # wabs == 0 exactly outside (every tap is 7 inside)
        outside = wabs[0] == 0
        assert 0.3 < outside.mean() < 0.95
        got = img[0].cpu().numpy()
        for ch, v in enumerate(_pad_values()):
            assert np.all(got[ch][outside] == v)
        _, _, wm = ar.mask_ref(np.full_like(src_mask, 7), geo, GRID, GRID, STRIDE, INP)
        assert (wm == 0).mean() > 0.3 and np.all(hm[0].cpu().numpy()[:, wm == 0] == np.float32(1.0))


def _bench_batch(B=32, S=480, seed=5):
    rs = np.random.RandomState(seed)
    samples = []
    for b in range(B):
        img, mask = ar.synth_sources(seed * 100 + b, 480, 640)
        n = int(rs.randint(0, 4))
        j = np.zeros((1 + n, 17, 3))
        j[..., 0], j[..., 1], j[..., 2] = rs.uniform(0, 640, (1 + n, 17)), rs.uniform(0, 480, (1 + n, 17)), rs.choice([0.0, 1.0, 2.0], (1 + n, 17))
        samples.append({"img": torch.from_numpy(img), "mask_miss": torch.from_numpy(mask), "objpos": (rs.uniform(100, 540), rs.uniform(100, 380)),
                        "scale_provided": float(rs.uniform(0.3, 1.0)), "joint_self": j[0], "joint_others": j[1:]})
    return samples


def test_full_size_batch_is_deterministic_and_batch_independent():
    """B = 32, 480 x 480 from 640 x 480 sources: two runs are bit-identical, and a sub-batch equals its rows of the full batch."""
    import random
    from multiposenet.pytorch_amd.datasets.augment import DeviceAugmenter, draw_dice
    samples = _bench_batch()
    rng = random.Random(3)
    dice = np.stack([draw_dice(rng) for _ in samples])
    da = DeviceAugmenter(480, 4)
    a = da(samples, dice=dice)
    b = da(samples, dice=dice)
    torch.cuda.synchronize()
    for x, y in zip(a[:3], b[:3]):
        assert tuple(x.shape)[0] == 32 and torch.equal(x, y)
    assert torch.isfinite(a[0]).all() and float(a[2].min()) >= 0.0 and float(a[2].max()) <= 1.0
    sub = [3, 17, 31]
    c = da([samples[k] for k in sub], dice=dice[sub])
    for x, y in zip(a[:3], c[:3]):
        assert torch.equal(x[sub], y)
    # the same stream through rng= gives the same batch
    d = da(samples, rng=random.Random(3))
    assert torch.equal(d[0], a[0]) and torch.equal(d[2], a[2]) and torch.equal(d[1], a[1])


def test_device_augmenter_end_to_end_on_the_golden_cases():
    """All golden cases with default parameters as ONE batch: the heat-maps equal put_gaussian_maps on the reference's own final
    joints bit for bit, every image / mask equals its single-sample run, and the image-only form returns the same img."""
    from multiposenet.pytorch_amd.datasets.augment import DeviceAugmenter
    from multiposenet.pytorch_amd.datasets.heatmap import put_gaussian_maps
    idx = [i for i, c in enumerate(CASES) if np.array_equal(c["params"], [0.8, 1.2, 1, 0.6, 40, 40, 0.3])]
    assert len(idx) >= 6
    da = DeviceAugmenter(INP, STRIDE)
    dice = np.stack([CASES[i]["dice"] for i in idx])
    img, heat, hm, meta = da([_sample(i, CASES[i]) for i in idx], dice=dice)
    maxP = max(1 + CASES[i]["joint_others_out"].shape[0] for i in idx)
    joints = np.zeros((len(idx), maxP, 18, 3))
    num = np.zeros(len(idx), dtype=np.int32)
    for b, i in enumerate(idx):
        c = CASES[i]
        n = c["joint_others_out"].shape[0]
        joints[b, 0], joints[b, 1:1 + n], num[b] = c["joint_self_out"], c["joint_others_out"], 1 + n
        assert np.array_equal(meta[b]["joint_self_out"], c["joint_self_out"])
    want = put_gaussian_maps(torch.from_numpy(joints).cuda(), torch.from_numpy(num).cuda(), INP, INP, STRIDE, 7.0)
    assert heat.dtype == torch.float32 and heat.is_contiguous() and torch.equal(heat, want) and float(heat.max()) > 0.5
    for b, i in enumerate(idx[:3]):
        _, im1, h1, m1, _ = _run_case(i)
        assert torch.equal(im1[0], img[b]) and torch.equal(m1[0], hm[b]) and torch.equal(h1[0], heat[b])
    img2, heat2, hm2, _ = da([_sample(i, CASES[i], with_mask=False) for i in idx], dice=dice)
    assert hm2 is None and torch.equal(img2, img) and torch.equal(heat2, heat)


def test_augmented_batch_trains_a_keypoint_subnet():
    """The triple goes unchanged through batch_processor and one eager train_step of an R50 keypoint_subnet at 128 x 128, and
    through the recorded step; both losses are finite."""
    from multiposenet.pytorch_amd.datasets.augment import DeviceAugmenter
    from multiposenet.pytorch_amd.optim import FusedAdam
    from multiposenet.pytorch_amd.replay import ReplayedTrainStep
    from multiposenet.pytorch_amd.training.batch_processor import batch_processor, train_step
    from test_model_gpu import get_model

    class _State(object):
        pass
    S = 128
    da = DeviceAugmenter(S, 4)
    idx = [0, 2]
    img, heat, hm, _ = da([_sample(i, CASES[i]) for i in idx], dice=np.stack([CASES[i]["dice"] for i in idx]))
    assert tuple(img.shape) == (2, 3, S, S) and tuple(heat.shape) == tuple(hm.shape) == (2, 18, S // 4, S // 4)
    for x in (img, heat, hm):
        assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()
    model = get_model(50, torch.bfloat16)
    for p in model.prn.parameters():
        p.requires_grad = False
    model.train()
    st = _State(); st.model = model; st.params = _State(); st.params.subnet_name = 'keypoint_subnet'; st.params.gpus = [0]
    inputs, gts, _ = batch_processor(st, (img, heat, hm))
    assert inputs[0][0].data_ptr() == img.data_ptr() and gts[1].data_ptr() == heat.data_ptr() and gts[2].data_ptr() == hm.data_ptr()
    opt = FusedAdam(model, lr=1e-4)
    loss, _ = train_step(model, opt, inputs, gts)
    assert np.isfinite(float(loss.detach())) and float(loss.detach()) > 0
    step = ReplayedTrainStep(model, opt)
    loss2, _ = step(inputs, gts)
    torch.cuda.synchronize()
    assert np.isfinite(float(loss2)) and float(loss2) > 0


def test_bad_inputs_raise():
    from multiposenet.pytorch_amd._lib import MpnError
    from multiposenet.pytorch_amd.datasets.augment import DeviceAugmenter
    da = DeviceAugmenter(64, 4)
    good = _sample(0, CASES[0])
    d = CASES[0]["dice"][None]
    da([good], dice=d)
    bad = [dict(good, img=good["img"].float()),                                      # not uint8
           dict(good, img=good["img"].permute(1, 0, 2)),                             # not contiguous
           dict(good, img=good["img"][:, :, :2].contiguous()),                       # not 3 channels
           dict(good, img=good["img"][:, :, 0].contiguous()),                        # not 3-dimensional
           dict(good, img=good["img"].cuda()),                                       # CPU tensors in
           dict(good, img=good["img"].numpy()),                                      # not a tensor
           dict(good, mask_miss=good["mask_miss"][:-1].contiguous()),                # mask of another size
           dict(good, mask_miss=good["mask_miss"].to(torch.int16)),
           dict(good, joint_self=np.zeros((16, 3))),
           dict(good, objpos=(-5000.0, 10.0))]                                       # the reference's slices would wrap
    for s in bad:
        with pytest.raises(MpnError):
            da([s], dice=d)
    with pytest.raises(MpnError):
        da([good, dict(good, mask_miss=None)], dice=np.concatenate([d, d]))          # mixed batch
    with pytest.raises(MpnError):
        da([good], dice=np.zeros((1, 5)))
    with pytest.raises(MpnError):
        da([], dice=np.zeros((0, 6)))
    with pytest.raises(MpnError):
        DeviceAugmenter(0, 4)
