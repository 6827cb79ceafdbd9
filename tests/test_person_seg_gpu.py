"""GPU tests of the person-segmentation target ``mask_all``: mpn_segm_person_masks (csrc/segm.hip's compose kernel in its
two-plane instantiation) and mpn_augment_plane (csrc/augment.hip's mask kernel with one channel and an explicit outside value),
through datasets/segm.py and ``DeviceAugmenter(mask_all=True)``.

MASKS: byte for byte against the sequential restatement tests/person_seg_ref.py on its committed inputs (which
tests/test_person_seg_cpu.py shows to reject four modelled misreadings), and the ``mask_miss`` plane byte for byte against
mpn_segm_mask_miss on the same annotations.  Sizes as in tests/test_mask_miss_gpu.py: below, on and beyond one word, two words,
one 512-row tile, one and two 64-column tiles, and widths whose rows lie on 4-byte boundaries (the four-bytes-per-lane store path).

WARP: on the recorded geometries of tests/golden/g17_augment.npz.  Fed the same source, the plane equals channel 0 of
mpn_augment_mask bit for bit wherever that kernel samples inside, and is exactly 0.0 where it is outside; against the float64
restatement (person_seg_ref.plane_ref = augment_ref.mask_ref with border 0) it stays within augment_ref's own derived bound
C_SUM_MASK u mag + W_ABS u wabs, which is 0 outside.
"""
import numpy as np
import pytest
import torch

import augment_bbox_ref as br
import augment_ref as ar
import mask_miss_ref as mr
import person_seg_ref as pr

pytestmark = pytest.mark.gpu

CASES, INP, STRIDE = ar.golden_cases()
GRID = INP // STRIDE


def _differ(got, want):
    return np.argwhere(got != want)


# ---- masks -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("h,w", pr.GPU_SIZES + [(37, 64), (70, 68), (130, 132)])
def test_both_planes_equal_the_restatement_byte_for_byte(h, w):
    from multiposenet.pytorch_amd.datasets import segm
    anns, _, want_miss, want_all = pr.case(h, w)
    miss, every, offsets = segm.person_masks_batch([anns], [(h, w)])
    only_miss = segm.mask_miss_batch([anns], [(h, w)])[0]
    assert offsets == [0] and miss.is_cuda and every.is_cuda and miss.dtype == every.dtype == torch.uint8
    assert miss.data_ptr() != every.data_ptr() and miss.numel() == every.numel() >= h * w
    got_miss, got_all = (t[:h * w].view(h, w).cpu().numpy() for t in (miss, every))
    for name, got, want in (("mask_miss", got_miss, want_miss), ("mask_all", got_all, want_all)):
        diff = _differ(got, want)
        print("%d x %d %s: %d cells are 255, %d differ" % (h, w, name, int((want == 255).sum()), diff.shape[0]))
        assert diff.shape[0] == 0, "%s differs at (y, x) %s" % (name, diff[:8].tolist())
        assert set(np.unique(want).tolist()) == {0, 255}
    assert np.array_equal(got_miss, only_miss[:h * w].view(h, w).cpu().numpy())          # the one-plane entry point's bytes
    one = segm.mask_all_from_annotations(anns, h, w)
    assert tuple(one.shape) == (h, w) and np.array_equal(one.cpu().numpy(), want_all)


def test_no_annotation_and_single_kinds():
    from multiposenet.pytorch_amd.datasets import segm
    h, w = 37, 53
    miss, every, _ = segm.person_masks_batch([[]], [(h, w)])
    assert bool((miss[:h * w] == 255).all()) and bool((every[:h * w] == 0).all())
    anns, masks, _, _ = pr.case(h, w)
    for i in (0, 1, 4):                                                  # a polygon, overlapping parts, an RLE: alone, as every kind
        for kind in (pr.K, pr.N, pr.C):
            ann = mr.annotation(anns[i]["segmentation"], kind)
            miss, every, _ = segm.person_masks_batch([[ann]], [(h, w)])
            assert np.array_equal(every[:h * w].view(h, w).cpu().numpy(), masks[i] * 255), (i, kind)
            assert np.array_equal(miss[:h * w].view(h, w).cpu().numpy(), mr.compose([masks[i]], [kind])), (i, kind)


def test_batch_of_three_sizes_offsets_and_determinism():
    from multiposenet.pytorch_amd.datasets import segm
    from multiposenet.pytorch_amd.datasets.augment import _aligned_offsets
    order = [(130, 70), (5, 6), (520, 131)]
    lists = [pr.case(h, w)[0] for h, w in order]
    a = segm.person_masks_batch(lists, order)
    b = segm.person_masks_batch(lists, order)
    one = segm.mask_miss_batch(lists, order)
    torch.cuda.synchronize()
    assert a[2] == b[2] == one[1] == _aligned_offsets([h * w for h, w in order])[0]
    for (h, w), off in zip(order, a[2]):
        _, _, want_miss, want_all = pr.case(h, w)
        for got, again, want in ((a[0], b[0], want_miss), (a[1], b[1], want_all)):
            g = got[off: off + h * w].view(h, w).cpu().numpy()
            diff = _differ(g, want)
            assert diff.shape[0] == 0, "%d x %d differs at (y, x) %s" % (h, w, diff[:8].tolist())
            assert np.array_equal(g, again[off: off + h * w].view(h, w).cpu().numpy())
        assert torch.equal(a[0][off: off + h * w], one[0][off: off + h * w])
    # offsets of the caller's, out of order, one of them on no 4-byte boundary (the byte store path)
    mine = [70000, 3, 100000]
    miss, every, offs = segm.person_masks_batch(lists, order, offsets=mine)
    assert offs == mine
    for (h, w), off in zip(order, mine):
        assert np.array_equal(miss[off: off + h * w].view(h, w).cpu().numpy(), pr.case(h, w)[2])
        assert np.array_equal(every[off: off + h * w].view(h, w).cpu().numpy(), pr.case(h, w)[3])


# ---- warp ------------------------------------------------------------------------------------------------------------------------------

def _golden_sample(i, c, **planes):
    img, _ = ar.synth_sources(40 + i, int(c["hw"][0]), int(c["hw"][1]))
    s = {"img": torch.from_numpy(img), "objpos": c["objpos_in"], "scale_provided": float(c["scale_provided"]),
         "joint_self": c["joint_self_in"], "joint_others": c["joint_others_in"], "objpos_other": c["objpos_other_in"]}
    s.update(planes)
    return s


def _ref_geo(c):
    o = (int(c["center"][0]) + INP // 2 - INP, int(c["center"][1]) + INP // 2 - INP)
    return ar.geometry(c["M"], c["scale"], c["stage_shapes"][0][:2], c["stage_shapes"][1][:2], o, int(c["flip"]))


def _outside(c, h, w):
    """Cells mpn_augment_mask does not sample: a constant source has no tap exactly there."""
    return ar.mask_ref(np.full((h, w), 7, dtype=np.uint8), _ref_geo(c), GRID, GRID, STRIDE, INP)[2] == 0


def test_golden_geometries_include_a_flip_and_a_crop_that_leaves_the_image():
    flips = [int(c["flip"]) for c in CASES]
    leaves = [float(_outside(c, int(c["hw"][0]), int(c["hw"][1])).mean()) for c in CASES]
    print("flip %s, outside fraction %s" % (flips, ["%.2f" % v for v in leaves]))
    assert 1 in flips and 0 in flips and max(leaves) > 0.1


@pytest.mark.parametrize("i", range(len(CASES)))
def test_plane_kernel_on_the_golden_geometries(i):
    from multiposenet.pytorch_amd.datasets.augment import DeviceAugmenter
    c = CASES[i]
    h, w = int(c["hw"][0]), int(c["hw"][1])
    src = ar.synth_sources(40 + i, h, w)[1]                              # one uint8 plane, fed to both kernels
    da = DeviceAugmenter(INP, STRIDE, ar.case_params(c), mask_all=True)
    plane = torch.from_numpy(src)
    img, heat, hm, ma, meta = da([_golden_sample(i, c, mask_miss=plane, mask_all=plane.clone())], dice=c["dice"][None])
    torch.cuda.synchronize()
    assert tuple(hm.shape) == (1, 18, GRID, GRID) and tuple(ma.shape) == (1, 1, GRID, GRID)
    assert ma.dtype == torch.float32 and ma.is_contiguous() and ma.is_cuda
    got, ch0 = ma[0, 0].cpu().numpy(), hm[0, 0].cpu().numpy()
    outside = _outside(c, h, w)
    assert np.array_equal(got[~outside].view(np.uint32), ch0[~outside].view(np.uint32))      # the same sample, bit for bit
    assert np.all(got[outside].view(np.uint32) == 0) and np.all(ch0[outside] == np.float32(1.0))
    ref, mag, wabs = pr.plane_ref(src, _ref_geo(c), GRID, GRID, STRIDE, INP, border=0.0)
    r = ar.ratio(got.astype(np.float64), ref, mag, wabs, ar.C_SUM_MASK)
    print("plane case %d: flip %d, outside %.2f, worst err/bound %.4f" % (i, int(c["flip"]), outside.mean(), r.max()))
    assert r.max() <= 1.0, (np.unravel_index(int(np.argmax(r)), r.shape), r.max())
    assert got.min() >= 0.0 and got.max() <= 1.0


def test_plane_kernel_ragged_grid_batch_of_two_and_other_outside_values():
    """Called directly at a grid of 3 x 87 = 261 cells (one full workgroup plus five lanes), two samples per launch, one flipped;
    the outside value is the caller's: 255 reproduces mpn_augment_mask's channel 0 everywhere."""
    from multiposenet.pytorch_amd.datasets import augment as aug
    pair = [next(i for i, c in enumerate(CASES) if int(c["flip"]) == f) for f in (0, 1)]
    GH, GW = 3, 87
    srcs = [ar.synth_sources(40 + i, int(CASES[i]["hw"][0]), int(CASES[i]["hw"][1]))[1] for i in pair]
    moff = [0, (srcs[0].size + 15) // 16 * 16]
    buf = np.zeros(moff[1] + srcs[1].size, dtype=np.uint8)
    rows, geos = [], []
    for b, i in enumerate(pair):
        c, (H, W) = CASES[i], srcs[b].shape
        buf[moff[b]: moff[b] + srcs[b].size] = srcs[b].reshape(-1)
        # the window hangs over the crop's left edge, so part of it is outside
        o = (int(c["center"][0]) + INP // 2 - INP - (GW * STRIDE) // 2, int(c["center"][1]) + INP // 2 - INP + (INP - GH * STRIDE) // 2)
        g = ar.geometry(c["M"], c["scale"], c["stage_shapes"][0][:2], c["stage_shapes"][1][:2], o, int(c["flip"]))
        geos.append(g)
        rows.append(aug.table_row(g, H, W, 0, W * 3, moff[b], W))
    d_buf, d_tab = torch.from_numpy(buf).cuda(), torch.from_numpy(np.stack(rows)).cuda()
    hm = aug.augment_mask(d_buf, d_tab, GH, GW, STRIDE, GW * STRIDE)
    p0 = aug.augment_plane(d_buf, d_tab, GH, GW, STRIDE, GW * STRIDE, 0.0)
    p255 = aug.augment_plane(d_buf, d_tab, GH, GW, STRIDE, GW * STRIDE, 255.0)
    p51 = aug.augment_plane(d_buf, d_tab, GH, GW, STRIDE, GW * STRIDE, 51.0)
    torch.cuda.synchronize()
    assert tuple(p0.shape) == (2, 1, GH, GW) and torch.equal(p255[:, 0], hm[:, 0])
    seen = inside = 0
    for b in range(2):
        ref, mag, wabs = pr.plane_ref(srcs[b], geos[b], GH, GW, STRIDE, GW * STRIDE, border=0.0)
        outside = pr.plane_ref(np.full_like(srcs[b], 7), geos[b], GH, GW, STRIDE, GW * STRIDE)[2] == 0
        seen += int(outside.sum())
        got = p0[b, 0].cpu().numpy()
        inside += int((~outside).sum())
        r = ar.ratio(got.astype(np.float64), ref, mag, wabs, ar.C_SUM_MASK)
        assert r.max() <= 1.0, (b, r.max())
        assert np.all(got[outside] == 0.0) and np.all(p51[b, 0].cpu().numpy()[outside] == np.float32(51.0) / np.float32(255.0))
        assert np.array_equal(got[~outside], hm[b, 0].cpu().numpy()[~outside])
    assert seen > 0 and inside > 0                                       # the window shows both


# ---- the augmenter ---------------------------------------------------------------------------------------------------------------------

def _samples():
    """Two samples of different sizes with their person annotations; the same two with both planes from the restatement; dice."""
    rs = np.random.RandomState(7)
    on_anns, on_plane = [], []
    for b, (h, w) in enumerate([(130, 70), (37, 53)]):
        anns, _, miss, every = pr.case(h, w)
        j = np.zeros((17, 3))
        j[:, 0], j[:, 1], j[:, 2] = rs.uniform(0, w, 17), rs.uniform(0, h, 17), rs.choice([0.0, 1.0, 2.0], 17)
        base = {"img": torch.from_numpy(br.synth_image(40 + b, h, w)), "objpos": (0.45 * w, 0.5 * h), "scale_provided": 0.6 if b else 1.2,
                "joint_self": j}
        on_anns.append(dict(base, person_anns=anns))
        on_plane.append(dict(base, mask_miss=torch.from_numpy(miss.copy()), mask_all=torch.from_numpy(every.copy())))
    dice = np.array([[0.2, 0.9, 0.8, 0.4, 0.6, 0.9], [0.5, 0.3, 0.1, 0.7, 0.2, 0.1]])
    return on_anns, on_plane, dice


def test_augmenter_on_person_anns_equals_itself_on_planes_and_default_is_unchanged():
    from multiposenet.pytorch_amd.datasets.augment import DeviceAugmenter
    import segm_cases as sc
    on_anns, on_plane, dice = _samples()
    da = DeviceAugmenter(64, 4, dict(center_perterb_max=10), mask_all=True)
    plain = DeviceAugmenter(64, 4, dict(center_perterb_max=10))
    a, p = da(on_anns, dice=dice), da(on_plane, dice=dice)
    assert len(a) == len(p) == 5 and tuple(a[3].shape) == (2, 1, 16, 16) and a[3].dtype == torch.float32
    for x, y in zip(a[:4], p[:4]):
        assert torch.equal(x, y)
    assert float(a[3].min()) == 0.0 and float(a[3].max()) > 0.5                          # somebody stands in the crop, and not everywhere
    # mask_all=False: four values, the same bytes as with it, and as a second call with the same dice
    q, q2 = plain(on_anns, dice=dice), plain(on_anns, dice=dice)
    assert len(q) == 4 and q[2] is not None
    for x, y, z in zip(q[:3], q2[:3], a[:3]):
        assert torch.equal(x, y) and torch.equal(x, z)
    q = plain(on_plane, dice=dice)                                                       # a mask_all plane nobody asked for is ignored
    assert len(q) == 4 and torch.equal(q[2], a[2])
    # with the box path's inputs next to it
    for s in on_anns + on_plane:
        h, w = s["img"].shape[:2]
        s["segmentations"], s["iscrowd"] = sc.segmentations(h, w)[0][:4], [0, 0, 1, 0]
    a, p, q = da.call_with_boxes(on_anns, dice=dice), da.call_with_boxes(on_plane, dice=dice), plain.call_with_boxes(on_anns, dice=dice)
    assert len(a) == len(p) == 6 and len(q) == 5
    for x, y in zip(a[:5], p[:5]):
        assert torch.equal(x, y)
    assert tuple(a[3].shape) == (2, 1, 16, 16) and tuple(a[4].shape) == (2, 3, 5)
    assert torch.equal(q[3], a[4]) and torch.equal(q[2], a[2])


# ---- the loss kernels, API form --------------------------------------------------------------------------------------------------------
# Values and gradients against the float64 reference of tests/person_seg_ref.py under the bounds derived there (loss_ref's own
# derivation with one operand less; nothing fitted); channels 0..17 of every gradient bit-equal to mpn_mse_heatmap_backward's and
# out[0..7] bit-equal to mpn_mse_heatmap_forward's.  Shapes: loss_ref.MSE_CASES (1 px, the last partial chunk, the second chunk,
# 257 chunks = 15 seg chunks) and 2 x 10 x 14, whose sides are no multiple of 8; 19- and 18-channel finals; pixel strides 19 and 32.

import loss_ref as lr

API_CASES = [(name, f19, None) for name in lr.MSE_CASES for f19 in (False, True)] + [("2x10x14 sides no multiple of 8", True, (2, 10, 14, [True] * 5)),
                                                                                      ("2x10x14 sides no multiple of 8", False, (2, 10, 14, [True] * 5))]


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


@pytest.mark.parametrize("name,final19,extra", API_CASES)
def test_seg_loss_forward_backward_api_form(name, final19, extra):
    from multiposenet.pytorch_amd.network import losses
    case = pr.seg_case(name, final19, extra)
    ref = pr.seg_ref(case)
    store = [_dev(s) for s in case["store"]]
    pm = [s[..., :C] for s, C in zip(store, case["C"])]
    assert [p.stride(2) for p in pm] == list(lr.MSE_STRIDE)                         # dense and 32-strided storage in one call
    heat, wgt, mask = _dev(case["gt"]), _dev(case["w"]), _dev(case["mask"])
    gs = torch.tensor([float(case["gs"])], dtype=torch.float32, device="cuda")
    out = losses.mse_seg_forward_raw(pm, heat, wgt, mask)
    grads = losses.mse_seg_backward_raw(pm, heat, wgt, mask, gs, case["need"])
    out8 = losses.mse_forward_raw(pm, heat, wgt)
    grads8 = losses.mse_backward_raw(pm, heat, wgt, gs, case["need"])
    torch.cuda.synchronize()
    npix = case["B"] * case["H"] * case["W"]
    route = "%d px, final %d channels" % (npix, case["C"][4])
    o = out.cpu().numpy()
    print("%s %s: out %s" % (name, route, o[:17].tolist()))
    assert o.shape == (20,) and np.array_equal(o[:8].view(np.uint32), out8.cpu().numpy().view(np.uint32)) and not o[17:].any()
    pr.check_seg_out("seg " + name, o, ref, lr.MSE_FWD_LEVELS, route)
    host = [None if g is None else g.permute(0, 2, 3, 1).cpu().numpy() for g in grads]
    pr.check_seg_grads("seg " + name, host, ref, case["need"], route)
    for j in range(5):
        if not case["need"][j]:
            assert grads[j] is None and grads8[j] is None
            continue
        assert tuple(grads[j].shape) == tuple(grads8[j].shape) == (case["B"], case["C"][j], case["H"], case["W"])
        assert torch.equal(grads[j][:, :18], grads8[j][:, :18]), "level %d: channels 0..17 differ from mpn_mse_heatmap_backward" % j
        if case["C"][j] >= 19:
            assert bool((grads8[j][:, 18] == 0).all()) and bool((grads[j][:, 18] != 0).any())


def test_build_keypoint_loss_with_mask_all_log_keys_and_autograd():
    from multiposenet.pytorch_amd._lib import MpnError
    from multiposenet.pytorch_amd.network import losses
    from multiposenet.pytorch_amd.network.posenet import poseNet
    g = torch.Generator().manual_seed(5)
    B, H, W = 2, 10, 14
    heat, wgt = torch.rand((B, 18, H, W), generator=g).cuda(), (torch.rand((B, 18, H, W), generator=g) > 0.1).float().cuda()
    mask = (torch.rand((B, 1, H, W), generator=g) > 0.5).float().cuda()
    heads = ['heatmap_loss_k2', 'seg_loss_k2', 'heatmap_loss_k3', 'seg_loss_k3', 'heatmap_loss_k4', 'seg_loss_k4', 'heatmap_loss_k5',
             'seg_loss_k5', 'heatmap_loss']
    for cfin in (18, 19):
        preds = [torch.randn((B, 19 if j < 4 else cfin, H, W), generator=g).cuda().requires_grad_(True) for j in range(5)]
        total, log = poseNet.build_loss(preds, 'keypoint_subnet', heat, wgt, mask)
        want = heads + (['seg_loss'] if cfin == 19 else []) + ['max_ht', 'min_ht'] + (['max_mask', 'min_mask'] if cfin == 19 else [])
        assert list(log.keys()) == want and all(type(v) is float for v in log.values())
        total.backward()
        plain, plog = poseNet.build_loss([p.detach().requires_grad_(True) for p in preds], 'keypoint_subnet', heat, wgt)
        assert list(plog.keys()) == [k for k in heads if k.startswith('heat')] + ['max_ht', 'min_ht']
        assert all(plog[k] == log[k] for k in plog)
        # float64 autograd on the same tensors
        p64 = [p.detach().double().requires_grad_(True) for p in preds]
        t64 = sum(((p[:, :18] * wgt.double() - wgt.double() * heat.double()) ** 2).mean() for p in p64)
        t64 = t64 + sum(((p[:, 18:19] - mask.double()) ** 2).mean() / 100.0 for p in p64 if p.shape[1] >= 19)
        t64.backward()
        assert abs(float(total) - float(t64)) <= 1e-5 * abs(float(t64))
        seg_sum = sum(log[k] for k in log if k.startswith('seg'))
        assert abs(float(total) - (float(plain) + seg_sum)) <= 1e-6 * abs(float(t64))
        for p, q in zip(preds, p64):
            assert p.grad.shape == q.grad.shape
            assert float((p.grad.double() - q.grad).abs().max()) <= 1e-6 * float(q.grad.abs().max())
            if p.shape[1] >= 19:
                assert float(p.grad[:, 18].abs().max()) > 0
        if cfin == 19:
            assert log['max_mask'] == float(preds[4][:, 18].max()) and log['min_mask'] == float(preds[4][:, 18].min())
    with pytest.raises(MpnError):
        poseNet.build_loss(preds, 'keypoint_subnet', heat, wgt, mask.cpu())
    with pytest.raises(MpnError):
        poseNet.build_loss(preds, 'keypoint_subnet', heat, wgt, mask[:, 0])


# ---- the model: R50 at 64 x 64, B = 2, eager steps -------------------------------------------------------------------------------------

def _fresh_model(person_seg, dtype):
    from multiposenet.pytorch_amd.network.posenet import poseNet
    from test_model_gpu import load_he
    m = poseNet(50, compute_dtype=dtype, person_seg=person_seg).cuda()
    load_he(m)
    for p in m.parameters():
        p.requires_grad = True
    return m


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("person_seg", [False, True], ids=["plain", "person_seg"])
def test_model_trains_channel_18_from_mask_all(person_seg, dtype):
    from multiposenet.pytorch_amd import synthetic as weightgen
    from multiposenet.pytorch_amd.network import losses
    from multiposenet.pytorch_amd.network.posenet import poseNet
    from test_model_gpu import t
    m = _fresh_model(person_seg, dtype)
    m.train()
    B, S = 2, 64
    img = t(weightgen.gen_images(7, B, S, S)).cuda()
    heat, wgt = (t(a).cuda() for a in weightgen.gen_keypoint_gt(8, B, S // 4, S // 4))
    anno = t(weightgen.gen_boxes_gt(9, B, S)).cuda()
    mask = (torch.rand((B, 1, S // 4, S // 4), generator=torch.Generator().manual_seed(3)) > 0.6).float().cuda()
    bn_state = {k: v.clone() for k, v in m.state_dict().items() if "running_" in k or "num_batches" in k}
    heads = [m.convfin_k2, m.convfin_k3, m.convfin_k4, m.convfin_k5] + ([m.convfin] if person_seg else [])
    assert m.convfin.out_channels == (19 if person_seg else 18) and m.person_seg == person_seg

    def step(subnet, mask_all):
        m.load_state_dict(bn_state, strict=False)
        m._arena.ensure_grads()
        m._arena.grad_flat.zero_()
        if subnet == "train_both":
            pred, (ks, ds) = m([img, subnet])
            gts = [heat, wgt, anno] + ([mask_all] if mask_all is not None else [])
            loss, log = poseNet.build_loss((ks, ds), subnet, *gts)
        else:
            pred, ks = m([img, subnet])
            gts = [heat, wgt] + ([mask_all] if mask_all is not None else [])
            loss, log = poseNet.build_loss(ks, subnet, *gts)
        assert pred.shape == (B, 19 if person_seg else 18, S // 4, S // 4)
        loss.backward()
        torch.cuda.synchronize()
        return loss.detach().clone(), m._arena.grad_flat.clone(), log, [k.detach() for k in ks], [h.weight.grad.clone() for h in heads]

    for subnet in ("keypoint_subnet", "train_both"):
        l0, g0, log0, _, hg0 = step(subnet, None)
        l1, g1, log1, ks, hg1 = step(subnet, mask)
        assert torch.isfinite(g1).all() and 'seg_loss_k2' in log1 and 'seg_loss_k2' not in log0
        assert ('seg_loss' in log1) == person_seg and ('max_mask' in log1) == person_seg
        for a, b in zip(hg0, hg1):
            assert a.shape[0] == 19 and bool((a[18] == 0).all()), "row 18 has a gradient without mask_all"
            assert float(b[18].abs().max()) > 0, "row 18 has no gradient with mask_all"
        if not person_seg:
            assert m.convfin.weight.grad.shape[0] == 18
        if dtype == torch.float32:
            # the total and the seg values against float64, on the model's own exported predictions
            case = dict(B=B, H=S // 4, W=S // 4, store=[k.permute(0, 2, 3, 1).contiguous().cpu().numpy() for k in ks],
                        gt=heat.permute(0, 2, 3, 1).contiguous().cpu().numpy(), w=wgt.permute(0, 2, 3, 1).contiguous().cpu().numpy(),
                        mask=mask[:, 0].cpu().numpy(), gs=np.float32(1.0), C=tuple(int(k.shape[1]) for k in ks))
            ref = pr.seg_ref(case)
            pm = [losses._pixel_major(k) for k in ks]
            out = losses.mse_seg_forward_raw(pm, losses.ops.nchw_to_nhwc_f32(heat), losses.ops.nchw_to_nhwc_f32(wgt), mask.contiguous())
            o = out.cpu().numpy()
            for k, i in (('seg_loss_k2', 8), ('seg_loss_k3', 9), ('seg_loss_k4', 10), ('seg_loss_k5', 11), ('heatmap_loss', 4)):
                assert np.float32(log1[k]) == o[i], k
            lr.chk("model %s seg values" % subnet, o[8:13], np.array(ref["seg"]), [],
                   extra_abs=np.array([lr.mse_loss_bound(*b, levels=lr.MSE_FWD_LEVELS) if b[1] else 0.0 for b in ref["seg_b"]]), names="j")
            kp_total = o[16]
            assert abs(kp_total - ref["total"]) <= 1e-5 * abs(ref["total"])
            if subnet == "keypoint_subnet":
                assert np.float32(float(l1)) == kp_total

    if dtype == torch.float32:
        # P[:, 18] == M == 0 through zero row-18 weights: the step with mask_all is the step without it
        for h in heads:
            h.weight.data[18].zero_()
            h.bias.data[18].zero_()
        zero = torch.zeros_like(mask)
        for subnet in ("keypoint_subnet", "train_both"):
            l0, g0, _, ks, _ = step(subnet, None)
            l1, g1, log1, _, _ = step(subnet, zero)
            assert all(bool((k[:, 18] == 0).all()) for k in ks if k.shape[1] >= 19)
            assert torch.equal(l0, l1) and torch.equal(g0, g1), "%s: a zero seg term changed the step" % subnet
            assert all(log1[k] == 0.0 for k in log1 if k.startswith('seg'))


# ---- the Tester with a person_seg model ---------------------------------------------------------------------------------------------------

def test_tester_results_of_a_person_seg_model_equal_the_plain_model_s():
    """One synthetic 96 x 128 image (tests/tta_standin.synth_image), R50 fp32 with seeded weights (the rig of
    tests/test_tta_fused_gpu.py: detector bias shifted so that people are found, seeded PRN weights); the person_seg model has the
    plain model's parameters, its convfin rows 0..17 included, and a random row 18."""
    import tta_standin
    from multiposenet.pytorch_amd import synthetic as weightgen
    from multiposenet.pytorch_amd.evaluate import tester as T
    from test_model_gpu import t
    plain, seg = _fresh_model(False, torch.float32), _fresh_model(True, torch.float32)
    sd = weightgen.gen_state_dict({k: tuple(v.shape) for k, v in plain.state_dict().items() if k.startswith("prn.")}, seed=3, flavour="he")
    plain.load_state_dict({k: t(v) for k, v in sd.items()}, strict=False)
    S = 128
    plain.eval()
    with torch.no_grad():
        _, (cls, _, _) = plain([torch.zeros(2, 3, S, S, device="cuda").normal_(), "detection_subnet"])
        s_ = cls.float().flatten().clamp(1e-6, 1 - 1e-6)
        q = torch.quantile(s_, 1.0 - 40.0 / float(cls.shape[1]))
        plain.classificationModel.output.bias.data += float(-torch.log(q / (1 - q)))
    state = {k: v.clone() for k, v in plain.state_dict().items() if not k.startswith("convfin.")}
    seg.load_state_dict(state, strict=False)
    seg.convfin.weight.data[:18].copy_(plain.convfin.weight.data)
    seg.convfin.bias.data[:18].copy_(plain.convfin.bias.data)
    seg.convfin.weight.data[18].normal_(std=0.05)
    seg.convfin.bias.data[18] = 0.3
    seg.eval()
    img = tta_standin.synth_image(5, 96, 128)
    x = torch.randn((1, 3, S, S), generator=torch.Generator().manual_seed(1)).cuda()
    with torch.no_grad():
        a, b = plain([x, 'keypoint_subnet'])[0], seg([x, 'keypoint_subnet'])[0]
        assert a.shape[1] == 18 and b.shape[1] == 19 and torch.equal(a, b[:, :18]) and float(b[:, 18].abs().max()) > 0
        hb, keep = seg.forward_heat(x)
        assert hb.shape[1] == 19 and torch.equal(hb, b)
        del keep
    results = []
    for m in (plain, seg):
        tp = T.TestParams()
        tp.ckpt, tp.inp_size = None, S
        te = T.Tester(m, tp)
        results.append((te.infer_image(img, "a.jpg", 7), te.infer_images_batched([img], ["a.jpg"], [7])[0],
                        te.infer_image_multiscale_fused(img, "a.jpg", 7), te.infer_image_multiscale(img, "a.jpg", 7)))
    for path, (ra, rb) in zip(("infer_image", "infer_images_batched", "fused multi-scale", "multi-scale"), zip(*results)):
        assert ra == rb, path
    assert sum(len(r) for r in results[0]) >= 1, "nobody is found: the comparison would be empty"


# ---- the recorded step with mask_all ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("person_seg", [False, True], ids=["plain", "person_seg"])
def test_recorded_step_with_mask_all_equals_the_eager_step_bit_for_bit(person_seg, dtype):
    """Three optimizer steps (eager body, recording, one replay) of ReplayedTrainStep against three batch_processor.train_step
    calls from the same start: parameters bit-identical, with the one-pass seg kernel (the default: 16 x 16 maps fit it) and with the
    forward / backward pair (fused_mse=False).  Log keys equal; log values equal with the pair and within the two summation trees'
    bound with the one-pass kernel.  The presence of mask_all is part of the recording's signature: the same stepper then runs a
    step without it."""
    import copy
    from collections import OrderedDict
    from multiposenet.pytorch_amd import synthetic as weightgen
    from multiposenet.pytorch_amd._lib import MpnError
    from multiposenet.pytorch_amd.network import losses
    from multiposenet.pytorch_amd.optim import FusedAdam
    from multiposenet.pytorch_amd.replay import ReplayedTrainStep
    from multiposenet.pytorch_amd.training.batch_processor import train_step
    from test_model_gpu import t
    m = _fresh_model(person_seg, dtype)
    for p in m.prn.parameters():
        p.requires_grad = False
    m.train()
    B, S = 2, 64
    img = t(weightgen.gen_images(7, B, S, S)).cuda()
    heat, wgt = (t(a).cuda() for a in weightgen.gen_keypoint_gt(8, B, S // 4, S // 4))
    anno = t(weightgen.gen_boxes_gt(9, B, S)).cuda()
    mask = (torch.rand((B, 1, S // 4, S // 4), generator=torch.Generator().manual_seed(3)) > 0.6).float().cuda()
    start = copy.deepcopy(m.state_dict())
    for subnet in ("keypoint_subnet", "train_both"):
        inputs = [[img, subnet]]
        gts = [subnet, heat, wgt] + ([anno] if subnet == "train_both" else []) + [mask]
        m.load_state_dict(start)
        opt = FusedAdam(m, lr=1e-3, weight_decay=1e-4)
        def run(fn):
            """[(loss, log)] of three steps, read right after each: the recorded step hands out its own log vector"""
            out = []
            for _ in range(3):
                loss, log = fn(inputs, gts)
                out.append((float(loss), OrderedDict((k, float(v)) for k, v in log.items())))
            return out
        eager = run(lambda i, g: train_step(m, opt, i, g))
        torch.cuda.synchronize()
        want = m._arena.flat.detach().clone()
        # sums of non-negative f32 squares in two summation trees (the API forward's and the one-pass kernel's): each is off the exact
        # sum by at most its levels * u relative (loss_ref), so the two differ by at most the sum of both, plus the final roundings
        rel = (lr.MSE_FWD_LEVELS + lr.MSE_TRAIN_LEVELS + 2) * lr.U
        for fused in (True, False):
            m.load_state_dict(start)
            opt = FusedAdam(m, lr=1e-3, weight_decay=1e-4)
            stepper = ReplayedTrainStep(m, opt, fused_mse=fused)
            calls = []
            real = losses.mse_seg_train_raw
            losses.mse_seg_train_raw = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
            try:
                rec = run(stepper)
            finally:
                losses.mse_seg_train_raw = real
            torch.cuda.synchronize()
            assert stepper.replays >= 1 and (len(calls) == 2) == fused, (fused, len(calls))    # the eager body and the recording
            assert torch.equal(m._arena.flat.detach(), want), "%s fused=%s: recorded and eager parameters differ" % (subnet, fused)
            for (le, loge), (lr_, logr) in zip(eager, rec):
                assert list(loge) == list(logr)
                for k in loge:
                    if fused and not k.startswith(("max_", "min_")):
                        assert abs(loge[k] - logr[k]) <= rel * max(abs(loge[k]), abs(logr[k])), (k, loge[k], logr[k])
                    else:
                        assert loge[k] == logr[k], (k, fused)
                assert abs(le - lr_) <= (0.0 if not fused else rel * max(abs(le), abs(lr_)))
                assert ('seg_loss' in logr) == person_seg and 'seg_loss_k5' in logr and ('max_mask' in logr) == person_seg
        # a step without mask_all on the same stepper: another signature, the existing path
        loss, log = stepper(inputs, gts[:-1])
        assert 'seg_loss_k2' not in log and np.isfinite(float(loss))
        with pytest.raises(MpnError):
            stepper(inputs, gts[:-1] + [mask[:, 0]])
        with pytest.raises(MpnError):
            stepper(inputs, gts[:-1] + [torch.zeros((B, 1, S // 4, S // 8), device="cuda")])


# ---- the loss kernels, one-pass form ---------------------------------------------------------------------------------------------------
# mpn_mse_heatmap_seg_train on loss_ref.TRAIN_CASES (one cell; nine cells = two blocks, the second ragged; two images with W != H) in
# f32, bf16 and f16, with a 19- and an 18-channel final.  Gradients: every stored element (all 32 lanes) bit-equal to the API
# backward (mpn_mse_heatmap_seg_backward on the exported, up-sampled predictions) followed by mpn_import_grad, channel 18
# included; lanes 0..17 and out[0..7] bit-equal to mpn_mse_heatmap_train's.  Values: under person_seg_ref's derived bounds with the
# one-pass summation tree (loss_ref.MSE_TRAIN_LEVELS).  Planted 1e3 in the padding lanes 19..31 of every level, and in lane 18 of an
# 18-channel final, reaches no output.

def _train_seg_case(name, final19):
    case = lr.train_case(name)
    B, H, W = case["B"], case["H"], case["W"]
    r = lr.rng(B * 77 + H + W + int(final19))
    lv = case["lv"]
    lv[0][..., 18] = r.standard_normal(lv[0].shape[:3]).astype(np.float32)         # a live value now, not loss_ref's planted one
    if final19:
        lv[4][..., 18] = r.standard_normal(lv[4].shape[:3]).astype(np.float32)
    for x in lv:
        x[..., 19:] = np.float32(lr.PLANT)
    m = (r.random_sample((B, 1, H, W)) < 0.4).astype(np.float32)
    soft = r.random_sample(m.shape) < 0.2
    m[soft] = r.random_sample(int(soft.sum())).astype(np.float32)
    case["mask"], case["C"] = m, (19, 19, 19, 19, 19 if final19 else 18)
    return case


@pytest.mark.parametrize("final19", [False, True], ids=["final18", "final19"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("name", list(lr.TRAIN_CASES))
def test_seg_loss_one_pass_form(name, dtype, final19):
    from multiposenet.pytorch_amd import ops
    from multiposenet.pytorch_amd.network import losses
    case = _train_seg_case(name, final19)
    B, H, W = case["B"], case["H"], case["W"]
    levels = [ops.Act(_dev(x), C) for x, C in zip(case["lv"], case["C"])]
    heat, wgt, mask = _dev(case["heat"]), _dev(case["w"]), _dev(case["mask"])
    assert losses.mse_seg_train_supported(levels, heat, wgt, mask)
    gs = torch.tensor([float(case["gs"]), 0.0], dtype=torch.float32, device="cuda")
    out, grads = losses.mse_seg_train_raw(levels, heat, wgt, mask, gs, dtype)
    # the heat-only one-pass launch on the same operands
    out8, grads8 = losses.mse_train_raw(levels, heat, wgt, gs, dtype)
    # the API chain: export (nearest up-sampling), the seg-aware backward, import
    pm = [losses._pixel_major(ops.export_f32(a, a.C, H, W)) for a in levels]
    api = losses.mse_seg_backward_raw(pm, ops.nchw_to_nhwc_f32(heat), ops.nchw_to_nhwc_f32(wgt), mask, gs, [True] * 5)
    want = [ops.import_grad(g, a, dtype) for g, a in zip(api, levels)]
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert o.shape == (20,) and np.array_equal(o[:8].view(np.uint32), out8.cpu().numpy().view(np.uint32)) and not o[17:].any()
    bits = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}[dtype]
    for j in range(5):
        g, w, g8 = grads[j].t, want[j].t, grads8[j].t
        assert g.dtype == dtype and g.shape == w.shape == levels[j].t.shape
        assert torch.equal(g.view(bits), w.view(bits)), "level %d: %d elements differ from backward + import_grad" % (j, int((g != w).sum()))
        assert torch.equal(g[..., :18].view(bits), g8[..., :18].view(bits)), "level %d: lanes 0..17 differ from mpn_mse_heatmap_train" % j
        assert bool((g[..., 19:] == 0).all()) and float(g.float().abs().max()) < lr.PLANT
        if case["C"][j] >= 19:
            assert bool((g[..., 18] != 0).any()) and bool((g8[..., 18] == 0).all())
        else:
            assert bool((g[..., 18] == 0).all())
    ref = pr.seg_ref(dict(lr.train_as_mse(case), C=case["C"], mask=case["mask"][:, 0]))
    w = pr.check_seg_out("one-pass seg " + name, o, ref, lr.MSE_TRAIN_LEVELS, route="%s final %d" % (str(dtype).split(".")[1], case["C"][4]))
    print("%s %s final %d: worst err/bound %.3f, seg %s" % (name, dtype, case["C"][4], w, o[8:14].tolist()))
    assert np.isfinite(o).all() and np.abs(o).max() < lr.PLANT
    assert not losses.mse_seg_train_supported(levels, heat, wgt, mask[:, 0]) and not losses.mse_seg_train_supported(levels, heat, wgt, mask.double())
