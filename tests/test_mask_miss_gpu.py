"""GPU tests of mask_miss built on the device from raw person annotations (csrc/segm.hip: the toggle launches and the compose
launch, through datasets/segm.py) and of DeviceAugmenter's ``person_anns`` input.

PARITY is byte for byte: the rule is integer-valued, so there is no tolerance anywhere in this file.  The truth is the sequential
restatement tests/mask_miss_ref.py over tests/segm_ref.py on the committed inputs (the seven instances of tests/segm_cases.py with
kinds N C C K C C N), computed once per size and shared; tests/test_mask_miss_cpu.py shows that those inputs reject eight
modelled misreadings of the rule at every size used here.  Sizes: the heights 5, 37, 64, 130, 513 and 520 fall below, on and
beyond one word, two words and one 512-row tile; the widths 6 .. 70 and 131 cross one and two 64-column tiles; at 520 x 131 an
instance rectangle straddles both tile boundaries.

The augmenter is compared with ITSELF on ``mask_miss`` planes built from the restatement, with the same dice.
"""
import ctypes

import numpy as np
import pytest
import torch

import augment_bbox_ref as br
import mask_miss_ref as mr
import segm_cases as sc

pytestmark = pytest.mark.gpu

K, N, C = mr.K, mr.N, mr.C


def _differ(got, want):
    return np.argwhere(got != want)


@pytest.mark.parametrize("h,w", mr.SIZES)
def test_mask_miss_equals_the_restatement_byte_for_byte(h, w):
    from multiposenet.pytorch_amd.datasets.segm import mask_miss_from_annotations
    anns, _, want = mr.case(h, w)
    got = mask_miss_from_annotations(anns, h, w)
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (h, w)
    got = got.cpu().numpy()
    diff = _differ(got, want)
    print("%d x %d: %d cells are 0, %d differ" % (h, w, int((want == 0).sum()), diff.shape[0]))
    assert diff.shape[0] == 0, "differs at (y, x) %s" % diff[:8].tolist()
    assert set(np.unique(want).tolist()) == {0, 255}


@pytest.mark.parametrize("h,w", [(37, 64), (70, 68), (130, 132)])
def test_widths_that_are_multiples_of_four(h, w):
    """None of the six sizes has rows on 4-byte boundaries; these have (the planes are stored four bytes per lane there), with the
    last 64-column tile full, 4 columns wide and absent."""
    from multiposenet.pytorch_amd.datasets.segm import mask_miss_from_annotations
    anns, _, want = mr.case(h, w)
    diff = _differ(mask_miss_from_annotations(anns, h, w).cpu().numpy(), want)
    assert diff.shape[0] == 0, "differs at (y, x) %s" % diff[:8].tolist()
    assert set(np.unique(want).tolist()) == {0, 255}


def test_520_by_131_has_a_rectangle_across_both_tile_boundaries():
    from multiposenet.pytorch_amd.datasets.segm import pack_mask_miss
    pack, _ = pack_mask_miss(mr.case(520, 131)[0], 520, 131)
    assert any(x0 < 64 < x0 + rw - 1 and y0 < 512 < y0 + rh - 1 for x0, y0, rw, rh in pack.rects())


@pytest.mark.parametrize("h,w", [(37, 53), (520, 131)])
def test_one_annotation_of_each_kind_alone(h, w):
    from multiposenet.pytorch_amd.datasets.segm import mask_miss_from_annotations
    anns, masks, _ = mr.case(h, w)
    for i in (0, 1, 3, 4, sc.EMPTY):                                    # star, overlapping parts, borders, RLE, the empty one
        for kind in (K, N, C):
            ann = mr.annotation(anns[i]["segmentation"], kind)
            want = mr.compose([masks[i]], [kind])
            got = mask_miss_from_annotations([ann], h, w).cpu().numpy()
            assert np.array_equal(got, want), (i, kind)
            assert (want == 255).all() == (kind == K or i == sc.EMPTY)    # K alone changes nothing; N and C alone take the mask out


def test_trailing_annotations_with_keypoints_change_nothing():
    """The packer drops a K after the image's last crowd; the kernel given the whole list computes the same bytes."""
    from multiposenet.pytorch_amd._lib import call
    from multiposenet.pytorch_amd import ops
    from multiposenet.pytorch_amd.datasets import segm
    h, w = 130, 70
    segms = sc.segmentations(h, w)[0]
    picks, kinds = [3, 0, 4, 1, 2, 0, 3], [K, N, C, K, N, K, K]
    anns = [mr.annotation(segms[i], k) for i, k in zip(picks, kinds)]
    want = mr.mask_miss(anns, h, w)
    dropped = segm.mask_miss_from_annotations(anns, h, w).cpu().numpy()
    assert segm.pack_mask_miss(anns, h, w)[0].n == 4 and np.array_equal(dropped, want)
    # the same list kept whole: packed without the dropping rule, through the same entry point
    pack = segm.pack_segmentations([a["segmentation"] for a in anns], h, w)
    code = {K: segm.KIND_KEYPOINTS, N: segm.KIND_NO_KEYPOINTS, C: segm.KIND_CROWD}
    kd = np.asarray([code[k] for k in kinds], dtype=np.int32)
    imgs = np.asarray([[h, w, 0, pack.n, 0, w]], dtype=np.int64)
    dev = torch.device("cuda", torch.cuda.current_device())
    (insts, parts, verts, vpart, estart, toggles, d_imgs, d_kd), _ = segm._upload(pack, dev, (imgs, kd))
    out = torch.empty(h * w, dtype=torch.uint8, device=dev)
    ws = torch.empty(int(call("mpn_segm_workspace_bytes", pack.words)), dtype=torch.uint8, device=dev)
    call("mpn_segm_mask_miss", ops.ptr(d_imgs), 1, ops.ptr(insts), ops.ptr(d_kd), pack.n, ops.ptr(parts), int(pack.parts.shape[0]),
         ops.ptr(verts), ops.ptr(vpart), ops.ptr(estart), int(pack.verts.shape[0]), int(pack.estart[-1]), ops.ptr(toggles),
         int(pack.toggles.shape[0]), w, h, ops.ptr(out), out.numel(), ops.ptr(ws), ws.numel(), ops.stream_ptr())
    assert np.array_equal(out.view(h, w).cpu().numpy(), want)


def test_mixed_batch_planes_offsets_and_determinism():
    from multiposenet.pytorch_amd.datasets import segm
    from multiposenet.pytorch_amd.datasets.augment import _aligned_offsets
    order = [(130, 70), (5, 6), (520, 131), (37, 53), (513, 66), (64, 65)]
    lists, wants = [], []
    for b, (h, w) in enumerate(order):
        anns, masks, want = mr.case(h, w)
        if b == 1:                                                       # no annotation: all 255
            anns, want = [], np.full((h, w), 255, dtype=np.uint8)
        elif b == 3:                                                     # only a crowd
            anns, want = [anns[4]], mr.compose([masks[4]], [C])
        lists.append(anns)
        wants.append(want)
    buf, offsets = segm.mask_miss_batch(lists, order)
    buf2, offsets2 = segm.mask_miss_batch(lists, order)
    torch.cuda.synchronize()
    assert offsets == offsets2 == _aligned_offsets([h * w for h, w in order])[0] and buf.dtype == torch.uint8 and buf.is_cuda
    a, b2 = buf.cpu().numpy(), buf2.cpu().numpy()
    for (h, w), off, want in zip(order, offsets, wants):
        assert off % 16 == 0
        got = a[off: off + h * w].reshape(h, w)
        diff = _differ(got, want)
        assert diff.shape[0] == 0, "%d x %d differs at (y, x) %s" % (h, w, diff[:8].tolist())
        assert np.array_equal(got, b2[off: off + h * w].reshape(h, w))
    assert (wants[1] == 255).all() and (wants[3] == 0).any()
    # offsets of the caller's, out of order and with gaps: every plane lies at its own
    mine = [70000, 3, 100000, 4096, 30000, 8192]                       # one of them on no 4-byte boundary
    buf3, offsets3 = segm.mask_miss_batch(lists, order, offsets=mine)
    c = buf3.cpu().numpy()
    assert offsets3 == mine
    for (h, w), off, want in zip(order, mine, wants):
        assert np.array_equal(c[off: off + h * w].reshape(h, w), want)


def _samples():
    """Two samples of different sizes with their person annotations, the same two with mask_miss from the restatement, dice."""
    rs = np.random.RandomState(7)
    on_anns, on_plane = [], []
    for b, (h, w) in enumerate([(130, 70), (37, 53)]):
        anns, _, want = mr.case(h, w)
        j = np.zeros((17, 3))
        j[:, 0], j[:, 1], j[:, 2] = rs.uniform(0, w, 17), rs.uniform(0, h, 17), rs.choice([0.0, 1.0, 2.0], 17)
        base = {"img": torch.from_numpy(br.synth_image(40 + b, h, w)), "objpos": (0.45 * w, 0.5 * h), "scale_provided": 0.6 if b else 1.2,
                "joint_self": j}
        on_anns.append(dict(base, person_anns=anns))
        on_plane.append(dict(base, mask_miss=torch.from_numpy(want.copy())))
    dice = np.array([[0.2, 0.9, 0.8, 0.4, 0.6, 0.9], [0.5, 0.3, 0.1, 0.7, 0.2, 0.1]])
    return on_anns, on_plane, dice


def test_augmenter_on_person_anns_equals_itself_on_mask_miss():
    from multiposenet.pytorch_amd.datasets.augment import DeviceAugmenter
    on_anns, on_plane, dice = _samples()
    da = DeviceAugmenter(64, 4, dict(center_perterb_max=10))
    img_a, heat_a, hm_a, _ = da(on_anns, dice=dice)
    img_p, heat_p, hm_p, _ = da(on_plane, dice=dice)
    assert hm_a is not None and tuple(hm_a.shape) == (2, 18, 16, 16) and hm_a.dtype == torch.float32
    assert torch.equal(img_a, img_p) and torch.equal(heat_a, heat_p) and torch.equal(hm_a, hm_p)
    assert float(hm_p.min()) < 0.5 < float(hm_p.max())                   # the crop sees both masked and unmasked cells
    # with the box path's own inputs next to it
    for s in on_anns + on_plane:
        h, w = s["img"].shape[:2]
        s["segmentations"], s["iscrowd"] = sc.segmentations(h, w)[0][:4], [0, 0, 1, 0]
    img_a, heat_a, hm_a, box_a, _ = da.call_with_boxes(on_anns, dice=dice)
    img_p, heat_p, hm_p, box_p, _ = da.call_with_boxes(on_plane, dice=dice)
    assert torch.equal(img_a, img_p) and torch.equal(heat_a, heat_p) and torch.equal(hm_a, hm_p) and torch.equal(box_a, box_p)
    assert tuple(box_a.shape) == (2, 3, 5) and int((box_a[:, :, 4] == 0).sum()) >= 1


def test_entry_point_refuses_bad_arguments_without_launching():
    from multiposenet.pytorch_amd import _lib
    L = _lib.lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    out = torch.full((4096,), 7, dtype=torch.uint8, device=dev)
    tab = torch.zeros(64, dtype=torch.int64, device=dev)
    ws = torch.full((64,), 9, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    p = lambda t, o=0: ctypes.c_void_p(t.data_ptr() + o)
    nul = ctypes.c_void_p(None)

    def call(imgs=p(tab), n_img=1, insts=p(tab), workspace=p(ws), o=p(out)):
        return L.mpn_segm_mask_miss(imgs, n_img, insts, p(tab), 1, p(tab), 1, p(tab), p(tab), p(tab), 3, 0, p(tab), 0, 64, 64, o, 4096,
                                    workspace, 64, nul)

    for kw in (dict(imgs=nul), dict(o=nul), dict(workspace=nul), dict(insts=nul), dict(n_img=0), dict(imgs=p(tab, 4)),
               dict(insts=p(tab, 4)), dict(workspace=p(ws, 4))):
        assert call(**kw) == -2, list(kw)
    torch.cuda.synchronize()
    assert bool((out == 7).all()) and bool((ws == 9).all())                # nothing was launched: not even the workspace memset
