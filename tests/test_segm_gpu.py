"""GPU tests of the segmentation rasteriser (csrc/segm.hip through datasets/segm.py) and of the ``segmentations`` path of
DeviceBBoxAugmenter and DeviceAugmenter.call_with_boxes.

PARITY is byte for byte: the rule is integer-valued, its float64 steps are separately rounded operations in a fixed order on both
sides, so there is no tolerance anywhere in this file.  The truth is the sequential restatement tests/segm_ref.py (sort-and-merge
form) on the committed inputs of tests/segm_cases.py, computed once per size and shared; tests/test_segm_cpu.py shows that those
inputs reject ten modelled misreadings of the rule.  Sizes 5 x 6, 37 x 53, 64 x 65 and 130 x 70: the heights fall below, on and
beyond one and two 64-bit words of a column.

The augmenters are compared with THEMSELVES on ``instances`` built from the restatement, with the same dice: the image and the
boxes must be the same bytes; where an instance rasterises empty the ``segmentations`` path keeps a -1 row in its slot and the
``instances`` path drops the row before numbering.
"""
import numpy as np
import pytest
import torch

import augment_bbox_ref as br
import segm_cases as sc
import segm_ref as sr

pytestmark = pytest.mark.gpu

_TRUTH = {}


def _truth(h, w):
    """(segmentations, uint8 [7, h, w] from the restatement), computed once."""
    if (h, w) not in _TRUTH:
        segms = sc.segmentations(h, w)[0]
        _TRUTH[(h, w)] = (segms, np.stack([sr.ann_to_mask(s, h, w) for s in segms]))
    return _TRUTH[(h, w)]


# ---- 1. dense masks -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("h,w", sc.SIZES)
def test_dense_masks_equal_the_restatement_byte_for_byte(h, w):
    from multiposenet.pytorch_amd.datasets.segm import rasterize_segmentations
    segms, want = _truth(h, w)
    got = rasterize_segmentations(segms, h, w)
    assert got.is_cuda and got.dtype == torch.uint8 and got.is_contiguous() and tuple(got.shape) == (sc.N_INST, h, w)
    got = got.cpu().numpy()
    for i in range(sc.N_INST):
        diff = np.argwhere(got[i] != want[i])
        print("%d x %d instance %d: %d ON cells, %d differ" % (h, w, i, int(want[i].sum()), diff.shape[0]))
        assert diff.shape[0] == 0, "instance %d differs at (y, x) %s" % (i, diff[:8].tolist())
    assert not want[sc.EMPTY].any() and all(want[i].any() for i in range(sc.N_INST) if i != sc.EMPTY)
    # every instance alone and the list reversed: no instance depends on its neighbours or its position
    rev = rasterize_segmentations(segms[::-1], h, w).cpu().numpy()
    assert np.array_equal(rev, want[::-1])
    one = rasterize_segmentations(segms[3:4], h, w).cpu().numpy()
    assert np.array_equal(one[0], want[3])


def test_packed_rectangles_any_flags_and_determinism():
    """The packed form of a mixed-size batch: every rectangle holds the restatement's cells at the offsets boxes_from_rects uses,
    the 'any cell ON' flags are right, and two runs give identical bytes (the XOR toggles are order-independent)."""
    from multiposenet.pytorch_amd.datasets import segm
    packs, wants = [], []
    for h, w in sc.SIZES:
        segms, want = _truth(h, w)
        packs.append(segm.pack_segmentations(segms, h, w))
        wants += list(want)
    pack = segm.concat_packs(packs)
    buf, anyon, _ = segm.rasterize_packed(pack)
    buf2, anyon2, _ = segm.rasterize_packed(pack)
    torch.cuda.synchronize()
    assert pack.n == 4 * sc.N_INST and anyon.dtype == torch.int32 and torch.equal(anyon, anyon2)
    assert anyon.cpu().tolist() == [int(m.any()) for m in wants] and anyon.cpu().tolist().count(0) == 4
    a, b = buf.cpu().numpy(), buf2.cpu().numpy()
    for i, (m, (x0, y0, rw, rh)) in enumerate(zip(wants, pack.rects())):
        off = int(pack.insts[i, segm.I_OUT_OFF])
        assert off % 16 == 0
        assert np.array_equal(a[off: off + rw * rh].reshape(rh, rw), m[y0:y0 + rh, x0:x0 + rw]), i
        assert np.array_equal(a[off: off + rw * rh], b[off: off + rw * rh])


def test_strict_false_drops_the_malformed_part_only():
    from multiposenet.pytorch_amd.datasets.segm import rasterize_segmentations
    h, w = 37, 53
    segms, want = _truth(h, w)
    got = rasterize_segmentations([segms[1] + [[1.0, 2.0, 3.0, 4.0]], [[1.0, 2.0]]], h, w, strict=False).cpu().numpy()
    assert np.array_equal(got[0], want[1]) and not got[1].any()


# ---- 2. the augmenters ----------------------------------------------------------------------------------------------------------

def _samples(S, with_empty):
    """B = 3: 53 x 67 with the seven annotations (one of them a crowd; with or without the one that rasterises empty), 50 x 70 with
    three of them, and a crowd-only sample.  Returns (samples on 'segmentations', the same on 'instances' from the restatement, dice)."""
    sp = 0.6 if S == 64 else 0.3
    out_s, out_i = [], []
    for b, (h, w, pick, crowd) in enumerate([(53, 67, list(range(7 if with_empty else 6)), 4), (50, 70, [3, 0, 5], None), (50, 70, [1], 1)]):
        segms, want = _truth(h, w)
        base = {"img": torch.from_numpy(br.synth_image(20 + b, h, w)), "objpos": (0.45 * w, 0.5 * h), "scale_provided": sp if b < 2 else 0.6,
                "iscrowd": [1 if i == crowd else 0 for i in pick]}
        out_s.append(dict(base, segmentations=[segms[i] for i in pick]))
        out_i.append(dict(base, instances=[want[i] for i in pick]))
    dice = np.array([[0.2, 0.9, 0.8, 0.4, 0.6, 0.9], [0.5, 0.3, 0.1, 0.7, 0.2, 0.1], [0.3, 0.5, 0.5, 0.5, 0.5, 0.9]])
    return out_s, out_i, dice


def _without_slot(rows, slot):
    """[N, 5] with row `slot` deleted and a -1 row appended."""
    return np.concatenate([rows[:slot], rows[slot + 1:], np.full((1, 5), -1.0, dtype=rows.dtype)])


@pytest.mark.parametrize("S", [64, 130, 480])
def test_bbox_augmenter_on_segmentations_equals_itself_on_instances(S):
    from multiposenet.pytorch_amd.datasets.augment import DeviceBBoxAugmenter
    da = DeviceBBoxAugmenter(S, 4, dict(center_perterb_max=10))
    # no instance comes out empty: the same bytes
    ss, si, dice = _samples(S, False)
    img_s, box_s, metas_s = da(ss, dice=dice)
    img_i, box_i, metas_i = da(si, dice=dice)
    assert tuple(box_s.shape) == (3, 5, 5) and box_s.dtype == torch.float32 and box_s.is_cuda
    assert torch.equal(img_s, img_i) and torch.equal(box_s, box_i)
    assert int((box_s[:2, :, 4] == 0).sum()) >= 5 and bool((box_s[2] == -1).all())                 # the crowd-only sample has no row
    assert [len(g["rects"]) for g in metas_s] == [5, 3, 0] and all(g["rects"][0][0] is None for g in metas_s[:2])
    # with the empty one: it keeps its slot as a -1 row, N counts it
    ss, si, dice = _samples(S, True)
    img_s, box_s, _ = da(ss, dice=dice)
    img_i, box_i, _ = da(si, dice=dice)
    assert tuple(box_s.shape) == (3, 6, 5) and tuple(box_i.shape) == (3, 5, 5) and torch.equal(img_s, img_i)
    got, want = box_s.cpu().numpy(), box_i.cpu().numpy()
    assert np.all(got[0, 5] == -1)                                                                 # slot 5: annotation 6 without the crowd
    assert np.array_equal(_without_slot(got[0], 5)[:5], want[0]) and np.array_equal(got[1:, :5], want[1:]) and np.all(got[1:, 5] == -1)
    # two runs of one batch: identical bytes; row_multiple pads
    _, again, _ = da(ss, dice=dice)
    _, b8, _ = DeviceBBoxAugmenter(S, 4, dict(center_perterb_max=10), row_multiple=8)(ss, dice=dice)
    torch.cuda.synchronize()
    assert torch.equal(again, box_s) and tuple(b8.shape) == (3, 8, 5) and torch.equal(b8[:, :6], box_s) and bool((b8[:, 6:] == -1).all())


def test_sample_whose_instances_are_all_empty_gives_minus_one_rows_and_no_error():
    from multiposenet.pytorch_amd.datasets.augment import DeviceBBoxAugmenter
    ss, _, dice = _samples(64, True)
    segms = _truth(53, 67)[0]
    s = dict(ss[0], segmentations=[segms[sc.EMPTY], segms[sc.EMPTY]], iscrowd=[0, 0])
    _, bbox, metas = DeviceBBoxAugmenter(64, 4, dict(center_perterb_max=10))([s], dice=dice[:1])
    assert tuple(bbox.shape) == (1, 2, 5) and bool((bbox == -1).all())


@pytest.mark.parametrize("S", [64, 130])
def test_call_with_boxes_on_segmentations_equals_itself_on_instances(S):
    from multiposenet.pytorch_amd.datasets.augment import DeviceAugmenter
    ss, si, dice = _samples(S, True)
    rs = np.random.RandomState(3)
    for a, b in zip(ss, si):
        j = np.zeros((17, 3))
        j[:, 0], j[:, 1], j[:, 2] = rs.uniform(0, 60, 17), rs.uniform(0, 50, 17), rs.choice([0.0, 1.0, 2.0], 17)
        a["joint_self"] = b["joint_self"] = j
    da = DeviceAugmenter(S, 4, dict(center_perterb_max=10))
    img_s, heat_s, hm_s, box_s, _ = da.call_with_boxes(ss, dice=dice)
    img_i, heat_i, hm_i, box_i, _ = da.call_with_boxes(si, dice=dice)
    assert torch.equal(img_s, img_i) and torch.equal(heat_s, heat_i) and hm_s is None and hm_i is None
    got, want = box_s.cpu().numpy(), box_i.cpu().numpy()
    assert got.shape == (3, 6, 5) and want.shape == (3, 5, 5) and int((want[:, :, 4] == 0).sum()) >= 5
    assert np.array_equal(_without_slot(got[0], 5)[:5], want[0]) and np.array_equal(got[1:, :5], want[1:]) and np.all(got[1:, 5] == -1)


def test_kinds_do_not_mix():
    from multiposenet.pytorch_amd._lib import MpnError
    from multiposenet.pytorch_amd.datasets.augment import DeviceAugmenter, DeviceBBoxAugmenter
    ss, si, dice = _samples(64, False)
    da = DeviceBBoxAugmenter(64, 4, dict(center_perterb_max=10))
    both = dict(ss[0], instances=si[0]["instances"])
    neither = {k: v for k, v in ss[0].items() if k != "segmentations"}
    for batch in ([both], [neither], [ss[0], si[1]], [dict(ss[0], iscrowd=[0])], [dict(ss[0], segmentations=[], iscrowd=[])],
                  [dict(ss[0], segmentations=[[[1.0, 2.0, 3.0, 4.0]]], iscrowd=[0])]):
        with pytest.raises(MpnError):
            da(batch, dice=dice[:len(batch)])
        with pytest.raises(MpnError):
            DeviceAugmenter(64, 4).call_with_boxes([dict(s, joint_self=np.ones((17, 3))) for s in batch], dice=dice[:len(batch)])
