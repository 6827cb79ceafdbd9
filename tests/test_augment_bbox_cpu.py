"""CPU tests of the detection loader's device augmentation (datasets/augment.py: augment_meta_bbox, instance_rects,
DeviceBBoxAugmenter.geometry; csrc/augment.hip: mpn_augment_boxes argument checks).

1. The host geometry against tests/golden/g19_augment_bbox.npz, recorded from the reference's REAL aug_scale_bbox / aug_rotate_bbox /
   aug_croppad_bbox / aug_flip_bbox (tests/golden/make_golden_augment_bbox.py): bit for bit.
2. The image-only keypoint geometry, fed the same inputs, crops somewhere else on the rotated cases: the reason augment_meta_bbox
   exists.
3. The float64 restatement of the box rule (tests/augment_bbox_ref.py): its row assembly equals the recorded outputs of the real
   get_ground_truth / bbox_collater, and it has teeth: seven modelled faults each leave [inner, outer] on a golden case.
4. The host rules of Cocobbox (zero masks, crowds, empty lists, padding) and the C entry point's argument checks.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import augment_bbox_ref as br
import augment_ref as ar
from helpers import ROOT

CASES, INP, STRIDE, G = br.golden()


def _meta(c, **kw):
    from multiposenet.pytorch_amd.datasets.augment import augment_meta_bbox
    return augment_meta_bbox(int(c["hw"][0]), int(c["hw"][1]), float(c["scale_provided"]), c["objpos_in"], c["dice"], INP, INP,
                             ar.case_params(c), **kw)


def test_golden_file_covers_the_cases_the_geometry_needs():
    assert len(CASES) >= 9
    deg = [(float(c["dice"][2]) - 0.5) * 2 * 40 for c in CASES]
    assert max(deg) == 40.0 and min(deg) == -40.0
    assert any(c["scale"] > 1 for c in CASES) and any(c["scale"] < 1 for c in CASES)
    assert any(c["flip"] and c["dice"][5] == c["params"][6] for c in CASES)              # a flip at dice == flip_prob
    assert any(c["hw"][0] % 2 and c["hw"][1] % 2 for c in CASES)
    assert any(np.isnan(c["dice"][1]) for c in CASES) and {0.0, 0.5, 1.0} <= {float(c["params"][2]) for c in CASES}
    assert any(c["seed"] >= 0 for c in CASES) and any(c["seed"] < 0 for c in CASES)
    assert any(np.all(c["origin"] < 0) for c in CASES)                                     # corner objpos: pad visible


@pytest.mark.parametrize("i", range(len(CASES)))
def test_augment_meta_bbox_matches_the_reference_bit_for_bit(i):
    c = CASES[i]
    m = _meta(c)
    assert m["scale"] == float(c["scale"])
    assert (m["nh"], m["nw"]) == tuple(c["stage_shapes"][0][:2]) == tuple(c["stage_shapes"][0][2:])      # masks: the image's rule
    assert (m["nH"], m["nW"]) == tuple(c["stage_shapes"][1][:2]) == tuple(c["stage_shapes"][1][2:])
    assert np.array_equal(m["M"], c["M"]) and np.array_equal(m["Minv"], ar.invert_affine(c["M"]))
    # objpos: scaled, then moved by nothing
    assert np.array_equal(m["objpos"], c["objpos_scale"])
    for k in ("objpos_rotate", "objpos_croppad", "objpos_flip"):
        assert np.array_equal(c[k], c["objpos_scale"])
    assert m["center"] == tuple(int(v) for v in c["center"]) and (m["ox"], m["oy"]) == tuple(int(v) for v in c["origin"])
    assert m["flip"] == bool(c["flip"])
    assert m["degree"] == (float(c["dice"][2]) - 0.5) * 2 * float(c["params"][4])
    # the (crop + 1)^2 mask frame next to the crop^2 image
    assert tuple(c["stage_shapes"][2]) == tuple(c["stage_shapes"][3]) == (INP, INP, INP + 1, INP + 1)
    # the flip turns the mask over its OWN width: final column x shows canvas column ox + (crop_x - x)
    u = np.arange(INP + 1)
    up = INP - u if m["flip"] else u
    cx = m["ox"] + up
    want = np.where((cx >= 0) & (cx < m["nW"]), cx, -1)
    assert np.array_equal(c["final_row_canvas_x"], want)
    v = np.arange(INP + 1)
    cy = m["oy"] + v
    assert np.array_equal(c["final_col0_canvas_y"], np.where((cy >= 0) & (cy < m["nH"]), cy, -1))


def test_seeded_cases_draw_the_dice_in_the_references_order():
    import random
    from multiposenet.pytorch_amd.datasets.augment import draw_dice
    n = 0
    for c in CASES:
        if c["seed"] >= 0:
            d = draw_dice(random.Random(int(c["seed"])), ar.case_params(c))
            assert np.array_equal(d, c["dice"], equal_nan=True)
            n += 1
    assert n >= 4


def test_image_only_keypoint_geometry_crops_elsewhere_on_rotated_cases():
    """aug_rotate_bbox leaves objpos unrotated, aug_rotate rotates it: same inputs, another crop centre."""
    from multiposenet.pytorch_amd.datasets.augment import augment_meta
    n = 0
    for c in CASES:
        k = augment_meta(int(c["hw"][0]), int(c["hw"][1]), float(c["scale_provided"]), c["objpos_in"], np.ones((18, 3)), np.zeros((0, 18, 3)),
                         c["dice"], INP, INP, ar.case_params(c), with_mask=False)
        m = _meta(c)
        assert np.array_equal(k["M"], m["M"]) and k["scale"] == m["scale"]
        if abs(m["degree"]) > 5:
            assert k["center"] != m["center"] and (k["ox"], k["oy"]) != (m["ox"], m["oy"])
            n += 1
    assert n >= 6


def test_augment_meta_bbox_refuses_slices_that_would_wrap_or_truncate():
    from multiposenet.pytorch_amd._lib import MpnError
    from multiposenet.pytorch_amd.datasets.augment import augment_meta_bbox
    d = np.array([0.7, np.nan, 0.5, 0.5, 0.5, 0.9])
    p = dict(ar.case_params(CASES[0]), scale_prob=0.0)
    augment_meta_bbox(100, 100, 0.6, (50.0, 50.0), d, 64, 64, p)
    # x0 = cx + 32; the mask slice [x0, x0 + 65) must fit into 100 + 128: cx <= 131 passes, 132 truncates the MASK (the image would fit)
    augment_meta_bbox(100, 100, 0.6, (131.0, 50.0), d, 64, 64, p)
    for pos in ((132.0, 50.0), (50.0, 132.0), (-33.0, 50.0), (50.0, -33.0), (float("nan"), 1.0)):
        with pytest.raises(MpnError):
            augment_meta_bbox(100, 100, 0.6, pos, d, 64, 64, p)
    augment_meta_bbox(100, 100, 0.6, (-32.0, -32.0), d, 64, 64, p)
    with pytest.raises(MpnError):
        augment_meta_bbox(100, 100, 0.6, (50.0, 50.0), d[:5], 64, 64, p)
    with pytest.raises(MpnError):
        augment_meta_bbox(100, 100, 0.6, (50.0, 50.0), np.array([0.1, np.nan, 0.5, 0.5, 0.5, 0.9]), 64, 64, dict(p, scale_prob=1))
    with pytest.raises(MpnError):
        augment_meta_bbox(100, 100, -1.0, (50.0, 50.0), d, 64, 64, p)


# ---- the restatement's row assembly against the real get_ground_truth / bbox_collater --------------------------------------------

def test_row_assembly_equals_the_recorded_get_ground_truth_and_collater():
    n = int(G["gt_n_images"])
    S = int(G["gt_crop"])
    rows = []
    for i in range(n):
        masks, crowd = G["gt%d_masks" % i], G["gt%d_iscrowd" % i]
        assert masks.shape[1:] == (S + 1, S + 1)
        r = br.rows_of(masks, crowd)
        assert r.shape == G["gt%d_rows" % i].shape and np.array_equal(r, G["gt%d_rows" % i])
        rows.append(r)
    got = br.collate(rows)
    assert got.dtype == np.float32 and np.array_equal(got, G["gt_collated"])
    assert tuple(br.collate([rows[3], rows[3]]).shape) == tuple(G["gt_collated_no_rows_shape"]) == (2, 0, 5)
    # what the recorded rows say: full mask reaches crop + 1, single pixel, empty, a crowd in the middle yields no row
    assert np.array_equal(G["gt0_rows"], [[0, 0, S + 1, S + 1, 0], [5, 3, 6, 4, 0], [-1, -1, -1, -1, -1]])
    assert G["gt2_rows"].shape[0] == 2 and G["gt3_rows"].shape[0] == 0
    assert br.collate(rows, row_multiple=8).shape == (n, 8, 5) and np.all(br.collate(rows, 8)[:, 4:] == -1)


# ---- teeth ---------------------------------------------------------------------------------------------------------------------

_REF = {}


def _truth(i, s):
    """inner / outer of shape s of golden case i (computed once)."""
    if (i, s) not in _REF:
        c = CASES[i]
        mask = br.instance_shapes(900 + i, int(c["hw"][0]), int(c["hw"][1]))[s]
        inner, outer, _, _ = br.inner_outer(mask, br.case_geo(c), INP)
        _REF[(i, s)] = (mask, inner, outer)
    return _REF[(i, s)]


def _outside(row, inner, outer):
    ok, _ = br.check_row(row, inner, outer)
    return not ok


def test_the_restatement_agrees_with_itself_and_is_decided_on_the_golden_cases():
    for i, s in ((0, 0), (3, 5), (5, 0)):
        mask, inner, outer = _truth(i, s)
        assert np.array_equal(inner, outer) and inner[4] == 0
        assert br.check_row(inner, inner, outer) == (True, 0)
    # a flipped case whose box touches the far edge of the (crop + 1) frame
    assert _truth(5, 0)[1][2] == INP + 1 and CASES[5]["flip"]


@pytest.mark.parametrize("fault", ["flip_over_crop_minus_1", "rotated_objpos", "threshold_0.25", "missing_plus_1", "tap_shift_1",
                                   "rectangle_test_dropped"])
def test_modelled_fault_leaves_the_inner_outer_interval(fault):
    from multiposenet.pytorch_amd.datasets.augment import augment_meta
    i, s = {"flip_over_crop_minus_1": (5, 0), "rotated_objpos": (0, 0), "threshold_0.25": (7, 1), "missing_plus_1": (0, 0),
            "tap_shift_1": (0, 0), "rectangle_test_dropped": (0, 0)}[fault]
    c = CASES[i]
    mask, inner, outer = _truth(i, s)
    geo = br.case_geo(c)
    if fault == "flip_over_crop_minus_1":
        assert c["flip"]
        row = br.inner_outer(mask, geo, INP, flip_w=INP)[0]
    elif fault == "rotated_objpos":
        k = augment_meta(int(c["hw"][0]), int(c["hw"][1]), float(c["scale_provided"]), c["objpos_in"], np.ones((18, 3)), np.zeros((0, 18, 3)),
                         c["dice"], INP, INP, ar.case_params(c), with_mask=False)
        row = br.inner_outer(mask, br.case_geo(c, origin=(k["ox"], k["oy"])), INP)[0]
    elif fault == "threshold_0.25":
        row = br.inner_outer(mask, geo, INP, thr=0.25)[0]
    elif fault == "missing_plus_1":
        row = br.inner_outer(mask, geo, INP, plus=0)[0]
    elif fault == "tap_shift_1":
        row = br.inner_outer(mask, geo, INP, tap_shift=1)[0]
    else:
        row = br.inner_outer(br.unpacked_view(mask, br.rect_of(mask)), geo, INP)[0]
    assert _outside(row, inner, outer), "%s: %s lies inside [%s, %s]" % (fault, row, inner, outer)


def test_modelled_fault_crowd_given_a_row_changes_the_recorded_rows():
    masks, crowd = G["gt2_masks"], G["gt2_iscrowd"]
    assert crowd.tolist() == [0, 1, 0]
    bad = br.rows_of(masks, crowd, crowd_rows=True)
    assert bad.shape[0] == 3 and not np.array_equal(bad[:2], G["gt2_rows"])


# ---- host rules ----------------------------------------------------------------------------------------------------------------

def _sample(H=50, W=70, instances=None, iscrowd=None, objpos=(35.0, 25.0)):
    img = torch.from_numpy(br.synth_image(3, H, W))
    return {"img": img, "objpos": objpos, "scale_provided": 0.6, "instances": instances, "iscrowd": iscrowd}


def _blob(H, W, y0, y1, x0, x1, dtype=np.uint8):
    m = np.zeros((H, W), dtype=dtype)
    m[y0:y1, x0:x1] = 1
    return m


def test_host_rules_of_cocobbox():
    from multiposenet.pytorch_amd._lib import MpnError
    from multiposenet.pytorch_amd.datasets.augment import DeviceBBoxAugmenter, instance_rects
    H, W = 50, 70
    a, b, z = _blob(H, W, 5, 9, 10, 30), _blob(H, W, 0, 50, 69, 70, np.bool_), np.zeros((H, W), dtype=np.uint8)
    # a zero mask is dropped, a crowd is skipped; the rectangle is the mask's own extents
    r = instance_rects(_sample(instances=[a, z, torch.from_numpy(b), a], iscrowd=[0, 0, 0, 1]), H, W)
    assert [x[1:] for x in r] == [(10, 5, 20, 4), (69, 0, 1, 50)]
    # a crowd counts for the list being non-empty but yields no row
    assert instance_rects(_sample(instances=[a], iscrowd=[1]), H, W) == []
    # an empty list raises, and so does one that holds zero masks only (the reference: IndexError at instance_mask_list[0])
    for inst, cr in (([], []), ([z], [0]), ([z, z], [1, 0])):
        with pytest.raises(MpnError):
            instance_rects(_sample(instances=inst, iscrowd=cr), H, W)
    # bad inputs
    for inst, cr in (([a], [0, 0]), ([a[:-1]], [0]), ([a.astype(np.int32)], [0]), ([a.astype(np.float32)], [0]), ([a[None]], [0]),
                     (None, [0]), ([a], None), ([[1, 2]], [0])):
        with pytest.raises(MpnError):
            instance_rects(_sample(instances=inst, iscrowd=cr), H, W)
    # geometry() runs without a GPU and carries the rectangles
    da = DeviceBBoxAugmenter(64, 4, row_multiple=8)
    dice = np.array([[0.5, 0.5, 0.3, 0.5, 0.5, 0.9]] * 2)
    metas = da.geometry([_sample(instances=[a, b], iscrowd=[0, 0]), _sample(instances=[a], iscrowd=[1])], dice=dice)
    assert [len(g["rects"]) for g in metas] == [2, 0] and metas[0]["H"] == H and metas[0]["flip"] is False
    assert set(("scale", "nh", "nw", "nH", "nW", "M", "Minv", "ox", "oy", "flip", "degree", "center", "objpos")) <= set(metas[0])
    with pytest.raises(MpnError):
        da.geometry([], dice=np.zeros((0, 6)))
    with pytest.raises(MpnError):
        da.geometry([_sample(instances=[a], iscrowd=[0])], dice=np.zeros((1, 5)))
    with pytest.raises(MpnError):
        DeviceBBoxAugmenter(64, 4, row_multiple=0)
    if not torch.cuda.is_available():
        with pytest.raises(MpnError):
            da([_sample(instances=[a], iscrowd=[0])], dice=dice[:1])


def test_device_augmenter_docstring_no_longer_calls_the_bbox_chain_identical():
    from multiposenet.pytorch_amd.datasets.augment import DeviceAugmenter
    assert "is the identical image chain" not in DeviceAugmenter.__doc__ and "augment_meta_bbox" in DeviceAugmenter.__doc__


def test_augment_boxes_argument_checks_return_error_codes():
    from multiposenet.pytorch_amd import _lib
    L = _lib.lib()
    BAD = int(re.search(r"#define\s+MPN_E_BADARG\s+\(?(-?\d+)\)?", open(os.path.join(ROOT, "include", "mpn.h")).read()).group(1))
    nul, one = ctypes.c_void_p(None), ctypes.c_void_p(0x1000)          # never dereferenced: validation fails first
    f = L.mpn_augment_boxes
    assert f(nul, 64, one, 1, one, 1, one, 480, 480, one, nul) == BAD       # no source
    assert f(one, 0, one, 1, one, 1, one, 480, 480, one, nul) == BAD        # empty source
    assert f(one, 64, nul, 1, one, 1, one, 480, 480, one, nul) == BAD       # no table
    assert f(one, 64, one, 1, one, 1, one, 480, 480, nul, nul) == BAD       # no workspace
    assert f(one, 64, one, 1, nul, 1, one, 480, 480, one, nul) == BAD       # no row map
    assert f(one, 64, one, 1, one, 1, nul, 480, 480, one, nul) == BAD       # no output
    assert f(one, 64, one, -1, one, 1, one, 480, 480, one, nul) == BAD
    assert f(one, 64, one, 65536, one, 1, one, 480, 480, one, nul) == BAD   # the instance is a grid dimension
    assert f(one, 64, one, 1, one, -1, one, 480, 480, one, nul) == BAD
    assert f(one, 64, one, 1, one, 1, one, 0, 480, one, nul) == BAD
    assert f(one, 64, one, 1, one, 1, one, 480, 65536, one, nul) == BAD
    assert f(nul, 0, nul, 0, nul, 0, nul, 480, 480, nul, nul) == 0          # nothing to do: no launch
    w = L.mpn_augment_boxes_workspace_bytes
    assert w(5, 480, 480) == 5 * 8 * 31 * 5 * 4 and w(1, 64, 64) == 2 * 5 * 5 * 4 and w(0, 480, 480) == 0 and w(-1, 480, 480) == 0
    assert _lib.SIGNATURES["mpn_augment_boxes"][0] is ctypes.c_int
