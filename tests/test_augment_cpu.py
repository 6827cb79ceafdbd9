"""Device augmentation (datasets/augment.py, csrc/augment.hip), the part that needs no GPU:

* the product's host geometry against tests/golden/g17_augment.npz, recorded from the reference's REAL aug_scale / aug_rotate /
  aug_croppad / aug_flip / add_neck / remove_illegal_joint (tests/golden/make_golden_augment.py): joints and objpos bit for bit,
  shapes, the warpAffine matrix, the crop and the flip exactly;
* the dice helper against the recorded draw order;
* the C entry points in header, library and ctypes table, and their argument checks;
* the teeth of the element-wise bound tests/test_augment_gpu.py applies: tests/augment_ref.py with one modelled fault at a time
  must violate it on the golden cases, and the weight-error figure the bound's absolute term rests on must hold.
"""
import ctypes
import os
import random
import re
import subprocess

import numpy as np
import pytest

import augment_ref as ar
from helpers import ROOT
from multiposenet.pytorch_amd.datasets import augment as aug

CASES, INP, STRIDE = ar.golden_cases()


def _geo(case):
    return aug.augment_meta(int(case["hw"][0]), int(case["hw"][1]), float(case["scale_provided"]), case["objpos_in"], case["joint_self_neck"],
                            case["joint_others_neck"], case["dice"], INP, INP, ar.case_params(case), case["objpos_other_in"])


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_golden_covers_what_it_should():
    assert len(CASES) >= 8
    flips = {int(c["flip"]) for c in CASES}
    scales = [float(c["scale"]) for c in CASES]
    deg = [(float(c["dice"][2]) - 0.5) * 80 for c in CASES]
    assert flips == {0, 1} and min(scales) < 1 < max(scales)
    assert max(deg) > 39 and min(deg) < -39 and min(abs(d) for d in deg) < 0.1
    assert {0} < {c["joint_others_in"].shape[0] for c in CASES}
    assert any(c["hw"][0] % 2 and c["hw"][1] % 2 for c in CASES)
    assert any(np.isnan(c["dice"][1]) for c in CASES)


@pytest.mark.parametrize("i", range(len(CASES)))
def test_host_geometry_reproduces_the_reference(i):
    c = CASES[i]
    js, jo = aug.add_neck(c["joint_self_in"], c["joint_others_in"])
    assert _same_bits(js, c["joint_self_neck"]) and _same_bits(jo, c["joint_others_neck"])
    g = _geo(c)
    assert g["scale"] == float(c["scale"])
    st = c["stage_shapes"]
    assert (g["nh"], g["nw"]) == tuple(st[0][:2]) and (g["nH"], g["nW"]) == tuple(st[1][:2])
    assert tuple(st[2]) == (INP, INP, INP + 1, INP + 1) and tuple(c["mask_grid"]) == (INP // STRIDE, INP // STRIDE)
    assert _same_bits(g["M"], c["M"])
    assert g["center"] == tuple(int(v) for v in c["center"])
    assert (g["ox"], g["oy"]) == (int(c["center"][0]) + INP // 2 - INP, int(c["center"][1]) + INP // 2 - INP)
    assert g["flip"] == bool(c["flip"])
    assert _same_bits(g["objpos"], c["objpos_flip"])
    assert _same_bits(g["joint_self"], c["joint_self_flip"]) and _same_bits(g["joint_others"], c["joint_others_flip"])
    js, jo = aug.remove_illegal_joint(g["joint_self"], g["joint_others"], INP, INP)
    assert _same_bits(js, c["joint_self_out"]) and _same_bits(jo, c["joint_others_out"])
    # the inverse really inverts, and the transformed objpos is where the geometry sends the source objpos
    full = np.vstack([g["M"], [0, 0, 1]])
    assert np.abs(np.vstack([g["Minv"], [0, 0, 1]]).dot(full) - np.eye(3)).max() < 1e-9
    assert _same_bits(g["Minv"], ar.invert_affine(c["M"]))


def test_dice_helper_draws_in_the_reference_order():
    seen = 0
    for c in CASES:
        if int(c["seed"]) < 0:
            continue
        seen += 1
        d = aug.draw_dice(random.Random(int(c["seed"])), ar.case_params(c))
        assert _same_bits(d, c["dice"]), (d, c["dice"])
    assert seen >= 3
    # dice2 is drawn exactly when dice <= scale_prob: the stream position after a sample shows it
    for prob, n in ((1, 6), (0.0, 5)):
        r1, r2 = random.Random(9), random.Random(9)
        aug.draw_dice(r1, dict(aug.DEFAULT_PARAMS, scale_prob=prob))
        for _ in range(n):
            r2.random()
        assert r1.random() == r2.random()


def test_default_params_are_the_reference_defaults():
    p = aug.DEFAULT_PARAMS
    assert (p["scale_min"], p["scale_max"], p["scale_prob"], p["target_dist"]) == (0.8, 1.2, 1, 0.6)
    assert (p["max_rotate_degree"], p["center_perterb_max"], p["flip_prob"], p["sigma"], p["np"], p["mode"]) == (40, 40, 0.3, 7.0, 56, 5)
    for c in CASES:
        if not np.array_equal(c["params"], [0.8, 1.2, 1, 0.6, 40, 40, 0.3]):
            continue
        assert ar.case_params(c) == {k: float(p[k]) for k in ar.PARAM_KEYS}


def test_add_neck_and_remove_illegal_joint_on_hand_made_rows():
    js = np.zeros((17, 3))
    js[:, 0] = np.arange(17) * 10.0
    js[:, 1] = np.arange(17) * 3.0 + 1
    js[:, 2] = 1.0
    js[5], js[6] = (51.0, 20.0, 1.0), (60.0, 23.0, 0.0)              # left / right shoulder
    out, others = aug.add_neck(js, np.zeros((0, 17, 3)))
    assert out.shape == (18, 3) and others.shape == (0, 18, 3)
    assert out[1].tolist() == [np.round(55.5), np.round(21.5), 1.0]      # round half to even: (56, 22), visible if either is 1
    assert out[0].tolist() == js[0].tolist() and out[2].tolist() == js[6].tolist() and out[5].tolist() == js[5].tolist()
    assert out[17].tolist() == js[3].tolist() and out[14].tolist() == js[2].tolist()
    a, b = js.copy(), js.copy()
    a[5, 2], a[6, 2] = 2.0, 1.0                                        # either shoulder missing -> neck missing
    b[5, 2], b[6, 2] = 0.0, 0.0                                        # both hidden -> product of the two
    o2, oth = aug.add_neck(js, np.stack([a, b]))
    assert oth.shape == (2, 18, 3) and oth[0, 1, 2] == 2.0 and oth[1, 1, 2] == 0.0
    rows = np.array([[0.0, 0.0, 1.0], [479.999, 479.0, 0.0], [480.0, 10.0, 1.0], [-0.001, 10.0, 0.0], [10.0, 480.0, 1.0], [10.0, -1.0, 2.0]] * 3)
    rs, ro = aug.remove_illegal_joint(rows, np.stack([rows, rows[::-1]]), 480, 480)
    assert rs[:6].tolist() == [[0.0, 0.0, 1.0], [479.999, 479.0, 0.0], [1, 1, 2], [1, 1, 2], [1, 1, 2], [1, 1, 2]]
    assert ro[0].tolist() == rs.tolist() and ro[1].tolist() == rs[::-1].tolist()
    assert rows[2].tolist() == [480.0, 10.0, 1.0]                      # the input is not modified


def test_crop_centre_far_outside_the_canvas_raises():
    from multiposenet.pytorch_amd._lib import MpnError
    c = CASES[0]
    args = dict(H=427, W=640, scale_provided=0.71, joint_self=c["joint_self_neck"], joint_others=c["joint_others_neck"], dice=c["dice"],
                crop_x=INP, crop_y=INP)
    aug.augment_meta(objpos=(320.0, 200.0), **args)
    for bad in ((-900.0, 200.0), (320.0, -900.0), (3000.0, 200.0), (320.0, 3000.0)):
        with pytest.raises(MpnError):
            aug.augment_meta(objpos=bad, **args)
    with pytest.raises(MpnError):
        aug.augment_meta(objpos=(float("nan"), 1.0), **args)


def test_slice_test_is_one_rule_for_both_chains():
    """The boundary list of test_augment_meta_bbox_refuses_slices_that_would_wrap_or_truncate through BOTH chains.  H = W = 100 at
    scale 1, 0 degrees (dice 0.5: the keypoint chain's rotation leaves objpos where it is), crop 64: x0 = cx + 32 and the canvas
    padded by the crop is 100 + 128 = 228 wide.  The mask slice [x0, x0 + 65) fits up to cx = 131; the image slice [x0, x0 + 64) is
    one shorter and fits up to cx = 132."""
    from multiposenet.pytorch_amd._lib import MpnError
    d = np.array([0.7, np.nan, 0.5, 0.5, 0.5, 0.9])
    p = dict(aug.DEFAULT_PARAMS, scale_prob=0.0)
    js = np.ones((18, 3))

    def bbox(pos):
        aug.augment_meta_bbox(100, 100, 0.6, pos, d, 64, 64, p)

    def keypoint(pos, with_mask=True):
        aug.augment_meta(100, 100, 0.6, pos, js, np.zeros((0, 18, 3)), d, 64, 64, p, with_mask=with_mask)

    def raises(f, *a):
        try:
            f(*a)
        except MpnError:
            return True
        return False

    cases = [((50.0, 50.0), False), ((131.0, 50.0), False), ((50.0, 131.0), False), ((-32.0, -32.0), False),
             ((132.0, 50.0), True), ((50.0, 132.0), True), ((-33.0, 50.0), True), ((50.0, -33.0), True), ((float("nan"), 1.0), True)]
    for pos, bad in cases:
        assert raises(bbox, pos) == bad, pos
        assert raises(keypoint, pos) == bad, pos
    for pos in ((132.0, 50.0), (50.0, 132.0)):
        assert not raises(keypoint, pos, False), pos
    for pos in ((133.0, 50.0), (50.0, 133.0), (-33.0, 50.0)):
        assert raises(keypoint, pos, False), pos


def test_aligned_offsets_start_every_block_on_16_bytes_without_overlap():
    for sizes in ([1, 16, 17, 0, 48], [], [0], [15, 1, 921600]):
        offsets, total = aug._aligned_offsets(sizes)
        assert len(offsets) == len(sizes) and all(o % 16 == 0 for o in offsets)
        ends = [o + s for o, s in zip(offsets, sizes)]
        assert all(e <= nxt for e, nxt in zip(ends, offsets[1:] + [total]))            # ranges in order, none overlapping
        assert total == sum((s + 15) // 16 * 16 for s in sizes)
    assert aug._aligned_offsets([1, 16, 17, 0, 48]) == ([0, 16, 32, 64, 64], 112)


# ---------------------------------------------------------------------------------------------------------------- C ABI
NEW = ("mpn_augment_image", "mpn_augment_mask")


def _badarg():
    src = open(os.path.join(ROOT, "include", "mpn.h")).read()
    return int(re.search(r"#define\s+MPN_E_BADARG\s+\(?(-?\d+)\)?", src).group(1))


def test_augment_entry_points_agree_across_header_library_and_ctypes_table():
    from multiposenet.pytorch_amd import _lib
    _lib.build()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mpn.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(mpn_[a-z0-9_]+)\s*\(", src))
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    exported = set(l.split()[-1] for l in out.splitlines() if " T mpn_" in l)
    for name in NEW:
        assert name in declared and name in exported and name in _lib.SIGNATURES, name
    # the table columns of the Python side are the header's
    for k, v in re.findall(r"#define\s+MPN_AUG_([A-Z_]+)\s+(\d+)", src):
        assert getattr(aug, "T_" + k) == int(v), k


def test_augment_entry_points_reject_bad_arguments_without_touching_the_gpu():
    from multiposenet.pytorch_amd import _lib
    L = _lib.lib()
    BAD = _badarg()
    nul = ctypes.c_void_p(None)
    a = ctypes.c_void_p(0x1000)                                       # never dereferenced: validation fails first
    ms = (ctypes.c_float * 6)(0.485, 0.456, 0.406, 0.229, 0.224, 0.225)
    img = lambda **k: L.mpn_augment_image(*[k.get(n, d) for n, d in (("src", a), ("bytes", 4096), ("table", a), ("B", 2), ("out", a),
                                                                      ("cy", 64), ("cx", 64), ("ms", ms), ("stream", nul))])
    msk = lambda **k: L.mpn_augment_mask(*[k.get(n, d) for n, d in (("src", a), ("bytes", 4096), ("table", a), ("B", 2), ("out", a),
                                                                     ("gh", 16), ("gw", 16), ("stride", 4), ("cx", 64), ("stream", nul))])
    for f in (img, msk):
        assert f(src=nul) == BAD and f(table=nul) == BAD and f(out=nul) == BAD
        assert f(bytes=0) == BAD and f(bytes=-1) == BAD and f(B=0) == BAD and f(B=-3) == BAD and f(cx=0) == BAD and f(cx=-64) == BAD
    assert img(cy=0) == BAD and img(cy=-1) == BAD and img(ms=None) == BAD
    assert img(ms=(ctypes.c_float * 6)(0.5, 0.5, 0.5, 0.2, 0.0, 0.2)) == BAD                    # a zero std
    assert msk(gh=0) == BAD and msk(gw=0) == BAD and msk(gh=-1) == BAD and msk(stride=0) == BAD and msk(stride=-4) == BAD


# ---------------------------------------------------------------------------------------------------------------- teeth
def test_float32_weight_error_stays_inside_the_figure_the_bound_uses():
    """W_AXIS u (augment_ref's operation count) bounds sum_k |w32_k - w64_k| at every float32 fraction tried; the float32 side is the
    CPU oracle's restatement of interpolateCubic, not the product."""
    from oracle.joint_oracle import _cubic_coeffs
    rs = np.random.RandomState(0)
    ts = np.concatenate([np.linspace(0, 1, 4097)[:-1], rs.uniform(0, 1, 4000), [2.0 ** -20, 1 - 2.0 ** -24]]).astype(np.float32)
    worst = 0.0
    for t in ts:
        w32 = _cubic_coeffs(t).astype(np.float64)
        worst = max(worst, float(np.abs(w32 - ar.cubic_weights64(np.float64(t))).sum()))
    assert worst <= ar.W_AXIS * ar.U24, worst / ar.U24
    assert max(float(np.abs(ar.cubic_weights64(t)).sum()) for t in np.linspace(0, 1, 1001)) <= 1.375


def _sources(i, c):
    return ar.synth_sources(40 + i, int(c["hw"][0]), int(c["hw"][1]))


def _ref_geo(c):
    o = (int(c["center"][0]) + INP // 2 - INP, int(c["center"][1]) + INP // 2 - INP)
    return ar.geometry(c["M"], c["scale"], c["stage_shapes"][0][:2], c["stage_shapes"][1][:2], o, int(c["flip"]))


FAULTS = {
    "A = -0.5": dict(A=-0.5),
    "taps shifted by one": dict(tap_shift=1),
    "half-pixel coordinate offset": dict(coord_off=0.5),
    "no BGR -> RGB swap": dict(swap=False),
    "flip over the wrong width": dict(flip_w="other"),
}


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_bound_of_the_gpu_test_has_teeth(fault):
    """The bound test_augment_gpu applies (augment_ref.bound) is violated by each modelled fault on every golden case the fault
    applies to (the flip fault on the flipped cases, the channel fault on the image): by a factor above 100 somewhere in the image and
    on more than 5 % of its elements, by a factor above 10 somewhere in the mask (case 5 shows little but pad)."""
    kw = dict(FAULTS[fault])
    gh = INP // STRIDE
    hit = 0
    for i, c in enumerate(CASES):
        geo = _ref_geo(c)
        img, mask = _sources(i, c)
        if "flip_w" in kw:
            if not geo["flip"]:
                continue
            ikw, mkw = dict(flip_w=INP + 1), dict(flip_w=INP)             # each one flipped over the other's width
        else:
            ikw, mkw = kw, {k: v for k, v in kw.items() if k != "swap"}
        ref, mag, wabs = ar.image_ref(img, geo, INP, INP)
        bad, _, _ = ar.image_ref(img, geo, INP, INP, **ikw)
        ratio = ar.ratio(bad, ref, mag, wabs, ar.C_SUM_IMAGE)
        assert ratio.max() > 100 and (ratio > 1).mean() > 0.05, (fault, i, ratio.max(), (ratio > 1).mean())
        hit += 1
        if "swap" in kw:
            continue
        ref, mag, wabs = ar.mask_ref(mask, geo, gh, gh, STRIDE, INP)
        bad, _, _ = ar.mask_ref(mask, geo, gh, gh, STRIDE, INP, **mkw)
        ratio = ar.ratio(bad, ref, mag, wabs, ar.C_SUM_MASK)
        assert ratio.max() > 10, (fault, i, "mask", ratio.max())
    assert hit >= 3


def test_restatement_agrees_with_itself_and_with_plain_geometry():
    """Sanity of augment_ref: the unfaulted reference meets its own bound trivially, pad is exactly the normalised 128 / 1.0, and
    where the transform is the identity (scale 1, 0 degrees, crop inside the image) it returns the source pixels."""
    H, W = 600, 640
    img, mask = ar.synth_sources(3, H, W)
    g = aug.augment_meta(H, W, 0.6, (320.0, 300.0), np.ones((18, 3)), np.zeros((0, 18, 3)), [0.7, np.nan, 0.5, 0.5, 0.5, 0.9], 64, 64,
                         dict(aug.DEFAULT_PARAMS, scale_prob=0.0))
    assert g["scale"] == 1.0 and (g["nH"], g["nW"]) == (H, W) and np.array_equal(g["M"], [[1, 0, 0], [0, 1, 0]])
    geo = ar.geometry(g["M"], g["scale"], (g["nh"], g["nw"]), (g["nH"], g["nW"]), (g["ox"], g["oy"]), g["flip"])
    ref, _, _ = ar.image_ref(img, geo, 64, 64)
    crop = img[g["oy"]:g["oy"] + 64, g["ox"]:g["ox"] + 64, ::-1].astype(np.float64).transpose(2, 0, 1)
    mean = np.array(ar.MEANS, dtype=np.float32).astype(np.float64)[:, None, None]
    std = np.array(ar.STDS, dtype=np.float32).astype(np.float64)[:, None, None]
    assert np.array_equal(ref, (crop / 255.0 - mean) / std)
    m1, _, _ = ar.mask_ref(mask, geo, 64, 64, 1, 64)
    assert np.array_equal(m1, mask[g["oy"]:g["oy"] + 64, g["ox"]:g["ox"] + 64] / 255.0)
