#!/usr/bin/env python3
"""Golden vectors for the geometry of the DETECTION loader's augmentation, produced by the REAL reference functions
datasets/coco_data/ImageAugmentation.py: aug_scale_bbox, aug_rotate_bbox (rotate_bound), aug_croppad_bbox, aug_flip_bbox and
datasets/coco_data/COCO_data_pipeline.py: Cocobbox.get_ground_truth, bbox_collater (build container only; the reference is
not on the GPU box).

Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_augment_bbox.py

Same stand-in technique as make_golden_augment.py (see there for the two unverified assumptions about cv2.resize):
  * cv2.resize / warpAffine produce arrays of the right SHAPE only and record their arguments; cv2.getRotationMatrix2D is the
    documented formula; cv2.flip REALLY flips (flipCode 1, into dst), because here the pixels carry information:
  * the instance mask handed to aug_croppad_bbox is an INDEX RAMP (pixel (y, x) of the rotated canvas holds 1 + y * nW + x, int64),
    planted between aug_rotate_bbox and aug_croppad_bbox.  The real pads, slices and flip then move real numbers, and the canvas
    coordinate of every pixel of the final mask is read back from the real functions' own output: the crop origin, the integer crop
    centre (a local of aug_croppad_bbox that it never writes to meta), the (crop + 1)^2 frame and the flip over the mask's own width.
random.random is patched to record the dice each function draws, from random.Random(seed) or from a scripted list.

Second part: the real Cocobbox.get_ground_truth(None, meta, instance_info) and bbox_collater on small hand-made FINAL masks.
"""
import math
import os
import random
import sys
import types

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference")

import numpy as np  # noqa: E402

CALLS = []


def _resize(src, dsize, fx=0, fy=0, interpolation=None):
    assert tuple(dsize) == (0, 0)
    h, w = src.shape[:2]
    out = np.zeros((int(round(h * fy)), int(round(w * fx))) + src.shape[2:], dtype=src.dtype)
    CALLS.append(("resize", src.shape, out.shape, float(fx), float(fy), interpolation))
    return out


def _rotation_matrix(center, angle, scale):
    a = float(angle) * math.pi / 180.0
    alpha, beta = math.cos(a) * scale, math.sin(a) * scale
    cx, cy = float(center[0]), float(center[1])
    return np.array([[alpha, beta, (1 - alpha) * cx - beta * cy], [-beta, alpha, beta * cx + (1 - alpha) * cy]], dtype=np.float64)


def _warp_affine(src, M, dsize, flags=None, borderMode=None, borderValue=None):
    out = np.zeros((int(dsize[1]), int(dsize[0])) + src.shape[2:], dtype=src.dtype)
    CALLS.append(("warpAffine", src.shape, out.shape, np.array(M, dtype=np.float64).copy(), borderValue))
    return out


def _flip(src, flipCode, dst=None):
    assert flipCode == 1 and dst is not None
    CALLS.append(("flip", src.shape, flipCode))
    dst[...] = src[:, ::-1].copy()
    return dst


cv2 = types.ModuleType("cv2")
cv2.resize, cv2.getRotationMatrix2D, cv2.warpAffine, cv2.flip = _resize, _rotation_matrix, _warp_affine, _flip
cv2.INTER_CUBIC, cv2.INTER_AREA, cv2.BORDER_CONSTANT = 2, 3, 0
sys.modules["cv2"] = cv2
for name in ("matplotlib", "matplotlib.pyplot", "scipy", "scipy.misc", "scipy.ndimage", "pycocotools", "pycocotools.coco"):
    sys.modules[name] = types.ModuleType(name)
sys.modules["matplotlib"].pyplot = sys.modules["matplotlib.pyplot"]
sys.modules["scipy"].misc, sys.modules["scipy"].ndimage = sys.modules["scipy.misc"], sys.modules["scipy.ndimage"]
sys.modules["pycocotools.coco"].COCO = sys.modules["pycocotools.coco"].maskUtils = object

from datasets.coco_data import ImageAugmentation as IA  # noqa: E402
from datasets.coco_data import COCO_data_pipeline as CP  # noqa: E402

INP, STRIDE = 480, 4

# (H, W, scale_provided, objpos as a fraction of (W, H), seed or None, scripted dice, parameter overrides)
# dice order: scale dice, scale dice2, rotate, croppad x, croppad y, flip
CASES = [
    (427, 640, 0.71, (0.45, 0.55), 1, None, {}),                                          # the plain case, seeded stream
    (480, 640, 0.40, (0.50, 0.50), None, [0.3, 0.9, 1.0, 0.2, 0.7, 0.10], {}),            # scale > 1, +40 deg, flip
    (375, 500, 1.30, (0.60, 0.40), None, [0.6, 0.1, 0.0, 0.9, 0.1, 0.85], {}),            # scale < 1, -40 deg, odd sizes
    (333, 517, 0.65, (0.30, 0.60), None, [0.5, 0.5, 0.5004, 0.5, 0.5, 0.30], {}),         # ~0 deg, flip at dice == flip_prob, odd sizes
    (480, 640, 0.55, (0.01, 0.02), 7, None, {}),                                          # objpos in the top-left corner: pad visible
    (427, 640, 0.80, (0.99, 0.98), None, [0.2, 0.4, 0.25, 0.99, 0.99, 0.05], {}),         # bottom-right corner, flipped, -20 deg
    (500, 375, 0.60, (0.50, 0.50), 3, None, {"scale_prob": 0.5, "flip_prob": 0.5}),       # dice2 drawn only when dice <= scale_prob
    (640, 427, 0.25, (0.40, 0.50), 11, None, {}),                                         # portrait, scale 1.9 .. 2.9
    (301, 299, 0.60, (0.55, 0.45), 5, None, {"scale_prob": 0.0}),                         # scale_prob 0: dice2 never drawn
    (480, 640, 0.50, (0.20, 0.30), None, [0.1, 0.75, 0.9, 0.0, 1.0, 0.31], {}),           # off-centre, +32 deg, perturbation extremes, no flip just above flip_prob
]


def run_case(idx, H, W, sp, objfrac, seed, script, over):
    pt = dict(CP.params_transform)
    pt.update({"crop_size_x": INP, "crop_size_y": INP, "stride": STRIDE})
    pt.update(over)
    n_inst = 2
    meta = {"objpos": np.array([objfrac[0] * W, objfrac[1] * H], dtype=np.float64), "scale_provided": sp,
            "instance_mask_list": [np.zeros((H, W), dtype=np.int64) for _ in range(n_inst)]}
    rec = {"hw": np.array([H, W], dtype=np.int64), "scale_provided": np.float64(sp), "objpos_in": meta["objpos"].copy(),
           "seed": np.int64(-1 if seed is None else seed),
           "params": np.array([pt[k] for k in ("scale_min", "scale_max", "scale_prob", "target_dist", "max_rotate_degree",
                                               "center_perterb_max", "flip_prob")], dtype=np.float64)}
    src = random.Random(seed).random if seed is not None else iter(script).__next__
    drawn = []

    def rec_random():
        v = src()
        drawn.append((sys._getframe(1).f_code.co_name, v))
        return v
    real, random.random = random.random, rec_random
    del CALLS[:]
    try:
        img = np.zeros((H, W, 3), dtype=np.uint8)
        shapes = []
        for f in (IA.aug_scale_bbox, IA.aug_rotate_bbox, IA.aug_croppad_bbox, IA.aug_flip_bbox):
            if f is IA.aug_croppad_bbox:
                nH, nW = meta["instance_mask_list"][0].shape
                ramp = 1 + np.arange(nH * nW, dtype=np.int64).reshape(nH, nW)
                meta["instance_mask_list"] = [ramp.copy() for _ in range(n_inst)]
            meta, img = f(meta, img, pt)
            assert len(meta["instance_mask_list"]) == n_inst and all(m.shape == meta["instance_mask_list"][0].shape
                                                                      for m in meta["instance_mask_list"])
            shapes.append(img.shape[:2] + meta["instance_mask_list"][0].shape[:2])
            rec["objpos_" + f.__name__[4:-5]] = np.array(meta["objpos"], dtype=np.float64).copy()
            if f is IA.aug_croppad_bbox:
                crop_mask = meta["instance_mask_list"][0].copy()
    finally:
        random.random = real
    dice = np.full(6, np.nan)
    slot = {"aug_rotate_bbox": [2], "aug_croppad_bbox": [3, 4], "aug_flip_bbox": [5]}
    sc = [v for n, v in drawn if n == "aug_scale_bbox"]
    dice[:len(sc)] = sc
    for n, lst in slot.items():
        vals = [v for m, v in drawn if m == n]
        assert len(vals) == len(lst), (n, vals)
        dice[lst] = vals
    assert [n for n, _ in drawn] == ["aug_scale_bbox"] * len(sc) + ["aug_rotate_bbox", "aug_croppad_bbox", "aug_croppad_bbox", "aug_flip_bbox"]
    rec["dice"] = dice
    rec["stage_shapes"] = np.array(shapes, dtype=np.int64)            # rows: scale, rotate, croppad, flip; (img h, w, mask h, w)
    warps = [c for c in CALLS if c[0] == "warpAffine"]
    assert len(warps) == 1 + n_inst and all(np.array_equal(warps[0][3], w[3]) for w in warps)      # masks and image share M
    assert warps[0][4] == (128, 128, 128) and all(w[4] == 0 for w in warps[1:])
    rec["M"] = warps[0][3]
    rs = [c for c in CALLS if c[0] == "resize"]
    assert len(rs) == 1 + n_inst and all(c[3] == rs[0][3] and c[4] == rs[0][3] and c[2][:2] == rs[0][2][:2] for c in rs)
    assert rs[0][5] == cv2.INTER_CUBIC and all(c[5] == cv2.INTER_AREA for c in rs[1:])
    rec["scale"] = np.float64(rs[0][3])
    flips = [c for c in CALLS if c[0] == "flip"]
    assert len(flips) in (0, 1 + n_inst)
    rec["flip"] = np.int64(len(flips) > 0)

    # read the geometry back from the ramp.  Canvas pixel of a ramp value r > 0: ((r - 1) % nW, (r - 1) // nW).
    def canvas(m):
        x = np.where(m > 0, (m - 1) % nW, -1)
        y = np.where(m > 0, (m - 1) // nW, -1)
        return x, y
    assert crop_mask.shape == (INP + 1, INP + 1)
    cx, cy = canvas(crop_mask)
    v, u = np.nonzero(crop_mask)
    assert v.size > 0, "the crop shows no canvas pixel: pick another case"
    ox, oy = cx[v[0], u[0]] - u[0], cy[v[0], u[0]] - v[0]
    assert np.all(cx[v, u] - u == ox) and np.all(cy[v, u] - v == oy)
    # every canvas pixel that the frame covers is there, everything else is the pad's 0
    uu, vv = np.meshgrid(np.arange(INP + 1), np.arange(INP + 1))
    want_in = (uu + ox >= 0) & (uu + ox < nW) & (vv + oy >= 0) & (vv + oy < nH)
    assert np.array_equal(want_in, crop_mask > 0)
    rec["origin"] = np.array([ox, oy], dtype=np.int64)                # canvas pixel of mask-crop pixel (0, 0)
    assert INP % 2 == 0
    rec["center"] = np.array([ox + INP - INP // 2, oy + INP - INP // 2], dtype=np.int64)     # slice start = center + int(crop / 2) - crop
    final = meta["instance_mask_list"][0]
    assert final.shape == (INP + 1, INP + 1)
    fx, fy = canvas(final)
    # canvas x of the final mask's columns along its first row that shows the canvas (-1 = pad): pins the flip over crop_x + 1 columns
    rec["final_row"] = np.int64(v[0])
    rec["final_row_canvas_x"] = fx[v[0]].astype(np.int64)
    rec["final_col0_canvas_y"] = fy[:, u[0] if not rec["flip"] else INP - u[0]].astype(np.int64)
    return rec


def _mask(S, ys, xs):
    m = np.zeros((S + 1, S + 1), dtype=np.uint8)
    m[ys, xs] = 1
    return m


def ground_truth_cases():
    """Hand-made FINAL masks (9 x 9: crop 8) per image -> the real get_ground_truth and bbox_collater."""
    import torch
    S = 8
    full = np.ones((S + 1, S + 1), dtype=np.uint8)
    empty = np.zeros((S + 1, S + 1), dtype=np.uint8)
    images = [
        # (masks, cls list: 1 or -1 for a crowd)
        ([full, _mask(S, 3, 5), empty], [1, 1, 1]),
        ([_mask(S, slice(0, 2), slice(2, 5)), _mask(S, slice(7, 9), slice(1, 3)), _mask(S, slice(2, 4), slice(0, 1)),
          _mask(S, slice(4, 6), slice(8, 9))], [1, 1, 1, 1]),                                  # touching top, bottom, left, right
        ([_mask(S, slice(1, 4), slice(1, 4)), full, _mask(S, slice(5, 8), slice(2, 7))], [1, -1, 1]),   # a crowd in the middle
        ([full], [-1]),                                                                        # an image with no rows
    ]
    data = {"gt_n_images": np.int64(len(images)), "gt_crop": np.int64(S)}
    items = []
    for i, (masks, cls) in enumerate(images):
        meta = {"instance_mask_list": masks, "instance_cls_list": cls}
        info = {"anns": [{"iscrowd": 1 if c == -1 else 0} for c in cls]}
        rows = CP.Cocobbox.get_ground_truth(None, meta, info)
        data["gt%d_masks" % i] = np.stack(masks)
        data["gt%d_iscrowd" % i] = np.array([a["iscrowd"] for a in info["anns"]], dtype=np.int64)
        data["gt%d_rows" % i] = np.array(rows, dtype=np.float64).reshape(-1, 5)
        bbox = torch.from_numpy(np.array(rows).astype(np.float32))               # Cocobbox.__getitem__, COCO_data_pipeline.py:437
        items.append((torch.zeros(1), bbox))
    _, padded = CP.bbox_collater(items)
    data["gt_collated"] = padded.numpy().astype(np.float32)
    _, none = CP.bbox_collater([items[3], items[3]])
    data["gt_collated_no_rows_shape"] = np.array(none.shape, dtype=np.int64)
    return data


def main():
    data = {"n_cases": np.int64(len(CASES)), "inp_stride": np.array([INP, STRIDE], dtype=np.int64)}
    for i, case in enumerate(CASES):
        for k, v in run_case(i, *case).items():
            data["c%d_%s" % (i, k)] = v
        print("case %d: dice %s stages %s flip %d origin %s center %s" % (
            i, np.round(data["c%d_dice" % i], 4).tolist(), data["c%d_stage_shapes" % i].tolist(), data["c%d_flip" % i],
            data["c%d_origin" % i].tolist(), data["c%d_center" % i].tolist()))
    data.update(ground_truth_cases())
    print("collated", data["gt_collated"].shape, "no rows", data["gt_collated_no_rows_shape"].tolist())
    path = os.path.join(HERE, "g19_augment_bbox.npz")
    with open(path, "wb") as f:                        # np.savez_compressed through a file object: no timestamps, byte-stable
        np.savez_compressed(f, **data)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
