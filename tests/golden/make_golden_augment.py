#!/usr/bin/env python3
"""Golden vectors for the geometry of the training augmentation, produced by the REAL reference functions
datasets/coco_data/ImageAugmentation.py: aug_scale, aug_rotate (rotate_bound, rotatepoint), aug_croppad, aug_flip and
datasets/coco_data/COCO_data_pipeline.py: Cocokeypoints.add_neck / remove_illegal_joint (build container only; the
reference is not on the GPU box).

Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_augment.py

Only the META-DATA side is pinned: where every joint lands, every stage's shape, the matrix handed to warpAffine, the
crop, the flip.  The reference's modules import cv2, matplotlib, scipy and pycocotools at module scope (all absent
here); stand-ins are pre-seeded:
  * cv2.resize / warpAffine / flip produce arrays of the right SHAPE only and record their arguments.  Two assumptions
    about the real cv2 sit in the resize stand-in and are NOT verified against a real cv2: with dsize (0, 0) and fx, fy
    given, dsize = (round(w * fx), round(h * fy)) (cvRound: half to even, like Python's round), and coordinates map with
    1 / fx (not with the ratio of the sizes).
  * cv2.getRotationMatrix2D is the documented formula: alpha = scale cos(angle), beta = scale sin(angle),
    [[alpha, beta, (1 - alpha) cx - beta cy], [-beta, alpha, beta cx + (1 - alpha) cy]], angle in degrees.
  * matplotlib / scipy / pycocotools are empty modules.
random.random is patched to record the dice each function draws, either from random.Random(seed) (so the draw ORDER
is pinned) or from a scripted list (so the corner cases are hit on purpose).
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
    CALLS.append(("resize", src.shape, out.shape, float(fx), float(fy)))
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
    CALLS.append(("flip", src.shape, flipCode))
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

# (H, W, scale_provided, others, objpos as a fraction of (W, H), seed or None, scripted dice, parameter overrides)
# dice order: scale dice, scale dice2, rotate, croppad x, croppad y, flip
CASES = [
    (427, 640, 0.71, 2, (0.45, 0.55), 1, None, {}),                                          # the plain case, seeded stream
    (480, 640, 0.40, 0, (0.50, 0.50), None, [0.3, 0.9, 0.995, 0.2, 0.7, 0.10], {}),          # scale > 1, +39.6 deg, flip, nobody else
    (375, 500, 1.30, 3, (0.60, 0.40), None, [0.6, 0.1, 0.004, 0.9, 0.1, 0.85], {}),          # scale < 1, -39.7 deg, odd sizes
    (333, 517, 0.65, 1, (0.30, 0.60), None, [0.5, 0.5, 0.5004, 0.5, 0.5, 0.30], {}),         # ~0 deg, flip at dice == flip_prob, odd sizes
    (480, 640, 0.55, 1, (0.01, 0.02), 7, None, {}),                                          # person in the top-left corner: pad visible
    (427, 640, 0.80, 2, (0.99, 0.98), None, [0.2, 0.4, 0.25, 0.99, 0.99, 0.05], {}),         # bottom-right corner, flipped
    (500, 375, 0.60, 5, (0.50, 0.50), 3, None, {"scale_prob": 0.5, "flip_prob": 0.5}),       # dice2 drawn only when dice <= scale_prob
    (640, 427, 0.25, 0, (0.40, 0.50), 11, None, {}),                                         # portrait, scale 1.9 .. 2.9
    (301, 299, 0.60, 4, (0.55, 0.45), 5, None, {"scale_prob": 0.0}),                         # scale_prob 0: dice2 never drawn
]


def make_meta(seed, H, W, n_other, objfrac):
    rs = np.random.RandomState(seed)

    def person():
        j = np.zeros((17, 3), dtype=np.float64)
        j[:, 0] = np.round(rs.uniform(-0.05 * W, 1.05 * W, size=17))
        j[:, 1] = np.round(rs.uniform(-0.05 * H, 1.05 * H, size=17))
        j[:, 2] = rs.choice([0.0, 1.0, 2.0], size=17, p=[0.3, 0.5, 0.2])
        return j
    meta = {"objpos": np.array([objfrac[0] * W, objfrac[1] * H], dtype=np.float64), "joint_self": person(),
            "numOtherPeople": n_other,
            "joint_others": np.stack([person() for _ in range(n_other)]) if n_other else np.zeros((0, 17, 3)),
            "objpos_other": rs.uniform(0, 1, size=(n_other, 2)) * np.array([W, H], dtype=np.float64)}
    return meta


def run_case(idx, H, W, sp, n_other, objfrac, seed, script, over):
    pt = dict(CP.params_transform)
    pt.update({"crop_size_x": INP, "crop_size_y": INP, "stride": STRIDE})
    pt.update(over)
    CP.params_transform.update(pt)                      # remove_illegal_joint reads the module's dict
    meta = make_meta(100 + idx, H, W, n_other, objfrac)
    meta["scale_provided"] = sp
    rec = {"hw": np.array([H, W], dtype=np.int64), "scale_provided": np.float64(sp), "objpos_in": meta["objpos"].copy(),
           "joint_self_in": meta["joint_self"].copy(), "joint_others_in": meta["joint_others"].copy(),
           "objpos_other_in": meta["objpos_other"].copy(), "seed": np.int64(-1 if seed is None else seed),
           "params": np.array([pt[k] for k in ("scale_min", "scale_max", "scale_prob", "target_dist", "max_rotate_degree",
                                               "center_perterb_max", "flip_prob")], dtype=np.float64)}
    meta = CP.Cocokeypoints.add_neck(None, meta)
    rec["joint_self_neck"] = meta["joint_self"].copy()
    rec["joint_others_neck"] = np.asarray(meta["joint_others"], dtype=np.float64).reshape(n_other, 18, 3).copy()

    src = random.Random(seed).random if seed is not None else iter(script).__next__
    drawn = []

    def rec_random():
        v = src()
        drawn.append((sys._getframe(1).f_code.co_name, v))
        return v
    real, random.random = random.random, rec_random
    del CALLS[:]
    try:
        img, mask = np.zeros((H, W, 3), dtype=np.uint8), np.zeros((H, W), dtype=np.uint8)
        shapes = []
        for f in (IA.aug_scale, IA.aug_rotate, IA.aug_croppad, IA.aug_flip):
            meta, img, mask = f(meta, img, mask, pt)
            shapes.append(img.shape[:2] + mask.shape[:2])
            if f is IA.aug_rotate:
                rec["objpos_rot"] = meta["objpos"].copy()
            if f is IA.aug_croppad:
                rec["joint_self_crop"] = meta["joint_self"].copy()
                rec["objpos_crop"] = meta["objpos"].copy()
    finally:
        random.random = real
    # the dice in the fixed layout of the product's helper; NaN = not drawn
    dice = np.full(6, np.nan)
    slot = {"aug_rotate": [2], "aug_croppad": [3, 4], "aug_flip": [5]}
    sc = [v for n, v in drawn if n == "aug_scale"]
    dice[:len(sc)] = sc
    for n, lst in slot.items():
        vals = [v for m, v in drawn if m == n]
        assert len(vals) == len(lst), (n, vals)
        dice[lst] = vals
    assert [n for n, _ in drawn] == ["aug_scale"] * len(sc) + ["aug_rotate", "aug_croppad", "aug_croppad", "aug_flip"]
    rec["dice"] = dice
    rec["stage_shapes"] = np.array(shapes, dtype=np.int64)             # rows: scale, rotate, croppad, flip; (img h, w, mask h, w)
    warps = [c for c in CALLS if c[0] == "warpAffine"]
    assert len(warps) == 2 and np.array_equal(warps[0][3], warps[1][3])
    rec["M"] = warps[0][3]
    rs = [c for c in CALLS if c[0] == "resize"]
    rec["scale"] = np.float64(rs[0][3])
    rec["flip"] = np.int64(any(c[0] == "flip" for c in CALLS))
    rec["mask_grid"] = np.array(_resize(mask, (0, 0), fx=1.0 / STRIDE, fy=1.0 / STRIDE).shape, dtype=np.int64)   # COCO_data_pipeline.py:211
    # aug_croppad's integer crop centre is a local of the function; it moves objpos by crop / 2 - center (ImageAugmentation.py:96-100),
    # an integer here, so it is read back from the real function's own output
    shift = np.round(rec["objpos_crop"] - rec["objpos_rot"])
    assert np.abs(shift - (rec["objpos_crop"] - rec["objpos_rot"])).max() < 1e-6 and INP % 2 == 0
    rec["center"] = (INP // 2 - shift).astype(np.int64)
    rec["objpos_flip"] = meta["objpos"].copy()
    rec["joint_self_flip"] = meta["joint_self"].copy()
    rec["joint_others_flip"] = np.asarray(meta["joint_others"], dtype=np.float64).reshape(n_other, 18, 3).copy()
    meta = CP.Cocokeypoints.remove_illegal_joint(None, meta)
    rec["joint_self_out"] = meta["joint_self"].copy()
    rec["joint_others_out"] = np.asarray(meta["joint_others"], dtype=np.float64).reshape(n_other, 18, 3).copy()
    return rec


def main():
    data = {"n_cases": np.int64(len(CASES)), "inp_stride": np.array([INP, STRIDE], dtype=np.int64)}
    for i, case in enumerate(CASES):
        for k, v in run_case(i, *case).items():
            data["c%d_%s" % (i, k)] = v
        print("case %d: dice %s stages %s flip %d" % (i, np.round(data["c%d_dice" % i], 4).tolist(),
                                                      data["c%d_stage_shapes" % i].tolist(), data["c%d_flip" % i]))
    path = os.path.join(HERE, "g17_augment.npz")
    with open(path, "wb") as f:                        # np.savez_compressed through a file object: no timestamps, byte-stable
        np.savez_compressed(f, **data)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
