"""Training augmentation of keypoint batches on the GPU, from raw uint8 images.

Device replacement for what the reference's ``Cocokeypoints.__getitem__`` (``datasets/coco_data/COCO_data_pipeline.py:238-291``)
does per image on the host between the decoded image and the tensors of a batch: ``aug_scale``, ``aug_rotate``,
``aug_croppad``, ``aug_flip`` (``datasets/coco_data/ImageAugmentation.py:25-231``), the mask's second resize
(``COCO_data_pipeline.py:211-215``) and ``resnet_preprocess`` (``preprocessing.py:15-26``).

Two halves:

* the META-DATA side (where every joint lands, every stage's size, the matrix handed to ``warpAffine``, the crop, the flip) is
  restated here op for op in numpy float64 — :func:`add_neck`, :func:`augment_meta`, :func:`remove_illegal_joint` — with the
  random draws as an explicit input (:func:`draw_dice` draws them from a ``random.Random`` in the reference's order);
* the PIXEL side runs in csrc/augment.hip: every output element is mapped through the composed inverse transform to a source
  coordinate and sampled ONCE with the 4x4 cubic kernel, without the intermediate uint8 images of the reference and without
  rounding (DESIGN.md section 7 states the deviation).  :class:`DeviceAugmenter` packs a batch, launches the two kernels and
  renders the heat-maps with :func:`..heatmap.put_gaussian_maps`.

Detection batches (``Cocobbox``, ``COCO_data_pipeline.py:296-458``) go through the ``aug_*_bbox`` chain
(``ImageAugmentation.py:234-340``), whose geometry is NOT the keypoint chain's: ``aug_rotate_bbox`` never rotates ``objpos``, so the
crop is centred elsewhere.  :func:`augment_meta_bbox` restates that chain, :class:`DeviceBBoxAugmenter` packs the instance masks'
bounding rectangles and ``mpn_augment_boxes`` reads every instance's box off the composed transform without warping a mask.

Decoding the image files and reading the COCO json stay with the loader.
"""
import ctypes
import math
import random

import numpy as np
import torch

from .._lib import MpnError, call
from .. import ops
from . import segm
from .heatmap import put_gaussian_maps

# COCO_data_pipeline.py:25-42
DEFAULT_PARAMS = {
    "mode": 5,
    "scale_min": 0.8, "scale_max": 1.2, "scale_prob": 1, "target_dist": 0.6,
    "max_rotate_degree": 40,
    "center_perterb_max": 40,
    "flip_prob": 0.3,
    "np": 56, "sigma": 7.0,
}

# preprocessing.py:17-18 (RGB order)
MEANS = (0.485, 0.456, 0.406)
STDS = (0.229, 0.224, 0.225)

# COCO_data_pipeline.py:138-139 and ImageAugmentation.py:148-149
OUR_ORDER = [0, 17, 6, 8, 10, 5, 7, 9, 12, 14, 16, 11, 13, 15, 2, 1, 4, 3]
FLIP_ORDER = [0, 1, 5, 6, 7, 2, 3, 4, 11, 12, 13, 8, 9, 10, 15, 14, 17, 16]

# dice layout: aug_scale dice, aug_scale dice2 (NaN when not drawn), aug_rotate dice, aug_croppad dice_x, dice_y, aug_flip dice
N_DICE = 6

# columns of the per-sample table the kernels read (include/mpn.h: MPN_AUG_*)
T_IMG_OFF, T_IMG_PITCH, T_MASK_OFF, T_MASK_PITCH, T_H, T_W, T_SCALE, T_NW, T_NH, T_CW, T_CH = range(11)
T_MINV, T_OX, T_OY, T_FLIP, T_COLS = 11, 17, 18, 19, 20
# columns an instance row of mpn_augment_boxes adds (MPN_AUGB_*): the instance's bounding rectangle inside its H x W source
TB_RX0, TB_RY0, TB_RW, TB_RH, TB_COLS = 20, 21, 22, 23, 24


def draw_dice(rng, params=None):
    """The six draws of one sample from ``rng`` (a ``random.Random`` or the ``random`` module) in the reference's order: aug_scale's
    ``dice`` and — only when ``dice <= scale_prob`` — ``dice2`` (ImageAugmentation.py:26-31), aug_rotate's ``dice`` (:206), aug_croppad's
    ``dice_x``, ``dice_y`` (:56-57), aug_flip's ``dice`` (:124).  The same seed gives the reference's stream."""
    p = DEFAULT_PARAMS if params is None else params
    d = np.full(N_DICE, np.nan, dtype=np.float64)
    d[0] = rng.random()
    if not d[0] > p["scale_prob"]:
        d[1] = rng.random()
    d[2] = rng.random()
    d[3] = rng.random()
    d[4] = rng.random()
    d[5] = rng.random()
    return d


def _neck(right_shoulder, left_shoulder):
    neck = (right_shoulder + left_shoulder) / 2
    if right_shoulder[2] == 2 or left_shoulder[2] == 2:
        neck[2] = 2
    elif right_shoulder[2] == 1 or left_shoulder[2] == 1:
        neck[2] = 1
    else:
        neck[2] = right_shoulder[2] * left_shoulder[2]
    return np.round(neck.reshape(1, len(neck)))


def add_neck(joint_self, joint_others):
    """COCO_data_pipeline.py:123-174: 17 COCO keypoints -> the 18 of this work (neck = rounded mean of the shoulders, visibility by
    the reference's rule), re-ordered.  joint_self [17, 3], joint_others [n, 17, 3] -> ([18, 3], [n, 18, 3]) float64."""
    js = np.array(joint_self, dtype=np.float64)
    jo = np.array(joint_others, dtype=np.float64).reshape(-1, 17, 3)
    js = np.vstack((js, _neck(js[6, :], js[5, :])))[OUR_ORDER, :]
    out = np.zeros((jo.shape[0], 18, 3), dtype=np.float64)
    for i in range(jo.shape[0]):
        out[i] = np.vstack((jo[i], _neck(jo[i, 6, :], jo[i, 5, :])))[OUR_ORDER, :]
    return js, out


def remove_illegal_joint(joint_self, joint_others, crop_x, crop_y):
    """COCO_data_pipeline.py:176-194: joints outside the crop become (1, 1, 2).  Returns new arrays."""
    js, jo = joint_self.copy(), joint_others.copy()
    for j in (js, jo):
        if j.size == 0:
            continue
        mask = np.logical_or.reduce((j[..., 0] >= crop_x, j[..., 0] < 0, j[..., 1] >= crop_y, j[..., 1] < 0))
        j[mask, :] = (1, 1, 2)
    return js, jo


def rotation_matrix(center, angle, scale):
    """The documented cv2.getRotationMatrix2D: angle in degrees, positive = counter-clockwise."""
    a = float(angle) * math.pi / 180.0
    alpha, beta = math.cos(a) * scale, math.sin(a) * scale
    cx, cy = float(center[0]), float(center[1])
    return np.array([[alpha, beta, (1 - alpha) * cx - beta * cy], [-beta, alpha, beta * cx + (1 - alpha) * cy]], dtype=np.float64)


def invert_affine(M):
    """Inverse of a 2x3 affine map in the operation order of warpAffine's own inversion (imgproc/imgwarp.cpp)."""
    M = np.array(M, dtype=np.float64)
    D = M[0, 0] * M[1, 1] - M[0, 1] * M[1, 0]
    D = 1.0 / D if D != 0 else 0.0
    A11, A22 = M[1, 1] * D, M[0, 0] * D
    iM = np.zeros((2, 3), dtype=np.float64)
    iM[0, 0], iM[0, 1], iM[1, 0], iM[1, 1] = A11, M[0, 1] * (-D), M[1, 0] * (-D), A22
    iM[0, 2] = -iM[0, 0] * M[0, 2] - iM[0, 1] * M[1, 2]
    iM[1, 2] = -iM[1, 0] * M[0, 2] - iM[1, 1] * M[1, 2]
    return iM


def _rotatepoint(p, R):
    # ImageAugmentation.py:161-172 (the same [2, 3] x [3, 1] product, so the same rounding)
    point = np.zeros((3, 1))
    point[0] = p[0]
    point[1] = p[1]
    point[2] = 1
    new_point = R.dot(point)
    p[0] = new_point[0, 0]
    p[1] = new_point[1, 0]
    return p


def _sample_dice(dice):
    dice = np.asarray(dice, dtype=np.float64)
    if dice.shape != (N_DICE,):
        raise MpnError("dice must hold %d draws per sample" % N_DICE)
    return dice


def _scale_and_canvas(H, W, scale_provided, dice, p):
    """What both chains do before anything is cropped: aug_scale / aug_scale_bbox (ImageAugmentation.py:25-52, :234-257) and
    rotate_bound (:179-202).  Returns the geometry dict with ``scale``, the scaled size ``(nh, nw)``, ``degree``, the matrix ``M``
    handed to warpAffine with ``Minv``, and the canvas size ``(nH, nW)``."""
    if dice[0] > p["scale_prob"]:
        scale_multiplier = 1
    else:
        if np.isnan(dice[1]):
            raise MpnError("dice[1] (aug_scale's dice2) is needed when dice[0] <= scale_prob")
        scale_multiplier = (p["scale_max"] - p["scale_min"]) * float(dice[1]) + p["scale_min"]
    scale_abs = p["target_dist"] / scale_provided
    scale = scale_abs * scale_multiplier
    if not (scale > 0 and math.isfinite(scale)):
        raise MpnError("scale_provided gives a non-positive or non-finite scale")
    nh, nw = int(round(H * scale)), int(round(W * scale))            # cv2.resize with fx, fy: dsize = round(size * f)
    if nh < 1 or nw < 1:
        raise MpnError("the scaled image is empty")
    degree = (float(dice[2]) - 0.5) * 2 * p["max_rotate_degree"]
    cX, cY = nw // 2, nh // 2
    M = rotation_matrix((cX, cY), -degree, 1.0)
    cos, sin = np.abs(M[0, 0]), np.abs(M[0, 1])
    nW = int((nh * sin) + (nw * cos))
    nH = int((nh * cos) + (nw * sin))
    M[0, 2] += (nW / 2) - cX
    M[1, 2] += (nH / 2) - cY
    return {"scale": float(scale), "nh": nh, "nw": nw, "nH": nH, "nW": nW, "M": M, "Minv": invert_affine(M), "degree": degree}


def _crop_origin(point, dice, crop_x, crop_y, nW, nH, extra, p):
    """aug_croppad / aug_croppad_bbox (:55-118, :260-304): the crop centred on ``point`` moved by the perturbation draws.  The slices
    [center + int(crop / 2), ... + crop + extra) of the canvas padded by crop on every side must lie inside it: a negative start
    would wrap, an end past the padded size would truncate the crop.  ``extra`` is 1 where a mask is sliced (one longer than the
    image), else 0.  Returns ``center`` and the canvas pixel ``(ox, oy)`` of crop pixel (0, 0)."""
    x_offset = int((float(dice[3]) - 0.5) * 2 * p["center_perterb_max"])
    y_offset = int((float(dice[4]) - 0.5) * 2 * p["center_perterb_max"])
    center = point + np.array([x_offset, y_offset])
    if not np.all(np.isfinite(center)):
        raise MpnError("objpos is not finite")
    center = center.astype(int)
    x0, y0 = int(center[0]) + int(crop_x / 2), int(center[1]) + int(crop_y / 2)
    if x0 < 0 or y0 < 0 or x0 + crop_x + extra > nW + 2 * crop_x or y0 + crop_y + extra > nH + 2 * crop_y:
        raise MpnError("crop centre (%d, %d) is too far outside the %d x %d canvas: the reference's slices would wrap or truncate"
                       % (center[0], center[1], nW, nH))
    return {"center": (int(center[0]), int(center[1])), "ox": x0 - crop_x, "oy": y0 - crop_y}


def augment_meta(H, W, scale_provided, objpos, joint_self, joint_others, dice, crop_x, crop_y, params=None, objpos_other=None,
                 with_mask=True):
    """The meta-data side of aug_scale -> aug_rotate -> aug_croppad -> aug_flip for one sample, op for op.

    joint_self [18, 3] / joint_others [n, 18, 3] (after :func:`add_neck`), objpos [2] in source pixels; ``dice`` as laid out by
    :func:`draw_dice`.  Returns a dict: the transformed ``joint_self`` / ``joint_others`` / ``objpos`` / ``objpos_other`` (before
    :func:`remove_illegal_joint`) and the numbers the kernels need — ``scale``, the scaled size ``(nh, nw)``, the canvas size
    ``(nH, nW)``, ``M`` (the matrix handed to warpAffine) and ``Minv``, the crop origin ``(ox, oy)`` on the canvas, ``flip`` — plus
    ``degree`` and ``center``."""
    p = DEFAULT_PARAMS if params is None else params
    dice = _sample_dice(dice)
    crop_x, crop_y = int(crop_x), int(crop_y)
    objpos = np.array(objpos, dtype=np.float64)
    js = np.array(joint_self, dtype=np.float64)
    jo = np.array(joint_others, dtype=np.float64).reshape(-1, 18, 3)
    n_other = jo.shape[0]
    oo = np.zeros((n_other, 2)) if objpos_other is None else np.array(objpos_other, dtype=np.float64).reshape(n_other, 2)
    if js.shape != (18, 3) or objpos.shape != (2,):
        raise MpnError("joint_self must be [18, 3] and objpos [2]")

    # --- aug_scale (ImageAugmentation.py:25-52)
    geo = _scale_and_canvas(H, W, scale_provided, dice, p)
    scale, M = geo["scale"], geo["M"]
    objpos *= scale
    js[:, :2] *= scale
    if n_other != 0:
        oo *= scale
        jo[:, :, :2] *= scale

    # --- aug_rotate (:205-231): unlike aug_rotate_bbox it moves objpos and every joint with rotate_bound's matrix
    objpos = _rotatepoint(objpos, M)
    for i in range(18):
        js[i, :] = _rotatepoint(js[i, :], M)
    for j in range(n_other):
        oo[j, :] = _rotatepoint(oo[j, :], M)
        for i in range(18):
            jo[j, i, :] = _rotatepoint(jo[j, i, :], M)

    # --- aug_croppad (:55-118), centred on the ROTATED objpos; the mask slice is one longer than the image's
    geo.update(_crop_origin(objpos, dice, crop_x, crop_y, geo["nW"], geo["nH"], 1 if with_mask else 0, p))
    center = geo["center"]
    offset = np.array([crop_x / 2 - center[0], crop_y / 2 - center[1]])
    objpos += offset
    js[:, :2] += offset
    mask = np.logical_or.reduce((js[:, 0] >= crop_x, js[:, 0] < 0, js[:, 1] >= crop_y, js[:, 1] < 0))
    js[mask, 2] = 2
    if n_other != 0:
        oo += offset
        jo[:, :, :2] += offset
        mask = np.logical_or.reduce((jo[:, :, 0] >= crop_x, jo[:, :, 0] < 0, jo[:, :, 1] >= crop_y, jo[:, :, 1] < 0))
        jo[mask, 2] = 2

    # --- aug_flip (:121-158); w is the IMAGE's width (the mask, one pixel wider, is flipped over its own)
    geo["flip"] = bool(dice[5] <= p["flip_prob"])
    if geo["flip"]:
        w = crop_x
        objpos[0] = w - 1 - objpos[0]
        js[:, 0] = w - 1 - js[:, 0]
        js = js[FLIP_ORDER]
        if n_other != 0:
            oo[:, 0] = w - 1 - oo[:, 0]
            jo[:, :, 0] = w - 1 - jo[:, :, 0]
            for i in range(n_other):
                jo[i] = jo[i][FLIP_ORDER]
    geo.update(joint_self=js, joint_others=jo, objpos=objpos, objpos_other=oo)
    return geo


def augment_meta_bbox(H, W, scale_provided, objpos, dice, crop_x, crop_y, params=None):
    """The meta-data side of aug_scale_bbox -> aug_rotate_bbox -> aug_croppad_bbox -> aug_flip_bbox (ImageAugmentation.py:234-340)
    for one sample, op for op.  Same geometry keys as :func:`augment_meta`.  Where the chain differs from the keypoint chain:

    * ``objpos`` is scaled and then moved by NOTHING: aug_rotate_bbox drops rotate_bound's matrix (:330), aug_croppad_bbox centres
      the crop on the unrotated point on the rotated canvas and does not write it back, aug_flip_bbox does not touch it;
    * every instance mask is sliced ``crop + 1`` long in BOTH axes (:296-297) while the image slice is ``crop`` long, and is flipped
      over its own width: mask column x becomes ``crop_x - x`` where image column u becomes ``crop_x - 1 - u``.  Boxes therefore
      live in the ``(crop + 1)``-wide mask frame and may reach ``crop + 1``.

    Masks and image share the resize rule (``cv2.resize(fx=scale)``: dsize = round(size * scale)) and ``M``."""
    p = DEFAULT_PARAMS if params is None else params
    dice = _sample_dice(dice)
    objpos = np.array(objpos, dtype=np.float64)
    if objpos.shape != (2,):
        raise MpnError("objpos must be [2]")
    # aug_scale_bbox (:234-257); aug_rotate_bbox (:325-340) hands rotate_bound's matrix to warpAffine only
    geo = _scale_and_canvas(H, W, scale_provided, dice, p)
    objpos *= geo["scale"]
    # aug_croppad_bbox (:260-304), centred on the UNROTATED objpos; always the mask's slice
    geo.update(_crop_origin(objpos, dice, int(crop_x), int(crop_y), geo["nW"], geo["nH"], 1, p))
    # aug_flip_bbox (:307-322)
    geo.update(objpos=objpos, flip=bool(dice[5] <= p["flip_prob"]))
    return geo


def table_row(geo, H, W, img_off, img_pitch, mask_off=0, mask_pitch=0):
    """One row of the per-sample table of mpn_augment_image / mpn_augment_mask (float64; every integer in it is exact)."""
    row = np.zeros(T_COLS, dtype=np.float64)
    row[[T_IMG_OFF, T_IMG_PITCH, T_MASK_OFF, T_MASK_PITCH, T_H, T_W]] = (img_off, img_pitch, mask_off, mask_pitch, H, W)
    row[[T_SCALE, T_NW, T_NH, T_CW, T_CH]] = (geo["scale"], geo["nw"], geo["nh"], geo["nW"], geo["nH"])
    row[T_MINV:T_MINV + 6] = geo["Minv"].reshape(6)
    row[[T_OX, T_OY, T_FLIP]] = (geo["ox"], geo["oy"], 1.0 if geo["flip"] else 0.0)
    return row


def _pinned(n, dtype):
    return torch.empty(n, dtype=dtype, pin_memory=True)


def _aligned_offsets(sizes):
    """Byte offsets of consecutive blocks of ``sizes`` bytes, every block starting on a 16-byte boundary -> (offsets, total)."""
    offsets, n = [], 0
    for s in sizes:
        offsets.append(n)
        n += (s + 15) // 16 * 16
    return offsets, n


def _pack_pinned(tensors):
    """The contiguous uint8 tensors of a batch, flat, in ONE pinned staging buffer (so one H2D copy) -> (buffer, offsets)."""
    offsets, n = _aligned_offsets([t.numel() for t in tensors])
    stage = _pinned(n, torch.uint8)
    for t, o in zip(tensors, offsets):
        stage[o: o + t.numel()] = t.view(-1)
    return stage, offsets


def _check_u8(t, what, dims):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.is_cuda or t.dim() != dims or not t.is_contiguous():
        raise MpnError("%s must be a contiguous uint8 CPU tensor with %d dimensions" % (what, dims))


def _batch_front(samples, dice, rng, params):
    """What both augmenters check before any geometry: the batch is not empty, the dice are [B, 6] (drawn from ``rng`` through
    :func:`draw_dice` when not given), every ``img`` is a uint8 [H, W, 3] CPU tensor.  Returns (dice, [(H, W)])."""
    B = len(samples)
    if B == 0:
        raise MpnError("empty batch")
    if dice is None:
        rng = random if rng is None else rng
        dice = np.stack([draw_dice(rng, params) for _ in range(B)])
    dice = np.asarray(dice, dtype=np.float64)
    if dice.shape != (B, N_DICE):
        raise MpnError("dice must be [B, %d]" % N_DICE)
    sizes = []
    for s in samples:
        img = s["img"]
        _check_u8(img, "img", 3)
        if img.shape[2] != 3 or img.shape[0] < 1 or img.shape[1] < 1:
            raise MpnError("img must be [H, W, 3]")
        sizes.append((int(img.shape[0]), int(img.shape[1])))
    return dice, sizes


def augment_image(src, table, crop_y, crop_x):
    """mpn_augment_image: packed uint8 BGR sources (device) + table [B, 20] float64 (device) -> float32 [B, 3, crop_y, crop_x]."""
    B = table.shape[0]
    out = torch.empty((B, 3, crop_y, crop_x), dtype=torch.float32, device=src.device)
    ms = (ctypes.c_float * 6)(*(MEANS + STDS))
    call("mpn_augment_image", ops.ptr(src), src.numel(), ops.ptr(table), B, ops.ptr(out), crop_y, crop_x, ms, ops.stream_ptr())
    return out


def augment_mask(src, table, gh, gw, stride, crop_x):
    """mpn_augment_mask: packed uint8 masks (device) + table -> float32 [B, 18, gh, gw], the 18 channels materialised."""
    B = table.shape[0]
    out = torch.empty((B, 18, gh, gw), dtype=torch.float32, device=src.device)
    call("mpn_augment_mask", ops.ptr(src), src.numel(), ops.ptr(table), B, ops.ptr(out), gh, gw, stride, crop_x, ops.stream_ptr())
    return out


def augment_plane(src, table, gh, gw, stride, crop_x, outside=0.0):
    """mpn_augment_plane: packed uint8 planes (device) at the table's MASK columns -> float32 [B, 1, gh, gw], sampled as
    :func:`augment_mask` samples, ``outside`` / 255 where the cell lies outside the canvas or the scaled image."""
    B = table.shape[0]
    out = torch.empty((B, 1, gh, gw), dtype=torch.float32, device=src.device)
    call("mpn_augment_plane", ops.ptr(src), src.numel(), ops.ptr(table), B, ops.ptr(out), gh, gw, stride, crop_x, float(outside),
         ops.stream_ptr())
    return out


def augment_boxes(src, table, row_inst, B, N, crop_y, crop_x):
    """mpn_augment_boxes: packed instance-mask rectangles (uint8, device; None when there is no instance) + instance table
    [n_inst, 24] float64 + row map int32 [B * N] (instance of each output row, -1 = padding) -> float32 [B, N, 5]."""
    n_inst = 0 if table is None else int(table.shape[0])
    dev = row_inst.device
    out = torch.empty((B, N, 5), dtype=torch.float32, device=dev)
    if B * N == 0:
        return out
    ws = torch.empty(max(int(call("mpn_augment_boxes_workspace_bytes", n_inst, crop_y, crop_x)), 16), dtype=torch.uint8, device=dev)
    call("mpn_augment_boxes", ops.ptr(src) if n_inst else None, src.numel() if n_inst else 0, ops.ptr(table) if n_inst else None, n_inst,
         ops.ptr(row_inst), B * N, ops.ptr(out), crop_y, crop_x, ops.ptr(ws), ops.stream_ptr())
    return out


def _mask_array(m, H, W):
    if isinstance(m, torch.Tensor):
        if m.is_cuda or m.dtype not in (torch.uint8, torch.bool):
            raise MpnError("an instance mask must be a uint8 or bool CPU tensor or array")
        m = m.numpy()
    if not isinstance(m, np.ndarray) or m.dtype not in (np.uint8, np.bool_):
        raise MpnError("an instance mask must be a uint8 or bool CPU tensor or array")
    if m.shape != (H, W):
        raise MpnError("an instance mask must have the image's [H, W]")
    return m.view(np.uint8)


def instance_rects(sample, H, W):
    """``Cocobbox.get_instance_mask`` / ``get_ground_truth`` on the host (COCO_data_pipeline.py:342-405): an all-zero mask is dropped
    (:354), a crowd counts for the list being non-empty but yields no row (:386-389), an empty list raises (the reference:
    IndexError at ``instance_mask_list[0]``).  Returns [(mask as uint8 array, rx0, ry0, rw, rh)] of the instances that get a row;
    the np.any scans that find the rectangle replace the reference's ``m.max() < 1``."""
    inst, crowd = sample.get("instances"), sample.get("iscrowd")
    if inst is None or crowd is None or len(inst) != len(crowd):
        raise MpnError("a sample needs 'instances' and an 'iscrowd' entry for each of them")
    rects, kept = [], 0
    for m, c in zip(inst, crowd):
        m = _mask_array(m, H, W)
        cols = np.flatnonzero(m.any(axis=0))
        if cols.size == 0:
            continue
        kept += 1
        if int(c):
            continue
        rws = np.flatnonzero(m.any(axis=1))
        rects.append((m, int(cols[0]), int(rws[0]), int(cols[-1]) - int(cols[0]) + 1, int(rws[-1]) - int(rws[0]) + 1))
    if kept == 0:
        raise MpnError("a sample has no instance with a non-zero mask")
    return rects


def batch_kind(samples):
    """"instances" or "segmentations": what every sample of the batch carries its objects as.  A sample with both or neither, and
    a batch that mixes the two, raise — before any dice are drawn."""
    kinds = set()
    for s in samples:
        has = [k for k in ("instances", "segmentations") if s.get(k) is not None]
        if len(has) != 1:
            raise MpnError("a sample carries either 'instances' or 'segmentations'")
        kinds.add(has[0])
    if len(kinds) > 1:
        raise MpnError("a batch carries either 'instances' or 'segmentations', not both kinds")
    return kinds.pop() if kinds else "instances"


def mask_source(samples):
    """"mask_miss", "person_anns" or None: where every sample of the batch gets its mask_miss from — the uint8 plane itself, the
    image's person annotations (rasterised and composed on the device, :func:`..segm.mask_miss_batch`) or nowhere (the image-only
    form).  A sample with both keys, a batch that mixes the two and a batch where only some samples have one raise — before any dice
    are drawn."""
    kinds = set()
    for s in samples:
        has = [k for k in ("mask_miss", "person_anns") if s.get(k) is not None]
        if len(has) > 1:
            raise MpnError("a sample carries either 'mask_miss' or 'person_anns'")
        kinds.add(has[0] if has else None)
    if "mask_miss" in kinds and "person_anns" in kinds:
        raise MpnError("a batch carries either 'mask_miss' or 'person_anns', not both kinds")
    if len(kinds) > 1:
        raise MpnError("either every sample of a batch has a mask_miss or none has")
    return kinds.pop() if kinds else None


def check_mask_all(samples, source):
    """What ``DeviceAugmenter(mask_all=True)`` asks of a batch, before any dice are drawn: a mask source (``source`` from
    :func:`mask_source`), and on a ``"mask_miss"`` batch a uint8 [H, W] ``"mask_all"`` plane in every sample."""
    if source is None:
        raise MpnError("mask_all needs a batch with 'person_anns' or with 'mask_miss' and 'mask_all' planes")
    if source == "person_anns":
        return
    for s in samples:
        if s.get("mask_all") is None:
            raise MpnError("with mask_all every 'mask_miss' sample also carries a 'mask_all' plane")
        _check_u8(s["mask_all"], "mask_all", 2)
        img = s.get("img")
        if isinstance(img, torch.Tensor) and img.dim() == 3 and tuple(s["mask_all"].shape) != tuple(img.shape[:2]):
            raise MpnError("mask_all must have the image's [H, W]")


def segmentation_pack(sample, H, W, strict=True):
    """The ``segmentations`` path's counterpart of :func:`instance_rects`: the sample's non-crowd annotations packed for
    mpn_segm_rasterize (:func:`..segm.pack_segmentations`; O(vertices), no pixel is touched).  A crowd yields no row and is not
    rasterised; EVERY non-crowd annotation keeps a row, in annotation order, whether or not its mask comes out empty (that is known
    only on the device).  An empty list raises, as it does for ``instances``."""
    sg, crowd = sample.get("segmentations"), sample.get("iscrowd")
    if sg is None or crowd is None or len(sg) != len(crowd):
        raise MpnError("a sample needs 'segmentations' and an 'iscrowd' entry for each of them")
    if len(sg) == 0:
        raise MpnError("a sample has no annotation")
    return segm.pack_segmentations([g for g, c in zip(sg, crowd) if not int(c)], H, W, strict)


def boxes_from_rects(rects, metas, S, row_multiple, dev, sample_rows=None, d_src=None):
    """Packs the rectangles of a batch (rects[b] from :func:`instance_rects`, metas[b] the sample's geometry with H, W) and launches
    mpn_augment_boxes.  One pinned buffer and one H2D copy for the rectangles; one pinned block of doubles and one H2D copy for the
    tables: the sample table ``sample_rows`` [B, 20] when given (returned as a device tensor), the instance table, and the int32
    row map in the tail.  With ``d_src`` the rectangles already lie on the device at these offsets (:func:`..segm.rasterize_packed`
    wrote them; the masks of ``rects`` are None) and nothing is staged.  Returns (bbox [B, N, 5], device sample table or None)."""
    B = len(rects)
    N = max(len(r) for r in rects)
    N = (N + row_multiple - 1) // row_multiple * row_multiple
    n_inst = sum(len(r) for r in rects)
    offsets, nbytes = _aligned_offsets([r[3] * r[4] for rs in rects for r in rs])
    stage = _pinned(max(nbytes, 16), torch.uint8) if d_src is None else None
    t0 = 0 if sample_rows is None else B * T_COLS
    t1 = t0 + n_inst * TB_COLS
    tab = _pinned(max(t1 + (B * N + 1) // 2, 1), torch.float64)
    if t0:
        tab[:t0] = torch.from_numpy(np.ascontiguousarray(sample_rows, dtype=np.float64).reshape(-1))
    table = tab[t0:t1].view(n_inst, TB_COLS)
    rowmap = tab[t1:].view(torch.int32)[:B * N].view(B, N)
    rowmap.fill_(-1)
    i = 0
    for b, (rs, g) in enumerate(zip(rects, metas)):
        for r, (m, rx0, ry0, rw, rh) in enumerate(rs):
            off = offsets[i]
            if stage is not None:
                stage[off: off + rw * rh].view(rh, rw).copy_(torch.from_numpy(m[ry0:ry0 + rh, rx0:rx0 + rw]))
            row = np.zeros(TB_COLS, dtype=np.float64)
            row[:T_COLS] = table_row(g, g["H"], g["W"], 0, 0, off, rw)
            row[TB_RX0:TB_COLS] = (rx0, ry0, rw, rh)
            table[i] = torch.from_numpy(row)
            rowmap[b, r] = i
            i += 1
    d_tab = tab.to(dev, non_blocking=True)
    d_samples = d_tab[:t0].view(B, T_COLS) if t0 else None
    d_table = d_tab[t0:t1].view(n_inst, TB_COLS) if n_inst else None
    d_rowmap = d_tab[t1:].view(torch.int32)[:B * N]
    if d_src is None:
        d_src = stage.to(dev, non_blocking=True) if n_inst else None
    return augment_boxes(d_src, d_table, d_rowmap, B, N, S, S), d_samples


def _segm_boxes(metas, S, row_multiple, dev, sample_rows=None):
    """The ``segmentations`` path of both augmenters: the batch's packs (``metas[b]["segm"]``) rasterised into the packed rectangles
    of :func:`boxes_from_rects` on the device, then the same box launch.  Nothing waits for the device."""
    pack = segm.concat_packs([g["segm"] for g in metas])
    d_src = segm.rasterize_packed(pack, dev)[0] if pack.n else None
    return boxes_from_rects([g["rects"] for g in metas], metas, S, row_multiple, dev, sample_rows, d_src=d_src)


class _Augmenter(object):
    """What the two augmenters share: the sizes, the merged parameters and the device they run on."""

    segm_strict = True                  # a malformed polygon part raises; False drops it (segm.pack_segmentations)

    def __init__(self, inp_size, feat_stride, params=None):
        self.inp_size, self.stride = int(inp_size), int(feat_stride)
        if self.inp_size <= 0 or self.stride <= 0 or int(self.inp_size / self.stride) <= 0:
            raise MpnError("inp_size and feat_stride must be positive, inp_size >= feat_stride")
        self.params = dict(DEFAULT_PARAMS)
        if params:
            self.params.update(params)

    def _device(self):
        if not torch.cuda.is_available():
            raise MpnError("%s runs on the MI355X only; there is no CPU path" % type(self).__name__)
        return torch.device("cuda", torch.cuda.current_device())


class DeviceAugmenter(_Augmenter):
    """``DeviceAugmenter(inp_size, feat_stride, params=None, mask_all=False)(samples)`` -> ``(img, heatmaps, heat_mask, meta)``: the reference's training triple
    for ``keypoint_subnet`` (float32, contiguous, on the current device) plus the host-side geometry of every sample.

    A sample is a dict with the decoded image and the reference's meta fields::

        {"img": uint8 tensor [H, W, 3] (BGR, CPU, contiguous), "mask_miss": uint8 tensor [H, W] or None,
         "objpos": (x, y), "scale_provided": s, "joint_self": [17, 3], "joint_others": [n, 17, 3] (optional),
         "objpos_other": [n, 2] (optional)}

    ``joint_self`` / ``joint_others`` with 18 rows are taken as already in this work's order (no neck is added).  With
    ``mask_miss`` None in every sample the image-only form is returned: ``heat_mask`` is None.  Instead of ``mask_miss`` a sample may
    carry ``"person_anns"``: the image's person annotation dicts in json order (``segmentation``, ``iscrowd``, ``num_keypoints`` or
    ``keypoints``; an empty list is allowed), from which the plane is built on the device by the rule of :mod:`..segm`, so no PNG
    is read and no H x W plane is uploaded; ``segm_strict`` applies (:func:`mask_source` states what a batch may mix).  (The ``aug_*_bbox`` chain of the
    detection loader is NOT this chain with the mask left out: it never rotates ``objpos`` and so crops elsewhere; see
    :func:`augment_meta_bbox` and :class:`DeviceBBoxAugmenter`.)  ``dice`` [B, 6] makes the draws explicit; otherwise they come from ``rng``
    (a ``random.Random``; default the ``random`` module, as in the reference) through :func:`draw_dice`.

    ``mask_all=True`` adds the target of the person-segmentation channel: ``(img, heatmaps, heat_mask, mask_all, meta)`` with
    ``mask_all`` float32 [B, 1, grid, grid] in [0, 1], ``mask_miss``'s sampling of the union of the image's person annotations with
    0 outside the image (``mpn_augment_plane``).  On a ``"person_anns"`` batch both planes come from the one
    compose launch (:func:`..segm.person_masks_batch`); on a ``"mask_miss"`` batch every sample also carries a uint8 [H, W]
    ``"mask_all"`` plane.  An image-only batch, a missing, mis-shaped or non-uint8 plane raise before any dice are drawn."""

    def __init__(self, inp_size, feat_stride, params=None, mask_all=False):
        super(DeviceAugmenter, self).__init__(inp_size, feat_stride, params)
        self.mask_all = bool(mask_all)

    def geometry(self, samples, dice=None, rng=None, mask_frame=False):
        """Part 1 for a batch: list of per-sample dicts of :func:`augment_meta` with the final (``remove_illegal_joint``) joints
        under ``joint_self_out`` / ``joint_others_out``.  Needs no GPU.  ``mask_frame`` asks for the ``crop + 1`` slice test of
        the masks even when the batch carries no ``mask_miss`` (instance masks take the same slices)."""
        source = mask_source(samples)                                  # before the dice are drawn: a refused batch leaves rng alone
        if self.mask_all:
            check_mask_all(samples, source)
        dice, sizes = _batch_front(samples, dice, rng, self.params)
        frame = source is not None or mask_frame
        metas = []
        for s, d, (H, W) in zip(samples, dice, sizes):
            if s.get("mask_miss") is not None:
                _check_u8(s["mask_miss"], "mask_miss", 2)
                if tuple(s["mask_miss"].shape) != (H, W):
                    raise MpnError("mask_miss must have the image's [H, W]")
            if s.get("person_anns") is not None and not isinstance(s["person_anns"], (list, tuple)):
                raise MpnError("person_anns must be the list of the image's annotation dicts")
            js = np.asarray(s["joint_self"], dtype=np.float64)
            jo = np.asarray(s.get("joint_others", np.zeros((0,) + js.shape)), dtype=np.float64)
            if js.shape == (17, 3):
                js, jo = add_neck(js, jo)
            elif js.shape != (18, 3):
                raise MpnError("joint_self must be [17, 3] (COCO order) or [18, 3]")
            jo = jo.reshape(-1, 18, 3)
            geo = augment_meta(H, W, s["scale_provided"], s["objpos"], js, jo, d, self.inp_size, self.inp_size, self.params,
                               s.get("objpos_other"), with_mask=frame)
            geo["joint_self_out"], geo["joint_others_out"] = remove_illegal_joint(geo["joint_self"], geo["joint_others"],
                                                                                  self.inp_size, self.inp_size)
            geo["dice"], geo["H"], geo["W"] = d.copy(), H, W
            metas.append(geo)
        return metas

    def __call__(self, samples, dice=None, rng=None):
        return self._run(samples, dice, rng, False)

    def call_with_boxes(self, samples, dice=None, rng=None):
        """For ``train_both``: ``(img, heatmaps, heat_mask, bbox, metas)``, with ``mask_all`` after ``heat_mask`` when the augmenter was
        built with ``mask_all=True``.  The samples also carry ``instances`` / ``iscrowd`` — or
        ``segmentations`` / ``iscrowd`` — as for :class:`DeviceBBoxAugmenter`; the boxes are read under THIS chain's geometry (rotated
        ``objpos``), through the same kernel."""
        return self._run(samples, dice, rng, True)

    def _run(self, samples, dice, rng, boxes):
        dev = self._device()
        kind = batch_kind(samples) if boxes else None
        metas = self.geometry(samples, dice, rng, mask_frame=boxes)
        if kind == "segmentations":
            for s, g in zip(samples, metas):
                g["segm"] = segmentation_pack(s, g["H"], g["W"], self.segm_strict)
                g["rects"] = [(None,) + r for r in g["segm"].rects()]
        rects = [instance_rects(s, g["H"], g["W"]) for s, g in zip(samples, metas)] if kind == "instances" else None
        B, S = len(samples), self.inp_size
        source = mask_source(samples)
        # one pinned staging buffer per kind (every source starts on a 16-byte boundary), one H2D copy each
        stage_i, img_off = _pack_pinned([s["img"] for s in samples])
        # the table carries the masks' offsets with or without a mask buffer, as it always has
        mask_off = _aligned_offsets([g["H"] * g["W"] for g in metas])[0]
        stage_m = _pack_pinned([s["mask_miss"] for s in samples])[0] if source == "mask_miss" else None
        stage_a = _pack_pinned([s["mask_all"] for s in samples])[0] if source == "mask_miss" and self.mask_all else None
        table = _pinned(B * T_COLS, torch.float64).view(B, T_COLS)
        maxP = max(1 + g["joint_others_out"].shape[0] for g in metas)
        joints = _pinned(B * maxP * 18 * 3, torch.float64).view(B, maxP, 18, 3).zero_()
        num = _pinned(B, torch.int32)
        for b, (s, g) in enumerate(zip(samples, metas)):
            table[b] = torch.from_numpy(table_row(g, g["H"], g["W"], img_off[b], g["W"] * 3, mask_off[b], g["W"]))
            n = g["joint_others_out"].shape[0]
            joints[b, 0] = torch.from_numpy(g["joint_self_out"])
            if n:
                joints[b, 1:1 + n] = torch.from_numpy(g["joint_others_out"])
            num[b] = 1 + n
        d_img = stage_i.to(dev, non_blocking=True)
        d_table = table.to(dev, non_blocking=True)
        img = augment_image(d_img, d_table, S, S)
        heat_mask = mask_all = d_all = None
        if source is not None:
            grid = int(S / self.stride)                               # COCO_data_pipeline.py:206-207
            if source == "person_anns":
                # the planes are composed on the device at the offsets and pitch W the table rows carry
                compose = segm.person_masks_batch if self.mask_all else segm.mask_miss_batch
                planes = compose([s["person_anns"] for s in samples], [(g["H"], g["W"]) for g in metas], mask_off, self.segm_strict, dev)
                d_mask, d_all = planes[0], planes[1] if self.mask_all else None
            else:
                d_mask = stage_m.to(dev, non_blocking=True)
                d_all = stage_a.to(dev, non_blocking=True) if self.mask_all else None
            heat_mask = augment_mask(d_mask, d_table, grid, grid, self.stride, S)
            if self.mask_all:
                mask_all = augment_plane(d_all, d_table, grid, grid, self.stride, S, 0.0)      # nobody stands outside the image
        heatmaps = put_gaussian_maps(joints.to(dev, non_blocking=True), num.to(dev, non_blocking=True), S, S, self.stride,
                                     self.params["sigma"])
        # the pinned staging buffers may go out of scope here: torch's caching host allocator records the stream of a non_blocking
        # copy and hands a block out again only after that copy has finished
        front = (img, heatmaps, heat_mask, mask_all) if self.mask_all else (img, heatmaps, heat_mask)
        if kind == "segmentations":
            return front + (_segm_boxes(metas, S, 1, dev)[0], metas)
        if boxes:
            return front + (boxes_from_rects(rects, metas, S, 1, dev)[0], metas)
        return front + (metas,)


class DeviceBBoxAugmenter(_Augmenter):
    """``DeviceBBoxAugmenter(inp_size, feat_stride)(samples)`` -> ``(img, bbox, metas)``: the reference's training pair for
    ``detection_subnet`` (``Cocobbox.__getitem__`` + ``bbox_collater``, COCO_data_pipeline.py:407-458) plus the host geometry.

    A sample is a dict::

        {"img": uint8 tensor [H, W, 3] (BGR, CPU, contiguous), "objpos": (x, y), "scale_provided": s,
         "instances": [uint8 or bool [H, W] masks (CPU tensors or arrays)], "iscrowd": [0 / 1 per instance]}

    ``img`` is float32 [B, 3, S, S] from mpn_augment_image under the bbox chain's geometry (:func:`augment_meta_bbox`); ``bbox`` is
    float32 [B, N, 5] on the device, rows ``[x1, y1, x2, y2, 0]`` in the ``(S + 1)``-wide mask frame, ``-1`` rows for an instance
    warped out of the crop and for padding.  ``N`` is the batch maximum of rows rounded up to ``row_multiple`` (1: bbox_collater's
    shape, ``[B, 0, 5]`` when no image has a row; 8: nothing left to pad for ReplayedTrainStep's ``anno_bucket``).

    Instead of ``instances`` a sample may carry the raw COCO fields, ``"segmentations": [polygon parts | RLE dict per annotation]``
    (:func:`..segm.pack_segmentations`), which are rasterised on the device (csrc/segm.hip) into the same packed rectangles; the
    host then touches no pixel and pycocotools is not needed.  A sample with both keys or neither, and a batch that mixes the two
    kinds, raise.  What differs on that path, because whether a mask is empty is known only on the device and nothing here waits
    for the device:

    * crowd annotations get no row and are not rasterised (as with ``instances``);
    * EVERY non-crowd annotation keeps its row slot, in annotation order.  One whose mask comes out empty reads ``-1`` in its slot
      (the consumers drop ``-1`` rows wherever they stand), where the ``instances`` path drops that row before numbering;
    * a sample whose masks are all empty yields ``-1`` rows and no error;
    * ``N`` is the batch maximum of non-crowd annotations rounded up to ``row_multiple``.

    ``segm_strict = False`` (attribute) drops polygon parts with an odd length or fewer than 6 numbers instead of raising."""

    def __init__(self, inp_size, feat_stride, params=None, row_multiple=1):
        super(DeviceBBoxAugmenter, self).__init__(inp_size, feat_stride, params)
        self.row_multiple = int(row_multiple)
        if self.row_multiple <= 0:
            raise MpnError("inp_size, feat_stride and row_multiple must be positive, inp_size >= feat_stride")

    def geometry(self, samples, dice=None, rng=None):
        """List of per-sample dicts of :func:`augment_meta_bbox` plus ``H``, ``W``, ``dice`` and ``rects`` (the instances that get a
        row, from :func:`instance_rects`; on the ``segmentations`` path the conservative rectangles of :func:`segmentation_pack`,
        masks None, with the pack itself under ``segm``).  Needs no GPU."""
        kind = batch_kind(samples)
        dice, sizes = _batch_front(samples, dice, rng, self.params)
        metas = []
        for s, d, (H, W) in zip(samples, dice, sizes):
            geo = augment_meta_bbox(H, W, s["scale_provided"], s["objpos"], d, self.inp_size, self.inp_size, self.params)
            geo["dice"], geo["H"], geo["W"] = d.copy(), H, W
            if kind == "segmentations":
                geo["segm"] = segmentation_pack(s, H, W, self.segm_strict)
                geo["rects"] = [(None,) + r for r in geo["segm"].rects()]
            else:
                geo["rects"] = instance_rects(s, H, W)
            metas.append(geo)
        return metas

    def __call__(self, samples, dice=None, rng=None):
        dev = self._device()
        metas = self.geometry(samples, dice, rng)
        stage_i, img_off = _pack_pinned([s["img"] for s in samples])
        rows = np.stack([table_row(g, g["H"], g["W"], off, g["W"] * 3) for g, off in zip(metas, img_off)])
        # three H2D copies in all: the images, the mask rectangles, the tables
        if "segm" in metas[0]:
            bbox, d_table = _segm_boxes(metas, self.inp_size, self.row_multiple, dev, rows)
        else:
            bbox, d_table = boxes_from_rects([g["rects"] for g in metas], metas, self.inp_size, self.row_multiple, dev, rows)
        img = augment_image(stage_i.to(dev, non_blocking=True), d_table, self.inp_size, self.inp_size)
        return img, bbox, metas
