"""numpy restatement of the fused test-time-augmentation kernels (csrc/tta.hip), built on the oracle's cv2.resize restatement.

``merge_ref``: mpn_tta_merge.  Per scale s the pair map U_s is float32 [rh, rw, 36] (channels 0..17 from the pass over the original
image, 18..35 from the pass over the mirrored one).  With R(U) = cv_resize(U, (H, W), cubic) — float32 — and r = float32(1 / n):

    a_o = 0.0; a_f = 0.0                                      (float64)
    for s in order: a_o = a_o + float64(R(U_s)[y, x, c] * r)                     (float32 product)
    for s in order: a_f = a_f + float64(R(U_s)[y, W - 1 - x, 18 + swap[c]] * r)
    out = float32((a_o + a_f) / 2.0)

which is Tester._get_outputs for both images, _handle_heat and the final .float() with their rounding points.  ``divide=True`` takes
a true float32 division by n in place of the product with the rounded reciprocal (what numpy does for ``hm / 5``; the device's
tensor library multiplies).  ``wrong`` selects one modelled misreading of the rule (tests/test_tta_fused_cpu.py).

``input_ref``: mpn_tta_input for one image of the pair (the caller mirrors the image for the other one)."""
import numpy as np

from oracle.joint_oracle import cv_resize

SWAP_HEAT = [0, 1, 5, 6, 7, 2, 3, 4, 11, 12, 13, 8, 9, 10, 15, 14, 17, 16]
MISREADINGS = ("no_mirror", "no_swap", "swap_original", "mirror_about_W", "one_accumulator", "divide_after_sum")


def _scaled(R, n, divide):
    n32 = np.float32(n)
    return (R / n32) if divide else (R * np.float32(1.0 / float(n)))


def merge_ref(pair_maps, H, W, swap=SWAP_HEAT, n_div=None, divide=False, wrong=None):
    assert wrong is None or wrong in MISREADINGS
    n = len(pair_maps) if n_div is None else n_div
    swap = np.asarray(swap, dtype=np.int64)
    a_o = np.zeros((H, W, 18), dtype=np.float64)
    a_f = np.zeros((H, W, 18), dtype=np.float64)
    full = [cv_resize(np.asarray(U, dtype=np.float32), (H, W), True) for U in pair_maps]
    cols = np.arange(W)[::-1]                                  # W - 1 - x
    if wrong == "no_mirror":
        cols = np.arange(W)
    elif wrong == "mirror_about_W":
        cols = np.minimum(W - np.arange(W), W - 1)
    ch_o = np.arange(18) if wrong != "swap_original" else swap
    ch_f = 18 + (swap if wrong not in ("no_swap", "swap_original") else np.arange(18))
    if wrong == "divide_after_sum":
        for R in full:
            a_o = a_o + R[:, :, ch_o].astype(np.float64)
            a_f = a_f + R[:, cols][:, :, ch_f].astype(np.float64)
        a_o, a_f = a_o / float(n), a_f / float(n)
        return ((a_o + a_f) / 2.0).astype(np.float32)
    if wrong == "one_accumulator":
        acc = np.zeros((H, W, 18), dtype=np.float64)
        for R in full:
            acc = acc + _scaled(R[:, :, ch_o], n, divide).astype(np.float64)
        for R in full:
            acc = acc + _scaled(R[:, cols][:, :, ch_f], n, divide).astype(np.float64)
        return (acc / 2.0).astype(np.float32)
    for R in full:
        a_o = a_o + _scaled(R[:, :, ch_o], n, divide).astype(np.float64)
    for R in full:
        a_f = a_f + _scaled(R[:, cols][:, :, ch_f], n, divide).astype(np.float64)
    return ((a_o + a_f) / 2.0).astype(np.float32)


def input_ref(img, h, w, hp, wp, inv_scale, divide=False):
    """float32 [3, hp, wp]: crop_with_factor(img, ..., pad_val=128)[0] through resnet_preprocess, for a float32 [H, W, 3] BGR image."""
    img = np.asarray(img, dtype=np.float32)
    padded = np.full((hp, wp, 3), 128.0, dtype=np.float32)
    padded[:h, :w] = cv_resize(img, (h, w), False, inv_scale=(inv_scale, inv_scale))
    x = (padded / np.float32(255.0)) if divide else (padded * np.float32(1.0 / 255.0))
    x = x[:, :, ::-1]
    mean = np.array([0.485, 0.456, 0.406], dtype=np.float32)
    std = np.array([0.229, 0.224, 0.225], dtype=np.float32)
    return np.ascontiguousarray(((x - mean) / std).transpose(2, 0, 1))


def upsample_crop_ref(heat_pair, rh, rw):
    """The pair map of one scale from its [2, 18, hq, wq] heat-maps: the first rh x rw of the x4 bicubic up-sampling, 36 channels."""
    hp = np.asarray(heat_pair, dtype=np.float32)
    hwc = np.ascontiguousarray(hp.reshape(36, hp.shape[2], hp.shape[3]).transpose(1, 2, 0))
    return cv_resize(hwc, (rh, rw), True, inv_scale=(0.25, 0.25))
