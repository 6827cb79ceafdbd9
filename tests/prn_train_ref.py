"""Float64 restatement of the reference's PRN training-pair construction (test-side only).

``get_data`` / ``get_anns`` transcribe ``datasets/coco_data/prn_data_pipeline.py:33-123`` statement for statement in plain Python
floats, numpy and ``scipy.ndimage``: the own-keypoint chain with its ``try/except`` (:51-72), the margin test on the raw ``bbox``
floats and the clamp chain of the image's annotations (:78-103), the two blurs (:105-107) and the channel permutation (:108-110).
``skimage.filters.gaussian`` is ``scipy.ndimage.gaussian_filter`` with truncate 4, i.e. per axis one ``correlate1d`` with the
reversed taps of ``_gaussian_kernel1d``; the taps are an argument here so that a test can hand in exactly the vectors the product
hands its kernel.  tests/golden/g18_prn_train.npz (real scikit-image) pins this file; tests/test_prn_train_cpu.py compares them.

``fault=`` applies ONE modelled mistake (``FAULTS``) so that the tests can show that the comparison has teeth.
"""
import math

import numpy as np
from scipy import ndimage

OUR_ORDER = [0, 6, 8, 10, 5, 7, 9, 12, 14, 16, 11, 13, 15, 2, 1, 4, 3]

FAULTS = ("independent_ifs", "no_negative_wrap", "no_try_except", "margin_on_int_bbox", "round_for_int", "sigma_swapped",
          "nearest_for_constant", "no_our_order", "own_filtered_by_margin")


def gaussian_taps(sigma, truncate=4.0):
    """scipy.ndimage._gaussian_kernel1d(sigma, 0, int(truncate * sigma + 0.5))."""
    radius = int(truncate * float(sigma) + 0.5)
    sigma2 = sigma * sigma
    x = np.arange(-radius, radius + 1)
    phi_x = np.exp(-0.5 / sigma2 * x ** 2)
    return phi_x / phi_x.sum()


def blur(plane, taps, mode):
    """gaussian_filter on a 2-D plane: axis 0, then axis 1 (scipy.ndimage.gaussian_filter's order)."""
    w = np.ascontiguousarray(np.asarray(taps, dtype=np.float64)[::-1])
    out = ndimage.correlate1d(plane, w, axis=0, mode=mode, cval=0.0)
    return ndimage.correlate1d(out, w, axis=1, mode=mode, cval=0.0)


class _Map(object):
    """A [H, W, 17] float64 array whose item assignment can be made to misbehave (fault 'no_negative_wrap')."""

    def __init__(self, H, W, wrap):
        self.a = np.zeros((H, W, 17))
        self.wrap = wrap

    def __setitem__(self, idx, v):
        y, x, j = idx
        if not self.wrap:
            H, W = self.a.shape[:2]
            if y >= H or x >= W:
                raise IndexError("index out of bounds")
            y, x = max(y, 0), max(x, 0)
        self.a[y, x, j] = v


def _to_int(v, fault):
    return int(round(v)) if fault == "round_for_int" else int(v)


def _chain(m, x0, y0, j, H, W, label, fault):
    """The seven-branch chain (:56-72 for the label, :90-103 for the input)."""
    if fault == "independent_ifs":
        if x0 >= W and y0 >= H:
            m[H - 1, W - 1, j] = 1
        if x0 >= W:
            m[y0, W - 1, j] = 1
        if y0 >= H:
            m[H - 1, x0, j] = 1
        if x0 < 0 and y0 < 0:
            m[0, 0, j] = 1
        if x0 < 0:
            m[y0, 0, j] = 1
        if y0 < 0:
            m[0, x0, j] = 1
        if 0 <= x0 < W and 0 <= y0 < H:
            m[y0, x0, j] = 1
        return
    if x0 >= W and y0 >= H:
        m[H - 1, W - 1, j] = 1
    elif x0 >= W:
        m[y0, W - 1, j] = 1
    elif y0 >= H:
        if label and fault != "no_try_except":
            try:
                m[H - 1, x0, j] = 1
            except Exception:
                m[H - 1, 0, j] = 1
        else:
            m[H - 1, x0, j] = 1
    elif x0 < 0 and y0 < 0:
        m[0, 0, j] = 1
    elif x0 < 0:
        m[y0, 0, j] = 1
    elif y0 < 0:
        m[0, x0, j] = 1
    else:
        m[y0, x0, j] = 1


def get_data(bbox, own_kp, img_kps, coeff, threshold, taps9=None, taps17=None, fault=None):
    """prn_data_pipeline.py:33-111.  bbox: 4 numbers (raw x, y, w, h); own_kp: the sample's 51 keypoint numbers; img_kps: the 51
    numbers of EVERY annotation of the sample's image, in the image's annotation order.  Returns float64 (weights, output), each
    [28 coeff, 18 coeff, 17]; raises what the reference raises (IndexError, ZeroDivisionError)."""
    assert fault is None or fault in FAULTS, fault
    H, W = coeff * 28, coeff * 18
    wrap = fault != "no_negative_wrap"
    weights, output = _Map(H, W, wrap), _Map(H, W, wrap)
    bbox = [float(v) for v in bbox]
    x = int(bbox[0])
    y = int(bbox[1])
    w = float(bbox[2])
    h = float(bbox[3])
    x_scale = float(W) / math.ceil(w)
    y_scale = float(H) / math.ceil(h)
    mx, my = (float(x), float(y)) if fault == "margin_on_int_bbox" else (bbox[0], bbox[1])

    def inside(px, py):
        if px > mx - bbox[2] * threshold and px < mx + bbox[2] * (1 + threshold):
            if py > my - bbox[3] * threshold and py < my + bbox[3] * (1 + threshold):
                return True
        return False

    own = [float(v) for v in np.asarray(own_kp, dtype=np.float64).reshape(-1)]
    kpx, kpy, kpv = own[0::3], own[1::3], own[2::3]
    for j in range(17):
        if kpv[j] > 0:
            if fault == "own_filtered_by_margin" and not inside(kpx[j], kpy[j]):
                continue
            x0 = _to_int((kpx[j] - x) * x_scale, fault)
            y0 = _to_int((kpy[j] - y) * y_scale, fault)
            _chain(output, x0, y0, j, H, W, True, fault)
    for ann in np.asarray(img_kps, dtype=np.float64).reshape(-1, 51):
        a = [float(v) for v in ann]
        kpx, kpy, kpv = a[0::3], a[1::3], a[2::3]
        for j in range(17):
            if kpv[j] > 0 and inside(kpx[j], kpy[j]):
                x0 = _to_int((kpx[j] - x) * x_scale, fault)
                y0 = _to_int((kpy[j] - y) * y_scale, fault)
                _chain(weights, x0, y0, j, H, W, False, fault)
    t9 = gaussian_taps(1.0) if taps9 is None else taps9
    t17 = gaussian_taps(2.0) if taps17 is None else taps17
    (tw, mw), (to, mo) = (t9, "nearest"), (t17, "constant")
    if fault == "sigma_swapped":
        tw, to = to, tw
    if fault == "nearest_for_constant":
        mo = "nearest"
    wa, oa = weights.a, output.a
    for t in range(17):
        wa[:, :, t] = blur(wa[:, :, t], tw, mw)
        oa[:, :, t] = blur(oa[:, :, t], to, mo)
    if fault != "no_our_order":
        wa, oa = wa[:, :, OUR_ORDER], oa[:, :, OUR_ORDER]
    return wa, oa


def get_anns(iscrowd, num_keypoints, num_of_keypoints):
    """prn_data_pipeline.py:113-123 on the per-annotation columns, in file order: positions of the kept annotations, sorted by
    num_keypoints descending with Python's stable sort."""
    keep = [i for i in range(len(iscrowd)) if iscrowd[i] == 0 and num_keypoints[i] > num_of_keypoints]
    return sorted(keep, key=lambda i: num_keypoints[i], reverse=True)


def image_rows(image_id, i):
    """Positions of all annotations of annotation i's image, in file order (pycocotools' imgToAnns)."""
    return [k for k in range(len(image_id)) if image_id[k] == image_id[i]]
