"""numpy restatement of the person-mask inference kernels (csrc/seg_infer.hip; include/mpn.h states the definitions), built on the
oracle's cv2.resize restatement like tests/tta_merge_ref.py.

q is channel 18 of the exported float32 maps of one image, thr a float32.

``plane_single_ref``: mpn_seg_masks' plane.  The H x W image was zero-padded to D x D, D = max(H, W), and resized to the network input,
so q is [S/4, S/4]:   P = cv_resize(q[:, :, None], (D, D), cubic)[:H, :W, 0].

``seg_upsample_ref`` / ``merge_mask_ref``: the multi-scale + flip chain.  Per scale the seg pair map U_s is float32 [rh, rw, 2] — the
first rh x rw of the x4 bicubic map of q[:hp/4, :wp/4] of the pass over the original image (channel 0) and over the mirrored one
(channel 1).  With R(U) = cv_resize(U, (H, W), cubic) and r = float32(1 / n):

    a_o = sum_s float64(R(U_s)[y, x, 0] * r);   a_f = sum_s float64(R(U_s)[y, W - 1 - x, 1] * r);   P = float32((a_o + a_f) / 2)

``mask_ref``: M = 255 where P > thr, else 0 (strict; a NaN gives 0).
``iou_counts_ref``: (inter, pred, gt) of two uint8 planes, a byte ON when non-zero.  ``summary_ref``: the float64 summary.

``wrong`` selects one modelled misreading (MISREADINGS; tests/test_seg_infer_cpu.py shows that each changes the committed cases)."""
import numpy as np

from oracle.joint_oracle import cv_resize

MISREADINGS = ("no_mirror", "mirror_about_W", "ge", "vote", "resize_padded", "grid_hw", "one_accumulator", "divide_after_sum",
               "union_sum", "on_255")
PLANE_MISREADINGS = ("no_mirror", "mirror_about_W", "one_accumulator", "divide_after_sum")


def plane_single_ref(q, H, W, wrong=None):
    assert wrong in (None, "grid_hw")
    q = np.asarray(q, dtype=np.float32)
    D = max(H, W)
    if wrong == "grid_hw":                                          # the grid of the image instead of the padded square's
        return cv_resize(q[:, :, None], (H, W), True)[:, :, 0]
    return np.ascontiguousarray(cv_resize(q[:, :, None], (D, D), True)[:H, :W, 0])


def mask_ref(P, thr, wrong=None):
    assert wrong in (None, "ge")
    P, thr = np.asarray(P, dtype=np.float32), np.float32(thr)
    with np.errstate(invalid="ignore"):
        on = (P >= thr) if wrong == "ge" else (P > thr)
    return np.where(on, 255, 0).astype(np.uint8)


def seg_upsample_ref(q_pair, rh, rw):
    """The seg pair map of one scale from channel 18 of both passes ([2, hq, wq], already cut to the padded input's quarter size): the
    first rh x rw of the x4 bicubic up-sampling, two channels."""
    qp = np.asarray(q_pair, dtype=np.float32)
    return cv_resize(np.ascontiguousarray(qp.transpose(1, 2, 0)), (rh, rw), True, inv_scale=(0.25, 0.25))


def merge_mask_ref(seg_pair_maps, H, W, wrong=None):
    """The float32 [H, W] plane of mpn_tta_merge_mask."""
    assert wrong is None or wrong in PLANE_MISREADINGS
    n = len(seg_pair_maps)
    r = np.float32(1.0 / float(n))
    full = [cv_resize(np.asarray(U, dtype=np.float32), (H, W), True) for U in seg_pair_maps]
    cols = np.arange(W)[::-1]                                      # W - 1 - x
    if wrong == "no_mirror":
        cols = np.arange(W)
    elif wrong == "mirror_about_W":
        cols = np.minimum(W - np.arange(W), W - 1)
    a_o = np.zeros((H, W), dtype=np.float64)
    a_f = np.zeros((H, W), dtype=np.float64)
    if wrong == "divide_after_sum":
        for R in full:
            a_o = a_o + R[:, :, 0].astype(np.float64)
            a_f = a_f + R[:, cols, 1].astype(np.float64)
        return ((a_o / float(n) + a_f / float(n)) / 2.0).astype(np.float32)
    if wrong == "one_accumulator":
        acc = np.zeros((H, W), dtype=np.float64)
        for R in full:
            acc = acc + (R[:, :, 0] * r).astype(np.float64)
        for R in full:
            acc = acc + (R[:, cols, 1] * r).astype(np.float64)
        return (acc / 2.0).astype(np.float32)
    for R in full:
        a_o = a_o + (R[:, :, 0] * r).astype(np.float64)
    for R in full:
        a_f = a_f + (R[:, cols, 1] * r).astype(np.float64)
    return ((a_o + a_f) / 2.0).astype(np.float32)


def chain_mask_ref(qs, geo, H, W, thr, wrong=None):
    """The mask of the multi-scale chain from the channel-18 maps: qs[s] is float32 [2, hp/4, wp/4] (both passes), geo[s] the
    unpadded (h, w) of scale s."""
    assert wrong is None or wrong in PLANE_MISREADINGS + ("ge", "vote", "resize_padded")
    if wrong == "resize_padded":                                    # the whole padded x4 map resized, the crop taken afterwards
        maps = []
        for q, (h, w) in zip(qs, geo):
            U = seg_upsample_ref(q, 4 * q.shape[1], 4 * q.shape[2])
            Hd, Wd = int(np.ceil(H * U.shape[0] / float(h))), int(np.ceil(W * U.shape[1] / float(w)))
            maps.append(np.ascontiguousarray(cv_resize(U, (Hd, Wd), True)[:H, :W]))
        return mask_ref(merge_mask_ref(maps, H, W), thr)            # the maps have the image's size: R is the identity
    maps = [seg_upsample_ref(q, min(h, 4 * q.shape[1]), min(w, 4 * q.shape[2])) for q, (h, w) in zip(qs, geo)]
    if wrong == "vote":                                             # a threshold per scale and pass, then the majority
        votes = np.zeros((H, W), dtype=np.int64)
        for U in maps:
            R = cv_resize(U, (H, W), True)
            votes += (R[:, :, 0] > np.float32(thr)).astype(np.int64) + (R[:, ::-1, 1] > np.float32(thr)).astype(np.int64)
        return np.where(votes > len(maps), 255, 0).astype(np.uint8)
    if wrong == "ge":
        return mask_ref(merge_mask_ref(maps, H, W), thr, wrong="ge")
    return mask_ref(merge_mask_ref(maps, H, W, wrong=wrong), thr)


def iou_counts_ref(pred, gt, wrong=None):
    """int64 (inter, pred, gt) of two uint8 [H, W] planes."""
    assert wrong in (None, "on_255")
    p, g = np.asarray(pred, dtype=np.uint8), np.asarray(gt, dtype=np.uint8)
    a, b = ((p == 255), (g == 255)) if wrong == "on_255" else ((p != 0), (g != 0))
    return np.array([int((a & b).sum()), int(a.sum()), int(b.sum())], dtype=np.int64)


def summary_ref(counts, sizes, wrong=None):
    """The summary dict from int64 counts [n, 3] and the pixel count of every image, in float64 from the exact integers."""
    assert wrong in (None, "union_sum")
    c = np.asarray(counts, dtype=np.int64).reshape(-1, 3)
    N = [int(v) for v in np.asarray(sizes).reshape(-1)]
    inter, pred, gt = [int(v) for v in c[:, 0]], [int(v) for v in c[:, 1]], [int(v) for v in c[:, 2]]
    union = [p + g if wrong == "union_sum" else p + g - i for i, p, g in zip(inter, pred, gt)]

    def ratio(a, b):
        return float(a) / float(b) if b > 0 else float("nan")
    per = [float(i) / float(u) for i, u in zip(inter, union) if u > 0]
    return {"iou": ratio(sum(inter), sum(union)),
            "mean_iou": float(np.mean(np.array(per, dtype=np.float64))) if per else float("nan"),
            "n_empty": sum(1 for u in union if u == 0),
            "precision": ratio(sum(inter), sum(pred)),
            "recall": ratio(sum(inter), sum(gt)),
            "pixel_acc": ratio(sum(n - u + i for n, u, i in zip(N, union, inter)), sum(N)),
            "n_images": len(N)}


# ---- the committed cases (seeded; computed once per process and shared: leave them unchanged) -------------------------------------------
SINGLE_CASES = [(5, 6, 4), (37, 53, 16), (64, 65, 32), (130, 70, 32)]            # (H, W, S/4)
MERGE_CASES = [(37, 53, 5), (64, 48, 5), (37, 53, 1), (130, 70, 3)]              # (H, W, scales)
THR = 0.5
_CACHE = {}


def single_case(H, W, hq):
    """-> (q float32 [hq, hq], plane, mask) of one single-scale case at THR."""
    key = ("single", H, W, hq)
    if key not in _CACHE:
        q = np.random.RandomState(1000 * H + W).uniform(0.0, 1.0, (hq, hq)).astype(np.float32)
        P = plane_single_ref(q, H, W)
        _CACHE[key] = (q, P, mask_ref(P, THR))
    return _CACHE[key]


def merge_case(H, W, scales):
    """-> (qs, geo, maps, plane, mask) of one multi-scale case at THR: qs[s] float32 [2, hp/4, wp/4], geo[s] = (h, w), maps[s] the seg
    pair map.  Multipliers as in tests/test_tta_fused_gpu.py (inp_size 48)."""
    from multiposenet.pytorch_amd.evaluate.tester import scale_geometry
    key = ("merge", H, W, scales)
    if key not in _CACHE:
        rs = np.random.RandomState(100 * H + scales)
        mult = [x * 48 / float(H) for x in [0.5, 1., 1.5, 2, 2.5]][:scales] if scales > 1 else [1.5 * 48 / float(H)]
        qs, geo = [], []
        for m in mult:
            _, h, w, hp, wp = scale_geometry(H, W, m * H, 32)
            qs.append(rs.uniform(0.0, 1.0, (2, hp // 4, wp // 4)).astype(np.float32))
            geo.append((h, w))
        maps = [seg_upsample_ref(q, min(h, 4 * q.shape[1]), min(w, 4 * q.shape[2])) for q, (h, w) in zip(qs, geo)]
        P = merge_mask_ref(maps, H, W)
        _CACHE[key] = (qs, geo, maps, P, mask_ref(P, THR))
    return _CACHE[key]


def iou_case(H, W):
    """-> (pred, gt) uint8 [H, W]: gt is mask_all of the committed annotations (tests/person_seg_ref.py), pred a seeded plane whose ON
    bytes take the values 255, 1 and 7."""
    import person_seg_ref
    key = ("iou", H, W)
    if key not in _CACHE:
        rs = np.random.RandomState(7 * H + W)
        pred = rs.choice(np.array([0, 0, 0, 255, 255, 1, 7], dtype=np.uint8), size=(H, W))
        _CACHE[key] = (pred, person_seg_ref.case(H, W)[3])
    return _CACHE[key]
