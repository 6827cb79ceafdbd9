"""Float64 restatement of the box rule of mpn_augment_boxes (csrc/augment.hip), test-side only, on top of augment_ref's sampler and
bound.  Shared by tests/test_augment_bbox_cpu.py (teeth, host rules) and tests/test_augment_bbox_gpu.py (parity).

The kernel samples every pixel (u, v) of the (S + 1) x (S + 1) mask frame once from the binary source mask (un-flip over S, crop
origin, inverse warpAffine matrix, inverse resize: float64 in the kernel's operation order, so inside/outside decisions and taps are
identical; cubic weights and the 16-term sum in float32) and calls it ON when the sum is >= 0.5f.  This file computes the same sum in
float64 and the element-wise bound of augment_ref on the float32 error,

    |got - ref| <= C_SUM_BOX u mag + W_ABS u wabs,     u = 2^-24,

with C_SUM_BOX = 9: the 8 roundings on the longest path of the 16-term sum (augment_ref's count; the products with a 0 / 1 tap are in
fact exact, so this is generous by 4) plus 1 for second-order terms; nothing follows the sum (no / 255, no normalisation).  A pixel
whose float64 value exceeds 0.5 by more than the bound is ON on the device whatever the rounding; one that lies below 0.5 by more
than the bound is OFF; the rest is undecided.  Hence per instance

    INNER box: extents of the surely-ON pixels,         OUTER box: extents of the surely-ON plus the undecided pixels,

and every device coordinate must lie between the two (x1, y1 from outer to inner; x2, y2 from inner to outer).  Where they agree
the device value must be EQUAL.  Rows are assembled as Cocobbox.get_ground_truth / bbox_collater do (COCO_data_pipeline.py:382-405,
:444-458); tests/golden/g19_augment_bbox.npz holds the real functions' outputs for that.
"""
import os

import numpy as np

import augment_ref as ar

C_SUM_BOX = 9.0
EMPTY = np.array([-1.0, -1.0, -1.0, -1.0, -1.0])


def golden():
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g19_augment_bbox.npz"), allow_pickle=False)
    n = int(g["n_cases"])
    cases = []
    for i in range(n):
        pre = "c%d_" % i
        cases.append({k[len(pre):]: g[k] for k in g.files if k.startswith(pre)})
    return cases, int(g["inp_stride"][0]), int(g["inp_stride"][1]), g


def case_geo(c, origin=None):
    """Sampling geometry of a golden case from its RECORDED values (never from the product's host code)."""
    o = c["origin"] if origin is None else origin
    return ar.geometry(c["M"], c["scale"], c["stage_shapes"][0][:2], c["stage_shapes"][1][:2], o, int(c["flip"]))


def product_geo(g):
    return {k: g[k] for k in ("Minv", "scale", "nh", "nw", "nH", "nW", "ox", "oy", "flip")}


# ---- row assembly ---------------------------------------------------------------------------------------------------------------

def box_of(on, plus=1):
    """get_ground_truth's rule for one final mask (boolean [h, w]): [x1, y1, x2 + 1, y2 + 1, 0], or five -1 when nothing is set."""
    xs = np.flatnonzero(np.any(on, axis=0))
    if xs.size == 0:
        return EMPTY.copy()
    ys = np.flatnonzero(np.any(on, axis=1))
    return np.array([xs[0], ys[0], xs[-1] + plus, ys[-1] + plus, 0], dtype=np.float64)


def rows_of(masks, iscrowd, crowd_rows=False, plus=1):
    """Rows of one image from its final masks: crowds yield no row (fault crowd_rows: they do)."""
    out = [box_of(np.asarray(m) != 0, plus) for m, c in zip(masks, iscrowd) if crowd_rows or not int(c)]
    return np.array(out, dtype=np.float64).reshape(-1, 5)


def collate(rows_list, row_multiple=1):
    """bbox_collater: float32 [B, N, 5], N the largest row count (rounded up to row_multiple), padded with -1."""
    n = max(r.shape[0] for r in rows_list)
    n = (n + row_multiple - 1) // row_multiple * row_multiple
    out = np.full((len(rows_list), n, 5), -1.0, dtype=np.float32)
    for b, r in enumerate(rows_list):
        out[b, :r.shape[0]] = r
    return out


# ---- sampling -------------------------------------------------------------------------------------------------------------------

def frame_values(mask, geo, S, flip_w=None, **fault):
    """Float64 value and float32 error bound of every pixel of the (S + 1)^2 mask frame.  mask: [H, W], non-zero = 1.
    Faults: flip_w (flip over another width; the right one is S + 1), tap_shift / coord_off / A for the sampler."""
    v, u = np.meshgrid(np.arange(S + 1, dtype=np.float64), np.arange(S + 1, dtype=np.float64), indexing="ij")
    fw = S + 1 if flip_w is None else flip_w
    up = (float(fw) - 1.0) - u if geo["flip"] else u
    src = (np.asarray(mask) != 0).astype(np.uint8)[:, :, None]
    val, mag, vmax = ar._sample(src, geo, up, v, 0.0, **fault)
    return val[..., 0], ar.bound(mag[..., 0], vmax[..., 0], C_SUM_BOX)


def inner_outer(mask, geo, S, thr=0.5, plus=1, **fault):
    """(inner row, outer row, number of undecided pixels, number of pixels exactly at thr) of one instance."""
    val, b = frame_values(mask, geo, S, **fault)
    sure = val - b > thr
    maybe = val + b >= thr
    return box_of(sure, plus), box_of(maybe, plus), int((maybe & ~sure).sum()), int((val == thr).sum())


def check_row(got, inner, outer):
    """Is the device row between inner and outer?  Returns (ok, number of coordinates that were undecided)."""
    got = np.asarray(got, dtype=np.float64)
    if np.array_equal(inner, outer):
        return bool(np.array_equal(got, inner)), 0
    if inner[4] < 0:                                # surely-ON set empty, undecided pixels exist: the -1 row or a box inside outer
        if np.array_equal(got, EMPTY):
            return True, 4
        ok = got[4] == 0 and outer[0] <= got[0] < got[2] <= outer[2] and outer[1] <= got[1] < got[3] <= outer[3]
        return bool(ok), 4
    ok = got[4] == 0 and outer[0] <= got[0] <= inner[0] and outer[1] <= got[1] <= inner[1] and \
        inner[2] <= got[2] <= outer[2] and inner[3] <= got[3] <= outer[3]
    return bool(ok), int(np.sum(inner[:4] != outer[:4]))


def unpacked_view(mask, rect):
    """What a kernel WITHOUT the rectangle test would read: the packed rectangle (pitch rw) addressed with full-source coordinates,
    row wrap-around included; bytes before / after the rectangle's own buffer read as 0.  Fault model only."""
    H, W = mask.shape
    rx0, ry0, rw, rh = rect
    packed = (np.asarray(mask) != 0)[ry0:ry0 + rh, rx0:rx0 + rw].reshape(-1)
    yy, xx = np.mgrid[0:H, 0:W]
    idx = (yy - ry0) * rw + (xx - rx0)
    ok = (idx >= 0) & (idx < packed.size)
    return np.where(ok, packed[np.clip(idx, 0, packed.size - 1)], False).astype(np.uint8)


def rect_of(mask):
    xs, ys = np.flatnonzero(np.any(mask, axis=0)), np.flatnonzero(np.any(mask, axis=1))
    return int(xs[0]), int(ys[0]), int(xs[-1] - xs[0] + 1), int(ys[-1] - ys[0] + 1)


# ---- instance shapes ------------------------------------------------------------------------------------------------------------

def instance_shapes(seed, H, W):
    """Seven seeded binary masks [H, W] uint8: four ellipses, a rectangle, a one-pixel-wide line and a single pixel."""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    out = []
    for _ in range(4):
        cy, cx = rs.uniform(0.1, 0.9) * H, rs.uniform(0.1, 0.9) * W
        ry, rx = rs.uniform(0.04, 0.3) * H, rs.uniform(0.04, 0.3) * W
        out.append((((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 < 1.0).astype(np.uint8))
    m = np.zeros((H, W), dtype=np.uint8)
    y0, x0 = int(rs.uniform(0.1, 0.6) * H), int(rs.uniform(0.1, 0.6) * W)
    m[y0:y0 + int(rs.uniform(0.1, 0.35) * H), x0:x0 + int(rs.uniform(0.1, 0.35) * W)] = 1
    out.append(m)
    m = np.zeros((H, W), dtype=np.uint8)
    m[int(0.2 * H):int(0.8 * H), int(rs.uniform(0.3, 0.7) * W)] = 1
    out.append(m)
    m = np.zeros((H, W), dtype=np.uint8)
    m[int(rs.uniform(0.3, 0.7) * H), int(rs.uniform(0.3, 0.7) * W)] = 1
    out.append(m)
    return out


def synth_image(seed, H, W):
    return ar.synth_sources(seed, H, W)[0]
