"""Float64 restatement of the one-pass sampling of csrc/augment.hip (test-side only, like stream_ref.py; the product never
imports it), shared by tests/test_augment_cpu.py (teeth) and tests/test_augment_gpu.py (parity).

Every output element is mapped through flip -> crop origin -> inverse warpAffine matrix -> inverse resize to a source coordinate
in float64 IN THE KERNEL'S OPERATION ORDER (numpy's element-wise float64 operations are the same IEEE operations, nothing is fused
on either side), so the inside/outside decisions, the taps and the float32-rounded fractions are identical; from there on this
file works in float64 where the kernel works in float32: the cubic weight polynomials, the 16-term sum and the normalisation.

Besides the value, every function returns what the element-wise bound needs:
    mag   the same sum over absolute values, carried through the normalisation (|v| / 255 + |mean|) / std,
    wabs  the largest tap value, carried through the same scale factors (for the absolute term of the weight polynomials).

BOUND (derived from operation counts, never tuned; u = 2^-24):
    |got - ref| <= C_SUM * u * mag + W_ABS * u * wabs
  * C_SUM: one rounding per product v * wx, three additions along a row, one product with wy, three additions down the column:
    8 roundings on the longest path to the sum (the uint8 -> float32 conversions and the clamp are exact), each at most u times
    the running sum of absolute values; then / 255, - mean, / std for the image (3 more) or / 255 for the mask (1 more); plus 1
    for the second-order terms of (1 + u)^n.  Image 8 + 3 + 1 = 12, mask 8 + 1 + 1 = 10.
  * W_ABS: the float32 weights against the float64 polynomial AT THE SAME float32 fraction t (the fraction is rounded to float32
    on both sides).  Operation count of OpenCV's interpolateCubic, A = -0.75, y = t + 1 in [1, 2):
      c0 = ((A y - 5A) y + 8A) y - 4A : rounding of y (<= u, |dc0/dy| <= 0.75); A y (|.| <= 1.5, amplified by y^2 <= 4) 6u;
           + 3.75 (<= 3) 12u; * y (<= 4.5, amplified by y <= 2) 9u; - 6 (<= 3) 6u; * y (<= 3.2) 3.2u; + 3 (<= 0.1) 0.1u  -> 37.05u <= 40u
      c1 = ((A + 2) t - (A + 3)) t t + 1 : five roundings of values <= 2.25, amplification <= 1                           -> 11.25u <= 12u
      c2 = c1 at 1 - t, whose own rounding (<= u / 2) passes through |dc2/dt| <= 1.5                                        -> <= 14u
      c3 = 1 - c0 - c1 - c2 : the three errors above plus three roundings of values <= 1.1                                  -> <= 70u
    so the four weights of one axis are off by at most 136u in total (tests/test_augment_cpu.py checks that figure against the
    float32 oracle of the weights on a dense grid).  With sum |w| <= 1.375 per axis (its maximum, at t = 0.5), the 16 products
    wy wx are off by at most 2 * 1.375 * 136u = 374u in total, each multiplying a tap value of at most wabs.
"""
import numpy as np

U24 = 2.0 ** -24
C_SUM_IMAGE, C_SUM_MASK = 12.0, 10.0
W_AXIS = 136.0
W_ABS = 2 * 1.375 * W_AXIS

MEANS = (0.485, 0.456, 0.406)
STDS = (0.229, 0.224, 0.225)


def cubic_weights64(t, A=-0.75):
    """interpolateCubic in float64 for an array of fractions; returns [..., 4]."""
    t = np.asarray(t, dtype=np.float64)
    y = t + 1.0
    c0 = ((A * y - 5.0 * A) * y + 8.0 * A) * y - 4.0 * A
    c1 = ((A + 2.0) * t - (A + 3.0)) * t * t + 1.0
    z = 1.0 - t
    c2 = ((A + 2.0) * z - (A + 3.0)) * z * z + 1.0
    c3 = 1.0 - c0 - c1 - c2
    return np.stack([c0, c1, c2, c3], axis=-1)


def invert_affine(M):
    """2x3 inverse in the operation order of warpAffine's own inversion (the product's host code does the same operations)."""
    D = M[0, 0] * M[1, 1] - M[0, 1] * M[1, 0]
    D = 1.0 / D if D != 0 else 0.0
    iM = np.zeros((2, 3), dtype=np.float64)
    iM[0, 0], iM[0, 1], iM[1, 0], iM[1, 1] = M[1, 1] * D, M[0, 1] * (-D), M[1, 0] * (-D), M[0, 0] * D
    iM[0, 2] = -iM[0, 0] * M[0, 2] - iM[0, 1] * M[1, 2]
    iM[1, 2] = -iM[1, 0] * M[0, 2] - iM[1, 1] * M[1, 2]
    return iM


def geometry(M, scale, scaled_hw, canvas_hw, origin, flip):
    """The numbers one sample's sampling needs, from recorded values (golden) or from the product's host geometry."""
    return {"Minv": invert_affine(np.asarray(M, dtype=np.float64)), "scale": float(scale), "nh": int(scaled_hw[0]), "nw": int(scaled_hw[1]),
            "nH": int(canvas_hw[0]), "nW": int(canvas_hw[1]), "ox": int(origin[0]), "oy": int(origin[1]), "flip": bool(flip)}


def _sample(src, geo, px, py, border, A=-0.75, tap_shift=0, coord_off=0.0):
    """src [H, W, C] uint8; (px, py) float64 crop-space points with the flip already undone.  Returns value (clamped to [0, 255]),
    sum over absolute values, largest tap, each [..., C] float64."""
    H, W, C = src.shape
    m = geo["Minv"]
    xr = float(geo["ox"]) + px
    yr = float(geo["oy"]) + py
    inside = (xr >= -0.5) & (xr < geo["nW"] - 0.5) & (yr >= -0.5) & (yr < geo["nH"] - 0.5)
    xs = (m[0, 0] * xr + m[0, 1] * yr) + m[0, 2]
    ys = (m[1, 0] * xr + m[1, 1] * yr) + m[1, 2]
    inside &= (xs >= -0.5) & (xs < geo["nw"] - 0.5) & (ys >= -0.5) & (ys < geo["nh"] - 0.5)
    sx = (xs + 0.5) / geo["scale"] - 0.5 + coord_off
    sy = (ys + 0.5) / geo["scale"] - 0.5 + coord_off
    sx, sy = np.where(inside, sx, 0.0), np.where(inside, sy, 0.0)
    fx, fy = np.floor(sx), np.floor(sy)
    wx = cubic_weights64((sx - fx).astype(np.float32).astype(np.float64), A)
    wy = cubic_weights64((sy - fy).astype(np.float32).astype(np.float64), A)
    ix = np.clip(fx, -4.0, W + 4.0).astype(np.int64)
    iy = np.clip(fy, -4.0, H + 4.0).astype(np.int64)
    s = src.astype(np.float64)
    val = np.zeros(px.shape + (C,))
    mag = np.zeros(px.shape + (C,))
    vmax = np.zeros(px.shape + (C,))
    for k in range(4):
        yk = np.clip(iy - 1 + k + tap_shift, 0, H - 1)
        for l in range(4):
            xl = np.clip(ix - 1 + l + tap_shift, 0, W - 1)
            v = s[yk, xl]
            w = (wy[..., k] * wx[..., l])[..., None]
            val += w * v
            mag += np.abs(w) * v
            vmax = np.maximum(vmax, v)
    ins = inside[..., None]
    val = np.where(ins, np.clip(val, 0.0, 255.0), float(border))
    mag = np.where(ins, mag, float(border))
    vmax = np.where(ins, vmax, 0.0)
    return val, mag, vmax


def image_ref(src_bgr, geo, crop_y, crop_x, swap=True, flip_w=None, **fault):
    """[3, crop_y, crop_x] float64: value, mag, wabs.  Faults (teeth test): swap=False leaves BGR, flip_w flips over another width,
    A / tap_shift / coord_off go to the sampler."""
    v, u = np.meshgrid(np.arange(crop_y, dtype=np.float64), np.arange(crop_x, dtype=np.float64), indexing="ij")
    fw = crop_x if flip_w is None else flip_w
    up = (fw - 1) - u if geo["flip"] else u
    val, mag, vmax = _sample(src_bgr, geo, up, v, 128.0, **fault)
    mean = np.array(MEANS, dtype=np.float32).astype(np.float64)
    std = np.array(STDS, dtype=np.float32).astype(np.float64)
    order = [2, 1, 0] if swap else [0, 1, 2]
    val, mag, vmax = (a[..., order].transpose(2, 0, 1) for a in (val, mag, vmax))
    out = (val / 255.0 - mean[:, None, None]) / std[:, None, None]
    mag = (mag / 255.0 + np.abs(mean)[:, None, None]) / std[:, None, None]
    return out, mag, vmax / 255.0 / std[:, None, None]


def mask_ref(src_mask, geo, gh, gw, stride, crop_x, flip_w=None, **fault):
    """[gh, gw] float64 (one channel; the kernel writes it 18 times): value, mag, wabs."""
    i, j = np.meshgrid(np.arange(gh, dtype=np.float64), np.arange(gw, dtype=np.float64), indexing="ij")
    px = (j + 0.5) * float(stride) - 0.5
    py = (i + 0.5) * float(stride) - 0.5
    fw = crop_x + 1 if flip_w is None else flip_w
    pf = (float(fw) - 1.0) - px if geo["flip"] else px
    val, mag, vmax = _sample(src_mask[:, :, None], geo, pf, py, 255.0, **fault)
    return val[..., 0] / 255.0, mag[..., 0] / 255.0, vmax[..., 0] / 255.0


def bound(mag, wabs, c_sum):
    return c_sum * U24 * mag + W_ABS * U24 * wabs


def ratio(got, ref, mag, wabs, c_sum):
    """|got - ref| / bound per element; an element whose bound is 0 (all 16 taps are 0) must be exact: 0 or inf.  NaN counts as inf."""
    err, b = np.abs(np.asarray(got, dtype=np.float64) - ref), bound(mag, wabs, c_sum)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(b > 0, err / b, np.where(err > 0, np.inf, 0.0))
    return np.where(np.isnan(r), np.inf, r)


def synth_sources(seed, H, W):
    """Seeded decoded-sample stand-in: BGR uint8 [H, W, 3] (channel-dependent smooth pattern plus noise, so a wrong kernel, a wrong
    channel order or a shifted coordinate is far outside the bound) and a mask_miss uint8 [H, W] (255 with a few 0 blobs)."""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    img = np.stack([125 + 80 * np.sin(xx / (11.0 + 3 * c) + c) * np.cos(yy / (17.0 - 2 * c) - c) for c in range(3)], 2)
    img += rs.uniform(-25, 25, size=img.shape)
    mask = np.full((H, W), 255.0)
    for _ in range(6):
        cy, cx, r = rs.uniform(0, H), rs.uniform(0, W), rs.uniform(0.05, 0.2) * min(H, W)
        mask[(yy - cy) ** 2 + (xx - cx) ** 2 < r * r] = 0.0
    mask += rs.uniform(-3, 0, size=mask.shape) * (mask > 0)
    return np.clip(np.round(img), 0, 255).astype(np.uint8), np.clip(np.round(mask), 0, 255).astype(np.uint8)


def golden_cases():
    """The recorded cases of tests/golden/g17_augment.npz as (index, dict of arrays)."""
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g17_augment.npz"), allow_pickle=False)
    n = int(g["n_cases"])
    out = []
    for i in range(n):
        pre = "c%d_" % i
        out.append({k[len(pre):]: g[k] for k in g.files if k.startswith(pre)})
    return out, int(g["inp_stride"][0]), int(g["inp_stride"][1])


PARAM_KEYS = ("scale_min", "scale_max", "scale_prob", "target_dist", "max_rotate_degree", "center_perterb_max", "flip_prob")


def case_params(case):
    return {k: float(v) for k, v in zip(PARAM_KEYS, case["params"])}
