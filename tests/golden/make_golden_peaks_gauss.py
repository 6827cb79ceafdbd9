#!/usr/bin/env python3
"""Golden vectors for the smoothed peak refinement: the REAL reference ``network/joint_utils.py: NMS(..., bool_gaussian_filt=True)``
with the REAL ``scipy.ndimage`` (``gaussian_filter``, ``maximum_filter``).  cv2 is not needed: a stand-in module is pre-seeded whose
``resize`` is oracle/joint_oracle.py's ``cv_resize_cubic`` (pinned separately, tests/test_postproc_parity_cpu.py).

Per case (18 planes each) the file holds the heat-maps, the factor, the result rows with the flag on and off, and — for a handful of
peaks — the up-sampled patch handed to ``gaussian_filter`` and what it returned; plus scipy's 25 weights for sigma 3.  Arrays only.

Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_peaks_gauss.py <directory of the reference checkout>
"""
import os
import sys
import types

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from oracle import joint_oracle as jo  # noqa: E402

J = 18
THRE1 = 0.1
KEEP_PATCHES = 6                    # recorded (up-sampled, smoothed) patch pairs per case, at most ...
KEEP_CELLS = 2600                   # ... this many cells together (the file stays at a few tens of KB)


def load_reference(ref_root):
    cv2 = types.ModuleType("cv2")
    cv2.INTER_CUBIC = 2

    def resize(src, dsize, fx=0.0, fy=0.0, interpolation=None):
        assert dsize is None and fx == fy and interpolation == cv2.INTER_CUBIC
        return jo.cv_resize_cubic(src, fx)

    cv2.resize = resize
    sys.modules["cv2"] = cv2
    sys.path.insert(0, ref_root)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")             # scipy.ndimage.filters is a deprecated namespace of the same functions
        from network import joint_utils
    import scipy.ndimage
    assert joint_utils.gaussian_filter is scipy.ndimage.gaussian_filter and joint_utils.maximum_filter is scipy.ndimage.maximum_filter
    return joint_utils


def blob(heat, j, cx, cy, amp, s):
    H, W = heat.shape[:2]
    yy, xx = np.mgrid[0:H, 0:W]
    g = (amp * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * s * s))).astype(np.float32)
    heat[:, :, j] += np.where(g > 0.004, g, np.float32(0))          # cut tails: the far field stays the (compressible) noise grid


def base(seed, H, W, noise=0.02):
    rng = np.random.RandomState(seed)
    return rng, (rng.randint(0, 8, size=(H, W, J)) * (noise / 8.0)).astype(np.float32)          # eight levels below `noise`


def blobs_case(seed, H, W, noise=0.03):
    """Interior blobs with sub-pixel centres, blobs on every edge and corner, pairs of close blobs of unequal height."""
    rng, heat = base(seed, H, W, noise)
    for j in range(0, 6):                                   # interior
        for _ in range(1 + j % 3):
            blob(heat, j, rng.uniform(3, W - 4), rng.uniform(3, H - 4), rng.uniform(0.3, 1.0), rng.uniform(0.8, 1.6))
    edge = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W / 2.0 + 0.3, 0), (0, H / 2.0 - 0.3), (W - 1, H / 2.0 + 0.4), (W / 2.0 - 0.4, H - 1)]
    for j in range(6, 10):                                  # edges and corners
        for cx, cy in edge[(j - 6) * 2:(j - 6) * 2 + 2]:
            blob(heat, j, cx, cy, rng.uniform(0.4, 0.9), rng.uniform(0.9, 1.4))
    for j in range(10, 16):                                 # two close blobs of unequal height: smoothing pulls the maximum across
        cx, cy = rng.uniform(4, W - 6), rng.uniform(4, H - 5)
        blob(heat, j, cx, cy, 0.9, 0.7)
        blob(heat, j, cx + rng.uniform(1.6, 2.4), cy + rng.uniform(-1.2, 1.2), rng.uniform(0.6, 0.85), 1.1)
    blob(heat, 16, 1.3, 1.4, 0.7, 1.0)                      # one cell off the corner: 4 x 4 source patch
    blob(heat, 16, W - 2.2, H - 2.4, 0.6, 1.0)
    return heat                                             # plane 17: noise only (no peak above thre1)


def plateau_case(seed, H, W):
    """Exact ties: ridges (constant along one axis), small plateaus, on an exactly zero background."""
    heat = np.zeros((H, W, J), dtype=np.float32)
    heat[H // 2, :, 0] = 0.5                                # horizontal ridge: every cell of it is a peak
    heat[:, W // 3, 1] = 0.75                               # vertical ridge
    heat[3:5, 4:6, 2] = 0.5                                 # 2 x 2 plateau
    heat[5:8, 6:9, 3] = 0.625                               # 3 x 3 plateau
    heat[0, :, 4] = 0.25                                    # ridge on the top border
    heat[:, W - 1, 5] = 0.375                               # ridge on the right border
    heat[2, 2:7, 6] = 0.5                                   # 1 x 5 bar
    heat[2:4, :, 7] = 0.5                                   # two-row band
    rng = np.random.RandomState(seed)
    for j in range(8, 12):
        blob(heat, j, rng.uniform(3, W - 4), rng.uniform(3, H - 4), 0.8, 1.2)
    return heat


def order_sensitive_case(H, W, want=3):
    """f = 1 (the up-sampled patch IS the source patch).  The order of correlate1d's float64 sum shows in a float32 result only when the
    sum lies within a float64 ulp or two of a float32 rounding boundary (about once in 2^29 values), so such patches are built: two
    background cells of a 5 x 5 patch are tuned — a coarse one up to the last value that leaves the peak's smoothed score unchanged,
    then a fine one (some 1e-14) by bisection over float32 values to the first value that raises it.  Where that value differs between
    the reference order (k = 12 .. 1) and the ascending order, the plane is kept: the two orders then give different score bits."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import peaks_gauss_ref as pg
    heat = np.zeros((H, W, J), dtype=np.float32)
    py, px = H // 2, W // 2
    f32 = np.float32
    ordinal = lambda v: int(f32(v).view(np.int32))
    value = lambda n: np.int32(n).view(np.float32)
    rng = np.random.RandomState(38)
    kept = 0
    for trial in range(200):
        if kept == min(want, J):
            break
        patch = np.zeros((5, 5), dtype=np.float32)
        patch[1:4, 1:4] = rng.uniform(0.2, 0.6, (3, 3)).astype(np.float32)
        patch[2, 2] = f32(rng.uniform(0.7, 0.95))

        def score(desc, d1, d2):
            p = patch.copy()
            p[0, 0], p[0, 4] = d1, d2
            return pg.gaussian_filter_f32(p, k_descending=desc).max()

        def first_raise(fn, lo, hi, base):
            """smallest float32 ordinal n in (lo, hi] with fn(value(n)) > base; fn is non-decreasing"""
            assert fn(value(lo)) == base < fn(value(hi))
            while hi - lo > 1:
                mid = (lo + hi) // 2
                lo, hi = (lo, mid) if fn(value(mid)) > base else (mid, hi)
            return hi

        r0 = score(True, f32(0), f32(0))
        d1 = value(first_raise(lambda v: score(True, v, f32(0)), 0, ordinal(1e-3), r0) - 1)
        if score(False, d1, f32(0)) != r0:
            continue
        t_desc = first_raise(lambda v: score(True, d1, v), 0, ordinal(1e-6), r0)
        t_asc = first_raise(lambda v: score(False, d1, v), 0, ordinal(1e-6), r0)
        if t_desc == t_asc:
            continue
        d2 = value(min(t_desc, t_asc))
        assert score(True, d1, d2) != score(False, d1, d2)
        patch[0, 0], patch[0, 4] = d1, d2
        heat[py - 2:py + 3, px - 2:px + 3, kept] = patch
        kept += 1
    assert kept >= 1, "no order-sensitive patch found"
    return heat


def run_case(ju, heat, f, data, name):
    param = {"thre1": THRE1}
    seen = []
    real = ju.gaussian_filter

    def recording(a, sigma):
        out = real(a, sigma=sigma)
        seen.append((np.array(a, copy=True), out))
        return out

    ju.gaussian_filter = recording
    try:
        on = ju.NMS(param, heat, f, bool_refine_center=True, bool_gaussian_filt=True)
    finally:
        ju.gaussian_filter = real
    off = ju.NMS(param, heat, f, bool_refine_center=True, bool_gaussian_filt=False)
    plain = ju.NMS(param, heat, f, bool_refine_center=False, bool_gaussian_filt=True)
    cat = lambda per: np.concatenate([np.concatenate([p.reshape(-1, 4), np.full((len(p), 1), float(j))], 1) for j, p in enumerate(per)])
    data["heat_" + name] = heat
    data["f_" + name] = np.array(float(f))
    data["on_" + name], data["off_" + name], data["plain_" + name] = cat(on), cat(off), cat(plain)
    assert all(a.dtype == np.float32 and o.dtype == np.float32 for a, o in seen)
    # the first patch of every distinct shape, then the first ones seen, up to KEEP_PATCHES
    order, shapes = [], set()
    for i, (a, _) in enumerate(seen):
        if a.shape not in shapes:
            shapes.add(a.shape)
            order.append(i)
    order += [i for i in range(len(seen)) if i not in order]
    kept, cells = [], 0
    for i in order:
        if len(kept) < KEEP_PATCHES and cells + seen[i][0].size <= KEEP_CELLS:
            kept.append(i)
            cells += seen[i][0].size
    kept = kept or [min(order, key=lambda i: seen[i][0].size)]
    for n, i in enumerate(kept):
        data["up_%s_%d" % (name, n)], data["sm_%s_%d" % (name, n)] = seen[i]
    data["npatch_" + name] = np.array(len(kept))
    return len(seen), sorted(shapes)


def cases():
    tworow = base(36, 2, 20)[1]
    for j in range(8):
        blob(tworow, j, 1.5 + 2.3 * j, 0.3 * (j % 4), 0.4 + 0.05 * j, 1.3)
    return (("c1", blobs_case(31, 16, 20), 4.0), ("c2", blobs_case(32, 12, 16), 1.0), ("c3", blobs_case(33, 14, 18), 2.5),
            ("c4", blobs_case(34, 20, 24), 8.0), ("c5", blobs_case(35, 12, 16), 12.8), ("c6", tworow, 4.0),
            ("c7", plateau_case(37, 12, 16), 1.0), ("c8", order_sensitive_case(12, 16), 1.0))


def main():
    ju = load_reference(sys.argv[1])
    from scipy.ndimage import _filters
    data = {"weights": np.asarray(_filters._gaussian_kernel1d(3.0, 0, 12)[::-1], dtype=np.float64)}
    for name, heat, f in cases():
        n, shapes = run_case(ju, heat, f, data, name)
        on, off = data["on_" + name], data["off_" + name]
        same_score = int((on[:, 2].astype(np.float32).view(np.uint32) == off[:, 2].astype(np.float32).view(np.uint32)).sum())
        moved = int((on[:, :2] != off[:, :2]).any(1).sum())
        print("%s f=%-5g map %dx%d: %3d peaks, %d keep their score bits, %d move; patch shapes %s" % (name, f, heat.shape[0], heat.shape[1], n, same_score, moved, shapes))
    path = os.path.join(HERE, "g20_peaks_gauss.npz")
    np.savez_compressed(path, **data)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
