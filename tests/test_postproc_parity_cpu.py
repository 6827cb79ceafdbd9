"""CPU side of the post-processing parity tests (tests/postproc_ref.py holds the references and the derivation of the bounds).

1. oracle/joint_oracle.py's restatement of cv2.resize (`cv_resize`, `cv_resize_cubic` through `nms_peaks(refine=True)`) is held to
   the independent float64 references under the same bounds and rules the GPU tests apply to the kernels: this pins the oracle, and
   shows that the bounds accept a correct float32 implementation.
2. A plain float32 model of the same arithmetic (below) passes too, and every modelled fault applied to it is rejected on at least one
   case: the bounds are tight enough to see the misreadings they are meant to see.
3. The share of undecided peaks (see postproc_ref) is asserted on the reference alone, before any comparison.
No GPU is needed."""
import numpy as np
import pytest
import torch

import postproc_ref as pr
from oracle import joint_oracle as jo

f32, f64 = np.float32, np.float64


# ------------------------------------------------------------------------------------------------ float32 model with fault switches
def model_coeffs(t, A):
    A, one = f32(A), f32(1)
    y = t + one
    c0 = ((A * y - f32(5) * A) * y + f32(8) * A) * y - f32(4) * A
    c1 = ((A + f32(2)) * t - (A + f32(3))) * t * t + one
    z = one - t
    c2 = ((A + f32(2)) * z - (A + f32(3))) * z * z + one
    return np.stack([c0, c1, c2, one - c0 - c1 - c2], 1).astype(f32)


def model_axis(n_dst, n_src, scale, cubic, fault):
    """(tap indices [n, K], tap validity [n, K] (0 where a faulty tap reads nothing), float32 weights [n, K])."""
    d = np.arange(n_dst, dtype=f64)
    if fault == "align_corners":
        s = d * ((n_src - 1.0) / (n_dst - 1.0) if n_dst > 1 else 0.0)
    else:
        s = (d + 0.5) * scale - 0.5
    fx = s.astype(f32)
    sx = (np.trunc(fx) if fault == "trunc" else np.floor(fx)).astype(np.int64)
    t = (fx - sx.astype(f32)).astype(f32)
    if cubic:
        co = model_coeffs(t, -0.5 if fault == "A" else -0.75)
        raw = sx[:, None] - 1 + np.arange(4)[None, :]
    else:
        low, high = sx < 0, sx >= n_src - 1
        t = np.where(low, f32(0), t)
        sx = np.where(low, 0, sx)
        if fault != "noclamp":
            t = np.where(high, f32(0), t)
            sx = np.where(high, n_src - 1, sx)
        co = np.stack([f32(1) - t, t], 1).astype(f32)
        raw = np.stack([sx, sx + 1], 1)
    clipped, ones = raw.clip(0, n_src - 1), np.ones_like(co)
    if fault == "wrap":
        return raw % n_src, ones, co
    if fault == "zero_pad":
        return clipped, ((raw >= 0) & (raw <= n_src - 1)).astype(f32), co
    if fault == "noclamp" and not cubic:
        # the second tap now lies past the edge with a weight above 0 and reads nothing (the clamp gives it weight 0 first)
        return clipped, (raw <= n_src - 1).astype(f32), co
    return clipped, ones, co


def model_resize(img, out_hw, cubic, inv_scale=None, fault=None):
    img = np.asarray(img, dtype=f32)
    Hs, Ws, _ = img.shape
    Hd, Wd = int(out_hw[0]), int(out_hw[1])
    if inv_scale is None or fault == "src_over_dst":
        sy, sx = float(Hs) / Hd, float(Ws) / Wd
    else:
        sy, sx = float(inv_scale[0]), float(inv_scale[1])
    if fault == "swap":
        sy, sx = sx, sy
    xi, xv, xc = model_axis(Wd, Ws, sx, cubic, fault)
    yi, yv, yc = model_axis(Hd, Hs, sy, cubic, fault)
    rows = None
    for k in range(xi.shape[1]):
        term = img[:, xi[:, k], :] * xv[None, :, k, None] * xc[None, :, k, None]
        rows = term if rows is None else rows + term
    out = None
    for k in range(yi.shape[1]):
        term = rows[yi[:, k]] * yv[:, k, None, None] * yc[:, k, None, None]
        out = term if out is None else out + term
    return out.astype(f32)


def model_nms(heat_jhw, thre1, f, fault=None):
    """Rows (x, y, score, id) per joint type from the float32 model."""
    J, H, W = heat_jhw.shape
    out, cnt = [], 0
    for j in range(J):
        rows = []
        for (px, py) in pr.find_peaks_ref(heat_jhw[j], thre1):
            x0, y0, x1, y1 = max(0, px - 2), max(0, py - 2), min(W - 1, px + 2), min(H - 1, py + 2)
            patch = heat_jhw[j, y0:y1 + 1, x0:x1 + 1]
            size = (lambda n: int(np.floor(n * f))) if fault == "floor_dsize" else (lambda n: pr.dsize(n, f))
            up = model_resize(patch[:, :, None], (size(patch.shape[0]), size(patch.shape[1])), True, (1.0 / f, 1.0 / f), fault)[:, :, 0]
            flat = up.reshape(-1)
            am = int(flat.size - 1 - np.argmax(flat[::-1])) if fault == "last_max" else int(np.argmax(flat))
            by, bx = am // up.shape[1], am % up.shape[1]
            rows.append((pr.final_coord(px, x0, bx, f), pr.final_coord(py, y0, by, f), float(up[by, bx]), float(cnt)))
            cnt += 1
        out.append(np.array(rows, dtype=f64).reshape(-1, 4))
    return out


def model_decode(an, d, mean_std, img_w, img_h, clip, fault=None):
    an, d = np.asarray(an, dtype=f32), np.asarray(d, dtype=f32)
    B, A, _ = d.shape
    ms = np.array(pr.DEFAULT_MEAN_STD if mean_std is None else mean_std, dtype=f32)
    i = np.arange(B * A)
    a = an[(i // A if fault == "div" else i % A)].reshape(B, A, 4)
    half = f32(0.5)
    w, h = a[..., 2] - a[..., 0], a[..., 3] - a[..., 1]
    cx, cy = a[..., 0] + half * w, a[..., 1] + half * h
    if fault == "std_after_mean":
        t = (d + ms[None, None, :4]) * ms[None, None, 4:]
    else:
        t = d * ms[None, None, 4:] + ms[None, None, :4]
    pcx, pcy = cx + t[..., 0] * w, cy + t[..., 1] * h
    with np.errstate(over="ignore"):
        pw, ph = np.exp(t[..., 2]) * w, np.exp(t[..., 3]) * h
    out = np.stack([pcx - half * pw, pcy - half * ph, pcx + half * pw, pcy + half * ph], -1).astype(f32)
    if clip:
        out[..., 0], out[..., 1] = np.maximum(out[..., 0], 0), np.maximum(out[..., 1], 0)
        out[..., 2] = np.minimum(out[..., 2], f32(img_h if fault == "clip_x2_h" else img_w))
        out[..., 3] = np.minimum(out[..., 3], f32(img_h))
    return out


# ------------------------------------------------------------------------------------------------ cases
def resize_cases():
    """(name, image, out_hw, cubic, inv_scale) of the case table and the fx / fy form."""
    out = []
    for c in pr.RESIZE_CASES:
        for cubic in (True, False):
            out.append(("%dx%dx%d->%dx%d %s" % (c + ("cubic" if cubic else "linear",)), pr.resize_input(*c[:3]), c[3:], cubic, None))
    for f in pr.FX_FACTORS:
        img, hw, inv = pr.fx_case(f)
        for cubic in (True, False):
            out.append(("fx=%g %s" % (f, "cubic" if cubic else "linear"), img, hw, cubic, inv))
    return out


PEAK_CASES = [(m, f) for m in pr.PEAK_MAPS for f in pr.PEAK_FACTORS]


# ------------------------------------------------------------------------------------------------ the constants of the derivation
def test_coefficient_constants_of_the_derivation():
    t = np.linspace(0.0, 1.0, 200001)
    c, err, rho = pr.coeff_model(t)
    A = pr.A_CUBIC
    closed = np.stack([A * t * (1 - t) ** 2, (A + 2) * t ** 3 - (A + 3) * t ** 2 + 1, (A + 2) * (1 - t) ** 3 - (A + 3) * (1 - t) ** 2 + 1,
                       A * (1 - t) * t ** 2])
    assert np.abs(c - closed).max() < 1e-14
    d = pr.coeff_derivs(t)
    assert np.abs(d.sum(0)).max() < 1e-14                                   # the weights sum to one identically
    assert np.abs(np.gradient(closed, t, axis=1)[:, 1:-1] - d[:, 1:-1]).max() < 1e-4
    assert np.abs(d).sum(0).max() <= pr.DC_CUBIC + 1e-12 and np.abs(d).sum(0)[[0, -1]].tolist() == [1.5, 1.5]
    assert np.abs(c).sum(0).max() <= pr.L_CUBIC_MAX + 1e-12
    assert err.sum(0).max() <= 29.5 * pr.U and rho.max() <= 2.5 * pr.U     # the figures quoted in postproc_ref's docstring


def test_coefficient_error_model_covers_float32():
    """The running-error model bounds the float32 evaluation of cubic_coeffs at every float32 t of a dense sweep."""
    t = np.unique(np.concatenate([np.linspace(0, 1, 300001)[:-1], np.random.RandomState(3).rand(300000)]).astype(f32))
    t = t[t < 1]
    got = model_coeffs(t, -0.75).astype(f64).T
    c, err, rho = pr.coeff_model(t.astype(f64))
    e = np.abs(got - c)
    assert (e[:3] <= err).all() and (e[3] <= err.sum(0) + rho).all()
    assert (np.abs(e[:3].sum(0)) > 0).any()


# ------------------------------------------------------------------------------------------------ oracle and model within the bounds
@pytest.mark.parametrize("impl", ["oracle", "model"])
def test_resize_float32_implementations_within_bounds(impl):
    fn = jo.cv_resize if impl == "oracle" else model_resize
    for name, img, hw, cubic, inv in resize_cases():
        got = fn(img, hw, cubic, inv)
        pr.check_resize("%s %s" % (impl, name), got, img, hw, cubic, inv, route="cpu float32 vs torch float64")
        if tuple(hw) == img.shape[:2] and inv is None:
            assert np.array_equal(got, img), name                            # identity
        if impl == "model":
            assert np.array_equal(got, jo.cv_resize(img, hw, cubic, inv)), name  # the model is the oracle's arithmetic, bit for bit


@pytest.mark.parametrize("name,f", PEAK_CASES)
def test_undecided_cap_then_oracle_and_model_peaks(name, f):
    heat, thre, expect = pr.peak_case(name, f)
    for b in range(heat.shape[0]):                                           # from the reference alone, before any comparison
        share, n = pr.undecided_share(expect[b])
        assert n > 0 and share <= 0.05, (name, f, b, n, share)
    for b in range(heat.shape[0]):
        tag = "%s f=%g image %d" % (name, f, b)
        oracle = jo.nms_peaks(thre, np.ascontiguousarray(heat[b].transpose(1, 2, 0)), f, refine=True)
        pr.check_peak_rows("oracle nms_peaks " + tag, oracle, expect[b], f, route="cpu float32 vs torch float64")
        model = model_nms(heat[b], thre, f)
        assert all(np.array_equal(m, o) for m, o in zip(model, oracle)), tag
    # at f = 1.5 the patch origin lands on k + 1/2 and rint (half to even) maps two neighbouring cells to one final coordinate
    # (1.5 + 0 -> 2, 1.5 + 1 -> 2): check_peak_rows then cannot tell the two apart from the device's row and accepts either
    assert (pr.colliding_peaks(expect, f) > 0) == (f == 1.5), (name, f)
    if f == 13.0:
        wide = [p["dw"] for b in expect for r in b for p in r]
        assert max(wide) == 65 and (name != "noise" or min(wide) == 39)


def test_exact_tie_takes_the_first_maximum():
    """tie_map at f = 4: every operation is exact in float32, so a float32 implementation equals the float64 reference bit for bit and
    the four-way tie must resolve to the first cell in row-major order."""
    heat, thre, expect = pr.peak_case("tie", 4.0)
    (p,) = [q for r in expect[0] for q in r]
    up = p["up"]
    assert p["gap"] == 0.0 and p["am"] == (9, 9) and up[9, 9] == up[9, 10] == up[10, 9] == up[10, 10] == up.max()
    assert np.array_equal(up * 2.0 ** 23, np.rint(up * 2.0 ** 23))            # multiples of 2^-23 below 2: exact in float32
    assert np.array_equal(jo.cv_resize_cubic(heat[0, 0, 2:7, 2:7], 4.0).astype(f64), up)
    oracle = jo.nms_peaks(thre, np.ascontiguousarray(heat[0].transpose(1, 2, 0)), 4.0, refine=True)
    pr.check_peak_rows("oracle tie", oracle, expect[0], 4.0, route="cpu exact", exact_scores=True)
    assert pr.check_peak_rows("model tie", model_nms(heat[0], thre, 4.0), expect[0], 4.0, exact_scores=True, raise_on_fail=False) is None
    bad = pr.check_peak_rows("model last maximum", model_nms(heat[0], thre, 4.0, "last_max"), expect[0], 4.0, exact_scores=True, raise_on_fail=False)
    assert bad is not None, "keeping the last maximum of an exact tie was accepted"


# ------------------------------------------------------------------------------------------------ modelled faults
RESIZE_FAULTS = ["A", "align_corners", "wrap", "zero_pad", "src_over_dst", "trunc", "noclamp", "swap"]


@pytest.mark.parametrize("fault", RESIZE_FAULTS)
def test_modelled_resize_fault_is_rejected(fault):
    rejected = []
    for name, img, hw, cubic, inv in resize_cases():
        got = model_resize(img, hw, cubic, inv, fault)
        if pr.check_resize(name, got, img, hw, cubic, inv, raise_on_fail=False) > 1.0:
            rejected.append(name)
    assert rejected, "no resize case rejects the fault %r" % fault


@pytest.mark.parametrize("fault", ["A", "align_corners", "wrap", "zero_pad", "src_over_dst", "trunc", "floor_dsize"])
def test_modelled_refinement_fault_is_rejected(fault):
    rejected = []
    for name, f in [("noise", 4.27), ("noise", 1.5), ("a", 13.0)]:
        heat, thre, expect = pr.peak_case(name, f)
        if pr.check_peak_rows(name, model_nms(heat[0], thre, f, fault), expect[0], f, raise_on_fail=False) is not None:
            rejected.append((name, f))
    assert rejected, "no peak case rejects the fault %r" % fault


@pytest.mark.parametrize("mean_std", [None, pr.NONDEFAULT_MEAN_STD], ids=["default", "nondefault"])
@pytest.mark.parametrize("clip", [True, False])
def test_decode_model_within_bound(mean_std, clip):
    an, d = pr.decode_inputs(mean_std)
    got = model_decode(an, d, mean_std, pr.IMG_W, pr.IMG_H, clip)
    pr.check_decode("decode model clip=%s %s" % (clip, "default" if mean_std is None else "nondefault"), got, an, d, mean_std, pr.IMG_W,
                    pr.IMG_H, clip, route="cpu float32 vs float64")
    t = d[:, :, 2].astype(f64) * (0.2 if mean_std is None else f64(f32(mean_std[6]))) + (0.0 if mean_std is None else f64(f32(mean_std[2])))
    assert t.min() < -7.99 and t.max() > 7.99


@pytest.mark.parametrize("fault", ["div", "std_after_mean", "clip_x2_h"])
def test_modelled_decode_fault_is_rejected(fault):
    rejected = []
    for mean_std in (None, pr.NONDEFAULT_MEAN_STD):
        an, d = pr.decode_inputs(mean_std)
        got = model_decode(an, d, mean_std, pr.IMG_W, pr.IMG_H, True, fault)
        if pr.check_decode(fault, got, an, d, mean_std, pr.IMG_W, pr.IMG_H, True, raise_on_fail=False) > 1.0:
            rejected.append(mean_std)
    assert rejected, "no decode case rejects the fault %r" % fault


def test_decode_saturating_ends_of_exp():
    """dw std = +100 overflows float32 (the reference says +-inf without the clip, exactly 0 / img_w with it); at -100 the float32
    exponential is subnormal (the TINY term of the bound) and the box collapses to its centre."""
    an, d = pr.decode_inputs(None, B=1, A=4)
    d[0, :, 2] = [500.0, -500.0, 500.0, -500.0]                                # times the default std 0.2: +-100
    t = d[0, :, 2].astype(f64) * float(f32(pr.DEFAULT_MEAN_STD[6]))
    assert np.abs(np.abs(t) - 100.0).max() < 1e-5 and 0.0 < np.exp(-100.0) < pr.TINY < pr.F32_MAX < np.exp(100.0)
    for clip in (True, False):
        ref, un, bd = pr.decode_ref(an, d, None, pr.IMG_W, pr.IMG_H, clip)
        assert np.isinf(un[0, 0, 0]) and un[0, 0, 0] < 0 and np.isinf(un[0, 0, 2]) and un[0, 0, 2] > 0
        assert (ref[0, 0, 0], ref[0, 0, 2]) == ((0.0, pr.IMG_W) if clip else (-np.inf, np.inf))
        got = model_decode(an, d, None, pr.IMG_W, pr.IMG_H, clip)
        assert np.array_equal(got[0, [0, 2]][:, [0, 2]].astype(f64), ref[0, [0, 2]][:, [0, 2]])
        rows = [1, 3]
        pr.check_bound("decode model exp(-100) clip=%s" % clip, got[:, rows], ref[:, rows], bd[:, rows], "cpu float32 vs float64", "bak")
        assert np.array_equal(un[0, rows, 0], un[0, rows, 2])                 # float64: the box is its centre


def test_bn_eval_model_within_bound_and_fault_rejected():
    for C in (1, 63, 64, 257, 2048):
        gamma, beta, rm, rv = pr.bn_inputs(C)
        eps = torch.tensor(1e-5, dtype=torch.float32)
        istd = 1.0 / torch.sqrt(rv + eps)
        scale = gamma * istd
        got = dict(mean=rm.clone(), invstd=istd, scale=scale, shift=beta - rm * scale)
        pr.check_bn_eval("bn eval model C=%d" % C, got, gamma, beta, rm, rv, route="cpu float32 vs float64")
        if C >= 63:
            assert bool((rv < 1e-5).any()) and bool((rm.abs() > 100).any()) and gamma[0] == 0 and gamma[1] < 0
            bad = dict(got, invstd=1.0 / (torch.sqrt(rv) + eps))              # eps outside the root
            with pytest.raises(AssertionError):
                pr.check_bn_eval("bn eval fault C=%d" % C, bad, gamma, beta, rm, rv, route="modelled fault")
            bad = dict(got, shift=beta - rm * gamma)                         # shift from gamma instead of scale
            with pytest.raises(AssertionError):
                pr.check_bn_eval("bn eval fault C=%d" % C, bad, gamma, beta, rm, rv, route="modelled fault")
