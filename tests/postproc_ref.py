"""Float64 references and derived per-element bounds of the inference post-processing arithmetic: `resize_kernel` and the refinement
half of `peaks_refine_kernel` (csrc/peaks.hip), `box_decode_clip_kernel` / `clip_boxes_kernel` (csrc/nms.hip) and
`bn_finalize_eval_kernel` (csrc/bn.hip).  Shared by tests/test_postproc_parity_gpu.py (which compares the kernels with them) and
tests/test_postproc_parity_cpu.py (which holds oracle/joint_oracle.py to the same references and shows that the bounds reject
modelled faults).  Test-side only; torch and numpy on the CPU.  Nothing here imports oracle.joint_oracle.

Resize reference.  torch's CPU `upsample_bicubic2d` / `upsample_bilinear2d` in float64 (A = -0.75, half-pixel coordinates, cubic taps
clamped to the image; the bilinear form clamps the second tap where OpenCV clamps the coordinate — the same value in exact arithmetic),
called with the destination size and, for the fx / fy call form, the forced scale.  It is an implementation of the published rule that
shares no code with the kernel or the oracle.

Resize bound.  u = 2^-24; nothing is fitted to a kernel.  Per axis and destination index d, with s = (d + 0.5) scale - 0.5:
  * coordinate: the kernel forms s in double and rounds it to float32 (at most half a float32 spacing at |s|), then t = fx - floor(fx)
    in float32, which rounds once more (u / 2) only when fx is in (-1, 0): dt = spacing_f32(|s|) / 2 [+ u / 2].  The interpolant is
    continuous in s across integers (c(1) of one footprint is c(0) of the next), so the value moves by at most dt * |sum_k p_k dc_k/dt|
    over the union of the footprints of s - dt and s + dt.  sum_k |dc_k/dt| <= DC_CUBIC = 3 on [0, 1] (c0' = A (3t - 1)(t - 1), c1' =
    3.75 t^2 - 4.5 t, c2'(t) = -c1'(1 - t), c3'(t) = -c0'(1 - t); the sum is 1.5 at t = 0 and t = 1 and peaks at 3.0 at t = 1/2 —
    asserted on a dense grid by the CPU test), which gives dt DC M with M = max |tap|.  The weights sum to one identically, so sum_k
    dc_k/dt = 0 and the same term is also at most dt DC R with R = max tap - min tap (a constant image does not feel its coordinate):
    the bound takes min(M, R).  Linear: the weights are 1 - t and t, the value moves by dt |p1 - p0| <= dt R.
  * coefficient polynomials: each float32 operation of cubic_coeffs (c0 by Horner in y = t + 1 with the constants -3.75, -6, -3
    folded; c1 in t; c2 in z = 1 - t) is charged half a float32 spacing of its result, and the errors of its operands are carried
    through it (|a| eb + |b| ea + ea eb for a product, ea + eb for a sum): `coeff_model` evaluates the polynomials in float64 with
    that running error, per destination index.  The single rounding of y (of z) reaches c0 (c2) through its derivative, |c0'| (|c2'|)
    times half a spacing of y (z).  Ep(t) = err(c0) + err(c1) + err(c2) is 19 u on average and at most 29 u: the Horner form of c0
    cancels from intermediates near 3 to a result below 0.12.  The fourth coefficient is the complement c3 = 1 - c0 - c1 - c2, so its
    error is minus the sum of the other three plus rho, the roundings of the three subtractions (<= 2 u): sum_k p_k dc_k = sum_{k<3}
    (p_k - p_3) dc_k + p_3 rho, at most R Ep + M rho.  Linear: the weight 1 - t rounds once, rho = u / 2, Ep = 0.
  * sums: a pass is p0 c0 + p1 c1 + p2 c2 + p3 c3 left to right in float32: every term passes one product and at most three additions,
    4 u sum_k |p_k c_k| <= 4 u L max |p| with L(t) = sum_k |c_k(t)| (<= 1.375, at t = 1/2).  Linear: two terms, 2 u each.
  Cubic, horizontal pass then vertical pass (a row value is at most Lx M, two row values differ by at most Lx R, and the error of a
  row value is carried through the vertical weights, Ly):
      bound = SQ * (R (Ly Epx + Lx Epy) + min(R, M) DC (Ly dtx + Lx dty) + M (Ly (rhox + 4 u Lx) + Lx (rhoy + 4 u Ly)))
  with M and R over the 4x4 (union) footprint.  Linear:
      bound = SQ * (4 u mag + 2 u Mtap + R (dtx + dty)),   mag = the same bilinear call on |img|, Mtap and R over the 2x2 footprint
  (2 u mag per pass for product + addition, u Mtap per pass covers the rounding of 1 - t).  SQ = 1 + 2^-10 covers the second-order
  terms and the float64 noise of the two coordinate computations.

Peak refinement.  `refine_ref` up-samples a patch with the same torch call at dsize = rint(size * f) and scale 1 / f.  The patch bound
is the cubic bound above with its three factors maximised over the up-sampled patch (`patch_factors`), R the range and M the largest
magnitude of the whole patch: about 60 u R + 33 u min(R, M) + 19 u M for a 5x5 patch.  A peak is
DECIDED when the gap between the two largest float64 values exceeds twice that bound: a float32 evaluation within the bound then has
the same argmax.  Rules (`check_peak_rows`): decided peaks match the float64 first argmax in x, y and id exactly; every score is within
the bound of the float64 value at the cell the device chose; the chosen cell of an undecided peak holds a float64 value within twice
the bound of the maximum.  `tie_map` is a map on which every operation of the refinement at f = 4 is exact in float32 (see there): the
device must equal the float64 reference bit for bit on it, first maximum included.

Box decode.  network/utils.py:19-43 and :55-59 in float64 on the float32 operands.  Per coordinate, with w the anchor extent, m_d =
|d std| + |mean| the magnitude of a standardised delta, Mc = |a1| + |w| / 2 (the centre cancels for an anchor around the origin), Md =
m_dx |w|, Mp = |pw| / 2:  w rounds once; cx = a1 + w / 2: 2 u Mc;  dx = d std + mean: 2 u m_dx, times w with w's own rounding and the
product's: 4 u Md;  pcx adds u (Mc + Md);  expf(dw) carries R_EXP u of its own and the argument's error 2 u m_dw, pw = expf(dw) w two
more roundings;  the final sum u (Mc + Md + Mp).  Together  SQ u (4 Mc + 6 Md + (3 + R_EXP + 2 m_dw) Mp) + TINY (1 + |w|)  (TINY =
2^-126: a width below the smallest normal float may be flushed).  expf: no accuracy table for the HIP math functions ships with the
ROCm installation (no document under its tree states a ulp figure), so it was measured once on an MI355X, by a stand-alone
program that only calls expf (tools/microbench/expf_sweep.hip, built with -O3 -ffp-contract=off like csrc/nms.hip): 2^27 equally spaced points on [-10, 10] against float64
exp gave a worst error of EXPF_ULP_MEASURED = 0.8576 ulp (at x = 3.72555065; mean 0.257 ulp; no point above 1 ulp).  The allowance is
twice that, EXPF_ULP_ALLOWED = 1.7152 ulp; 1 ulp <= 2 u relative, so R_EXP = 2 * 1.7152.  Nothing is taken from the decode kernel's output.
Clipping is exact: where the float64 coordinate lies beyond the limit by more than the bound the result equals 0, img_w or img_h bit for
bit, and no clipped coordinate ever lies outside [0, limit].

Eval BN finalize.  scale = gamma / sqrt(rv + eps), shift = beta - rm scale, with eps the float32 the kernel receives.  invstd: the sum,
the (correctly rounded) square root and the division, 3 roundings; scale one more (4); shift carries scale's 4 on |rm scale| plus the
product and the difference on |beta| + |rm scale| (the two cancel): 6 roundings on that magnitude.  mean is running_mean, exactly."""
import numpy as np
import torch

from helpers import U24, check_elementwise, report
from stream_ref import exact, roundings

f32, f64 = np.float32, np.float64
U = U24
SQ = 1.0 + 2.0 ** -10
TINY = 2.0 ** -126
A_CUBIC = -0.75
DC_CUBIC = 3.0
L_CUBIC_MAX = 1.375
EXPF_ULP_MEASURED = 0.8576              # worst of 2^27 points on [-10, 10], MI355X, ROCm 7.0 (see the docstring)
EXPF_ULP_ALLOWED = 2 * EXPF_ULP_MEASURED
R_EXP = 2 * EXPF_ULP_ALLOWED            # in units of u
EPS32 = float(f32(1e-5))
F32_MAX = float(np.finfo(f32).max)


def spacing32(v):
    """Spacing of float32 at |v| (float64 array), never below the smallest subnormal."""
    return np.spacing(np.abs(np.asarray(v, dtype=f64)).astype(f32)).astype(f64)


# ------------------------------------------------------------------------------------------------ coefficient model
def _rn(v, e):
    return v, e + 0.5 * spacing32(np.abs(v) + e)


def _add(a, b):
    return _rn(a[0] + b[0], a[1] + b[1])


def _mul(a, b):
    return _rn(a[0] * b[0], np.abs(a[0]) * b[1] + np.abs(b[0]) * a[1] + a[1] * b[1])


def _k(c, like):
    return np.full_like(like, c), np.zeros_like(like)


def _neg(a):
    return -a[0], a[1]


def coeff_model(t, A=A_CUBIC):
    """cubic_coeffs (csrc/common.h) in float64 with the running float32 rounding error of every operation.
    t: float64 array in [0, 1].  Returns (c [4, n], err [3, n] of c0, c1, c2, rho [n]: the roundings of forming c3 = 1 - c0 - c1 - c2)."""
    t = np.asarray(t, dtype=f64)
    zero = np.zeros_like(t)
    x = (t, zero)
    y = (t + 1.0, zero)                                         # taken as exact here: its one rounding enters through |c0'| below
    z = (1.0 - t, zero)                                         # likewise through |c2'|
    c0 = _add(_mul(_add(_mul(_add(_mul(_k(A, t), y), _k(-5.0 * A, t)), y), _k(8.0 * A, t)), y), _k(-4.0 * A, t))

    def mid(v):
        return _add(_mul(_mul(_add(_mul(_k(A + 2.0, t), v), _k(-(A + 3.0), t)), v), v), _k(1.0, t))

    c1, c2 = mid(x), mid(z)
    d = np.abs(coeff_derivs(t, A))
    c0 = (c0[0], c0[1] + d[0] * 0.5 * spacing32(y[0]))
    c2 = (c2[0], c2[1] + d[2] * 0.5 * spacing32(z[0]))
    c3 = _add(_add(_add(_k(1.0, t), _neg(c0)), _neg(c1)), _neg(c2))
    err = np.stack([c0[1], c1[1], c2[1]])
    return np.stack([c0[0], c1[0], c2[0], c3[0]]), err, c3[1] - err.sum(0)


def coeff_derivs(t, A=A_CUBIC):
    """d c_k / d t in closed form, [4, n]."""
    t = np.asarray(t, dtype=f64)
    d0 = A * (3 * t - 1) * (t - 1)
    d1 = 3 * (A + 2) * t * t - 2 * (A + 3) * t
    r = 1 - t
    return np.stack([d0, d1, -(3 * (A + 2) * r * r - 2 * (A + 3) * r), -(A * (3 * r - 1) * (r - 1))])


def axis_table(n_dst, n_src, scale, cubic):
    """Per destination index: s, dt, Ep (error sum of the directly computed coefficients), rho (roundings of the complementary one), L
    (sum |c|) and the clamped indices of the union footprint [n_dst, K]."""
    d = np.arange(n_dst, dtype=f64)
    s = (d + 0.5) * float(scale) - 0.5
    ds = 0.5 * spacing32(s)
    dt = ds + np.where(s < 0, 0.5 * U, 0.0)
    t = s - np.floor(s)
    if cubic:
        c, e, rho = coeff_model(t)
        Ep, L = e.sum(0), np.abs(c).sum(0)
        before, after = 1, 2
    else:
        Ep, rho, L = np.zeros(n_dst), np.full(n_dst, 0.5 * U), np.ones(n_dst)
        before, after = 0, 1
    lo = np.floor(s - ds).astype(np.int64) - before
    hi = np.floor(s + ds).astype(np.int64) + after
    K = before + after + 2
    idx = np.minimum(lo[:, None] + np.arange(K)[None, :], hi[:, None]).clip(0, n_src - 1)
    return dict(s=s, dt=dt, Ep=Ep, rho=rho, L=L, idx=idx)


def _scales(src_hw, out_hw, inv_scale):
    (Hs, Ws), (Hd, Wd) = src_hw, out_hw
    if inv_scale is None:
        return float(Hs) / float(Hd), float(Ws) / float(Wd)
    return float(inv_scale[0]), float(inv_scale[1])


def _torch_resize(x_hwc64, out_hw, cubic, inv_scale):
    x = torch.from_numpy(np.ascontiguousarray(x_hwc64)).permute(2, 0, 1)[None].contiguous()
    sh, sw = (None, None) if inv_scale is None else (1.0 / float(inv_scale[0]), 1.0 / float(inv_scale[1]))
    fn = torch._C._nn.upsample_bicubic2d if cubic else torch._C._nn.upsample_bilinear2d
    return fn(x, [int(out_hw[0]), int(out_hw[1])], False, sh, sw)[0].permute(1, 2, 0).contiguous().numpy()


def footprint_max(img_abs, ty, tx):
    """max |tap| over the union footprint of every destination element: [Hd, Wd, C]."""
    mx = img_abs[:, tx["idx"], :].max(2)                        # [Hs, Wd, C]
    return mx[ty["idx"]].max(1)                                 # [Hd, Wd, C]


def resize_ref(img_hwc, out_hw, cubic, inv_scale=None):
    """float64 torch resize of a float32 [H, W, C] array on exactly its values, and the magnitude array of the bound: the same call on
    |img| (linear) or max |tap| over the 4x4 footprint (cubic: the weights are signed)."""
    img = np.asarray(img_hwc, dtype=f32).astype(f64)
    Hd, Wd = int(out_hw[0]), int(out_hw[1])
    ref = _torch_resize(img, (Hd, Wd), cubic, inv_scale)
    if cubic:
        sy, sx = _scales(img.shape[:2], (Hd, Wd), inv_scale)
        mag = footprint_max(np.abs(img), axis_table(Hd, img.shape[0], sy, True), axis_table(Wd, img.shape[1], sx, True))
    else:
        mag = _torch_resize(np.abs(img), (Hd, Wd), cubic, inv_scale)
    return ref, mag


def resize_bound(img_hwc, out_hw, cubic, inv_scale, mag):
    """The per-element bound of the docstring, [Hd, Wd, C]."""
    img = np.asarray(img_hwc, dtype=f32).astype(f64)
    Hd, Wd = int(out_hw[0]), int(out_hw[1])
    sy, sx = _scales(img.shape[:2], (Hd, Wd), inv_scale)
    ty, tx = axis_table(Hd, img.shape[0], sy, cubic), axis_table(Wd, img.shape[1], sx, cubic)
    rng = footprint_max(img, ty, tx) + footprint_max(-img, ty, tx)          # max tap - min tap
    if cubic:
        f_coef, f_coord, f_mag = (f[:, :, None] for f in _cubic_factors(ty, tx))
        return SQ * (rng * f_coef + np.minimum(rng, mag) * f_coord + mag * f_mag)
    mtap = footprint_max(np.abs(img), ty, tx)
    return SQ * (4 * U * mag + 2 * U * mtap + rng * (ty["dt"][:, None] + tx["dt"][None, :])[:, :, None])


def _cubic_factors(ty, tx):
    """(factor of the footprint range from the coefficient roundings, factor of min(range, max |tap|) from the coordinate, factor of
    max |tap| from the complement's roundings and the sums), each [Hd, Wd]."""
    Ly, Lx = ty["L"][:, None], tx["L"][None, :]
    return (Ly * tx["Ep"][None, :] + Lx * ty["Ep"][:, None],
            DC_CUBIC * (Ly * tx["dt"][None, :] + Lx * ty["dt"][:, None]),
            Ly * (tx["rho"] + 4 * U * tx["L"])[None, :] + Lx * (ty["rho"] + 4 * U * ty["L"])[:, None])


def check_resize(name, got_hwc, img_hwc, out_hw, cubic, inv_scale=None, route="", raise_on_fail=True):
    """Every element of a float32 resize result against resize_ref.  Returns the worst err / bound (inf where NaN)."""
    ref, mag = resize_ref(img_hwc, out_hw, cubic, inv_scale)
    bound = resize_bound(img_hwc, out_hw, cubic, inv_scale, mag)
    return check_bound(name, np.asarray(got_hwc), ref, bound, route, "yxc", raise_on_fail)


def check_bound(name, got, ref, bound, route="", names="i", raise_on_fail=True):
    """|got - ref| <= bound element-wise (NaN fails); one report line with the worst err / bound and where."""
    got = np.asarray(got, dtype=f64)
    assert got.shape == ref.shape == bound.shape, (name, got.shape, ref.shape, bound.shape)
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    ratio = np.where(np.isnan(ratio), np.inf, ratio)
    wf = int(np.argmax(ratio)) if ratio.size else 0
    worst = float(ratio.reshape(-1)[wf]) if ratio.size else 0.0
    loc = np.unravel_index(wf, ratio.shape) if ratio.size else ()
    where = "(%s)" % ", ".join("%s=%d" % (k, i) for k, i in zip(names, loc))
    ok = worst <= 1.0
    if raise_on_fail:
        report("%-58s %-52s worst err/bound=%.3f at %s  %s" % (name, route, worst, where, "OK" if ok else "FAIL"))
        assert ok, "%s: element %s got %r, float64 reference %r, |err| %.3e > bound %.3e" % (
            name, where, float(got[loc]), float(ref[loc]), float(err[loc]), float(bound[loc]))
    return worst


# ------------------------------------------------------------------------------------------------ peak refinement
def dsize(n, f):
    return int(np.rint(n * float(f)))


def refine_ref(patch, f):
    """(float64 up-sampled patch at dsize = rint(size * f) with scale 1 / f, its row-major first argmax (by, bx), the gap between its
    two largest values)."""
    p = np.asarray(patch, dtype=f32).astype(f64)
    sh, sw = p.shape
    up = _torch_resize(p[:, :, None], (dsize(sh, f), dsize(sw, f)), True, (1.0 / float(f), 1.0 / float(f)))[:, :, 0]
    flat = up.reshape(-1)
    am = int(np.argmax(flat))                                   # numpy: the first occurrence
    top = np.partition(flat, -2)[-2:] if flat.size > 1 else np.array([-np.inf, flat[0]])
    return up, (am // up.shape[1], am % up.shape[1]), float(top[1] - top[0])


_PF = {}


def patch_factors(sh, sw, f):
    """The three cubic factors, each maximised over the up-sampled patch (they depend on the patch shape and the factor only)."""
    key = (sh, sw, float(f))
    if key not in _PF:
        ty = axis_table(dsize(sh, f), sh, 1.0 / float(f), True)
        tx = axis_table(dsize(sw, f), sw, 1.0 / float(f), True)
        _PF[key] = tuple(float(a.max()) for a in _cubic_factors(ty, tx))
    return _PF[key]


def patch_bound(patch, f):
    """One bound for every cell of the up-sampled patch: the cubic bound with the range and max |.| of the whole patch."""
    p = np.asarray(patch, dtype=f64)
    f_coef, f_coord, f_mag = patch_factors(p.shape[0], p.shape[1], f)
    rng, mag = float(p.max() - p.min()), float(np.abs(p).max())
    return SQ * (rng * f_coef + min(rng, mag) * f_coord + mag * f_mag)


def find_peaks_ref(plane, thre1):
    """Cells above thre1 that no 4-neighbour exceeds (joint_utils.py:19-31), as [(x, y), ...] in row-major order."""
    m = np.asarray(plane)
    p = np.pad(m, 1, mode="constant", constant_values=-np.inf)
    nb = np.maximum(np.maximum(p[:-2, 1:-1], p[2:, 1:-1]), np.maximum(p[1:-1, :-2], p[1:-1, 2:]))
    ys, xs = np.nonzero((m >= nb) & (m > thre1))
    return list(zip(xs.tolist(), ys.tolist()))


def peaks_expect(heat_jhw, thre1, f):
    """The float64 expectation of every peak of one image (joint types in order, peaks row-major, running id): a list per joint type of
    dicts px, py, id, x_min, y_min, up (float64 patch), am, gap, bound, decided, dw, dh."""
    heat = np.asarray(heat_jhw, dtype=f32)
    J, H, W = heat.shape
    out, cnt = [], 0
    for j in range(J):
        rows = []
        for (px, py) in find_peaks_ref(heat[j], thre1):
            x0, y0 = max(0, px - 2), max(0, py - 2)
            x1, y1 = min(W - 1, px + 2), min(H - 1, py + 2)
            patch = heat[j, y0:y1 + 1, x0:x1 + 1]
            up, am, gap = refine_ref(patch, f)
            b = patch_bound(patch, f)
            rows.append(dict(px=px, py=py, id=cnt, x_min=x0, y_min=y0, up=up, am=am, gap=gap, bound=b, decided=gap > 2 * b,
                             dh=up.shape[0], dw=up.shape[1]))
            cnt += 1
        out.append(rows)
    return out


def undecided_share(expect):
    n = sum(len(r) for r in expect)
    return (sum(1 for r in expect for p in r if not p["decided"]) / float(n)) if n else 0.0, n


def colliding_peaks(expect, f):
    """Peaks (over the images of a peak_case) with two up-sampled cells on one final coordinate, on either axis."""
    n = 0
    for e in expect:
        for r in e:
            for p in r:
                xs = [final_coord(p["px"], p["x_min"], b, f) for b in range(p["dw"])]
                ys = [final_coord(p["py"], p["y_min"], b, f) for b in range(p["dh"])]
                n += int(len(set(xs)) < len(xs) or len(set(ys)) < len(ys))
    return n


def final_coord(p, c_min, b, f):
    """The reference's (and the kernel's) float64 expression of a final coordinate from the chosen up-sampled cell b."""
    centre = ((p - c_min) + 0.5) * f - 0.5
    return float(np.rint(((p + 0.5) * f - 0.5) + (b - centre)))


def check_peak_rows(name, got, expect, f, route="", exact_scores=False, raise_on_fail=True):
    """got: list per joint type of [n, 4] (x, y, score, id) arrays; expect: peaks_expect(...).  Applies the rules of the docstring;
    exact_scores (tie_map): x, y, id and the score equal the float64 reference bit for bit.  Returns (worst score err / bound, peaks,
    undecided) or, with raise_on_fail False, the first violation as a string (None when there is none)."""
    f = float(f)
    worst, n, und, where = 0.0, 0, 0, ""
    fail = None

    def bad(msg):
        nonlocal fail
        if fail is None:
            fail = "%s: %s" % (name, msg)

    if [len(g) for g in got] != [len(e) for e in expect]:
        bad("peak counts %s differ from the reference's %s" % ([len(g) for g in got], [len(e) for e in expect]))
    else:
        for j, (gj, ej) in enumerate(zip(got, expect)):
            for i, e in enumerate(ej):
                x, y, score, pid = (float(v) for v in gj[i])
                n += 1
                tag = "joint %d peak %d at (%d, %d)" % (j, i, e["px"], e["py"])
                if pid != e["id"]:
                    bad("%s: id %r, expected %d" % (tag, pid, e["id"]))
                up, (by, bx) = e["up"], e["am"]
                ex, ey = final_coord(e["px"], e["x_min"], bx, f), final_coord(e["py"], e["y_min"], by, f)
                if exact_scores:
                    if (x, y) != (ex, ey) or score != float(up[by, bx]):
                        bad("%s: (%r, %r, %r) is not the exact (%r, %r, %r)" % (tag, x, y, score, ex, ey, float(up[by, bx])))
                    continue
                if e["decided"] and (x, y) != (ex, ey):
                    bad("%s: decided (gap %.3e > 2 * %.3e) but (%r, %r) != float64 argmax's (%r, %r)" % (tag, e["gap"], e["bound"], x, y, ex, ey))
                und += 0 if e["decided"] else 1
                # the cells whose final coordinates are the device's.  One cell per axis, except at f = 1.5: the patch origin x_min f is
                # then k + 1/2 for odd x_min and rint (half to even) maps cells b and b + 1 to one coordinate (1.5 -> 2, 2.5 -> 2), which
                # the device's row cannot tell apart (colliding_peaks counts them; the CPU test asserts where they occur)
                cxs = [b for b in range(e["dw"]) if final_coord(e["px"], e["x_min"], b, f) == x]
                cys = [b for b in range(e["dh"]) if final_coord(e["py"], e["y_min"], b, f) == y]
                if not cxs or not cys:
                    bad("%s: (%r, %r) is no cell of the %dx%d up-sampled patch" % (tag, x, y, e["dh"], e["dw"]))
                    continue
                vals = np.array([up[cy, cx] for cy in cys for cx in cxs])
                k = int(np.argmin(np.abs(vals - score)))
                r = abs(score - vals[k]) / e["bound"] if e["bound"] > 0 else (0.0 if score == vals[k] else np.inf)
                if not r <= 1.0:
                    bad("%s: score %r, float64 value at the chosen cell %r, |err| %.3e > bound %.3e" % (tag, score, vals[k], abs(score - vals[k]), e["bound"]))
                if r > worst or not r == r:
                    worst, where = (r if r == r else np.inf), tag
                if not e["decided"] and not (up.max() - vals.max() <= 2 * e["bound"]):
                    bad("%s: undecided, but the chosen cell is %.3e below the maximum (> 2 * %.3e)" % (tag, up.max() - vals.max(), e["bound"]))
    if not raise_on_fail:
        return fail
    report("%-58s %-52s peaks=%d undecided=%d worst score err/bound=%.3f %s  %s" % (name, route, n, und, worst, where, "OK" if fail is None else "FAIL"))
    assert fail is None, fail
    return worst, n, und


def tie_map():
    """[1, 1, 9, 9] map with one mirror-symmetric bump (1 at the centre, 1/2 left, right, above and below).  At f = 4 the fractions t
    are multiples of 1/8, so every coefficient is a dyadic rational with denominator 2^11 and every intermediate of cubic_coeffs has at
    most 14 significant bits; patch values are multiples of 1/2, row values multiples of 2^-12 and results multiples of 2^-23 below 2:
    all exact in float32 (and in float64 along torch's route).  The four cells around the centre (9 and 10 on both axes of the 20x20
    patch) tie exactly; the first in row-major order is (9, 9)."""
    m = np.zeros((1, 1, 9, 9), dtype=f32)
    m[0, 0, 4, 4] = 1.0
    m[0, 0, 4, 3] = m[0, 0, 4, 5] = m[0, 0, 3, 4] = m[0, 0, 5, 4] = 0.5
    return m


def noise_map():
    """(2, 3, 9, 70) uniform noise with a peak in each corner and on each edge of plane (0, 0) (3x3, 3x5 and 5x3 patches) and a 2x2
    plateau in plane (1, 2)."""
    rng = np.random.RandomState(970)
    m = rng.rand(2, 3, 9, 70).astype(f32)
    for (y, x) in [(0, 0), (0, 69), (8, 0), (8, 69), (0, 30), (8, 41), (4, 0), (5, 69)]:
        m[0, 0, y, x] = 1.5
    m[1, 2, 3:5, 20:22] = 1.25
    return m


NOISE_THRE = 0.8


# ------------------------------------------------------------------------------------------------ box decode / clip
DEFAULT_MEAN_STD = (0.0, 0.0, 0.0, 0.0, 0.1, 0.1, 0.2, 0.2)


def decode_ref(anchors, deltas, mean_std, img_w, img_h, clip):
    """anchors [A, 4], deltas [B, A, 4] float32 arrays.  Returns (ref [B, A, 4] float64 after the clip, unclipped float64, bound).
    A width or height whose float32 product overflows is +inf, as the float32 formula gives."""
    an = np.asarray(anchors, dtype=f32).astype(f64).reshape(-1, 4)
    d = np.asarray(deltas, dtype=f32).astype(f64)
    ms = np.array([float(f32(v)) for v in (DEFAULT_MEAN_STD if mean_std is None else mean_std)])
    mean, std = ms[:4], ms[4:]
    un, bd = np.zeros(d.shape), np.zeros(d.shape)
    with np.errstate(over="ignore", invalid="ignore"):
        for ax in (0, 1):
            a1, a2 = an[None, :, ax], an[None, :, ax + 2]
            w = a2 - a1
            c = a1 + 0.5 * w
            dc = d[:, :, ax] * std[ax] + mean[ax]
            ds = d[:, :, ax + 2] * std[ax + 2] + mean[ax + 2]
            m_dc = np.abs(d[:, :, ax] * std[ax]) + abs(mean[ax])
            m_ds = np.abs(d[:, :, ax + 2] * std[ax + 2]) + abs(mean[ax + 2])
            pc = c + dc * w
            pw = np.exp(ds) * w
            pw = np.where(np.abs(pw) > F32_MAX, np.sign(pw) * np.inf, pw)
            Mc, Md, Mp = np.abs(a1) + 0.5 * np.abs(w), m_dc * np.abs(w), 0.5 * np.abs(pw)
            b = SQ * U * (4 * Mc + 6 * Md + (3 + R_EXP + 2 * m_ds) * Mp) + TINY * (1 + np.abs(w))
            un[:, :, ax], un[:, :, ax + 2] = pc - 0.5 * pw, pc + 0.5 * pw
            bd[:, :, ax] = bd[:, :, ax + 2] = b
    ref = un.copy()
    if clip:
        ref[:, :, 0:2] = np.maximum(ref[:, :, 0:2], 0.0)
        ref[:, :, 2] = np.minimum(ref[:, :, 2], float(img_w))
        ref[:, :, 3] = np.minimum(ref[:, :, 3], float(img_h))
    return ref, un, bd


def check_decode(name, got, anchors, deltas, mean_std, img_w, img_h, clip, route="", raise_on_fail=True):
    """Every coordinate within the bound of decode_ref; with clip, exactly 0 / img_w / img_h wherever the float64 coordinate is beyond
    the limit by more than the bound, and never outside [0, limit]."""
    got = np.asarray(got, dtype=f64)
    ref, un, bd = decode_ref(anchors, deltas, mean_std, img_w, img_h, clip)
    worst = check_bound(name, got, ref, bd, route, "bak", raise_on_fail)
    ok = True
    if clip:
        lim = np.array([0.0, 0.0, float(img_w), float(img_h)])
        lo, hi = un[:, :, :2] < -bd[:, :, :2], un[:, :, 2:] > lim[2:] + bd[:, :, 2:]
        ok = bool((got[:, :, :2][lo] == 0.0).all()) and bool((np.broadcast_to(lim[2:], hi.shape)[hi] == got[:, :, 2:][hi]).all()) \
            and bool((got[:, :, :2] >= 0.0).all()) and bool((got[:, :, 2:] <= lim[2:]).all())
        if raise_on_fail:
            report("%-58s %-52s clipped low=%d high=%d exact  %s" % (name, route, int(lo.sum()), int(hi.sum()), "OK" if ok else "FAIL"))
            assert ok, "%s: a clipped coordinate is not exactly 0 / img_w / img_h" % name
            assert int(lo.sum()) > 0 and int(hi.sum()) > 0, "%s: the case clips nothing" % name
    return worst if ok else float("inf")


# ------------------------------------------------------------------------------------------------ eval BN finalize
def bn_eval_ref(gamma, beta, rm, rv, eps=EPS32):
    """float64 (mean, invstd, scale, shift) and the magnitude the shift's roundings are carried on, |beta| + |rm scale|."""
    g, b, m, v = (t.detach().cpu().double() for t in (gamma, beta, rm, rv))
    istd = 1.0 / torch.sqrt(v + float(eps))
    scale = g * istd
    return m, istd, scale, b - m * scale, b.abs() + (m * scale).abs()


def check_bn_eval(tag, got, gamma, beta, rm, rv, eps=EPS32, route=""):
    """got: the device's mean, invstd, scale, shift (an ops.BNState or a dict)."""
    get = (lambda k: got[k]) if isinstance(got, dict) else (lambda k: getattr(got, k))
    mean, istd, scale, shift, smag = bn_eval_ref(gamma, beta, rm, rv, eps)
    F32 = torch.float32
    exact(tag + " mean", get("mean").cpu().double(), mean, route)
    return max(check_elementwise(tag + " invstd", get("invstd"), istd, istd.abs(), F32, route=route, names="c", **roundings(3)),
               check_elementwise(tag + " scale", get("scale"), scale, scale.abs(), F32, route=route, names="c", **roundings(4)),
               check_elementwise(tag + " shift", get("shift"), shift, smag, F32, route=route, names="c", **roundings(6)))


# ------------------------------------------------------------------------------------------------ shared inputs
RESIZE_CASES = [(30, 40, 18, 120, 160), (120, 160, 18, 97, 133), (64, 48, 3, 23, 31), (7, 5, 1, 7, 5), (1, 1, 1, 4, 4), (2, 1, 1, 7, 3),
                (5, 5, 1, 20, 20)]
FX_SHAPE, FX_FACTORS = (37, 53, 3), (0.73, 1.37, 2.0)
PEAK_FACTORS = (4.0, 4.27, 1.5, 13.0)
PEAK_MAPS = ("a", "b", "c", "noise")
GOLD_THRE = 0.1


def resize_input(Hs, Ws, C, seed=0):
    """Mixed-sign float32 image: the magnitude array of the bound matters."""
    rng = np.random.RandomState(1000 * Hs + 10 * Ws + C + seed)
    return (rng.rand(Hs, Ws, C) * 4.0 - 2.0).astype(f32)


def fx_case(f):
    """(image, (Hd, Wd), inv_scale) of the fx / fy call form: the size from rint, the scale exactly 1 / f."""
    img = resize_input(*FX_SHAPE, seed=int(f * 100))
    return img, (int(np.rint(FX_SHAPE[0] * f)), int(np.rint(FX_SHAPE[1] * f))), (1.0 / f, 1.0 / f)


def peak_map(name):
    """(heat [B, J, H, W] float32, thre1)."""
    if name == "noise":
        return noise_map(), NOISE_THRE
    if name == "tie":
        return tie_map(), GOLD_THRE
    from helpers import gold
    return np.ascontiguousarray(gold("g10_peaks.npz")["heat_" + name].transpose(2, 0, 1))[None], GOLD_THRE


_PE = {}


def peak_case(name, f):
    """(heat, thre1, [peaks_expect of image b]) — computed once per (map, factor) and shared, never modified."""
    key = (name, float(f))
    if key not in _PE:
        heat, thre = peak_map(name)
        _PE[key] = (heat, thre, [peaks_expect(heat[b], thre, f) for b in range(heat.shape[0])])
    return _PE[key]


def decode_inputs(mean_std, B=3, A=257, seed=5):
    """Distinct anchors per index (x1, y1 of either sign, extents 4 .. 300) and deltas whose dw std + mean, dh std + mean span [-8, 8]."""
    rng = np.random.RandomState(seed)
    ms = np.array(DEFAULT_MEAN_STD if mean_std is None else mean_std, dtype=f64)
    an = np.zeros((A, 4), dtype=f32)
    an[:, 0], an[:, 1] = rng.uniform(-60, 600, A), rng.uniform(-60, 440, A)
    an[:, 2], an[:, 3] = an[:, 0] + rng.uniform(4, 300, A).astype(f32), an[:, 1] + rng.uniform(4, 300, A).astype(f32)
    d = np.zeros((B, A, 4), dtype=f32)
    d[:, :, :2] = rng.randn(B, A, 2) * 3.0
    for k in (2, 3):
        target = rng.permutation(np.linspace(-8.0, 8.0, B * A)).reshape(B, A)
        d[:, :, k] = (target - ms[k]) / ms[4 + k]
    return an, d


NONDEFAULT_MEAN_STD = (0.05, -0.1, 0.3, -0.2, 0.15, 0.12, 0.25, 0.3)
IMG_W, IMG_H = 640.0, 480.0


def bn_inputs(C, seed=0):
    """gamma (0 and a negative value among them), beta, running_mean up to 1e3 in magnitude, running_var in [1e-8, 10]."""
    g = torch.Generator().manual_seed(100 + C + seed)
    gamma = torch.randn(C, generator=g)
    beta = torch.randn(C, generator=g)
    rm = torch.sign(torch.randn(C, generator=g)) * 10.0 ** (torch.rand(C, generator=g) * 6.0 - 3.0)
    rv = 10.0 ** (torch.rand(C, generator=g) * 9.0 - 8.0)
    if C > 2:
        gamma[0], gamma[1] = 0.0, -gamma[1].abs() - 0.5
        rv[2], rv[C - 1] = 1e-8, 10.0
    return gamma, beta, rm, rv.clamp(1e-8, 10.0)
