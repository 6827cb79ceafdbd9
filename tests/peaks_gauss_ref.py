"""Independent numpy restatement of the smoothed peak refinement (test-side only): ``NMS(..., bool_gaussian_filt=True)`` of
network/joint_utils.py:109-128 = cv2.resize(INTER_CUBIC) of the clipped 5x5 patch (oracle/joint_oracle.py: cv_resize_cubic),
``scipy.ndimage.gaussian_filter(map_upsamp, sigma=3)``, first row-major maximum of the SMOOTHED patch, score = smoothed value.

``gaussian_filter`` on a float32 array, as scipy computes it (mode 'reflect', truncate 4.0, order 0):
  * weights: exp(-x^2 / (2 sigma^2)) for x = -r .. r with r = int(4 sigma + 0.5), normalised by their sum (float64);
  * axis 0 first, then axis 1; each pass line by line on the values widened to float64;
  * a line of n values is extended by r at both ends with PERIODIC reflection: i -> m = i mod 2n, m >= n -> 2n - 1 - m
    (n <= r wraps more than once);
  * output l:  t = x[l] w[r];  for k = r .. 1:  t += (x[l-k] + x[l+k]) w[r-k]   in this order, float64, no fused multiply-add;
  * one rounding to float32 at the end of each pass.
tests/test_peaks_gauss_cpu.py holds this file to the live scipy function bit for bit and to the recorded reference run
(tests/golden/g20_peaks_gauss.npz).  Every switch below models ONE misreading of the definition; the default is the definition.
"""
import numpy as np

from oracle import joint_oracle as jo

SIGMA = 3.0


def gaussian_weights(sigma=SIGMA, truncate=4.0, radius=None):
    r = int(truncate * float(sigma) + 0.5) if radius is None else radius
    x = np.arange(-r, r + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    return phi / phi.sum()


def extension_index(n, r, reflect="periodic"):
    """Source index of line positions -r .. n + r - 1."""
    i = np.arange(-r, n + r)
    if reflect == "periodic":                       # scipy 'reflect': d c b a | a b c d | d c b a | a b ...
        m = np.mod(i, 2 * n)
        return np.where(m >= n, 2 * n - 1 - m, m)
    if reflect == "single":                         # fault: reflected once, then clamped
        m = np.where(i < 0, -1 - i, np.where(i >= n, 2 * n - 1 - i, i))
        return np.clip(m, 0, n - 1)
    if reflect == "mirror":                         # fault: scipy 'mirror' (the edge cell is not repeated), periodic
        if n == 1:
            return np.zeros_like(i)
        m = np.mod(i, 2 * n - 2)
        return np.where(m >= n, 2 * n - 2 - m, m)
    raise ValueError(reflect)


def correlate_axis(a32, w, axis, acc=np.float64, reflect="periodic", k_descending=True, out=np.float32):
    w = np.asarray(w)
    r = len(w) // 2
    x = np.moveaxis(np.asarray(a32), axis, -1).astype(acc)
    n = x.shape[-1]
    ext = x[..., extension_index(n, r, reflect)]
    wa = w.astype(acc)
    t = ext[..., r:r + n] * wa[r]
    for k in (range(r, 0, -1) if k_descending else range(1, r + 1)):
        t = t + (ext[..., r - k:r - k + n] + ext[..., r + k:r + k + n]) * wa[r - k]
    return np.moveaxis(t.astype(out), -1, axis)


def gaussian_filter_f32(a32, w=None, axes=(0, 1), acc=np.float64, reflect="periodic", k_descending=True, round_between=True):
    """scipy.ndimage.gaussian_filter(a32, sigma=3) for a 2-D float32 array (defaults), or one modelled misreading of it."""
    w = gaussian_weights() if w is None else w
    a = np.asarray(a32, dtype=np.float32)
    for n, axis in enumerate(axes):
        last = n == len(axes) - 1
        a = correlate_axis(a, w, axis, acc, reflect, k_descending, np.float32 if (round_between or last) else acc)
    return a


def upsampled_patches(thre1, heatmaps, upsamp):
    """Per joint type, per peak in row-major order: (px, py, x0, y0, up-sampled clipped 5x5 patch) — everything before the filter."""
    heatmaps = np.asarray(heatmaps)
    out = []
    for joint in range(heatmaps.shape[2]):
        m = heatmaps[:, :, joint]
        per = []
        for px, py in jo.find_peaks(thre1, m):
            x0, y0 = max(0, px - 2), max(0, py - 2)
            x1, y1 = min(m.shape[1] - 1, px + 2), min(m.shape[0] - 1, py + 2)
            per.append((int(px), int(py), int(x0), int(y0), jo.cv_resize_cubic(m[y0:y1 + 1, x0:x1 + 1], upsamp)))
        out.append(per)
    return out


def nms_from_patches(patches, upsamp, smooth=gaussian_filter_f32, score_from="smoothed", tie="first"):
    """The filter, the arg-max and the coordinates.  score_from / tie: modelled faults."""
    out, cnt = [], 0
    for per in patches:
        peaks = np.zeros((len(per), 4))
        for i, (px, py, x0, y0, up) in enumerate(per):
            sm = smooth(up)
            flat = sm.reshape(-1)
            best = int(np.argmax(flat)) if tie == "first" else int(len(flat) - 1 - np.argmax(flat[::-1]))
            by, bx = divmod(best, sm.shape[1])
            cy, cx = (py - y0 + 0.5) * upsamp - 0.5, (px - x0 + 0.5) * upsamp - 0.5
            x = int(round(((px + 0.5) * upsamp - 0.5) + (bx - cx)))
            y = int(round(((py + 0.5) * upsamp - 0.5) + (by - cy)))
            score = sm[by, bx] if score_from == "smoothed" else up[by, bx]
            peaks[i] = (x, y, score, cnt)
            cnt += 1
        out.append(peaks)
    return out


def nms_peaks_smooth(thre1, heatmaps, upsamp=1.0, **kw):
    """joint_utils.py:61-138 with bool_refine_center=True, bool_gaussian_filt=True.  heatmaps: float32 [H, W, J].
    Returns a list of J arrays [n, 4] = (x, y, score, id)."""
    return nms_from_patches(upsampled_patches(thre1, heatmaps, upsamp), upsamp, **kw)


def rows(per_type):
    """A list of J [n, 4] arrays as one [N, 5] array (x, y, score, id, joint type)."""
    return np.concatenate([np.concatenate([p.reshape(-1, 4), np.full((len(p), 1), float(j))], 1) for j, p in enumerate(per_type)])
