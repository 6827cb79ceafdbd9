"""Plain-Python restatement of COCO maskApi.c for the tests of datasets/segm.py and csrc/segm.hip: rleFrPoly, rleMerge as a
union, rleDecode and rleFrString.

SEQUENTIAL, as the library is written: the points of every edge are listed in walking order into one long list, consecutive
points of that list are compared, the crossings become toggles on the column-major flat index.  The kernel instead evaluates each
(edge, step) pair from closed formulas; nothing here is shared with that formulation.  Two forms of "toggles -> mask" are kept:

* :func:`counts_from_toggles` + :func:`decode`: the library's own — append h * w, sort, take differences, merge zero-length runs,
  then paint alternating OFF / ON runs;
* :func:`parity_mask`: cell i is ON iff the number of toggles a <= i is odd.

``(int)`` of C is Python's ``int()`` (truncation toward zero); every float step is one separately rounded float64 operation.

``mis`` names ONE modelled misreading of the rule (tests/test_segm_cpu.py checks that the committed inputs reject each of them):
"round", "scale4", "clamp_h1", "floor", "clamp_col", "row_major", "rising_u", "xor_parts", "no_cancel", "first_on".
"""
import math

import numpy as np

SCALE = 5.0


def upsample(xy, mis=None):
    """Step 1: the k vertices of a part ([x0, y0, x1, y1, ...]) on the 5x grid -> ([X], [Y]) with the ring closed (k + 1 long)."""
    scale = 4.0 if mis == "scale4" else SCALE
    k = len(xy) // 2
    if mis == "round":
        X = [int(math.floor(scale * xy[2 * j] + 0.5)) for j in range(k)]
        Y = [int(math.floor(scale * xy[2 * j + 1] + 0.5)) for j in range(k)]
    else:
        X = [int(scale * xy[2 * j] + 0.5) for j in range(k)]
        Y = [int(scale * xy[2 * j + 1] + 0.5) for j in range(k)]
    return X + X[:1], Y + Y[:1]


def boundary_points(X, Y):
    """Step 2: every edge's points in walking order, all edges in one list (so the last point of an edge is followed by the first
    point of the next, as in the library)."""
    u, v = [], []
    for j in range(len(X) - 1):
        xs, xe, ys, ye = X[j], X[j + 1], Y[j], Y[j + 1]
        dx, dy = abs(xe - xs), abs(ys - ye)
        flip = (dx >= dy and xs > xe) or (dx < dy and ys > ye)
        if flip:
            xs, xe, ys, ye = xe, xs, ye, ys
        if dx == 0 and dy == 0:
            u.append(xs)                       # s = 0 / 0: the library's v is undefined here and is never read
            v.append(ys)
            continue
        s = float(ye - ys) / dx if dx >= dy else float(xe - xs) / dy
        if dx >= dy:
            for d in range(dx + 1):
                t = dx - d if flip else d
                u.append(t + xs)
                v.append(int(ys + s * t + 0.5))
        else:
            for d in range(dy + 1):
                t = dy - d if flip else d
                v.append(t + ys)
                u.append(int(xs + s * t + 0.5))
    return u, v


def toggles_of_part(xy, h, w, mis=None):
    """Steps 1-3: the toggles (flat column-major indices, unsorted, h * w possible) of one polygon part."""
    scale = 4.0 if mis == "scale4" else SCALE
    X, Y = upsample(xy, mis)
    u, v = boundary_points(X, Y)
    out = []
    for j in range(1, len(u)):
        if u[j] == u[j - 1]:
            continue
        xd = float(u[j] if (u[j] < u[j - 1] or mis == "rising_u") else u[j] - 1)
        xd = (xd + 0.5) / scale - 0.5
        if mis == "clamp_col":
            if math.floor(xd) != xd:
                continue
            xd = min(max(xd, 0.0), float(w - 1))
        elif math.floor(xd) != xd or xd < 0 or xd > w - 1:
            continue
        yd = float(v[j] if v[j] < v[j - 1] else v[j - 1])
        yd = (yd + 0.5) / scale - 0.5
        top = h - 1 if mis == "clamp_h1" else h
        if yd < 0:
            yd = 0.0
        elif yd > top:
            yd = float(top)
        yd = math.floor(yd) if mis == "floor" else math.ceil(yd)
        out.append(int(xd) * h + int(yd))
    return out


def counts_from_toggles(toggles, h, w):
    """The library's form: append h * w, sort, take differences, merge the zero-length runs -> run lengths OFF, ON, ..."""
    a = sorted(list(toggles) + [h * w])
    p, d = 0, []
    for t in a:
        d.append(t - p)
        p = t
    b = [d[0]]
    j = 1
    while j < len(d):
        if d[j] > 0:
            b.append(d[j])
            j += 1
        else:
            j += 1
            if j < len(d):
                b[-1] += d[j]
                j += 1
    return b


def decode(counts, h, w, mis=None):
    """rleDecode: alternating runs, the first one OFF, painted in column-major order -> uint8 [h, w]."""
    flat = np.zeros(h * w, dtype=np.uint8)
    pos, val = 0, 1 if mis == "first_on" else 0
    for c in counts:
        end = min(pos + int(c), h * w)
        if val and end > pos:
            flat[pos:end] = 1
        pos, val = pos + int(c), 1 - val
    if mis == "row_major":
        return flat.reshape(h, w).copy()
    return flat.reshape(w, h).T.copy()


def parity_mask(toggles, h, w, mis=None):
    """Step 4: cell i ON iff the number of toggles a <= i is odd (a = h * w has no effect)."""
    hits = np.zeros(h * w + 1, dtype=np.int64)
    for a in (set(toggles) if mis == "no_cancel" else toggles):
        hits[min(a, h * w)] += 1
    flat = (np.cumsum(hits[:h * w]) & 1).astype(np.uint8)
    if mis == "row_major":
        return flat.reshape(h, w).copy()
    return flat.reshape(w, h).T.copy()


def part_mask(xy, h, w, form="sort", mis=None):
    t = toggles_of_part(xy, h, w, mis)
    if form == "sort" and mis != "no_cancel":
        return decode(counts_from_toggles(t, h, w), h, w, mis)
    return parity_mask(t, h, w, mis)


def string_counts(s):
    """rleFrString: the compressed ``counts`` (str or bytes) -> list of run lengths."""
    if isinstance(s, str):
        s = s.encode("ascii")
    cnts, p = [], 0
    while p < len(s):
        x, k, more = 0, 0, True
        while more:
            c = s[p] - 48
            x |= (c & 0x1f) << (5 * k)
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if len(cnts) > 2:
            x += cnts[-2]
        cnts.append(x)
    return cnts


def ann_to_mask(segm, h, w, form="sort", mis=None):
    """annToMask of one annotation's ``segmentation``: a list of polygon parts (their union), or an RLE dict with a list or a
    compressed string of counts -> uint8 [h, w]."""
    if isinstance(segm, dict):
        assert list(segm["size"]) == [h, w]
        counts = segm["counts"]
        if isinstance(counts, (str, bytes)):
            counts = string_counts(counts)
        if form == "sort":
            return decode(counts, h, w, mis)
        toggles = [int(a) for a in np.cumsum(np.asarray(counts, dtype=np.int64))]
        return parity_mask(([0] if mis == "first_on" else []) + toggles, h, w, mis)
    out = np.zeros((h, w), dtype=np.uint8)
    for xy in segm:
        m = part_mask(xy, h, w, form, mis)
        out = (out ^ m) if mis == "xor_parts" else (out | m)
    return out
