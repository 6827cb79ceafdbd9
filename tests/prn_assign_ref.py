"""Scene generator, references, comparisons and numpy kernel models for the PRN-assignment parity tests (csrc/prn_assign.hip).

References (nothing here restates what it checks, except where proven equal first by the CPU tier):
  occ / blurred input : oracle.prn_assign_oracle.build_maps per image (``build_maps_hw`` = the same with h, w as parameters, proven
                        equal to the oracle at 56x36 on every scene by test_prn_assign_parity_cpu.py);
  window scores       : np.sum(prn_assign_oracle.crop(plane, (y, x), N)) on float32 planes;
  arg-max             : np.argmax of the flattened plane;
  assignment          : prn_assign_oracle.assign.
Every comparison is an equality.  The ``check_*`` functions are what the GPU tier applies to the kernels' results; the CPU tier
applies the same functions to the numpy models below (accepted) and to their named mutants (rejected)."""
import functools
import math

import numpy as np

from oracle import prn_assign_oracle as O

f32, f64 = np.float32, np.float64
H0, W0 = 56, 36
SENT_F = f32(-777.25)                      # sentinels the tests pre-fill outputs with
SENT_I = np.int32(-777)
NS = (1, 3, 5, 9, 15)

_X = np.arange(-4, 5)
W9 = np.exp(-0.5 / 1.0 * _X ** 2)
W9 = W9 / W9.sum()                          # scipy.ndimage._gaussian_kernel1d(sigma=1, order=0, radius=4)
# A symmetric 9-tap kernel whose far pairs cancel (2e17 - 2e17): with it the ORDER in which the pairs are summed decides whether the
# near taps survive, so it shows in the float32 result — with the gaussian weights the order moves the float64 sum by 2^-52 only,
# which the cast to float32 hides.  The reference for it is scipy.ndimage.correlate1d itself (its symmetric-kernel branch).
CANCEL_W9 = np.array([1e17, -1e17, 3.0, 0.25, 1.0, 0.25, 3.0, -1e17, 1e17])


# ====================================================================================================== scenes
class Scene(object):
    """kps[i]: list of (x, y, 1, 0, joint type) in input order; boxes[i]: list of (x1, y1, x2, y2) — the reference's arguments."""

    def __init__(self, name, kps, boxes, in_thres=0.21, planted=None):
        self.name, self.kps, self.boxes, self.in_thres = name, kps, boxes, in_thres
        self.planted = planted or {}
        self.nimg = len(kps)

    def arrays(self):
        """The flat form of prn_assign_arrays: peaks_xy, joint_off[nimg][18], boxes_xywh, box_start (+ box_img)."""
        peaks, joff, bx, bs = [], [], [], [0]
        for i in range(self.nimg):
            offs = []
            for t in range(17):
                offs.append(len(peaks))
                peaks += [[k[0], k[1]] for k in self.kps[i] if k[-1] == t]
            offs.append(len(peaks))
            joff.append(offs)
            bx += [[b[0], b[1], b[2] - b[0], b[3] - b[1]] for b in self.boxes[i]]          # tester.py:355-357
            bs.append(len(bx))
        box_start = np.asarray(bs, dtype=np.int32)
        return dict(peaks=np.asarray(peaks, dtype=f64).reshape(-1, 2), joint_off=np.asarray(joff, dtype=np.int32),
                    boxes=np.asarray(bx, dtype=f64).reshape(-1, 4), box_start=box_start,
                    box_img=np.repeat(np.arange(self.nimg, dtype=np.int32), np.diff(box_start)).astype(np.int32))


def xywh(b):
    return [b[0], b[1], b[2] - b[0], b[3] - b[1]]


def edges(b, in_thres):
    """The four strict bounds of the inside test in the reference's own expressions (tester.py:369-372), b = (x, y, w, h)."""
    return b[0] - b[2] * in_thres, b[1] - b[3] * in_thres, b[0] + b[2] * (1.0 + in_thres), b[1] + b[3] * (1.0 + in_thres)


def clamp_class(p, b, h, w):
    """(x class, y class) in {-1 low, 0 in range, 1 high} of a peak for box b = (x, y, w, h): which branch of the clamp chain it meets."""
    x0 = int((p[0] - b[0]) * (float(w) / math.ceil(b[2])))
    y0 = int((p[1] - b[1]) * (float(h) / math.ceil(b[3])))
    return (1 if x0 >= w else (-1 if x0 < 0 else 0)), (1 if y0 >= h else (-1 if y0 < 0 else 0))


def is_inside(p, b, in_thres):
    lx, ly, hx, hy = edges(b, in_thres)
    return p[0] > lx and p[1] > ly and p[0] < hx and p[1] < hy


_CLS_RANGE = {-1: (-0.2, -0.06), 0: (0.05, 0.95), 1: (1.03, 1.2)}


def _image(rs, boxes, missing, planted, img):
    """Peaks of one image: per box 3 planted per clamp class, the strict edges and their nextafter neighbours, 60 uniform ones,
    cell collisions and a duplicated position; joint types in `missing` get none."""
    types = [t for t in range(17) if t not in missing]
    kps = []

    def add(x, y, t=None, tag=None, bi=None):
        t = types[rs.randint(len(types))] if t is None else t
        kps.append((float(x), float(y), 1, 0, t))
        if tag is not None:
            planted.setdefault(tag, []).append((img, bi, len(kps) - 1))

    for bi, bb in enumerate(boxes):
        b = xywh(bb)
        for cx in (-1, 0, 1):
            for cy in (-1, 0, 1):
                for _ in range(3):
                    u, v = rs.uniform(*_CLS_RANGE[cx]), rs.uniform(*_CLS_RANGE[cy])
                    add(b[0] + u * b[2], b[1] + v * b[3], tag=("class", cx, cy), bi=bi)
        lx, ly, hx, hy = edges(b, 0.21)
        mx, my = b[0] + 0.4 * b[2], b[1] + 0.6 * b[3]
        for tag, (x, y), (xi, yi) in (("x lo", (lx, my), (np.nextafter(lx, np.inf), my)), ("y lo", (mx, ly), (mx, np.nextafter(ly, np.inf))),
                                      ("x hi", (hx, my), (np.nextafter(hx, -np.inf), my)), ("y hi", (mx, hy), (mx, np.nextafter(hy, -np.inf)))):
            add(x, y, tag=("edge out", tag), bi=bi)
            add(xi, yi, tag=("edge in", tag), bi=bi)
        for _ in range(60):
            u, v = rs.uniform(-0.23, 1.23, 2)
            add(b[0] + u * b[2], b[1] + v * b[3])
        # three peaks of one type within a hundredth of a pixel (one cell of this box: the last one wins), and an exact duplicate
        t = types[bi % len(types)]
        cx, cy = b[0] + 0.31 * b[2], b[1] + 0.47 * b[3]
        for d in (0.0, 0.004, 0.008):
            add(cx + d, cy + d, t=t, tag="collide", bi=bi)
        add(b[0] + 0.7 * b[2], b[1] + 0.2 * b[3], t=t, tag="dup", bi=bi)
        add(b[0] + 0.7 * b[2], b[1] + 0.2 * b[3], t=t, tag="dup", bi=bi)
    return kps


@functools.lru_cache(maxsize=None)
def normal_scene():
    """3 images: 4 boxes / none (between the two) / 3 boxes; image 0's first box has integer geometry (scale exactly 0.5) for the
    products that land on an integer or in (-1, 0); image 2 has no peaks of joint types 4 and 11, image 0 none of type 7."""
    rs = np.random.RandomState(1234)
    planted = {}
    boxes0 = [(100.0, 50.0, 172.0, 162.0), (130.3, 61.7, 251.9, 290.2), (300.25, 20.5, 391.0, 201.75), (20.1, 200.6, 133.7, 467.3)]
    boxes2 = [(50.5, 40.25, 171.3, 301.9), (90.7, 70.1, 230.2, 350.6), (400.0, 100.0, 450.3, 181.4)]
    k0 = _image(rs, boxes0, (7,), planted, 0)
    # box 0 of image 0: w = 72, h = 112 -> x_scale = y_scale = 0.5 exactly
    exact = [(100.0 + 2 * 5, 50.0 + 2 * 7, "integer"), (100.0 + 2 * 35, 50.0 + 2 * 55, "integer"), (100.0 + 72.0, 50.0 + 112.0, "integer"),
             (100.0 - 1.0, 50.0 + 20.0, "(-1,0) x"), (100.0 + 20.0, 50.0 - 1.0, "(-1,0) y"), (100.0 - 1.5, 50.0 - 0.5, "(-1,0) xy")]
    for x, y, tag in exact:
        k0.append((x, y, 1, 0, 9))
        planted.setdefault(tag, []).append((0, 0, len(k0) - 1))
    k1 = [(float(rs.uniform(0, 600)), float(rs.uniform(0, 400)), 1, 0, int(rs.randint(17))) for _ in range(40)]
    k2 = _image(rs, boxes2, (4, 11), planted, 2)
    return Scene("normal", [k0, k1, k2], [boxes0, [], boxes2], planted=planted)


@functools.lru_cache(maxsize=None)
def dense_scene():
    """One type with 2600 peaks in and around one box (most cells of its plane occupied, many overwritten), a second box overlapping it."""
    rs = np.random.RandomState(4321)
    boxes = [(60.0, 30.0, 241.7, 400.3), (100.5, 80.5, 300.0, 420.0)]
    b = xywh(boxes[0])
    kps = [(b[0] + u * b[2], b[1] + v * b[3], 1, 0, 3) for u, v in rs.uniform(-0.2, 1.2, (2600, 2))]
    kps += [(float(rs.uniform(50, 310)), float(rs.uniform(20, 430)), 1, 0, int(t)) for t in rs.randint(0, 17, 60)]
    return Scene("dense", [kps], [boxes])


@functools.lru_cache(maxsize=None)
def index_error_scene():
    """in_thres 1.5: a peak right of box 1 and more than one box height above it passes the inside test, takes the `x0 >= w` branch
    alone and keeps y0 < -h: the reference raises IndexError (tester.py:392).  Boxes 0 and 2 are too far away to see that peak."""
    rs = np.random.RandomState(99)
    boxes = [(0.0, 1000.0, 60.0, 1100.0), (1000.0, 1000.0, 1080.0, 1120.0), (2000.0, 1000.0, 2050.0, 1090.0)]
    kps = []
    for bb in boxes:
        b = xywh(bb)
        kps += [(b[0] + u * b[2], b[1] + v * b[3], 1, 0, int(t)) for (u, v), t in zip(rs.uniform(-0.9, 1.9, (25, 2)), rs.randint(0, 17, 25))]
    b = xywh(boxes[1])
    bad = (b[0] + 1.1 * b[2], b[1] - 1.2 * b[3], 1, 0, 5)
    kps.insert(30, bad)
    return Scene("index error", [kps], [boxes], in_thres=1.5, planted={"bad": [(0, 1, 30)]})


def crowded_scene(seed, nimg=6):
    """Random crowded images as in test_prn_assign.py: up to 12 overlapping boxes, up to 40 peaks per joint type, types nobody has."""
    rs = np.random.RandomState(seed)
    kps, boxes = [], []
    for i in range(nimg):
        bl = []
        for _ in range(rs.randint(0, 13)):
            cx, cy, bw, bh = rs.uniform(100, 540), rs.uniform(100, 380), rs.uniform(40, 200), rs.uniform(80, 300)
            bl.append((cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2))
        kl = []
        for t in range(17):
            n = 0 if (t in (4, 11) and i % 3 == 0) else rs.randint(1, 41)
            kl += [(float(x), float(y), 1, 0, t) for x, y in zip(rs.uniform(0, 640, n), rs.uniform(0, 480, n))]
        kps.append(kl)
        boxes.append(bl)
    return Scene("crowded %d" % seed, kps, boxes)


# ====================================================================================================== references
def build_maps_hw(kps, bbox_list, h, w, in_thres=0.21):
    """prn_assign_oracle.build_maps (tester.py:337-397) with the map size as parameters instead of 56x36."""
    idx = 0
    peaks = []
    for j in range(17):
        tl = []
        for k in kps:
            if k[-1] == j:
                tl.append([k[0], k[1], 1, idx])
                idx += 1
        peaks.append(tl)
    bboxes = [[b[0], b[1], b[2] - b[0], b[3] - b[1]] for b in bbox_list]
    weights_bbox = np.zeros((len(bboxes), h, w, 4, 17))
    for joint_id, peak in enumerate(peaks):
        for instance in peak:
            p_x, p_y = instance[0], instance[1]
            for bbox_id, b in enumerate(bboxes):
                inside = (p_x > b[0] - b[2] * in_thres and p_y > b[1] - b[3] * in_thres and
                          p_x < b[0] + b[2] * (1.0 + in_thres) and p_y < b[1] + b[3] * (1.0 + in_thres))
                if not inside:
                    continue
                x_scale = float(w) / math.ceil(b[2])
                y_scale = float(h) / math.ceil(b[3])
                x0 = int((p_x - b[0]) * x_scale)
                y0 = int((p_y - b[1]) * y_scale)
                if x0 >= w and y0 >= h:
                    x0, y0 = w - 1, h - 1
                elif x0 >= w:
                    x0 = w - 1
                elif y0 >= h:
                    y0 = h - 1
                elif x0 < 0 and y0 < 0:
                    x0, y0 = 0, 0
                elif x0 < 0:
                    x0 = 0
                elif y0 < 0:
                    y0 = 0
                weights_bbox[bbox_id, y0, x0, :, joint_id] = [1, instance[2], instance[3], 1e-9]
    old = np.copy(weights_bbox)
    inp = np.zeros((len(bboxes), h, w, 17))
    for j in range(len(bboxes)):
        for t in range(17):
            inp[j, :, :, t] = O.gaussian(weights_bbox[j, :, :, 0, t])
    return peaks, bboxes, old, inp


def occ_of(old):
    """occ [n,17,h,w] int32 = 1 + peak id where a cell is taken, as test_prn_assign.py forms it."""
    return np.where(old[:, :, :, 0, :] == 1, old[:, :, :, 2, :] + 1, 0).transpose(0, 3, 1, 2).astype(np.int32)


_MAPS = {}


def scene_maps(scene, h=H0, w=W0, skip_boxes=()):
    """Per image the reference's (peaks, bboxes, old, inp) — the oracle itself at 56x36, its restatement elsewhere — and the
    batch-wide occ [nb,17,h,w] / prn_in [nb,h,w,17] float32.  skip_boxes: (image, box) pairs left out of the reference run (their
    rows of occ / prn_in are not filled and must not be compared)."""
    key = (scene.name, h, w, tuple(skip_boxes))
    if key not in _MAPS:
        per, occs, ins, valid = [], [], [], []
        for i in range(scene.nimg):
            use = [bi for bi in range(len(scene.boxes[i])) if (i, bi) not in skip_boxes]
            bl = [scene.boxes[i][bi] for bi in use]
            if (h, w) == (H0, W0):
                r = O.build_maps(scene.kps[i], bl, in_thres=scene.in_thres)
            else:
                r = build_maps_hw(scene.kps[i], bl, h, w, scene.in_thres)
            per.append(r)
            o = np.zeros((len(scene.boxes[i]), 17, h, w), dtype=np.int32)
            p = np.zeros((len(scene.boxes[i]), h, w, 17), dtype=f32)
            if use:
                o[use] = occ_of(r[2])
                p[use] = r[3].astype(f32)
            occs.append(o)
            ins.append(p)
            valid += [(i, bi) not in skip_boxes for bi in range(len(scene.boxes[i]))]
        for a in (occs, ins):
            for x in a:
                x.setflags(write=False)
        _MAPS[key] = dict(per=per, occ=np.concatenate(occs, 0), prn_in=np.concatenate(ins, 0), valid=np.asarray(valid, dtype=bool))
    return _MAPS[key]


def ref_blur(scene, wts, h=H0, w=W0):
    """prn_in [nb,h,w,17] float32 for the kernel weights `wts`: scipy.ndimage.correlate1d along rows then columns with 'nearest' edges
    (what gaussian_filter does with its own weights) on the reference's one-hot planes."""
    from scipy import ndimage as ndi
    occ = scene_maps(scene, h, w)["occ"]
    res = np.zeros((occ.shape[0], h, w, 17), dtype=f32)
    for b in range(occ.shape[0]):
        for t in range(17):
            plane = (occ[b, t] > 0).astype(f64)
            res[b, :, :, t] = ndi.correlate1d(ndi.correlate1d(plane, wts, 0, mode="nearest"), wts, 1, mode="nearest").astype(f32)
    return res


def check_blur(scene, wts, prn_in, h=H0, w=W0):
    want = ref_blur(scene, wts, h, w)
    assert prn_in.dtype == f32 and np.isfinite(want).all()
    assert np.array_equal(prn_in.view(np.uint32), want.view(np.uint32)), "%s: blur with the given weights differs from scipy's correlate1d in %d values" % (
        scene.name, int((prn_in.view(np.uint32) != want.view(np.uint32)).sum()))
    return want.size


def window_shape(y, x, N, h=H0, w=W0):
    return O.crop(np.empty((h, w), dtype=np.int8), (y, x), N).shape


def ref_scores(out, occ, N):
    """{(b, t, y, x): np.sum of the reference's crop} for the occupied cells, in np.argwhere order (a dict keeps insertion order)."""
    res = {}
    for b, t, y, x in np.argwhere(occ > 0):
        res[(int(b), int(t), int(y), int(x))] = np.sum(O.crop(out[b, :, :, t], (y, x), N=N))
    return res


def ref_argmax(out):
    nb, h, w, _ = out.shape
    return np.stack([[np.argmax(out[b, :, :, t].reshape(-1)) for t in range(17)] for b in range(nb)]).astype(np.int32)


def ref_candidates(out, occ, N, cap, limit=None):
    """The compact result as the reference implies it: cand_n [nb,17], cand_id / cand_score [nb,17,cap] with the sentinels in every
    slot at or beyond min(count, cap), overflow word.  Entries follow np.argwhere's order (tester.py:415)."""
    nb = occ.shape[0]
    cn = np.zeros((nb, 17), dtype=np.int32)
    ci = np.full((nb, 17, cap), SENT_I, dtype=np.int32)
    cs = np.full((nb, 17, cap), SENT_F, dtype=f32)
    for b in range(nb):
        for t in range(17):
            cells = np.argwhere(occ[b, t] > 0)
            cn[b, t] = len(cells)
            for k, (y, x) in enumerate(cells[:cap]):
                ci[b, t, k] = occ[b, t, y, x] - 1
                cs[b, t, k] = np.sum(O.crop(out[b, :, :, t], (y, x), N=N))
    return cn, ci, cs, int((cn > cap).any())


def ref_assign(scene, out, maps=None):
    """prn_assign_oracle.assign per image -> keypoints [nb,17,3]."""
    maps = maps or scene_maps(scene)
    res, b0 = [], 0
    for i in range(scene.nimg):
        peaks, bboxes, old, _ = maps["per"][i]
        n = len(bboxes)
        if n:
            res.append(O.assign(peaks, bboxes, old, out[b0:b0 + n]))
        b0 += n
    return np.concatenate(res, 0) if res else np.zeros((0, 17, 3))


# ---------------------------------------------------------------------------------------------- inputs of the score kernels
@functools.lru_cache(maxsize=None)
def score_case(kind, h=H0, w=W0):
    """prn_out [2,h,w,17] float32 and a synthetic occ with one fully occupied plane per box (-> every window shape) and 1 % elsewhere.
    kind 'unit': uniform in (0, 1); 'signed': both signs, magnitudes over eight binades (summation order shows in the low bits)."""
    rs = np.random.RandomState({"unit": 5, "signed": 6}[kind])
    nb = 2
    out = rs.uniform(0.0, 1.0, (nb, h, w, 17)).astype(f32)
    out = np.where(out == 0, f32(0.5), out)
    if kind == "signed":
        out = (out * np.exp2(rs.randint(-4, 4, out.shape)).astype(f32) * np.where(rs.rand(*out.shape) < 0.5, -1, 1).astype(f32)).astype(f32)
    occ = np.where(rs.rand(nb, 17, h, w) < 0.01, rs.randint(1, 500, (nb, 17, h, w)), 0).astype(np.int32)
    occ[0, 3] = 1 + np.arange(h * w).reshape(h, w)
    occ[1, 16] = 1 + rs.permutation(h * w).reshape(h, w)
    out.setflags(write=False)
    occ.setflags(write=False)
    return out, occ


@functools.lru_cache(maxsize=None)
def score_ref(kind, N):
    out, occ = score_case(kind)
    return ref_scores(out, occ, N)


COUNT_CLASSES = {1: (0, 1, 2, H0 * W0), 64: (0, 1, 63, 64, 65, H0 * W0)}       # {0, 1, cap-1, cap, cap+1, all} for each cap


@functools.lru_cache(maxsize=None)
def count_case(cap, overflow):
    """occ [2,17,56,36] whose planes cycle through the planted count classes of `cap` (overflow=False: only those <= cap), cells at
    random places of the plane; prn_out uniform (0, 1)."""
    rs = np.random.RandomState(100 + cap + int(overflow))
    classes = [c for c in COUNT_CLASSES[cap] if overflow or c <= cap]
    nb, n = 2, H0 * W0
    occ = np.zeros((nb, 17, n), dtype=np.int32)
    for p in range(nb * 17):
        c = classes[p % len(classes)]
        cells = rs.permutation(n)[:c]
        occ[p // 17, p % 17, cells] = 1 + rs.randint(0, 1000, c)
    out = rs.uniform(0.0, 1.0, (nb, H0, W0, 17)).astype(f32)
    occ = occ.reshape(nb, 17, H0, W0)
    out.setflags(write=False)
    occ.setflags(write=False)
    return out, occ


@functools.lru_cache(maxsize=None)
def count_ref(cap, overflow):
    out, occ = count_case(cap, overflow)
    return ref_candidates(out, occ, 15, cap)


@functools.lru_cache(maxsize=None)
def argmax_case():
    """prn_out [5,56,36,17]: plane p = b*17 + t.  p < 64: a unique maximum whose index has lane p (i % 64 == p), in chunk p % 31;
    then equal maxima at i and i + 64 (one lane), at i and i + 1, at the first and the last cell, a constant plane, and a maximum in
    the last partial chunk (2016 = 31 * 64 + 32).  The rest are random with a unique maximum.  Returns (out, {plane: description})."""
    rs = np.random.RandomState(8)
    nb, n = 5, H0 * W0
    planes = rs.uniform(0.0, 1.0, (nb * 17, n)).astype(f32)
    what = {}
    for p in range(64):
        planes[p, 64 * (p % 31) + p] = 2.0
        what[p] = "unique lane %d" % p
    planes[64, [200, 264]] = 2.0
    what[64] = "i and i+64"
    planes[65, [777, 778]] = 2.0
    what[65] = "i and i+1"
    planes[66, [0, n - 1]] = 2.0
    what[66] = "first and last"
    planes[67, :] = 0.25
    what[67] = "constant"
    planes[68, 31 * 64 + 5] = 2.0
    what[68] = "last partial chunk"
    planes[69, [31 * 64 + 31, 63]] = 2.0
    what[69] = "last cell of the partial chunk and lane 63"
    out = np.ascontiguousarray(planes.reshape(nb, 17, H0, W0).transpose(0, 2, 3, 1))
    out.setflags(write=False)
    return out, what


# ====================================================================================================== comparisons
def check_build_maps(scene, h, w, occ, prn_in, err, want_err=0, skip_boxes=()):
    m = scene_maps(scene, h, w, tuple(skip_boxes))
    v = m["valid"]
    assert int(err) == want_err, "err word %d, expected %d" % (int(err), want_err)
    assert occ.dtype == np.int32 and prn_in.dtype == f32 and occ.shape == m["occ"].shape and prn_in.shape == m["prn_in"].shape
    bad = np.argwhere(occ[v] != m["occ"][v])
    assert len(bad) == 0, "%s %dx%d: occ differs in %d cells, first (valid box, type, y, x) = %s" % (scene.name, h, w, len(bad), bad[0])
    assert np.array_equal(prn_in[v].view(np.uint32), m["prn_in"][v].view(np.uint32)), \
        "%s %dx%d: blurred input differs from scipy's arithmetic in %d values" % (scene.name, h, w, int((prn_in[v] != m["prn_in"][v]).sum()))
    return int(v.sum()) * 17 * h * w


def check_scores(out, occ, ref, score, amax):
    """score [nb,17,h,w] (pre-filled with SENT_F) and amax [nb,17] of mpn_prn_scores against the np.sum dict and np.argmax."""
    keys = np.array(list(ref.keys()), dtype=np.int64).reshape(-1, 4)
    want = np.full(score.shape, SENT_F, dtype=f32)
    want[keys[:, 0], keys[:, 1], keys[:, 2], keys[:, 3]] = np.array(list(ref.values()), dtype=f32)
    assert len(ref) == int((occ > 0).sum())
    bad = np.argwhere(score.view(np.uint32) != want.view(np.uint32))
    assert len(bad) == 0, "%d cells differ from np.sum / the sentinel, first (b, t, y, x) = %s: got %r want %r" % (
        len(bad), bad[0], score[tuple(bad[0])], want[tuple(bad[0])])
    check_argmax(out, amax)
    return len(ref)


def check_argmax(out, amax):
    want = ref_argmax(out)
    assert amax.dtype == np.int32 and np.array_equal(amax, want), "arg-max differs at (b, t) = %s" % np.argwhere(amax != want)[:4].tolist()


def check_compact(out, ref, cap, cand_n, cand_id, cand_sc, amax, overflow):
    """The five results of mpn_prn_scores_compact (cand_id / cand_sc pre-filled with the sentinels) against ref_candidates()."""
    cn, ci, cs, over = ref
    assert np.array_equal(cand_n, cn), "cand_n differs at %s" % np.argwhere(cand_n != cn)[:4].tolist()
    assert np.array_equal(cand_id, ci), "cand_id (or a slot that should keep its sentinel) differs at %s" % np.argwhere(cand_id != ci)[:4].tolist()
    assert np.array_equal(cand_sc.view(np.uint32), cs.view(np.uint32)), "cand_score differs at %s" % np.argwhere(cand_sc != cs)[:4].tolist()
    assert int(overflow) == over, "overflow word %d, expected %d" % (int(overflow), over)
    check_argmax(out, amax)
    return int(np.minimum(cn, cap).sum())


def check_match(scene, want_kp, out_kp, flags, max_flagged=0, must_flag=()):
    """out_kp [nb,17,3] of the fast path against prn_assign_oracle.assign for every (image, type) the matcher did not flag."""
    a = scene.arrays()
    flags = np.asarray(flags).reshape(scene.nimg, 17)
    for im, t in must_flag:
        assert flags[im, t], "(image %d, type %d) must be flagged" % (im, t)
    nflag = int((flags != 0).sum())
    assert nflag <= max_flagged, "%d (image, type) pairs flagged, at most %d expected: %s" % (nflag, max_flagged, np.argwhere(flags).tolist())
    ok = flags[a["box_img"]] == 0                                    # [nb, 17]
    assert np.array_equal(out_kp[ok], want_kp[ok]), "%s: keypoints differ from the reference's assignment at (box, type) %s" % (
        scene.name, np.argwhere((out_kp != want_kp).any(-1) & ok)[:6].tolist())
    return int(ok.sum()), nflag


# ====================================================================================================== numpy models of the kernels
def blur_model(plane, wts=W9, mut=None):
    """prn_build_maps_kernel's blur in float64: centre tap, then pairs from the far tap inwards, rows then columns, clamped edges."""
    h, w = plane.shape

    def idx(n, d):
        i = np.arange(n) + d
        if mut == "reflect":                                         # scipy 'reflect': (d c b a | a b c d | d c b a)
            i = np.where(i < 0, -i - 1, i)
            i = np.where(i >= n, 2 * n - 1 - i, i)
        return np.clip(i, 0, n - 1)

    def axis(a, ax):
        n = a.shape[ax]
        tmp = a * wts[4]
        order = range(-4, 0) if mut != "near tap" else range(-1, -5, -1)
        for jj in order:
            tmp = tmp + (np.take(a, idx(n, jj), ax) + np.take(a, idx(n, -jj), ax)) * wts[4 + jj]
        return tmp

    return axis(axis(np.asarray(plane, dtype=f64), 0), 1)


def model_build_maps(a, h, w, in_thres, mut=None, wts=W9):
    """prn_build_maps_kernel on the flat arrays `a` of Scene.arrays() -> occ, prn_in, err."""
    nb = a["boxes"].shape[0]
    occ = np.zeros((nb, 17, h, w), dtype=np.int32)
    prn_in = np.zeros((nb, h, w, 17), dtype=f32)
    err = 0
    for b in range(nb):
        bx, by, bw, bh = a["boxes"][b]
        off = a["joint_off"][a["box_img"][b]]
        first = 0 if mut == "no rebase" else off[0]
        lo_x, lo_y, hi_x, hi_y = bx - bw * in_thres, by - bh * in_thres, bx + bw * (1.0 + in_thres), by + bh * (1.0 + in_thres)
        xs, ys = float(w) / math.ceil(bw), float(h) / math.ceil(bh)
        for t in range(17):
            for p in range(off[t], off[t + 1]):
                px, py = a["peaks"][p]
                if mut == ">= inside":
                    if not (px >= lo_x and py >= lo_y and px <= hi_x and py <= hi_y):
                        continue
                elif not (px > lo_x and py > lo_y and px < hi_x and py < hi_y):
                    continue
                x0, y0 = int((px - bx) * xs), int((py - by) * ys)
                if mut == "independent ifs":
                    if x0 >= w: x0 = w - 1
                    if y0 >= h: y0 = h - 1
                    if x0 < 0: x0 = 0
                    if y0 < 0: y0 = 0
                elif x0 >= w and y0 >= h: x0, y0 = w - 1, h - 1
                elif x0 >= w: x0 = w - 1
                elif y0 >= h: y0 = h - 1
                elif x0 < 0 and y0 < 0: x0, y0 = 0, 0
                elif x0 < 0: x0 = 0
                elif y0 < 0: y0 = 0
                if mut == "no wrap":
                    if x0 < 0 or y0 < 0:
                        continue
                else:
                    if x0 < 0: x0 += w
                    if y0 < 0: y0 += h
                if x0 < 0 or x0 >= w or y0 < 0 or y0 >= h:
                    err = 1
                    continue
                if mut == "first wins" and occ[b, t, y0, x0]:
                    continue
                occ[b, t, y0, x0] = p - first + 1
            prn_in[b, :, :, t] = blur_model((occ[b, t] > 0).astype(f64), wts, mut).astype(f32)
    return occ, prn_in, err


def _block(v, mut=None):
    n = len(v)
    if n < 8 or mut == "left to right":
        res = f32(0)
        for x in v:
            res = f32(res + x)
        return res
    r = v[:8].copy()
    m = n - n % 8
    for i in range(8, m, 8):
        r += v[i:i + 8]
    res = f32(f32(f32(r[0] + r[1]) + f32(r[2] + r[3])) + f32(f32(r[4] + r[5]) + f32(r[6] + r[7])))
    for x in v[m:]:
        res = f32(res + x)
    return res


def np_sum_model(v, mut=None):
    """np_sum_window of the kernel on the flattened float32 window v (n <= 256)."""
    v = np.ascontiguousarray(v, dtype=f32).reshape(-1)
    n = len(v)
    if n <= 128 or mut == "left to right":
        return _block(v, mut)
    n2 = n // 2
    if mut != "split not rounded":
        n2 -= n2 % 8
    return f32(_block(v[:n2]) + _block(v[n2:]))


def window_model(plane, y, x, N, mut=None):
    h, w = plane.shape
    half = (N - 1) // 2
    r0, c0 = max(y - half, 0), max(x - half, 0)
    if mut == "r1 off by one":                                     # clipped to the last index instead of one past it
        r1, c1 = min(y + half + 1, h - 1), min(x + half + 1, w - 1)
        r1, c1 = max(r1, r0 + 1), max(c1, c0 + 1)
    else:
        r1, c1 = (h if y + half + 1 > h - 1 else y + half + 1), (w if x + half + 1 > w - 1 else x + half + 1)
    return plane[r0:r1, c0:c1]


def argmax_model(flat, mut=None):
    """The kernels' arg-max: per lane the first maximum of its strided indices, then the butterfly keeping the lower index."""
    best, best_i = np.full(64, -np.inf, dtype=f32), np.full(64, 0x7fffffff, dtype=np.int64)
    for i0 in range(0, len(flat), 64):
        v = flat[i0:i0 + 64]
        k = len(v)
        up = (v >= best[:k]) if mut == "last maximum" else (v > best[:k])
        best[:k] = np.where(up, v, best[:k])
        best_i[:k] = np.where(up, i0 + np.arange(k), best_i[:k])
    m = best.max()
    cand = best_i[best == m]
    return int(cand.max() if mut == "last maximum" else cand.min())


def model_scores(out, occ, N, score, mut=None):
    """prn_scores_kernel: writes into `score` (pre-filled by the caller) and returns argmax."""
    nb, h, w, _ = out.shape
    amax = np.zeros((nb, 17), dtype=np.int32)
    for b in range(nb):
        for t in range(17):
            plane = out[b, :, :, t]
            amax[b, t] = argmax_model(plane.reshape(-1), mut)
            for y, x in np.argwhere(occ[b, t] > 0):
                score[b, t, y, x] = np_sum_model(window_model(plane, y, x, N, mut), mut)
    return amax


def model_compact(out, occ, N, cap, mut=None, max_scored=None):
    """prn_scores_compact_kernel -> cand_n, cand_id, cand_sc (sentinel-filled), argmax, overflow."""
    nb, h, w, _ = out.shape
    n = h * w
    cn = np.zeros((nb, 17), dtype=np.int32)
    ci = np.full((nb, 17, cap), SENT_I, dtype=np.int32)
    cs = np.full((nb, 17, cap), SENT_F, dtype=f32)
    amax = np.zeros((nb, 17), dtype=np.int32)
    over = 0
    lim = cap + 1 if mut == "pos <= cap" else cap
    for b in range(nb):
        for t in range(17):
            plane = out[b, :, :, t]
            amax[b, t] = argmax_model(plane.reshape(-1), mut)
            cells = np.nonzero(occ[b, t].reshape(-1) > 0)[0]
            if mut == "per lane order":
                cells = np.array(sorted(cells, key=lambda i: (i % 64, i)), dtype=np.int64)
            cn[b, t] = len(cells)
            flat_i, flat_s = ci.reshape(-1), cs.reshape(-1)
            base = (b * 17 + t) * cap
            for pos, i in enumerate(cells[:lim]):
                if base + pos < flat_i.size:                        # (the mutant's extra slot is the next plane's first)
                    flat_i[base + pos] = occ[b, t].reshape(-1)[i] - 1
                    flat_s[base + pos] = np_sum_model(window_model(plane, i // w, i % w, N, mut), mut)
            if (len(cells) >= cap) if mut == "overflow >= cap" else (len(cells) > cap):
                over = 1
    return cn, ci, cs, amax, over


def model_match(a, cand_n, cand_id, cand_sc, cap, amax, h, w, mut=None):
    """mpn_prn_match_host in numpy -> out_kp [nb,17,3], tie_flags [nimg,17]."""
    nimg = len(a["box_start"]) - 1
    nb = a["boxes"].shape[0]
    out = np.zeros((nb, 17, 3))
    flags = np.zeros((nimg, 17), dtype=np.uint8)
    for im in range(nimg):
        b0, n = int(a["box_start"][im]), int(a["box_start"][im + 1] - a["box_start"][im])
        if n <= 0:
            continue
        first = int(a["joint_off"][im, 0])
        any_empty = False
        for t in range(17):
            ids, total = [], 0
            for bi in range(n):
                c = int(cand_n[b0 + bi, t])
                total += c
                if c > cap:
                    flags[im, t] = 1
                    break
                for k in range(c):
                    i = int(cand_id[b0 + bi, t, k])
                    if i not in ids:
                        if len(ids) >= 512:
                            flags[im, t] = 1
                            break
                        ids.append(i)
            if total == 0:
                any_empty = True
                continue
            if flags[im, t]:
                continue
            ncol = len(ids)
            if n > 64 or ncol > 64:
                flags[im, t] = 1
                continue
            table = np.zeros((n, ncol))
            for bi in range(n):
                for k in range(int(cand_n[b0 + bi, t])):
                    table[bi, ids.index(int(cand_id[b0 + bi, t, k]))] = float(cand_sc[b0 + bi, t, k])
            tie = False
            for bi in range(n):
                pos = np.sort(table[bi][table[bi] > 0])
                tie = tie or bool((np.diff(pos) == 0).any())
            if mut != "ties in rows only":
                for c in range(ncol):
                    pos = np.sort(table[:, c][table[:, c] > 0])
                    tie = tie or bool((np.diff(pos) == 0).any())
            if tie:
                flags[im, t] = 1
                continue
            for bi in range(n):
                used = np.zeros(ncol, dtype=bool)
                for _ in range(ncol):
                    r = -1
                    for c in range(ncol):
                        if not used[c] and (r < 0 or table[bi, c] > table[bi, r]):
                            r = c
                    used[r] = True
                    if not table[bi, r] > 0:
                        break
                    bestb = 0
                    for b2 in range(1, n):
                        if table[b2, r] > table[bestb, r]:
                            bestb = b2
                    take = bestb == bi
                    if not take and mut != "no worst column":
                        take = all(table[bestb, c] > table[bestb, r] for c in range(ncol) if c != r)
                    if take:
                        out[b0 + bi, t] = [a["peaks"][first + ids[r], 0], a["peaks"][first + ids[r], 1], 1.0]
                        break
        if any_empty:
            for bi in range(n):
                bx = a["boxes"][b0 + bi]
                xs, ys = float(w) / math.ceil(bx[2]), float(h) / math.ceil(bx[3])
                for t in range(17):
                    if cand_n[b0 + bi, t] != 0:
                        continue
                    am = int(amax[b0 + bi, t])
                    out[b0 + bi, t] = [float(am % w) / xs + bx[0], float(am // w) / ys + bx[1], 0.0]
    return out, flags


# ====================================================================================================== the host matcher through ctypes
def match_host(a, cand_n, cand_id, cand_sc, cap, amax, h=H0, w=W0, guard=64):
    """mpn_prn_match_host of the built library (no device needed) -> out_kp, tie_flags.  out_kp and tie_flags sit between guard
    bands that must come back untouched."""
    import ctypes
    from multiposenet.pytorch_amd import _lib
    L = _lib.lib()
    nimg = len(a["box_start"]) - 1
    nb = a["boxes"].shape[0]
    kp = np.zeros(guard + nb * 51 + guard)
    kp[:guard] = kp[guard + nb * 51:] = 12345.5
    fl = np.zeros(guard + nimg * 17 + guard, dtype=np.uint8)
    fl[:guard] = fl[guard + nimg * 17:] = 0xAB
    keep = [np.ascontiguousarray(a["box_start"], dtype=np.int32), np.ascontiguousarray(a["boxes"], dtype=f64),
            np.ascontiguousarray(a["joint_off"], dtype=np.int32), np.ascontiguousarray(a["peaks"] if len(a["peaks"]) else np.zeros((1, 2)), dtype=f64),
            np.ascontiguousarray(cand_n, dtype=np.int32), np.ascontiguousarray(cand_id, dtype=np.int32), np.ascontiguousarray(cand_sc, dtype=f32),
            np.ascontiguousarray(amax, dtype=np.int32)]
    p = [ctypes.c_void_p(x.ctypes.data) for x in keep]
    st = L.mpn_prn_match_host(nimg, p[0], p[1], p[2], p[3], p[4], p[5], p[6], int(cap), p[7], h, w,
                              ctypes.c_void_p(kp.ctypes.data + guard * 8), ctypes.c_void_p(fl.ctypes.data + guard))
    assert st == 0, "mpn_prn_match_host returned %d" % st
    assert (kp[:guard] == 12345.5).all() and (kp[guard + nb * 51:] == 12345.5).all(), "out_kp written out of bounds"
    assert (fl[:guard] == 0xAB).all() and (fl[guard + nimg * 17:] == 0xAB).all(), "tie_flags written out of bounds"
    return kp[guard:guard + nb * 51].reshape(nb, 17, 3).copy(), fl[guard:guard + nimg * 17].reshape(nimg, 17).copy()


def standin_out(scene, seed, maps=None):
    """A random stand-in for the PRN output of every box of the scene, float32 in (0, 1)."""
    nb = sum(len(b) for b in scene.boxes)
    return np.random.RandomState(seed).uniform(0.01, 1.0, (nb, H0, W0, 17)).astype(f32)


# ---------------------------------------------------------------------------------------------- planted matcher cases
# two boxes of integer geometry (scale 0.5), B = A shifted by 30 px in x; peak sites at least 15 cells apart in both boxes so that the
# 15x15 windows of one box never hold two planted values: a window sum is then exactly the planted score
BOX_A, BOX_B = (100.0, 100.0, 172.0, 212.0), (130.0, 100.0, 202.0, 212.0)
SITES = {"P0": (136.0, 110.0), "P1": (166.0, 150.0), "P2": (140.0, 190.0), "PA": (90.0, 150.0)}     # PA: inside A's margin only


def planted_scene(sites, nboxes=2):
    """One image, boxes A (and B), the named sites as peaks of joint type 0 (peak id = position in `sites`); other types empty."""
    return Scene("planted " + " ".join(sites) + " %d" % nboxes, [[(SITES[s][0], SITES[s][1], 1, 0, 0) for s in sites]], [[BOX_A, BOX_B][:nboxes]])


def planted_out(scene, scores):
    """PRN output that is zero except at the cells of the planted peaks: scores = {(box, peak id): value} -> out [nb,56,36,17]."""
    m = scene_maps(scene)
    out = np.zeros((m["occ"].shape[0], H0, W0, 17), dtype=f32)
    for (b, k), v in scores.items():
        cell = np.argwhere(m["occ"][b, 0] == k + 1)
        assert len(cell) == 1, "peak %d is not a cell of box %d" % (k, b)
        out[b, cell[0][0], cell[0][1], 0] = v
    return out
