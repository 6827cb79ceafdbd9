#!/usr/bin/env python3
"""g18_prn_train.npz: the (input, label) pairs of the REAL ``PRN_CocoDataset`` (datasets/coco_data/prn_data_pipeline.py:10-123, with
the real ``skimage.filters.gaussian``) on a small hand-made annotation set, for coeff 1, 2 and 3.

Run with an interpreter that has scikit-image, as make_golden_prn_gaussian.py is:
    python3 tests/golden/make_golden_prn_train.py REFERENCE_ROOT
(REFERENCE_ROOT: a checkout of the reference).  That interpreter need not have torch: the module's
two project imports are never touched by get_data / get_anns, so ``torch.utils.data.Dataset`` and ``datasets.coco_data.heatmap``
are stubbed and the module is loaded by file path.  ``coco`` is a small stand-in with the three pycocotools calls the class makes
(getAnnIds, loadAnns, loadImgs), keeping pycocotools' orders: annotation ids in file order, an image's annotations in file order.

Recorded per coeff: float64 ``weights`` / ``output`` of every sample in get_anns order (zeros where the reference raises) and the
name of the exception; once: the annotation columns, the get_anns order, both tap vectors as this interpreter's scipy computes
them, and the library versions.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import scipy
import skimage
from scipy.ndimage import filters as _ndf

HERE = os.path.dirname(os.path.abspath(__file__))
if len(sys.argv) != 2:
    raise SystemExit(__doc__)
REFERENCE = sys.argv[1]
THRESHOLD, NUM_OF_KEYPOINTS = 0.21, 3


def stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def load_reference():
    stub("torch")
    stub("torch.utils")
    stub("torch.utils.data", Dataset=object)
    stub("datasets")
    stub("datasets.coco_data")
    stub("datasets.coco_data.heatmap", putGaussianMaps=None)
    spec = importlib.util.spec_from_file_location("prn_data_pipeline", os.path.join(REFERENCE, "datasets", "coco_data", "prn_data_pipeline.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class FakeCoco(object):
    def __init__(self, anns):
        self.anns = {}
        self.imgToAnns = {}
        for a in anns:
            self.anns[a["id"]] = a
            self.imgToAnns.setdefault(a["image_id"], []).append(a)

    def getAnnIds(self, imgIds=[]):
        if imgIds == []:
            return list(self.anns.keys())
        return [a["id"] for a in self.imgToAnns[imgIds]]

    def loadAnns(self, ids=[]):
        if isinstance(ids, (list, tuple)):
            return [self.anns[i] for i in ids]
        return [self.anns[ids]]

    def loadImgs(self, ids=[]):
        return [{"id": ids}]


def person(box, nk, rel, vis, crowd=0, frame=None):
    """Keypoints at frame_origin + rel * (ceil(w), ceil(h)) of ``frame`` (default: the own box, origin int(x), int(y)): rel 0..1
    is inside, beyond is outside by that many box sizes.  Non-integer coordinates unless rel says otherwise."""
    f = box if frame is None else frame
    ox, oy, cw, ch = int(f[0]), int(f[1]), max(np.ceil(f[2]), 1.0), max(np.ceil(f[3]), 1.0)
    kp = []
    for (rx, ry), v in zip(rel, vis):
        kp += [float(ox + rx * cw), float(oy + ry * ch), v]
    return {"bbox": [float(b) for b in box], "num_keypoints": nk, "iscrowd": crowd, "keypoints": kp}


def inside_rel(rs, n=17):
    return [(float(rs.uniform(0.03, 0.97)), float(rs.uniform(0.03, 0.97))) for _ in range(n)]


def annotations():
    rs = np.random.RandomState(18)
    A_BOX = [100.5, 50.25, 80.3, 200.7]
    anns = []
    # B: overlaps A.  Its joints 0..3 lie in A's margin (negative cells of A's input: x only, y only, both), joint 4 between
    # int(bbox[0]) - w t and bbox[0] - w t of A (inside only if the margin test wrongly uses the truncated corner), joints 12..14
    # are v = 0 with coordinates inside A (must be ignored), joint 5 shares a cell with A's and the crowd's joint 5.
    b_rel = inside_rel(rs)
    b = person([90.0, 40.0, 85.0, 215.0], 14, b_rel, [2, 1, 2, 1, 2, 2, 1, 2, 1, 2, 1, 2, 0, 0, 0, 1, 2])
    for j, (px, py) in {0: (95.3, 120.6), 1: (130.7, 42.1), 2: (92.2, 41.3), 3: (84.9, 30.2), 4: (83.4, 150.3), 5: (140.4, 130.8),
                        12: (120.0, 100.0), 13: (150.5, 160.5), 14: (110.0, 200.0)}.items():
        b["keypoints"][3 * j], b["keypoints"][3 * j + 1] = px, py
    anns.append(b)
    # crowd annotation: contributes to the inputs of its image, is never a sample
    c = person([95.0, 45.0, 120.0, 230.0], 10, inside_rel(rs), [1] * 10 + [0] * 7, crowd=1, frame=A_BOX)
    c["keypoints"][15], c["keypoints"][16] = 140.4, 130.8
    anns.append(c)
    # A: everything inside its box
    a = person(A_BOX, 17, inside_rel(rs), [2, 1] * 8 + [2])
    a["keypoints"][15], a["keypoints"][16] = 140.4, 130.8
    anns.append(a)
    # two keypoints only: contributes, is not a sample (num_keypoints <= 3)
    anns.append(person([110.0, 60.0, 30.0, 90.0], 2, inside_rel(rs), [0, 2, 0, 0, 0, 0, 2] + [0] * 10, frame=A_BOX))
    # D: IndexError (x0 >= W with y0 < -H) on joint 0
    anns.append(person([400.0, 300.0, 30.0, 60.0], 12, [(1.4, -1.5)] + inside_rel(rs, 16), [2] + [1] * 11 + [0] * 5))
    # the single person of the second image: integer box and integer keypoints
    rel_l = [(round(rx * 100) / 100.0, round(ry * 150) / 150.0) for rx, ry in inside_rel(rs)]
    anns.append(dict(person([20, 30, 100, 150], 17, rel_l, [2] * 8 + [0] + [1] * 8), image_id=202))
    # C: own keypoints beyond the box on every side
    c_rel = inside_rel(rs)
    c_rel[0] = (1.3, 0.5)        # x0 >= W
    c_rel[1] = (0.4, 1.2)        # y0 >= H
    c_rel[2] = (1.5, 1.7)        # both
    c_rel[3] = (1.2, -0.4)       # x0 >= W, y0 in [-H, 0): wraps
    c_rel[4] = (-0.5, 1.3)       # y0 >= H, x0 in [-W, 0): wraps
    c_rel[5] = (-1.6, 1.1)       # y0 >= H, x0 < -W: the try/except
    c_rel[6] = (-0.15, 0.6)      # x0 < 0
    c_rel[7] = (0.7, -0.12)      # y0 < 0
    c_rel[8] = (-0.1, -0.1)      # both < 0
    c_rel[9] = (1.1, -1.005)     # x0 >= W, y0 == -H: the last row index that still wraps
    c_rel[10] = (1.05, 1.0)      # exactly on the far corner
    anns.append(person([300.4, 200.6, 40.2, 100.9], 17, c_rel, [1, 2] * 8 + [1]))
    # ZeroDivisionError: w == 0
    anns.append(person([520.0, 300.0, 0.0, 40.0], 8, inside_rel(rs), [1] * 8 + [0] * 9))
    # E: IndexError on joint 9
    e_rel = inside_rel(rs)
    e_rel[9] = (2.0, -1.2)
    anns.append(person([50.7, 400.2, 20.5, 30.5], 12, e_rel, [0] * 5 + [2] * 12))
    # F: w < 1, ceil(w) == 1
    anns.append(person([500.2, 100.6, 0.6, 50.0], 8, [(0.25 + 0.04 * k, 0.05 + 0.055 * k) for k in range(17)], [2] * 8 + [0] * 9))
    # K: just above the keypoint threshold, integer coordinates next to A
    k = person([150.0, 80.0, 60.0, 120.0], 4, inside_rel(rs), [0] * 13 + [2, 2, 1, 1])
    k["keypoints"] = [float(round(v)) for v in k["keypoints"]]
    anns.append(k)
    # ZeroDivisionError: ceil(-0.5) == 0
    anns.append(person([10.0, 10.0, 20.0, -0.5], 8, inside_rel(rs), [1] * 8 + [0] * 9))
    for i, an in enumerate(anns):
        an.setdefault("image_id", 101)
        an["id"] = 9000 + 7 * i
    return anns


def main():
    mod = load_reference()
    anns = annotations()
    coco = FakeCoco(anns)
    pos = {a["id"]: i for i, a in enumerate(anns)}
    out = {
        "bbox": np.array([a["bbox"] for a in anns], dtype=np.float64),
        "keypoints": np.array([a["keypoints"] for a in anns], dtype=np.float64),
        "image_id": np.array([a["image_id"] for a in anns], dtype=np.int64),
        "iscrowd": np.array([a["iscrowd"] for a in anns], dtype=np.int64),
        "num_keypoints": np.array([a["num_keypoints"] for a in anns], dtype=np.int64),
        "threshold": np.array(THRESHOLD), "num_of_keypoints": np.array(NUM_OF_KEYPOINTS),
        "taps9": _ndf._gaussian_kernel1d(1.0, 0, 4), "taps17": _ndf._gaussian_kernel1d(2.0, 0, 8),
        "skimage_version": np.array(skimage.__version__), "scipy_version": np.array(scipy.__version__),
        "numpy_version": np.array(np.__version__),
    }
    for coeff in (1, 2, 3):
        ds = mod.PRN_CocoDataset(coco, NUM_OF_KEYPOINTS, coeff, THRESHOLD, 480, 4)
        order = np.array([pos[a["id"]] for a in ds.anns], dtype=np.int64)
        if coeff == 1:
            out["order"] = order
        assert np.array_equal(order, out["order"])
        H, W = 28 * coeff, 18 * coeff
        weights, output, exc = np.zeros((len(ds), H, W, 17)), np.zeros((len(ds), H, W, 17)), []
        for s in range(len(ds)):
            try:
                weights[s], output[s] = ds[s]
                exc.append("")
            except Exception as e:                        # recorded, not hidden: the name is part of the fixture
                exc.append(type(e).__name__)
        out["weights_%d" % coeff], out["output_%d" % coeff], out["exc_%d" % coeff] = weights, output, np.array(exc)
        print("coeff %d: %d samples, raising %s, weights max %.4f, output max %.4f" % (
            coeff, len(ds), [(s, e) for s, e in enumerate(exc) if e], weights.max(), output.max()))
    path = os.path.join(HERE, "g18_prn_train.npz")
    np.savez_compressed(path, **out)
    print("skimage", skimage.__version__, "scipy", scipy.__version__, "numpy", np.__version__, "->", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
