#!/usr/bin/env python
"""Generate g16_focal_mc.npz: the reference's own multi-class FocalLoss (network/losses.py:27-137) on the CPU.

For K in {3, 80}: the classification and regression losses and, from autograd, d(cls loss)/d(classification) and
d(reg loss)/d(regression).  Every image holds valid annotations (losses.py:49-53 cannot run an empty image under current torch);
annotations of several classes are placed on anchors (positives), next to them (IoU in [0.4, 0.5): ignored), and probabilities are
driven past both clamp bounds.  Shims as make_golden.py: Tensor.cuda / Module.cuda are no-ops and bool.__rsub__ is patched for the
dead statement at losses.py:124.
"""
import os
import sys

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
REF = os.environ.get("MPN_REFERENCE", "/root/reference")
sys.path.insert(0, REF)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

from multiposenet.pytorch_amd import synthetic as weightgen  # noqa: E402
from oracle import posenet_oracle as po  # noqa: E402

torch.Tensor.cuda = lambda self, *a, **k: self
nn.Module.cuda = lambda self, *a, **k: self
_orig_rsub = torch.Tensor.__rsub__


def _rsub(self, other):
    if self.dtype == torch.bool:
        return torch.logical_not(self)
    return _orig_rsub(self, other)


torch.Tensor.__rsub__ = _rsub

from network.losses import FocalLoss  # noqa: E402

# (K, B, H, W): K = 80 on a small image keeps the file under 1 MiB
CASES = ((3, 3, 128, 96), (80, 2, 64, 48))


def make_case(K, B, H, W, seed):
    an = po.anchors_for_image(H, W)[0]                                   # [A, 4]
    A = an.shape[0]
    g = np.random.default_rng(seed)
    maxn = 6
    anno = -np.ones((B, maxn, 5), np.float32)
    for b in range(B):
        n = 3 + b % 2
        picks = g.choice(A, size=n, replace=False)
        for i, a in enumerate(picks):
            box = an[a].copy()
            w, h = box[2] - box[0], box[3] - box[1]
            if i == n - 1:
                box[2] += 0.6 * w                                         # a stretched box: its own anchor lands near the ignored band
            else:
                box += np.float32(0.03) * np.array([w, h, w, h], np.float32) * g.uniform(-1, 1, 4).astype(np.float32)
            anno[b, i, :4] = box
            anno[b, i, 4] = float((b * 7 + i * 5) % K)                    # several classes per image and across images
    cls = weightgen.uniform(16, "cls_k%d" % K, (B, A, K), 0.0, 1.0)
    flat = cls.reshape(-1)
    idx = g.choice(flat.size, size=max(8, flat.size // 50), replace=False)
    q = len(idx) // 4
    flat[idx[:q]] = 0.0                                                   # below the lower clamp bound
    flat[idx[q:2 * q]] = 1.0                                              # above the upper one
    flat[idx[2 * q:3 * q]] = 5e-5
    flat[idx[3 * q:]] = 1.0 - 5e-5
    reg = weightgen.normal(16, "reg_k%d" % K, (B, A, 4), std=0.5)
    return an, anno, cls, reg


def band_counts(an, anno):
    t = torch.from_numpy
    pos = ign = 0
    for b in range(anno.shape[0]):
        v = anno[b][anno[b, :, 4] != -1]
        iou = po.calc_iou(t(an), t(v[:, :4])).max(dim=1)[0]
        pos += int((iou >= 0.5).sum())
        ign += int(((iou >= 0.4) & (iou < 0.5)).sum())
    return pos, ign


def main():
    out = {}
    for K, B, H, W in CASES:
        an, anno, cls_np, reg_np = make_case(K, B, H, W, seed=K)
        pos, ign = band_counts(an, anno)
        assert pos > 0 and ign > 0, (K, pos, ign)
        cls = torch.from_numpy(cls_np.copy()).requires_grad_(True)
        reg = torch.from_numpy(reg_np.copy()).requires_grad_(True)
        c, r = FocalLoss()(cls, reg, torch.from_numpy(an)[None], torch.from_numpy(anno))
        c = c.mean()
        r = r.mean()
        dcls, = torch.autograd.grad(c, cls, retain_graph=True)
        dreg, = torch.autograd.grad(r, reg)
        p = "k%d_" % K
        out[p + "anchors"] = an
        out[p + "anno"] = anno
        out[p + "cls"] = cls_np
        out[p + "reg"] = reg_np
        out[p + "loss"] = np.array([c.item(), r.item()], dtype=np.float64)
        out[p + "dcls"] = dcls.numpy()
        out[p + "dreg"] = dreg.numpy()
        print("K=%d B=%d %dx%d A=%d: positives %d, ignored %d, cls %.6f reg %.6f" % (K, B, H, W, an.shape[0], pos, ign, c.item(), r.item()))
    out["ks"] = np.array([k for k, _, _, _ in CASES], np.int64)
    path = os.path.join(HERE, "g16_focal_mc.npz")
    np.savez_compressed(path, **out)
    print("wrote g16_focal_mc.npz (%.1f KB)" % (os.path.getsize(path) / 1024.0))


if __name__ == "__main__":
    main()
