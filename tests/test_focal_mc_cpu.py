"""The oracle's focal loss with K > 1 classes (one-hot targets) against the reference's own FocalLoss: losses and autograd gradients
of g16_focal_mc.npz (tests/golden/make_golden_focal_mc.py), for K = 3 and K = 80 with positives of several classes, anchors in the
ignored IoU band and probabilities past both clamp bounds.  This pins the yardstick the GPU tests of the multi-class kernels use."""
import numpy as np
import pytest
import torch

from helpers import gold
from oracle import posenet_oracle as po


def t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


@pytest.mark.parametrize("K", [3, 80])
def test_oracle_multiclass_focal_matches_reference_golden(K):
    g = gold("g16_focal_mc.npz")
    p = "k%d_" % K
    cls = t(g[p + "cls"]).requires_grad_(True)
    reg = t(g[p + "reg"]).requires_grad_(True)
    assert cls.shape[2] == K
    c, r = po.focal_loss(cls, reg, t(g[p + "anchors"])[None], t(g[p + "anno"]))
    c, r = c.mean(), r.mean()
    ref = g[p + "loss"]
    assert abs(c.item() - ref[0]) <= 1e-6 * abs(ref[0]), (c.item(), ref[0])
    assert abs(r.item() - ref[1]) <= 1e-6 * abs(ref[1]), (r.item(), ref[1])
    dcls, = torch.autograd.grad(c, cls, retain_graph=True)
    dreg, = torch.autograd.grad(r, reg)
    for got, want in ((dcls, t(g[p + "dcls"])), (dreg, t(g[p + "dreg"]))):
        err = (got.double() - want.double()).abs()
        assert bool((err <= 1e-5 * want.double().abs() + 1e-7 * want.abs().max().item()).all()), err.max().item()
    # the cases exercise what they claim: positives of more than one class, clamped probabilities on both sides
    anno = g[p + "anno"]
    assert len(np.unique(anno[anno[:, :, 4] != -1][:, 4])) > 1
    cl = g[p + "cls"]
    assert (cl < 1e-4).any() and (cl > 1 - 1e-4).any()
    assert (g[p + "dcls"][cl < 1e-4] == 0).all() and (g[p + "dcls"][cl > 1 - 1e-4] == 0).all()
