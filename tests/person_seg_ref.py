"""Plain-numpy restatement of the two planes mpn_segm_person_masks composes and of the warp of ``mask_all``, for
tests/test_person_seg_cpu.py and tests/test_person_seg_gpu.py (test-side only; the product never imports it).

For one image, its person annotations in json order, ``M_p`` = ``segm_ref.ann_to_mask`` of annotation ``p``, the kernel's walk is
restated SEQUENTIALLY over whole H x W arrays (:func:`compose`)::

    all = 0; miss = 0; uni = 0
    for p in order:
        uni |= M_p                                            # everyone, whatever the kind
        if iscrowd(p):            miss |= M_p & ~all
        else:                     all  |= M_p
                                  if num_keypoints(p) <= 0: miss |= M_p
    mask_miss = 255 where miss == 0, else 0                   # mask_miss_ref.compose, unchanged
    mask_all  = 255 where uni  != 0, else 0

:func:`closed_form` is the rule as the issue states it, without a walk: the OR of all masks.  An empty list gives all 0.

``mis`` names ONE modelled misreading of ``mask_all`` (test_person_seg_cpu.py checks that the committed inputs reject each):
  "no_crowd"       crowds left out (``all`` of the mask_miss walk stored as it is);
  "crowd_reduced"  crowds reduced by ``all``: inside a crowd's mask the plane is ASSIGNED the reduced crowd ``M_c & ~all`` (all as
                   accumulated so far) instead of being ORed with the crowd, so the people a crowd overlaps vanish;
  "no_nokp"        people without keypoints left out;
  "dropped"        the dropping rule of ``pack_mask_miss`` applied to the two-plane pack: people with keypoints after the image's
                   last crowd never reach the kernel.
The warp's misreading, "outside 255", is :func:`plane_ref` with ``border=255``.

The committed case is the seven instances of tests/segm_cases.py, as mask_miss_ref builds their annotations, with the kinds
:data:`CASE_KINDS`: a crowd over earlier people, people with keypoints AFTER the last crowd, one person without keypoints.  At
5 x 6 those instances cannot reject all four (one of them covers the whole image and only two of the rest own a cell), so the case
at that size is the hand-written :data:`HAND` with the same roles.
"""
import numpy as np

import augment_ref as ar
import mask_miss_ref as mr
import segm_cases as sc
import segm_ref as sr

K, N, C = mr.K, mr.N, mr.C
MISREADINGS = ["no_crowd", "crowd_reduced", "no_nokp", "dropped"]

# star K, overlapping parts C, mixed N, borders C (the last crowd), band K, corner K, the empty one N
CASE_KINDS = (K, C, N, C, K, K, N)
SIZES = [(5, 6), (37, 53), (64, 65), (130, 70)]                 # the CPU sizes; the GPU tests add the tile edges
GPU_SIZES = SIZES + [(513, 66), (520, 131)]


def compose(masks, kinds, mis=None):
    """The walk above over ready masks (at least one) -> mask_all, uint8 [h, w]."""
    masks = [np.asarray(m).astype(bool) for m in masks]
    kinds = list(kinds)
    if mis == "dropped":
        last_crowd = max([i for i, k in enumerate(kinds) if k == C] or [-1])
        keep = [i for i, k in enumerate(kinds) if k != K or i < last_crowd]
        masks, kinds = [masks[i] for i in keep], [kinds[i] for i in keep]
        if not masks:
            return None
    every = np.zeros_like(masks[0])
    uni = np.zeros_like(masks[0])
    for m, k in zip(masks, kinds):
        if k == C:
            if mis == "no_crowd":
                continue
            if mis == "crowd_reduced":
                uni = (uni & ~m) | (m & ~every)
            else:
                uni |= m
        else:
            every |= m
            if k == N and mis == "no_nokp":
                continue
            uni |= m
    return np.where(uni, 255, 0).astype(np.uint8)


def closed_form(masks):
    """255 where any mask covers the pixel."""
    return np.where(np.any(np.stack([np.asarray(m).astype(bool) for m in masks]), axis=0), 255, 0).astype(np.uint8)


def mask_all(anns, h, w, mis=None):
    """mask_all of one h x w image from its annotation dicts."""
    if len(anns) == 0:
        return np.zeros((h, w), dtype=np.uint8)
    got = compose([sr.ann_to_mask(a["segmentation"], h, w) for a in anns], [mr.kind_of(a) for a in anns], mis)
    return np.zeros((h, w), dtype=np.uint8) if got is None else got


def _rle(rows):
    m = np.array([[int(ch) for ch in row] for row in rows], dtype=np.uint8)
    return {"size": list(m.shape), "counts": sc.mask_counts(m)}


# 5 x 6: a person, a crowd over part of it, a person without keypoints, a person with keypoints after the last crowd
HAND = [(["000000", "011100", "011100", "011100", "000000"], K),
        (["000000", "000000", "001111", "001111", "001111"], C),
        (["110000", "110000", "000000", "000000", "000000"], N),
        (["000011", "000000", "000000", "000000", "000000"], K)]


def case_annotations(h, w):
    """-> (annotations, kinds) of the committed case at one size."""
    if (h, w) == (5, 6):
        return [mr.annotation(_rle(rows), k) for rows, k in HAND], tuple(k for _, k in HAND)
    return mr.case_annotations(h, w, CASE_KINDS), CASE_KINDS


_CASE = {}


def case(h, w):
    """The committed case at one size, computed once and shared: (annotations, [masks], mask_miss, mask_all).  Leave it unchanged."""
    if (h, w) not in _CASE:
        anns, kinds = case_annotations(h, w)
        masks = [sr.ann_to_mask(a["segmentation"], h, w) for a in anns]
        _CASE[(h, w)] = (anns, masks, mr.compose(masks, kinds), compose(masks, kinds))
    return _CASE[(h, w)]


def plane_ref(src, geo, gh, gw, stride, crop_x, border=0.0):
    """augment_ref.mask_ref with the border value as an argument (its own is mask_miss's 255): [gh, gw] float64 value, mag, wabs.
    With border 0 an outside cell has mag = wabs = 0, so augment_ref.ratio demands exactly 0 there."""
    i, j = np.meshgrid(np.arange(gh, dtype=np.float64), np.arange(gw, dtype=np.float64), indexing="ij")
    px = (j + 0.5) * float(stride) - 0.5
    py = (i + 0.5) * float(stride) - 0.5
    pf = float(crop_x) - px if geo["flip"] else px                # the (crop_x + 1)-wide frame flipped over its own width
    val, mag, vmax = ar._sample(src[:, :, None], geo, pf, py, float(border))
    return val[..., 0] / 255.0, mag[..., 0] / 255.0, vmax[..., 0] / 255.0


# ====================================================================================================== the loss
# Definition (the issue's, after the reference's commented-out loss2): P_j prediction j of the five, M the [B, H, W] target,
#   seg_j = mean_{b,y,x} (P_j[b,y,x,18] - M[b,y,x])^2 / 100 for every level with a nineteenth channel (C_j >= 19), else 0;
#   total = heat-map total + sum_j seg_j;   d total / d P_j[.., 18] = gs * 2 * (P - M) / (100 * B*H*W).
# Bounds, derived as loss_ref derives the heat term's (u = 2^-24; the operation chain is the same with one operand less):
#   value: d = P - M is ONE rounding (loss_ref has a, b and a - b), so |delta d| <= u |d| and per = 2 |d| |d| + d^2; the summation
#          tree is mse_fwd_kernel's (16 adds per lane, the block), double after that: loss_ref.mse_loss_bound with N = 100 * npix.
#   seg total: four fp32 additions of the five; total: one more addition of the two totals.
#   gradient: d (1 rounding), ks = gs * 2 / (float)(100 npix) (the cast and the division: 2), the product (1): 4 roundings of
#          |ks d|, where loss_ref counts 5 for the heat term, which also has k * w.
LOSS_MISREADINGS = ["weighted", "norm18", "no100", "grad_without_channel"]


def seg_case(name, final19, extra=None):
    """loss_ref.mse_case(name) (or the shape ``extra`` = (B, H, W, need) under that name) with a mask_all target and, with
    ``final19``, a live nineteenth channel in the final prediction's storage.  Without it that lane keeps loss_ref's planted 1e3,
    which no output may see.  Channel 18 of level 0 loses loss_ref's planted -1e3: there it is a live value now."""
    import loss_ref as lr
    if extra is not None:
        lr.MSE_CASES[name] = extra
    try:
        case = lr.mse_case(name)
    finally:
        if extra is not None:
            del lr.MSE_CASES[name]
    r = lr.rng(len(name) * 13 + case["B"] * case["H"] * case["W"] + int(final19))
    shape = (case["B"], case["H"], case["W"])
    case["store"][0][0, 0, 0, 18] = np.float32(r.standard_normal())
    if final19:
        case["store"][4][..., 18] = r.standard_normal(shape).astype(np.float32)
    case["C"] = (19, 19, 19, 19, 19 if final19 else 18)
    # a mask as the warp gives it: mostly 0 and 1, some cells between
    m = (r.random_sample(shape) < 0.4).astype(np.float32)
    soft = r.random_sample(shape) < 0.2
    m[soft] = r.random_sample(int(soft.sum())).astype(np.float32)
    case["mask"] = m
    return case


def seg_ref(case, mis=None):
    """float64: seg[5], seg_total, total (with loss_ref.mse_ref's heat part under "heat"), max / min of channel 18 of the final,
    grads [B,H,W,C_j] with channel 18 filled, and the bound terms.  ``mis``: one modelled misreading of the seg term."""
    import loss_ref as lr
    f64 = np.float64
    heat = lr.mse_ref(case)
    npix = case["B"] * case["H"] * case["W"]
    N = npix * (18.0 if mis == "norm18" else 1.0) * (1.0 if mis == "no100" else 100.0)
    m = case["mask"].astype(f64)
    ks = f64(case["gs"]) * 2.0 / N
    ref = dict(heat=heat, seg=[], seg_b=[], grad=[], grad_terms=[])
    for j in range(5):
        C = case["C"][j]
        gr = np.zeros(case["store"][j].shape[:3] + (C,), f64)
        gr[..., :18] = heat["grad"][j][..., :18]
        terms = [(n, np.concatenate([t[..., :18], np.zeros(t.shape[:3] + (C - 18,))], -1)) for n, t in heat["grad_terms"][j]]
        has = C >= 19 or (mis == "grad_without_channel" and j == 4)
        if not has:
            ref["seg"].append(0.0)
            ref["seg_b"].append((0.0, 0.0, N, 0.0))
        else:
            p = case["store"][j][..., 18].astype(f64)
            d = p - m
            if mis == "weighted":
                d = d * case["w"][..., 0].astype(f64)
            L = (d * d).sum() / N
            ref["seg"].append(L if C >= 19 else 0.0)
            ref["seg_b"].append((3.0 * (d * d).sum(), (d * d).sum(), N, L))
            if C >= 19:
                gr[..., 18] = ks * d * (case["w"][..., 0].astype(f64) if mis == "weighted" else 1.0)
                t4 = np.zeros_like(gr)
                t4[..., 18] = np.abs(gr[..., 18])
                terms = terms + [(4, t4)]
            else:                                   # the misreading writes where there is no channel: reported, not stored
                ref["stray"] = ks * d
        ref["grad"].append(gr)
        ref["grad_terms"].append(terms)
    ref["seg_total"] = sum(ref["seg"])
    ref["total"] = heat["total"] + ref["seg_total"]
    if case["C"][4] >= 19:
        p4 = case["store"][4][..., 18]
        ref["max_mask"], ref["min_mask"] = p4.max(), p4.min()
    else:
        ref["max_mask"], ref["min_mask"] = 0.0, 0.0
    return ref


def seg_torch_ref(case):
    """The same numbers from torch float64 autograd over sum(heat) + sum(seg): (total, [grad per level, [B,H,W,C_j]])."""
    import torch
    w, g, m = (torch.from_numpy(case[k].astype(np.float64)) for k in ("w", "gt", "mask"))
    ps = [torch.from_numpy(s[..., :C].astype(np.float64)).requires_grad_(True) for s, C in zip(case["store"], case["C"])]
    total = 0.0
    for p in ps:
        total = total + ((p[..., :18] * w - w * g) ** 2).mean()
        if p.shape[-1] >= 19:
            total = total + ((p[..., 18] - m) ** 2).mean() / 100.0
    (total * float(case["gs"])).backward()
    return float(total.detach()), [p.grad.numpy() for p in ps]


def check_seg_out(tag, out, ref, levels, route=""):
    """out: the kernel's [>= 17] vector.  [0..7] go through loss_ref.check_mse_out; the rest under the bounds stated above."""
    import loss_ref as lr
    out = np.asarray(out, dtype=np.float64).reshape(-1)
    w = lr.check_mse_out(tag, out[:8], ref["heat"], levels, route)
    bs = [lr.mse_loss_bound(*b, levels=levels) if b[1] else 0.0 for b in ref["seg_b"]]
    w = max(w, lr.chk(tag + " five seg losses", out[8:13], np.array(ref["seg"]), [], extra_abs=np.array(bs), route=route, names="j"))
    w = max(w, lr.chk(tag + " seg total", out[13], ref["seg_total"], [(4, sum(abs(x) for x in ref["seg"]))], extra_abs=sum(bs), route=route))
    hb = sum(lr.mse_loss_bound(*b, levels=levels) for b in ref["heat"]["loss_b"])
    mags = sum(abs(x) for x in ref["heat"]["loss"]) + sum(abs(x) for x in ref["seg"])
    w = max(w, lr.chk(tag + " total", out[16], ref["total"], [(5, mags)], extra_abs=sum(bs) + hb, route=route))
    lr.same(tag + " max / min of channel 18 of the final prediction", out[14:16].astype(np.float32),
            np.array([ref["max_mask"], ref["min_mask"]], np.float32), route)
    return w


def check_seg_grads(tag, grads, ref, need, route=""):
    import loss_ref as lr
    w = 0.0
    for j in range(5):
        if not need[j]:
            assert grads[j] is None
            continue
        g = np.asarray(grads[j], dtype=np.float64)
        w = max(w, lr.chk("%s d/d pred %d" % (tag, j), g, ref["grad"][j], ref["grad_terms"][j], route=route, names="bhwc"))
    return w
