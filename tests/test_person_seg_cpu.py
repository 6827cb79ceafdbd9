"""CPU tests of the person-segmentation target ``mask_all``: its rule and the restatement tests/person_seg_ref.py, the two-plane
packer of datasets/segm.py, ``DeviceAugmenter(mask_all=True)``'s refusals, and the C ABI of mpn_segm_person_masks and
mpn_augment_plane (header, library, ctypes table, refusals before any HIP call).

The rule is integer-valued: every mask comparison is byte for byte.  The committed inputs (person_seg_ref.case: the hand-written
5 x 6 case and the seven instances of tests/segm_cases.py with kinds K C N C K K N) must reject every modelled misreading at every
size, and the warp's reference must tell an outside value of 255 from 0.

The loss (section 7): the float64 reference of the seg term (person_seg_ref.seg_ref, against torch float64 autograd and a
hand-computed 2 x 2 case), four modelled misreadings it must reject on the committed loss cases, the C ABI of the seg-aware
forward / backward entry points and of mpn_step_log_seg, build_loss's refusals and the recorded step's log names.
"""
import ctypes
import os
import random
import re
import subprocess

import numpy as np
import pytest
import torch

import augment_ref as ar
import mask_miss_ref as mr
import person_seg_ref as pr
import segm_cases as sc

K, N, C = mr.K, mr.N, mr.C
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rows(m):
    return ["".join("1" if v == 255 else ("0" if v == 0 else "?") for v in row) for row in m]


# ---- 1. the rule on hand-checkable 5 x 6 cases ---------------------------------------------------------------------------------------

def test_mask_all_rule_on_hand_checkable_cases():
    (person, _), (crowd, _), (nokp, _), (late, _) = pr.HAND
    ann = lambda rows, kind: mr.annotation(pr._rle(rows), kind)
    # a crowd alone is part of mask_all (it is what mask_miss takes OUT of the heat-map loss)
    assert _rows(pr.mask_all([ann(crowd, C)], 5, 6)) == ["000000", "000000", "001111", "001111", "001111"]
    # a crowd over a person: the union, whichever comes first
    both = ["000000", "011100", "011111", "011111", "001111"]
    assert _rows(pr.mask_all([ann(person, K), ann(crowd, C)], 5, 6)) == both
    assert _rows(pr.mask_all([ann(crowd, C), ann(person, K)], 5, 6)) == both
    # a person without keypoints is a person
    assert _rows(pr.mask_all([ann(nokp, N)], 5, 6)) == ["110000", "110000", "000000", "000000", "000000"]
    # nobody: all 0 (mask_miss of the same list is all 255)
    assert _rows(pr.mask_all([], 5, 6)) == ["000000"] * 5 and _rows(mr.mask_miss([], 5, 6)) == ["111111"] * 5
    # people listed after the last crowd count, in every order
    full = ["110011", "111100", "011111", "011111", "001111"]
    anns = [ann(r, k) for r, k in pr.HAND]
    for order in ([0, 1, 2, 3], [3, 2, 1, 0], [1, 3, 0, 2]):
        assert _rows(pr.mask_all([anns[i] for i in order], 5, 6)) == full
    got = pr.mask_all(anns, 5, 6)
    assert got.dtype == np.uint8 and set(np.unique(got).tolist()) == {0, 255}
    assert pr.case(5, 6)[3].tolist() == got.tolist()


# ---- 2. the sequential restatement against the closed form ---------------------------------------------------------------------------

@pytest.mark.parametrize("h,w", pr.SIZES)
def test_sequential_restatement_equals_the_or_of_all_masks(h, w):
    anns, masks, miss, want = pr.case(h, w)
    kinds = [mr.kind_of(a) for a in anns]
    assert np.array_equal(pr.closed_form(masks), want) and np.array_equal(pr.mask_all(anns, h, w), want)
    assert np.array_equal(mr.mask_miss(anns, h, w), miss)
    assert set(np.unique(want).tolist()) == {0, 255}
    rng = random.Random(h * 1000 + w)
    for _ in range(4):                                                  # order and kinds do not matter
        order = list(range(len(masks)))
        rng.shuffle(order)
        assert np.array_equal(pr.compose([masks[i] for i in order], [rng.choice([K, N, C]) for _ in order]), want)
    # wherever mask_miss is 0 somebody stands: mask_miss takes out only cells that mask_all holds
    assert np.all(want[miss == 0] == 255)


# ---- 3. modelled misreadings of the masks and of the warp ----------------------------------------------------------------------------

@pytest.mark.parametrize("h,w", pr.SIZES)
def test_committed_inputs_reject_every_misreading(h, w):
    anns, masks, _, want = pr.case(h, w)
    kinds = [mr.kind_of(a) for a in anns]
    for mis in pr.MISREADINGS:
        got = pr.compose(masks, kinds, mis)
        n = int((got != want).sum())
        print("%d x %d %s: %d cells differ" % (h, w, mis, n))
        assert n > 0, mis
    # the warp: a crop that leaves the image on the left and at the top (identity geometry, origin (-8, -8), stride 4)
    geo = ar.geometry([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]], 1.0, (h, w), (h, w), (-8, -8), False)
    g = (max(h, w) + 16 + 3) // 4
    v0, m0, w0 = pr.plane_ref(want, geo, g, g, 4, g * 4, border=0.0)
    v255 = pr.plane_ref(want, geo, g, g, 4, g * 4, border=255.0)[0]
    outside = pr.plane_ref(np.full_like(want, 7), geo, g, g, 4, g * 4)[2] == 0        # a constant source: no tap only outside
    assert outside[:2, :].all() and outside[:, :2].all() and not outside.all()
    assert np.all(v0[outside] == 0.0) and np.all(m0[outside] == 0.0) and np.all(v255[outside] == 1.0)
    r = ar.ratio(v255, v0, m0, w0, ar.C_SUM_MASK)
    assert np.isinf(r[outside]).all() and np.array_equal(v0[~outside], v255[~outside])
    # augment_ref.mask_ref is this function at border 255
    assert np.array_equal(ar.mask_ref(want, geo, g, g, 4, g * 4)[0], v255)


# ---- 4. the packer --------------------------------------------------------------------------------------------------------------------

def test_two_plane_pack_keeps_every_annotation_and_pack_mask_miss_still_drops():
    from multiposenet.pytorch_amd._lib import MpnError
    from multiposenet.pytorch_amd.datasets import segm
    h, w = 37, 53
    segms = sc.segmentations(h, w)[0]
    anns = [mr.annotation(segms[i], k) for i, k in zip([0, 1, 4, 3, 2, 1, 0], [K, N, C, K, N, K, K])]
    pack, kinds = segm.pack_mask_miss(anns, h, w)
    assert pack.n == 4 and kinds.tolist() == [0, 1, 2, 1]                                # as before: the K's after the crowd go
    pack, kinds = segm.pack_mask_miss(anns, h, w, keep_all=True)
    want = segm.pack_segmentations([a["segmentation"] for a in anns], h, w)
    assert pack.n == 7 and kinds.dtype == np.int32 and kinds.tolist() == [0, 1, 2, 0, 1, 0, 0]
    for a, b in zip((pack.insts, pack.parts, pack.verts, pack.vpart, pack.estart, pack.toggles),
                    (want.insts, want.parts, want.verts, want.vpart, want.estart, want.toggles)):
        assert np.array_equal(a, b)
    # no crowd at all: mask_miss needs the N only, mask_all everyone
    people = [mr.annotation(segms[i], k) for i, k in zip(range(4), [K, N, K, K])]
    assert segm.pack_mask_miss(people, h, w)[0].n == 1 and segm.pack_mask_miss(people, h, w, keep_all=True)[0].n == 4
    # a kept annotation is looked at: what pack_mask_miss never reads is refused here
    bad_part = [[1.0, 2.0, 3.0, 4.0]]
    late_bad = [mr.annotation(segms[4], C), mr.annotation(bad_part, K)]
    assert segm.pack_mask_miss(late_bad, h, w)[0].n == 1
    with pytest.raises(MpnError):
        segm.pack_mask_miss(late_bad, h, w, keep_all=True)
    assert segm.pack_mask_miss(late_bad, h, w, strict=False, keep_all=True)[0].n == 2     # the instance stays, without the part
    for bad in ([{"segmentation": segms[0], "iscrowd": 0}], [{"iscrowd": 1}], [mr.annotation("polygon", K)],
                [mr.annotation({"size": [h, w], "counts": [3, 4]}, C)]):
        with pytest.raises(MpnError):
            segm.pack_mask_miss(bad, h, w, keep_all=True)
    # the batch form: the image table counts every annotation
    sizes = [(37, 53), (5, 6), (64, 65)]
    lists = [pr.case(37, 53)[0], [], pr.case(64, 65)[0][:5]]
    pack, kinds, imgs, offsets, nbytes = segm.pack_mask_miss_batch(lists, sizes, keep_all=True)
    assert imgs[:, 2:4].tolist() == [[0, 7], [7, 7], [7, 12]] and pack.n == 12
    assert kinds.tolist() == [0, 2, 1, 2, 0, 0, 1, 0, 2, 1, 2, 0]
    dropped = segm.pack_mask_miss_batch(lists, sizes)
    assert dropped[0].n == 9 and dropped[3] == offsets and dropped[4] == nbytes           # K K after the last crowd, K after it
    if not torch.cuda.is_available():                                                    # no CPU path
        with pytest.raises(MpnError):
            segm.person_masks_batch(lists, sizes)
        with pytest.raises(MpnError):
            segm.mask_all_from_annotations(lists[0], 37, 53)


# ---- 5. the augmenter's refusals -------------------------------------------------------------------------------------------------------

def _sample(h, w, **extra):
    s = {"img": torch.zeros((h, w, 3), dtype=torch.uint8), "objpos": (0.5 * w, 0.5 * h), "scale_provided": 0.6,
         "joint_self": np.ones((17, 3))}
    s.update(extra)
    return s


def test_mask_all_augmenter_refusals_leave_the_rng_untouched():
    from multiposenet.pytorch_amd._lib import MpnError
    from multiposenet.pytorch_amd.datasets.augment import DeviceAugmenter
    da = DeviceAugmenter(64, 4, dict(center_perterb_max=4), mask_all=True)
    plain = DeviceAugmenter(64, 4, dict(center_perterb_max=4))
    assert da.mask_all is True and plain.mask_all is False and DeviceAugmenter(64, 4).params["center_perterb_max"] == 40
    anns = pr.case(37, 53)[0]
    miss = torch.full((37, 53), 255, dtype=torch.uint8)
    every = torch.zeros((37, 53), dtype=torch.uint8)
    good_a, good_p = _sample(37, 53, person_anns=anns), _sample(37, 53, mask_miss=miss, mask_all=every)
    rng = random.Random(11)
    state = rng.getstate()
    for batch in ([_sample(37, 53)],                                                        # image only
                  [_sample(37, 53, mask_miss=miss)],                                        # no mask_all plane
                  [good_p, _sample(37, 53, mask_miss=miss)],
                  [_sample(37, 53, mask_miss=miss, mask_all=torch.zeros((53, 37), dtype=torch.uint8))],
                  [_sample(37, 53, mask_miss=miss, mask_all=torch.zeros((37, 53, 1), dtype=torch.uint8))],
                  [_sample(37, 53, mask_miss=miss, mask_all=torch.zeros((37, 53), dtype=torch.float32))],
                  [_sample(37, 53, mask_miss=miss, mask_all=np.zeros((37, 53), dtype=np.uint8))],
                  [_sample(37, 53, mask_miss=miss, mask_all=torch.zeros((37, 106), dtype=torch.uint8)[:, ::2])],
                  [good_a, good_p]):
        with pytest.raises(MpnError):
            da.geometry(batch, rng=rng)
        assert rng.getstate() == state
    # the same dice give the same geometry on either source, with or without mask_all
    dice = np.array([[0.2, 0.9, 0.8, 0.4, 0.6, 0.9]])
    ga, gp, g0 = da.geometry([good_a], dice=dice)[0], da.geometry([good_p], dice=dice)[0], plain.geometry([good_a], dice=dice)[0]
    for k in ("ox", "oy", "flip", "nW", "nH", "scale"):
        assert ga[k] == gp[k] == g0[k]
    assert plain.geometry([_sample(37, 53, mask_miss=miss)], dice=dice)[0]["ox"] == ga["ox"]     # mask_all=False asks for no plane
    if not torch.cuda.is_available():
        with pytest.raises(MpnError):
            da([good_a], dice=dice)


# ---- 6. the C ABI ----------------------------------------------------------------------------------------------------------------------

NEW = {"mpn_segm_person_masks": 22, "mpn_augment_plane": 11}


def test_new_symbols_in_header_library_and_ctypes_table_and_old_signatures_unchanged():
    from multiposenet.pytorch_amd import _lib
    _lib.build()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mpn.h")).read(), flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    exported = set(l.split()[-1] for l in out.splitlines() if " T mpn_" in l)
    for name, nargs in NEW.items():
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, src)
        assert decl and name in exported and name in _lib.SIGNATURES, name
        assert len(decl.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name][1]), name
        assert _lib.SIGNATURES[name][0] is ctypes.c_int
    i, i64, vp, f = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_float
    assert _lib.SIGNATURES["mpn_segm_mask_miss"] == (i, [vp, i, vp, vp, i, vp, i, vp, vp, vp, i, i64, vp, i, i, i, vp, i64, vp, i64, vp])
    assert _lib.SIGNATURES["mpn_augment_mask"] == (i, [vp, i64, vp, i, vp, i, i, i, i, vp])
    miss, both = _lib.SIGNATURES["mpn_segm_mask_miss"][1], _lib.SIGNATURES["mpn_segm_person_masks"][1]
    assert both == miss[:17] + [vp] + miss[17:]                              # mask_miss's arguments plus the second buffer
    assert _lib.SIGNATURES["mpn_augment_plane"][1] == _lib.SIGNATURES["mpn_augment_mask"][1][:9] + [f, vp]
    for name in ("mpn_segm_mask_miss", "mpn_augment_mask"):
        assert len(re.search(r"\b%s\s*\(([^)]*)\)" % name, src).group(1).split(",")) == len(_lib.SIGNATURES[name][1])


def test_new_entry_points_reject_bad_arguments_before_any_hip_call():
    from multiposenet.pytorch_amd import _lib
    L = _lib.lib()
    BAD = int(re.search(r"#define\s+MPN_E_BADARG\s+\(?(-?\d+)\)?", open(os.path.join(ROOT, "include", "mpn.h")).read()).group(1))
    one, two, odd, odd4, nul = (ctypes.c_void_p(v) for v in (0x1000, 0x3000, 0x1004, 0x1002, None))
    good = dict(imgs=one, n_img=1, insts=one, kind=one, n_inst=1, parts=one, n_parts=1, verts=one, vpart=one, estart=one, n_verts=3,
                n_steps=10, toggles=one, n_tog=2, max_w=64, max_h=64, out=one, out_all=two, out_bytes=4096, ws=one, ws_bytes=64)

    def masks(**kw):
        a = dict(good, **kw)
        return L.mpn_segm_person_masks(a["imgs"], a["n_img"], a["insts"], a["kind"], a["n_inst"], a["parts"], a["n_parts"], a["verts"],
                                       a["vpart"], a["estart"], a["n_verts"], a["n_steps"], a["toggles"], a["n_tog"], a["max_w"],
                                       a["max_h"], a["out"], a["out_all"], a["out_bytes"], a["ws"], a["ws_bytes"], nul)

    for kw in (dict(imgs=nul), dict(insts=nul), dict(kind=nul), dict(parts=nul), dict(verts=nul), dict(vpart=nul), dict(estart=nul),
               dict(toggles=nul), dict(out=nul), dict(out_all=nul), dict(out_all=one), dict(ws=nul),
               dict(n_img=0), dict(n_img=-1), dict(n_img=65536), dict(n_inst=-1), dict(n_inst=65536), dict(n_parts=-1), dict(n_verts=-1),
               dict(n_tog=-1), dict(n_steps=-1), dict(n_steps=2 ** 31), dict(n_verts=0, n_steps=5),
               dict(max_w=0), dict(max_w=65537), dict(max_h=0), dict(max_h=65537), dict(out_bytes=0), dict(out_bytes=2 ** 40 + 1),
               dict(ws_bytes=0), dict(ws_bytes=12), dict(ws_bytes=8 * 2 ** 31),
               dict(imgs=odd), dict(insts=odd), dict(parts=odd), dict(ws=odd), dict(kind=odd4), dict(verts=odd4), dict(vpart=odd4),
               dict(estart=odd4), dict(toggles=odd4)):
        assert masks(**kw) == BAD, kw

    def plane(**k):
        return L.mpn_augment_plane(*[k.get(n, d) for n, d in (("src", one), ("bytes", 4096), ("table", one), ("B", 2), ("out", one), ("gh", 16),
                                                              ("gw", 16), ("stride", 4), ("cx", 64), ("outside", 0.0), ("stream", nul))])

    for kw in (dict(src=nul), dict(table=nul), dict(out=nul), dict(bytes=0), dict(bytes=-1), dict(B=0), dict(B=-3), dict(B=65536),
               dict(gh=0), dict(gw=0), dict(gh=-1), dict(gh=65536, gw=65536), dict(stride=0), dict(stride=-4), dict(cx=0), dict(cx=-64),
               dict(outside=-1.0), dict(outside=256.0), dict(outside=float("nan")), dict(table=odd), dict(out=odd4)):
        assert plane(**kw) == BAD, kw


# ---- 7. the loss: its float64 reference, a hand-computed case, modelled misreadings, the new entry points ------------------------------

import loss_ref as lr

LOSS_CASES = [(name, f19, None) for name in ("1px", "227px last partial chunk", "228px second chunk of 8") for f19 in (False, True)] \
    + [("2x10x14 sides no multiple of 8", True, (2, 10, 14, [True] * 5))]


def test_float64_loss_reference_on_a_hand_computed_case():
    """B = 1, 2 x 2 pixels.  Heat term: level 0 predicts 1 in channel 0 of pixel (0, 0), everything else 0, weights 1, targets 0:
    1 / (4 * 18).  Seg term, M = [[0, 0], [0, 1]]: level 0 predicts [[1, 0], [0, 0]] (two cells off by 1: mean 1/2, / 100 = 0.005),
    levels 1..3 predict M (0), the 19-channel final predicts 2 M (one cell off by 1: 1/4 / 100 = 0.0025)."""
    M = np.array([[[0.0, 0.0], [0.0, 1.0]]], np.float32)
    store = [np.zeros((1, 2, 2, 19), np.float32) for _ in range(5)]
    store[0][0, 0, 0, 0] = 1.0
    store[0][0, :, :, 18] = [[1.0, 0.0], [0.0, 0.0]]
    for j in (1, 2, 3):
        store[j][..., 18] = M
    store[4][..., 18] = 2 * M
    case = dict(B=1, H=2, W=2, store=store, gt=np.zeros((1, 2, 2, 18), np.float32), w=np.ones((1, 2, 2, 18), np.float32), mask=M,
                gs=np.float32(1.0), C=(19,) * 5)
    want = 1.0 / 72 + 0.005 + 0.0025
    total, grads = pr.seg_torch_ref(case)
    ref = pr.seg_ref(case)
    assert abs(total - want) < 1e-15 and abs(ref["total"] - want) < 1e-15
    assert np.allclose(ref["seg"], [0.005, 0, 0, 0, 0.0025], rtol=0, atol=1e-17) and abs(ref["seg_total"] - 0.0075) < 1e-17
    assert (ref["max_mask"], ref["min_mask"]) == (2.0, 0.0)
    hand = [np.zeros((1, 2, 2, 19)) for _ in range(5)]
    hand[0][0, 0, 0, 0] = 2.0 / 72
    hand[0][0, 0, 0, 18], hand[0][0, 1, 1, 18] = 2.0 / 400, -2.0 / 400
    hand[4][0, 1, 1, 18] = 2.0 / 400
    for j in range(5):
        assert np.allclose(grads[j], hand[j], rtol=0, atol=1e-17) and np.allclose(ref["grad"][j], hand[j], rtol=0, atol=1e-17), j
    # an 18-channel final: its term and its gradient are gone, nothing else moves
    case18 = dict(case, C=(19, 19, 19, 19, 18))
    total18, grads18 = pr.seg_torch_ref(case18)
    assert abs(total18 - (want - 0.0025)) < 1e-15 and grads18[4].shape[-1] == 18 and not grads18[4].any()
    assert abs(pr.seg_ref(case18)["total"] - total18) < 1e-15 and pr.seg_ref(case18)["max_mask"] == 0.0


@pytest.mark.parametrize("name,final19,extra", LOSS_CASES)
def test_loss_reference_agrees_with_autograd_and_rejects_every_misreading(name, final19, extra):
    case = pr.seg_case(name, final19, extra)
    ref = pr.seg_ref(case)
    total, grads = pr.seg_torch_ref(case)
    assert abs(total - ref["total"]) <= 1e-13 * abs(total)
    for j in range(5):
        assert grads[j].shape == ref["grad"][j].shape and np.abs(grads[j] - ref["grad"][j]).max() <= 1e-15
        assert grads[j].shape[-1] == case["C"][j] and (case["C"][j] == 18 or (ref["grad"][j][..., 18] != 0).any())
    # what the GPU test allows the total to be off by
    bound = sum(lr.mse_loss_bound(*b, levels=lr.MSE_FWD_LEVELS) for b in ref["heat"]["loss_b"] + [b for b in ref["seg_b"] if b[1]]) \
        + 6 * lr.U * abs(ref["total"])
    for mis in pr.LOSS_MISREADINGS[:3]:
        bad = pr.seg_ref(case, mis)
        off = abs(bad["total"] - ref["total"])
        goff = max(np.abs(a - b).max() for a, b in zip(bad["grad"], ref["grad"]))
        print("%s final19=%s %s: total off by %.3e (bound %.3e), a gradient by %.3e" % (name, final19, mis, off, bound, goff))
        assert off > 10 * bound and goff > 0, mis
        assert all(np.array_equal(a[..., :18], b[..., :18]) for a, b in zip(bad["grad"], ref["grad"]))   # the heat term is untouched
    stray = pr.seg_ref(case, "grad_without_channel")
    if final19:
        assert "stray" not in stray                                  # every level has the channel: nothing to misread
    else:
        # the final prediction has 18 channels: the reference has no element to hold a seg gradient, and the planted lane would give one
        assert ref["grad"][4].shape[-1] == 18 and ref["seg"][4] == 0.0 and np.abs(stray["stray"]).min() > 0
        assert ref["max_mask"] == 0.0 and ref["min_mask"] == 0.0


def test_loss_symbols_and_refusals_before_any_hip_call():
    from multiposenet.pytorch_amd import _lib
    L = _lib.lib()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mpn.h")).read(), flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    exported = set(l.split()[-1] for l in out.splitlines() if " T mpn_" in l)
    for name, nargs in (("mpn_mse_seg_chunks", 1), ("mpn_mse_heatmap_seg_forward", 13), ("mpn_mse_heatmap_seg_backward", 11)):
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, src)
        assert decl and name in exported and len(decl.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name][1]), name
    i, i64, vp = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    assert _lib.SIGNATURES["mpn_mse_heatmap_forward"] == (i, [vp, vp, vp, vp, i64, vp, i, vp, vp])
    assert _lib.SIGNATURES["mpn_mse_heatmap_backward"] == (i, [vp, vp, vp, vp, vp, vp, vp, i64, vp, vp])
    assert int(re.search(r"#define\s+MPN_MSE_SEG_OUT\s+(\d+)", src).group(1)) == 20
    from multiposenet.pytorch_amd.network import losses
    assert losses.SEG_OUT == 20
    assert [L.mpn_mse_seg_chunks(n) for n in (1, 4096, 4097)] == [1, 1, 2] and L.mpn_mse_chunks(228) == 2
    BAD = int(re.search(r"#define\s+MPN_E_BADARG\s+\(?(-?\d+)\)?", open(os.path.join(ROOT, "include", "mpn.h")).read()).group(1))
    one, odd, nul = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1002), ctypes.c_void_p(None)
    p5 = lambda v: (ctypes.c_void_p * 5)(*([v] * 5))
    s5 = lambda v: (ctypes.c_int64 * 5)(*([v] * 5))
    c5 = lambda *v: (ctypes.c_int32 * 5)(*v)
    good = dict(preds=p5(0x1000), sP=s5(32), C=c5(19, 19, 19, 19, 18), gt=one, wgt=one, mask=one, npix=228, part=one, chunks=2, spart=one,
                schunks=1, out=one)

    def fwd(**kw):
        a = dict(good, **kw)
        return L.mpn_mse_heatmap_seg_forward(a["preds"], a["sP"], a["C"], a["gt"], a["wgt"], a["mask"], a["npix"], a["part"], a["chunks"],
                                             a["spart"], a["schunks"], a["out"], nul)

    for kw in (dict(preds=None), dict(sP=None), dict(C=None), dict(gt=nul), dict(wgt=nul), dict(mask=nul), dict(part=nul), dict(spart=nul),
               dict(out=nul), dict(npix=0), dict(npix=-5), dict(npix=2 ** 31), dict(chunks=1), dict(chunks=3), dict(schunks=0), dict(schunks=2),
               dict(preds=p5(None)), dict(preds=p5(0x1002)), dict(C=c5(19, 19, 19, 19, 17)), dict(C=c5(33, 19, 19, 19, 18)), dict(sP=s5(18)),
               dict(gt=odd), dict(wgt=odd), dict(mask=odd), dict(part=odd), dict(spart=odd), dict(out=odd)):
        assert fwd(**kw) == BAD, kw
    goodb = dict(preds=p5(0x1000), d=p5(0x2000), sP=s5(32), dsP=s5(19), C=c5(19, 19, 19, 19, 18), gt=one, wgt=one, mask=one, npix=228, gs=one)

    def bwd(**kw):
        a = dict(goodb, **kw)
        return L.mpn_mse_heatmap_seg_backward(a["preds"], a["d"], a["sP"], a["dsP"], a["C"], a["gt"], a["wgt"], a["mask"], a["npix"],
                                              a["gs"], nul)

    for kw in (dict(preds=None), dict(d=None), dict(sP=None), dict(dsP=None), dict(C=None), dict(gt=nul), dict(wgt=nul), dict(mask=nul),
               dict(npix=0), dict(npix=2 ** 31), dict(preds=p5(None)), dict(preds=p5(0x1002)), dict(d=p5(0x2002)), dict(C=c5(19, 19, 19, 19, 17)),
               dict(C=c5(33, 19, 19, 19, 18)), dict(C=c5(0, 0, 0, 0, 0)), dict(sP=s5(18)), dict(dsP=s5(18)), dict(gt=odd), dict(wgt=odd),
               dict(mask=odd), dict(gs=odd)):
        assert bwd(**kw) == BAD, kw


def test_step_log_seg_symbol_refusals_and_the_recorded_step_s_log_names():
    from multiposenet.pytorch_amd import _lib
    from multiposenet.pytorch_amd.replay import ReplayedTrainStep
    L = _lib.lib()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mpn.h")).read(), flags=re.S)
    assert re.search(r"\bmpn_step_log_seg\s*\(", src) and int(re.search(r"#define\s+MPN_STEP_LOG_SEG\s+(\d+)", src).group(1)) == 21
    assert _lib.SIGNATURES["mpn_step_log_seg"] == _lib.SIGNATURES["mpn_step_log"] == (ctypes.c_int, [ctypes.c_void_p] * 4)
    one, odd, nul = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1002), ctypes.c_void_p(None)
    for args in ((nul, one, one), (one, nul, nul), (nul, nul, one), (odd, one, one), (one, odd, one), (one, one, odd)):
        assert L.mpn_step_log_seg(args[0], args[1], args[2], nul) == -2, args
    names = ReplayedTrainStep._log_names
    plain = [k for k, _ in names(True, True)]
    assert plain == ['heatmap_loss_k2', 'heatmap_loss_k3', 'heatmap_loss_k4', 'heatmap_loss_k5', 'heatmap_loss', 'max_ht', 'min_ht',
                     'total_loss', 'classification_loss', 'regression_loss']                      # as before
    assert names("seg", False) == [('heatmap_loss_k2', 0), ('seg_loss_k2', 13), ('heatmap_loss_k3', 1), ('seg_loss_k3', 14),
                                   ('heatmap_loss_k4', 2), ('seg_loss_k4', 15), ('heatmap_loss_k5', 3), ('seg_loss_k5', 16),
                                   ('heatmap_loss', 4), ('max_ht', 6), ('min_ht', 7)]
    assert names("seg19", True, True)[8:] == [('heatmap_loss', 4), ('seg_loss', 17), ('max_ht', 6), ('min_ht', 7), ('max_mask', 19),
                                              ('min_mask', 20), ('total_loss', 8), ('classification_loss', 9), ('regression_loss', 10),
                                              ('max_grad', 12)]


def test_build_keypoint_loss_refuses_a_bad_mask_all_before_any_launch():
    from multiposenet.pytorch_amd._lib import MpnError
    from multiposenet.pytorch_amd.network import losses
    from multiposenet.pytorch_amd.network.posenet import poseNet
    preds = [torch.zeros((2, 19, 4, 6)) for _ in range(4)] + [torch.zeros((2, 18, 4, 6))]
    heat, wgt = torch.zeros((2, 18, 4, 6)), torch.ones((2, 18, 4, 6))
    for bad in (torch.zeros((2, 4, 6)), torch.zeros((2, 18, 4, 6)), torch.zeros((1, 1, 4, 6)), torch.zeros((2, 1, 6, 4)), np.zeros((2, 1, 4, 6)),
                torch.zeros((2, 1, 4, 6), device="meta")):
        with pytest.raises(MpnError):
            losses.build_keypoint_loss(preds, heat, wgt, bad)
        with pytest.raises(MpnError):
            poseNet.build_loss(preds, 'keypoint_subnet', heat, wgt, bad)
        with pytest.raises(MpnError):
            poseNet.build_loss((preds, None), 'train_both', heat, wgt, None, bad)
    assert losses.build_names() == ['heatmap_loss_k2', 'seg_loss_k2', 'heatmap_loss_k3', 'seg_loss_k3', 'heatmap_loss_k4', 'seg_loss_k4',
                                    'heatmap_loss_k5', 'seg_loss_k5', 'heatmap_loss', 'seg_loss']


def test_batch_processor_passes_mask_all_through(monkeypatch):
    """batch_processor called with 3-, 4- and 5-element batches (the device moves are no-ops here: there is no GPU in this test)."""
    import inspect
    from multiposenet.pytorch_amd.training import batch_processor as bp

    class _S(object):
        pass
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    monkeypatch.setattr(torch.Tensor, "to", lambda self, *a, **k: self)
    st = _S(); st.params = _S(); st.params.gpus = [0]; st.model = _S(); st.model.training = True
    inp, heat, wgt, anno, mask = (torch.full((1,), float(i)) for i in range(5))
    st.params.subnet_name = 'keypoint_subnet'
    inputs, gts, ev = bp.batch_processor(st, (inp, heat, wgt))
    assert inputs[0][0] is inp and inputs[0][1] == 'keypoint_subnet' and len(gts) == 3 and gts[1] is heat and gts[2] is wgt and ev == []
    inputs, gts, _ = bp.batch_processor(st, (inp, heat, wgt, mask))
    assert len(gts) == 4 and gts[0] == 'keypoint_subnet' and gts[1] is heat and gts[2] is wgt and gts[3] is mask
    st.params.subnet_name = 'train_both'
    inputs, gts, _ = bp.batch_processor(st, (inp, heat, wgt, anno))
    assert len(gts) == 4 and gts[3] is anno
    inputs, gts, _ = bp.batch_processor(st, (inp, heat, wgt, anno, mask))
    assert len(gts) == 5 and gts[0] == 'train_both' and gts[1] is heat and gts[2] is wgt and gts[3] is anno and gts[4] is mask
    assert inputs[0][0] is inp and inputs[0][1] == 'train_both'
    from multiposenet.pytorch_amd.network.posenet import poseNet
    sig = inspect.signature(poseNet.__init__)
    assert sig.parameters["person_seg"].default is False and list(sig.parameters)[-1] == "person_seg"


def test_one_pass_seg_entry_point_and_overlapping_mask_buffers_are_refused():
    from multiposenet.pytorch_amd import _lib
    L = _lib.lib()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mpn.h")).read(), flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    decl = re.search(r"\bmpn_mse_heatmap_seg_train\s*\(([^)]*)\)", src)
    assert decl and " T mpn_mse_heatmap_seg_train" in out and len(decl.group(1).split(",")) == 19 == len(_lib.SIGNATURES["mpn_mse_heatmap_seg_train"][1])
    i, i64, vp = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    assert _lib.SIGNATURES["mpn_mse_heatmap_train"] == (i, [vp, vp, vp, i, vp, vp, i64, i64, i64, i, i, i, vp, vp, i, vp, vp])
    one, odd, odd4, nul = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1002), ctypes.c_void_p(0x1004), ctypes.c_void_p(None)
    p5 = lambda v: (ctypes.c_void_p * 5)(*([v] * 5))
    c5 = lambda *v: (ctypes.c_int32 * 5)(*v)
    good = dict(lv=p5(0x1000), d=p5(0x2000), Cs=c5(32, 32, 32, 32, 32), C=c5(19, 19, 19, 19, 18), dtype=1, gt=one, wgt=one, mask=one,
                sB=18 * 64, sC=64, sH=8, B=1, H=8, W=8, gs=one, part=one, blocks=1, out=one)

    def train(**kw):
        a = dict(good, **kw)
        return L.mpn_mse_heatmap_seg_train(a["lv"], a["d"], a["Cs"], a["C"], a["dtype"], a["gt"], a["wgt"], a["mask"], a["sB"], a["sC"], a["sH"],
                                           a["B"], a["H"], a["W"], a["gs"], a["part"], a["blocks"], a["out"], nul)

    for kw in (dict(lv=None), dict(d=None), dict(Cs=None), dict(C=None), dict(gt=nul), dict(wgt=nul), dict(mask=nul), dict(part=nul), dict(out=nul),
               dict(B=0), dict(H=0), dict(H=12), dict(W=4), dict(blocks=2), dict(blocks=0), dict(dtype=3), dict(dtype=-1),
               dict(lv=p5(None)), dict(d=p5(None)), dict(lv=p5(0x1002)), dict(Cs=c5(32, 32, 32, 32, 19)), dict(C=c5(19, 19, 19, 19, 17)),
               dict(C=c5(33, 19, 19, 19, 18)), dict(sH=6), dict(sC=62), dict(sB=18 * 64 + 2), dict(gt=odd4), dict(wgt=odd4), dict(mask=odd4),
               dict(mask=odd), dict(part=odd), dict(out=odd), dict(gs=odd)):
        assert train(**kw) == -2, kw
    # two plane buffers closer than out_bytes overlap
    g = dict(imgs=one, n_img=1, insts=one, kind=one, n_inst=1, parts=one, n_parts=1, verts=one, vpart=one, estart=one, n_verts=3,
             n_steps=10, toggles=one, n_tog=2, max_w=64, max_h=64, out=ctypes.c_void_p(0x10000), out_bytes=4096, ws=one, ws_bytes=64)
    for other in (0x10000, 0x10000 + 4095, 0x10000 - 4095, 0x10000 + 16):
        assert L.mpn_segm_person_masks(g["imgs"], 1, g["insts"], g["kind"], 1, g["parts"], 1, g["verts"], g["vpart"], g["estart"], 3, 10,
                                       g["toggles"], 2, 64, 64, g["out"], ctypes.c_void_p(other), 4096, g["ws"], 64, nul) == -2, hex(other)


def test_closed_form_on_the_committed_instances_at_5_by_6_too():
    """person_seg_ref.case(5, 6) is hand-written; the seven committed instances still pin the restatement to the closed form there."""
    anns = mr.case_annotations(5, 6, pr.CASE_KINDS)
    import segm_ref as sr
    masks = [sr.ann_to_mask(a["segmentation"], 5, 6) for a in anns]
    want = pr.closed_form(masks)
    assert np.array_equal(pr.compose(masks, pr.CASE_KINDS), want) and np.array_equal(pr.mask_all(anns, 5, 6), want)
    assert np.array_equal(pr.compose(masks, mr.CASE_KINDS), want) and np.array_equal(pr.compose(masks[::-1], pr.CASE_KINDS[::-1]), want)
    assert (want == 255).all()                                     # why it cannot serve the misreadings: one instance covers everything
