"""Person masks at inference, CPU tier: the numpy restatement (tests/seg_infer_ref.py) on hand-checkable cases, pinned to the already
pinned merge restatement (tests/tta_merge_ref.py), the ten modelled misreadings it must reject on the committed cases, the ON share of
those cases, and the argument validation of the three entry points (csrc/seg_infer.hip)."""
import ctypes
import os
import re

import numpy as np
import pytest

from helpers import ROOT
import seg_infer_ref as ref
import tta_merge_ref


# ---- hand-checkable -----------------------------------------------------------------------------------------------------------------------

def test_a_constant_plane_stays_constant():
    """The four cubic weights sum to 1 only up to rounding for a general fraction; 0.75 and the weights of a x4 / x(1/4) grid are
    dyadic, so the constant survives exactly."""
    q = np.full((8, 8), 0.75, dtype=np.float32)
    assert np.array_equal(ref.plane_single_ref(q, 32, 24), np.full((32, 24), 0.75, dtype=np.float32))
    maps = [np.full((16, 12, 2), 0.75, dtype=np.float32), np.full((32, 24, 2), 0.75, dtype=np.float32)]
    assert np.array_equal(ref.merge_mask_ref(maps, 32, 24), np.full((32, 24), 0.75, dtype=np.float32))


def test_a_map_of_the_square_s_own_size_is_returned_exactly():
    q = np.random.RandomState(0).uniform(-1, 1, (9, 9)).astype(np.float32)
    assert np.array_equal(ref.plane_single_ref(q, 9, 7), q[:, :7]) and np.array_equal(ref.plane_single_ref(q, 5, 9), q[:5])


def test_threshold_is_strict_and_a_nan_gives_zero():
    P = np.array([[0.5, np.nextafter(np.float32(0.5), np.float32(1)), np.nan, -np.inf, np.inf, 0.25]], dtype=np.float32)
    assert ref.mask_ref(P, 0.5).tolist() == [[0, 255, 0, 0, 255, 0]]
    assert ref.mask_ref(P, 0.5, wrong="ge").tolist() == [[255, 255, 0, 0, 255, 0]]
    assert ref.mask_ref(P, 0.5).dtype == np.uint8


def test_counts_and_summary_by_hand():
    pred = np.array([[255, 1, 0, 0], [0, 7, 0, 0]], dtype=np.uint8)
    gt = np.array([[255, 0, 255, 0], [0, 255, 0, 0]], dtype=np.uint8)
    c = ref.iou_counts_ref(pred, gt)
    assert c.tolist() == [2, 3, 3] and c.dtype == np.int64
    empty = ref.iou_counts_ref(np.zeros((3, 3), np.uint8), np.zeros((3, 3), np.uint8))
    s = ref.summary_ref([c, empty], [8, 9])
    assert s == {"iou": 2 / 4, "mean_iou": 0.5, "n_empty": 1, "precision": 2 / 3, "recall": 2 / 3, "pixel_acc": (6 + 9) / 17, "n_images": 2}
    from multiposenet.pytorch_amd.evaluate.seg_eval import summarize_counts
    assert summarize_counts(np.stack([c, empty]), [8, 9]) == s
    nobody = summarize_counts(np.stack([empty]), [9])
    assert nobody["n_empty"] == 1 and np.isnan(nobody["iou"]) and np.isnan(nobody["mean_iou"]) and nobody["pixel_acc"] == 1.0


# ---- pinned to the merge restatement -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,W,scales", ref.MERGE_CASES)
def test_merge_mask_restatement_is_channel_0_of_the_pinned_merge_restatement(H, W, scales):
    """Channels 0 and 1 of SWAP_HEAT map to themselves: a seg pair map copied into channels 0 and 18 of a 36-channel pair map must give
    merge_ref(...)[:, :, 0] bit for bit."""
    assert tta_merge_ref.SWAP_HEAT[0] == 0 and tta_merge_ref.SWAP_HEAT[1] == 1
    _, _, maps, P, _ = ref.merge_case(H, W, scales)
    rs = np.random.RandomState(9)
    wide = []
    for U in maps:
        X = rs.uniform(0, 1, U.shape[:2] + (36,)).astype(np.float32)
        X[:, :, 0], X[:, :, 18] = U[:, :, 0], U[:, :, 1]
        wide.append(X)
    assert np.array_equal(tta_merge_ref.merge_ref(wide, H, W)[:, :, 0], P)
    for wrong in ref.PLANE_MISREADINGS:
        assert np.array_equal(tta_merge_ref.merge_ref(wide, H, W, wrong=wrong)[:, :, 0], ref.merge_mask_ref(maps, H, W, wrong=wrong)), wrong


# ---- the committed cases -------------------------------------------------------------------------------------------------------------------

def test_committed_cases_have_an_on_share_between_10_and_90_percent():
    shares = [float((ref.single_case(*c)[2] != 0).mean()) for c in ref.SINGLE_CASES] + \
             [float((ref.merge_case(*c)[4] != 0).mean()) for c in ref.MERGE_CASES]
    print("ON shares: %s" % ", ".join("%.3f" % s for s in shares))
    assert all(0.10 <= s <= 0.90 for s in shares), shares
    for H, W in [(5, 6), (37, 53), (64, 65), (130, 70)]:
        pred, gt = ref.iou_case(H, W)
        assert 0.10 <= float((pred != 0).mean()) <= 0.90 and 0 < int((gt != 0).sum()) < H * W
        assert set(np.unique(pred).tolist()) >= {0, 1, 255}, "the prediction has no ON value other than 255"


def _rounding_case(wrong):
    """one_accumulator and divide_after_sum move roundings only.  A constructed table shows them (the one of
    tests/test_tta_fused_cpu.py): its first scale has the image's own size and holds 2^40 in the original pass and -2^40 in the mirrored
    one, so the two cancel exactly and what is left of the O(1) terms depends on where they were rounded.  thr is the smaller of the two
    planes' values at the first pixel where they differ: one plane is above it there, the other is not."""
    rs = np.random.RandomState(5)
    H, W = 9, 11
    maps = [rs.uniform(0.1, 1.0, (7 + s, 6 + s, 2)).astype(np.float32) for s in range(1, 5)]
    first = np.empty((H, W, 2), dtype=np.float32)
    first[:, :, 0], first[:, :, 1] = 2.0 ** 40, -2.0 ** 40
    maps = [first] + maps
    good, bad = ref.merge_mask_ref(maps, H, W), ref.merge_mask_ref(maps, H, W, wrong=wrong)
    assert not np.array_equal(good, bad), wrong
    y, x = np.argwhere(good != bad)[0]
    thr = min(good[y, x], bad[y, x])
    return ref.mask_ref(good, thr), ref.mask_ref(bad, thr)


@pytest.mark.parametrize("wrong", ref.MISREADINGS)
def test_every_modelled_misreading_changes_a_byte_or_a_count(wrong):
    changed = []
    if wrong == "grid_hw":
        for H, W, hq in ref.SINGLE_CASES:
            q, _, M = ref.single_case(H, W, hq)
            bad = ref.mask_ref(ref.plane_single_ref(q, H, W, wrong=wrong), ref.THR)
            changed.append(int((bad != M).sum()))
    elif wrong in ("one_accumulator", "divide_after_sum"):
        good, bad = _rounding_case(wrong)
        changed.append(int((good != bad).sum()))
    elif wrong == "ge":
        # P == thr is hit exactly where thr is a value of the plane
        for H, W, scales in ref.MERGE_CASES:
            qs, geo, _, P, _ = ref.merge_case(H, W, scales)
            thr = np.sort(P.ravel())[P.size // 2]
            changed.append(int((ref.chain_mask_ref(qs, geo, H, W, thr, wrong=wrong) != ref.chain_mask_ref(qs, geo, H, W, thr)).sum()))
        for H, W, hq in ref.SINGLE_CASES:
            P = ref.single_case(H, W, hq)[1]
            thr = np.sort(P.ravel())[P.size // 2]
            changed.append(int((ref.mask_ref(P, thr, wrong=wrong) != ref.mask_ref(P, thr)).sum()))
    elif wrong in ("union_sum", "on_255"):
        for H, W in [(5, 6), (37, 53), (64, 65), (130, 70)]:
            pred, gt = ref.iou_case(H, W)
            c = ref.iou_counts_ref(pred, gt)
            if wrong == "on_255":
                changed.append(int((ref.iou_counts_ref(pred, gt, wrong=wrong) != c).sum()))
            else:
                a, b = ref.summary_ref([c], [H * W]), ref.summary_ref([c], [H * W], wrong=wrong)
                changed.append(sum(1 for k in ("iou", "mean_iou", "pixel_acc") if a[k] != b[k]))
    else:
        for H, W, scales in ref.MERGE_CASES:
            qs, geo, _, _, M = ref.merge_case(H, W, scales)
            assert np.array_equal(ref.chain_mask_ref(qs, geo, H, W, ref.THR), M)
            changed.append(int((ref.chain_mask_ref(qs, geo, H, W, ref.THR, wrong=wrong) != M).sum()))
    print("%s: changed %s" % (wrong, changed))
    assert all(c > 0 for c in changed), (wrong, changed)


# ---- argument validation ---------------------------------------------------------------------------------------------------------------

def test_seg_entry_points_reject_bad_arguments_without_touching_the_gpu():
    from multiposenet.pytorch_amd import _lib
    L = _lib.lib()
    src = open(os.path.join(ROOT, "include", "mpn.h")).read()
    BAD = int(re.search(r"#define\s+MPN_E_BADARG\s+\(?(-?\d+)\)?", src).group(1))
    nul = ctypes.c_void_p(None)                                       # nothing below is dereferenced: validation fails first
    P = lambda a: ctypes.c_void_p(a)

    ok = dict(src=P(0x100000), sY=32, sX=1, Hs=32, Ws=32, n_src=3 * 19 * 1024, imgs=P(0x1000), n=3, max_w=70, max_h=130, thr=0.5,
              out=P(0x200000), out_bytes=40000, planes=P(0x300000), n_pl=40000)

    def seg_masks(**kw):
        a = dict(ok, **kw)
        return L.mpn_seg_masks(a["src"], a["sY"], a["sX"], a["Hs"], a["Ws"], a["n_src"], a["imgs"], a["n"], a["max_w"], a["max_h"], a["thr"],
                               a["out"], a["out_bytes"], a["planes"], a["n_pl"], nul)
    for bad in (dict(src=nul), dict(imgs=nul), dict(out=nul), dict(Hs=0), dict(Ws=-1), dict(sY=0), dict(sX=0), dict(n=0), dict(n=65536),
                dict(max_w=0), dict(max_h=0), dict(max_w=65537), dict(max_h=65537), dict(out_bytes=0), dict(n_src=0),
                dict(n_src=31 * 32 + 31),                              # one [32][32] map needs 31 * 32 + 31 + 1 floats
                dict(planes=nul), dict(n_pl=0),                        # a length without a buffer, a buffer without a length
                dict(imgs=P(0x1004)), dict(src=P(0x100002)), dict(planes=P(0x300001)),
                dict(out=P(0x100000 + 16)), dict(planes=P(0x200000 + 8)), dict(planes=P(0x100000 + 4 * 3 * 19 * 1024 - 4))):
        assert seg_masks(**bad) == BAD, bad
    assert seg_masks(planes=nul, n_pl=0, src=nul) == BAD               # the plane-less form validates the rest alike

    def table(n, **kw):
        t = (_lib.TtaScale * max(n, 1))()
        for s in range(max(n, 1)):
            t[s].u, t[s].rh, t[s].rw, t[s].pitch = 0x1000, 24, 34, 34 * 2
            for k, v in kw.items():
                setattr(t[s], k, v)
        return t

    def merge_mask(t, n, H=37, W=53, plane=P(0x100000), mask=P(0x200000), pitch=53):
        return L.mpn_tta_merge_mask(t, n, H, W, 0.5, plane, mask, pitch, nul)
    assert merge_mask(None, 5) == BAD and merge_mask(table(5), 5, plane=nul, mask=nul) == BAD
    assert merge_mask(table(1), 0) == BAD and merge_mask(table(9), 9) == BAD
    assert merge_mask(table(5, u=None), 5) == BAD and merge_mask(table(5, rh=0), 5) == BAD and merge_mask(table(5, rw=-3), 5) == BAD
    assert merge_mask(table(5, pitch=34 * 2 - 1), 5) == BAD
    assert merge_mask(table(5), 5, H=0) == BAD and merge_mask(table(5), 5, W=0) == BAD and merge_mask(table(5), 5, H=65537) == BAD
    assert merge_mask(table(5), 5, pitch=52) == BAD and merge_mask(table(5), 5, plane=P(0x100002)) == BAD
    assert merge_mask(table(5), 5, mask=P(0x100000 + 100)) == BAD      # the mask inside the plane

    okc = dict(pred=P(0x100000), n_pred=40000, gt=P(0x200000), n_gt=40000, imgs=P(0x1000), n=3, max_h=130, counts=P(0x300000))

    def mask_iou(**kw):
        a = dict(okc, **kw)
        return L.mpn_mask_iou(a["pred"], a["n_pred"], a["gt"], a["n_gt"], a["imgs"], a["n"], a["max_h"], a["counts"], nul)
    for bad in (dict(pred=nul), dict(gt=nul), dict(imgs=nul), dict(counts=nul), dict(n=0), dict(n=65536), dict(max_h=0), dict(max_h=65537),
                dict(n_pred=0), dict(n_gt=-1), dict(imgs=P(0x1004)), dict(counts=P(0x300004)), dict(counts=P(0x100000 + 8)),
                dict(counts=P(0x200000 - 8))):
        assert mask_iou(**bad) == BAD, bad


def test_header_states_the_column_macros_the_wrappers_use():
    src = open(os.path.join(ROOT, "include", "mpn.h")).read()
    from multiposenet.pytorch_amd.evaluate import seg_eval
    cols = dict((m.group(1), int(m.group(2))) for m in re.finditer(r"#define\s+(MPN_(?:SEGV|MIOU)_[A-Z_]+)\s+(\d+)", src))
    assert [cols["MPN_SEGV_" + k] for k in ("SRC_OFF", "D", "H", "W", "OUT_OFF", "OUT_PITCH", "PLANE_OFF", "COLS")] == list(range(8))
    assert [cols["MPN_MIOU_" + k] for k in ("H", "W", "PRED_OFF", "PRED_PITCH", "GT_OFF", "GT_PITCH", "COLS")] == list(range(7))
    assert seg_eval.MIOU_COLS == cols["MPN_MIOU_COLS"]
