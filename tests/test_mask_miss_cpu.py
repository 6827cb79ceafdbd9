"""CPU tests of the mask_miss rule and of its host side (tests/mask_miss_ref.py, datasets/segm.py: annotation_kind, pack_mask_miss,
pack_mask_miss_batch; DeviceAugmenter's ``person_anns`` checks; the C ABI's refusals).

The rule is integer-valued: every comparison here is byte for byte.  The hand-checkable cases show that the rule depends on the
annotation order; the per-pixel closed form is an independent statement of it; eight modelled misreadings must each differ from
the truth on the committed inputs (the seven instances of tests/segm_cases.py with kinds N C C K C C N) at every size the GPU
tests use.
"""
import ctypes
import random

import numpy as np
import pytest
import torch

import mask_miss_ref as mr
import segm_cases as sc
import segm_ref as sr

K, N, C = mr.K, mr.N, mr.C


def _rle(rows):
    """Rows of '0' / '1' -> an uncompressed RLE segmentation of that mask."""
    m = np.array([[int(ch) for ch in row] for row in rows], dtype=np.uint8)
    return {"size": list(m.shape), "counts": sc.mask_counts(m)}


def _rows(m):
    return ["".join("1" if v == 255 else ("0" if v == 0 else "?") for v in row) for row in m]


# ---- 1. hand-checkable cases on 5 x 6 ---------------------------------------------------------------------------------------------

PERSON = ["000000",
          "011100",
          "011100",
          "011100",
          "000000"]
CROWD = ["000000",
         "000000",
         "001111",
         "001111",
         "001111"]
NOKP = ["110000",
        "110000",
        "000000",
        "000000",
        "000000"]


def test_hand_checkable_cases_show_the_order_dependence():
    person, crowd, nokp = mr.annotation(_rle(PERSON), K), mr.annotation(_rle(CROWD), C), mr.annotation(_rle(NOKP), N)
    # the person first: the crowd loses the cells the person already covers
    assert _rows(mr.mask_miss([person, crowd], 5, 6)) == ["111111",
                                                           "111111",
                                                           "111100",
                                                           "111100",
                                                           "110000"]
    # the crowd first: nothing is covered yet, all of it is taken out
    assert _rows(mr.mask_miss([crowd, person], 5, 6)) == ["111111",
                                                           "111111",
                                                           "110000",
                                                           "110000",
                                                           "110000"]
    # a person without keypoints is taken out whole, wherever it stands; one with keypoints alone changes nothing
    for order in ([nokp, person, crowd], [person, crowd, nokp], [person, nokp, crowd]):
        assert _rows(mr.mask_miss(order, 5, 6)) == ["001111",
                                                    "001111",
                                                    "111100",
                                                    "111100",
                                                    "110000"]
    assert _rows(mr.mask_miss([person], 5, 6)) == ["111111"] * 5 and _rows(mr.mask_miss([], 5, 6)) == ["111111"] * 5
    # two crowds, a person between them: each crowd is reduced by what came BEFORE it
    crowd2 = mr.annotation(_rle(["000000", "011110", "000000", "000000", "000000"]), C)
    assert _rows(mr.mask_miss([crowd2, person, crowd], 5, 6)) == ["111111",
                                                                   "100001",
                                                                   "111100",
                                                                   "111100",
                                                                   "110000"]
    got = mr.mask_miss([person, crowd], 5, 6)
    assert got.dtype == np.uint8 and set(np.unique(got).tolist()) == {0, 255}


# ---- 2. the closed form ------------------------------------------------------------------------------------------------------------

def test_closed_form_equals_the_sequential_form():
    rng = random.Random(5)
    for h, w in mr.SIZES:
        anns, masks, want = mr.case(h, w)
        assert np.array_equal(mr.closed_form(masks, mr.CASE_KINDS), want)
        for _ in range(6 if h * w < 20000 else 2):                                     # the same masks under other kinds and orders
            order = list(range(len(masks)))
            rng.shuffle(order)
            kinds = [rng.choice([K, N, C, C]) for _ in order]
            ms = [masks[i] for i in order]
            assert np.array_equal(mr.closed_form(ms, kinds), mr.compose(ms, kinds))
    rs = np.random.RandomState(2)
    for _ in range(50):                                                                # dense random masks: every overlap pattern
        n = rs.randint(1, 7)
        ms = [rs.rand(9, 11) < 0.4 for _ in range(n)]
        kinds = [[K, N, C][rs.randint(3)] for _ in range(n)]
        assert np.array_equal(mr.closed_form(ms, kinds), mr.compose(ms, kinds))


# ---- 3. the committed inputs reject every modelled misreading at every size ---------------------------------------------------------

@pytest.mark.parametrize("h,w", mr.SIZES)
def test_committed_inputs_reject_every_misreading(h, w):
    anns, masks, want = mr.case(h, w)
    assert [mr.kind_of(a) for a in anns] == list(mr.CASE_KINDS)
    assert np.array_equal(mr.mask_miss(anns, h, w), want)
    assert set(np.unique(want).tolist()) == {0, 255}                                   # the truth holds both values
    for mis in mr.MISREADINGS:
        got = mr.compose(masks, mr.CASE_KINDS, mis)
        n = int((got != want).sum())
        print("%d x %d %s: %d cells differ" % (h, w, mis, n))
        assert n > 0, mis
        if mis in mr.MISREADINGS[:6]:
            assert n >= 7, mis


# ---- 4. the packer -----------------------------------------------------------------------------------------------------------------

def test_annotation_kind_and_the_keypoints_fallback():
    from multiposenet.pytorch_amd._lib import MpnError
    from multiposenet.pytorch_amd.datasets import segm
    assert (segm.KIND_KEYPOINTS, segm.KIND_NO_KEYPOINTS, segm.KIND_CROWD) == (0, 1, 2)
    code = {K: segm.KIND_KEYPOINTS, N: segm.KIND_NO_KEYPOINTS, C: segm.KIND_CROWD}
    anns = mr.case_annotations(37, 53)
    assert [segm.annotation_kind(a) for a in anns] == [code[k] for k in mr.CASE_KINDS]
    assert any("num_keypoints" not in a for a in anns) and any("num_keypoints" in a for a in anns)
    kp = [1.0, 2.0, 0] * 16 + [3.0, 4.0, 1]
    assert segm.annotation_kind({"keypoints": kp}) == segm.KIND_KEYPOINTS              # one v > 0; iscrowd absent = not a crowd
    assert segm.annotation_kind({"keypoints": [1.0, 2.0, 0] * 17, "iscrowd": 0}) == segm.KIND_NO_KEYPOINTS
    assert segm.annotation_kind({"num_keypoints": 0, "keypoints": kp}) == segm.KIND_NO_KEYPOINTS      # the field wins
    assert segm.annotation_kind({"num_keypoints": -1}) == segm.KIND_NO_KEYPOINTS
    assert segm.annotation_kind({"iscrowd": 1}) == segm.KIND_CROWD                     # a crowd needs neither
    assert segm.annotation_kind({"iscrowd": 1, "num_keypoints": 9}) == segm.KIND_CROWD
    with pytest.raises(MpnError):
        segm.annotation_kind({"iscrowd": 0})
    with pytest.raises(MpnError):
        segm.annotation_kind({"segmentation": []})


def test_pack_mask_miss_kinds_dropping_rule_and_refusals():
    from multiposenet.pytorch_amd._lib import MpnError
    from multiposenet.pytorch_amd.datasets import segm
    h, w = 37, 53
    segms = sc.segmentations(h, w)[0]
    # the committed case: the only K stands before the last crowd, so all seven stay
    pack, kinds = segm.pack_mask_miss(mr.case_annotations(h, w), h, w)
    assert pack.n == 7 and kinds.dtype == np.int32 and kinds.tolist() == [1, 2, 2, 0, 2, 2, 1]
    # K N C K N K K: the K's after the crowd go, the one before it stays
    anns = [mr.annotation(segms[i], k) for i, k in zip([0, 1, 4, 3, 2, 1, 0], [K, N, C, K, N, K, K])]
    pack, kinds = segm.pack_mask_miss(anns, h, w)
    want = segm.pack_segmentations([segms[0], segms[1], segms[4], segms[2]], h, w)
    assert kinds.tolist() == [0, 1, 2, 1]
    for a, b in zip((pack.insts, pack.parts, pack.verts, pack.vpart, pack.estart, pack.toggles),
                    (want.insts, want.parts, want.verts, want.vpart, want.estart, want.toggles)):
        assert np.array_equal(a, b)
    assert pack.words == want.words
    # no crowd at all: only the N's are rasterised
    pack, kinds = segm.pack_mask_miss([mr.annotation(segms[i], k) for i, k in zip(range(4), [K, N, K, K])], h, w)
    assert pack.n == 1 and kinds.tolist() == [1] and np.array_equal(pack.insts, segm.pack_segmentations([segms[1]], h, w).insts)
    # no annotation; only crowds; only people with keypoints
    pack, kinds = segm.pack_mask_miss([], h, w)
    assert pack.n == 0 and kinds.shape == (0,) and kinds.dtype == np.int32 and pack.words == 0
    pack, kinds = segm.pack_mask_miss([mr.annotation(segms[4], C), mr.annotation(segms[5], C)], h, w)
    assert pack.n == 2 and kinds.tolist() == [2, 2]
    assert segm.pack_mask_miss([mr.annotation(segms[0], K), mr.annotation(segms[3], K)], h, w)[0].n == 0
    # refusals: pack_segmentations' own, the missing fields
    bad_part = [[1.0, 2.0, 3.0, 4.0]]
    for anns in ([{"segmentation": segms[0], "iscrowd": 0}],                                       # neither num_keypoints nor keypoints
                 [{"iscrowd": 1}],                                                                 # no segmentation
                 [{"num_keypoints": 0, "iscrowd": 0, "segmentation": None}],
                 [mr.annotation(bad_part, N)],
                 [mr.annotation([[1.0, 2.0, 3.0, 4.0, 5.0, float("nan")]], N)],
                 [mr.annotation([[1.0, 2.0, 3.0, 4.0, 5.0, 2.0 ** 21]], C)],
                 [mr.annotation({"size": [h + 1, w], "counts": [h * w + w]}, C)],
                 [mr.annotation({"size": [h, w], "counts": [3, 4]}, C)],
                 [mr.annotation("polygon", N)]):
        with pytest.raises(MpnError):
            segm.pack_mask_miss(anns, h, w)
    with pytest.raises(MpnError):
        segm.pack_mask_miss([mr.annotation(segms[0], N)], 0, w)
    # a dropped annotation is never looked at: a K after the last crowd may hold anything as its segmentation
    assert segm.pack_mask_miss([mr.annotation(segms[4], C), mr.annotation(bad_part, K)], h, w)[0].n == 1
    # strict=False drops the malformed part only
    pack, kinds = segm.pack_mask_miss([mr.annotation(segms[1] + bad_part, N)], h, w, strict=False)
    assert pack.n == 1 and pack.parts.shape[0] == 2


def test_image_table_of_a_mixed_size_batch():
    from multiposenet.pytorch_amd._lib import MpnError
    from multiposenet.pytorch_amd.datasets import segm
    from multiposenet.pytorch_amd.datasets.augment import _aligned_offsets
    sizes = [(37, 53), (5, 6), (130, 70), (64, 65)]
    lists = [mr.case_annotations(37, 53), [], [mr.annotation(sc.segmentations(130, 70)[0][4], C)], mr.case_annotations(64, 65)[:3]]
    pack, kinds, imgs, offsets, nbytes = segm.pack_mask_miss_batch(lists, sizes)
    assert offsets == _aligned_offsets([h * w for h, w in sizes])[0] == [0, 1968, 2000, 11104]
    assert nbytes == 11104 + 64 * 65
    assert imgs.dtype == np.int64 and imgs.tolist() == [[37, 53, 0, 7, 0, 53], [5, 6, 7, 7, 1968, 6], [130, 70, 7, 8, 2000, 70],
                                                        [64, 65, 8, 11, 11104, 65]]
    assert pack.n == 11 and kinds.tolist() == [1, 2, 2, 0, 2, 2, 1, 2, 1, 2, 2]
    for (h, w, i0, i1, _, _) in imgs.tolist():                                         # every instance carries its image's size
        assert np.all(pack.insts[i0:i1, segm.I_H] == h) and np.all(pack.insts[i0:i1, segm.I_W] == w)
    assert np.array_equal(pack.parts[:, segm.P_INST], np.repeat(np.arange(11), np.diff(np.r_[pack.insts[:, segm.I_P0], pack.parts.shape[0]])))
    # offsets of the caller's
    _, _, imgs, offsets, nbytes = segm.pack_mask_miss_batch(lists[:2], sizes[:2], offsets=[4096, 16])
    assert imgs[:, segm.M_OUT_OFF].tolist() == [4096, 16] and offsets == [4096, 16] and nbytes == 4096 + 37 * 53
    # a batch without any annotation is a batch
    pack, kinds, imgs, _, _ = segm.pack_mask_miss_batch([[], []], sizes[:2])
    assert pack.n == 0 and kinds.shape == (0,) and imgs[:, 2:4].tolist() == [[0, 0], [0, 0]]
    for bad in (([], []), (lists[:2], sizes[:1]), (lists[:2], sizes[:2], [0]), (lists[:2], sizes[:2], [0, -16])):
        with pytest.raises(MpnError):
            segm.pack_mask_miss_batch(*bad)


# ---- 5. the augmenter's checks ------------------------------------------------------------------------------------------------------

def _sample(h, w, **extra):
    s = {"img": torch.zeros((h, w, 3), dtype=torch.uint8), "objpos": (0.5 * w, 0.5 * h), "scale_provided": 0.6,
         "joint_self": np.ones((17, 3))}
    s.update(extra)
    return s


def test_augmenter_refusals_leave_the_rng_untouched():
    from multiposenet.pytorch_amd._lib import MpnError
    from multiposenet.pytorch_amd.datasets.augment import DeviceAugmenter, mask_source
    da = DeviceAugmenter(64, 4, dict(center_perterb_max=4))
    anns = mr.case_annotations(37, 53)
    plane = torch.full((37, 53), 255, dtype=torch.uint8)
    with_anns, with_plane, bare = _sample(37, 53, person_anns=anns), _sample(37, 53, mask_miss=plane), _sample(37, 53)
    both = _sample(37, 53, person_anns=anns, mask_miss=plane)
    rng = random.Random(11)
    state = rng.getstate()
    for batch in ([both], [with_anns, both], [with_anns, with_plane], [with_plane, with_anns], [with_anns, bare], [bare, with_anns],
                  [with_plane, bare], [_sample(37, 53, person_anns=[]), bare]):
        with pytest.raises(MpnError):
            da.geometry(batch, rng=rng)
        with pytest.raises(MpnError):
            mask_source(batch)
        assert rng.getstate() == state
    assert mask_source([with_anns, _sample(5, 6, person_anns=[])]) == "person_anns"       # an empty list is a mask
    assert mask_source([with_plane]) == "mask_miss" and mask_source([bare, bare]) is None
    # person_anns selects the crop + 1 slice frame, as a mask_miss does: the same geometry from the same dice
    dice = np.array([[0.2, 0.9, 0.8, 0.4, 0.6, 0.9]])
    ga, gp = da.geometry([with_anns], dice=dice)[0], da.geometry([with_plane], dice=dice)[0]
    assert (ga["ox"], ga["oy"], ga["flip"], ga["nW"], ga["nH"]) == (gp["ox"], gp["oy"], gp["flip"], gp["nW"], gp["nH"])
    with pytest.raises(MpnError):
        da.geometry([_sample(37, 53, person_anns="anns")], dice=dice)
    # without a GPU the call itself refuses instead of falling back
    if not torch.cuda.is_available():
        from multiposenet.pytorch_amd.datasets.segm import mask_miss_batch, mask_miss_from_annotations
        with pytest.raises(MpnError):
            mask_miss_from_annotations(anns, 37, 53)
        with pytest.raises(MpnError):
            mask_miss_batch([anns], [(37, 53)])
        with pytest.raises(MpnError):
            da([with_anns], dice=dice)


# ---- 6. the C ABI's refusals (no HIP call is made, so this runs without a GPU) --------------------------------------------------------

def test_entry_point_rejects_bad_arguments_before_any_hip_call():
    from multiposenet.pytorch_amd import _lib
    L = _lib.lib()
    BAD = -2
    one, odd, odd4, nul = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1004), ctypes.c_void_p(0x1002), ctypes.c_void_p(None)
    good = dict(imgs=one, n_img=1, insts=one, kind=one, n_inst=1, parts=one, n_parts=1, verts=one, vpart=one, estart=one, n_verts=3,
                n_steps=10, toggles=one, n_tog=2, max_w=64, max_h=64, out=one, out_bytes=4096, ws=one, ws_bytes=64)

    def call(**kw):
        a = dict(good, **kw)
        return L.mpn_segm_mask_miss(a["imgs"], a["n_img"], a["insts"], a["kind"], a["n_inst"], a["parts"], a["n_parts"], a["verts"],
                                    a["vpart"], a["estart"], a["n_verts"], a["n_steps"], a["toggles"], a["n_tog"], a["max_w"],
                                    a["max_h"], a["out"], a["out_bytes"], a["ws"], a["ws_bytes"], nul)

    for kw in (dict(imgs=nul), dict(insts=nul), dict(kind=nul), dict(parts=nul), dict(verts=nul), dict(vpart=nul), dict(estart=nul),
               dict(toggles=nul), dict(out=nul), dict(ws=nul),
               dict(n_img=0), dict(n_img=-1), dict(n_img=65536), dict(n_inst=-1), dict(n_inst=65536), dict(n_parts=-1), dict(n_verts=-1),
               dict(n_tog=-1), dict(n_steps=-1), dict(n_steps=2 ** 31), dict(n_verts=0, n_steps=5),
               dict(max_w=0), dict(max_w=65537), dict(max_h=0), dict(max_h=65537), dict(out_bytes=0), dict(out_bytes=2 ** 40 + 1),
               dict(ws_bytes=0), dict(ws_bytes=12), dict(ws_bytes=8 * 2 ** 31),
               dict(imgs=odd), dict(insts=odd), dict(parts=odd), dict(ws=odd), dict(kind=odd4), dict(verts=odd4), dict(vpart=odd4),
               dict(estart=odd4), dict(toggles=odd4)):
        assert call(**kw) == BAD, kw
