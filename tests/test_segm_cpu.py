"""CPU tests of the segmentation rasteriser's rule and host side (tests/segm_ref.py, datasets/segm.py, the C ABI of csrc/segm.hip).

The rule (COCO maskApi.c: rleFrPoly, rleMerge as a union, rleDecode, rleFrString) is restated in tests/segm_ref.py, sequentially and
in two forms (sort-and-merge as the library does, and toggle parity).  Here: the hand-checkable pins, the two forms against each
other, the string decoder against an encoder, the packer's tables, its refusals and its conservative rectangles, the entry points'
refusals, and ten modelled misreadings of the rule, each of which the committed inputs (tests/segm_cases.py) must reject.
The comparison with a live pycocotools skips where that library is absent.
"""
import ctypes
import os
import random
import re

import numpy as np
import pytest

import segm_cases as sc
import segm_ref as sr
from helpers import ROOT


def _rows(m):
    return ["".join(str(int(v)) for v in row) for row in m]


# ---- 1. pins --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["sort", "parity"])
def test_hand_checkable_pins(form):
    m = sr.ann_to_mask([[10, 10, 20, 10, 20, 20, 10, 20]], 40, 50, form)
    want = np.zeros((40, 50), dtype=np.uint8)
    want[10:20, 10:20] = 1
    assert np.array_equal(m, want) and int(m.sum()) == 100
    m = sr.ann_to_mask([[1.5, 1.5, 3.5, 1.5, 3.5, 3.5, 1.5, 3.5]], 6, 6, form)
    want = np.zeros((6, 6), dtype=np.uint8)
    want[2:4, 2:4] = 1
    assert np.array_equal(m, want)
    m = sr.ann_to_mask([[2, 1, 2, 1, 5, 1, 5, 4, 5, 4, 2, 4]], 6, 7, form)            # repeated vertices
    want = np.zeros((6, 7), dtype=np.uint8)
    want[1:4, 2:5] = 1
    assert np.array_equal(m, want)
    assert sr.ann_to_mask([[-3, -3, 9, -3, 9, 9, -3, 9]], 4, 5, form).tolist() == np.ones((4, 5), dtype=np.uint8).tolist()
    assert _rows(sr.ann_to_mask([[0, 0, 4, 0, 0, 4]], 5, 6, form)) == ["111000", "110000", "100000", "000000", "000000"]


# ---- 2. the two forms -----------------------------------------------------------------------------------------------------------

def _random_part(rng, h, w, k):
    xy = []
    for _ in range(k):
        xy += [rng.choice([rng.uniform(-6, w + 6), float(rng.randint(-6, w + 6))]),
               rng.choice([rng.uniform(-6, h + 6), float(rng.randint(-6, h + 6))])]
        if rng.random() < 0.2:
            xy += xy[-2:]                                                              # a repeated vertex
    return xy


def _random_cases(n, seed, kmin=1):
    rng = random.Random(seed)
    for _ in range(n):
        h, w = rng.randint(1, 40), rng.randint(1, 40)
        yield h, w, _random_part(rng, h, w, rng.randint(kmin, 9))


def test_sort_and_merge_form_equals_parity_form():
    """Vertices up to 6 px outside every border, negative coordinates, repeated vertices, 1- and 2-vertex parts (straight to the
    restatement: the packer refuses those)."""
    small = 0
    for h, w, xy in _random_cases(1500, 11):
        small += len(xy) <= 4
        assert np.array_equal(sr.part_mask(xy, h, w, "sort"), sr.part_mask(xy, h, w, "parity")), (h, w, xy)
    assert small >= 100
    for h, w in sc.SIZES:
        for segm in sc.segmentations(h, w)[0]:
            assert np.array_equal(sr.ann_to_mask(segm, h, w, "sort"), sr.ann_to_mask(segm, h, w, "parity"))


# ---- 3. the string form ---------------------------------------------------------------------------------------------------------

def test_string_decoder_round_trip():
    from multiposenet.pytorch_amd.datasets.segm import string_counts
    rng = random.Random(4)
    for _ in range(200):
        n = rng.randint(1, 12)
        counts = [rng.choice([0, 1, 15, 16, 31, 32, 1023, 1024, rng.randint(0, 70000), rng.randint(0, 2 ** 28)]) for _ in range(n)]
        s = sc.counts_string(counts)
        assert all(48 <= ord(c) < 48 + 64 for c in s)
        assert sr.string_counts(s) == counts and sr.string_counts(s.encode("ascii")) == counts
        assert string_counts(s) == counts and string_counts(s.encode("ascii")) == counts
    # the encoder itself against a mask: its counts paint the mask back
    for h, w in sc.SIZES:
        for m in sc.segmentations(h, w)[1]:
            c = sc.mask_counts(m)
            assert sum(c) == h * w and np.array_equal(sr.decode(sr.string_counts(sc.counts_string(c)), h, w), m)
    assert sc.mask_counts(sc.segmentations(5, 6)[1][1])[0] == 0                        # the zero-length first run of case 5


# ---- 4. the packer --------------------------------------------------------------------------------------------------------------

def test_packer_tables():
    from multiposenet.pytorch_amd.datasets import segm
    from multiposenet.pytorch_amd.datasets.augment import _aligned_offsets
    h, w = 37, 53
    segms, (band, corner) = sc.segmentations(h, w)
    k = segm.pack_segmentations(segms, h, w)
    assert k.n == sc.N_INST and k.insts.dtype == np.int64 and k.parts.dtype == np.int64
    assert k.verts.dtype == k.vpart.dtype == k.estart.dtype == k.toggles.dtype == np.int32
    n_parts = [1, 2, 4, 2, 1, 1, 1]
    assert (k.insts[:, segm.I_P1] - k.insts[:, segm.I_P0]).tolist() == n_parts and k.parts.shape == (sum(n_parts), segm.P_COLS)
    assert k.insts[:, segm.I_P0].tolist() == np.cumsum([0] + n_parts[:-1]).tolist()
    assert np.all(k.insts[:, segm.I_H] == h) and np.all(k.insts[:, segm.I_W] == w)
    # vertices: (int)(5 x + 0.5), one edge per vertex, the step counts are max(|dX|, |dY|) to the next vertex of the part
    polys = [p for s in segms if not isinstance(s, dict) for p in s]
    assert k.verts.shape[0] == sum(len(p) // 2 for p in polys) and k.estart.shape[0] == k.verts.shape[0] + 1 and k.estart[0] == 0
    rows = [r for r in k.parts if r[segm.P_V1] > r[segm.P_V0]]
    assert len(rows) == len(polys)
    for r, p in zip(rows, polys):
        v0, v1 = int(r[segm.P_V0]), int(r[segm.P_V1])
        X, Y = sr.upsample(p)
        assert k.verts[v0:v1, 0].tolist() == X[:-1] and k.verts[v0:v1, 1].tolist() == Y[:-1]
        steps = [max(abs(X[j + 1] - X[j]), abs(Y[j + 1] - Y[j])) for j in range(len(X) - 1)]
        assert np.diff(k.estart[v0:v1 + 1]).tolist() == steps
        assert np.all(k.vpart[v0:v1] == np.flatnonzero((k.parts == r).all(axis=1))[0])
    assert int(k.estart[-1]) == sum(len(sr.boundary_points(*sr.upsample(p))[0]) - len(p) // 2 for p in polys)
    # RLE: the toggle list is the cumulative sums below h * w, under the RLE's own part
    for i, m in ((4, band), (5, corner)):
        p = int(k.insts[i, segm.I_P0])
        cum = np.cumsum(sc.mask_counts(m))
        assert k.toggles[k.toggles[:, 0] == p, 1].tolist() == cum[cum < h * w].tolist()
        assert tuple(k.parts[p, 1:3]) == (0, 0)
    # bitmaps: (h / 64 + 1) words per rectangle column and part, one after the other
    cw, words = h // 64 + 1, 0
    for i in range(k.n):
        for p in range(int(k.insts[i, segm.I_P0]), int(k.insts[i, segm.I_P1])):
            assert k.parts[p, segm.P_INST] == i and k.parts[p, segm.P_BM] == words
            words += cw * int(k.insts[i, segm.I_RW])
    assert k.words == words
    # layouts
    sizes = [int(r[segm.I_RW] * r[segm.I_RH]) for r in k.insts]
    offs, total = _aligned_offsets(sizes)
    assert k.packed_layout() == total and k.insts[:, segm.I_OUT_OFF].tolist() == offs
    assert k.insts[:, segm.I_OUT_PITCH].tolist() == k.insts[:, segm.I_RW].tolist()
    assert k.dense_layout() == k.n * h * w and np.all(k.insts[:, segm.I_OUT_PITCH] == w)
    assert k.insts[:, segm.I_OUT_OFF].tolist() == [i * h * w + int(r[segm.I_RY0]) * w + int(r[segm.I_RX0]) for i, r in enumerate(k.insts)]
    # a batch: indices shifted, instances in order
    k.packed_layout()
    k2 = segm.pack_segmentations(sc.segmentations(64, 65)[0][:3], 64, 65)
    both = segm.concat_packs([k, k2, segm.pack_segmentations([], 5, 6)])
    assert both.n == k.n + 3 and both.words == k.words + k2.words and both.verts.shape[0] == k.verts.shape[0] + k2.verts.shape[0]
    assert np.array_equal(both.insts[:k.n], k.insts) and both.insts[k.n:, segm.I_P0].tolist() == (k2.insts[:, segm.I_P0] + k.parts.shape[0]).tolist()
    assert both.parts[k.parts.shape[0]:, segm.P_BM].tolist() == (k2.parts[:, segm.P_BM] + k.words).tolist()
    assert np.array_equal(np.diff(both.estart), np.concatenate([np.diff(k.estart), np.diff(k2.estart)]))
    assert both.vpart[k.verts.shape[0]:].tolist() == (k2.vpart + k.parts.shape[0]).tolist()
    assert both.insts[k.n, segm.I_OUT_OFF] == total


def test_packer_refusals():
    from multiposenet.pytorch_amd._lib import MpnError
    from multiposenet.pytorch_amd.datasets.segm import pack_segmentations, string_counts
    h, w = 10, 12
    good = [[1.0, 1.0, 8.0, 1.0, 8.0, 7.0]]
    pack_segmentations([good, {"size": [h, w], "counts": [5, 10, h * w - 15]}], h, w)
    bad = [{"size": [w, h], "counts": [h * w]},                                        # another size
           {"size": [h, w], "counts": [5, 10, h * w - 16]},                            # does not sum to h * w
           {"size": [h, w], "counts": [5, 10, h * w - 14]},
           {"size": [h, w], "counts": [-1, h * w + 1]},
           {"size": [h, w], "counts": [0.5, h * w - 0.5]},
           {"size": [h, w], "counts": sc.counts_string([5, 10, h * w - 16])},          # the compressed form is checked as well
           {"size": [h, w], "counts": []},
           {"counts": [h * w]},
           [[1.0, 1.0, float("nan"), 1.0, 8.0, 7.0]],
           [[1.0, 1.0, float("inf"), 1.0, 8.0, 7.0]],
           [[1.0, 1.0, 8.0, 1.0, 8.0, 7.0, 3.0]],                                      # odd length
           [[1.0, 1.0, 8.0, 1.0]],                                                     # pycocotools would read a box
           [[1.0, 1.0]],
           [good[0], []],
           [[1.0, 1.0, 3e6, 1.0, 8.0, 7.0]],                                           # beyond +-2^20
           "abc", 7]
    for s in bad:
        with pytest.raises(MpnError):
            pack_segmentations([s], h, w)
    # strict=False drops the malformed PART and keeps the rest; numbers that are not finite still raise
    k = pack_segmentations([[good[0], [1.0, 1.0, 8.0, 1.0], [1.0, 2.0, 3.0]], [[1.0, 1.0]]], h, w, strict=False)
    assert k.n == 2 and k.parts.shape[0] == 1 and k.verts.shape[0] == 3 and tuple(k.insts[1, 2:6]) == (0, 0, 1, 1)
    with pytest.raises(MpnError):
        pack_segmentations([[[1.0, float("nan")]]], h, w, strict=False)
    for hw in ((0, 5), (5, 0), (70000, 5), (65536, 65536)):
        with pytest.raises(MpnError):
            pack_segmentations([good], *hw)
    for s in ("\x10", "o", "5~"):                                                      # below '0', an unfinished group, above 'o'
        with pytest.raises(MpnError):
            string_counts(s)


def test_conservative_rectangle_contains_every_on_cell():
    from multiposenet.pytorch_amd.datasets.segm import pack_segmentations
    checked = 0
    cases = [(h, w, [xy]) for h, w, xy in _random_cases(600, 23, kmin=3)]
    cases += [(h, w, s) for h, w in sc.SIZES for s in sc.segmentations(h, w)[0]]
    rng = random.Random(8)
    for _ in range(100):                                                               # random RLEs, some empty, some full
        h, w = rng.randint(1, 30), rng.randint(1, 30)
        cuts = sorted(rng.randint(0, h * w) for _ in range(rng.randint(0, 6)))
        cases.append((h, w, {"size": [h, w], "counts": np.diff([0] + cuts + [h * w]).tolist()}))
    for h, w, segm in cases:
        k = pack_segmentations([segm], h, w)
        x0, y0, rw, rh = k.rects()[0]
        assert 0 <= x0 and 0 <= y0 and rw >= 1 and rh >= 1 and x0 + rw <= w and y0 + rh <= h
        m = sr.ann_to_mask(segm, h, w)
        inside = np.zeros_like(m)
        inside[y0:y0 + rh, x0:x0 + rw] = 1
        assert not np.any(m & (1 - inside)), (h, w, segm)
        checked += int(m.any())
    assert checked >= 300


# ---- 5. the C ABI ---------------------------------------------------------------------------------------------------------------

def test_entry_points_exist_and_refuse_bad_arguments_before_any_hip_call():
    from multiposenet.pytorch_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mpn.h")).read(), flags=re.S)
    L = _lib.lib()
    for name in ("mpn_segm_workspace_bytes", "mpn_segm_rasterize"):
        assert re.search(r"\b%s\s*\(" % name, src) and name in _lib.SIGNATURES and getattr(L, name) is not None
    for col, v in (("MPN_SEGI_COLS", 10), ("MPN_SEGP_COLS", 4), ("MPN_SEGI_OUT_OFF", 6), ("MPN_SEGP_BM", 3)):
        assert re.search(r"#define\s+%s\s+%d\b" % (col, v), src)
    BAD = int(re.search(r"#define\s+MPN_E_BADARG\s+\(?(-?\d+)\)?", src).group(1))
    assert L.mpn_segm_workspace_bytes(0) == 8 and L.mpn_segm_workspace_bytes(100) == 800
    assert L.mpn_segm_workspace_bytes(-1) == 0 and L.mpn_segm_workspace_bytes(2 ** 31) == 0
    one, odd, nul = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1004), None            # never dereferenced: validation fails first
    good = dict(insts=one, n_inst=1, parts=one, n_parts=1, verts=one, vpart=one, estart=one, n_verts=3, n_steps=10, toggles=one, n_tog=1,
                max_rw=8, max_h=8, out=one, out_bytes=64, dense=0, any_on=one, ws=one, ws_bytes=64, stream=nul)

    def status(**kw):
        a = dict(good, **kw)
        return L.mpn_segm_rasterize(*[a[k] for k in good])
    bad = [dict(insts=nul), dict(parts=nul), dict(out=nul), dict(any_on=nul), dict(ws=nul), dict(estart=nul), dict(verts=nul), dict(vpart=nul),
           dict(toggles=nul), dict(n_inst=0), dict(n_inst=65536), dict(n_parts=-1), dict(n_verts=-1), dict(n_tog=-1), dict(n_steps=-1),
           dict(n_steps=2 ** 31), dict(n_verts=0, verts=nul, vpart=nul), dict(max_rw=0), dict(max_rw=65537), dict(max_h=0), dict(max_h=65537),
           dict(out_bytes=0), dict(out_bytes=2 ** 40 + 1), dict(dense=2), dict(ws_bytes=0), dict(ws_bytes=12), dict(ws_bytes=2 ** 34 + 8),
           dict(insts=odd), dict(parts=odd), dict(ws=odd), dict(verts=ctypes.c_void_p(0x1002)), dict(any_on=ctypes.c_void_p(0x1001))]
    for kw in bad:
        assert status(**kw) == BAD, kw


# ---- 6. live pycocotools (absent here: this leg is unpinned on a machine without it) ------------------------------------------------

def test_restatement_equals_live_pycocotools():
    mu = pytest.importorskip("pycocotools.mask")
    for h, w in sc.SIZES:
        for segm in sc.segmentations(h, w)[0]:
            if isinstance(segm, dict):
                rle = mu.frUnCompressedRLE(segm, h, w) if isinstance(segm["counts"], list) else segm
            else:
                rle = mu.merge(mu.frPyObjects(segm, h, w))
            assert np.array_equal(mu.decode(rle), sr.ann_to_mask(segm, h, w))
    for h, w, xy in _random_cases(300, 31, kmin=3):
        assert np.array_equal(mu.decode(mu.merge(mu.frPyObjects([xy], h, w))), sr.part_mask(xy, h, w))


# ---- 7. modelled misreadings ----------------------------------------------------------------------------------------------------

MISREADINGS = ["round", "scale4", "clamp_h1", "floor", "clamp_col", "row_major", "rising_u", "xor_parts", "no_cancel", "first_on"]


@pytest.mark.parametrize("mis", MISREADINGS)
def test_committed_inputs_reject_each_modelled_misreading(mis):
    """Each misreading of the rule, built into the restatement as a switch, must change a mask of the committed inputs — otherwise
    a kernel that makes this mistake would pass tests/test_segm_gpu.py."""
    hit = []
    for h, w in sc.SIZES:
        for i, segm in enumerate(sc.segmentations(h, w)[0]):
            if not np.array_equal(sr.ann_to_mask(segm, h, w), sr.ann_to_mask(segm, h, w, mis=mis)):
                hit.append((h, w, i))
    print("%s rejected by %s" % (mis, hit))
    assert hit, "no committed input tells '%s' from the rule" % mis
