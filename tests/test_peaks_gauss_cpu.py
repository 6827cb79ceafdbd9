"""CPU side of the smoothed peak refinement (NMS(..., bool_gaussian_filt=True)); no GPU needed.

1. tests/peaks_gauss_ref.py's restatement of scipy.ndimage.gaussian_filter (float32 array, sigma 3) equals the LIVE scipy function
   bit for bit, and equals what the reference's own NMS recorded in tests/golden/g20_peaks_gauss.npz (patches and result rows).
2. The product's weights (datasets/prn_data.py: gaussian_taps(3.0)) are scipy's, bitwise.
3. Conditions on the golden alone, so that a kernel ignoring the flag cannot pass the GPU tests: in every case the flag changes the
   score bits of every refined peak, and over the f = 4 and f = 8 blob cases at least five peaks change their integer coordinates.
4. Every modelled misreading of the definition is rejected by g20.
5. The new entry point refuses bad arguments before any HIP call.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import peaks_gauss_ref as pg
from helpers import ROOT, gold

# c1 f=4 blobs / edges / corners / close pairs; c2 f=1; c3 f=2.5; c4 f=8; c5 f=12.8; c6 two-row map; c7 plateaus and ridges (ties);
# c8 patches built so that the order of the float64 sum decides a float32 rounding (make_golden_peaks_gauss.py: order_sensitive_case)
CASES = ("c1", "c2", "c3", "c4", "c5", "c6", "c7", "c8")
THRE1 = 0.1
_cache = {}


def g20():
    if "g" not in _cache:
        _cache["g"] = gold("g20_peaks_gauss.npz")
    return _cache["g"]


def patches(case):
    """The up-sampled patches of a case: computed once, shared by every test (the faults only redo the filter)."""
    if case not in _cache:
        g = g20()
        _cache[case] = pg.upsampled_patches(THRE1, g["heat_" + case], float(g["f_" + case]))
    return _cache[case]


def bits32(col):
    return np.asarray(col, dtype=np.float64).astype(np.float32).view(np.uint32)


def same_rows(a, b):
    """x, y, id, joint type equal; scores equal as float32 bits."""
    return a.shape == b.shape and np.array_equal(a[:, [0, 1, 3, 4]], b[:, [0, 1, 3, 4]]) and np.array_equal(bits32(a[:, 2]), bits32(b[:, 2])) \
        and np.array_equal(a[:, 2], b[:, 2])


def test_restatement_equals_live_scipy_bit_for_bit():
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.RandomState(7)
    shapes = [(5, 5), (3, 5), (3, 3), (1, 5), (12, 20), (20, 20), (24, 40), (40, 40), (64, 64), (38, 64), (8, 16), (2, 20)]
    n = 0
    for shape in shapes:
        for rep in range(14):
            a = (rng.standard_normal(shape) * (10.0 ** rng.randint(-3, 3))).astype(np.float32) if rep % 2 else rng.uniform(0, 1, shape).astype(np.float32)
            want = ndi.gaussian_filter(a, sigma=3)
            got = pg.gaussian_filter_f32(a)
            assert want.dtype == np.float32 and got.dtype == np.float32
            assert np.array_equal(want.view(np.uint32), got.view(np.uint32)), "shape %s sample %d differs from scipy" % (shape, rep)
            n += 1
    assert n >= 160


def test_weights_are_scipys():
    from multiposenet.pytorch_amd.datasets.prn_data import gaussian_taps
    w = g20()["weights"]
    assert w.shape == (25,) and w.dtype == np.float64
    assert np.array_equal(gaussian_taps(3.0).view(np.uint64), w.view(np.uint64))
    assert np.array_equal(pg.gaussian_weights().view(np.uint64), w.view(np.uint64))
    assert np.array_equal(w.view(np.uint64), w[::-1].view(np.uint64)), "scipy's kernel is bitwise symmetric (the C ABI requires it)"


@pytest.mark.parametrize("case", CASES)
def test_restatement_equals_recorded_patches_and_rows(case):
    g = g20()
    f = float(g["f_" + case])
    assert g["heat_" + case].dtype == np.float32 and g["heat_" + case].shape[2] == 18
    assert int(g["npatch_" + case]) >= 1
    mine = {}
    for per in patches(case):
        for _, _, _, _, up in per:
            mine.setdefault(up.shape, []).append(up)
    for n in range(int(g["npatch_" + case])):
        up, sm = g["up_%s_%d" % (case, n)], g["sm_%s_%d" % (case, n)]
        assert np.array_equal(pg.gaussian_filter_f32(up).view(np.uint32), sm.view(np.uint32)), "recorded patch %d of %s" % (n, case)
        assert any(np.array_equal(up.view(np.uint32), u.view(np.uint32)) for u in mine[up.shape]), "recorded up-sampled patch %d is none of mine" % n
    assert same_rows(pg.rows(pg.nms_from_patches(patches(case), f)), g["on_" + case])
    # with the refinement off the flag is never reached: the recorded rows are the plain ones
    from oracle import joint_oracle as jo
    assert same_rows(pg.rows(jo.nms_peaks(THRE1, g["heat_" + case], f, refine=False)), g["plain_" + case])


def test_golden_conditions():
    g = g20()
    moved = 0
    for case in CASES:
        on, off = g["on_" + case], g["off_" + case]
        assert len(on) == len(off) >= 6 and np.array_equal(on[:, 3:], off[:, 3:])
        unchanged = bits32(on[:, 2]) == bits32(off[:, 2])
        assert not unchanged.any(), "%s: %d peaks keep their score bits with the flag on" % (case, int(unchanged.sum()))
        if case in ("c1", "c4"):
            moved += int((on[:, :2] != off[:, :2]).any(1).sum())
    assert moved >= 5, "only %d peaks of the f = 4 and f = 8 cases move" % moved
    # the shapes the cases are there for
    shapes = {case: {up.shape for per in patches(case) for *_, up in per} for case in CASES}
    assert {(20, 20), (12, 20), (20, 12), (12, 12)} <= shapes["c1"]
    assert {(5, 5), (3, 5), (5, 3), (3, 3)} <= shapes["c2"]
    assert {(12, 12), (8, 12), (8, 8)} <= shapes["c3"]
    assert (40, 40) in shapes["c4"] and (64, 64) in shapes["c5"] and {(38, 64), (64, 38)} <= shapes["c5"]
    assert all(s[0] == 8 for s in shapes["c6"])
    # ties at the maximum exist (the plateau case): the last maximum is another cell for some peak
    first = pg.rows(pg.nms_from_patches(patches("c7"), 1.0))
    last = pg.rows(pg.nms_from_patches(patches("c7"), 1.0, tie="last"))
    assert np.array_equal(first[:, 2], last[:, 2]) and (first[:, :2] != last[:, :2]).any()


W11 = pg.gaussian_weights(radius=11)
FAULTS = {
    "single_reflection": dict(smooth=lambda a: pg.gaussian_filter_f32(a, reflect="single")),
    "mirror_reflection": dict(smooth=lambda a: pg.gaussian_filter_f32(a, reflect="mirror")),
    "float32_accumulation": dict(smooth=lambda a: pg.gaussian_filter_f32(a, acc=np.float32)),
    "no_rounding_between_passes": dict(smooth=lambda a: pg.gaussian_filter_f32(a, round_between=False)),
    "axis1_first": dict(smooth=lambda a: pg.gaussian_filter_f32(a, axes=(1, 0))),
    "radius_11": dict(smooth=lambda a: pg.gaussian_filter_f32(a, w=W11)),
    "score_unsmoothed": dict(score_from="upsampled"),
    "last_maximum": dict(tie="last"),
    "k_ascending": dict(smooth=lambda a: pg.gaussian_filter_f32(a, k_descending=False)),
}


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_modelled_fault_fails_against_golden(fault):
    g = g20()
    hit = [case for case in CASES
           if not same_rows(pg.rows(pg.nms_from_patches(patches(case), float(g["f_" + case]), **FAULTS[fault])), g["on_" + case])]
    assert hit, "the fault %r changes nothing on the fixtures" % fault


def test_entry_point_rejects_bad_arguments_without_touching_the_gpu():
    from multiposenet.pytorch_amd import _lib
    L = _lib.lib()
    src = open(os.path.join(ROOT, "include", "mpn.h")).read()
    BAD = int(re.search(r"#define\s+MPN_E_BADARG\s+\(?(-?\d+)\)?", src).group(1))
    UNSUP = int(re.search(r"#define\s+MPN_E_UNSUPPORTED\s+\(?(-?\d+)\)?", src).group(1))
    nul, one = ctypes.c_void_p(None), ctypes.c_void_p(0x1000)            # never dereferenced: validation fails first
    w = g20()["weights"]
    arr = lambda v: (ctypes.c_double * len(v))(*v)

    def call(taps, radius, heat=one, cap=16, ws=one, upsamp=4.0, refine=1):
        return L.mpn_heatmap_peaks_smooth(heat, 0, 0, 0, 0, 1, 18, 8, 8, 0.1, upsamp, refine, taps, radius, one, one, cap, ws, nul)

    assert call(None, 12) == BAD                                           # null taps
    assert call(arr(w), 0) == BAD and call(arr(w), -1) == BAD and call(arr(np.ones(35) / 35), 17) == BAD
    skew = w.copy()
    skew[3] = np.nextafter(skew[3], 1.0)
    assert call(arr(skew), 12) == BAD                                      # not bitwise symmetric
    neg = np.array([-0.0, 1.0, 0.0])
    assert call(arr(neg), 1) == BAD                                        # -0.0 and 0.0 differ in bits
    assert call(arr(w), 12, heat=nul) == BAD and call(arr(w), 12, cap=0) == BAD and call(arr(w), 12, ws=nul) == BAD
    assert call(arr(w), 12, upsamp=13.0) == UNSUP                          # rint(65) > 64, refused before any launch
    assert call(arr(w), 12, upsamp=0.0) == BAD
    assert call(arr(w), 12, upsamp=13.0, refine=0, heat=nul) == BAD        # refine == 0: mpn_heatmap_peaks' own checks
