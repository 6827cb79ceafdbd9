"""CPU tier of the PRN-assignment parity tests (csrc/prn_assign.hip; generator, references and models in tests/prn_assign_ref.py).

1. Anchoring: the h, w-parametrised build_maps restatement equals prn_assign_oracle.build_maps at 56x36 on every scene; the float64
   model of the kernel's blur order equals prn_assign_oracle.gaussian (scipy) bit for bit; the model of np_sum_window equals np.sum.
2. Generator conditions the GPU tier relies on.
3. mpn_prn_match_host itself — plain C++, run here through ctypes — against prn_assign_oracle.assign, with its limits driven.
4. Teeth: numpy models of the three kernels and of the matcher pass the GPU tier's comparisons; each named mutant fails one."""
import numpy as np
import pytest

import prn_assign_ref as R
from helpers import report
from oracle import prn_assign_oracle as O
from prn_assign_ref import H0, W0, f32, f64


SCENES = {"normal": R.normal_scene, "dense": R.dense_scene}
SHAPES = [(56, 36), (9, 5), (3, 7), (1, 1), (64, 64)]


def all_windows(h=H0, w=W0, N=15):
    return {(y, x): R.window_shape(y, x, N, h, w) for y in range(h) for x in range(w)}


# ====================================================================================================== 1. anchoring
@pytest.mark.parametrize("name", ["normal", "dense", "index error", "crowded"])
def test_parametrised_build_maps_equals_the_oracle_at_56x36(name):
    if name == "index error":
        sc = R.index_error_scene()
        with pytest.raises(IndexError):
            O.build_maps(sc.kps[0], sc.boxes[0], in_thres=sc.in_thres)
        with pytest.raises(IndexError):
            R.build_maps_hw(sc.kps[0], sc.boxes[0], H0, W0, sc.in_thres)
        cases = [(sc.kps[0], [sc.boxes[0][0], sc.boxes[0][2]], sc.in_thres)]
    else:
        sc = R.crowded_scene(77) if name == "crowded" else SCENES[name]()
        cases = [(sc.kps[i], sc.boxes[i], sc.in_thres) for i in range(sc.nimg)]
    cells = 0
    for kps, boxes, thr in cases:
        a, b = O.build_maps(kps, boxes, in_thres=thr), R.build_maps_hw(kps, boxes, H0, W0, thr)
        assert a[0] == b[0] and a[1] == b[1]
        assert np.array_equal(a[2], b[2]) and np.array_equal(a[3].view(np.uint64), b[3].view(np.uint64))
        cells += a[2].size
    report("prn_assign cpu: build_maps restatement == oracle on %-12s %d table values, %d images" % (name, cells, len(cases)))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_blur_model_equals_scipy_bit_for_bit(shape):
    rs = np.random.RandomState(shape[0] * 100 + shape[1])
    n = 0
    for fill in (0.02, 0.3, 1.0):
        for _ in range(20):
            plane = (rs.rand(*shape) < fill).astype(f64)
            if fill == 0.02 and not plane.any():
                plane[rs.randint(shape[0]), rs.randint(shape[1])] = 1.0
            assert np.array_equal(R.blur_model(plane).view(np.uint64), O.gaussian(plane).view(np.uint64)), (shape, fill)
            n += 1
    report("prn_assign cpu: blur model == scipy gaussian_filter at %dx%d on %d planes (2 %%, 30 %%, full)" % (shape + (n,)))


def test_window_sum_model_equals_np_sum_on_every_window_shape():
    rs = np.random.RandomState(3)
    shapes = set(all_windows().values())
    assert len(shapes) == 64
    n = 0
    for N in R.NS:
        for sh in sorted(set(all_windows(N=N).values())):
            for kind in range(3):
                v = rs.uniform(0, 1, sh).astype(f32)
                if kind == 1:
                    v = (v * np.exp2(rs.randint(-4, 4, sh)) * np.where(rs.rand(*sh) < 0.5, -1, 1)).astype(f32)
                assert R.np_sum_model(v).view(np.uint32) == np.sum(v).view(np.uint32), (N, sh)
                n += 1
    report("prn_assign cpu: np_sum_window model == np.sum on %d windows (64 shapes at N = 15, N in %s)" % (n, list(R.NS)))


# ====================================================================================================== 2. generator conditions
def test_normal_scene_holds_every_planted_condition():
    sc = R.normal_scene()
    a = sc.arrays()
    assert [len(b) for b in sc.boxes] == [4, 0, 3] and 2 <= len(a["boxes"]) <= 10
    assert a["joint_off"][1, 0] > 0 and a["joint_off"][2, 0] > a["joint_off"][1, 0]           # ids of later images need rebasing
    for i, missing in ((0, (7,)), (2, (4, 11))):
        for t in range(17):
            assert (a["joint_off"][i, t + 1] == a["joint_off"][i, t]) == (t in missing)
    # every clamp class for every box, among the peaks that pass its inside test
    for i in (0, 2):
        for bb in sc.boxes[i]:
            b = R.xywh(bb)
            seen = {}
            for k in sc.kps[i]:
                if R.is_inside(k, b, 0.21):
                    c = R.clamp_class(k, b, H0, W0)
                    seen[c] = seen.get(c, 0) + 1
            assert len(seen) == 9 and min(seen.values()) >= 3, seen
    # strict edges: the edge itself is outside, its neighbour inside — decided by the oracle, one peak at a time
    for kind, want in (("edge out", 0), ("edge in", 1)):
        for tag in ("x lo", "y lo", "x hi", "y hi"):
            pl = sc.planted[(kind, tag)]
            assert len(pl) == 7
            for img, bi, ki in pl:
                _, _, old, _ = O.build_maps([sc.kps[img][ki]], [sc.boxes[img][bi]])
                assert int(old[0, :, :, 0, :].sum()) == want, (kind, tag, img, bi)
    # products exactly on an integer, and in (-1, 0)
    b = R.xywh(sc.boxes[0][0])
    assert W0 / np.ceil(b[2]) == 0.5 and H0 / np.ceil(b[3]) == 0.5
    for img, bi, ki in sc.planted["integer"]:
        k = sc.kps[img][ki]
        px, py = (k[0] - b[0]) * 0.5, (k[1] - b[1]) * 0.5
        assert px == int(px) and py == int(py)
    assert any((sc.kps[0][ki][0] - b[0]) * 0.5 == W0 and (sc.kps[0][ki][1] - b[1]) * 0.5 == H0 for _, _, ki in sc.planted["integer"])
    for tag, ax in (("(-1,0) x", (0,)), ("(-1,0) y", (1,)), ("(-1,0) xy", (0, 1))):
        for img, bi, ki in sc.planted[tag]:
            for d in ax:
                assert -1 < (sc.kps[img][ki][d] - b[d]) * 0.5 < 0
            assert R.clamp_class(sc.kps[img][ki], b, H0, W0) == (0, 0) and R.is_inside(sc.kps[img][ki], b, 0.21)
    # collisions: the three near-identical peaks share one cell of their box, and the duplicate is exact
    for img, bi, ki in sc.planted["collide"]:
        b = R.xywh(sc.boxes[img][bi])
        first = sc.kps[img][[k for (im2, b2, k) in sc.planted["collide"] if (im2, b2) == (img, bi)][0]]
        sx, sy = W0 / np.ceil(b[2]), H0 / np.ceil(b[3])
        assert (int((sc.kps[img][ki][0] - b[0]) * sx), int((sc.kps[img][ki][1] - b[1]) * sy)) == (int((first[0] - b[0]) * sx), int((first[1] - b[1]) * sy))
    dups = sc.planted["dup"]
    assert all(sc.kps[dups[j][0]][dups[j][2]] == sc.kps[dups[j + 1][0]][dups[j + 1][2]] for j in range(0, len(dups), 2))
    # cells overwritten by a later peak, in every box: more (peak, box) pairs pass the inside test than cells end up occupied
    m = R.scene_maps(sc)
    b0 = 0
    for i in (0, 2):
        for bi, bb in enumerate(sc.boxes[i]):
            inside = sum(R.is_inside(k, R.xywh(bb), 0.21) for k in sc.kps[i])
            assert inside >= int((m["occ"][b0 + bi] > 0).sum()) + 3, (i, bi)
        b0 += len(sc.boxes[i])
    assert int((m["occ"] > 0).sum()) > 400
    report("prn_assign cpu: normal scene: %d peaks, %d boxes, %d occupied cells, 9/9 clamp classes per box, 56 strict-edge peaks" % (
        len(a["peaks"]), len(a["boxes"]), int((m["occ"] > 0).sum())))


def test_dense_and_index_error_scenes_are_what_they_claim():
    m = R.scene_maps(R.dense_scene())
    assert (m["occ"][0, 3] > 0).sum() > H0 * W0 // 2
    sc = R.index_error_scene()
    (img, bi, ki), = sc.planted["bad"]
    for j, bb in enumerate(sc.boxes[0]):
        if j == bi:
            with pytest.raises(IndexError):
                O.build_maps([sc.kps[0][ki]], [bb], in_thres=sc.in_thres)
        else:
            assert not R.is_inside(sc.kps[0][ki], R.xywh(bb), sc.in_thres)
    R.scene_maps(sc, skip_boxes=((0, 1),))                          # the other two boxes raise nothing
    report("prn_assign cpu: dense plane %d / %d cells occupied; IndexError scene raises for box 1 only" % ((m["occ"][0, 3] > 0).sum(), H0 * W0))


def test_score_cases_reach_every_window_shape_and_count_class():
    for kind in ("unit", "signed"):
        out, occ = R.score_case(kind)
        assert (occ[0, 3] > 0).all() and (occ[1, 16] > 0).all() and 0 < (occ[0, 0] > 0).sum() < 100
        shapes = {R.window_shape(y, x, 15) for b, t, y, x in np.argwhere(occ > 0)}
        assert len(shapes) == 64 == len(set(all_windows().values()))
        assert (out > 0).all() if kind == "unit" else ((out < 0).any() and np.log2(np.abs(out).max() / np.abs(out).min()) > 6)
    # the window sizes meet every path of the sum: n < 8 (N = 1 only), n % 8 tails, one block, two blocks
    sizes = {N: {s[0] * s[1] for s in all_windows(N=N).values()} for N in R.NS}
    assert sizes[1] == {1} and max(sizes[15]) == 225 and any(n > 128 for n in sizes[15]) and any(n <= 128 for n in sizes[15])
    assert {n % 8 for n in sizes[15]} == set(range(8)) and {4, 6} <= sizes[3]                # every tail length; n < 8 beyond N = 1
    for cap in (1, 64):
        for over in (True, False):
            _, occ = R.count_case(cap, over)
            counts = set((occ > 0).sum(axis=(2, 3)).reshape(-1).tolist())
            assert counts == {c for c in R.COUNT_CLASSES[cap] if over or c <= cap}
        assert {0, 1, cap - 1, cap, cap + 1, H0 * W0} == set(R.COUNT_CLASSES[cap])
    out, what = R.argmax_case()
    flat = out.transpose(0, 3, 1, 2).reshape(-1, H0 * W0)
    assert {int(np.argmax(flat[p])) % 64 for p in range(64)} == set(range(64))
    for p, pair in ((64, (200, 264)), (65, (777, 778)), (66, (0, 2015))):
        assert np.array_equal(np.nonzero(flat[p] == flat[p].max())[0], pair)
    assert (flat[67] == flat[67][0]).all() and np.argmax(flat[68]) == 31 * 64 + 5 and np.argmax(flat[69]) == 63
    report("prn_assign cpu: score cases: 64 window shapes, count classes %s, %d arg-max planes" % (dict(R.COUNT_CLASSES), len(what)))


def _tables(scene, out):
    """Per (image, type) the list of candidate scores of the reference's table (positive and not)."""
    occ = R.scene_maps(scene)["occ"]
    a = scene.arrays()
    res = {}
    for (b, t, y, x), s in R.ref_scores(out, occ, 15).items():
        res.setdefault((int(a["box_img"][b]), t), []).append(float(s))
    return res


def test_tie_free_scenes_have_no_equal_scores_in_a_table():
    n = 0
    for sc, seed in ((R.normal_scene(), 11), (R.dense_scene(), 12)):
        for key, v in _tables(sc, R.standin_out(sc, seed)).items():
            assert len(set(v)) == len(v), (sc.name, key)
            n += len(v)
    report("prn_assign cpu: tie-free scenes: %d candidate scores, no two equal in one (image, type) table" % n)


# ====================================================================================================== 3. mpn_prn_match_host directly
def _host_path(scene, out, cap=64, maps=None):
    """Candidate lists from the references (np.sum over the oracle's crop, np.argwhere order), then the C++ matcher."""
    maps = maps or R.scene_maps(scene)
    cn, ci, cs, _ = R.ref_candidates(out, maps["occ"], 15, cap)
    amax = R.ref_argmax(out)
    return R.match_host(scene.arrays(), cn, ci, cs, cap, amax), (cn, ci, cs, amax)


def test_matcher_equals_the_oracle_on_the_generated_scenes():
    for sc, seed in ((R.normal_scene(), 11), (R.dense_scene(), 12)):
        out = R.standin_out(sc, seed)
        cap = 2048 if sc.name == "dense" else 64
        (kp, flags), _ = _host_path(sc, out, cap)
        dense_big = sc.name == "dense"                                # > 64 ids of type 3: the matcher must hand that pair back
        pairs, nflag = R.check_match(sc, R.ref_assign(sc, out), kp, flags, max_flagged=1 if dense_big else 0, must_flag=[(0, 3)] if dense_big else [])
        report("prn_assign cpu: mpn_prn_match_host == oracle.assign on %-7s %d (box, type) pairs compared, %d (image, type) flagged" % (sc.name, pairs, nflag))


@pytest.mark.parametrize("seed", [77, 78])
def test_matcher_equals_the_oracle_on_crowded_scenes_without_a_flag(seed):
    sc = R.crowded_scene(seed, nimg=4)
    out = R.standin_out(sc, seed)
    (kp, flags), _ = _host_path(sc, out)
    pairs, nflag = R.check_match(sc, R.ref_assign(sc, out), kp, flags, max_flagged=0)
    report("prn_assign cpu: mpn_prn_match_host == oracle.assign on crowded scene %d: %d boxes, %d pairs compared, %d flagged" % (
        seed, sum(len(b) for b in sc.boxes), pairs, nflag))


PLANTED = {
    # name: (sites, boxes, {(box, peak): score}, flagged?, expected peak per box or None)
    "single column": (("P0",), 2, {(0, 0): 0.5, (1, 0): 0.9}, False, (0, 0)),
    "single column, one box without a positive score": (("P0",), 2, {(0, 0): 0.0, (1, 0): 0.9}, False, (None, 0)),
    "best peak is the other box's worst column": (("P0", "P1"), 2, {(0, 0): 0.9, (0, 1): 0.1, (1, 0): 0.95, (1, 1): 0.99}, False, (0, 1)),
    "the same with an empty cell in that row": (("P0", "P1", "PA"), 2, {(0, 0): 0.9, (0, 1): 0.1, (0, 2): 0.05, (1, 0): 0.95, (1, 1): 0.99}, False, (2, 1)),
    "equal scores in one row": (("P0", "P1"), 2, {(0, 0): 0.5, (0, 1): 0.5, (1, 0): 0.25, (1, 1): 0.75}, True, None),
    "equal scores in one column": (("P0", "P1"), 2, {(0, 0): 0.5, (0, 1): 0.3, (1, 0): 0.5, (1, 1): 0.75}, True, None),
    "equal scores in different rows and columns": (("P0", "P1"), 2, {(0, 0): 0.5, (0, 1): 0.3, (1, 0): 0.25, (1, 1): 0.5}, False, (0, 1)),
}


def planted(name):
    sites, nbx, scores, flagged, want = PLANTED[name]
    sc = R.planted_scene(sites, nbx)
    out = R.planted_out(sc, scores)
    maps = R.scene_maps(sc)
    # the planted value IS the window sum (every other cell of the plane is zero and no window holds two sites)
    got = R.ref_scores(out, maps["occ"], 15)
    for (b, k), v in scores.items():
        (y, x), = np.argwhere(maps["occ"][b, 0] == k + 1)
        assert got[(b, 0, int(y), int(x))] == f32(v)
    return sc, out, flagged, want


@pytest.mark.parametrize("name", list(PLANTED))
def test_matcher_planted_tables(name):
    sc, out, flagged, want = planted(name)
    (kp, flags), _ = _host_path(sc, out)
    assert bool(flags[0, 0]) == flagged and not flags[0, 1:].any()
    ref = R.ref_assign(sc, out)
    pairs, nflag = R.check_match(sc, ref, kp, flags, max_flagged=int(flagged), must_flag=[(0, 0)] if flagged else [])
    if want is not None:                                            # the outcome the case was built for, stated from the reference
        for b, k in enumerate(want):
            exp = [0.0, 0.0, 0.0] if k is None else [sc.kps[0][k][0], sc.kps[0][k][1], 1.0]
            assert ref[b, 0].tolist() == exp, (name, b, ref[b, 0])
    assert (kp[:, 1:, 2] == 0).all() and np.array_equal(kp[:, 1:], ref[:, 1:])          # 16 empty types: the arg-max fallback everywhere
    report("prn_assign cpu: matcher planted %-52s %d pairs compared, %d flagged" % (name, pairs, nflag))


def test_matcher_fallback_leaves_assigned_types_alone_and_skips_an_image_without_boxes():
    sc = R.normal_scene()
    out = R.standin_out(sc, 11)
    (kp, flags), (cn, _, _, _) = _host_path(sc, out)
    ref = R.ref_assign(sc, out)
    a = sc.arrays()
    assert a["box_start"].tolist() == [0, 4, 4, 7] and not flags[1].any()
    empty = cn == 0
    assert empty.any() and (kp[empty][:, 2] == 0).all() and np.array_equal(kp, ref)
    assert (kp[~empty][:, 2] == 1).any()
    report("prn_assign cpu: matcher fallback: %d (box, type) pairs from the arg-max, %d assigned, image 1 has no boxes" % (empty.sum(), (kp[..., 2] == 1).sum()))


def limit_cases():
    """name -> (Scene, cap, truncate?, flagged (image, type) set): scenes that drive the matcher's fixed tables."""
    cases = {}
    # 65 boxes in one image (table[64*64] / used[64] hold 64): a 13 x 5 grid of boxes, one peak of types 0 and 1 in each
    boxes = [(100.0 * i, 150.0 * j, 100.0 * i + 60.0, 150.0 * j + 100.0) for j in range(5) for i in range(13)]
    kps = [(b[0] + 30.0, b[1] + 40.0 + 10 * t, 1, 0, t) for t in (0, 1) for b in boxes]
    cases["65 boxes"] = (R.Scene("65 boxes", [kps], [boxes]), 64, False, {(0, 0), (0, 1)})
    big = (0.0, 0.0, 360.0, 560.0)                                   # scale 0.1: a peak every 10 px is a cell of its own

    def grid(n, t):
        return [(10.0 * (k % 36) + 5.0, 10.0 * (k // 36) + 5.0, 1, 0, t) for k in range(n)]
    cases["64 ids"] = (R.Scene("64 ids", [grid(64, 5) + grid(3, 6)], [[big, (5.0, 5.0, 300.0, 500.0)]]), 128, False, set())
    cases["65 ids"] = (R.Scene("65 ids", [grid(65, 5) + grid(3, 6)], [[big, (5.0, 5.0, 300.0, 500.0)]]), 128, False, {(0, 5)})
    cases["520 ids"] = (R.Scene("520 ids", [grid(520, 5) + grid(3, 6)], [[big]]), 600, False, {(0, 5)})
    cases["600 ids in two boxes"] = (R.Scene("600 ids", [grid(600, 5) + grid(3, 6)], [[big, (-3600.0, 0.0, 3960.0, 560.0)]]), 1024, False, {(0, 5)})
    cases["cand_n > cap"] = (R.Scene("cand_n > cap", [grid(5, 5) + grid(3, 6)], [[big, (5.0, 5.0, 300.0, 500.0)]]), 4, True, {(0, 5)})
    return cases


@pytest.mark.parametrize("name", ["65 boxes", "64 ids", "65 ids", "520 ids", "600 ids in two boxes", "cand_n > cap"])
def test_matcher_limits_are_flagged_and_write_nothing_out_of_bounds(name):
    sc, cap, _, want_flags = limit_cases()[name]
    nb = sum(len(b) for b in sc.boxes)
    out = np.random.RandomState(5).uniform(0.01, 1.0, (nb, H0, W0, 17)).astype(f32)
    (kp, flags), (cn, ci, _, _) = _host_path(sc, out, cap)           # match_host asserts its guard bands
    assert {(int(i), int(t)) for i, t in np.argwhere(flags)} == want_flags
    if name == "cand_n > cap":
        assert (cn[:, 5] > cap).any()
    if name.endswith("ids") or "ids in" in name:
        assert len(set(ci[:, 5][ci[:, 5] != R.SENT_I].tolist())) == int(name.split()[0])
    pairs, nflag = R.check_match(sc, R.ref_assign(sc, out), kp, flags, max_flagged=len(want_flags), must_flag=sorted(want_flags))
    for im, t in want_flags:
        assert (kp[:, t] == 0).all()                                 # a flagged pair is left to the caller: nothing written
    report("prn_assign cpu: matcher limit %-22s %d pairs compared, %d flagged (exactly the expected ones)" % (name, pairs, nflag))


# ====================================================================================================== 4. teeth
BUILD_MUTANTS = ["no rebase", "independent ifs", "no wrap", ">= inside", "first wins", "reflect", "near tap"]


def _build_checks(mut):
    """Every build_maps comparison of the GPU tier, on the model: returns the names of those that fail."""
    failed = []
    runs = [(R.normal_scene(), H0, W0, 0, ()), (R.dense_scene(), H0, W0, 0, ()), (R.index_error_scene(), H0, W0, 1, ((0, 1),)),
            (R.normal_scene(), 9, 5, 0, ()), (R.normal_scene(), 1, 1, 0, ()), (R.normal_scene(), 64, 64, 0, ())]
    for sc, h, w, want_err, skip in runs:
        occ, pin, err = R.model_build_maps(sc.arrays(), h, w, sc.in_thres, mut)
        try:
            R.check_build_maps(sc, h, w, occ, pin, err, want_err, skip)
        except AssertionError:
            failed.append("%s %dx%d" % (sc.name, h, w))
    # the blur order with the cancelling kernel (with the gaussian weights the order moves the float64 sum in its last bit only, which
    # the float32 result hides: see prn_assign_ref.CANCEL_W9)
    sc = R.dense_scene()
    _, pin, _ = R.model_build_maps(sc.arrays(), H0, W0, sc.in_thres, mut, wts=R.CANCEL_W9)
    try:
        R.check_blur(sc, R.CANCEL_W9, pin)
    except AssertionError:
        failed.append("cancelling kernel")
    return failed


def test_build_maps_model_is_accepted():
    assert _build_checks(None) == []
    report("prn_assign cpu: teeth: build_maps model accepted by all 7 comparisons")


@pytest.mark.parametrize("mut", BUILD_MUTANTS)
def test_build_maps_mutant_is_rejected(mut):
    failed = _build_checks(mut)
    assert failed, "mutant '%s' passes every comparison" % mut
    report("prn_assign cpu: teeth: build_maps mutant %-18s rejected by %s" % (mut, failed))


SCORE_MUTANTS = ["r1 off by one", "left to right", "split not rounded", "last maximum"]


def _score_checks(mut):
    failed = []
    for kind in ("unit", "signed"):
        out, occ = R.score_case(kind)
        score = np.full(occ.shape, R.SENT_F, dtype=f32)
        amax = R.model_scores(out, occ, 15, score, mut)
        try:
            R.check_scores(out, occ, R.score_ref(kind, 15), score, amax)
        except AssertionError:
            failed.append("scores " + kind)
    out, _ = R.argmax_case()
    amax = np.array([[R.argmax_model(out[b, :, :, t].reshape(-1), mut) for t in range(17)] for b in range(out.shape[0])], dtype=np.int32)
    try:
        R.check_argmax(out, amax)
    except AssertionError:
        failed.append("arg-max planes")
    return failed


def test_scores_model_is_accepted():
    assert _score_checks(None) == []
    for N in (1, 3, 5, 9):
        out, occ = R.score_case("signed")
        score = np.full(occ.shape, R.SENT_F, dtype=f32)
        amax = R.model_scores(out, occ, N, score)
        R.check_scores(out, occ, R.score_ref("signed", N), score, amax)
    report("prn_assign cpu: teeth: scores / arg-max model accepted (N in %s)" % list(R.NS))


@pytest.mark.parametrize("mut", SCORE_MUTANTS)
def test_scores_mutant_is_rejected(mut):
    failed = _score_checks(mut)
    assert failed, "mutant '%s' passes every comparison" % mut
    report("prn_assign cpu: teeth: scores mutant %-18s rejected by %s" % (mut, failed))


COMPACT_MUTANTS = ["per lane order", "pos <= cap", "overflow >= cap"] + SCORE_MUTANTS


def _compact_checks(mut):
    failed = []
    for cap in (1, 64):
        for over in (True, False):
            out, occ = R.count_case(cap, over)
            res = R.model_compact(out, occ, 15, cap, mut)
            try:
                R.check_compact(out, R.count_ref(cap, over), cap, *res)
            except AssertionError:
                failed.append("cap %d%s" % (cap, " overflowing" if over else ""))
    return failed


def test_compact_model_is_accepted():
    assert _compact_checks(None) == []
    report("prn_assign cpu: teeth: compact model accepted by the 4 count-class comparisons")


@pytest.mark.parametrize("mut", COMPACT_MUTANTS[:3] + ["r1 off by one", "left to right"])
def test_compact_mutant_is_rejected(mut):
    failed = _compact_checks(mut)
    assert failed, "mutant '%s' passes every comparison" % mut
    report("prn_assign cpu: teeth: compact mutant %-18s rejected by %s" % (mut, failed))


def _match_checks(mut):
    failed = []
    runs = [(n,) + planted(n)[:3] for n in PLANTED] + [("normal", R.normal_scene(), R.standin_out(R.normal_scene(), 11), False)]
    for name, sc, out, flagged in runs:
        maps = R.scene_maps(sc)
        cn, ci, cs, _ = R.ref_candidates(out, maps["occ"], 15, 64)
        kp, flags = R.model_match(sc.arrays(), cn, ci, cs, 64, R.ref_argmax(out), H0, W0, mut)
        try:
            R.check_match(sc, R.ref_assign(sc, out), kp, flags, max_flagged=int(flagged), must_flag=[(0, 0)] if flagged else [])
        except AssertionError:
            failed.append(name)
    return failed


def test_matcher_model_is_accepted_and_equals_the_library():
    assert _match_checks(None) == []
    sc = R.normal_scene()
    out = R.standin_out(sc, 11)
    (kp, flags), (cn, ci, cs, amax) = _host_path(sc, out)
    kp2, flags2 = R.model_match(sc.arrays(), cn, ci, cs, 64, amax, H0, W0)
    assert np.array_equal(kp, kp2) and np.array_equal(flags, flags2)
    report("prn_assign cpu: teeth: matcher model accepted by %d comparisons and equal to mpn_prn_match_host" % (len(PLANTED) + 1))


@pytest.mark.parametrize("mut", ["no worst column", "ties in rows only"])
def test_matcher_mutant_is_rejected(mut):
    failed = _match_checks(mut)
    assert failed, "mutant '%s' passes every comparison" % mut
    report("prn_assign cpu: teeth: matcher mutant %-18s rejected by %s" % (mut, failed))
