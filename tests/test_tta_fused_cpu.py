"""Fused, flip-paired test-time augmentation, CPU tier: the numpy restatement of the merge rule (tests/tta_merge_ref.py) pinned to the
recorded run of the real reference Tester (tests/golden/g15_tta.npz), the modelled misreadings it must reject, the shared
scale-geometry helper, and the argument validation of the two entry points."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from helpers import ROOT, gold
import tta_merge_ref as ref
import tta_standin

INP = 48                      # params.inp_size of the recorded run (tests/golden/make_golden_tta.py)
BOUND = 2e-5                  # tests/test_round4_gpu.py: heat_avg_* of the product against the recording
FLIP_TAG = 7.0                # the stand-in's boxes depend on the padded shape only: the mirrored pass is told apart by this shift


def _chain(img):
    """The fused data flow restated on the CPU: per scale the pair input, the stand-in network on both images, the x4 up-sampled and
    cropped pair map; the person boxes (score > 0.5, class 0, times 1 / im_scale in float32) of every scale and pass."""
    from multiposenet.pytorch_amd.evaluate.tester import scale_geometry
    H, W = img.shape[0], img.shape[1]
    maps, shapes, boxes = [], [], []
    for m in [x * INP / float(H) for x in [0.5, 1., 1.5, 2, 2.5]]:
        im_scale, h, w, hp, wp = scale_geometry(H, W, m * H, 32)
        shapes.append((1, 3, hp, wp))
        heats, per_pass = [], []
        for p, src in enumerate((img, img[:, ::-1])):
            x = ref.input_ref(src, h, w, hp, wp, 1.0 / im_scale)
            heat, (s, c, b) = tta_standin.standin_outputs(torch.from_numpy(x)[None])
            heats.append(heat.numpy())
            s, c, b = s.numpy(), c.numpy(), b.numpy() + np.float32(FLIP_TAG * p)
            per_pass.append([(b[j, :] * (1.0 / im_scale)).tolist() for j in np.where(s > 0.5)[0] if int(c[j]) == 0])
        boxes.append(per_pass)
        maps.append(ref.upsample_crop_ref(np.concatenate(heats), h, w))
    return maps, shapes, boxes


@pytest.fixture(scope="module")
def chains():
    g = gold("g15_tta.npz")
    return g, {tag: _chain(g["img_" + tag]) for tag in ("a", "b")}


def test_scale_geometry_gives_the_recorded_padded_input_shapes(chains):
    g, ch = chains
    for tag in ("a", "b"):
        assert [list(s) for s in ch[tag][1]] == g["shapes_" + tag].tolist() == g["shapes_flip_" + tag].tolist()


def test_merge_restatement_matches_the_recorded_reference_run(chains):
    g, ch = chains
    for tag in ("a", "b"):
        img = g["img_" + tag]
        got = ref.merge_ref(ch[tag][0], img.shape[0], img.shape[1])
        err = float(np.abs(got.astype(np.float64) - g["heat_avg_" + tag]).max())
        print("image %s: merge restatement vs recorded heat_avg %.3e" % (tag, err))
        assert got.dtype == np.float32 and got.shape == g["heat_avg_" + tag].shape and err <= BOUND, (tag, err)
        # the true-division form (numpy's hm / 5) is the same rule up to one float32 rounding per scale
        assert float(np.abs(ref.merge_ref(ch[tag][0], img.shape[0], img.shape[1], divide=True).astype(np.float64) - g["heat_avg_" + tag]).max()) <= BOUND


@pytest.mark.parametrize("wrong", ["no_mirror", "no_swap", "swap_original", "mirror_about_W"])
def test_committed_inputs_reject_the_modelled_misreadings(chains, wrong):
    g, ch = chains
    for tag in ("a", "b"):
        img = g["img_" + tag]
        bad = ref.merge_ref(ch[tag][0], img.shape[0], img.shape[1], wrong=wrong)
        err = float(np.abs(bad.astype(np.float64) - g["heat_avg_" + tag]).max())
        print("image %s, %s: %.3e" % (tag, wrong, err))
        assert err > BOUND, (tag, wrong, err)


@pytest.mark.parametrize("wrong", ["one_accumulator", "divide_after_sum"])
def test_rounding_only_misreadings_differ_bitwise_on_a_constructed_input(wrong):
    """Both differ from the rule only in where float64 / float32 roundings fall: far below 2e-5 on real maps, so they are shown on a
    constructed table.  Its first scale has the image's own size (the bicubic sample is then the source value, coefficients 0 1 0 0)
    and holds 2^40 in the original stream and, mirrored and swapped, -2^40 in the flipped one: the two terms cancel exactly, and what
    is left of the O(1) terms of the other scales depends on whether they were added to 2^40 / 5 (float64 spacing 2^-15) or not."""
    rs = np.random.RandomState(5)
    H, W = 9, 11
    maps = [rs.uniform(0.1, 1.0, (7 + s, 6 + s, 36)).astype(np.float32) for s in range(1, 5)]
    first = np.empty((H, W, 36), dtype=np.float32)
    first[:, :, :18] = 2.0 ** 40
    first[:, :, 18:] = -2.0 ** 40
    maps = [first] + maps
    good = ref.merge_ref(maps, H, W)
    bad = ref.merge_ref(maps, H, W, wrong=wrong)
    assert good.shape == bad.shape and not np.array_equal(good, bad), wrong
    assert np.abs(good.astype(np.float64) - bad).max() <= 2.0 ** -12            # ... and in nothing but the rounding of those sums


def test_boxes_come_from_scale_index_one_of_the_original_pass(chains):
    g, ch = chains
    for i, tag in enumerate(("a", "b")):
        want = g["prn_boxes_%d" % i]
        boxes = ch[tag][2]

        def dist(sel):
            got = np.array(sel, dtype=np.float64).reshape(-1, 4)
            return float("inf") if got.shape != want.shape else float(np.abs(got - want).max())
        assert dist(boxes[1][0]) <= 1e-3, tag
        assert dist(boxes[1][1]) > 1e-3, "scale-1 boxes of the mirrored pass pass for the original's"
        assert dist(boxes[0][0]) > 1e-3, "boxes of scale index 0 pass for those of index 1"


def test_swap_table_is_the_testers():
    from multiposenet.pytorch_amd.evaluate.tester import SWAP_HEAT
    assert ref.SWAP_HEAT == SWAP_HEAT and sorted(SWAP_HEAT) == list(range(18))


def test_tta_entry_points_reject_bad_arguments_without_touching_the_gpu():
    from multiposenet.pytorch_amd import _lib
    L = _lib.lib()
    src = open(os.path.join(ROOT, "include", "mpn.h")).read()
    BAD = int(re.search(r"#define\s+MPN_E_BADARG\s+\(?(-?\d+)\)?", src).group(1))
    nul, one = ctypes.c_void_p(None), ctypes.c_void_p(0x1000)            # never dereferenced: validation fails first
    ok = dict(img=one, sY=159, sX=3, sC=1, H=37, W=53, out=one, h=24, w=34, hp=32, wp=64, inv=1.5)

    def tta_input(**kw):
        a = dict(ok, **kw)
        return L.mpn_tta_input(a["img"], a["sY"], a["sX"], a["sC"], a["H"], a["W"], a["out"], a["h"], a["w"], a["hp"], a["wp"], a["inv"], nul)
    for bad in (dict(img=nul), dict(out=nul), dict(H=0), dict(W=-1), dict(h=0), dict(w=0), dict(h=33), dict(w=65), dict(inv=0.0), dict(inv=-1.0)):
        assert tta_input(**bad) == BAD, bad

    def table(n, **kw):
        t = (_lib.TtaScale * max(n, 1))()
        for s in range(max(n, 1)):
            t[s].u, t[s].rh, t[s].rw, t[s].pitch = 0x1000, 24, 34, 34 * 36
            for k, v in kw.items():
                setattr(t[s], k, v)
        return t
    swap = (ctypes.c_int32 * 18)(*ref.SWAP_HEAT)

    def tta_merge(t, n, sw=swap, out=one, H=37, W=53):
        return L.mpn_tta_merge(t, n, sw, out, H, W, nul)
    assert tta_merge(None, 5) == BAD and tta_merge(table(5), 5, sw=None) == BAD and tta_merge(table(5), 5, out=nul) == BAD
    assert tta_merge(table(1), 0) == BAD and tta_merge(table(9), 9) == BAD
    assert tta_merge(table(5, u=None), 5) == BAD and tta_merge(table(5, rh=0), 5) == BAD and tta_merge(table(5, rw=-3), 5) == BAD
    assert tta_merge(table(5, pitch=34 * 36 - 1), 5) == BAD
    assert tta_merge(table(5), 5, H=0) == BAD and tta_merge(table(5), 5, W=0) == BAD
    for bad in ([0] * 18, list(range(1, 19)), ref.SWAP_HEAT[:17] + [ref.SWAP_HEAT[0]], [-1] + list(range(1, 18))):
        assert tta_merge(table(5), 5, sw=(ctypes.c_int32 * 18)(*bad)) == BAD, bad
