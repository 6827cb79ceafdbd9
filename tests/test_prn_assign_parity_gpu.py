"""GPU tier of the PRN-assignment parity tests: mpn_prn_build_maps, mpn_prn_scores, mpn_prn_scores_compact and the fast path
(compact + mpn_prn_match_host) against prn_assign_oracle, np.sum and np.argmax.  Every comparison is an equality; inputs,
references and the comparison functions are in tests/prn_assign_ref.py, their conditions and teeth in test_prn_assign_parity_cpu.py."""
import numpy as np
import pytest
import torch

import prn_assign_ref as R
from helpers import report
from prn_assign_ref import H0, W0, f32

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()            # a copy: the cached inputs are read-only


def run_build_maps(scene, h, w, status_only=False, wts=R.W9):
    from multiposenet.pytorch_amd import _lib, ops
    a = scene.arrays()
    nb = a["boxes"].shape[0]
    d_peaks, d_off, d_boxes, d_img, d_w9 = dev(a["peaks"]), dev(a["joint_off"]), dev(a["boxes"]), dev(a["box_img"]), dev(wts)
    occ = torch.full((nb, 17, h, w), int(R.SENT_I), dtype=torch.int32, device="cuda")
    pin = torch.full((nb, h, w, 17), float(R.SENT_F), dtype=torch.float32, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    st = _lib.lib().mpn_prn_build_maps(ops.ptr(d_peaks), ops.ptr(d_off), ops.ptr(d_boxes), ops.ptr(d_img), nb, h, w, float(scene.in_thres),
                                       ops.ptr(d_w9), ops.ptr(occ), ops.ptr(pin), ops.ptr(err), ops.stream_ptr())
    torch.cuda.synchronize()
    if status_only:
        return st, occ.cpu().numpy(), pin.cpu().numpy()
    assert st == 0
    return occ.cpu().numpy(), pin.cpu().numpy(), int(err.item())


def run_scores(out, occ, N):
    from multiposenet.pytorch_amd import ops
    from multiposenet.pytorch_amd._lib import call
    nb, h, w, _ = out.shape
    d_out, d_occ = dev(out), dev(occ)
    score = torch.full(occ.shape, float(R.SENT_F), dtype=torch.float32, device="cuda")
    amax = torch.full((nb, 17), int(R.SENT_I), dtype=torch.int32, device="cuda")
    call("mpn_prn_scores", ops.ptr(d_out), ops.ptr(d_occ), nb, h, w, N, ops.ptr(score), ops.ptr(amax), ops.stream_ptr())
    return score.cpu().numpy(), amax.cpu().numpy()


def run_compact(out, occ, N, cap):
    from multiposenet.pytorch_amd import ops
    from multiposenet.pytorch_amd._lib import call
    nb, h, w, _ = out.shape
    d_out, d_occ = dev(out), dev(occ)
    cn = torch.full((nb, 17), int(R.SENT_I), dtype=torch.int32, device="cuda")
    ci = torch.full((nb, 17, cap), int(R.SENT_I), dtype=torch.int32, device="cuda")
    cs = torch.full((nb, 17, cap), float(R.SENT_F), dtype=torch.float32, device="cuda")
    amax = torch.full((nb, 17), int(R.SENT_I), dtype=torch.int32, device="cuda")
    over = torch.zeros(1, dtype=torch.int32, device="cuda")
    call("mpn_prn_scores_compact", ops.ptr(d_out), ops.ptr(d_occ), nb, h, w, N, cap, ops.ptr(cn), ops.ptr(ci), ops.ptr(cs), ops.ptr(amax),
         ops.ptr(over), ops.stream_ptr())
    return cn.cpu().numpy(), ci.cpu().numpy(), cs.cpu().numpy(), amax.cpu().numpy(), int(over.item())


# ====================================================================================================== mpn_prn_build_maps
@pytest.mark.parametrize("name", ["normal", "dense"])
def test_build_maps_equals_the_oracle_on_a_multi_image_scene(name):
    sc = R.normal_scene() if name == "normal" else R.dense_scene()
    occ, pin, err = run_build_maps(sc, H0, W0)
    cells = R.check_build_maps(sc, H0, W0, occ, pin, err, want_err=0)
    report("prn_assign gpu: build_maps %-7s occ and blurred input equal the oracle: %d cells of %d boxes in %d images, %d occupied, err 0" % (
        name, cells, occ.shape[0], sc.nimg, int((occ > 0).sum())))


def test_build_maps_flags_the_reference_index_error_and_finishes_the_other_boxes():
    sc = R.index_error_scene()
    occ, pin, err = run_build_maps(sc, H0, W0)
    cells = R.check_build_maps(sc, H0, W0, occ, pin, err, want_err=1, skip_boxes=((0, 1),))
    report("prn_assign gpu: build_maps IndexError scene: err 1, the 2 other boxes equal the oracle (%d cells)" % cells)


def test_prn_assign_arrays_raises_index_error_on_both_paths():
    from multiposenet.pytorch_amd.evaluate import prn_process as pp
    from multiposenet.pytorch_amd.network.posenet import poseNet
    from test_prn_assign import _prn_weights
    model = poseNet(50, compute_dtype=torch.float32).cuda()
    model.load_state_dict({k: torch.from_numpy(v) for k, v in _prn_weights(model).items()}, strict=False)
    model.eval()
    sc = R.index_error_scene()
    a = sc.arrays()
    for fast in (True, False):
        with pytest.raises(IndexError):
            pp.prn_assign_arrays(model, a["peaks"], a["joint_off"], a["boxes"], a["box_start"], in_thres=sc.in_thres, fast=fast)
    report("prn_assign gpu: prn_assign_arrays raises IndexError on the fast and the full path (2 paths)")


def test_build_maps_blur_order_with_a_cancelling_kernel():
    """The summation order of the blur (centre, then pairs from the far tap inwards) cannot show in a float32 result with the
    gaussian weights; with weights whose far pairs cancel it does, and scipy.ndimage.correlate1d is the reference."""
    sc = R.dense_scene()
    occ, pin, err = run_build_maps(sc, H0, W0, wts=R.CANCEL_W9)
    assert err == 0 and np.array_equal(occ, R.scene_maps(sc)["occ"])
    n = R.check_blur(sc, R.CANCEL_W9, pin)
    report("prn_assign gpu: build_maps blur with a cancelling symmetric kernel equals scipy correlate1d: %d values" % n)


@pytest.mark.parametrize("shape", [(9, 5), (1, 1), (64, 64)], ids=lambda s: "%dx%d" % s)
def test_build_maps_at_other_map_sizes(shape):
    h, w = shape
    sc = R.normal_scene()
    occ, pin, err = run_build_maps(sc, h, w)
    cells = R.check_build_maps(sc, h, w, occ, pin, err, want_err=0)
    report("prn_assign gpu: build_maps at %dx%d equals the parametrised oracle: %d cells, %d occupied" % (h, w, cells, int((occ > 0).sum())))


def test_build_maps_refuses_4097_cells_without_launching():
    sc = R.normal_scene()
    for h, w in ((4097, 1), (1, 4097), (17, 241)):
        st, occ, pin = run_build_maps(sc, h, w, status_only=True)
        assert st == -3, "status %d, expected MPN_E_UNSUPPORTED (-3)" % st
        assert (occ == R.SENT_I).all() and (pin == R.SENT_F).all()           # nothing ran
    report("prn_assign gpu: build_maps returns MPN_E_UNSUPPORTED for 3 shapes of 4097 cells, outputs untouched")


# ====================================================================================================== mpn_prn_scores
@pytest.mark.parametrize("kind", ["unit", "signed"])
@pytest.mark.parametrize("N", R.NS)
def test_window_scores_equal_np_sum_bit_for_bit(N, kind):
    out, occ = R.score_case(kind)
    ref = R.score_ref(kind, N)
    score, amax = run_scores(out, occ, N)
    n = R.check_scores(out, occ, ref, score, amax)
    shapes = {R.window_shape(y, x, N) for (_, _, y, x) in ref}
    report("prn_assign gpu: scores N=%-2d %-6s %d cells equal np.sum, %d window shapes, %d empty cells keep the sentinel, %d arg-max planes" % (
        N, kind, n, len(shapes), occ.size - n, amax.size))


def test_arg_max_on_planted_planes():
    out, what = R.argmax_case()
    occ = np.zeros((out.shape[0], 17, H0, W0), dtype=np.int32)
    score, amax = run_scores(out, occ, 15)
    assert (score == R.SENT_F).all()
    R.check_argmax(out, amax)
    assert amax.reshape(-1)[67] == 0 and amax.reshape(-1)[66] == 0 and amax.reshape(-1)[64] == 200 and amax.reshape(-1)[65] == 777
    _, _, _, amax_c, over = run_compact(out, occ, 15, 4)
    R.check_argmax(out, amax_c)
    assert over == 0
    report("prn_assign gpu: arg-max equals np.argmax on %d planes (%d planted: lanes 0..63, ties, constant, partial chunk), both kernels" % (
        amax.size, len(what)))


# ====================================================================================================== mpn_prn_scores_compact
@pytest.mark.parametrize("kind", ["unit", "signed"])
def test_compact_candidates_equal_the_score_planes_and_np_sum(kind):
    out, occ = R.score_case(kind)
    cap = 64
    got = run_compact(out, occ, 15, cap)
    ref = R.score_ref(kind, 15)
    # reference lists from the np.sum dict (np.argwhere order = the dict's order within a plane)
    cn = (occ > 0).sum(axis=(2, 3)).astype(np.int32)
    ci = np.full((occ.shape[0], 17, cap), R.SENT_I, dtype=np.int32)
    cs = np.full((occ.shape[0], 17, cap), R.SENT_F, dtype=f32)
    fill = np.zeros((occ.shape[0], 17), dtype=np.int64)
    for (b, t, y, x), s in ref.items():
        k = fill[b, t]
        if k < cap:
            ci[b, t, k], cs[b, t, k] = occ[b, t, y, x] - 1, s
        fill[b, t] += 1
    n = R.check_compact(out, (cn, ci, cs, 1), cap, *got)
    score, amax = run_scores(out, occ, 15)
    for b in range(occ.shape[0]):                                    # ... and bit-equal to mpn_prn_scores' plane
        for t in range(17):
            cells = np.argwhere(occ[b, t] > 0)[:cap]
            assert np.array_equal(got[2][b, t, :len(cells)].view(np.uint32), score[b, t, cells[:, 0], cells[:, 1]].view(np.uint32))
    assert np.array_equal(got[3], amax)
    report("prn_assign gpu: compact %-6s %d candidates equal (occ - 1, np.sum) in argwhere order and the score planes; overflow 1" % (kind, n))


@pytest.mark.parametrize("over", [True, False], ids=["overflowing", "fitting"])
@pytest.mark.parametrize("cap", [1, 64])
def test_compact_count_classes_sentinels_and_overflow_word(cap, over):
    out, occ = R.count_case(cap, over)
    got = run_compact(out, occ, 15, cap)
    n = R.check_compact(out, R.count_ref(cap, over), cap, *got)
    assert got[4] == int(over)
    report("prn_assign gpu: compact cap=%-2d counts %s: %d candidates, %d sentinel slots kept, overflow %d" % (
        cap, sorted(set(got[0].reshape(-1).tolist())), n, int((got[1] == R.SENT_I).sum()), got[4]))


# ====================================================================================================== the fast path without a model
@pytest.mark.parametrize("name", ["normal", "dense", "crowded"])
def test_fast_path_equals_the_oracle_assignment(name):
    sc = {"normal": R.normal_scene, "dense": R.dense_scene, "crowded": lambda: R.crowded_scene(77, nimg=3)}[name]()
    out = R.standin_out(sc, 11)
    occ, _, err = run_build_maps(sc, H0, W0)
    assert err == 0
    cap = 64
    cn, ci, cs, amax, over = run_compact(out, occ, 15, cap)
    kp, flags = R.match_host(sc.arrays(), cn, ci, cs, cap, amax)
    # the dense scene's type 3 holds more than 64 candidates per plane: the one pair the matcher must hand back
    dense = name == "dense"
    assert over == int(dense)
    pairs, nflag = R.check_match(sc, R.ref_assign(sc, out), kp, flags, max_flagged=int(dense), must_flag=[(0, 3)] if dense else [])
    assert nflag == int(dense)
    report("prn_assign gpu: fast path (compact + match_host) == oracle.assign on %-7s %d (box, type) pairs compared, %d candidates, %d flagged" % (
        name, pairs, int(np.minimum(cn, cap).sum()), nflag))
