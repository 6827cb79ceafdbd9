"""Element-wise parity of the loss and PRN head kernels (csrc/losses.hip) against float64.

Every kernel is launched through the wrapper production uses (losses.mse_forward_raw / mse_backward_raw / mse_train_raw /
focal_forward_raw / focal_backward_raw, _lib.call("mpn_...") for the PRN pieces) and EVERY element it writes is compared with the
float64 reference of tests/loss_ref.py under the bound derived there (nothing fitted; tests/test_loss_parity_cpu.py shows that the
bounds accept an fp32 model of each kernel and reject the modelled faults).  Discrete or copied quantities — max / min of the
heat-map, npos, nvalid, the bad counts, dropout masks, every zero a kernel must write — compare exactly.  One report line per
comparison (worst err / bound and where).  The shapes are the smallest that reach each structural edge (the case tables of
loss_ref.py name the edge each one is there for)."""
import numpy as np
import pytest
import torch

import loss_ref as L
from loss_ref import BF, F32, H16, f32

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests selected but no GPU is visible"
    from multiposenet.pytorch_amd import _lib
    _lib.lib()
    n = torch.get_num_threads()
    torch.set_num_threads(min(n, 16))
    yield
    torch.set_num_threads(n)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(t):
    return t.detach().float().cpu().double().numpy() if t.dtype != torch.float32 else t.detach().cpu().numpy()


# ------------------------------------------------------------------------------------------------ heat-map MSE
@pytest.mark.parametrize("name", list(L.MSE_CASES))
def test_mse_forward_backward(name):
    from multiposenet.pytorch_amd.network import losses
    case = L.mse_case(name)
    ref = L.mse_ref(case)
    store = [dev(s) for s in case["store"]]
    pm = [s[..., :C] for s, C in zip(store, L.MSE_C)]                            # pixel strides 19 and 32 mixed in one call
    assert [p.stride(2) for p in pm] == list(L.MSE_STRIDE)
    heat, wgt = dev(case["gt"]), dev(case["w"])
    out = losses.mse_forward_raw(pm, heat, wgt)
    gs = torch.tensor([float(case["gs"])], dtype=torch.float32, device="cuda")
    grads = losses.mse_backward_raw(pm, heat, wgt, gs, case["need"])
    torch.cuda.synchronize()
    route = "%d px, %d chunks" % (case["B"] * case["H"] * case["W"], -(-case["B"] * case["H"] * case["W"] * 18 // L.MSE_CHUNK))
    L.check_mse_out("mse " + name, host(out), ref, L.MSE_FWD_LEVELS, route)
    L.check_mse_grads("mse " + name, [None if g is None else host(g.permute(0, 2, 3, 1)) for g in grads], ref, case["need"], route)


@pytest.mark.parametrize("dtype", [F32, BF, H16])
@pytest.mark.parametrize("name", list(L.TRAIN_CASES))
def test_one_pass_heatmap_loss(name, dtype):
    from multiposenet.pytorch_amd import ops
    from multiposenet.pytorch_amd.network import losses
    case = L.train_case(name)
    ref = L.train_ref(case)
    levels = [ops.Act(dev(x), C) for x, C in zip(case["lv"], L.MSE_C)]
    heat, wgt = dev(case["heat"]), dev(case["w"])
    assert losses.mse_train_supported(levels, heat, wgt)
    gs = torch.tensor([float(case["gs"]), 0.0], dtype=torch.float32, device="cuda")
    out, grads = losses.mse_train_raw(levels, heat, wgt, gs, dtype)
    torch.cuda.synchronize()
    assert all(g.t.dtype == dtype and g.t.shape == a.t.shape for g, a in zip(grads, levels))
    L.check_train("one-pass mse " + name, host(out), [host(g.t) for g in grads], ref, dtype, route=str(dtype).split(".")[1])


# ------------------------------------------------------------------------------------------------ focal loss
@pytest.mark.parametrize("key", L.focal_cases(), ids=L.focal_tag)
def test_focal_forward_backward(key):
    from multiposenet.pytorch_amd.network import losses
    case = L.make_focal(key)                                                     # asserts the generator conditions on the reference
    ref = L.focal_eval(case)
    out, saved = losses.focal_forward_raw(dev(case["cls"]), dev(case["reg"]), dev(case["anchors"])[None], dev(case["anno"]))
    gs = torch.tensor([float(v) for v in L.FOCAL_GS], dtype=torch.float32, device="cuda")
    dcls, dreg = losses.focal_backward_raw(saved, gs)
    torch.cuda.synchronize()
    got = dict(out=host(out), per_img=host(saved[4]), bad=host(saved[5]) if len(saved) > 5 else None, dcls=host(dcls), dreg=host(dreg))
    assert (len(saved) > 5) == (key[2] > 1)
    L.check_focal(L.focal_tag(key), got, ref)
    # an image with annotations and no positive anchor: the classification term is divided by 1, dreg is all zeros and finite
    for b in range(min(key[4], 4)):
        if ref["per_img"][b, 3] > 0 and ref["per_img"][b, 2] == 0:
            assert (got["dreg"][b] == 0).all() and np.isfinite(got["dcls"][b]).all()


# ------------------------------------------------------------------------------------------------ sigmoid
@pytest.mark.parametrize("n", L.SIG_N)
def test_sigmoid_forward_backward(n):
    from multiposenet.pytorch_amd import ops
    from multiposenet.pytorch_amd._lib import call
    x, dp, p = L.sigmoid_case(n)
    xd = dev(x)
    y = torch.full_like(xd, float("nan"))
    call("mpn_sigmoid_forward", ops.ptr(xd), ops.ptr(y), n, ops.stream_ptr())
    inplace = xd.clone()
    call("mpn_sigmoid_forward", ops.ptr(inplace), ops.ptr(inplace), n, ops.stream_ptr())
    dl = torch.full_like(xd, float("nan"))
    dpd, pd = dev(dp), dev(p)
    call("mpn_sigmoid_backward", ops.ptr(dpd), ops.ptr(pd), ops.ptr(dl), n, ops.stream_ptr())
    torch.cuda.synchronize()
    L.check_sigmoid("sigmoid n=%d" % n, host(y), x, "out of place")
    L.check_sigmoid("sigmoid n=%d" % n, host(inplace), x, "in place")
    L.check_sigmoid_bwd("sigmoid backward n=%d" % n, host(dl), dp, p)


# ------------------------------------------------------------------------------------------------ PRN softmax
@pytest.mark.parametrize("padded", [0, 1])
@pytest.mark.parametrize("cols", L.SM_COLS)
def test_prn_softmax_forward_backward(cols, padded):
    from multiposenet.pytorch_amd import ops
    from multiposenet.pytorch_amd._lib import call
    c = L.softmax_case(cols, padded)
    a, res, dp, pre = dev(c["a"]), dev(c["res"]), dev(c["dp"]), dev(c["pre"])
    for relu in (1, 0):
        out = torch.full((L.SM_ROWS, cols), float("nan"), device="cuda")
        call("mpn_add_softmax_rows", ops.ptr(a), c["stride"], ops.ptr(res), ops.ptr(out), L.SM_ROWS, cols, relu, ops.stream_ptr())
        torch.cuda.synchronize()
        L.check_softmax("softmax cols=%d" % cols, host(out), c["a"], c["res"], cols, relu, "a_stride=%d relu=%d" % (c["stride"], relu))
    p = host(out)
    for with_pre in (True, False):
        dl = torch.full((L.SM_ROWS, cols), float("nan"), device="cuda")
        call("mpn_softmax_rows_backward", ops.ptr(out), ops.ptr(dp), ops.ptr(pre) if with_pre else None, c["stride"], ops.ptr(dl),
             L.SM_ROWS, cols, ops.stream_ptr())
        torch.cuda.synchronize()
        L.check_softmax_bwd("softmax backward cols=%d" % cols, host(dl), p, c["dp"], c["pre"] if with_pre else None, cols,
                            "pre_stride=%d" % c["stride"] if with_pre else "no pre")


# ------------------------------------------------------------------------------------------------ BCE
@pytest.mark.parametrize("n", L.BCE_N)
def test_bce_forward_backward(n):
    from multiposenet.pytorch_amd import ops
    from multiposenet.pytorch_amd._lib import call
    p, y = L.bce_case(n)
    pd, yd = dev(p), dev(y)
    chunks = call("mpn_bce_chunks", n)
    assert chunks == -(-n // 4096)
    part = ops.workspace(chunks * 4, pd.device, slot=7)
    res = torch.full((1,), float("nan"), device="cuda")
    call("mpn_bce_mean_forward", ops.ptr(pd), ops.ptr(yd), n, ops.ptr(part), chunks, ops.ptr(res), ops.stream_ptr())
    gs = torch.tensor([L.BCE_GS], dtype=torch.float32, device="cuda")
    dp = torch.full_like(pd, float("nan"))
    call("mpn_bce_mean_backward", ops.ptr(pd), ops.ptr(yd), ops.ptr(dp), n, ops.ptr(gs), ops.stream_ptr())
    torch.cuda.synchronize()
    ref, bound = L.bce_ref(p, y)
    assert np.isfinite(host(res)).all()                                          # p exactly 0 / 1 against labels 1 / 0: the -100 clamp
    L.chk("bce mean n=%d" % n, host(res), ref, [], extra_abs=bound, route="%d chunks" % chunks)
    gref, terms = L.bce_bwd_ref(p, y, L.BCE_GS)
    assert np.isfinite(host(dp)).all()
    L.chk("bce backward n=%d" % n, host(dp), gref, terms)


# ------------------------------------------------------------------------------------------------ dropout
@pytest.mark.parametrize("dtype", [F32, BF, H16])
@pytest.mark.parametrize("n", L.DROP_N)
def test_dropout_mask_and_survivors(n, dtype):
    from multiposenet.pytorch_amd import ops
    from multiposenet.pytorch_amd._lib import call
    x = (torch.from_numpy(L.rng(n).standard_normal(n).astype(f32)) * 3).to(dtype)
    xd = x.cuda()
    masks = {}
    for p in L.DROP_P:
        for seed in (0x123456789ABCDEF, 7):
            y = torch.full_like(xd, float("nan"))
            call("mpn_dropout", ops.ptr(xd), ops.ptr(y), n, seed, float(p), ops.dtype_code(dtype), ops.stream_ptr())
            torch.cuda.synchronize()
            ref, keep = L.dropout_ref(x, seed, p)
            L.same("dropout n=%d p=%.1f seed=%d %s" % (n, p, seed, str(dtype).split(".")[1]), y.cpu().view(torch.uint8), ref.view(torch.uint8))
            masks[p, seed] = keep
        if p == 0:
            assert torch.equal(y.cpu().view(torch.uint8), x.view(torch.uint8))   # the identity
    if n >= 255:
        assert not torch.equal(masks[0.5, 7], masks[0.5, 0x123456789ABCDEF])     # two seeds, two masks


# ------------------------------------------------------------------------------------------------ step log
@pytest.mark.parametrize("which", ["kp8 only", "det2 only", "both"])
def test_step_log(which):
    from multiposenet.pytorch_amd import ops
    from multiposenet.pytorch_amd._lib import call
    kp8 = (np.arange(1, 9, dtype=f32) / f32(3)) if which != "det2 only" else None
    det2 = np.array([0.7, 0.2000001], f32) if which != "kp8 only" else None
    before = np.full(13, -5.0, f32)
    logv = dev(before)
    kd, dd = None if kp8 is None else dev(kp8), None if det2 is None else dev(det2)
    call("mpn_step_log", ops.ptr(kd), ops.ptr(dd), ops.ptr(logv), ops.stream_ptr())
    torch.cuda.synchronize()
    L.same("step log " + which, logv.cpu(), L.step_log_ref(kp8, det2, before))
