"""Gradient clipping by the infinity norm on the device against torch.nn.utils.clip_grad_norm_(params, max_norm, inf) (the
reference Trainer's max_grad_norm option): the max-abs reduction and the clip coefficient bit for bit (NaN / inf included), the
clipped Adam update against torch's clip followed by FusedAdam.step(), the recorded step against the eager step with clipping
(a layer frozen midway included: its stale .grad is reduced and scaled too), and the Trainer's stepper."""
import ctypes
import math

import numpy as np
import pytest
import torch

from helpers import report
from test_round2_gpu import _train_setup

pytestmark = pytest.mark.gpu

INF = float("inf")


def _lib():
    from multiposenet.pytorch_amd import _lib, ops
    return _lib, ops


def _device_clip(flat, runs, max_norm):
    """max |g| over `runs` of the f32 arena `flat` and the clip coefficient, through the C ABI."""
    L, ops = _lib()
    parts = [L.call("mpn_grad_absmax_workspace_bytes", e - s) // 4 for s, e in runs]
    ws = torch.full((sum(parts),), -7.0, dtype=torch.float32, device="cuda")
    out = torch.full((3,), -7.0, dtype=torch.float32, device="cuda")       # [max_norm, total, coef]
    out[0] = max_norm
    k = 0
    for (s, e), n in zip(runs, parts):
        L.call("mpn_grad_absmax_partial", ops.ptr(flat[s:e]), e - s, ops.ptr(ws[k:]), ops.stream_ptr())
        k += n
    L.call("mpn_grad_clip_finalize", ops.ptr(ws), k, ops.ptr(out[0:]), ops.ptr(out[1:]), ops.ptr(out[2:]), ops.stream_ptr())
    torch.cuda.synchronize()
    return out[1].clone(), out[2].clone()


def _torch_clip(tensors, max_norm):
    """What clip_grad_norm_(..., inf) computes (nn/utils/clip_grad.py), on copies."""
    grads = [g.clone() for g in tensors]
    total = torch.nn.utils.get_total_norm(grads, INF)
    coef = torch.clamp(max_norm / (total + 1e-6), max=1.0)
    return total, coef


def _arena(sizes, gaps, fill):
    """A 16-byte aligned f32 arena holding runs of `sizes` floats separated by `gaps` floats of garbage (not reduced)."""
    runs, off = [], 0
    for n, gap in zip(sizes, gaps):
        off = (off + gap + 3) // 4 * 4
        runs.append((off, off + n))
        off += n
    flat = torch.full((off + 8,), 1e30, dtype=torch.float32, device="cuda")
    for s, e in runs:
        flat[s:e] = fill(e - s)
    return flat, runs


@pytest.mark.parametrize("case", ["one", "tail3", "gaps", "max_last", "max_tail", "negative", "zeros", "large"])
def test_absmax_and_coefficient_equal_torch_on_awkward_arenas(case):
    g = torch.Generator().manual_seed(sum(map(ord, case)))

    def rnd(n):
        return (torch.randn(n, generator=g) * 0.01).cuda()
    if case == "one":
        flat, runs = _arena([1], [0], rnd)
    elif case == "tail3":
        flat, runs = _arena([4099], [0], rnd)
    elif case == "gaps":
        flat, runs = _arena([37, 4096 * 3 + 2, 5, 129], [0, 16, 5, 64], rnd)
    elif case == "max_last":
        flat, runs = _arena([4096 * 5], [0], rnd)
        flat[runs[0][1] - 1] = 3.5
    elif case == "max_tail":
        flat, runs = _arena([1000, 70001], [0, 9], rnd)
        flat[runs[1][1] - 2] = -2.25
    elif case == "negative":
        flat, runs = _arena([513, 77], [0, 3], rnd)
        flat[runs[0][0] + 100] = -9.0
    elif case == "zeros":
        flat, runs = _arena([4096 * 2 + 1, 3], [0, 1], lambda n: torch.zeros(n, device="cuda"))
    else:                                         # more partials than one workgroup of the finalize holds, several runs
        flat, runs = _arena([4096 * 1024 * 2 + 13, 4096 * 300 + 1], [0, 4], rnd)
        flat[runs[0][0] + 4096 * 1500 + 7] = -0.75
    tensors = [flat[s:e] for s, e in runs]
    for max_norm in (1e-3, 0.5, 1.0, 100.0):
        total, coef = _device_clip(flat, runs, max_norm)
        t_total, t_coef = _torch_clip(tensors, max_norm)
        assert torch.equal(total, t_total.reshape(())), (case, total.item(), t_total.item())
        assert torch.equal(total, torch.max(torch.stack([x.abs().max() for x in tensors])))
        assert torch.equal(coef, t_coef.reshape(())), (case, max_norm, coef.item(), t_coef.item())


def test_clip_coefficient_is_bit_identical_to_torch_over_random_totals():
    """coef = clamp(max_norm / (total + 1e-6), max=1) for 2 x 10^4 (total, max_norm) pairs on both sides of each other, each pair
    through the reduction and finalize kernels (total placed in a one-element arena), against torch's own expression."""
    L, ops = _lib()
    rng = np.random.default_rng(7)
    n = 20000
    totals = (10.0 ** rng.uniform(-9, 4, n)).astype(np.float32)
    ratio = (10.0 ** rng.uniform(-3, 3, n)).astype(np.float32)
    max_norms = (totals.astype(np.float64) * ratio).astype(np.float32)
    max_norms[::7] = totals[::7]                         # max_norm == total: the coefficient lands just below 1
    totals[:4] = [0.0, 1e-6, 1e-30, 1e30]
    g = torch.from_numpy(totals).cuda()
    mn = torch.from_numpy(max_norms).cuda()
    out = torch.empty(n, 3, dtype=torch.float32, device="cuda")
    ws = torch.empty(n, dtype=torch.float32, device="cuda")
    st = ops.stream_ptr()
    base_o, base_w, base_m = out.data_ptr(), ws.data_ptr(), mn.data_ptr()
    fp = L.lib().mpn_grad_absmax_partial
    ff = L.lib().mpn_grad_clip_finalize
    stage = torch.empty(n, 4, dtype=torch.float32, device="cuda")     # 16-byte aligned copies of the totals
    stage[:, 0] = -g
    for i in range(n):
        assert fp(ctypes.c_void_p(stage.data_ptr() + 16 * i), 1, ctypes.c_void_p(base_w + 4 * i), st) == 0
        assert ff(ctypes.c_void_p(base_w + 4 * i), 1, ctypes.c_void_p(base_m + 4 * i), ctypes.c_void_p(base_o + 12 * i + 4),
                  ctypes.c_void_p(base_o + 12 * i + 8), st) == 0
    torch.cuda.synchronize()
    # torch as clip_grad.py forms it (python float / 0-d f32 tensor = reciprocal * max_norm, then clamp), pair by pair for a
    # sample, vectorised for all (the same f32 operations) once the sample shows the two agree
    sample = torch.stack([torch.clamp(float(max_norms[i]) / (g[i] + 1e-6), max=1.0) for i in range(0, n, 20)])
    want = torch.clamp((g + 1e-6).reciprocal() * mn, max=1.0)
    assert torch.equal(sample, want[::20])
    assert torch.equal(out[:, 1], g)
    bad = (out[:, 2] != want).nonzero().flatten()
    assert bad.numel() == 0, "coef differs from torch at %d pairs, e.g. total %r max_norm %r: %r vs %r" % (
        bad.numel(), g[bad[0]].item(), max_norms[bad[0].item()], out[bad[0], 2].item(), want[bad[0]].item())
    assert (want < 1).any() and (want == 1).any()
    report("grad clip: coefficient bit-identical to torch over %d (total, max_norm) pairs" % n)


@pytest.mark.parametrize("special", ["nan_mid", "nan_tail", "inf", "neg_inf", "inf_and_nan"])
def test_nan_and_inf_follow_torch(special):
    flat, runs = _arena([4096 + 3, 50], [0, 4], lambda n: torch.linspace(-1, 1, n, device="cuda"))
    pos = {"nan_mid": [(runs[0][0] + 2000, math.nan)], "nan_tail": [(runs[0][1] - 1, math.nan)],
           "inf": [(runs[1][0] + 3, INF)], "neg_inf": [(runs[0][0] + 5, -INF)],
           "inf_and_nan": [(runs[0][0] + 9, INF), (runs[1][0], math.nan)]}[special]
    for i, v in pos:
        flat[i] = v
    tensors = [flat[s:e] for s, e in runs]
    total, coef = _device_clip(flat, runs, 0.5)
    t_total, t_coef = _torch_clip(tensors, 0.5)
    torch.testing.assert_close(total, t_total.reshape(()), rtol=0, atol=0, equal_nan=True)
    torch.testing.assert_close(coef, t_coef.reshape(()), rtol=0, atol=0, equal_nan=True)
    # and the scaled gradients: torch's in-place multiply against mpn_scale_by_dev
    L, ops = _lib()
    ref = [x.clone() for x in tensors]
    params = [torch.nn.Parameter(torch.zeros_like(x)) for x in ref]
    for p, x in zip(params, ref):
        p.grad = x
    torch.nn.utils.clip_grad_norm_(params, 0.5, INF)
    c = coef.reshape(1).clone()
    for s, e in runs:
        L.call("mpn_scale_by_dev", ops.ptr(flat[s:e]), e - s, ops.ptr(c), ops.stream_ptr())
    torch.cuda.synchronize()
    for (s, e), p in zip(runs, params):
        torch.testing.assert_close(flat[s:e], p.grad, rtol=0, atol=0, equal_nan=True)


# ------------------------------------------------------------------------------------------------ FusedAdam with clipping
def _model_and_grads(seed):
    m, inputs, gts = _train_setup(50, torch.bfloat16, 2, 64, seed=seed)
    for p in m.parameters():
        p.grad = None
    return m, inputs, gts


def _backward(m, opt, inputs, gts):
    _, saved = m(*inputs)
    loss, _ = m.build_loss(saved, *gts)
    opt.zero_grad()
    loss.backward()


@pytest.mark.parametrize("grad_scale,wd", [(1.0, 0.0), (0.37, 0.0), (1.0, 1e-2), (2.5, 3e-3)])
def test_clipped_adam_equals_torch_clip_then_fused_adam(grad_scale, wd):
    from multiposenet.pytorch_amd.optim import FusedAdam
    m, inputs, gts = _model_and_grads(300)
    state0 = {k: v.clone() for k, v in m.state_dict().items()}
    results = []
    for device_clip in (False, True):
        m.load_state_dict(state0)
        for p in m.parameters():
            p.grad = None
        opt = FusedAdam(m, lr=1e-3, weight_decay=wd)
        opt.grad_scale = grad_scale
        totals = []
        for i, max_norm in enumerate((1e-4, 1e4, 1e-3)):          # clips, does not clip, clips
            _backward(m, opt, inputs, gts)
            if device_clip:
                totals.append(opt.clip_grad_norm_inf_(max_norm).clone())
            else:
                totals.append(torch.nn.utils.clip_grad_norm_(m.parameters(), max_norm, INF))
            opt.step()
        torch.cuda.synchronize()
        results.append((m._arena.flat.clone(), opt._m.clone(), opt._v.clone(), m._arena.grad_flat.clone(), torch.stack(totals)))
    a, b = results
    assert torch.equal(a[4], b[4]), (a[4], b[4])
    assert a[4][0] > 1e-4 and a[4][1] < 1e4
    for x, y, what in zip(a[:4], b[:4], ("parameters", "exp_avg", "exp_avg_sq", "gradients")):
        assert torch.equal(x, y), what
    report("clipped FusedAdam (grad_scale %g, wd %g): parameters, moments, gradients bit-identical to torch clip + step; totals %s"
           % (grad_scale, wd, [float(v) for v in a[4]]))


# ------------------------------------------------------------------------------------------------ recorded step
def _run(m, state0, make_step, batches, clip_at, freeze_at=None):
    from multiposenet.pytorch_amd.optim import FusedAdam
    m.load_state_dict(state0)
    m.train()
    for p in m.parameters():
        p.requires_grad = True
        p.grad = None
    for p in m.prn.parameters():
        p.requires_grad = False
    opt = FusedAdam(m, lr=1e-3)
    step = make_step(m, opt)
    logs = []
    for i, (inputs, gts) in enumerate(batches):
        if freeze_at is not None and i == freeze_at:
            for p in m.fpn.layer1.parameters():
                p.requires_grad = False
            opt = FusedAdam(m, lr=1e-3)
            step = make_step(m, opt)
        step.max_grad_norm = clip_at[i]
        a = [[inputs[0][0].clone(), inputs[0][1]]]
        b = [gts[0]] + [x.clone() for x in gts[1:]]
        loss, log = step(a, b)
        logs.append((float(loss), dict((k, float(v)) for k, v in log.items())))
    torch.cuda.synchronize()
    bn = {k: v.clone() for k, v in m.state_dict().items() if "running_" in k or "num_batches" in k}
    return m._arena.flat.clone(), opt._m.clone(), opt._v.clone(), bn, logs, step, m._arena.grad_flat.clone()


class _EagerClip(object):
    """The Trainer's eager path with clipping (training/trainer.py _Stepper): train_step with torch's clip between backward and
    step."""

    def __init__(self, m, opt):
        self.m, self.opt, self.max_grad_norm = m, opt, None

    def __call__(self, inputs, gts):
        _, saved = self.m(*inputs)
        loss, log = self.m.build_loss(saved, *gts)
        self.opt.zero_grad()
        loss.backward()
        log["max_grad"] = float(torch.nn.utils.clip_grad_norm_(self.m.parameters(), self.max_grad_norm, INF))
        self.opt.step()
        return loss, log


def _pick(subnet, inp, g):
    if subnet == "train_both":
        return inp, g
    if subnet == "keypoint_subnet":
        return [[inp[0][0], subnet]], [subnet, g[1], g[2]]
    return [[inp[0][0], subnet]], [subnet, g[3]]


def _compare(eager, rep, clip_at, what):
    assert rep[5].replays == 4, rep[5].replays                   # one eager pass, one recording, four replays
    totals = [e[1]["max_grad"] for e in eager[4]]
    assert [r[1]["max_grad"] for r in rep[4]] == totals, "max_grad logs differ"
    clipped = [t > c for t, c in zip(totals, clip_at)]
    assert any(clipped) and not all(clipped), (totals, clip_at)
    for x, y, name in zip(eager[:3], rep[:3], ("parameters", "exp_avg", "exp_avg_sq")):
        assert torch.equal(x, y), "%s differ (%s)" % (name, what)
    assert all(torch.equal(eager[3][k], rep[3][k]) for k in eager[3]), "BN statistics differ (%s)" % what
    for (la, da), (lb, db) in zip(eager[4], rep[4]):
        assert list(da) == list(db)
        for k in da:
            assert abs(da[k] - db[k]) <= 2e-6 * max(abs(da[k]), abs(db[k]), 1e-30), (k, da[k], db[k])
    return totals, clipped


@pytest.mark.parametrize("subnet", ["train_both", "keypoint_subnet", "detection_subnet"])
def test_recorded_step_with_clipping_is_bit_identical_to_the_eager_clip(subnet):
    from multiposenet.pytorch_amd.replay import ReplayedTrainStep
    m, inputs, gts = _train_setup(50, torch.bfloat16, 4, 128, seed=210)
    _, inputs_b, gts_b = _train_setup(50, torch.bfloat16, 4, 128, seed=220)
    batches = [_pick(subnet, inputs, gts) if i % 2 == 0 else _pick(subnet, inputs_b, gts_b) for i in range(6)]
    state0 = {k: v.clone() for k, v in m.state_dict().items()}
    # a probe with no clipping gives the gradient norms' scale; then max_norm changes between steps (the recording reads it from
    # device memory): steps 0, 2, 3, 5 clip hard, steps 1 and 4 do not clip
    probe = _run(m, state0, _EagerClip, batches, [1e30] * 6)
    t = [e[1]["max_grad"] for e in probe[4]]
    clip_at = [0.2 * min(t), 5.0 * max(t), 0.2 * min(t), 0.2 * min(t), 5.0 * max(t), 0.2 * min(t)]
    eager = _run(m, state0, _EagerClip, batches, clip_at)
    rep = _run(m, state0, lambda mm, oo: ReplayedTrainStep(mm, oo, max_grad_norm=1.0), batches, clip_at)
    assert rep[5].bucketed_update is False
    assert torch.equal(eager[6], rep[6]), "gradient arena differs"
    totals, clipped = _compare(eager, rep, clip_at, subnet)
    report("recorded step with clipping (%s, R50 128x128 B=4 bf16): 6 steps bit-identical to the eager clip; max_grad %s, clipped %s"
           % (subnet, ["%.4g" % x for x in totals], clipped))


def test_recorded_step_with_clipping_scales_the_stale_gradient_of_a_layer_frozen_midway():
    from multiposenet.pytorch_amd.replay import ReplayedTrainStep
    m, inputs, gts = _train_setup(50, torch.bfloat16, 2, 64, seed=230)
    _, inputs_b, gts_b = _train_setup(50, torch.bfloat16, 2, 64, seed=240)
    batches = [(inputs, gts) if i % 2 == 0 else (inputs_b, gts_b) for i in range(8)]
    state0 = {k: v.clone() for k, v in m.state_dict().items()}
    probe = _run(m, state0, _EagerClip, batches, [1e30] * 8)
    t = [e[1]["max_grad"] for e in probe[4]]
    clip_at = [0.2 * min(t), 5.0 * max(t)] * 4
    eager = _run(m, state0, _EagerClip, batches, clip_at, freeze_at=2)
    frozen = [p for p in m.fpn.layer1.parameters()]
    assert all(p.grad is not None for p in frozen)
    rep = _run(m, state0, lambda mm, oo: ReplayedTrainStep(mm, oo, max_grad_norm=1.0), batches, clip_at, freeze_at=2)
    assert torch.equal(eager[6], rep[6]), "gradient arena (stale gradients of the frozen layer included) differs"
    totals, clipped = _compare(eager, rep, clip_at, "frozen midway")
    for p in m.parameters():
        p.requires_grad = True
    report("recorded step with clipping, fpn.layer1 frozen after 2 steps: bit-identical to the eager clip; max_grad %s"
           % ["%.4g" % x for x in totals])


def test_trainer_stepper_records_clipping_and_logs_max_grad_lazily():
    from multiposenet.pytorch_amd.network import losses
    from multiposenet.pytorch_amd.optim import FusedAdam
    from multiposenet.pytorch_amd.training.trainer import TrainParams, _Stepper
    m, inputs, gts = _train_setup(50, torch.bfloat16, 2, 64, seed=250)
    state0 = {k: v.clone() for k, v in m.state_dict().items()}
    out = {}
    was = losses.set_lazy_log(True)
    try:
        for launch in ("eager", "replay"):
            m.load_state_dict(state0)
            for p in m.parameters():
                p.grad = None
            opt = FusedAdam(m, lr=1e-3)
            st = _Stepper(m, opt, TrainParams(max_grad_norm=2e-3, launch=launch))
            assert (st.fast is not None) == (launch == "replay")
            logs = []
            for i in range(4):
                a = [[inputs[0][0].clone(), inputs[0][1]]]
                b = [gts[0]] + [x.clone() for x in gts[1:]]
                _, log = st(a, b)
                logs.append(log["max_grad"])
            if launch == "replay":
                assert st.fast.replays == 2
                assert all(isinstance(v, losses.LazyFloat) for v in logs)
            torch.cuda.synchronize()
            out[launch] = ([float(v) for v in logs], m._arena.flat.clone())
    finally:
        losses.set_lazy_log(was)
    assert out["eager"][0] == out["replay"][0]
    assert torch.equal(out["eager"][1], out["replay"][1])
    report("Trainer stepper with max_grad_norm: recorded, max_grad (LazyFloat) == eager %s" % out["eager"][0])
