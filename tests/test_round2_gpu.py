"""Round-2 GPU tests: fp16 arithmetic (BASELINE config 5), segmented batch NMS, the hipGraph-captured training step,
FusedAdam checkpoint state, full-size configuration checks (cfg3 train step at 480x480 B=32, cfg4 at B=8, cfg5 at
640x640 B=64 fp16) and two-process data parallelism on the device."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import ROOT, gold, report
from test_model_gpu import close, get_model, load_he, t

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests selected but no GPU is visible"
    from multiposenet.pytorch_amd import _lib
    _lib.lib()


# ------------------------------------------------------------------------------------------------ fp16
def test_f16_forward_against_reference_goldens():
    """dtype code 2 (v_mfma_f32_16x16x32_f16, fp32 accumulate): heat-maps and detection outputs of the REAL reference
    (fixtures g2) within fp16 bounds — rel-L2 <= 5e-3 (10-bit mantissa; bf16's gate is 3e-2)."""
    from multiposenet.pytorch_amd import synthetic as weightgen
    for layers in (50, 101):
        g = gold("g2_forward_r%d.npz" % layers)
        model = get_model(layers, torch.float16)
        model.eval()
        for b, h, w in ((2, 64, 64), (2, 128, 128)):
            tag = "eval_%dx%dx%d" % (b, h, w)
            img = t(weightgen.gen_images(1, b, h, w)).cuda()
            with torch.no_grad():
                pred, saved = model([img, "keypoint_subnet"])
                ref = t(g["kp_pred_" + tag])
                close("f16 R%d kp pred %s" % (layers, tag), pred, ref, 2e-2 * float(ref.abs().max()), 5e-3)
                _, ds = model([img, "detection_subnet"])
                close("f16 R%d det cls %s" % (layers, tag), ds[0], t(g["det_cls_" + tag]), 5e-3, 5e-3)
                ref = t(g["det_reg_" + tag])
                close("f16 R%d det reg %s" % (layers, tag), ds[1], ref, 2e-2 * float(ref.abs().max()), 5e-3)
                heat, det = model([img, "both"])
                ref = t(g["both_heat_" + tag])
                close("f16 R%d both heat %s" % (layers, tag), heat, ref, 2e-2 * float(ref.abs().max()), 5e-3)
                assert abs(det[0].shape[0] - g["both_scores_" + tag].shape[0]) <= max(2, g["both_scores_" + tag].shape[0] // 20)


def test_f16_kernels_against_fp32_oracle_arithmetic():
    """conv forward / dgrad / wgrad and BN through the C ABI in f16 vs the same operands rounded to f16 and computed in
    float64 on the CPU."""
    from helpers import check_close, from_act, rnd, rng_normal, to_act, w_krsc
    from multiposenet.pytorch_amd import ops
    dt = torch.float16
    for (B, C, H, W, O, R, stride, pad) in ((2, 64, 20, 24, 96, 3, 1, 1), (3, 128, 15, 15, 256, 1, 1, 0), (2, 64, 17, 19, 64, 3, 2, 1)):
        x = rnd(dt, rng_normal(1, B, C, H, W))
        w = rnd(dt, rng_normal(2, O, C, R, R) * 0.05)
        ref = torch.nn.functional.conv2d(x.double(), w.double(), stride=stride, padding=pad).float()
        y, _ = ops.conv_forward(to_act(x, dt), w_krsc(w, dt), O, R, R, stride, pad)
        check_close("f16 conv fwd %dx%d s%d %d->%d" % (R, R, stride, C, O), from_act(y), rnd(dt, ref), dt)
        # wgrad (LDS-DMA kernel, f16 instantiation): dW = sum_p dY (x) X
        dy = rnd(dt, rng_normal(3, *ref.shape) * 0.1)
        xd = x.double().requires_grad_(True)
        wd = w.double().requires_grad_(True)
        torch.nn.functional.conv2d(xd, wd, stride=stride, padding=pad).backward(dy.double())
        dw = torch.zeros(O, R, R, C, dtype=torch.float32, device="cuda")
        ops.conv_wgrad(to_act(x, dt), to_act(dy, dt), dw.view(-1), O, R, R, stride, pad)
        check_close("f16 wgrad %dx%d s%d %d->%d" % (R, R, stride, C, O), dw.cpu().permute(0, 3, 1, 2), wd.grad.float(), dt, factor=0.5)
        # dgrad through the transposed operand
        opad = (O + 31) // 32 * 32
        wt = torch.zeros(C, R, R, opad, dtype=dt, device="cuda")
        ops.weight_transpose(w.permute(0, 2, 3, 1).contiguous().cuda(), wt, O, R * R, C, opad)
        g = ops.Act(torch.empty(B, H, W, C, dtype=dt, device="cuda"), C)
        ops.conv_forward(to_act(dy, dt), wt, C, R, R, stride, pad, mode=1, out_hw=(H, W), cin=opad, out=g)
        check_close("f16 dgrad %dx%d s%d %d->%d" % (R, R, stride, C, O), from_act(g), rnd(dt, xd.grad.float()), dt)


# ------------------------------------------------------------------------------------------------ segmented NMS
def test_batched_nms_equals_per_image_nms_and_oracle():
    from multiposenet.pytorch_amd import ops
    from multiposenet.pytorch_amd._lib import call
    from oracle import nms_oracle
    rs = np.random.RandomState(3)
    counts = [0, 1, 63, 64, 65, 700, 0, 1500, 129]
    B, cap = len(counts), 1600
    dets = np.zeros((B, cap, 5), np.float32)
    for b, n in enumerate(counts):
        xy = rs.uniform(0, 300, (n, 2)); wh = rs.uniform(8, 150, (n, 2))
        sc = np.round(rs.uniform(0.05, 1.0, (n, 1)), 2)            # rounded: plenty of score ties
        dets[b, :n] = np.concatenate([xy, xy + wh, sc], 1)
    d = torch.from_numpy(dets).cuda()
    cnt = torch.tensor(counts, dtype=torch.int32, device="cuda")
    nmax = max(counts)
    for mode, name in ((0, "gpu"), (1, "cpu")):
        keep = torch.full((B, nmax), -1, dtype=torch.int64, device="cuda")
        num = torch.full((B,), -1, dtype=torch.int64, device="cuda")
        ws = torch.empty(call("mpn_nms_batched_workspace_bytes", B, nmax), dtype=torch.uint8, device="cuda")
        call("mpn_nms_batched", ops.ptr(d), cap * 5, ops.ptr(cnt), B, nmax, 0.5, mode, ops.ptr(keep), nmax, ops.ptr(num), ops.ptr(ws), ops.stream_ptr())
        torch.cuda.synchronize()
        for b, n in enumerate(counts):
            k = int(num[b])
            got = keep[b, :k].cpu().numpy()
            want = nms_oracle.nms(dets[b, :n], 0.5, name) if n else np.zeros(0, np.int64)
            assert np.array_equal(got, want), "image %d (n=%d, mode %s): batched NMS differs from the oracle" % (b, n, name)
            if n:
                single = ops.nms(d[b, :n].contiguous(), 0.5, mode).cpu().numpy()
                assert np.array_equal(got, single)
    report("segmented NMS: %d images with %s candidates bit-exact vs per-image launches and the C oracle, both modes" % (B, counts))


def test_cfg5_640_batch64_f16_all_images():
    """BASELINE config 5: R101 inference 640x640, batch 64, fp16, with NMS for every image.  Size-independent checks at
    the FULL size: shapes, boxes inside the image, scores sorted and above 0.05, three sampled images bit-identical to
    running them alone (the reference semantics, posenet.py:236-285), and exactly two host read-backs for the whole
    batch in the detection post-processing (none per image)."""
    from multiposenet.pytorch_amd import synthetic as weightgen
    m = get_model(101, torch.float16)
    m.eval()
    B, S = 64, 640
    img = t(weightgen.gen_images(41, B, S, S)).cuda()
    calls = {"n": 0}
    orig_tolist, orig_item = torch.Tensor.tolist, torch.Tensor.item

    def tolist(self):
        calls["n"] += 1 if self.is_cuda else 0
        return orig_tolist(self)

    def item(self):
        calls["n"] += 1 if self.is_cuda else 0
        return orig_item(self)
    torch.Tensor.tolist, torch.Tensor.item = tolist, item
    try:
        with torch.no_grad():
            heat, dets = m.forward_all_images(img)
        torch.cuda.synchronize()
    finally:
        torch.Tensor.tolist, torch.Tensor.item = orig_tolist, orig_item
    assert calls["n"] == 2, "detection post-processing made %d device read-backs for the batch (expected 2)" % calls["n"]
    assert heat.shape == (B, 18, 160, 160) and len(dets) == B and torch.isfinite(heat).all()
    kept = [int(d[0].numel()) for d in dets]
    assert max(kept) > 0
    for scores, cls_idx, boxes in dets:
        if scores.numel():
            assert float(scores.min()) > 0.05 and bool((scores[:-1] >= scores[1:]).all())
            assert float(boxes.min()) >= 0.0 and float(boxes.max()) <= float(S)
    with torch.no_grad():
        for b in (0, 37, 63):
            h1, d1 = m([img[b:b + 1].contiguous(), "both"])
            assert torch.equal(h1, heat[b:b + 1])
            assert d1[0].shape == dets[b][0].shape and torch.equal(d1[0].to(dets[b][0].device), dets[b][0]) and torch.equal(d1[2].to(dets[b][2].device), dets[b][2])
    report("cfg5 (R101 640x640 B=64 f16): heat-maps finite, kept boxes per image min/median/max = %d/%d/%d, 3 images bit-identical to single-image runs, 2 host read-backs"
           % (min(kept), sorted(kept)[B // 2], max(kept)))


# ------------------------------------------------------------------------------------------------ hipGraph step + Adam state
def _train_setup(layers, dtype, B, S, seed=50):
    from multiposenet.pytorch_amd import synthetic as weightgen
    m = get_model(layers, dtype)
    for p in m.prn.parameters():
        p.requires_grad = False
    m.train()
    img = t(weightgen.gen_images(seed, B, S, S)).cuda()
    heat, wgt = (t(a).cuda() for a in weightgen.gen_keypoint_gt(seed + 1, B, S // 4, S // 4))
    anno = t(weightgen.gen_boxes_gt(seed + 2, B, S)).cuda()
    return m, [[img, "train_both"]], ["train_both", heat, wgt, anno]


def test_fused_adam_state_interchanges_with_torch_adam_on_the_device():
    """Take 2 steps with FusedAdam, hand its state_dict to torch.optim.Adam (and back): the third step of both optimizers
    moves the parameters identically (<= 1e-7 abs: same fp32 formula, different association)."""
    from multiposenet.pytorch_amd.optim import FusedAdam
    from multiposenet.pytorch_amd.training.batch_processor import train_step
    m, inputs, gts = _train_setup(50, torch.float32, 2, 64, seed=80)
    opt = FusedAdam(m, lr=1e-3)
    for _ in range(2):
        train_step(m, opt, inputs, gts)
    sd = copy.deepcopy(opt.state_dict())
    snapshot = {k: v.clone() for k, v in m.state_dict().items()}
    train_step(m, opt, inputs, gts)
    fused = m._arena.flat.clone()
    # same third step with torch.optim.Adam restored from the FusedAdam state
    m.load_state_dict(snapshot)
    params = [p for p in m.parameters() if p.requires_grad]
    ref = torch.optim.Adam(params, lr=1e-3)
    ref.load_state_dict(copy.deepcopy(sd))        # torch adopts device tensors without copying: keep `sd` pristine
    train_step(m, ref, inputs, gts)
    err = (m._arena.flat - fused).abs().max().item()
    report("FusedAdam -> torch.optim.Adam state hand-over: third-step parameter difference %.3e" % err)
    assert err <= 1e-6
    # and back: a fresh FusedAdam restored from torch's state dict
    sd_t = copy.deepcopy(ref.state_dict())
    m.load_state_dict(snapshot)
    opt2 = FusedAdam(m, lr=1e-3)
    opt2.load_state_dict(sd)
    train_step(m, opt2, inputs, gts)
    assert torch.equal(m._arena.flat, fused)
    assert opt2.step_count() == 3 and float(sd_t["state"][0]["step"]) == 3.0
    # torch's own state dict (after ITS third step) loads too: moments equal FusedAdam's after three steps
    opt3 = FusedAdam(m, lr=1e-3)
    opt3.load_state_dict(sd_t)
    assert opt3.step_count() == 3
    assert float((opt3._m - opt2._m).abs().max()) <= 1e-6 * float(opt2._m.abs().max()) + 1e-12


# ------------------------------------------------------------------------------------------------ full-size configurations
def test_cfg3_train_step_480_batch32_bf16_full_size():
    """BASELINE config 3 at its exact per-GPU size (R101 full posenet, 480x480, 32 images, bf16): losses and the whole
    gradient arena finite and bit-reproducible; the bf16 loss within 2 % of the same step computed with the exact-fp32
    kernels (whose arithmetic is pinned to the reference at fixture size); with frozen BatchNorm statistics the bf16
    heat-maps are within rel-L2 3e-2 of fp32.  (With BATCH statistics and He-random weights bf16 rounding noise is
    amplified ~6 % per bottleneck by the renormalisation — 0.3 % after the stem, 13 % after layer3, the same at 128x128
    batch 8 and at 480x480 batch 32, uniform over images: tools/stage_diff.py — so that case is gated on the loss and the
    gradient direction, not on element-wise heat-map agreement.)"""
    from multiposenet.pytorch_amd.network.posenet import poseNet
    m, inputs, gts = _train_setup(101, torch.bfloat16, 32, 480, seed=90)
    bn_state = {k: v.clone() for k, v in m.state_dict().items() if "running_" in k or "num_batches" in k}

    def run():
        m.load_state_dict(bn_state, strict=False)
        m._arena.ensure_grads()
        m._arena.grad_flat.zero_()
        pred, saved = m(*inputs)
        loss, log = poseNet.build_loss(saved, *gts)
        loss.backward()
        torch.cuda.synchronize()
        return pred.detach().float().clone(), loss.detach().clone(), m._arena.grad_flat.clone(), log
    p0, l0, g0, log0 = run()
    p1, l1, g1, _ = run()
    assert p0.shape == (32, 18, 120, 120)
    assert torch.isfinite(l0) and torch.isfinite(g0).all() and float(g0.abs().max()) > 0
    assert torch.equal(l0, l1) and torch.equal(g0, g1) and torch.equal(p0, p1)
    m.compute_dtype = torch.float32
    try:
        p32, l32, g32, _ = run()
    finally:
        m.compute_dtype = torch.bfloat16
    rel = abs(float(l0) - float(l32)) / abs(float(l32))
    rl2 = float((p0 - p32).norm() / p32.norm())
    gcos = float(torch.dot(g0, g32) / (g0.norm() * g32.norm()))
    report("cfg3 full size (R101 480x480 B=32, batch-stat BN): bf16 loss %.5f vs fp32 %.5f (rel %.2e), heat-map rel-L2 %.2e, gradient cosine %.5f"
           % (float(l0), float(l32), rel, rl2, gcos))
    assert rel <= 2e-2 and rl2 <= 0.3 and gcos >= 0.9
    m.eval()
    with torch.no_grad():
        pe16, _ = m(*inputs)
        m.compute_dtype = torch.float32
        try:
            pe32, _ = m(*inputs)
        finally:
            m.compute_dtype = torch.bfloat16
    rl2e = float((pe16.float() - pe32.float()).norm() / pe32.float().norm())
    report("cfg3 full size, frozen BN: bf16 vs fp32 heat-map rel-L2 %.2e" % rl2e)
    assert rl2e <= 3e-2


def test_cfg4_800_batch8_full_size():
    """BASELINE config 4 at its exact per-GPU size (R101 full posenet, 800x800, 8 images, bf16; A = 120 087 anchors)."""
    from multiposenet.pytorch_amd.network.posenet import poseNet
    m, inputs, gts = _train_setup(101, torch.bfloat16, 8, 800, seed=95)
    bn_state = {k: v.clone() for k, v in m.state_dict().items() if "running_" in k or "num_batches" in k}
    outs = []
    for _ in range(2):
        m.load_state_dict(bn_state, strict=False)
        m._arena.ensure_grads()
        m._arena.grad_flat.zero_()
        pred, (ks, ds) = m(*inputs)
        assert pred.shape == (8, 18, 200, 200) and ds[0].shape == (8, 120087, 1)
        loss, log = poseNet.build_loss((ks, ds), *gts)
        loss.backward()
        torch.cuda.synchronize()
        outs.append((loss.detach().clone(), m._arena.grad_flat.clone()))
    assert torch.isfinite(outs[0][0]) and torch.isfinite(outs[0][1]).all()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    report("cfg4 full size (R101 800x800 B=8 bf16): train step finite and bit-reproducible, loss %.4f" % outs[0][0].item())


# ------------------------------------------------------------------------------------------------ data parallel on the device
def test_two_rank_data_parallel_equals_global_batch_on_device():
    """Two processes (RCCL over two GPUs when the box has them, otherwise both ranks share the one GPU and the buckets go
    through gloo): with frozen BatchNorm the average of the two shards' gradients equals the gradient of the global
    batch computed by one process; both ranks end with bit-identical gradients and the same bucket schedule."""
    import socket
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    import tempfile
    out = tempfile.mkdtemp(prefix="mpn_ddp2_")          # the arenas are ~170 MB each: not for gpurun_out/
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), MPN_DDP_OUT=out, HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "ddp_worker.py")], env=dict(env, RANK=str(r), WORLD_SIZE="2", LOCAL_RANK=str(r)),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    logs = [p.communicate(timeout=600)[0] for p in procs]
    for r, (p, lg) in enumerate(zip(procs, logs)):
        assert p.returncode == 0, "rank %d failed:\n%s" % (r, lg[-3000:])
    res = [np.load(os.path.join(out, "rank%d.npz" % r)) for r in range(2)]
    assert np.array_equal(res[0]["grad"], res[1]["grad"]), "ranks disagree after the all-reduce"
    assert np.array_equal(res[0]["buckets"], res[1]["buckets"]) and res[0]["launched"] == res[1]["launched"] == len(res[0]["buckets"])
    ref, got = res[0]["global_grad"].astype(np.float64), res[0]["grad"].astype(np.float64)
    rel = np.linalg.norm(got - ref) / np.linalg.norm(ref)
    report("2-rank DDP on device (%s): mean of shard gradients vs global-batch gradient rel-L2 %.3e, %d buckets"
           % (str(res[0]["backend"]), rel, len(res[0]["buckets"])))
    assert rel <= 1e-4
    assert abs(float(res[0]["loss_mean"]) - float(res[0]["global_loss"])) <= 1e-5 * abs(float(res[0]["global_loss"]))


def test_two_rank_recorded_step_equals_the_eager_data_parallel_step():
    """The recorded launch list contains the reducer's collectives: four optimizer steps of a 2-rank job (1 eager + 1 recording +
    2 replays) end with the same parameters, bit for bit, as four eager data-parallel steps — on both ranks."""
    import socket
    import tempfile
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    out = tempfile.mkdtemp(prefix="mpn_ddp2r_")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), MPN_DDP_OUT=out, MPN_DDP_MODE="replay", HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "ddp_worker.py")], env=dict(env, RANK=str(r), WORLD_SIZE="2", LOCAL_RANK=str(r)),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    logs = [p.communicate(timeout=600)[0] for p in procs]
    for r, (p, lg) in enumerate(zip(procs, logs)):
        assert p.returncode == 0, "rank %d failed:\n%s" % (r, lg[-3000:])
    res = [np.load(os.path.join(out, "rank%d.npz" % r)) for r in range(2)]
    for r in range(2):
        assert int(res[r]["replays"]) == 2
        # round 6: the recorded step's Adam ran bucket by bucket behind each all-reduce, the eager job's as one
        # launch after backward — and the parameters still agree bit for bit
        assert int(res[r]["bucketed"]) == 1 and int(res[r]["bucket_updates"]) == int(res[r]["buckets"]) >= 2
        assert np.array_equal(res[r]["eager_params"], res[r]["replay_params"]), "rank %d: recorded step diverged from the eager step" % r
        assert np.allclose(res[r]["eager_loss"], res[r]["replay_loss"], rtol=2e-6, atol=0)      # heat-map loss: f32 summation order only
    assert np.array_equal(res[0]["replay_params"], res[1]["replay_params"]), "ranks hold different parameters after four steps"
    assert not np.array_equal(res[0]["eager_loss"], res[1]["eager_loss"]), "the two ranks should see different shards"
    report("2-rank recorded step (%s): parameters bit-identical to the eager data-parallel job after 4 steps on both ranks"
           % str(res[0]["backend"]))


# ------------------------------------------------------------------------------------------------ pyramid towers
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_pyramid_towers_equal_the_per_level_launches(dtype):
    """The RetinaNet towers share weights over p3..p7 (posenet.py:327-328): running each layer ONCE over the whole pyramid
    (MpnConvParams.nseg) gives bit-identical outputs (same k-order per output element whatever the tile) and the same
    gradients up to the summation order of the split weight-gradient reduction."""
    from multiposenet.pytorch_amd.network.posenet import poseNet
    m, inputs, gts = _train_setup(50, dtype, 2, 160, seed=140)
    res = []
    for pyramid in (False, True):
        m._engine.pyramid_towers = pyramid
        m._arena.ensure_grads()
        m._arena.grad_flat.zero_()
        pred, (ks, ds) = m(*inputs)
        loss, log = poseNet.build_loss((ks, ds), *gts)
        loss.backward()
        torch.cuda.synchronize()
        res.append((ds[0].detach().clone(), ds[1].detach().clone(), loss.detach().clone(), m._arena.grad_flat.clone()))
    m._engine.pyramid_towers = True
    (c0, r0, l0, g0), (c1, r1, l1, g1) = res
    assert torch.equal(c0, c1) and torch.equal(r0, r1) and torch.equal(l0, l1)
    rel = float((g0 - g1).norm() / g0.norm())
    report("pyramid towers (%s): outputs and loss bit-identical to per-level launches, gradient arena rel-L2 %.2e" % (str(dtype), rel))
    assert rel <= (1e-6 if dtype == torch.float32 else 2e-3)
    # the tower weights themselves: every level contributed
    w = m.regressionModel.conv2.weight
    i = m._arena.index[id(w)]
    seg = slice(m._arena.offsets[i], m._arena.offsets[i] + m._arena.sizes[i])
    assert float((g0[seg] - g1[seg]).norm() / g0[seg].norm()) <= (1e-6 if dtype == torch.float32 else 2e-3)


@pytest.mark.parametrize("dtype,mode", [(torch.bfloat16, "train"), (torch.float32, "train"), (torch.bfloat16, "frozen_affine")])
def test_bn_backward_statistics_in_the_dgrad_epilogue(dtype, mode):
    """The launch that completes dz of a BatchNorm also produces (sum g, sum g*xhat) per pixel tile (MpnConvParams.bnb_*), so
    mpn_bn_bwd_reduce's pass over dz / y / z disappears.  Same training step with the fusion on and off: loss identical, the
    whole gradient arena equal up to the summation order of the per-channel statistics."""
    from multiposenet.pytorch_amd.network.posenet import poseNet
    m, inputs, gts = _train_setup(101, dtype, 2, 160, seed=150)
    if mode == "frozen_affine":
        m.freeze_bn()                    # eval-mode statistics, gamma/beta still trained: statistics are needed for dgamma/dbeta only
    res = []
    calls = []
    from multiposenet.pytorch_amd import _lib
    orig = _lib.call

    def counting(name, *a):
        if name == "mpn_bn_bwd_reduce":
            calls[-1] += 1
        return orig(name, *a)
    import multiposenet.pytorch_amd.ops as ops_mod
    ops_mod.call = counting
    try:
        for fused in (False, True):
            calls.append(0)
            m._engine.fuse_bn_stats = fused
            bn_state = {k: v.clone() for k, v in m.state_dict().items() if "running_" in k or "num_batches" in k} if not res else res[0][2]
            m.load_state_dict(bn_state, strict=False)
            m._arena.ensure_grads()
            m._arena.grad_flat.zero_()
            pred, saved = m(*inputs)
            loss, log = poseNet.build_loss(saved, *gts)
            loss.backward()
            torch.cuda.synchronize()
            res.append((loss.detach().clone(), m._arena.grad_flat.clone(), bn_state))
    finally:
        ops_mod.call = orig
        m._engine.fuse_bn_stats = True
        m.train()
    (l0, g0, _), (l1, g1, _) = res
    assert torch.equal(l0, l1)
    nbn = len(m._bns)
    assert calls[0] == nbn and calls[1] <= 8, "separate reductions: %d without fusion (%d BN layers), %d with" % (calls[0], nbn, calls[1])
    rel = float((g0 - g1).norm() / g0.norm())
    report("BN backward statistics in the dgrad epilogue (%s, %s): %d -> %d separate reduction launches, gradient arena rel-L2 %.2e"
           % (str(dtype), mode, calls[0], calls[1], rel))
    assert rel <= (2e-5 if dtype == torch.float32 else 1e-2)


@pytest.mark.parametrize("dtype,mode,size", [(torch.bfloat16, "train", 160), (torch.float32, "train", 160), (torch.bfloat16, "frozen_affine", 160),
                                             (torch.bfloat16, "train", 320)])
def test_bn_finalize_inside_the_conv_launch(dtype, mode, size):
    """The last workgroup to finish a channel tile reduces that tile's partial statistics and writes the BatchNorm coefficients
    (MpnConvParams.fin_*): mpn_bn_finalize_train / mpn_bn_bwd_finalize launches disappear from the step.  Same step with the
    in-launch finalize on and off: same loss, running statistics and gradients up to the rounding of one double reduction, and
    the ticket counters are back at zero.  160x160: every layer has <= 64 pixel tiles and finalizes in the launch; 320x320: the larger
    layers keep their finalize launches (the two-level in-launch form of round 3 was measured slower and removed)."""
    from multiposenet.pytorch_amd.network.posenet import poseNet
    from multiposenet.pytorch_amd import _lib
    import multiposenet.pytorch_amd.ops as ops_mod
    m, inputs, gts = _train_setup(101, dtype, 2, size, seed=151)
    if mode == "frozen_affine":
        m.freeze_bn()
    orig = _lib.call
    calls = []

    def counting(name, *a):
        if name in ("mpn_bn_finalize_train", "mpn_bn_bwd_finalize"):
            calls[-1] += 1
        return orig(name, *a)
    ops_mod.call = counting
    res = []
    bn0 = {k: v.clone() for k, v in m.state_dict().items() if "running_" in k or "num_batches" in k}
    try:
        for fused in (False, True):
            calls.append(0)
            m._engine.fuse_bn_finalize = fused
            m.load_state_dict(bn0, strict=False)
            m._arena.ensure_grads()
            m._arena.grad_flat.zero_()
            pred, saved = m(*inputs)
            loss, log = poseNet.build_loss(saved, *gts)
            loss.backward()
            torch.cuda.synchronize()
            res.append((loss.detach().clone(), m._arena.grad_flat.clone(),
                        {k: v.clone() for k, v in m.state_dict().items() if "running_" in k}))
    finally:
        ops_mod.call = orig
        m._engine.fuse_bn_finalize = True
        m.train()
    (l0, g0, r0), (l1, g1, r1) = res
    assert int(ops_mod.fin_counters(g0.device).abs().sum()) == 0, "ticket counters not reset"
    rel_l = abs(float(l0) - float(l1)) / abs(float(l0))
    rel = float((g0 - g1).norm() / g0.norm())
    rs = max(float((r0[k].float() - r1[k].float()).abs().max() / r0[k].float().abs().max().clamp_min(1e-12)) for k in r0)
    report("BN finalize inside the conv launch (%s, %s, %dx%d): %d -> %d finalize launches; loss rel %.1e, gradient arena rel-L2 %.2e, "
           "running statistics max rel %.1e" % (str(dtype), mode, size, size, calls[0], calls[1], rel_l, rel, rs))
    # (<= 11 of 208 stay separate at 160x160: three of them since round 4 — the stride-2 input gradients run as four parity-class launches,
    #  whose shared partial table is reduced by a finalize launch)
    assert calls[0] >= len(m._bns) and (calls[1] <= 11 if size <= 160 else calls[1] < calls[0])
    assert rel_l <= (1e-6 if dtype == torch.float32 else 1e-3) and rs <= 1e-5
    assert rel <= (2e-5 if dtype == torch.float32 else 1e-2)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_folded_batchnorm_inference_equals_the_separate_passes(dtype):
    """Inference with frozen statistics folds BatchNorm (+ReLU, + the residual add of a Bottleneck, fpn.py:28-34) into the
    conv epilogue (act code 3).  Same network, fold on / off: fp32 agrees to rounding (the fold skips one rounding of y),
    fp16 within its own precision."""
    from multiposenet.pytorch_amd import synthetic as weightgen
    m = get_model(101, dtype)
    m.eval()
    img = t(weightgen.gen_images(160, 2, 192, 160)).cuda()
    outs = []
    for fold in (False, True):
        m._engine.fold_bn = fold
        with torch.no_grad():
            heat, _ = m([img, "keypoint_subnet"])
            _, ds = m([img, "detection_subnet"])
        outs.append((heat.float().clone(), ds[0].float().clone(), ds[1].float().clone()))
    m._engine.fold_bn = True
    lim = 2e-5 if dtype == torch.float32 else 5e-3
    for name, a, b in zip(("heat", "cls", "reg"), outs[0], outs[1]):
        rel = float((a - b).norm() / b.norm())
        report("folded BN (%s) %s: rel-L2 vs separate passes %.2e" % (str(dtype), name, rel))
        assert rel <= lim


# ------------------------------------------------------------------------------------------------ shared pixel tile of the 3x3 kernel
@pytest.mark.parametrize("geom", [(3, 4, 4, 64, 64), (2, 8, 8, 256, 128), (2, 15, 15, 64, 256), (1, 30, 30, 128, 128), (2, 17, 33, 64, 64),
                                  (1, 60, 60, 64, 64), (32, 30, 30, 256, 256), (4, 115, 113, 256, 256)])
@pytest.mark.parametrize("mode", [0, 1])
def test_3x3_kernel_with_shared_pixel_tile_is_exact_at_the_borders(geom, mode):
    """conv_igemm_s3_kernel lands the pixel tile of a kernel row once and reads it at three column shifts; the image's left / right
    border is a per-lane select, the top / bottom border a DMA-time zero fill.  bf16 operands, fp32 output (no output rounding):
    against torch's fp32 convolution of the same bf16-rounded operands the result may differ by accumulation order only — any
    border slip would be an O(1) error.  Forward and stride-1 dgrad, tiles that span several image lines (W = 4, 8, 15), lines
    that span tiles (W = 33, 60), images that end inside a tile.  Channel tile (pick_tc, asserted): 64 rows for the six small
    geometries, 128 rows for (32, 30, 30, 256, 256) (225 pixel tiles: below the 400 workgroups of the 256-row rule), 256 rows for
    (4, 115, 113, 256, 256) (407 pixel tiles, the last one 12 pixels) in both modes."""
    import torch.nn.functional as F
    from multiposenet.pytorch_amd import ops
    from helpers import from_act, rnd, rng_normal, to_act, w_krsc
    B, H, W, Cin, Cout = geom
    dt = torch.bfloat16
    x = rnd(dt, rng_normal(31, B, Cin, H, W))
    w = rnd(dt, rng_normal(32, Cout, Cin, 3, 3) / (Cin * 9) ** 0.5)
    if mode == 0:
        ref = F.conv2d(x, w, None, stride=1, padding=1)
        run = lambda: ops.conv_forward(to_act(x, dt), w_krsc(w, dt), Cout, 3, 3, 1, 1, out_f32=True)
    else:
        dy = rnd(dt, rng_normal(33, B, Cout, H, W))
        ref = F.conv_transpose2d(dy, w, None, stride=1, padding=1)          # = dgrad of the forward convolution
        kc = 32
        cout_pad = (Cout + kc - 1) // kc * kc
        wm = w.permute(0, 2, 3, 1).contiguous().cuda()
        wt = torch.empty((Cin, 3, 3, cout_pad), dtype=dt, device="cuda")
        ops.weight_transpose(wm, wt, Cout, 9, Cin, cout_pad)
        run = lambda: ops.conv_forward(to_act(dy, dt), wt, Cin, 3, 3, 1, 1, mode=1, out_hw=(H, W), cin=cout_pad, out_f32=True)
    ops.KERNEL_EVENTS.enable()
    try:
        out, _ = run()
        names = [r[0] for r in ops.KERNEL_EVENTS.rec]
    finally:
        ops.KERNEL_EVENTS.disable()
    torch.cuda.synchronize()
    tc = {(32, 30, 30, 256, 256): 128, (4, 115, 113, 256, 256): 256}.get(geom, 64)
    assert names == ["conv_igemm_s3_kernel<bf16, %d, 128, true, false>" % tc], names
    got = from_act(out).float()
    err = float((got - ref).abs().max() / ref.abs().max())
    report("3x3 shared-pixel-tile kernel %s mode %d: max err / max |ref| = %.2e" % (str(geom), mode, err))
    assert err <= 2e-5
