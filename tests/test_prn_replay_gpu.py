"""The recorded PRN training step on the device: the three new kernels against what they replace, byte for byte, and the step
itself (replay.ReplayedTrainStep with 'prn_subnet') against batch_processor.train_step.

* mpn_dropout_dev writes the bytes of mpn_dropout(seed = (state + k) mod 2^64); mpn_dropout_advance moves the word.
* mpn_prn_pack writes the bytes of the eager construction in poseNet.prn_forward (zeros + copy_ / cast_lowp / view).
* mpn_prn_head_train: dl equals the bytes of mpn_add_softmax_rows -> mpn_bce_mean_backward -> mpn_softmax_rows_backward -> the
  cast / pad copy on the same device operands; the loss is within prn_head_ref.head_loss_ref's bound of float64.
* the recorded step leaves parameters and both Adam moments torch.equal to the eager step's, through a reseed, a second batch
  size, a change of the dropout probability and an eager step in between.

Every output is poisoned with NaN (all-ones bytes) before the launch that must fill it."""
from collections import OrderedDict

import numpy as np
import pytest
import torch

import loss_ref as L
import prn_head_ref as H
from loss_ref import BF, F32, H16, U, f32

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
DTYPES = [F32, BF, H16]


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


def poisoned(shape, dtype):
    t = torch.empty(shape, dtype=dtype, device="cuda")
    t.view(torch.uint8).fill_(0xFF)          # NaN in f32 / bf16 / f16
    return t


def raw(t):
    return t.detach().contiguous().cpu().view(torch.uint8).numpy()


def word(v):
    return torch.tensor([v - (1 << 64) if v >> 63 else v], dtype=torch.int64).cuda()


def name(dtype):
    return str(dtype).split(".")[1]


# ------------------------------------------------------------------------------------------------ dropout from a device word
@pytest.mark.parametrize("dtype", DTYPES)
def test_dropout_dev_equals_dropout_with_the_summed_seed(dtype):
    from multiposenet.pytorch_amd import ops
    from multiposenet.pytorch_amd._lib import call
    code = ops.dtype_code(dtype)
    for n in L.DROP_N:
        x = torch.from_numpy(L.rng(n).standard_normal(n).astype(f32)).to(dtype).cuda()
        for p in L.DROP_P:
            for state in (7, 0x123456789ABCDEF, M64):
                st = word(state)
                for k in (1, 2):
                    y, want = poisoned(n, dtype), poisoned(n, dtype)
                    call("mpn_dropout_dev", ops.ptr(x), ops.ptr(y), n, ops.ptr(st), k, float(p), code, ops.stream_ptr())
                    call("mpn_dropout", ops.ptr(x), ops.ptr(want), n, (state + k) & M64, float(p), code, ops.stream_ptr())
                    L.same("dropout_dev n=%d p=%.1f state=%#x k=%d %s" % (n, p, state, k, name(dtype)), y.view(torch.uint8).cpu(),
                           want.view(torch.uint8).cpu().numpy())
                    if p == 0.5 and n == 5000:
                        assert 0.4 < float((y != 0).float().mean()) < 0.6          # a mask, not all or nothing
                assert raw(st).view(np.uint64)[0] == state                          # the launches only read the word
                call("mpn_dropout_advance", ops.ptr(st), 2, ops.stream_ptr())
                assert int(raw(st).view(np.uint64)[0]) == (state + 2) & M64


def test_dropout_dev_masks_differ_between_k_and_follow_the_advance():
    from multiposenet.pytorch_amd import ops
    from multiposenet.pytorch_amd._lib import call
    n = 5000
    x = torch.ones(n, device="cuda")
    st = word(M64 - 1)
    ys = []
    for k in (1, 2, 3):
        y = poisoned(n, F32)
        call("mpn_dropout_dev", ops.ptr(x), ops.ptr(y), n, ops.ptr(st), k, 0.5, 0, ops.stream_ptr())
        ys.append(y)
    assert not torch.equal(ys[0], ys[1]) and not torch.equal(ys[1], ys[2])
    call("mpn_dropout_advance", ops.ptr(st), 2, ops.stream_ptr())
    y = poisoned(n, F32)
    call("mpn_dropout_dev", ops.ptr(x), ops.ptr(y), n, ops.ptr(st), 1, 0.5, 0, ops.stream_ptr())
    assert torch.equal(y, ys[2])                                                    # (state + 2) + 1 == state + 3, across the wrap
    keep = L.dropout_keep(n, (M64 - 1 + 3) & M64, 0.5)
    assert np.array_equal(y.cpu().numpy() != 0, keep)


# ------------------------------------------------------------------------------------------------ input packing
def _pack_input(B, n):
    x = L.rng(n).standard_normal((B, n)).astype(f32)
    sp = np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 65519.9, 65520.0, 7e4, 1e-8, 6e-8, -0.0, 0.0,
                   3.3e38, -1e-40, 1e-45], f32)                                     # ties of both 16-bit formats, f16 overflow / underflow
    x[0, :sp.size] = sp
    x[B - 1, n - sp.size:] = -sp
    return x


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [8568, 34272])
def test_prn_pack_equals_the_eager_construction(n, dtype):
    from multiposenet.pytorch_amd import ops
    from multiposenet.pytorch_amd._lib import call
    B = 3
    npad = ops.round_up(n, 32)
    assert npad - n == (8 if n == 8568 else 0)
    res = dev(_pack_input(B, n))
    # poseNet.prn_forward's construction
    if npad != n:
        want = torch.zeros((B, 1, 1, npad), dtype=dtype, device="cuda")
        want[:, 0, 0, :n].copy_(res)
    elif ops.is16(dtype):
        want = torch.empty((B, 1, 1, n), dtype=dtype, device="cuda")
        ops.cast_lowp(res, want)
    else:
        want = res.view(B, 1, 1, n)
    got = poisoned((B, 1, 1, npad), dtype)
    call("mpn_prn_pack", ops.ptr(res), ops.ptr(got), B, n, npad, ops.dtype_code(dtype), ops.stream_ptr())
    torch.cuda.synchronize()
    L.same("prn_pack n=%d %s" % (n, name(dtype)), got.view(torch.uint8).cpu(), want.contiguous().view(torch.uint8).cpu().numpy())
    if npad != n:
        assert not raw(got.view(B, npad)[:, n:]).any()


# ------------------------------------------------------------------------------------------------ loss head
HEAD_CASES = [("cols=%d %s" % (c, "padded" if p else "dense"), c, p) for c in L.SM_COLS for p in (0, 1)] + [("saturating 3x8568", 8568, 1)]
_chain = {}


def _head_case(tag, cols, padded):
    """Operands on the device and the chain's f32 results (p, dl), computed once per case and left unchanged."""
    if tag not in _chain:
        from multiposenet.pytorch_amd import ops
        from multiposenet.pytorch_amd._lib import call
        if tag.startswith("saturating"):
            c = H.saturating_case()
        else:
            c = L.softmax_case(cols, padded)
            c["y"] = H.softmax_label(c)
        rows = c["a"].shape[0]
        a, res, y = dev(c["a"]), dev(c["res"]), dev(c["y"])
        gs = torch.ones(1, device="cuda")
        p, dp, dl = poisoned((rows, cols), F32), poisoned((rows, cols), F32), poisoned((rows, cols), F32)
        st = ops.stream_ptr()
        call("mpn_add_softmax_rows", ops.ptr(a), c["stride"], ops.ptr(res), ops.ptr(p), rows, cols, 1, st)
        call("mpn_bce_mean_backward", ops.ptr(p), ops.ptr(y), ops.ptr(dp), rows * cols, ops.ptr(gs), st)
        call("mpn_softmax_rows_backward", ops.ptr(p), ops.ptr(dp), ops.ptr(a), c["stride"], ops.ptr(dl), rows, cols, st)
        torch.cuda.synchronize()
        _chain[tag] = (c, a, res, y, gs, p, dl)
    return _chain[tag]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tag,cols,padded", HEAD_CASES, ids=[c[0] for c in HEAD_CASES])
def test_head_train_equals_the_chain(tag, cols, padded, dtype):
    from multiposenet.pytorch_amd import ops
    from multiposenet.pytorch_amd._lib import call
    c, a, res, y, gs, p, dl32 = _head_case(tag, cols, padded)
    rows, npad = c["a"].shape[0], ops.round_up(cols, 32)
    # the cast / pad copy at the end of poseNet.prn_forward's backward closure
    if npad != cols:
        want = torch.zeros((rows, 1, 1, npad), dtype=dtype, device="cuda")
        want[:, 0, 0, :cols].copy_(dl32)
    elif ops.is16(dtype):
        want = torch.empty((rows, 1, 1, cols), dtype=dtype, device="cuda")
        ops.cast_lowp(dl32, want)
    else:
        want = dl32.view(rows, 1, 1, cols)
    for gscale in (gs, None):                                                       # a device 1.0 and the NULL default
        got, part, loss = poisoned((rows, 1, 1, npad), dtype), poisoned(rows, F32), poisoned(1, F32)
        call("mpn_prn_head_train", ops.ptr(a), c["stride"], ops.ptr(res), ops.ptr(y), ops.ptr(gscale), ops.ptr(got), rows, cols, npad,
             ops.dtype_code(dtype), ops.ptr(part), ops.ptr(loss), ops.stream_ptr())
        torch.cuda.synchronize()
        err, bound = H.check_head("head %s %s" % (tag, name(dtype)), raw(got).reshape(rows, -1), float(loss.cpu()[0]),
                                  raw(want).reshape(rows, -1), p.cpu().numpy(), c["y"], cols, npad)
        print("head %s %s: loss err %.3e bound %.3e" % (tag, name(dtype), err, bound))
        assert torch.isfinite(part).all()
    if tag.startswith("saturating"):
        pn = p.cpu().numpy()
        assert (pn * (1 - pn) < 1e-12).sum() > 100 and (pn == 0).sum() > 1000 and (c["a"][:, :cols] == 0).sum() > 1000
        assert torch.isfinite(dl32).all() and float(dl32.abs().max()) > 0


def test_head_train_gradient_scale_is_read_from_the_device():
    from multiposenet.pytorch_amd import ops
    from multiposenet.pytorch_amd._lib import call
    c, a, res, y, gs, p, dl32 = _head_case("cols=257 padded", 257, 1)
    rows, cols, npad = 3, 257, 288
    g2 = torch.full((1,), 1.7, device="cuda")
    dp, want = poisoned((rows, cols), F32), poisoned((rows, cols), F32)
    call("mpn_bce_mean_backward", ops.ptr(p), ops.ptr(y), ops.ptr(dp), rows * cols, ops.ptr(g2), ops.stream_ptr())
    call("mpn_softmax_rows_backward", ops.ptr(p), ops.ptr(dp), ops.ptr(a), c["stride"], ops.ptr(want), rows, cols, ops.stream_ptr())
    got, part, loss = poisoned((rows, npad), F32), poisoned(rows, F32), poisoned(1, F32)
    call("mpn_prn_head_train", ops.ptr(a), c["stride"], ops.ptr(res), ops.ptr(y), ops.ptr(g2), ops.ptr(got), rows, cols, npad, 0,
         ops.ptr(part), ops.ptr(loss), ops.stream_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(raw(got[:, :cols]), raw(want)) and not raw(got[:, cols:]).any() and not torch.equal(want, dl32)


# ------------------------------------------------------------------------------------------------ the recorded step
_prn_models = {}


def _model(dtype):
    """poseNet(50, prn_node_count=64, prn_coeff=1) with everything but the PRN frozen, and its initial PRN state."""
    from multiposenet.pytorch_amd.network.posenet import poseNet
    if dtype not in _prn_models:
        _prn_models.clear()
        torch.cuda.empty_cache()
        torch.manual_seed(3)
        m = poseNet(50, prn_node_count=64, prn_coeff=1, compute_dtype=dtype).cuda()
        for n, p in m.named_parameters():
            p.requires_grad = n.startswith("prn.")
        _prn_models[dtype] = (m, {k: v.detach().clone() for k, v in m.state_dict().items() if k.startswith("prn.")})
    m, state0 = _prn_models[dtype]
    m.load_state_dict(state0, strict=False)
    m.train()
    m.prn.drop.p = 0.5
    m._engine._drop_calls = 0                                                       # both runs start the eager seed sequence at the same point
    return m


def _batch(i, B):
    g = torch.Generator().manual_seed(1000 + i)
    x = torch.rand((B, 28, 18, 17), generator=g) * (torch.rand((B, 28, 18, 17), generator=g) < 0.05).float()
    y = (torch.rand((B, 28, 18, 17), generator=g) < 0.02).float() * torch.rand((B, 28, 18, 17), generator=g)
    return x.cuda(), y.cuda()


def _loss_gap_bound(l):
    """Both routes sum the same non-negative float32 terms (the gradient bytes are equal, so the probabilities are), in different
    orders.  bce_ref's bound with sum |term| = n L and |1 - y| qa <= 2^-24 per element is ((R_LOG + 3) + levels + 1) u L + u;
    the eager loss has levels = BCE_LEVELS (4 096-element chunks), the head's ceil(8568 / 256) + BLOCK_LEVELS.  Their distance
    is at most the sum of the two."""
    l = abs(float(l))
    one = lambda levels: ((L.R_LOG + 3) + levels + 1) * U * l + U
    return one(L.BCE_LEVELS) + one(H.head_levels(8568))


def _run(dtype, recorded, seed, script):
    """Run `script` (a list of operations) through train_step or ReplayedTrainStep; returns the snapshots it asks for."""
    from multiposenet.pytorch_amd.optim import FusedAdam
    from multiposenet.pytorch_amd.replay import ReplayedTrainStep
    from multiposenet.pytorch_amd.training.batch_processor import train_step
    m = _model(dtype)
    opt = FusedAdam(m, lr=1e-3)
    step = ReplayedTrainStep(m, opt) if recorded else (lambda inputs, gts: train_step(m, opt, inputs, gts))
    torch.manual_seed(seed)
    out = OrderedDict(losses=[], snaps=[], replays=[], entries=[])
    i = 0
    for op in script:
        if op[0] == "seed":
            torch.manual_seed(op[1])
        elif op[0] == "p":
            m.prn.drop.p = op[1]
        elif op[0] == "snap":
            torch.cuda.synchronize()
            out["snaps"].append((m._arena.flat.detach().clone(), opt._m.clone(), opt._v.clone()))
        else:
            x, y = _batch(i, op[1])
            i += 1
            fn = (lambda inputs, gts: train_step(m, opt, inputs, gts)) if op[0] == "eager" else step
            loss, log = fn([[x, "prn_subnet"]], ["prn_subnet", y])
            assert list(log) == ["PRN loss"]
            out["losses"].append((float(loss.detach()), float(log["PRN loss"])))
            if recorded:
                out["replays"].append(step.replays)
                out["entries"].append(list(step._entries.values()))          # (the objects: an id could be reused)
    out["step"] = step
    return out


SCRIPT = ([("step", 3)] * 3 + [("seed", 4242)] + [("step", 3)] * 3 + [("snap",)]      # six steps, reseeded after the third
          + [("step", 2), ("step", 2), ("step", 3), ("snap",)]                        # a second batch size: its own recording
          + [("eager", 3), ("step", 3), ("snap",)]                                    # a plain eager step between replays
          + [("p", 0.25), ("step", 3), ("step", 3), ("snap",)])                       # another dropout probability: re-recorded


@pytest.mark.parametrize("dtype", [BF, F32])
def test_recorded_prn_step_equals_the_eager_step(dtype):
    eager = _run(dtype, False, 11, SCRIPT)
    rec = _run(dtype, True, 11, SCRIPT)
    # 1 eager pass, 1 recording, 4 replays | B = 2: eager pass, recording, then B = 3 replays | train_step, replay | new p: the first
    # call records again at once (the signature has been seen), the second replays
    assert rec["replays"][:6] == [0, 0, 1, 2, 3, 4], rec["replays"]
    assert rec["replays"][6:9] == [4, 4, 5] and rec["replays"][9:11] == [5, 6] and rec["replays"][11:] == [6, 7], rec["replays"]
    ent = rec["entries"]
    assert len(ent[5]) == 1 and len(ent[7]) == 2 and len(ent[11]) == 2
    assert all(ent[11][-1] is not e for e in ent[10]), "drop.p changed: the B = 3 step must be recorded again"
    for k, (a, b) in enumerate(zip(eager["snaps"], rec["snaps"])):
        for what, ta, tb in zip(("parameters", "exp_avg", "exp_avg_sq"), a, b):
            assert torch.isfinite(tb).all()
            assert torch.equal(ta, tb), "%s differ after phase %d (%d elements)" % (what, k, int((ta != tb).sum()))
    for (le, _), (lr, lg) in zip(eager["losses"], rec["losses"]):
        assert lr == lg and np.isfinite(lr) and lr > 0
        assert abs(le - lr) <= _loss_gap_bound(le), "loss %.9e (eager) vs %.9e (recorded): gap %.3e > %.3e" % (le, lr, abs(le - lr),
                                                                                                           _loss_gap_bound(le))
    # the host counter kept pace: every step, eager or recorded, drew two seeds
    assert rec["step"].model._engine._drop_calls == 2 * len(rec["losses"])
    # the parameters moved, and a different seed moves them elsewhere (a dropout that silently vanished would not notice the seed)
    other = _run(dtype, True, 12, SCRIPT[:8])
    assert not torch.equal(other["snaps"][0][0], rec["snaps"][0][0])
    again = _run(dtype, True, 11, SCRIPT[:8])
    assert torch.equal(again["snaps"][0][0], rec["snaps"][0][0])


def test_recorded_prn_step_in_eval_mode_launches_no_dropout():
    from multiposenet.pytorch_amd import _lib
    from multiposenet.pytorch_amd.optim import FusedAdam
    from multiposenet.pytorch_amd.replay import ReplayedTrainStep
    from multiposenet.pytorch_amd.training.batch_processor import train_step
    res = []
    for recorded in (False, True):
        m = _model(BF)
        m.prn.drop.eval()
        opt = FusedAdam(m, lr=1e-3)
        step = ReplayedTrainStep(m, opt) if recorded else (lambda i, g: train_step(m, opt, i, g))
        for i in range(3):
            x, y = _batch(i, 3)
            step([[x, "prn_subnet"]], ["prn_subnet", y])
        torch.cuda.synchronize()
        res.append(m._arena.flat.detach().clone())
        assert m._engine._drop_calls == 0
        if recorded:
            assert step.replays == 1
            names = [getattr(fn, "__name__", "") for fn, _, is_c in next(iter(step._entries.values())).tape if is_c]
            assert "mpn_prn_head_train" in names and "mpn_prn_pack" in names
            assert not any(n.startswith("mpn_dropout") for n in names)
    assert torch.equal(res[0], res[1])


def test_recorded_prn_list_holds_the_new_launches_and_no_eager_head():
    from multiposenet.pytorch_amd.optim import FusedAdam
    from multiposenet.pytorch_amd.replay import ReplayedTrainStep
    m = _model(BF)
    step = ReplayedTrainStep(m, FusedAdam(m, lr=1e-3))
    for i in range(2):
        x, y = _batch(i, 3)
        step([[x, "prn_subnet"]], ["prn_subnet", y])
    names = [getattr(fn, "__name__", "") for fn, _, is_c in next(iter(step._entries.values())).tape if is_c]
    assert names.count("mpn_dropout_dev") == 4 and names.count("mpn_dropout_advance") == 1 and names[-1] == "mpn_dropout_advance"
    assert names.count("mpn_prn_pack") == 1 and names.count("mpn_prn_head_train") == 1
    for old in ("mpn_dropout", "mpn_add_softmax_rows", "mpn_bce_mean_forward", "mpn_bce_mean_backward", "mpn_softmax_rows_backward"):
        assert old not in names, old


# ------------------------------------------------------------------------------------------------ Trainer
def test_trainer_takes_the_recorded_path_for_the_prn(tmp_path):
    """PRNDeviceLoader -> batch_processor -> Trainer, one epoch of four batches, launch='replay' against launch='eager'."""
    from multiposenet.pytorch_amd.datasets import DevicePRNBatcher, PRNDeviceLoader, PRNSampleSet
    from multiposenet.pytorch_amd.network import losses
    from multiposenet.pytorch_amd.optim import FusedAdam
    from multiposenet.pytorch_amd.training.batch_processor import batch_processor
    from multiposenet.pytorch_amd.training.trainer import Trainer, TrainParams
    from test_prn_train_cpu import NK, THR, annotations
    ss = PRNSampleSet(annotations(), NK, coeff=1, threshold=THR)
    assert len(ss) >= 2
    got = {}
    was_lazy = losses.LAZY_LOG
    try:
        for launch in ("eager", "replay"):
            m = _model(BF)
            loader = PRNDeviceLoader(ss, DevicePRNBatcher(coeff=1, threshold=THR), 2, seed=5, indices=[i % len(ss) for i in range(8)])
            assert len(loader) == 4
            P = TrainParams(exp_name="prn_" + launch, subnet_name="prn_subnet", batch_size=2, max_epoch=1, save_dir=str(tmp_path / launch),
                            print_freq=2, val_nbatch_end_epoch=0, launch=launch)
            P.optimizer = FusedAdam(m, lr=1e-3)
            torch.manual_seed(21)
            tr = Trainer(m, P, batch_processor, loader, None)
            tr.train()
            torch.cuda.synchronize()
            got[launch] = m._arena.flat.detach().clone()
            if launch == "replay":
                assert tr._step.fast is not None and tr._step.fast.replays == 2          # 1 eager pass + 1 recording + 2 replays
            else:
                assert tr._step.fast is None
            assert m._engine._drop_calls == 8
    finally:
        losses.set_lazy_log(was_lazy)
    assert torch.isfinite(got["replay"]).all() and torch.equal(got["eager"], got["replay"])
