"""Engine tier on the MI355X (tests/engine_ref.py): every section of R50 through the engine's own composition method and
Engine.run_backward — side stream, joins and completion reports included — under every configuration of the case table, against
the oracle: in fp32 element by element against its float64 run under 16 x its float32 run's deviation, in bf16 against its
storage-rounding model under the gates of the two teacher-forced tests; and the exact properties of the bookkeeping in both.

The odd-size sections (S1o, S5o, S7K1o) run the stem, the two pyramids and the detection head at the extents of an image that is no
multiple of 32.  The keypoint head and 'both' have no such section: the reference's keypoint head concatenates exact x2 / x4 / x8
maps and raises at any other size, so there is nothing to compare with."""
import pytest
import torch

import engine_ref as er
from engine_ref import BF, F32, F64
from helpers import report

pytestmark = pytest.mark.gpu

_state = {}          # dtype -> model; "orig_head": {id(model): its K = 1 head}
_refs = {}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests selected but no GPU is visible"
    from multiposenet.pytorch_amd import _lib
    _lib.lib()
    yield
    for dt in (F32, BF):          # the models are test_model_gpu's: hand them back as get_model leaves them
        m = _state.get(dt)
        if m is not None:
            _use_head(m, 1)
            for p in m.parameters():
                p.requires_grad = True
            m.train()
    _state.clear()
    _refs.clear()


def _cdt(case):
    return F32 if case[0] == "fp32" else BF


def model_for(dtype):
    """One R50 per dtype for the whole module, with the 'he' weights (running statistics away from the identity)."""
    if dtype not in _state:
        from test_model_gpu import get_model
        _state[dtype] = get_model(50, dtype)
    return _state[dtype]


def _use_head(m, K):
    from multiposenet.pytorch_amd.engine import num_classes
    from multiposenet.pytorch_amd.network.posenet import ClassificationModel
    if num_classes(m.classificationModel) != K:
        heads = _state.setdefault("orig_head", {})
        if K == 1:
            m.classificationModel = heads[id(m)]
        else:
            heads.setdefault(id(m), m.classificationModel)
            head = ClassificationModel(256, num_classes=K)
            pre = "classificationModel."
            head.load_state_dict({n[len(pre):]: v for n, v in er.gen_state("S7K3", F32).items() if n.startswith(pre)})
            m.classificationModel = head
    m._prepare(torch.zeros(1, device="cuda"))          # (re)build the arena if the head changed; refresh the 16-bit operand copies


def reference(kind, section, stats, variant, times=1, classes=False):
    """Oracle runs shared by the cases: kind "f64" / "f32" (reference, yardstick) or "bf16" (the rounding model)."""
    key = (kind, section, stats, variant, times, classes)
    if key not in _refs:
        seed = er.SEEDS[(section, stats)]
        if kind == "bf16":
            _refs[key] = er.run_oracle(section, seed, F32, stats == "batch", variant, quant=BF, conv2_classes=classes, times=times)
        else:
            _refs[key] = er.run_oracle(section, seed, F64 if kind == "f64" else F32, stats == "batch", variant, times=times)
    return _refs[key]


class Counting(dict):
    """ctx.lazy_res / ctx.bnb that remember every key put into them."""

    def __init__(self):
        dict.__init__(self)
        self.seen = set()

    def __setitem__(self, k, v):
        self.seen.add(k)
        dict.__setitem__(self, k, v)


class Rec(object):
    """The bucket schedule Engine.run_backward reports to."""

    def __init__(self):
        self.launch_stream = None
        self.ready, self.began, self.finished, self.on_bucket = {}, 0, 0, []

    def begin(self, on_bucket):
        self.began += 1
        self.on_bucket.append(on_bucket)

    def param_ready(self, p):
        self.ready[id(p)] = self.ready.get(id(p), 0) + 1

    def finish(self):
        self.finished += 1


def _act(x, dtype, needs_grad=False):
    from multiposenet.pytorch_amd import ops
    return ops.Act(x.permute(0, 2, 3, 1).contiguous().to(dtype).cuda(), x.shape[1], needs_grad=needs_grad)


def _nchw(a):
    return a.t[..., : a.C].float().cpu().permute(0, 3, 1, 2).contiguous()


def compose(m, ctx, section, xs, cdt, need):
    """The section through the engine's own composition -> (leaf Acts, outputs, slots, conv launches of S6, the activation between the
    two blocks of S1 - S4): outputs are Acts (S1 - S5, gradients go in with ctx.set_grad) or API tensors (S6 / S7, gradients go in by
    slot name)."""
    from multiposenet.pytorch_amd import ops
    eng, f = m._engine, m.fpn
    dev = torch.device("cuda", torch.cuda.current_device())
    section = er.base(section)          # an odd-size section is its base section's composition on other extents
    if section == "S1":
        c = eng.stem(ctx, xs[0].cuda())
        c = eng.bottleneck(ctx, c, f.layer1[0])
        return [None], [eng.bottleneck(ctx, c, f.layer1[1])], None, None, c
    leaves = [_act(x, cdt, need) for x in xs]
    if section in ("S2", "S3", "S4"):
        layer = getattr(f, "layer%s" % section[1])
        c = eng.bottleneck(ctx, leaves[0], layer[0])
        return leaves, [eng.bottleneck(ctx, c, layer[1])], None, None, c
    if section == "S5":
        x, c4, c3, c2 = leaves
        c5 = eng.bottleneck(ctx, x, f.layer4[2])
        kp = eng.kp_pyramid(ctx, c2, c3, c4, c5)
        det = eng.det_pyramid(ctx, c3, c4, c5)
        eng.join_forward_side(ctx, dev)
        return leaves, kp + det, None, None, None
    if section == "S6":
        ev = ops.KERNEL_EVENTS
        ev.enable()
        ev.detail = True
        try:
            pred, saved = eng.keypoint_head(ctx, leaves, True)
        finally:
            ev.disable()
            ev.detail = False
        route = [r[0] for r in ev.rec]
        ev.rec = []
        return leaves, saved + [pred], ["k0", "k1", "k2", "k3", "pred"], route, None
    cls, reg = eng.detection_head(ctx, leaves)
    return leaves, [cls, reg], ["cls", "reg"], None, None


def run_device(case, times=1):
    """-> (result in run_oracle's form, observations for check_exact, conv2-by-classes route taken)."""
    from multiposenet.pytorch_amd.engine import Ctx
    _, section, cfg, variant = case
    cdt = _cdt(case)
    m = model_for(cdt)
    _use_head(m, er.num_classes(section))
    names = er.param_names(section)
    pd = dict(m.named_parameters())
    bd = dict(m.named_buffers())
    name_of = {id(p): n for n, p in pd.items()}
    state = er.gen_state(section, F32)
    for n, v in state.items():          # the model holds exactly the values the references (and the seed table) were computed with
        assert torch.equal((pd[n] if n in pd else bd[n]).detach().cpu(), v), n
    stats0 = {n: bd[n].clone() for n in state if er.is_stat(n)}
    xs, gs = er.gen_inputs(section, er.case_seed(case), cdt)
    idx = er.outputs_with_gradient(section, variant)
    er.apply_config(m, section, cfg)
    try:
        m._prepare(torch.zeros(1, device="cuda"))
        ar = m._arena
        ar.ensure_grads()
        ar.grad_flat.zero_()
        for _ in range(times):
            ctx, rec, snap = Ctx(True), Rec(), {}
            ctx.lazy_res, ctx.bnb = Counting(), Counting()
            leaves = []

            def at_end_of_tape():          # first on the tape = last to run: what the pass left behind, before run_backward tidies up
                mine = {id(x) for x in leaves if x is not None}
                snap["leaf"] = [ctx.grad_of(x) if x is not None else None for x in leaves]
                left = {"grads": len([k for k in ctx.grads if k not in mine]), "lazy_res": len(ctx.lazy_res), "bnb": len(ctx.bnb)}
                snap["left"] = ["%s: %d" % kv for kv in left.items() if kv[1]]
            ctx.tape.append(at_end_of_tape)
            got_leaves, outs, slots, route, mid = compose(m, ctx, section, xs, cdt, er.leaf_grad(cfg))
            leaves.extend(got_leaves)
            out_grads = {}
            for i in idx:
                if slots is not None:
                    out_grads[slots[i]] = gs[i].cuda()
                elif outs[i].needs_grad:
                    ctx.set_grad(outs[i], _act(gs[i], cdt))
            m._engine.run_backward(ctx, out_grads, schedule=rec)
        torch.cuda.synchronize()
        res = {"outs": [o.detach().float().cpu() if torch.is_tensor(o) else _nchw(o) for o in outs],
               "leaf_grads": [None if g is None else _nchw(g) for g in snap["leaf"]], "param_grads": {}, "running": {}}
        tr = er.trainable_set(section, cfg)
        frozen_nonzero = set()
        rest = ar.grad_flat.clone()
        for n in names:
            i = ar.index[id(pd[n])]
            seg = ar.grad_seg(pd[n])
            touched = bool((seg.view(torch.int32) != 0).any())
            res["param_grads"][n] = ar._view(ar.grad_flat, i, pd[n].shape).detach().cpu().clone() if (touched and n in tr) else None
            if n in tr:
                rest[ar.offsets[i]: ar.offsets[i] + ar.sizes[i]] = 0
            elif touched:
                frozen_nonzero.add(n)
        if bool((rest.view(torch.int32) != 0).any()):
            frozen_nonzero.add("<arena outside the trainable slices>")
        for n in stats0:
            res["running"][n] = bd[n].detach().cpu().clone()
        obs = {"frozen_nonzero": frozen_nonzero,
               "stats_changed": {n for n, v in stats0.items() if not torch.equal(v.view(torch.int32), bd[n].view(torch.int32))},
               "ready": dict({n: 0 for n in names}, **{name_of[k]: c for k, c in rec.ready.items()}),
               "uses_left": {name_of[k] for k, c in ctx.uses.items() if c != 0}, "leftovers": snap["left"],
               "leaf_buffers": [g is not None for g in snap["leaf"]], "began": rec.began, "finished": rec.finished,
               "deferred": mid is not None and id(mid) in ctx.lazy_res.seen, "stats_rode": mid is not None and id(mid) in ctx.bnb.seen}
        assert rec.on_bucket == [None] and not ctx.tape and not ctx.grads and not ctx.lazy_res
        return res, obs, route
    finally:
        for n, v in stats0.items():
            bd[n].copy_(v)
        ar = m._arena
        if ar.grad_flat is not None:
            ar.grad_flat.zero_()
        torch.cuda.synchronize()


def _took_classes(route):
    return route is not None and any("->2304 " in r for r in route)


@pytest.mark.parametrize("case", er.CASES, ids=er.case_id)
def test_engine_section_matches_the_oracle(case):
    """fp32: every element of every output, leaf gradient, trainable parameter gradient (A: updated running statistics too) within
    16 x the float32 CPU run's own deviation from float64.  bf16: rel-L2 against the rounding oracle, gates 2e-3 / 3e-2 (towers 8e-2)
    / 5e-2.  Both: the exact properties (engine_ref.check_exact), and a gradient is absent exactly where the reference has none."""
    dtype, section, cfg, variant = case
    stats = er.CONFIGS[cfg][1]
    got, obs, route = run_device(case)
    if section == "S6":
        # the extents are multiples of 8: conv2 must have gone by position classes (nine class maps of 256 channels from the x8 / x4 members)
        assert _took_classes(route), "S6 did not take the position-class route: %s" % route
    if dtype == "fp32":
        r64, r32 = (er.view_for(reference(k, section, stats, variant), section, cfg) for k in ("f64", "f32"))
        er.compare_fp32(case, got, r64, r32)
    else:
        ref = er.view_for(reference("bf16", section, stats, variant, classes=_took_classes(route)), section, cfg)
        er.compare_bf16(case, got, ref)
    er.check_exact(case, obs)
    eng = model_for(_cdt(case))._engine
    want = er.expected_routes(section, cfg)
    if want is not None and eng.defer_shortcut_grad and eng.bn_mask_bits and eng.fuse_bn_stats:
        # the two-block chains exist to reach these two branches: say so if a case did not
        assert (obs["deferred"], obs["stats_rode"]) == want, (obs["deferred"], obs["stats_rode"], want)
    if variant is not None:          # what only the unused outputs reach: no buffer, no written slice — not a zero tensor
        assert any(g is None for g in got["param_grads"].values())


@pytest.mark.parametrize("case", [("fp32", "S2", "A", None), ("fp32", "S3", "D", None)], ids=er.case_id)
def test_two_backward_passes_accumulate_into_the_arena(case):
    """The same forward + backward twice without clearing the gradient arena: every gradient is twice the reference under the same
    allowance, frozen slices stay zero bits."""
    _, section, cfg, variant = case
    stats = er.CONFIGS[cfg][1]
    got, obs, _ = run_device(case, times=2)
    r64, r32 = (er.view_for(reference(k, section, stats, variant, times=2), section, cfg) for k in ("f64", "f32"))
    er.compare_fp32(("fp32", section, cfg, "x2"), got, r64, r32)
    er.check_exact(case, obs)
    once = reference("f64", section, stats, variant)
    n = sorted(er.trainable_set(section, cfg))[0]
    assert torch.equal(r64["param_grads"][n], 2.0 * once["param_grads"][n])
    report("engine %s: two passes into one arena = 2 x the reference; frozen slices zero" % er.case_id(case))
