"""Element-wise parity of the conv2 position-class kernels (csrc/conv2cls.hip) against float64.

Every kernel is launched through what production uses (ops.conv2cls_expand / conv2cls_pool / conv2cls_classsum / conv2cls_tapsum,
ops.Conv2ClsOperands, _lib.call("mpn_conv2cls_combine" | "mpn_conv2cls_fold")) on NaN-prefilled outputs (the allocations inside ops are
NaN-filled through _NanAlloc; fold's accumulated dW holds a known non-zero pattern), and EVERY element is compared with the reference
of tests/conv2cls_ref.py, built from the definition on exactly the operand values the kernel reads (inputs quantised through the
storage type; tapsum in the chain test is referenced both from the DEVICE's P and, end to end, from dy).  Bounds (conv2cls_ref.check_sum,
nothing fitted; tests/test_conv2cls_parity_cpu.py shows they accept fp32 models of the kernels and reject the modelled faults):
  combine    Wm, Wtap8 / 4 copies: bit-equal.  Frame filters: float64 sum of the contributing taps, n - 1 roundings on sum |w| (n <= 9);
             entries of <= 2 taps (0, a copy, one correctly rounded add) bit-equal.
  expand     M8[class8] + M4[class4]: f32 bit-equal; 16 bit: 1 rounding on |a| + |c| + half an output spacing.
  classsum   up to 9 terms, zero outside: n - 1 roundings on sum |t|.
  pool       1 / 2 / 4 and 1 / 6 / 36 pixels per class: n - 1 roundings on sum |dy| + half an output spacing; one-pixel classes bit-equal.
  tapsum     up to 9 stored P terms: n - 1 roundings + half an output spacing.
  fold       dw0 + g: bit-equal to the CPU's fp32 add (fp16: g's two per-tap slices times 64 / 16 first, exact).
  chain      dy -> pool -> tapsum against G straight from dy: the term count of dy + half a spacing of every stored P term + half of G's.
fp16 stores P in f32 (no output spacing allowed for) and G as G / s^2 (referenced as the scaled sum): conv2cls_ref.pool_store / g_scale.
No convolution is launched in these (the convolutions between the stages have their own parity files).  One report line per comparison.
Measured on an MI355X: 58 tests in 3.4 s; worst err / bound combine 1.000, classsum 0.515, expand 0.999, pool 1.000 (f32 0.997), tapsum
1.000 (f32 0.476), chain 1.000 (f32 0.468) — ratios at 1 are two-term sums and ties at half a 16-bit spacing.

test_conv2_backward_composition runs conv2's WHOLE backward as the engine issues it (Engine.conv2cls_begin / conv_cat_cls and the
tape's _conv_cat_cls_bwd: pool -> tapsum -> 1x1 input / filter gradients -> fold; beside it the plain route) on hand-made q5 .. q2 and
an injected dy, and compares every element of dq5, dq4, the three parts of dW and db with the float64 reference of the definition,
on input sets that span the fp16 range (nominal; dy = 1536 / 6144 (1 + u / 4) of one sign per channel; |dy| in [2^-14, 2^-10]), weights
as large as the outputs allow (conv2cls_ref.bwd_case; tests/test_conv2cls_parity_cpu.py section 5 pins the inputs and the bound).
Measured on an MI355X with the library of this change (18 cases, 1 - 2 s each), worst over sets and shapes:
  err / bound, class route   bf16: dq5 0.051, dq4 0.054, dW5 0.828, dW4 0.417, dWm 0.044, db 0.001
                             fp16: dq5 0.095, dq4 0.133, dW5 0.982, dW4 0.781, dWm 0.057, db 0.001    (f32: all <= 0.082)
  err / bound, plain route   bf16: dq5 0.560, dq4 0.689, dW <= 0.151;  fp16: dq5 0.465, dq4 0.571, dW <= 0.193
  class error / plain error against the same reference (rms over the elements; worst set):
                             bf16: dq5 1.57, dq4 1.38, dW5 5.8e4, dW4 4.1e4;  fp16: dq5 1.42, dq4 1.36, dW5 3.6e3, dW4 2.2e3;  f32: dq 1.07, dW5 / dW4 0.41
  (dWm and db are the same launches in both routes: 1.00.)  The input gradients stay inside the 1.6 the norm-level test allows; the
  per-tap filter gradients do not: the plain route contracts q with dy itself (fp32-exact given its 16-bit operands, rel. 1e-7), the
  class route with a G rounded to the compute type (rel. rms 2.3e-3 of |dW| in bf16, 2.1e-4 in fp16 — the level of any stored 16-bit
  activation gradient).
With the parent's library (P and G in the compute type, unscaled) the same cases fail in fp16 on both loss-scaled sets and both shapes,
first at dq5 (b=0, h=0, w=0, c=0) = NaN (G8 = inf meets filter taps of both signs); everything else passes there."""
import pytest
import torch

import conv2cls_ref as R
from conv2cls_ref import F32, TYPES, dn
from helpers import report
from stream_ref import exact

pytestmark = pytest.mark.gpu
NAN = float("nan")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests selected but no GPU is visible"
    from multiposenet.pytorch_amd import _lib
    _lib.lib()
    n = torch.get_num_threads()
    torch.set_num_threads(min(n, 16))
    yield
    torch.set_num_threads(n)


def _ops():
    from multiposenet.pytorch_amd import ops
    return ops


class _NanAlloc(object):
    """Inside the block, ops' (and, with engine=True, the engine's) torch.empty / empty_like return NaN-filled tensors, so an element a
    kernel leaves unwritten cannot hold a stale correct value."""

    class _Shim(object):
        def __getattr__(self, k):
            return getattr(torch, k)

        @staticmethod
        def _nan(t):
            return t.fill_(NAN) if t.is_floating_point() else t

        def empty(self, *a, **k):
            return self._nan(torch.empty(*a, **k))

        def empty_like(self, *a, **k):
            return self._nan(torch.empty_like(*a, **k))

    def __init__(self, engine=False):
        self.mods = [_ops()]
        if engine:
            from multiposenet.pytorch_amd import engine as eng_mod
            self.mods.append(eng_mod)

    def __enter__(self):
        self.ops = self.mods[0]
        for m in self.mods:
            m.torch = self._Shim()
        return self.ops

    def __exit__(self, *exc):
        for m in self.mods:
            m.torch = torch
        torch.cuda.synchronize()
        return False


def _act(t5, dtype):
    """[B, h, w, 9, O] (or [B, H, W, O]) CPU values -> dense device Act in the storage type."""
    t = t5.reshape(t5.shape[0], t5.shape[1], t5.shape[2], -1).to(dtype).cuda().contiguous()
    return _ops().Act(t, t.shape[3])


def _planes(a):
    """Act [B, h, w, 9 O] -> CPU [B, h, w, 9, O]."""
    t = a.t.cpu()
    return t.reshape(t.shape[0], t.shape[1], t.shape[2], 9, t.shape[3] // 9)


# ------------------------------------------------------------------------------------------------ combine / fold / operands
@pytest.mark.parametrize("name", list(R.COMBINE_CASES))
def test_combine(name):
    ops = _ops()
    (O, C), _ = R.COMBINE_CASES[name]
    w = R.combine_input(name)
    n = ops.call("mpn_conv2cls_comb_elems", O, C)
    assert n == sum(R.comb_sizes(O, C)) + sum(R.comb_sizes(O, C)[1:])
    comb = torch.full((n + 64,), NAN, device="cuda")                             # 64 guard elements behind the result
    ops.call("mpn_conv2cls_combine", ops.ptr(w.cuda()), ops.ptr(comb), O, C, ops.stream_ptr())
    torch.cuda.synchronize()
    assert bool(torch.isnan(comb[n:]).all()), "combine wrote behind comb"
    R.check_combine("combine O=%d C=%d" % (O, C), comb[:n], w, "%d elements, %d workgroups" % (n, -(-n // 256)))


@pytest.mark.parametrize("name", list(R.COMBINE_CASES))
def test_fold(name):
    ops = _ops()
    (O, C), _ = R.COMBINE_CASES[name]
    dcomb, dw0 = R.fold_inputs(O, C)
    for dtype in TYPES:                                                          # the type of the backward that made dcomb: fp16's tap slices carry 1 / s^2
        dw = torch.cat([dw0, torch.full((64,), NAN)]).cuda()
        ops.call("mpn_conv2cls_fold", ops.ptr(dcomb.cuda()), ops.ptr(dw), O, C, ops.dtype_code(dtype), ops.stream_ptr())
        torch.cuda.synchronize()
        assert bool(torch.isnan(dw[dw0.numel():]).all()), "fold wrote behind dW"
        k = R.fold_scale(dtype)
        assert k == ((64.0, 16.0) if dtype == torch.float16 else (1.0, 1.0))
        exact("fold O=%d C=%d dW += g%s" % (O, C, "" if dtype == TYPES[0] else " (%s%s)" % (dn(dtype), "" if k[0] == 1.0 else ": tap slices x 64 / x 16")),
              dw[: dw0.numel()].cpu().reshape(O, 9, 4 * C), R.fold_ref(dcomb, dw0, O, C, scale=k), "%d elements" % dw0.numel())


@pytest.mark.parametrize("dtype", TYPES, ids=dn)
def test_operands_slices_and_transposes(dtype):
    O, C = 256, 128
    w = R.combine_input("256x128")
    with _NanAlloc() as ops:
        wo = ops.Conv2ClsOperands(w.cuda(), O, C, dtype, True)
    tag, route = "Conv2ClsOperands %s " % dn(dtype), "O=256 C=128 want_t"
    comb32 = wo.keep.cpu()
    R.check_combine(tag + "comb32", comb32, w, route)
    ref = R.operands_ref(comb32, O, C, dtype)
    assert (wo.comb is wo.keep) == (dtype == F32) and (wo.nm, wo.nc, wo.nt) == R.comb_sizes(O, C)
    for k in ("comb", "wm", "wm_t"):
        assert getattr(wo, k).dtype == dtype
        exact(tag + k, getattr(wo, k).cpu().float(), ref[k].float(), route)
    for k in ("wc", "wtap", "wtap_t"):
        for m in range(2):
            assert getattr(wo, k)[m].dtype == dtype
            exact("%s%s[%d]" % (tag, k, m), getattr(wo, k)[m].cpu().float(), ref[k][m].float(), route)


# ------------------------------------------------------------------------------------------------ forward: classsum, expand
@pytest.mark.parametrize("name", list(R.CLASSSUM_CASES))
def test_classsum(name):
    (B, h, w, O), _ = R.CLASSSUM_CASES[name]
    t = R.low_input("classsum", name, F32)
    with _NanAlloc() as ops:
        m = ops.conv2cls_classsum(_act(t, F32))
    assert m.t.shape == (B, h, w, 9 * O) and m.t.dtype == F32
    R.check_sum("classsum " + name, _planes(m), R.reduce_terms(R.classsum_terms(t)), F32, "%d threads" % (B * h * w * 9 * (O // 4)))


@pytest.mark.parametrize("dtype", TYPES, ids=dn)
@pytest.mark.parametrize("name", list(R.EXPAND_CASES))
def test_expand(name, dtype):
    (B, H, W, O), _ = R.EXPAND_CASES[name]
    m8, m4 = R.expand_input(name)
    with _NanAlloc() as ops:
        e = ops.conv2cls_expand(_act(m8, F32), _act(m4, F32), B, H, W, O, dtype)
    assert e.t.shape == (B, H, W, O) and e.t.dtype == dtype
    R.check_sum("expand %s %s" % (name, dn(dtype)), e.t.cpu(), R.reduce_terms(R.expand_terms(m8, m4, H, W)), dtype,
                "%d threads" % (B * H * W * (O // 4)), "bhwo", exact_n=2 if dtype == F32 else 1)


# ------------------------------------------------------------------------------------------------ backward: pool, tapsum, chain
@pytest.mark.parametrize("dtype", TYPES, ids=dn)
@pytest.mark.parametrize("name", list(R.POOL_CASES))
def test_pool(name, dtype):
    (B, H, W, O), _ = R.POOL_CASES[name]
    threads = R.pool_threads(B, H, W, O)
    assert threads == R.POOL_THREADS[name]                                       # 2x16x24x24: 288 = one full workgroup + 32 live lanes
    dy = R.pool_input("pool", name, dtype)
    with _NanAlloc() as ops:
        p8, p4 = ops.conv2cls_pool(_act(dy, dtype))
    pt = R.pool_store(dtype)                                                     # fp16: f32 class sums, no output spacing allowed for
    assert p8.t.shape == (B, H // 8, W // 8, 9 * O) and p4.t.shape == (B, H // 4, W // 4, 9 * O) and p8.t.dtype == p4.t.dtype == pt
    route = "%d threads, %d workgroups" % (threads, -(-threads // 256))
    for s, p in ((8, p8), (4, p4)):
        R.check_sum("pool %s %s P%d" % (name, dn(dtype), s), _planes(p), R.reduce_terms(R.pool_terms(dy, s)), pt, route)


@pytest.mark.parametrize("dtype", TYPES, ids=dn)
@pytest.mark.parametrize("name", list(R.LOW_CASES))
def test_tapsum(name, dtype):
    (B, h, w, O), _ = R.LOW_CASES[name]
    pt = R.pool_store(dtype)
    P = R.low_input("tapsum", name, pt)
    for s in ((8, 4) if dtype == torch.float16 else (8,)):                       # fp16 stores G / s^2: both members' factors
        with _NanAlloc() as ops:
            g = ops.conv2cls_tapsum(_act(P, pt), s, dtype)
        assert g.t.shape == (B, h, w, 9 * O) and g.t.dtype == dtype
        k = R.g_scale(dtype, s)
        R.check_sum("tapsum %s %s%s" % (name, dn(dtype), "" if k == 1.0 else " / %d" % (s * s)), _planes(g),
                    R.scaled(R.reduce_terms(R.tapsum_terms(P)), k), dtype, "%d threads" % (B * h * w * 9 * (O // 4)))


@pytest.mark.parametrize("dtype", TYPES, ids=dn)
@pytest.mark.parametrize("name", list(R.CHAIN_CASES))
def test_chain_pool_then_tapsum(name, dtype):
    (B, H, W, O), _ = R.CHAIN_CASES[name]
    dy = R.pool_input("chain", name, dtype)
    with _NanAlloc() as ops:
        p8, p4 = ops.conv2cls_pool(_act(dy, dtype))
        g8, g4 = ops.conv2cls_tapsum(p8, 8, dtype), ops.conv2cls_tapsum(p4, 4, dtype)
    pt = R.pool_store(dtype)
    for s, p, g in ((8, p8, g8), (4, p4, g4)):
        tag = "chain %s %s G%d " % (name, dn(dtype), s)
        k = R.g_scale(dtype, s)
        Pd = _planes(p).float()                                                  # the device's stored class sums
        R.check_sum(tag + "from the device's P", _planes(g), R.scaled(R.reduce_terms(R.tapsum_terms(Pd)), k), dtype, "tapsum alone")
        R.check_sum(tag + "from dy", _planes(g), R.scaled(R.tap_direct(dy, s), k), dtype, "pool + tapsum", exact_n=-1,
                    extra_abs=k * R.chain_extra(Pd, pt))


# ------------------------------------------------------------------------------------------------ conv2's whole backward, as the engine issues it
def _conv2_backward(m, case, classes):
    """conv2 forward (act = 0: the injected dy passes through no ReLU mask) and backward through the ENGINE's own composition —
    Engine.conv2cls_begin / conv_cat_cls and the tape's _conv_cat_cls_bwd with classes, else the plain route keypoint_head would take —
    on hand-made q5 .. q2 and an injected output gradient.  One stream (the NaN prefill of a tensor allocated inside a side-stream
    closure would race with the kernel that writes it; test_round6_gpu pins the two schedules to identical bits).  -> BWD_OUTPUTS."""
    from multiposenet.pytorch_amd import ops
    from multiposenet.pytorch_amd.engine import Ctx
    eng, dt = m._engine, m.compute_dtype
    B, H, W = case.B, case.H, case.W
    saved = eng.overlap_wgrad
    eng.overlap_wgrad = False
    try:
        with torch.no_grad():
            m.conv2.weight.copy_(case.w.permute(0, 3, 1, 2))
            m.conv2.bias.zero_()
        m._prepare(torch.zeros((B, 3, 4 * H, 4 * W), device="cuda"))             # refreshes the 16-bit operand copies of the arena
        m._arena.ensure_grads()
        m._arena.grad_flat.zero_()
        ctx = Ctx(True)
        got = {}
        qs = [ops.Act(t.to(dt).cuda().contiguous(), R.C2, needs_grad=True) for t in case.q]
        ctx.tape.append(lambda: got.update(dq5=ctx.grad_of(qs[0]), dq4=ctx.grad_of(qs[1])))      # runs last: the tape is walked backwards
        with _NanAlloc(engine=True):
            if classes:
                st = eng.conv2cls_begin(ctx, qs[0], qs[1], H, W, m.conv2)
                assert st is not None and ops.conv2cls_supported(qs, H, W)
                y = eng.conv_cat_cls(ctx, qs, H, W, m.conv2, 0, st)
            elif ops.cat_supported(qs, H, W):
                y = eng.conv_cat(ctx, qs, H, W, m.conv2, act=0)
            else:
                y, _ = eng.conv(ctx, eng.concat_up(ctx, qs, H, W), m.conv2, act=0)
            eng.export_internal(ctx, y, "y")
            assert y.Cs == R.O2
            ctx.out_grads = {"y": ops.Act(case.dy.to(dt).cuda().contiguous(), R.O2)}
            eng.run_backward(ctx, ctx.out_grads)
        dw = m.conv2.weight.grad.detach().float().cpu().permute(0, 2, 3, 1)
        got = {k: v.t.float().cpu() for k, v in got.items()}
        got.update(dW5=dw[..., : R.C2], dW4=dw[..., R.C2: 2 * R.C2], dWm=dw[..., 2 * R.C2:], db=m.conv2.bias.grad.detach().float().cpu().clone())
        m._arena.grad_flat.zero_()
        return got
    finally:
        eng.overlap_wgrad = saved


BWD_CASES = [(dt, sh, st) for dt in TYPES for sh in R.BWD_SHAPES for st in R.BWD_SETS if dt != F32 or st == "nominal"]


@pytest.mark.parametrize("dtype,shape,setname", BWD_CASES, ids=["%s-%s-%s" % (dn(dt), st, sh) for dt, sh, st in BWD_CASES])
def test_conv2_backward_composition(dtype, shape, setname):
    """Every element of dq5, dq4, the three parts of dW and db, from the class route AND from the plain route (the yardstick), against
    the float64 reference of conv2's backward from the definition (conv2cls_ref.bwd_case), on input sets that span the fp16 range;
    bounds conv2cls_ref.bwd_specs (structural).  A second report line per output: class-route error / plain-route error (rms, max)."""
    from test_model_gpu import get_model
    case = R.bwd_case(shape, setname, dtype)
    m = get_model(50, dtype)
    m.train()
    plain = _conv2_backward(m, case, False)
    cls = _conv2_backward(m, case, True)
    get_model(50, dtype)                                                         # conv2's own weights back
    tag = "conv2 bwd %s %s %s " % (shape, setname, dn(dtype))
    R.check_bwd(tag + "plain", plain, R.bwd_specs(case, "plain"), "conv_cat / concat_up")
    R.check_bwd(tag + "class", cls, R.bwd_specs(case, "class"), "conv_cat_cls")
    for k in R.BWD_OUTPUTS:
        rms, mx = R.error_ratio(cls[k], plain[k], case.ref[k])
        report("%-58s %-52s class / plain error: rms %.3f  max %.3f" % (tag + k, "against the same float64 reference", rms, mx))
