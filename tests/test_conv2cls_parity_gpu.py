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
  fold       dw0 + g: bit-equal to the CPU's fp32 add.
  chain      dy -> pool -> tapsum against G straight from dy: the term count of dy + half a spacing of every stored P term + half of G's.
No convolution is launched here (the convolutions between the stages have their own parity files).  One report line per comparison.
Measured on an MI355X: 58 tests in 3.4 s; worst err / bound combine 1.000, classsum 0.515, expand 0.999, pool 1.000 (f32 0.997), tapsum
1.000 (f32 0.476), chain 1.000 (f32 0.468) — ratios at 1 are two-term sums and ties at half a 16-bit spacing."""
import pytest
import torch

import conv2cls_ref as R
from conv2cls_ref import F32, TYPES, dn
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
    """Inside the block, ops' torch.empty / empty_like return NaN-filled tensors, so an element a kernel leaves unwritten cannot hold a
    stale correct value."""

    class _Shim(object):
        def __getattr__(self, k):
            return getattr(torch, k)

        def empty(self, *a, **k):
            return torch.empty(*a, **k).fill_(NAN)

        def empty_like(self, *a, **k):
            return torch.empty_like(*a, **k).fill_(NAN)

    def __enter__(self):
        self.ops = _ops()
        self.ops.torch = self._Shim()
        return self.ops

    def __exit__(self, *exc):
        self.ops.torch = torch
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
    dw = torch.cat([dw0, torch.full((64,), NAN)]).cuda()
    ops.call("mpn_conv2cls_fold", ops.ptr(dcomb.cuda()), ops.ptr(dw), O, C, ops.stream_ptr())
    torch.cuda.synchronize()
    assert bool(torch.isnan(dw[dw0.numel():]).all()), "fold wrote behind dW"
    exact("fold O=%d C=%d dW += g" % (O, C), dw[: dw0.numel()].cpu().reshape(O, 9, 4 * C), R.fold_ref(dcomb, dw0, O, C),
          "%d elements" % dw0.numel())


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
    assert p8.t.shape == (B, H // 8, W // 8, 9 * O) and p4.t.shape == (B, H // 4, W // 4, 9 * O) and p8.t.dtype == p4.t.dtype == dtype
    route = "%d threads, %d workgroups" % (threads, -(-threads // 256))
    for s, p in ((8, p8), (4, p4)):
        R.check_sum("pool %s %s P%d" % (name, dn(dtype), s), _planes(p), R.reduce_terms(R.pool_terms(dy, s)), dtype, route)


@pytest.mark.parametrize("dtype", TYPES, ids=dn)
@pytest.mark.parametrize("name", list(R.LOW_CASES))
def test_tapsum(name, dtype):
    (B, h, w, O), _ = R.LOW_CASES[name]
    P = R.low_input("tapsum", name, dtype)
    with _NanAlloc() as ops:
        g = ops.conv2cls_tapsum(_act(P, dtype))
    assert g.t.shape == (B, h, w, 9 * O) and g.t.dtype == dtype
    R.check_sum("tapsum %s %s" % (name, dn(dtype)), _planes(g), R.reduce_terms(R.tapsum_terms(P)), dtype,
                "%d threads" % (B * h * w * 9 * (O // 4)))


@pytest.mark.parametrize("dtype", TYPES, ids=dn)
@pytest.mark.parametrize("name", list(R.CHAIN_CASES))
def test_chain_pool_then_tapsum(name, dtype):
    (B, H, W, O), _ = R.CHAIN_CASES[name]
    dy = R.pool_input("chain", name, dtype)
    with _NanAlloc() as ops:
        p8, p4 = ops.conv2cls_pool(_act(dy, dtype))
        g8, g4 = ops.conv2cls_tapsum(p8), ops.conv2cls_tapsum(p4)
    for s, p, g in ((8, p8, g8), (4, p4, g4)):
        tag = "chain %s %s G%d " % (name, dn(dtype), s)
        Pd = _planes(p).float()                                                  # the device's stored class sums
        R.check_sum(tag + "from the device's P", _planes(g), R.reduce_terms(R.tapsum_terms(Pd)), dtype, "tapsum alone")
        R.check_sum(tag + "from dy", _planes(g), R.tap_direct(dy, s), dtype, "pool + tapsum", exact_n=-1, extra_abs=R.chain_extra(Pd, dtype))
