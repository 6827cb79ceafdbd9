"""Element-wise tier for the parameter path (csrc/weight_prep.hip) on the MI355X: every cast, transpose, packing, padding, fill and copy
bit for bit against tests/param_ref.py's references, the Adam arithmetic of all three entry points element by element against the
float64 update under the derived bounds there, and adam_advance_kernel's bias corrections against the float32 betas widened to double.

Every destination sits inside an allocation sized for the widest type with guards before and after the written range; the guards must
keep their fill bit for bit.  Every pointer is a real allocation; slices handed to the 16-byte entry points start at multiples of four
floats; no input is an f32 subnormal.  Teeth: tests/test_param_path_cpu.py."""
import ctypes

import numpy as np
import pytest
import torch

import param_ref as R
from helpers import report

pytestmark = pytest.mark.gpu

f32 = np.float32
BADARG = -2
FILL = 0x5A                    # guard byte: 0x5A5A is 1.5e16 as bf16, 0x5A5A5A5A 1.5e16 as f32 — nothing a case writes
PRE = 64                       # guard elements (of f32 size) before the destination


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests selected but no GPU is visible"
    from multiposenet.pytorch_amd import _lib
    _lib.lib()


def _L():
    from multiposenet.pytorch_amd import _lib, ops
    return _lib, ops


def code(dtype):
    return {R.F32: 0, R.BF: 1, R.H16: 2}[dtype]


def dev(x):
    return (torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x).cuda()


class Guarded(object):
    """n elements of `dtype` inside an allocation of PRE + n + PRE f32-sized slots filled with FILL: the destination starts 256 bytes in,
    whatever follows its n elements (at least PRE slots, more for a 16-bit type) is guard."""

    def __init__(self, n, dtype):
        es = torch.empty((), dtype=dtype).element_size()
        self.raw = torch.full((4 * (PRE + n + PRE),), FILL, dtype=torch.uint8, device="cuda")
        self.lo, self.hi = 4 * PRE, 4 * PRE + n * es
        self.t = self.raw[self.lo: self.hi].view(dtype)

    def check(self, name):
        torch.cuda.synchronize()
        for part, what in ((self.raw[: self.lo], "before"), (self.raw[self.hi:], "after")):
            assert torch.equal(part, torch.full_like(part, FILL)), "%s: guard %s the destination was written" % (name, what)

    def untouched(self, name):
        self.check(name)
        assert torch.equal(self.t.view(torch.uint8), torch.full((self.hi - self.lo,), FILL, dtype=torch.uint8, device="cuda")), \
            "%s: destination written" % name


def bit_equal(name, got, want):
    got, want = got.cpu(), want.cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape, got.dtype, want.dtype)
    gi, wi = R.ibits(got).reshape(-1), R.ibits(want).reshape(-1)
    bad = torch.nonzero(gi != wi)
    assert len(bad) == 0, "%s: %d of %d elements differ in bits, first at flat index %d: got %r, reference %r" % (
        name, len(bad), gi.numel(), int(bad[0]), float(got.reshape(-1)[int(bad[0])]), float(want.reshape(-1)[int(bad[0])]))


# ====================================================================================================== casts
@pytest.mark.parametrize("entry,dtype", [("mpn_cast_f32", R.BF), ("mpn_cast_f32", R.H16), ("mpn_cast_f32_to_bf16", R.BF)])
def test_cast_is_round_to_nearest_even_bit_for_bit(entry, dtype):
    L, ops = _L()

    def run(src, dst, n):
        if entry == "mpn_cast_f32":
            L.call(entry, ops.ptr(src), ops.ptr(dst), n, code(dtype), ops.stream_ptr())
        else:
            L.call(entry, ops.ptr(src), ops.ptr(dst), n, ops.stream_ptr())
    for n in R.CAST_SIZES:
        x = R.cast_input(n)
        d = Guarded(n, dtype)
        run(dev(x), d.t, n)
        d.check("%s %s n=%d" % (entry, R.dn(dtype), n))
        R.check_cast("%s %s n=%d" % (entry, R.dn(dtype), n), d.t, x, dtype)
    # source and destination 64 elements into larger buffers (the arena's flat[split:] / lowp[split:])
    n = 4096 + 5
    x = R.cast_input(64 + n)
    src = dev(x)
    d = Guarded(64 + n, dtype)
    run(src[64:], d.t[64:], n)
    d.check("%s %s offset 64" % (entry, R.dn(dtype)))
    assert torch.equal(d.t[:64].view(torch.uint8), torch.full((64 * d.t.element_size(),), FILL, dtype=torch.uint8, device="cuda"))
    R.check_cast("%s %s offset 64" % (entry, R.dn(dtype)), d.t[64:], x[64:], dtype)
    report("%-58s %s: %d sizes + offset case bit-equal to torch RNE (ties, +-0, overflow, f16 subnormals, inf; NaN kept)" % (
        entry, R.dn(dtype), len(R.CAST_SIZES)))


# ====================================================================================================== transposes
@pytest.mark.parametrize("dtype", R.TYPES)
def test_weight_transpose_per_layer_and_batched(dtype):
    L, ops = _L()
    rows, src_total, dst_total, blocks = R.wt_layout(R.TRANSPOSE_GEOMS)
    arena = torch.zeros(src_total)
    per_layer = []
    for k, ((O, RS, I, opad), row) in enumerate(zip(R.TRANSPOSE_GEOMS, rows)):
        w = R.weights(100 + k, O * RS * I)
        arena[row[0]: row[0] + w.numel()] = w
        ref = R.transpose_ref(w, O, RS, I, opad, dtype)
        d = Guarded(I * RS * opad, dtype)
        L.call("mpn_weight_transpose", ops.ptr(dev(w)), ops.ptr(d.t), O, RS, I, opad, code(dtype), ops.stream_ptr())
        name = "weight_transpose %s (O=%d RS=%d I=%d pad=%d)" % (R.dn(dtype), O, RS, I, opad)
        d.check(name)
        bit_equal(name, d.t.view(I, RS, opad), ref)
        assert not bool(R.ibits(d.t.view(I, RS, opad)[..., O:]).any()), name + ": pad columns are not +0"
        per_layer.append((row[1], d.t.clone(), ref))
    # one batched launch over all six, regions placed as Engine._wt_plan places them
    d = Guarded(dst_total, dtype)
    table = torch.tensor(rows, dtype=torch.int64, device="cuda")
    arena = arena.cuda()
    L.call("mpn_weight_transpose_batched", ops.ptr(arena), ops.ptr(d.t), ops.ptr(table), len(rows), blocks, code(dtype), ops.stream_ptr())
    d.check("weight_transpose_batched %s" % R.dn(dtype))
    es = d.t.element_size()
    want = torch.full((dst_total * es,), FILL, dtype=torch.uint8).view(dtype)          # gaps between regions keep the guard fill
    for off, single, ref in per_layer:
        want[off: off + ref.numel()] = ref.reshape(-1)
        assert torch.equal(R.ibits(d.t[off: off + ref.numel()]), R.ibits(single)), "batched differs from the per-layer launch"
    gaps = sum(int(r[1]) for r in rows[1:]) - sum(int(a[1]) + g[2] * g[1] * g[3] for a, g in zip(rows[:-1], R.TRANSPOSE_GEOMS[:-1]))
    assert gaps > 0                                                                    # the case does have gaps
    bit_equal("weight_transpose_batched %s" % R.dn(dtype), d.t, want)
    report("%-58s %s: %d geometries per layer and batched bit-equal to the permutation, pad columns +0, %d gap elements untouched" % (
        "weight_transpose", R.dn(dtype), len(rows), gaps))


def test_engine_table_and_arena_cast_on_the_model_itself():
    """Engine._wt_plan()'s own table on the model's own arena: every planned layer's view against its permuted master weight; and the
    16-bit copy of the whole arena after _prepare, alignment pads included."""
    from test_round2_gpu import _train_setup
    L, ops = _L()
    m, inputs, _ = _train_setup(50, torch.bfloat16, 2, 64)
    img = inputs[0][0]
    m._prepare(img)
    m._prepare(img, prn=True)
    ar, cdt = m._arena, m.compute_dtype
    torch.cuda.synchronize()
    assert torch.equal(R.ibits(ar.lowp[cdt]), R.ibits(ar.flat.to(cdt))), "the arena's 16-bit copy is not flat.to(dtype)"
    plan = m._engine._wt_plan()
    d = Guarded(plan["total"], cdt)
    L.call("mpn_weight_transpose_batched", ops.ptr(ar.flat), ops.ptr(d.t), ops.ptr(plan["table"]), plan["n"], plan["blocks"], code(cdt),
           ops.stream_ptr())
    d.check("engine table")
    want = torch.full((plan["total"] * d.t.element_size(),), FILL, dtype=torch.uint8, device="cuda").view(cdt)
    by_id = {id(p): p for p in m.parameters()}
    assert len(plan["views"]) == plan["n"] > 50
    for key, (off, (I, R_, S, opad)) in plan["views"].items():
        p = by_id[key]
        O = p.shape[0]
        w = p.detach().reshape(O, I, R_, S) if p.dim() == 4 else p.detach().reshape(O, I, 1, 1)
        region = torch.zeros(I, R_, S, opad, dtype=cdt, device="cuda")
        region[..., :O] = w.permute(1, 2, 3, 0).to(cdt)
        want[off: off + region.numel()] = region.reshape(-1)
        assert torch.equal(R.ibits(d.t[off: off + region.numel()].view(I, R_, S, opad)), R.ibits(region)), \
            "planned layer at %d (O=%d I=%d %dx%d pad=%d)" % (off, O, I, R_, S, opad)
    assert torch.equal(R.ibits(d.t), R.ibits(want)), "an element between the planned regions was written"
    report("%-58s %d layers, %d elements: every view bit-equal to its permuted master weight, gaps untouched; lowp == flat.to(bf16) over %d" % (
        "engine wt table (R50 bf16)", plan["n"], plan["total"], ar.total))


# ====================================================================================================== padding and the stem
@pytest.mark.parametrize("dtype", R.TYPES)
def test_weight_pad_k(dtype):
    L, ops = _L()
    for Cout, K, Kpad in R.PAD_K_SHAPES:
        w = R.weights(Cout + K, Cout * K)
        d = Guarded(Cout * Kpad, dtype)
        L.call("mpn_weight_pad_k", ops.ptr(dev(w)), ops.ptr(d.t), Cout, K, Kpad, code(dtype), ops.stream_ptr())
        name = "weight_pad_k %s %dx%d->%d" % (R.dn(dtype), Cout, K, Kpad)
        d.check(name)
        bit_equal(name, d.t.view(Cout, Kpad), R.pad_k_ref(w, Cout, K, Kpad, dtype))
    report("%-58s %s: %d shapes bit-equal to F.pad(w).to(dtype)" % ("weight_pad_k", R.dn(dtype), len(R.PAD_K_SHAPES)))


@pytest.mark.parametrize("dtype", R.TYPES)
def test_stem_pack_weight(dtype):
    L, ops = _L()
    for Cout in R.STEM_COUTS:
        w = R.weights(200 + Cout, Cout * 147)
        d = Guarded(Cout * 7 * 32, dtype)
        L.call("mpn_stem_pack_weight", ops.ptr(dev(w)), ops.ptr(d.t), Cout, code(dtype), ops.stream_ptr())
        name = "stem_pack_weight %s Cout=%d" % (R.dn(dtype), Cout)
        d.check(name)
        got = d.t.view(Cout, 7, 8, 4)
        assert not bool(R.ibits(got[..., 3]).any()) and not bool(R.ibits(got[:, :, 7]).any()), name + ": a pad slot is not +0"
        bit_equal(name, d.t.view(Cout, 7, 32), R.stem_pack_weight_ref(w, Cout, dtype))
    report("%-58s %s: Cout %s bit-equal, slots c == 3 and s == 7 are +0" % ("stem_pack_weight", R.dn(dtype), list(R.STEM_COUTS)))


def test_stem_unpack_wgrad_accumulates_the_live_slots_only():
    L, ops = _L()
    for Cout in R.STEM_COUTS:
        dp = torch.full((Cout, 7, 8, 4), 1e30)
        dp[:, :, :7, :3] = R.weights(300 + Cout, Cout * 147).view(Cout, 7, 7, 3)
        dw = R.weights(400 + Cout, Cout * 147) * 3.0 + 0.25
        d = Guarded(Cout * 147, R.F32)
        d.t.copy_(dw)
        L.call("mpn_stem_unpack_wgrad", ops.ptr(dev(dp)), ops.ptr(d.t), Cout, ops.stream_ptr())
        d.check("stem_unpack_wgrad Cout=%d" % Cout)
        bit_equal("stem_unpack_wgrad Cout=%d" % Cout, d.t, R.stem_unpack_ref(dw, dp.reshape(Cout, 7, 32), Cout))
    report("%-58s Cout %s: dw == fl32(dw + dp[live]) bit for bit, the 1e30 pad slots never reach dw" % ("stem_unpack_wgrad", list(R.STEM_COUTS)))


@pytest.mark.parametrize("dtype", R.TYPES)
def test_stem_pack_image(dtype):
    L, ops = _L()
    for B, H, W in R.IMAGE_SHAPES:
        for layout, (base, view) in R.image_views(B, H, W, B * 100 + H).items():
            x = view(base.cuda())
            assert x.shape == (B, 3, H, W)
            if layout == "strided":
                assert x.stride(3) == 2 and x.storage_offset() > 0
            d = Guarded(B * (H + 6) * (W + 8) * 4, dtype)
            L.call("mpn_stem_pack_image", ops.ptr(x), x.stride(0), x.stride(1), x.stride(2), x.stride(3), ops.ptr(d.t), B, H, W, code(dtype),
                   ops.stream_ptr())
            name = "stem_pack_image %s %s %dx%dx%d" % (R.dn(dtype), layout, B, H, W)
            d.check(name)
            got = d.t.view(B, H + 6, W + 8, 4)
            for part, what in ((got[:, :3], "top rows"), (got[:, H + 3:], "bottom rows"), (got[:, :, :3], "left columns"),
                               (got[:, :, W + 3:], "right columns"), (got[..., 3], "fourth channel")):
                assert not bool(R.ibits(part).any()), "%s: %s are not +0" % (name, what)
            assert got[:, H + 3:].shape[1] == 3 and got[:, :, W + 3:].shape[2] == 5
            bit_equal(name, got, R.stem_pack_image_ref(view(base), dtype))
    report("%-58s %s: %d shapes x (nchw, channels_last, strided view) bit-equal, borders 3/3/3/5 and channel 3 are +0" % (
        "stem_pack_image", R.dn(dtype), len(R.IMAGE_SHAPES)))


# ====================================================================================================== fill, copy
def test_fill_and_copy_bytes():
    L, ops = _L()
    for n in (1, 255, 256, 257):
        for val in (0.0, -0.0, 1.5):
            d = Guarded(n, R.F32)
            L.call("mpn_fill_f32", ops.ptr(d.t), val, n, ops.stream_ptr())
            d.check("fill n=%d" % n)
            bit_equal("fill %r n=%d" % (val, n), d.t, torch.full((n,), val))
            if str(val) == "-0.0":
                assert bool((R.ibits(d.t) == -2 ** 31).all())
    for nbytes in (1, 3, 17, 4096):
        src = (torch.arange(nbytes + 8, dtype=torch.int32) * 37 + 11).to(torch.uint8).cuda()
        d = Guarded((nbytes + 3) // 4, R.F32)
        L.call("mpn_copy_bytes", ops.ptr(d.t), ops.ptr(src), nbytes, ops.stream_ptr())
        torch.cuda.synchronize()
        raw = d.raw.cpu()
        want = torch.full_like(raw, FILL)
        want[d.lo: d.lo + nbytes] = src[:nbytes].cpu()
        assert torch.equal(raw, want), "copy_bytes nbytes=%d" % nbytes
    report("%-58s n in {1, 255, 256, 257} x {0.0, -0.0, 1.5} and copies of {1, 3, 17, 4096} bytes exact, guards untouched" % "fill_f32 / copy_bytes")


# ====================================================================================================== dtype validation
def test_unknown_dtype_code_is_refused_before_any_launch():
    L, ops = _L()
    lib = L.lib()
    st = ops.stream_ptr()
    O, RS, I, opad = 33, 9, 31, 64
    w = dev(R.weights(1, O * RS * I))
    rows, src_total, dst_total, blocks = R.wt_layout(R.TRANSPOSE_GEOMS[:2])
    arena = torch.zeros(src_total, device="cuda")
    table = torch.tensor(rows, dtype=torch.int64, device="cuda")
    img = torch.randn(2, 3, 7, 5, device="cuda")
    cases = [
        ("mpn_weight_transpose", I * RS * opad, lambda d: lib.mpn_weight_transpose(ops.ptr(w), ops.ptr(d), O, RS, I, opad, 7, st)),
        ("mpn_weight_transpose_batched", dst_total,
         lambda d: lib.mpn_weight_transpose_batched(ops.ptr(arena), ops.ptr(d), ops.ptr(table), len(rows), blocks, 7, st)),
        ("mpn_weight_pad_k", 5 * 32, lambda d: lib.mpn_weight_pad_k(ops.ptr(w), ops.ptr(d), 5, 17, 32, 7, st)),
        ("mpn_stem_pack_weight", 3 * 7 * 32, lambda d: lib.mpn_stem_pack_weight(ops.ptr(w), ops.ptr(d), 3, 7, st)),
        ("mpn_stem_pack_image", 2 * 13 * 13 * 4,
         lambda d: lib.mpn_stem_pack_image(ops.ptr(img), img.stride(0), img.stride(1), img.stride(2), img.stride(3), ops.ptr(d), 2, 7, 5, 7, st)),
    ]
    for name, n, launch in cases:
        d = Guarded(n, R.F32)
        assert launch(d.t) == BADARG, name + ": dtype code 7 was not refused"
        d.untouched(name)
    report("%-58s dtype code 7 -> MPN_E_BADARG from the five MPN_DISPATCH_T entry points, destinations untouched" % "dtype validation")


# ====================================================================================================== adam_advance
def _advance(h_np):
    L, ops = _L()
    h = dev(h_np.copy())
    L.call("mpn_adam_advance", ops.ptr(h), ops.stream_ptr())
    torch.cuda.synchronize()
    return h, h.cpu().numpy()


@pytest.mark.parametrize("betas", R.BETAS)
def test_adam_advance_rebuilds_both_bias_corrections(betas):
    equal = total = 0
    for t in R.ADVANCE_STEPS:
        h0 = R.hyper_vector(b1=betas[0], b2=betas[1], wd=1e-2, gs=0.37, step=t - 1)
        _, h1 = _advance(h0)
        assert int(h1[8:9].view(np.int32)[0]) == t
        keep = [0, 1, 2, 3, 4, 5] + list(range(9, R.HYPER_N))
        assert np.array_equal(R.bits32(h1)[keep], R.bits32(h0)[keep]), "adam_advance changed a slot that is not its own (t=%d)" % t
        for got, want, what in zip(h1[6:8], R.bias_corrections(h0[1], h0[2], t), ("bc1", "bc2s")):
            d = R.spacings_apart(got, want)
            assert got > 0 and d <= 1, "%s at t=%d betas=%s: device %r, float64 reference %r (%d spacings)" % (what, t, betas, got, want, d)
            equal += d == 0
            total += 1
        if t == 100000:
            assert h1[6] == 1.0 and h1[7] == 1.0           # b^t has underflowed below half a spacing of 1
    report("%-58s betas %s: %d of %d bias corrections bit-equal to float32(1 - float64(b_f32)^t), none more than one spacing off" % (
        "adam_advance", betas, equal, total))


# ====================================================================================================== Adam arithmetic
def _adam_call(entry, bufs, s, e, h_dev, h_np, coef=None):
    L, ops = _L()
    P, G, M, V = (bufs[k][s:e] for k in "pgmv")
    if entry == "mpn_adam_step":
        L.call(entry, ops.ptr(P), ops.ptr(G), ops.ptr(M), ops.ptr(V), e - s, *[ctypes.c_float(float(h_np[i])) for i in (0, 1, 2, 3, 4, 6, 7, 5)],
               ops.stream_ptr())
    elif entry == "mpn_adam_step_dev":
        L.call(entry, ops.ptr(P), ops.ptr(G), ops.ptr(M), ops.ptr(V), e - s, ops.ptr(h_dev), ops.stream_ptr())
    else:
        L.call(entry, ops.ptr(P), ops.ptr(G), ops.ptr(M), ops.ptr(V), e - s, ops.ptr(h_dev), ops.ptr(coef), ops.stream_ptr())


COEF = 0.37109375              # the clip coefficient of the clip cases (an f32 value)


@pytest.mark.parametrize("wd,gs", R.ADAM_SETTINGS)
@pytest.mark.parametrize("entry", ["mpn_adam_step", "mpn_adam_step_dev", "mpn_adam_step_clip_dev"])
def test_adam_update_against_float64_every_element(entry, wd, gs):
    """Sizes x step counts x (zero | non-zero moments); the slice starts 8 floats into a buffer with 8 spare floats behind its end
    (mpn_adam_step, scalar accesses, also at the odd offset 7)."""
    worst = R.Worst()
    coef = torch.tensor([COEF], device="cuda") if entry.endswith("clip_dev") else None
    for t in R.ADAM_STEPS:
        h_dev, h = _advance(R.hyper_vector(wd=wd, gs=gs, step=t - 1))           # bc1 / bc2s: the device's own, read back
        for n in R.ADAM_SIZES:
            for moments in (False, True):
                starts = (8, 7) if (entry == "mpn_adam_step" and n in (5, 1025)) else (8,)
                for s in starts:
                    tot = s + R.round_up(n, 4) + 8
                    before = dict(zip("pgmv", R.adam_inputs(tot, 1000 * t + 2 * n + moments, moments)))
                    bufs = {k: dev(x) for k, x in before.items()}
                    _adam_call(entry, bufs, s, s + n, h_dev, h, coef)
                    torch.cuda.synchronize()
                    after = {k: x.cpu().numpy() for k, x in bufs.items()}
                    g_in = (before["g"][s:s + n] * f32(COEF)).astype(f32) if coef is not None else None
                    res = R.check_adam_slice("%s wd=%g gs=%g t=%d n=%d mom=%d s=%d" % (entry, wd, gs, t, n, moments, s), before, after,
                                             s, s + n, h, g_in)
                    worst.add(res, "t=%d n=%d mom=%d s=%d" % (t, n, moments, s))
    for line in worst.lines("%s wd=%g gs=%g" % (entry, wd, gs)):
        report(line)


@pytest.mark.parametrize("wd,gs", [(1e-2, 1.0), (3e-3, 2.5)])
def test_clipped_update_is_scale_then_update(wd, gs):
    """mpn_adam_step_clip_dev: the gradient afterwards is fl32(g coef) (checked against numpy in the test above, here too) and p, m, v
    are bit-equal to mpn_scale_by_dev followed by mpn_adam_step_dev on copies."""
    L, ops = _L()
    coef = torch.tensor([COEF], device="cuda")
    h_dev, h = _advance(R.hyper_vector(wd=wd, gs=gs, step=9))
    for n in (5, 1025, 4099):
        s, tot = 8, 8 + R.round_up(n, 4) + 8
        before = dict(zip("pgmv", R.adam_inputs(tot, n, True)))
        a = {k: dev(x) for k, x in before.items()}
        b = {k: dev(x) for k, x in before.items()}
        _adam_call("mpn_adam_step_clip_dev", a, s, s + n, h_dev, h, coef)
        L.call("mpn_scale_by_dev", ops.ptr(b["g"][s:s + n]), n, ops.ptr(coef), ops.stream_ptr())
        _adam_call("mpn_adam_step_dev", b, s, s + n, h_dev, h)
        torch.cuda.synchronize()
        bit_equal("clip: gradient n=%d" % n, a["g"][s:s + n], torch.from_numpy((before["g"][s:s + n] * f32(COEF)).astype(f32)))
        for k in "pgmv":
            bit_equal("clip vs scale + step: %s n=%d" % (k, n), a[k], b[k])
    report("%-58s wd=%g gs=%g: g == fl32(g coef); p, m, v bit-equal to scale_by_dev + adam_step_dev" % ("adam_step_clip_dev", wd, gs))


@pytest.mark.parametrize("entry", ["mpn_adam_step", "mpn_adam_step_dev", "mpn_adam_step_clip_dev"])
def test_neutral_elements_stay_plus_zero(entry):
    """g = m = v = p = 0 stays +0 in p, m and v (the arena's alignment pads rely on it), with weight decay and through the clip."""
    coef = torch.tensor([COEF], device="cuda") if entry.endswith("clip_dev") else None
    for wd in (0.0, 1e-2):
        h_dev, h = _advance(R.hyper_vector(wd=wd, gs=0.37, step=2))
        for n in (3, 4, 1025):
            bufs = {k: torch.zeros(8 + R.round_up(n, 4) + 8, device="cuda") for k in "pgmv"}
            _adam_call(entry, bufs, 8, 8 + n, h_dev, h, coef)
            torch.cuda.synchronize()
            for k in "pgmv":
                assert not bool(R.ibits(bufs[k]).any()), "%s wd=%g n=%d: %s is no longer +0" % (entry, wd, n, k)


# ====================================================================================================== the arena through FusedAdam
def _small_model():
    from test_round2_gpu import _train_setup
    m, _, _ = _train_setup(50, torch.bfloat16, 2, 64)
    for p in m.parameters():
        p.grad = None
    return m


def test_fused_adam_on_the_arena_against_float64():
    """Three FusedAdam steps (wd 1e-2, grad_scale 0.5; fpn.layer1, fpn.layer3 and fpn.smooth2 frozen besides the PRN: several runs) on
    synthetic gradients written into grad_flat, against the float64 update formed with torch element-wise operations on the device."""
    from multiposenet.pytorch_amd.optim import FusedAdam
    m = _small_model()
    try:
        for p in list(m.fpn.layer1.parameters()) + list(m.fpn.layer3.parameters()) + list(m.fpn.smooth2.parameters()):
            p.requires_grad = False
        opt = FusedAdam(m, lr=1e-3, weight_decay=1e-2)
        opt.grad_scale = 0.5
        ar = opt._bind()
        ar.ensure_grads()
        runs = ar.trainable_runs()
        assert len(runs) >= 3, runs
        train = torch.zeros(ar.total, dtype=torch.bool, device="cuda")
        for s, e in runs:
            train[s:e] = True
        live = torch.zeros(ar.total, dtype=torch.bool, device="cuda")
        for off, n in zip(ar.offsets, ar.sizes):
            live[off: off + n] = True
        assert not bool(ar.flat[~live].view(torch.int32).any())
        gen = torch.Generator(device="cuda").manual_seed(5)
        D = torch.float64
        worst = {"m'": 0.0, "v'": 0.0, "p'": 0.0}
        where = dict(worst)
        for step in range(3):
            mag = 10.0 ** (torch.rand(ar.total, generator=gen, device="cuda") * 8 - 7)
            g = torch.where(live & train, mag * torch.sign(torch.randn(ar.total, generator=gen, device="cuda")), torch.zeros_like(mag))
            ar.grad_flat.copy_(g)
            p0, m0, v0 = ar.flat.clone(), opt._m.clone(), opt._v.clone()
            opt.step()
            torch.cuda.synchronize()
            h = opt._hyper.clone()
            lr, b1, b2, eps, wd, gs, bc1, bc2s = (h[i].double() for i in range(8))
            assert int(h[8:9].view(torch.int32).item()) == step + 1
            G, Gm = g.double() * gs + wd * p0.double(), (g.double() * gs).abs() + (wd * p0.double()).abs()
            M, Mm = b1 * m0.double() + (1 - b1) * G, b1 * m0.double().abs() + (1 - b1) * Gm
            V, Vm = b2 * v0.double() + (1 - b2) * G * G, b2 * v0.double().abs() + (1 - b2) * Gm * Gm
            Uv = (lr / bc1) * opt._m.double() / (opt._v.double().sqrt() / bc2s + eps)
            P, Pm = p0.double() - Uv, p0.double().abs() + (1 + R.U_OPS) * Uv.abs()
            for name, got, ref, mg, ops_ in (("m'", opt._m, M, Mm, R.M_OPS), ("v'", opt._v, V, Vm, R.V_OPS), ("p'", ar.flat, P, Pm, 1)):
                err, bound = (got.double() - ref).abs()[train], (ops_ * R.U * mg)[train]
                assert bool((err <= bound).all()), "step %d %s: %d elements out of bound" % (step + 1, name, int((~(err <= bound)).sum()))
                ratio = torch.where(bound > 0, err / bound, torch.zeros_like(err))
                w = float(ratio.max())
                if w > worst[name]:
                    worst[name], where[name] = w, "step %d arena index %d" % (step + 1, int(torch.nonzero(train)[int(ratio.argmax())]))
            for name, got, old in (("p", ar.flat, p0), ("m", opt._m, m0), ("v", opt._v, v0)):
                assert torch.equal(got[~train].view(torch.int32), old[~train].view(torch.int32)), "frozen %s changed" % name
                assert not bool(got[~live].view(torch.int32).any()), "an alignment pad of %s is no longer +0" % name
            del G, Gm, M, Mm, V, Vm, Uv, P, Pm
        assert opt.step_count() == 3
        for k in ("m'", "v'", "p'"):
            report("%-58s %-4s worst err/bound=%.3f at %s  OK%s" % ("FusedAdam arena (R50, %d runs, %d trainable)" % (len(runs), int(train.sum())),
                                                                  k, worst[k], where[k], "  (above 0.8)" if worst[k] > 0.8 else ""))
    finally:
        for p in m.parameters():
            p.requires_grad = True
            p.grad = None


def test_loaded_step_count_gives_the_same_bias_corrections_as_taking_the_steps():
    """load_state_dict(step = 7) then one step: hyper[6..8] bit-equal to an optimizer that took 8 steps itself — the host-computed
    placeholders _set_step writes are never what an update reads."""
    from multiposenet.pytorch_amd.optim import FusedAdam
    m = _small_model()
    try:
        a = FusedAdam(m, lr=1e-3)
        ar = a._bind()
        ar.ensure_grads()
        ar.grad_flat.zero_()
        for _ in range(7):
            a.step()
        sd = a.state_dict()
        assert all(int(float(s["step"])) == 7 for s in sd["state"].values()) and len(sd["state"]) > 0
        a.step()
        b = FusedAdam(m, lr=1e-3)
        b.load_state_dict(sd)
        assert b.step_count() == 7
        b.step()
        torch.cuda.synchronize()
        assert a.step_count() == 8 and b.step_count() == 8
        assert torch.equal(a._hyper[6:9].view(torch.int32), b._hyper[6:9].view(torch.int32)), (a._hyper[6:9], b._hyper[6:9])
        want = R.bias_corrections(0.9, 0.999, 8)
        got = a._hyper[6:8].cpu().numpy()
        assert R.spacings_apart(got[0], want[0]) <= 1 and R.spacings_apart(got[1], want[1]) <= 1
    finally:
        for p in m.parameters():
            p.grad = None
