"""Teeth for the streaming-kernel parity bounds (CPU tier).

tests/test_stream_parity_gpu.py compares every element the kernels of csrc/bn.hip and csrc/resample.hip write with a float64 reference
under the checks of tests/stream_ref.py (the bounds live there, so both tiers apply the same ones).  Here each kernel's fp32 arithmetic
is modelled on the CPU at the structures the GPU cases run — the (lanes, iters) walk of bn_act / bn_bwd_apply with a ragged last block
(4 lanes x 7 iters as at Cs = 256 in f32, 4 x 3 as at Cs = 512 in 16-bit), the lanes-strided chunk sums of bn_bwd_reduce with its
LDS combine, reduce_slices' 8-wide loop and tail, the coefficient formulas — and the checks must

  * ACCEPT the correct model in FMA-contracted and uncontracted form and in other summation orders, and
  * REJECT: a pixel of the walk skipped or visited twice at a block seam; the last ragged block not processed; a partial row dropped
    by the 8-wide loop of the finalize; a tail row counted twice; the ReLU mask taken from the unrounded value instead of the stored
    one; a mask byte read at p * G + g with the wrong G; dres overwritten instead of accumulated; k3 with the wrong sign on the a
    term; the max-pool tie going to the last maximum; a clipped border window indexing its taps by in-range count instead of window
    position; nearest children enumerated with floor instead of ceil_div; a pad lane left non-zero.

ReLU mask predicates: bn_act's sign bytes, and the z and sign-byte modes of the backward, use the STORED value (rounded to the element
type) > 0; the remask mode recomputes y * scale + shift > 0 in fp32, unrounded.  The two differ exactly on elements that are positive in
fp32 and round to 0 in the storage type (f16 below 2^-25); test_mask_predicate_is_the_stored_value constructs such elements.

The nearest-rule pin: the kernels use floor(o * Hs / Ho); torch's CPU nearest uses floor(o * float(Hs / Ho)).  The two agree for every
fine size 1 .. 1199 with Hc = ceil(Hf / 2) and for the exact factors 2, 4, 8 — the only pairs the FPN produces, and the condition under
which the product equals the reference's F.upsample — and disagree elsewhere (e.g. 26 -> 44), where the C ABI follows the integer rule."""
import pytest
import torch

import stream_ref as R
from helpers import rng_normal
from stream_ref import BF, F32, H16

NAN = float("nan")


@pytest.fixture(scope="module", autouse=True)
def _threads():
    n = torch.get_num_threads()
    torch.set_num_threads(min(n, 16))
    yield
    torch.set_num_threads(n)


def f32(x):
    """Round a float64 tensor to fp32 (kept as float64)."""
    return x.float().double()


def _rejects(fn, *a, **k):
    with pytest.raises(AssertionError):
        fn(*a, **k)


def _q(seed, shape, dtype):
    return rng_normal(seed, *shape).to(dtype)


# ------------------------------------------------------------------------------------------------ launch plans
def test_plan_mirror_reaches_the_production_iters():
    """cfg3 (R101 480^2 B=32 bf16): iters 7 at the stem and layer1, 3 at layer2's 512-channel tensors, 1 elsewhere."""
    assert R.plan(32 * 240 * 240, 64, BF)[:2] == (32, 7)
    assert R.plan(32 * 120 * 120, 256, BF)[:2] == (8, 7)
    assert R.plan(32 * 60 * 60, 512, BF)[:2] == (4, 3)
    assert R.plan(32 * 30 * 30, 1024, BF)[:2] == (2, 1)
    assert R.plan(32 * 15 * 15, 2048, BF)[:2] == (1, 1)
    assert R.geo(2048, F32) == (512, 256, 1, 2) and R.geo(32, BF) == (4, 4, 64, 1)
    assert R.pick_iters(1 << 40, 1) == 32
    # reduce_chunk at its clamps: low (4 lanes), middle rounded up to lanes, high (4096)
    assert R.reduce_chunk(126, 64) == 256 and R.reduce_chunk(19594, 8) == 40 and R.reduce_chunk(2113550, 64) == 4096


# ------------------------------------------------------------------------------------------------ the (lanes, iters) walk
def walk_counts(P, lanes, iters, block_stride=None, blocks=None):
    """Visits per pixel of the bn_act / bn_bwd_apply walk p = block * lanes * iters + it * lanes + lane (threads break at p >= P).
    block_stride / blocks model a wrong seam (pixels skipped or visited twice) and a last block that never runs."""
    bs = lanes * iters if block_stride is None else block_stride
    gx = (P + lanes * iters - 1) // (lanes * iters) if blocks is None else blocks
    p = (torch.arange(gx).reshape(-1, 1, 1) * bs + torch.arange(iters).reshape(1, -1, 1) * lanes + torch.arange(lanes).reshape(1, 1, -1))
    p = p.reshape(-1)
    return torch.bincount(p[p < P], minlength=P)


WALKS = [(F32, 4, 7, 28 * 40 + 16, 256, 252), (BF, 4, 3, 12 * 90 + 6, 512, 508)]      # dtype, lanes, iters, P, Cs, C


def act_model(y, sc, sf, res, relu, C, dtype, fma):
    """fp32 model of bn_act: returns (x fp32-valued [P, Cs] before the store, z in the storage type)."""
    yl = y.double()
    Cs = y.shape[1]
    scp, sfp = torch.zeros(Cs, dtype=torch.float64), torch.zeros(Cs, dtype=torch.float64)
    scp[:C], sfp[:C] = sc.double(), sf.double()
    x = f32(yl * scp + sfp) if fma else f32(f32(yl * scp) + sfp)
    if res is not None:
        x = f32(x + res.double())
    if relu:
        x = x.clamp(min=0.0)
    x[:, C:] = 0.0
    return x, x.float().to(dtype)


def _walk_operands(dtype, P, Cs, C, seed):
    y, res, dz = _q(seed, (P, Cs), dtype), _q(seed + 1, (P, Cs), dtype), _q(seed + 2, (P, Cs), dtype)
    sc, sf = rng_normal(seed + 3, C), rng_normal(seed + 4, C)
    return y, res, dz, sc, sf


@pytest.mark.parametrize("dtype,lanes,iters,P,Cs,C", WALKS, ids=["f32-4x7", "bf16-4x3"])
def test_walk_faults_in_bn_act(dtype, lanes, iters, P, Cs, C):
    assert R.geo(Cs, dtype)[2] == lanes and P % (lanes * iters) not in (0,) and lanes * iters - P % (lanes * iters) > lanes
    y, res, dz, sc, sf = _walk_operands(dtype, P, Cs, C, 5)
    assert bool((walk_counts(P, lanes, iters) == 1).all())                                # the walk covers every pixel once
    for fma in (False, True):
        for relu, r in ((0, None), (1, None), (1, res)):
            x, z = act_model(y, sc, sf, r, relu, C, dtype, fma)
            R.check_act("cpu bn_act accept fma=%d relu=%d res=%d" % (fma, relu, r is not None), z, y, sc, sf, r, relu, C, dtype, "")
    x, z = act_model(y, sc, sf, res, 1, C, dtype, True)

    def unvisited(counts):
        bad = z.clone()
        bad[counts == 0] = NAN                                                            # the NaN prefill shows through
        return bad
    skipped = walk_counts(P, lanes, iters, block_stride=lanes * iters + 1)
    assert int((skipped == 0).sum()) > 0
    _rejects(R.check_act, "cpu bn_act REJECT seam pixel skipped", unvisited(skipped), y, sc, sf, res, 1, C, dtype, "")
    nolast = walk_counts(P, lanes, iters, blocks=P // (lanes * iters))
    assert int((nolast == 0).sum()) == P % (lanes * iters)
    _rejects(R.check_act, "cpu bn_act REJECT last ragged block not processed", unvisited(nolast), y, sc, sf, res, 1, C, dtype, "")
    # a pad lane left non-zero
    bad = z.clone()
    bad[P // 2, C] = 0.25
    _rejects(R.check_act, "cpu bn_act REJECT pad lane non-zero", bad, y, sc, sf, res, 1, C, dtype, "")


def apply_model(dz, y, pos, k, dres0, C, dtype, fma, counts=None, overwrite=False):
    """fp32 model of bn_bwd_apply over the live channels: (dy, dres) in the storage type; counts = visits per pixel (dres += g once
    per visit), overwrite = the modelled fault dres = g."""
    P, Cs = dz.shape
    g = dz.double() * pos
    k1, k2, k3 = (torch.zeros(Cs, dtype=torch.float64) for _ in range(3))
    k1[:C], k2[:C], k3[:C] = k[0].double(), k[1].double(), k[2].double()
    yl = y.double()
    dy = f32(k1 * g + f32(k2 * yl + k3)) if fma else f32(f32(f32(k1 * g) + f32(k2 * yl)) + k3)
    dy[:, C:] = 0.0
    live = torch.zeros(Cs, dtype=torch.float64)
    live[:C] = 1.0
    r = torch.zeros(P, Cs, dtype=torch.float64) if overwrite else dres0.double()
    n = 1 if counts is None else int(counts.max())
    for v in range(n):
        m = 1.0 if counts is None else (counts > v).double().reshape(-1, 1)
        r = f32(r + g * live * m).float().to(dtype).double()                              # each visit loads, adds and stores
    return dy.float().to(dtype), r.float().to(dtype)


@pytest.mark.parametrize("dtype,lanes,iters,P,Cs,C", WALKS, ids=["f32-4x7", "bf16-4x3"])
def test_walk_and_accumulate_faults_in_bn_bwd_apply(dtype, lanes, iters, P, Cs, C):
    y, res, dz, sc, sf = _walk_operands(dtype, P, Cs, C, 9)
    _, z = act_model(y, sc, sf, res, 1, C, dtype, True)
    dres0 = _q(13, (P, Cs), dtype)
    k = (rng_normal(14, C), rng_normal(15, C) * 0.3, rng_normal(16, C) * 0.3)
    pos, _ = R.relu_pos("z", z, y, sc, sf, C)
    posf = torch.zeros(P, Cs, dtype=torch.float64)
    posf[:, :C] = pos

    def check(what, dy, dres, mode="acc"):
        return R.check_apply("cpu bn_bwd_apply %s " % what, dy, dres, dres0, mode, dz, y, pos, None, k, C, dtype, "")
    for fma in (False, True):
        dy, dres = apply_model(dz, y, posf, k, dres0, C, dtype, fma)
        check("accept fma=%d" % fma, dy, dres)
    twice = walk_counts(P, lanes, iters, block_stride=lanes * iters - 1)
    assert int((twice == 2).sum()) > 0
    dy2, dres2 = apply_model(dz, y, posf, k, dres0, C, dtype, True, counts=twice.clamp(min=1))
    assert torch.equal(dy2, dy)                                                           # a second visit leaves dy alone ...
    _rejects(check, "REJECT seam pixel visited twice", dy2, dres2)                        # ... and shows in the accumulated dres
    _, over = apply_model(dz, y, posf, k, dres0, C, dtype, True, overwrite=True)
    _rejects(check, "REJECT dres overwritten instead of accumulated", None, over)
    check("accept dres set", None, over, mode="set")
    # a mask byte read at p * G + g with the wrong G (half the row pitch)
    G = Cs // R.vec(dtype)
    bytes_ = R.pack_mask(z > 0, dtype)
    assert torch.equal(R.unpack_mask(bytes_, dtype), z > 0)
    flat = bytes_.reshape(-1)
    wrong = flat[(torch.arange(P).reshape(-1, 1) * (G // 2) + torch.arange(G).reshape(1, -1))]
    posw = R.unpack_mask(wrong, dtype).double()
    posw[:, C:] = 0
    dyw, dresw = apply_model(dz, y, posw, k, dres0, C, dtype, True)
    _rejects(check, "REJECT mask byte at the wrong row pitch (dy)", dyw, None)
    _rejects(check, "REJECT mask byte at the wrong row pitch (dres)", None, dresw)
    # a pad lane of dy left non-zero
    bad = dy.clone()
    bad[3, Cs - 1] = 1.0
    _rejects(check, "REJECT dy pad lane non-zero", bad, None)


def test_mask_predicate_is_the_stored_value():
    """Elements that are positive in fp32 and round to 0 in f16: bn_act's bytes (and the z / sign-byte modes) must say 0 there."""
    P, Cs, C = 64, 32, 28
    y = _q(21, (P, Cs), H16)
    sc, sf = torch.full((C,), 1.0), torch.zeros(C)
    sc[:8] = 2e-8                                                                        # |z| < 2^-25 on these channels
    x, z = act_model(y, sc, sf, None, 1, C, H16, True)
    stored, unrounded = z > 0, x > 0
    assert int((unrounded & ~stored).sum()) > 50                                          # the two predicates differ
    R.check_mask("cpu mask accept stored", R.pack_mask(stored, H16), z, H16, "")
    _rejects(R.check_mask, "cpu mask REJECT unrounded predicate", R.pack_mask(unrounded, H16), z, H16, "")
    # and the backward: gradient let through where the stored z is 0
    dz = _q(22, (P, Cs), H16)
    k = (torch.ones(C), torch.zeros(C), torch.zeros(C))
    pos, _ = R.relu_pos("bits", z, y, sc, sf, C)
    dyf, _ = apply_model(dz, y, unrounded.double(), k, torch.zeros(P, Cs, dtype=H16), C, H16, True)
    dyo, _ = apply_model(dz, y, stored.double(), k, torch.zeros(P, Cs, dtype=H16), C, H16, True)
    R.check_apply("cpu mask bwd accept ", dyo, None, None, None, dz, y, pos, None, k, C, H16, "")
    _rejects(R.check_apply, "cpu mask bwd REJECT unrounded ", dyf, None, None, None, dz, y, pos, None, k, C, H16, "")
    # the remask mode's own predicate IS the unrounded one: its reference accepts it
    posr, amb = R.relu_pos("remask", None, y, sc, sf, C)
    R.check_apply("cpu remask accept ", dyf, None, None, None, dz, y, posr, amb, k, C, H16, "")


# ------------------------------------------------------------------------------------------------ bn_bwd_reduce
def reduce_model(dz, y, pos, mean, istd, chunk, lanes, C, fma, reverse=False, skip_pixel=None, dup_pixel=None, drop_last=False):
    """fp32 model of bn_bwd_reduce over the live channels: per chunk, lane l sums pixels begin + l, begin + l + lanes, ... in order
    (reverse: backwards), then lane 0 adds the other lanes in order.  Returns [chunks, C, 2] as f32."""
    P = dz.shape[0]
    g = dz[:, :C].double() * pos
    w = torch.ones(P, 1, dtype=torch.float64)
    if skip_pixel is not None:
        w[skip_pixel] = 0
    if dup_pixel is not None:
        w[dup_pixel] = 2
    xh = f32(f32(y[:, :C].double() - mean.double()) * istd.double())
    n = (P + chunk - 1) // chunk
    steps = (chunk + lanes - 1) // lanes
    pad = n * steps * lanes - P if chunk % lanes == 0 else None
    assert pad is not None

    def lay(t):
        return torch.cat([t, torch.zeros(pad, t.shape[1], dtype=t.dtype)], 0).reshape(n, steps, lanes, -1)
    g4, x4, w4 = lay(g), lay(xh), lay(w.expand(P, 1).contiguous())
    s1 = torch.zeros(n, lanes, C, dtype=torch.float64)
    s2 = torch.zeros(n, lanes, C, dtype=torch.float64)
    for j in (range(steps - 1, -1, -1) if reverse else range(steps)):
        for v in range(2):                                                                # a doubled pixel is added twice
            m = (w4[:, j] > v).double()
            s1 = f32(s1 + g4[:, j] * m)
            s2 = f32(s2 + g4[:, j] * x4[:, j] * m) if fma else f32(s2 + f32(g4[:, j] * x4[:, j]) * m)
    a1, a2 = s1[:, 0], s2[:, 0]
    for l in range(1, lanes):
        a1, a2 = f32(a1 + s1[:, l]), f32(a2 + s2[:, l])
    out = torch.stack([a1, a2], -1).float()
    if drop_last:
        out[-1] = NAN
    return out


@pytest.mark.parametrize("dtype,Cs,C,P,chunk", [(F32, 256, 252, 452 * 3 + 332, 452), (BF, 512, 508, 228 * 3 + 66, 228),
                                                (H16, 64, 36, 128 * 5 + 71, 128), (H16, 32, 12, 4096 * 2 + 14, 4096)],
                         ids=["f32-chunk452x4", "bf16-chunk228x4", "f16-chunk128x32", "f16-chunk4096x64"])
def test_reduce_bound(dtype, Cs, C, P, chunk):
    """At the chunk x lanes structures of the GPU cases layer1-f32-iters7, layer2-bf16-iters3, f16-cs64 and f16-cs32-chunkcap (the bound is
    linear in K while the error of a sum grows like its square root, so the GPU tier reports ratios far below 1 for this kernel: what
    matters is that one pixel more or less still violates it, which is shown here)."""
    lanes = R.geo(Cs, dtype)[2]
    assert chunk % lanes == 0 and P % chunk != 0
    y, dz, z = _q(31, (P, Cs), dtype), _q(32, (P, Cs), dtype), _q(33, (P, Cs), dtype)
    mean, istd = rng_normal(34, C) * 0.5, rng_normal(35, C).abs() + 0.5
    pos, _ = R.relu_pos("z", z, y, None, None, C)

    def check(what, part):
        return R.check_reduce("cpu bn_bwd_reduce %s " % what, part, dz, y, pos, None, mean, istd, chunk, lanes, C, "")
    for fma in (False, True):
        for rev in (False, True):
            check("accept fma=%d reversed=%d" % (fma, rev), reduce_model(dz, y, pos, mean, istd, chunk, lanes, C, fma, rev))
    _rejects(check, "REJECT pixel skipped at a chunk seam", reduce_model(dz, y, pos, mean, istd, chunk, lanes, C, True, skip_pixel=chunk))
    _rejects(check, "REJECT pixel visited twice at a chunk seam", reduce_model(dz, y, pos, mean, istd, chunk, lanes, C, True, dup_pixel=chunk - 1))
    _rejects(check, "REJECT ragged last chunk not processed", reduce_model(dz, y, pos, mean, istd, chunk, lanes, C, True, drop_last=True))


# ------------------------------------------------------------------------------------------------ reduce_slices and the finalizes
def reduce_slices_model(part, drop_main=None, dup_tail=None):
    """float64 model of reduce_slices + the combine: slice sl of 64 takes rows sl, sl + 64, ...: eight at a time while t + 7 * 64 < n,
    then a tail of up to eight.  drop_main = slice whose first 8-wide trip loses its last row; dup_tail = slice whose last tail row is
    added twice.  Returns float64 (S1, S2) per channel."""
    n, C = part.shape[:2]
    p = part.double()
    tot = torch.zeros(C, 2, dtype=torch.float64)
    hit = False
    for sl in range(min(64, n)):
        s = torch.zeros(C, 2, dtype=torch.float64)
        t, trip = sl, 0
        while t + 7 * 64 < n:
            for u in range(8):
                if drop_main == sl and trip == 0 and u == 7:
                    hit = True
                    continue
                s = s + p[t + u * 64]
            t, trip = t + 8 * 64, trip + 1
        rows = [t + u * 64 for u in range(8) if t + u * 64 < n]
        for r in rows:
            s = s + p[r]
        if dup_tail == sl and rows:
            s = s + p[rows[-1]]
            hit = True
        tot = tot + s
    assert hit or (drop_main is None and dup_tail is None), "the modelled fault did not occur at n = %d" % n
    return tot[:, 0], tot[:, 1]


def finalize_train_model(part, count, gamma, beta, rm0, rv0, fma, **fault):
    S1, S2 = reduce_slices_model(part, **fault)
    mu = S1 / count
    var = (S2 / count - mu * mu).clamp(min=0.0)
    is_ = f32(1.0 / torch.sqrt(var + R.EPS32))
    mean = f32(mu)
    sc = f32(gamma.double() * is_)
    shift = f32(beta.double() - mean * sc) if fma else f32(beta.double() - f32(mean * sc))
    om = f32(torch.tensor(1.0 - R.MOM32, dtype=torch.float64))
    rm = f32(f32(om * rm0.double()) + f32(R.MOM32 * mean))
    unb = var * count / (count - 1.0) if count > 1 else var
    rv = f32(f32(om * rv0.double()) + f32(R.MOM32 * f32(unb)))
    return {"mean": mean.float(), "invstd": is_.float(), "scale": sc.float(), "shift": shift.float(), "rm": rm.float(), "rv": rv.float()}


def _partials(seed, n, C):
    """As the GPU tier's: per-row magnitudes spread over 2^+-6, s2 positive."""
    g = torch.Generator().manual_seed(seed)
    mag = torch.exp2(torch.rand(n, 1, generator=g) * 12 - 6)
    s1 = torch.randn(n, C, generator=g) * mag
    s2 = (torch.randn(n, C, generator=g) ** 2 + 64) * mag
    return torch.stack([s1, s2], -1).float().contiguous()


ROWS = [1, 5, 63, 64, 65, 448, 449, 511, 512, 513, 1023, 3600, 14400]


@pytest.mark.parametrize("n", ROWS)
def test_finalize_bounds_accept_the_model(n):
    C, count = 6, 64 * n
    part = _partials(n, n, C)
    gamma, beta, rm0, rv0 = rng_normal(1, C), rng_normal(2, C), rng_normal(3, C), rng_normal(4, C).abs() + 0.5
    for fma in (False, True):
        got = finalize_train_model(part, count, gamma, beta, rm0, rv0, fma)
        R.check_finalize_train("cpu finalize_train accept n=%d fma=%d " % (n, fma), part, count, gamma, beta, rm0, rv0, got, "")
    mean, istd, dg0, db0 = rng_normal(5, C), rng_normal(6, C).abs() + 0.3, rng_normal(7, C), rng_normal(8, C)
    for fma in (False, True):
        dgamma, dbeta, coef = bwd_finalize_model(part, count + 3, gamma, mean, istd, dg0, db0, fma)
        R.check_bwd_finalize("cpu bwd_finalize accept n=%d fma=%d " % (n, fma), part, count + 3, gamma, mean, istd, dg0, db0, 1, dgamma,
                             dbeta, coef, "")


# the row a fault touches: slice 3's row 3 + 7 * 64 (first 8-wide trip) / slice 0's last tail row
@pytest.mark.parametrize("n", [452, 513, 1023, 3600, 14400])
def test_finalize_rejects_a_row_dropped_by_the_8_wide_loop(n):
    C, count = 6, 64 * n
    part = _partials(n, n, C)
    part[3 + 7 * 64] *= 64.0 / part[3 + 7 * 64, 0, 1].abs().clamp(max=64.0)      # input condition: the row is one of the large ones
    gamma, beta, rm0, rv0 = rng_normal(1, C), rng_normal(2, C), rng_normal(3, C), rng_normal(4, C).abs() + 0.5
    got = finalize_train_model(part, count, gamma, beta, rm0, rv0, True, drop_main=3)
    _rejects(R.check_finalize_train, "cpu finalize_train REJECT dropped row n=%d " % n, part, count, gamma, beta, rm0, rv0, got, "")
    mean, istd, dg0, db0 = rng_normal(5, C), rng_normal(6, C).abs() + 0.3, rng_normal(7, C), rng_normal(8, C)
    bad = bwd_finalize_model(part, count, gamma, mean, istd, dg0, db0, True, drop_main=3)
    _rejects(R.check_bwd_finalize, "cpu bwd_finalize REJECT dropped row n=%d " % n, part, count, gamma, mean, istd, dg0, db0, 1, *bad, "")


@pytest.mark.parametrize("n", [1, 5, 65, 449, 513, 14400])
def test_finalize_rejects_a_tail_row_counted_twice(n):
    C, count = 6, 64 * n
    part = _partials(n, n, C)
    gamma, beta, rm0, rv0 = rng_normal(1, C), rng_normal(2, C), rng_normal(3, C), rng_normal(4, C).abs() + 0.5
    sl = next(s for s in range(min(64, n)) if ((n - s + 63) // 64) % 8 != 0)             # a slice whose tail is not empty
    got = finalize_train_model(part, count, gamma, beta, rm0, rv0, True, dup_tail=sl)
    _rejects(R.check_finalize_train, "cpu finalize_train REJECT tail row twice n=%d " % n, part, count, gamma, beta, rm0, rv0, got, "")
    mean, istd, dg0, db0 = rng_normal(5, C), rng_normal(6, C).abs() + 0.3, rng_normal(7, C), rng_normal(8, C)
    bad = bwd_finalize_model(part, count, gamma, mean, istd, dg0, db0, True, dup_tail=sl)
    _rejects(R.check_bwd_finalize, "cpu bwd_finalize REJECT tail row twice n=%d " % n, part, count, gamma, mean, istd, dg0, db0, 1, *bad, "")


def bwd_finalize_model(part, count, gamma, mean, istd, dg0, db0, fma, k3_sign=-1.0, **fault):
    S1, S2 = reduce_slices_model(part, **fault)
    dbeta, dgamma = f32(db0.double() + f32(S1)), f32(dg0.double() + f32(S2))
    a, b = f32(S1 / count), f32(S2 / count)
    gm, mu, is_ = gamma.double(), mean.double(), istd.double()
    gi = f32(gm * is_)
    k2 = f32(f32(f32(-gm * is_) * is_) * b)
    t = f32(f32(mu * is_) * b + k3_sign * a) if fma else f32(f32(f32(mu * is_) * b) + k3_sign * a)
    k3 = f32(gi * t)
    return dgamma.float(), dbeta.float(), torch.stack([gi, k2, k3]).float()


def test_k3_sign_and_frozen_coefficients():
    n, C = 513, 66
    part = _partials(77, n, C)
    count = 64 * n
    gamma, mean, istd, dg0, db0 = rng_normal(1, C), rng_normal(5, C), rng_normal(6, C).abs() + 0.3, rng_normal(7, C), rng_normal(8, C)
    for fma in (False, True):
        ok = bwd_finalize_model(part, count, gamma, mean, istd, dg0, db0, fma)
        R.check_bwd_finalize("cpu k3 accept fma=%d " % fma, part, count, gamma, mean, istd, dg0, db0, 1, *ok, "")
    bad = bwd_finalize_model(part, count, gamma, mean, istd, dg0, db0, True, k3_sign=+1.0)
    _rejects(R.check_bwd_finalize, "cpu k3 REJECT wrong sign on a ", part, count, gamma, mean, istd, dg0, db0, 1, *bad, "")
    frozen = (ok[0], ok[1], torch.stack([ok[2][0], torch.zeros(C), torch.zeros(C)]))
    R.check_bwd_finalize("cpu frozen accept ", part, count, gamma, mean, istd, dg0, db0, 0, *frozen, "")
    _rejects(R.check_bwd_finalize, "cpu frozen REJECT k2 left in ", part, count, gamma, mean, istd, dg0, db0, 0, *ok, "")


def test_running_var_and_clamp():
    """count == 1 keeps the biased variance (an unbiased one would divide by zero); an all-equal channel is clamped at var = 0."""
    part = torch.tensor([[[0.5, 1.25], [-2.0, 4.5], [0.0, 0.0], [3.0, 9.0]]], dtype=F32)
    one, zero = torch.ones(4), torch.zeros(4)
    got = finalize_train_model(part, 1, one, zero, zero, one * 2, True)
    R.check_finalize_train("cpu count=1 accept ", part, 1, one, zero, zero, one * 2, got, "")
    bad = dict(got)
    bad["rv"] = (0.9 * 2 + 0.1 * torch.tensor([2.0, 1.0, 0.0, 0.0]))                       # "unbiased" with a made-up factor 2
    _rejects(R.check_finalize_train, "cpu count=1 REJECT ", part, 1, one, zero, zero, one * 2, bad, "")
    n = 65
    part = _partials(3, n, 4)
    part[:, 1, 0] = 64 * 1.1
    part[:, 1, 1] = float(torch.tensor(64 * 1.1 * 1.1, dtype=F32)) * (1 - 2.0 ** -20)
    S1, S2, _, _ = R.slice_sums(part)
    assert float(S2[1] / (64 * n) - (S1[1] / (64 * n)) ** 2) < 0
    got = finalize_train_model(part, 64 * n, one, zero, zero, one, True)
    R.check_finalize_train("cpu clamp accept ", part, 64 * n, one, zero, zero, one, got, "")
    bad = dict(got)
    mu = S1 / (64 * n)
    bad["invstd"] = (1.0 / torch.sqrt((S2 / (64 * n) - mu * mu).abs() + R.EPS32)).float()  # |var| instead of the clamp
    bad["scale"] = bad["invstd"]
    _rejects(R.check_finalize_train, "cpu clamp REJECT ", part, 64 * n, one, zero, zero, one, bad, "")


# ------------------------------------------------------------------------------------------------ max-pool
def _pool_input(H, W, dtype, B=2, C=8):
    g = torch.Generator().manual_seed(H * 1000 + W)
    x = torch.tensor([-1.5, 0.0, 2.0])[torch.randint(0, 3, (B, H, W, C), generator=g)].to(dtype)
    return x.double().permute(0, 3, 1, 2).contiguous()


@pytest.mark.parametrize("hw", [(2, 3), (13, 18), (17, 17), (60, 60)], ids=lambda s: "%dx%d" % s)
def test_maxpool_tie_and_border_rules(hw):
    H, W = hw
    x = _pool_input(H, W, BF)
    m, idx, tied = R.pool_first_max(x)
    if H >= 13:
        assert tied > 0.5
    R.check_pool("cpu accept", m, idx, x, "")
    _, last, _ = R.pool_first_max(x, last=True)
    _rejects(R.check_pool, "cpu REJECT tie to the last maximum", m, last, x, "")
    # a clipped window indexing its taps by in-range count: position among the in-range taps instead of r * 3 + s
    taps, Ho, Wo = R.pool_taps(x)
    inr = taps > float("-inf")
    cnt = (inr.cumsum(2) - 1).gather(2, idx.reshape(x.shape[0], x.shape[1], 1, -1)).reshape(idx.shape)
    inner = (slice(None), slice(None), slice(1, Ho), slice(1, Wo - W % 2))               # windows clipped at the top, left or right
    assert bool((cnt != idx).any()) and torch.equal(cnt[inner], idx[inner])               # differ, the others (and the bottom) do not
    _rejects(R.check_pool, "cpu REJECT border taps by in-range count", m, cnt, x, "")
    dy = rng_normal(H + W, *m.shape).to(BF).double()
    dx, _ = R.pool_scatter(dy, idx, H, W)
    R.check_pool_bwd("cpu accept", dx.float().to(BF), dy, idx, BF, "")
    dxl, _ = R.pool_scatter(dy, last, H, W)
    _rejects(R.check_pool_bwd, "cpu REJECT gradient to the last maximum", dxl.float().to(BF), dy, idx, BF, "")


def test_maxpool_single_tap():
    x = _pool_input(1, 1, H16)
    m, idx, tied = R.pool_first_max(x)
    assert tied == 0.0 and bool((idx == 4).all()) and torch.equal(m, x)


# ------------------------------------------------------------------------------------------------ nearest rules
def test_nearest_rule_pin():
    for hf in range(1, 1200):
        hc = (hf + 1) // 2
        assert torch.equal(R.nearest_map(hf, hc), R.torch_nearest_map(hf, hc)), (hf, hc)
    for f in (2, 4, 8):
        for hc in range(1, 151):
            assert torch.equal(R.nearest_map(hc * f, hc), R.torch_nearest_map(hc * f, hc)), (hc * f, hc)
    for hs, ho in ((26, 44), (28, 46), (39, 66)):                                        # outside the set the two rules differ
        assert not torch.equal(R.nearest_map(ho, hs), R.torch_nearest_map(ho, hs)), (hs, ho)


def _children_sum_model(fine, Hc, Wc, floor_rule):
    """Sum over the child ranges [lo, hi) of each coarse pixel, fp32 accumulation in scan order."""
    B, Hf, Wf, C = fine.shape
    hl, hh = R.children(Hf, Hc, floor_rule)
    wl, wh = R.children(Wf, Wc, floor_rule)
    out = torch.zeros(B, Hc, Wc, C, dtype=torch.float64)
    for h in range(Hc):
        for w in range(Wc):
            acc = torch.zeros(B, C, dtype=torch.float64)
            for fh in range(int(hl[h]), int(hh[h])):
                for fw in range(int(wl[w]), int(wh[w])):
                    acc = f32(acc + fine[:, fh, fw].double())
            out[:, h, w] = acc
    return out


@pytest.mark.parametrize("pair", [((26, 24), (13, 12)), ((16, 24), (2, 3)), ((25, 23), (13, 12))], ids=["x2", "x8", "odd"])
def test_children_of_nearest(pair):
    (Hf, Wf), (Hc, Wc) = pair
    for n_out, n_src in ((Hf, Hc), (Wf, Wc)):
        lo, hi = R.children(n_out, n_src)
        m = R.nearest_map(n_out, n_src)
        for s in range(n_src):                                                           # ceil_div ranges are the inverse of the map
            assert torch.equal(torch.nonzero(m == s).reshape(-1), torch.arange(int(lo[s]), int(hi[s])))
    fine = _q(Hf, (2, Hf, Wf, 8), BF)
    ok = _children_sum_model(fine, Hc, Wc, False).float().to(BF)
    R.check_children_sum("cpu children accept", ok, fine, Hc, Wc, BF, "")
    base = _q(Wf, (2, Hc, Wc, 8), BF)
    acc = f32(_children_sum_model(fine, Hc, Wc, False) + base.double()).float().to(BF)
    R.check_children_sum("cpu children accept accumulate", acc, fine, Hc, Wc, BF, "", base=base)
    _rejects(R.check_children_sum, "cpu children REJECT accumulate dropped", ok, fine, Hc, Wc, BF, "", base=base)
    if Hf % Hc:
        # floor instead of ceil_div differs only where the factor is not an integer: the odd sizes of stride-2 stages
        bad = _children_sum_model(fine, Hc, Wc, True).float().to(BF)
        _rejects(R.check_children_sum, "cpu children REJECT floor instead of ceil_div", bad, fine, Hc, Wc, BF, "")
