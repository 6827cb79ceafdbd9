"""Element-wise parity of the streaming kernels (csrc/bn.hip, csrc/resample.hip) against float64.

Every kernel is launched through ops (the stages of the BatchNorm backward, which ops only offers as one chain, through ops.call),
into outputs prefilled with NaN where the kernel must overwrite and with a known pattern where it must accumulate (ops' own
allocations are NaN-filled through _NanAlloc), and EVERY element is compared with a float64 reference computed from exactly the operand
values the kernel reads: inputs are quantised through the storage type first, and stage n + 1 of a chain is referenced from the
DEVICE's stage-n output (mean / invstd / scale / shift, the chunk partials, k1 / k2 / k3), so each kernel is judged alone.

Bounds (helpers.check_elementwise; `roundings(n)` = n fp32 roundings on the magnitude, nothing fitted):
  bn_finalize_train  float64 sum of the f32 partials as stored.  mean, invstd: one rounding + the fp64 noise n 2^-53 sum|partial| /
                     count (for invstd carried through var = s2 / count - mu^2 relative to var + eps).  scale 1, shift 2 (on |b| +
                     |mu sc|), running_mean 4, running_var 5 roundings (1 - m, the cast, two products, the sum).
  bn_act             y * scale + shift (+ res), ReLU: 3 roundings on |y scale| + |shift| + |res| + half an output spacing.  Pad lanes
                     are exactly 0.  The mask bytes [P][Cs / V] equal (stored z > 0) bit for bit; the reference sign can differ from
                     the stored one only within the bound (implied: |ref| <= |got - ref| there).
  bn_bwd_reduce      per chunk and channel float64 sums over the chunk's own pixels of g and g * xhat; K = ceil(chunk / lanes) + lanes
                     sequential terms, + 3 roundings for xhat.
  bn_bwd_finalize    float64 sum of the device partials, landing on prefilled dgamma / dbeta (2 roundings); k1 1, k2 4, k3 7 roundings,
                     k3 on |gamma is| (|mu is b| + |a|) because it cancels.  Frozen: k2 = k3 = 0 exactly.
  bn_bwd_apply       k1 g + k2 y + k3 from the device's coefficients: 4 roundings; dres = g exactly, dres += g one rounding.
  max-pool           forward torch.equal with float64 F.max_pool2d; idx equals the first maximum in window coordinates; backward the
                     float64 scatter by that idx (K = 4).
  nearest kernels    copies torch.equal with an index-map gather; sums over children K = children (+ 1 with accumulate).
  det / relu / add / layout   exact, or one rounding where a sum is stored.
ReLU mask predicates: z and sign-bit modes use the STORED (rounded) z > 0; remask recomputes y * scale + shift > 0 in fp32 without
rounding to the storage type.  The remask reference takes the float64 sign and accepts either sign where |y scale + shift| is within
3 roundings of zero.

The nearest index maps are built from the kernels' integer rule floor(o * Hs / Ho) (stream_ref.nearest_map); all shapes used are also
inside the set where torch's rule agrees (tests/test_stream_parity_cpu.py pins that set).

Launch plans: stream_ref mirrors Geo, pick_iters and reduce_chunk; every BN case states the (lanes, iters, grid.x, grid.y, chunks) it is
meant to reach and asserts it (chunks also against mpn_bn_bwd_chunks) before launching, so a change of the block target fails here
instead of shrinking coverage.  iters is 7 / 3 / 1 at the configured shapes; the cap of 32 needs >= 268 M elements, which no
configured shape reaches, and is not chased."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import stream_ref as R
from helpers import U24, report, rng_normal, ulp_out
from stream_ref import BF, F32, H16, roundings

pytestmark = pytest.mark.gpu

DTYPES = [BF, H16, F32]
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
    """Inside the block, ops' torch.empty / empty_like return NaN-filled (0xff for integer types) tensors, so an element a kernel
    leaves unwritten cannot hold a stale correct value."""

    class _Shim(object):
        def __getattr__(self, k):
            return getattr(torch, k)

        @staticmethod
        def _fill(t):
            return t.fill_(NAN) if t.is_floating_point() else t.fill_(255)

        def empty(self, *a, **k):
            return self._fill(torch.empty(*a, **k))

        def empty_like(self, *a, **k):
            return self._fill(torch.empty_like(*a, **k))

    def __enter__(self):
        self.ops = _ops()
        self.ops.torch = self._Shim()
        return self.ops

    def __exit__(self, *exc):
        self.ops.torch = torch
        torch.cuda.synchronize()
        return False


def _dn(dtype):
    return {BF: "bf16", H16: "f16", F32: "f32"}[dtype]


def _rand(seed, shape, dtype, scale=1.0):
    """Unit normals quantised through `dtype` (CPU tensor of that dtype)."""
    return (rng_normal(seed, *shape) * scale).to(dtype)


def _act(t, C):
    from multiposenet.pytorch_amd.ops import Act
    return Act(t.cuda(), C)


_check, _exact = R.check_rows, R.exact


# ===================================================================================================== bn_finalize_train / bwd_finalize
ROWS = [1, 5, 63, 64, 65, 448, 449, 511, 512, 513, 1023, 3600, 14400]
# reduce_slices per slice of 64: rows/64 < 8 -> tail only (1 .. 511: 449 = first n whose slice 0 has 8 rows and takes the main loop once,
# 448 / 511 around it); 512 / 513: main loop for every / one slice plus a one-row tail; 1023, 3600, 14400: several trips (225 .. 14 400
# conv tiles in production)


def _partials(seed, n, C):
    """[n, C, 2] f32 rows with per-row magnitudes spread over 2^+-6; s2 rows are positive and large enough that var > 0 (count =
    64 n).  A dropped or doubled row moves a sum by far more than the bound."""
    g = torch.Generator().manual_seed(seed)
    mag = torch.exp2(torch.rand(n, 1, generator=g) * 12 - 6)
    s1 = torch.randn(n, C, generator=g) * mag
    s2 = (torch.randn(n, C, generator=g) ** 2 + 64) * mag
    return torch.stack([s1, s2], -1).float().contiguous()


def _chan_cases(n):
    return [4, 6, 66] + ([2048] if n in (1, 449, 512, 14400) else [])


@pytest.mark.parametrize("n", ROWS)
def test_bn_finalize_train(n):
    ops = _ops()
    for C in _chan_cases(n):
        count = 64 * n
        part = _partials(1000 + n + C, n, C)
        # channel 1: all values equal (s1 = 64 v, s2 just under 64 v^2): var < 0 in exact arithmetic, the clamp decides invstd
        v = 1.1
        part[:, 1, 0] = 64 * v
        part[:, 1, 1] = float(torch.tensor(64 * v * v, dtype=F32)) * (1 - 2.0 ** -20)
        g = torch.Generator().manual_seed(n * 7 + C)
        gamma, beta, rm0 = (torch.randn(C, generator=g) for _ in range(3))
        rv0 = torch.rand(C, generator=g) + 0.5
        rm, rv = rm0.clone().cuda(), rv0.clone().cuda()
        with _NanAlloc():
            st = ops.bn_finalize_train(part.cuda(), count, gamma.cuda(), beta.cuda(), rm, rv)
        S1, S2, _, _ = R.slice_sums(part)
        assert float(S2[1] / count - (S1[1] / count) ** 2) < 0                                 # the clamp case is a clamp case
        got = {"mean": st.mean, "invstd": st.invstd, "scale": st.scale, "shift": st.shift, "rm": rm, "rv": rv}
        R.check_finalize_train("bn_finalize_train n=%d C=%d " % (n, C), part, count, gamma, beta, rm0, rv0, got,
                               "rows=%d C=%d blocks=%d" % (n, C, (C + 3) // 4))


def test_bn_finalize_train_count_one_keeps_biased_variance():
    ops = _ops()
    part = torch.tensor([[[0.5, 1.25], [-2.0, 4.5], [0.0, 0.0], [3.0, 9.0]]], dtype=F32)          # var = 1, 0.5, 0, 0
    rv = torch.full((4,), 2.0).cuda()
    with _NanAlloc():
        st = ops.bn_finalize_train(part.cuda(), 1, None, None, None, rv)
    assert R.finalize_train_ref(part, 1)[1].tolist() == [1.0, 0.5, 0.0, 0.0]
    got = {"mean": st.mean, "invstd": st.invstd, "scale": st.scale, "shift": st.shift, "rv": rv}
    R.check_finalize_train("bn_finalize_train count=1 (gamma, beta, running_mean null) ", part, 1, None, None, None, torch.full((4,), 2.0),
                           got, "rows=1 C=4")


@pytest.mark.parametrize("n", ROWS)
def test_bn_bwd_finalize(n):
    ops = _ops()
    for C in _chan_cases(n):
        count = 64 * n + 3
        part = _partials(2000 + n + C, n, C)
        part[..., 1] = part[..., 1] * torch.sign(rng_normal(n + C, n, C))              # sum g * xhat has both signs
        g = torch.Generator().manual_seed(n * 11 + C)
        gamma, mean, dg0, db0 = (torch.randn(C, generator=g) for _ in range(4))
        istd = torch.rand(C, generator=g) * 3 + 0.1
        route = "rows=%d C=%d blocks=%d" % (n, C, (C + 3) // 4)
        for train in (1, 0):
            dgamma, dbeta = dg0.clone().cuda(), db0.clone().cuda()
            coef = torch.full((3, C), NAN).cuda()
            dev = [t.cuda() for t in (part, gamma, mean, istd)]
            ops.call("mpn_bn_bwd_finalize", ops.ptr(dev[0]), n, C, count, ops.ptr(dev[1]), ops.ptr(dev[2]), ops.ptr(dev[3]), train,
                     ops.ptr(dgamma), ops.ptr(dbeta), ops.ptr(coef), ops.stream_ptr())
            torch.cuda.synchronize()
            R.check_bwd_finalize("bn_bwd_finalize n=%d C=%d %s " % (n, C, "train" if train else "frozen"), part, count, gamma, mean, istd,
                                 dg0, db0, train, dgamma, dbeta, coef, route)


# ===================================================================================================== the BN streaming kernels
# id, dtype, B, H, W, C, Cs, (lanes, iters, grid.x, grid.y, chunks), what runs
BN_CASES = [
    # layer1's 256-channel geometry (cfg3: R101 480^2, P = B 120 120) in f32 at B = 16, the smallest tensor that reaches iters 7:
    # 230 400 % 28 = 16, so the last block breaks at it = 4, and an image ends inside a block (14 400 % 28 = 8); 510 chunks of 452 pixels
    # (450 rounded up to the lanes: the middle range of the chunk plan), the last ragged
    ("layer1-f32-iters7", F32, 16, 120, 120, 256, 256, (4, 7, 8229, 1, 510), "big"),
    # layer2's 512-channel geometry in bf16 (cfg3: P = 115 200) at a ragged neighbour: iters 3, 115 206 % 12 = 6 (it 0 full, it 1 half the
    # lanes, it 2 breaks), image 57 603 % 12 = 3; 506 chunks of 228 pixels, the last ragged
    ("layer2-bf16-iters3", BF, 2, 273, 211, 512, 512, (4, 3, 9601, 1, 506), "big"),
    ("bf16-cs32-smallP", BF, 2, 9, 7, 20, 32, (64, 1, 2, 1, 1), "all"),                 # G = 4, 64 lanes; P / 512 < 4 lanes: one chunk
    ("f16-cs64", H16, 3, 37, 41, 36, 64, (32, 1, 143, 1, 36), "all"),                   # chunk at the low clamp, ragged
    ("f16-cs256", H16, 2, 23, 19, 252, 256, (8, 1, 110, 1, 28), "all"),
    ("bf16-cs2048", BF, 2, 15, 15, 2044, 2048, (1, 1, 450, 1, 113), "all"),             # GB = 256, one pixel lane
    ("f32-cs2048-two-yblocks", F32, 2, 7, 9, 2044, 2048, (1, 1, 126, 2, 32), "all"),    # G = 512: blockIdx.y = 1
    ("f32-cs32", F32, 2, 9, 7, 12, 32, (32, 1, 4, 1, 1), "all"),
    # P / 512 > 4096: chunk at the high clamp (4096 pixels), last chunk 14 pixels (reduce only; 12 live channels keep the float64 side small)
    ("f16-cs32-chunkcap", H16, 2, 1025, 1031, 12, 32, (64, 4, 8257, 1, 517), "reduce"),
]


class _BN(object):
    """Operands of one case, quantised through the storage type; float64 copies over the live channels are made on demand."""

    def __init__(self, cid, dtype, B, H, W, C, Cs, want, what):
        ops = _ops()
        self.cid, self.dtype, self.C, self.Cs, self.P, self.what = cid, dtype, C, Cs, B * H * W, what
        self.shape = (B, H, W, Cs)
        self.plan = R.plan(self.P, Cs, dtype)
        assert self.plan == want, "%s: the launch plan is %s, the case was written for %s" % (cid, self.plan, want)
        assert ops.call("mpn_bn_bwd_chunks", self.P, Cs, ops.dtype_code(dtype)) == want[4], cid
        lanes, iters = want[0], want[1]
        if iters > 1:
            rem = self.P % (lanes * iters)
            assert rem != 0 and lanes * iters - rem > lanes and (H * W) % (lanes * iters) != 0, (cid, rem)
        self.chunk = R.reduce_chunk(self.P, lanes)
        assert self.P % self.chunk != 0 or want[4] == 1, cid
        self.route = "%s C=%d Cs=%d P=%d plan=%s" % (_dn(dtype), C, Cs, self.P, want)
        seed = sum(ord(c) for c in cid)
        self.y = _rand(seed, self.shape, dtype)                       # pad lanes hold finite junk: the kernels must write zeros there
        self.dz = _rand(seed + 1, self.shape, dtype)
        self.res = _rand(seed + 2, self.shape, dtype) if what != "reduce" else None
        g = torch.Generator().manual_seed(seed + 3)
        self.gamma = torch.randn(C, generator=g)
        self.gamma[1] = 3e-8                                          # channel 1: z underflows the f16 range (rounds to 0 / a subnormal)
        self.beta = torch.randn(C, generator=g) * 0.5
        self.beta[1] = 0.0

    def flat(self, t):
        return t.reshape(self.P, self.Cs)

    def live(self, t):
        return self.flat(t)[:, : self.C].double()

    def stats(self):
        """Per-128-pixel-tile (sum, sum^2) of y, float64 rounded to f32: what the conv epilogue hands to the finalize."""
        y = self.live(self.y)
        return torch.stack([R.chunk_sums(y, 128), R.chunk_sums(y * y, 128)], -1).float().contiguous()


def _forward(b, st, relu, res, mask):
    ops = _ops()
    tag = "bn_act %s relu=%d res=%d mask=%d" % (b.cid, relu, res, mask)
    with _NanAlloc():
        z = ops.bn_act(_act(b.y, b.C), st, bool(relu), res=_act(b.res, b.C) if res else None, want_mask=bool(mask))
    zc = b.flat(z.t.cpu())
    w, ref = R.check_act(tag, zc, b.flat(b.y), st.scale.cpu(), st.shift.cpu(), b.flat(b.res) if res else None, relu, b.C, b.dtype, b.route)
    if mask:
        assert z.mask.is_contiguous()
        R.check_mask(tag, z.mask, zc, b.dtype, b.route)
    if b.dtype == H16 and relu and not res:
        # input condition: some live elements are positive before rounding and 0 as stored (where the two mask predicates differ)
        assert bool(((ref[:, 1] > 0) & (zc[:, 1] == 0)).any()), b.cid
    return z, w


def _pos_from(b, mode, z, st):
    return R.relu_pos(mode, b.flat(z.t.cpu()) if z is not None else None, b.flat(b.y), st.scale.cpu(), st.shift.cpu(), b.C)


def _reduce(b, st, mode, z):
    ops = _ops()
    dc = ops.dtype_code(b.dtype)
    lanes, chunks = b.plan[0], b.plan[4]
    part = torch.full((chunks, b.C, 2), NAN).cuda()
    yd, dzd = b.y.cuda(), b.dz.cuda()
    relu, remask = mode != "none", mode == "remask"
    ops.call("mpn_bn_bwd_reduce", ops.ptr(dzd), ops.ptr(z.t) if (relu and not remask) else None, ops.ptr(yd), ops.ptr(st.mean),
             ops.ptr(st.invstd), ops.ptr(st.scale) if remask else None, ops.ptr(st.shift) if remask else None, ops.ptr(part),
             chunks, b.P, b.C, b.Cs, 1 if relu else 0, dc, ops.stream_ptr())
    torch.cuda.synchronize()
    pos, amb = _pos_from(b, mode, z, st)
    w = R.check_reduce("bn_bwd_reduce %s mask=%s " % (b.cid, mode), part, b.flat(b.dz), b.flat(b.y), pos, amb, st.mean.cpu(), st.invstd.cpu(),
                       b.chunk, lanes, b.C, b.route)
    return part, w


def _bwd_finalize(b, st, part, train):
    ops = _ops()
    chunks = part.shape[0]
    g = torch.Generator().manual_seed(b.P + b.C)
    dg0, db0 = torch.randn(b.C, generator=g), torch.randn(b.C, generator=g)
    dgamma, dbeta = dg0.clone().cuda(), db0.clone().cuda()
    coef = torch.full((3, b.C), NAN).cuda()
    gdev = b.gamma.cuda()
    ops.call("mpn_bn_bwd_finalize", ops.ptr(part), chunks, b.C, b.P, ops.ptr(gdev), ops.ptr(st.mean), ops.ptr(st.invstd),
             train, ops.ptr(dgamma), ops.ptr(dbeta), ops.ptr(coef), ops.stream_ptr())
    torch.cuda.synchronize()
    w = R.check_bwd_finalize("bn_bwd_finalize %s %s " % (b.cid, "train" if train else "frozen"), part.cpu(), b.P, b.gamma, st.mean.cpu(),
                             st.invstd.cpu(), dg0, db0, train, dgamma, dbeta, coef, b.route)
    return coef, w


def _apply(b, st, mode, z, k, want_dy, dres_mode):
    """One bn_bwd_apply launch: k = (k1, k2, k3) device vectors (k2 = k3 = None: frozen); dres_mode None / 'set' / 'acc'."""
    ops = _ops()
    dc = ops.dtype_code(b.dtype)
    relu, remask, bits = mode != "none", mode == "remask", mode == "bits"
    dy = torch.full(b.shape, NAN, dtype=b.dtype).cuda() if want_dy else None
    dres0 = b.res if dres_mode == "acc" else None                     # the prefill of the accumulate mode: any known tensor
    dres = None if dres_mode is None else (dres0.clone().cuda() if dres_mode == "acc" else torch.full(b.shape, NAN, dtype=b.dtype).cuda())
    tag = "bn_bwd_apply %s mask=%s dy=%d dres=%s%s " % (b.cid, mode, want_dy, dres_mode, "" if k[1] is not None else " frozen")
    if bits and not want_dy and dres_mode == "set":
        ops.masked_copy(_act(b.dz, b.C), z.mask, ops.Act(dres, b.C))
    else:
        yd, dzd = b.y.cuda(), b.dz.cuda()
        ops.call("mpn_bn_bwd_apply", ops.ptr(dzd), ops.ptr(z.t) if mode == "z" else None, ops.ptr(yd), ops.ptr(k[0]), ops.ptr(k[1]),
                 ops.ptr(k[2]), ops.ptr(st.scale) if remask else None, ops.ptr(st.shift) if remask else None, ops.ptr(dy), ops.ptr(dres),
                 1 if dres_mode == "acc" else 0, b.P, b.C, b.Cs, 1 if relu else 0, dc, ops.ptr(z.mask) if bits else None, ops.stream_ptr())
    torch.cuda.synchronize()
    pos, amb = _pos_from(b, mode, z, st)
    return R.check_apply(tag, b.flat(dy.cpu()) if dy is not None else None, b.flat(dres.cpu()) if dres is not None else None,
                         b.flat(dres0) if dres0 is not None else None, dres_mode, b.flat(b.dz), b.flat(b.y), pos, amb,
                         tuple(t.cpu() if t is not None else None for t in k), b.C, b.dtype, b.route)


@pytest.mark.parametrize("case", BN_CASES, ids=[c[0] for c in BN_CASES])
def test_bn_stream_kernels(case):
    ops = _ops()
    b = _BN(*case)
    g = torch.Generator().manual_seed(b.P)
    rm, rv = torch.randn(b.C, generator=g).cuda(), (torch.rand(b.C, generator=g) + 0.5).cuda()
    with _NanAlloc():
        st = ops.bn_finalize_train(b.stats().cuda(), b.P, b.gamma.cuda(), b.beta.cuda(), rm, rv)
    for t in (st.mean, st.invstd, st.scale, st.shift):
        assert bool(torch.isfinite(t).all()), b.cid
    worst = {}
    if b.what == "reduce":
        z = _act(_rand(7, b.shape, b.dtype), b.C)                     # any tensor serves as the mask source of the z mode
        _, worst["reduce"] = _reduce(b, st, "z", z)
    else:
        fwd = [(1, 1, 1)] if b.what == "big" else [(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 1)]
        wf = []
        for relu, res, mask in fwd:
            z, w = _forward(b, st, relu, res, mask)                   # the last one (relu + res + mask) is the backward's mask source
            wf.append(w)
        worst["act"] = max(wf)
        zplain = ops.Act(z.t, b.C)                                    # the same z without sign bytes: the z mode
        modes = ["z"] if b.what == "big" else ["none", "z", "remask"]
        wr, parts = [], {}
        for m in modes:
            parts[m], w = _reduce(b, st, m, zplain)
            wr.append(w)
        worst["reduce"] = max(wr)
        coef, worst["finalize"] = _bwd_finalize(b, st, parts["z"], 1)
        k = (coef[0], coef[1], coef[2])
        wa = [_apply(b, st, "bits", z, k, True, "acc")]                  # the largest cases run this one launch: dy and dres += together
        if b.what == "all":
            _, w = _bwd_finalize(b, st, parts["z"], 0)
            worst["finalize"] = max(worst["finalize"], w)
            wa += [_apply(b, st, "none", None, k, True, None),
                   _apply(b, st, "z", zplain, k, True, "set"),
                   _apply(b, st, "bits", z, k, False, "set"),          # ops.masked_copy
                   _apply(b, st, "z", zplain, k, False, "acc"),
                   _apply(b, st, "remask", None, k, True, "set"),
                   _apply(b, st, "remask", None, k, True, "acc"),
                   _apply(b, st, "z", zplain, (st.scale, None, None), True, "acc")]      # frozen: k2 = k3 = null
        worst["apply"] = max(wa)
    report("SUMMARY bn %-28s %s worst err/bound: %s" % (b.cid, b.route, "  ".join("%s=%.3f" % kv for kv in sorted(worst.items()))))


@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
def test_bn_end_to_end_vs_float64_autograd(dtype):
    """finalize -> bn_act(+ res, ReLU, sign bytes) -> ops.bn_backward against float64 F.batch_norm autograd: catches an error in the
    staging itself.  The bound is the product of the stage bounds: with kappa = max_c E[y^2] / (var + eps) (the conditioning of the
    variance; the f32 tile sums carry one rounding each, so d invstd / invstd <= 1.5 kappa 2^-24 and scale inherits it),
      z      : 3 (bn_act) + 2 (shift) + 2 (scale, mean) + 1.5 kappa roundings on |y scale| + |mu scale| + |beta| + |res|;
      dy     : K_reduce + 3 (reduce) + 7 (finalize) + 4 (apply) + 2 + 4.5 kappa (invstd in k1, in xhat of b, in k2 y + k3) roundings on
               |gamma is| (|g| + mean|g| + xhat_abs mean|g xhat_abs|), xhat_abs = (|y| + |mu|) is;
      dgamma : K_reduce + 3 + 2 + 1.5 kappa + 2 on sum |g| xhat_abs;  dbeta: K_reduce + 2 on sum |g|;  dres = g exactly.
    The residual is built so that no pre-activation lies near zero (asserted), so the ReLU mask is the same on both sides."""
    ops = _ops()
    B, H, W, C, Cs = 4, 24, 24, 36, 64
    P = B * H * W
    lanes, iters, gx, gy, chunks = R.plan(P, Cs, dtype)
    assert iters == 1 and gy == 1
    y = _rand(31, (B, H, W, Cs), dtype)
    y[..., C:] = 0
    dz = _rand(32, (B, H, W, Cs), dtype)
    g = torch.Generator().manual_seed(33)
    gamma, beta = torch.randn(C, generator=g) + 1.5, torch.randn(C, generator=g) * 0.5
    y64 = y.reshape(P, Cs)[:, :C].double().requires_grad_(True)
    gm64, bt64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    bn = F.batch_norm(y64.t().reshape(1, C, P), None, None, gm64, bt64, True, 0.1, R.EPS32).reshape(C, P).t()
    want = torch.sign(rng_normal(34, P, C)) * (1 + rng_normal(35, P, C).abs())
    res = torch.zeros(B, H, W, Cs)
    res.reshape(P, Cs)[:, :C] = (want - bn.detach()).float()
    res = res.to(dtype)
    r64 = res.reshape(P, Cs)[:, :C].double().requires_grad_(True)
    pre = bn + r64
    dz64 = dz.reshape(P, Cs)[:, :C].double()
    (pre.clamp(min=0) * dz64).sum().backward()
    mu = y64.detach().mean(0)
    var = y64.detach().var(0, unbiased=False)
    is_ = 1 / torch.sqrt(var + R.EPS32)
    kappa = float(((y64.detach() ** 2).mean(0) / (var + R.EPS32)).max())
    stats = torch.stack([R.chunk_sums(y64.detach(), 128), R.chunk_sums(y64.detach() ** 2, 128)], -1).float().contiguous()
    dgamma, dbeta = torch.zeros(C).cuda(), torch.zeros(C).cuda()
    with _NanAlloc():
        st = ops.bn_finalize_train(stats.cuda(), P, gamma.cuda(), beta.cuda(), None, None)
        yA = _act(y, C)
        z = ops.bn_act(yA, st, True, res=_act(res, C), want_mask=True)
        dres = ops.Act(torch.full((B, H, W, Cs), NAN, dtype=dtype).cuda(), C)
        dy = ops.bn_backward(_act(dz, C), z, yA, st, gamma.cuda(), True, True, dgamma=dgamma, dbeta=dbeta, want_dy=True, dres=dres)
    route = "%s plan=%s kappa=%.2f" % (_dn(dtype), (lanes, iters, gx, gy, chunks), kappa)
    yd = y64.detach()
    sc = gamma.double() * is_
    zmag = (yd * sc).abs() + (mu * sc).abs() + beta.double().abs() + r64.detach().abs()
    nz = 7 + 1.5 * kappa
    zb = 0.5 * ulp_out(pre.detach(), dtype) + nz * U24 * zmag
    assert bool((pre.detach().abs() > 100 * zb).all()), "a pre-activation lies near zero: the ReLU mask would be ambiguous"
    tag = "bn end-to-end %s " % _dn(dtype)
    _check(tag + "z", z.t.reshape(P, Cs)[:, :C], pre.detach().clamp(min=0), zmag, dtype, route, **roundings(nz))
    gmask = dz64 * (pre.detach() > 0)
    xa = (yd.abs() + mu.abs()) * is_
    Kr = (R.reduce_chunk(P, lanes) + lanes - 1) // lanes + lanes
    dymag = sc.abs() * (gmask.abs() + gmask.abs().mean(0) + xa * (gmask.abs() * xa).mean(0))
    _check(tag + "dy", dy.t.reshape(P, Cs)[:, :C], y64.grad, dymag, dtype, route, k_step=1, K=Kr, extra_terms=16 + 4.5 * kappa - 3)
    _check(tag + "dgamma", dgamma, gm64.grad, (gmask.abs() * xa).sum(0), F32, route, "c", k_step=1, K=Kr, extra_terms=7 + 1.5 * kappa - 3)
    _check(tag + "dbeta", dbeta, bt64.grad, gmask.abs().sum(0), F32, route, "c", k_step=1, K=Kr, extra_terms=2 - 3)
    _exact(tag + "dres", dres.t.reshape(P, Cs)[:, :C].double(), r64.grad, route)
    assert bool((dy.t.reshape(P, Cs)[:, C:] == 0).all())


# ===================================================================================================== max-pool
POOL_SHAPES = [(1, 1), (2, 3), (13, 18), (17, 17), (240, 240)]


@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
@pytest.mark.parametrize("hw", POOL_SHAPES, ids=lambda s: "%dx%d" % s)
def test_maxpool_ties_and_clipped_windows(hw, dtype):
    """Inputs from a 3-value alphabet (a negative, 0, a positive), so most windows have a tied maximum: the gradient must go to the
    FIRST maximum in scan order over the in-range taps, indexed by window position r * 3 + s (also in the clipped windows of odd sizes
    and at H, W of 1 or 2)."""
    ops = _ops()
    H, W = hw
    B, Cs = 2, 64
    g = torch.Generator().manual_seed(H * 1000 + W)
    x = torch.tensor([-1.5, 0.0, 2.0])[torch.randint(0, 3, (B, H, W, Cs), generator=g)].to(dtype)
    xn = x.double().permute(0, 3, 1, 2).contiguous()
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    route = "%s B=%d %dx%d->%dx%d Cs=%d" % (_dn(dtype), B, H, W, Ho, Wo, Cs)
    with _NanAlloc():
        xa = _act(x, Cs)
        ya, di = ops.maxpool_forward(xa, needs_grad=True)
    idx, tied = R.check_pool(route, ya.t.cpu().permute(0, 3, 1, 2), di.cpu().permute(0, 3, 1, 2), xn, route)
    report("maxpool %s: %.2f of the windows have a tied maximum" % (route, tied))
    if H >= 13 and W >= 13:
        assert tied > 0.5, "only %.2f of the windows have a tied maximum" % tied          # a condition on the inputs
    dy = _rand(H + W, (B, Ho, Wo, Cs), dtype)
    with _NanAlloc():
        dx = ops.maxpool_backward(_act(dy, Cs), di, xa)
    R.check_pool_bwd(route, dx.t.cpu().permute(0, 3, 1, 2), dy.permute(0, 3, 1, 2), idx, dtype, route)


# ===================================================================================================== nearest resampling
# (fine H, W) -> (coarse H, W): factors 2, 4, 8 and the odd fine sizes with Hc = ceil(Hf / 2) that stride-2 stages produce
NEAREST = [((26, 24), (13, 12)), ((16, 20), (4, 5)), ((16, 24), (2, 3)), ((25, 115), (13, 58)), ((115, 25), (58, 13))]


def _nid(p):
    return "%dx%d-%dx%d" % (p[0] + p[1])


@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
@pytest.mark.parametrize("pair", NEAREST, ids=_nid)
def test_upsample_backward(pair, dtype):
    ops = _ops()
    (Hf, Wf), (Hc, Wc) = pair
    for n_out, n_src in ((Hf, Hc), (Wf, Wc)):
        assert torch.equal(R.nearest_map(n_out, n_src), R.torch_nearest_map(n_out, n_src))       # inside the agreeing set
    B, Cs = 2, 32
    fine = _rand(Hf * Wf, (B, Hf, Wf, Cs), dtype)
    c0 = _rand(Hc + Wc, (B, Hc, Wc, Cs), dtype)
    for acc in (False, True):
        route = "%s %dx%d<-%dx%d acc=%d" % (_dn(dtype), Hc, Wc, Hf, Wf, acc)
        dc = ops.Act(c0.clone().cuda() if acc else torch.full((B, Hc, Wc, Cs), NAN, dtype=dtype).cuda(), Cs)
        ops.upsample_backward(_act(fine, Cs), dc, acc)
        torch.cuda.synchronize()
        R.check_children_sum("upsample_backward " + route, dc.t, fine, Hc, Wc, dtype, route, base=c0 if acc else None)


@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
@pytest.mark.parametrize("c_off", [0, 128, 384])
def test_upsample_slice_and_backward(c_off, dtype):
    ops = _ops()
    B, Csrc, Cdst = 2, 128, 512
    for (Hf, Wf), (Hc, Wc) in NEAREST[:4]:
        route = "%s %dx%d->%dx%d c_off=%d of %d" % (_dn(dtype), Hc, Wc, Hf, Wf, c_off, Cdst)
        src = _rand(Hc * Wf + c_off, (B, Hc, Wc, Csrc), dtype)
        dst0 = _rand(Hf + c_off, (B, Hf, Wf, Cdst), dtype)
        dst = ops.Act(dst0.clone().cuda(), Cdst)
        ops.upsample_slice(_act(src, Csrc), dst, c_off)
        torch.cuda.synchronize()
        want = dst0.clone()
        want[..., c_off:c_off + Csrc] = R.gather_nearest(src, Hf, Wf)
        _exact("upsample_slice " + route, dst.t.cpu().double(), want.double(), route)          # the other channels untouched
        dsrc = ops.Act(torch.full((B, Hc, Wc, Csrc), NAN, dtype=dtype).cuda(), Csrc)
        ops.upsample_slice_backward(_act(dst0, Cdst), dsrc, c_off)
        torch.cuda.synchronize()
        R.check_children_sum("upsample_slice_backward " + route, dsrc.t, dst0[..., c_off:c_off + Csrc], Hc, Wc, dtype, route)


@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
def test_export_f32_and_import_grad(dtype):
    ops = _ops()
    B, C, Cs = 2, 17, 32
    for (Ho, Wo), (Hs, Ws) in NEAREST + [((7, 9), (7, 9))]:
        route = "%s %dx%d->%dx%d C=%d Cs=%d" % (_dn(dtype), Hs, Ws, Ho, Wo, C, Cs)
        src = _rand(Ho * Ws, (B, Hs, Ws, Cs), dtype)
        with _NanAlloc():
            out = ops.export_f32(_act(src, C), C, Ho, Wo)
        assert out.shape == (B, C, Ho, Wo)
        _exact("export_f32 " + route, out.cpu().double(), R.gather_nearest(src, Ho, Wo)[..., :C].double().permute(0, 3, 1, 2), route)
        g = rng_normal(Ho + Ws, B, C, Ho, Wo)
        wide = rng_normal(Ho + Ws + 1, B, Ho, Wo, C + 11)
        forms = {"nchw-contiguous (copied)": g.cuda(),                                                   # stride(3) != 1: .contiguous()
                 "channels-last (in place)": g.cuda().contiguous(memory_format=torch.channels_last),
                 "slice of a wider NHWC (pixel stride 28)": wide.cuda()[..., 5:5 + C].permute(0, 3, 1, 2)}
        like = _act(src, C)
        for form, gt in forms.items():
            with _NanAlloc():
                d = ops.import_grad(gt, like, dtype)
            R.check_children_sum("import_grad %s %s" % (route, form), d.t[..., :C], gt.cpu().permute(0, 2, 3, 1), Hs, Ws, dtype, route)
            R.pad_zero("import_grad " + route, d.t, C)


# ===================================================================================================== det heads, relu, add, layout
@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
@pytest.mark.parametrize("K", [1, 3, 80])
def test_det_pack_unpack_pyramid(K, dtype):
    """Five levels packed into one [B, A, K] buffer (dst_sB = A * K > HW * C of any level) and unpacked from it again."""
    ops = _ops()
    B, C = 2, 9 * K
    Cs = (C + 31) // 32 * 32
    assert Cs == {1: 32, 3: 32, 80: 736}[K]
    levels = [(8, 10), (4, 5), (2, 3), (1, 2), (1, 1)]
    A = 9 * sum(h * w for h, w in levels)
    route = "%s K=%d C=%d Cs=%d A=%d" % (_dn(dtype), K, C, Cs, A)
    allbuf = torch.full((B, A, K), NAN).cuda()
    grad = rng_normal(K, B, A, K)
    gdev = grad.cuda()
    want = torch.empty(B, A, K)
    o = 0
    for li, (h, w) in enumerate(levels):
        n = h * w
        src = _rand(K * 10 + li, (B, h, w, Cs), dtype)
        sdev = src.cuda()
        ops.call("mpn_det_pack", ops.ptr(sdev), ops.dtype_code(dtype), ctypes.c_void_p(allbuf.data_ptr() + o * K * 4), B, n, Cs, C,
                 A * K, ops.stream_ptr())
        want[:, o:o + 9 * n] = src[..., :C].float().reshape(B, n * 9, K)
        d = torch.full((B, h, w, Cs), NAN, dtype=dtype).cuda()
        ops.call("mpn_det_unpack", ctypes.c_void_p(gdev.data_ptr() + o * K * 4), ops.ptr(d), ops.dtype_code(dtype), B, n, Cs, C, A * K,
                 ops.stream_ptr())
        torch.cuda.synchronize()
        wd = torch.zeros(B, h, w, Cs, dtype=dtype)
        wd[..., :C] = grad[:, o:o + 9 * n].reshape(B, h, w, C).to(dtype)                # round to nearest even, pad lanes 0
        _exact("det_unpack %s level %d" % (route, li), d.cpu().double(), wd.double(), route)
        o += 9 * n
    assert o == A
    _exact("det_pack %s five levels" % route, allbuf.cpu(), want, route)


@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
def test_relu_add_and_layout(dtype):
    ops = _ops()
    shape = (3, 11, 13, 96)                                           # 41 184 elements: the last block is partial
    route = "%s n=%d" % (_dn(dtype), 3 * 11 * 13 * 96)
    x, dz, a0 = _rand(1, shape, dtype), _rand(2, shape, dtype), _rand(3, shape, dtype)
    x.reshape(-1)[::7] = 0.0
    x.reshape(-1)[3::7] = -0.0
    with _NanAlloc():
        z = ops.relu_forward(_act(x, 96))
        dx = ops.relu_backward(_act(dz, 96), z)
    _exact("relu_forward " + route, z.t.cpu().double(), x.double().clamp(min=0), route)
    g = dz.double() * (x.double() > 0)
    _exact("relu_backward " + route, dx.t.cpu().double(), g, route)
    acc = ops.Act(a0.clone().cuda(), 96)
    ops.relu_backward(_act(dz, 96), z, acc, accumulate=True)
    _check("relu_backward accumulate " + route, acc.t, a0.double() + g, a0.double().abs() + g.abs(), dtype, route, "bhwc", **roundings(1))
    dst = ops.Act(a0.clone().cuda(), 96)
    ops.add_inplace(dst, _act(dz, 96))
    torch.cuda.synchronize()
    _check("add_inplace " + route, dst.t, a0.double() + dz.double(), a0.double().abs() + dz.double().abs(), dtype, route, "bhwc", **roundings(1))
    if dtype == F32:
        big = rng_normal(9, 3, 10, 12, 30).cuda()
        for name, t in (("strided slice", big[:, 1:8:2, 2:-1, ::3]), ("channels-last view", big.permute(0, 3, 1, 2)),
                        ("expanded batch", big[:1].expand(3, 10, 12, 30))):
            with _NanAlloc():
                out = ops.nchw_to_nhwc_f32(t)
            _exact("nchw_to_nhwc_f32 %s strides=%s" % (name, tuple(t.stride())), out.cpu(), t.cpu().permute(0, 2, 3, 1).contiguous(), route)
