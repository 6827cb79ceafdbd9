"""References, per-element bounds, input builders and modelled faults of the parameter path (csrc/weight_prep.hip: the f32 -> 16-bit
operand refresh, the transposed dgrad operands, the stem's packings, the Linear layers' K padding, the Adam update and its device-side
bias corrections, the fill), shared by tests/test_param_path_gpu.py (which compares the kernels with them) and
tests/test_param_path_cpu.py (which anchors the references and shows that they reject the faults).  Test-side only; numpy and plain
torch on the CPU.

Two groups.

BIT-EXACT: casts, transposes, packings, padding, fill, copy.  Each is a re-indexing plus at most one round-to-nearest-even conversion,
so the reference (`torch.Tensor.to(dtype)` on the CPU of the re-indexed f32 values) has one right answer per element; integer views are
compared, so -0.0 and pad zeros count.  `rne_bf16_bits` / `rne_f16_bits` restate the rounding on bit patterns (the CPU file anchors
torch's conversion to them) and carry the modelled faults (half-up, truncation).

BOUNDED: the Adam arithmetic.  The kernel reads float32 hyper-parameters; the reference widens exactly those to float64 — this is Adam
with the float32-rounded betas, self-consistent between the weights 1 - b and the corrections 1 - b^t (see `beta_rounding_distance`
for how far that is from the host doubles 0.9 / 0.999).  With u = 2^-24 and magnitudes = the same formula on absolute values:

    G = g gs + wd p                    Gm = |g gs| + |wd p|
    M = b1 m + (1 - b1) G              Mm = b1 |m| + (1 - b1) Gm          |m' - M| <=  6 u Mm
    V = b2 v + (1 - b2) G^2            Vm = b2 |v| + (1 - b2) Gm^2        |v' - V| <= 11 u Vm
    U = (lr / bc1) m' / (sqrt(v') / bc2s + eps)      from the DEVICE's m', v' (each stage referenced from the previous one)
    P = p - U                                                              |p' - P| <= u (|p| + |U|) + 9 u |U|

The constants count one u per fp32 operation of the kernel text.  m': g gs, wd p, their sum, 1 - b1, two products, the final sum; the
deepest path through them (g gs -> + -> (1 - b1) G with the rounded 1 - b1 -> +) carries 5 roundings relative to Mm, so 6 u also covers
the second-order terms.  v': 5 of its own (1 - b2, two products, b2 v, the sum) and the 3 of G twice because G enters squared: 11; the
deepest path carries 8.  p': the subtraction's rounding on |p| + |U|, and on |U| sqrt and the division by bc2s counted twice each (the
build does not pin their rounding to half a spacing), + eps (every term of the denominator is non-negative, so its roundings stay
relative), lr / bc1, m' / denom and the product: 9.  A fused multiply-add drops a rounding, it never adds one, so the bounds hold for the
uncontracted evaluation and for either contraction the compiler may choose (weight_prep.o is built without -ffp-contract=off).
Nothing is fitted to device output."""
import numpy as np
import torch


f32, f64 = np.float32, np.float64
BF, H16, F32 = torch.bfloat16, torch.float16, torch.float32
TYPES = (F32, BF, H16)
U = 2.0 ** -24
M_OPS, V_OPS, U_OPS = 6, 11, 9


def dn(dtype):
    return {BF: "bf16", H16: "f16", F32: "f32"}[dtype]


def round_up(v, m):
    return (v + m - 1) // m * m


def bits32(x):
    return np.ascontiguousarray(x, dtype=f32).view(np.uint32)


def from_bits(b):
    return np.asarray(b, dtype=np.uint32).view(f32)


def ibits(t):
    """Integer view of a torch tensor (bit comparison: -0.0 != +0.0, NaN payloads count)."""
    return t.contiguous().view({4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()])


# ------------------------------------------------------------------------------------------------ casts
def rne_bf16_bits(x, mode="rne"):
    """uint16 bfloat16 patterns of f32 `x` (no NaN).  mode: 'rne' | 'half_up' (ties away from zero in magnitude) | 'trunc'."""
    b = bits32(x).astype(np.uint64)
    if mode == "trunc":
        return (b >> 16).astype(np.uint16)
    if mode == "half_up":
        return ((b + 0x8000) >> 16).astype(np.uint16)
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)


def rne_f16_bits(x):
    """uint16 IEEE half patterns of f32 `x` (no NaN) by exact integer arithmetic: |x| = q 2^e with the target spacing 2^e."""
    b = bits32(x).astype(np.int64)
    sign = ((b >> 16) & 0x8000).astype(np.int64)
    mag = b & 0x7FFFFFFF
    inf = mag >= 0x7F800000
    E = (mag >> 23) - 127                                            # unbiased exponent of a normal f32
    sig = (mag & 0x7FFFFF) | 0x800000                               # 24-bit significand: |x| = sig 2^(E - 23)
    shift = np.where(E >= -14, 13, 13 + (-14 - E)).clip(max=40)     # bits dropped: spacing 2^(E - 10) normal, 2^-24 below 2^-14
    q = sig >> shift
    rem = sig & ((np.int64(1) << shift) - 1)
    half = np.int64(1) << (shift - 1)
    q = q + ((rem > half) | ((rem == half) & ((q & 1) == 1)))
    # normal: q in [2^10, 2^11] -> pattern (E + 15 - 1) << 10 + q (a carry into the exponent is the next binade or inf: the same sum)
    normal = ((E + 14) << 10) + q
    res = np.where(E >= -14, normal, q)                              # subnormal: pattern q (q = 2^10 is the smallest normal)
    res = np.where(mag == 0, 0, res)
    res = np.where(inf | (res >= 0x7C00), 0x7C00, res)
    return (res | sign).astype(np.uint16)


def cast_edge_values():
    """f32 values built from bit patterns: every rounding edge of both 16-bit types, no f32 subnormal, the NaN last."""
    pats = []

    def around(p):
        pats.extend([p - 1, p, p + 1, (p - 1) | 0x80000000, p | 0x80000000, (p + 1) | 0x80000000])
    for base in (0x3F800000, 0x40490000, 0x00800000, 0x7F000000, 0x2F000000):      # bf16 ties: low half 0x8000
        around(base | 0x8000)                       # lower neighbour even
        around(base | 0x18000)                      # lower neighbour odd
    for base in (0x3F800000, 0x40490000, 0x38800000, 0x477F8000):                  # f16 ties (normal range): low 13 bits 0x1000
        around(base | 0x1000)                       # lower neighbour even
        around(base | 0x3000)                       # lower neighbour odd
    pats += [0x00000000, 0x80000000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0xFF800000]
    for v in (65504.0, 65520.0, 65536.0):           # the f16 overflow boundary: 65520 is the tie between 65504 and 2^16 (-> inf)
        around(int(bits32(f32(v)).reshape(-1)[0]))
    around(0x33000000)                              # 2^-25: the tie between 0 and the smallest f16 subnormal
    around(0x33800000)                              # 2^-24
    around(0x33C00000)                              # 3 2^-25: tie between 2^-24 (odd) and 2^-23 (even)
    around(0x34200000)                              # 5 2^-25: tie between 2^-23 (even) and 3 2^-24 (odd)
    pats += list(range(0x33800000, 0x38800000, 0x00123457))                        # normal f32 across the f16-subnormal range
    pats += [p | 0x80000000 for p in range(0x33800123, 0x38800000, 0x00523457)]
    pats.append(0x7FC00000)
    v = from_bits(np.array(pats, dtype=np.uint64).astype(np.uint32))
    mag = bits32(v) & 0x7FFFFFFF
    assert not ((mag > 0) & (mag < 0x00800000)).any(), "f32 subnormal among the cast inputs"
    assert int(np.isnan(v).sum()) == 1
    return v


CAST_SIZES = (1, 7, 8, 9, 2047, 2048, 2049) + tuple(4096 + k for k in range(8))


def cast_input(n):
    """n values cycling through the edge set, rotated by n so that the scalar tail of each size sees different ones."""
    e = cast_edge_values()
    return e[(np.arange(n) + 3 * n) % len(e)].copy()


def cast_ref(x, dtype):
    """torch's own round-to-nearest-even conversion on the CPU."""
    return torch.from_numpy(np.ascontiguousarray(x, dtype=f32)).to(dtype)


def check_cast(name, got, x, dtype):
    """Bit-equal wherever the input is no NaN; NaN where it is."""
    got = got.cpu()
    want = cast_ref(x, dtype)
    nan = torch.from_numpy(np.isnan(x))
    assert got.shape == want.shape and got.dtype == dtype, (name, got.shape, got.dtype)
    assert bool(torch.isnan(want.float())[nan].all()) and bool(torch.isnan(got.float())[nan].all()), "%s: NaN not kept" % name
    gi, wi = ibits(got), ibits(want)
    bad = torch.nonzero((gi != wi) & ~nan)
    assert len(bad) == 0, "%s: %d elements differ, first at %d: input %r (0x%08x) -> 0x%04x, reference 0x%04x" % (
        name, len(bad), int(bad[0]), float(x[int(bad[0])]), int(bits32(x)[int(bad[0])]), int(gi[int(bad[0])]) & 0xFFFF,
        int(wi[int(bad[0])]) & 0xFFFF)


# ------------------------------------------------------------------------------------------------ re-indexings
TRANSPOSE_GEOMS = ((1, 1, 1, 32), (33, 9, 31, 64), (5, 49, 3, 32), (3, 1, 40, 96), (64, 9, 64, 64), (19, 1, 256, 32))   # O, RS, I, Cout_pad
PAD_K_SHAPES = ((5, 17, 32), (8, 100, 128), (3, 64, 64))                                                                # Cout, K, Kpad
STEM_COUTS = (1, 3, 64)
IMAGE_SHAPES = ((2, 7, 5), (1, 1, 1), (2, 32, 48))                                                                      # B, H, W


def weights(seed, n):
    """Distinct-looking f32 values of both signs whose 16-bit roundings are not all exact (a ramp would be)."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, generator=g) * 0.05


def transpose_ref(w, O, RS, I, opad, dtype, prev=None):
    """w f32 [O * RS * I] in [O][RS][I] order -> Wt [I][RS][opad]: columns O .. opad - 1 exactly +0.  prev: the modelled fault that
    leaves the destination's previous contents in the pad columns."""
    out = torch.zeros(I, RS, opad, dtype=F32) if prev is None else prev.float().reshape(I, RS, opad).clone()
    out[..., :O] = w.view(O, RS, I).permute(2, 1, 0)
    return out.to(dtype)


def wt_layout(geoms):
    """Region offsets (elements) as Engine._wt_plan places them, the table rows for one f32 source holding the layers back to back
    at 64-float alignment, the destination's total and the block count."""
    rows, soff, doff, blk = [], 0, 0, 0
    for O, RS, I, opad in geoms:
        gx, gy = (I + 31) // 32, (opad + 31) // 32
        rows.append([soff, doff, O, RS, I, opad, blk, gx])
        soff += round_up(O * RS * I, 64)
        doff += round_up(I * RS * opad, 64)
        blk += gx * gy * RS
    return rows, soff, doff, blk


def pad_k_ref(w, Cout, K, Kpad, dtype):
    return torch.nn.functional.pad(w.view(Cout, K), (0, Kpad - K)).to(dtype)


def stem_pack_weight_ref(w, Cout, dtype):
    """w f32 [Cout][7][7][3] -> packed [Cout][7][32]: slot s * 4 + c; c == 3 and s == 7 are +0."""
    wn = w.numpy().reshape(Cout, 7, 7, 3)
    out = np.zeros((Cout, 7, 8, 4), dtype=f32)
    out[:, :, :7, :3] = wn
    return torch.from_numpy(out.reshape(Cout, 7, 32)).to(dtype)


def stem_unpack_ref(dw, dp, Cout, mut=None):
    """dw f32 [Cout * 147] + the live slots of dp f32 [Cout][7][32], one fp32 rounding.  mut: 'assign'."""
    live = dp.numpy().reshape(Cout, 7, 8, 4)[:, :, :7, :3].reshape(-1)
    return torch.from_numpy(live.copy() if mut == "assign" else (dw.numpy() + live).astype(f32))


def stem_pack_image_ref(x, dtype, mut=None):
    """x f32 [B, 3, H, W] (any strides) -> [B][H + 6][W + 8][4]: 3 zero rows above and below, 3 zero columns left, 5 right, the fourth
    channel +0.  mut: 'next_pixel' (the fourth channel takes the next pixel's first)."""
    B, _, H, W = x.shape
    out = torch.zeros(B, H + 6, W + 8, 4, dtype=F32)
    out[:, 3:3 + H, 3:3 + W, :3] = x.permute(0, 2, 3, 1)
    if mut == "next_pixel":
        flat = out.reshape(-1)
        flat[3::4][:-1] = flat[4::4].clone()
    return out.to(dtype)


def image_views(B, H, W, seed):
    """The three source layouts of one case: NCHW contiguous, channels_last, and a strided view with an offset."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 3, H, W, generator=g)
    big = torch.randn(B, 3, H + 2, 2 * W, generator=g)
    return {"nchw": (x, lambda d: d), "channels_last": (x, lambda d: d.contiguous(memory_format=torch.channels_last)),
            "strided": (big, lambda d: d[:, :, 1:-1, ::2])}


# ------------------------------------------------------------------------------------------------ Adam
HYPER_N = 16
ADAM_SETTINGS = ((0.0, 1.0), (1e-2, 1.0), (0.0, 0.37), (3e-3, 2.5))       # (wd, gs)
ADAM_STEPS = (1, 2, 10, 1000)
ADAM_SIZES = (1, 3, 4, 5, 1023, 1024, 1025, 4099)
ADVANCE_STEPS = (1, 2, 3, 10, 100, 1000, 100000)
BETAS = ((0.9, 0.999), (0.8, 0.99))


def hyper_vector(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.0, gs=1.0, step=0):
    """The 16-float device vector: slots 0..5 hyper-parameters, 6..7 bias corrections (here a sentinel until adam_advance writes
    them), 8 the step count as int32 bits, 9..15 distinct sentinels."""
    h = np.zeros(HYPER_N, dtype=f32)
    h[:6] = [lr, b1, b2, eps, wd, gs]
    h[6:8] = [-7.0, -9.0]
    h[8:9].view(np.int32)[0] = step
    h[9:] = np.arange(9, HYPER_N, dtype=f32) * 1.25 + 100.0
    return h


def bias_corrections(b1f, b2f, t):
    """(bc1, bc2s) as float32 from the FLOAT32 betas widened to double: what adam_advance_kernel forms."""
    b1, b2 = f64(f32(b1f)), f64(f32(b2f))
    return f32(1.0 - b1 ** f64(t)), f32(np.sqrt(1.0 - b2 ** f64(t)))


def spacings_apart(a, b):
    """Distance of two positive float32 values in units of the float32 grid."""
    return abs(int(bits32(f32(a)).reshape(-1)[0]) - int(bits32(f32(b)).reshape(-1)[0]))


def beta_rounding_distance(b1=0.9, b2=0.999, tmax=100000):
    """Largest relative difference over t = 1 .. tmax between the float32 bias corrections from the float32 betas (the device) and
    from the Python doubles (torch.optim.Adam on the host): (for bc1, for bc2s, and the t at which each occurs)."""
    t = np.arange(1, tmax + 1, dtype=f64)
    dev1 = (1.0 - f64(f32(b1)) ** t).astype(f32).astype(f64)
    host1 = (1.0 - f64(b1) ** t).astype(f32).astype(f64)
    dev2 = np.sqrt(1.0 - f64(f32(b2)) ** t).astype(f32).astype(f64)
    host2 = np.sqrt(1.0 - f64(b2) ** t).astype(f32).astype(f64)
    r1, r2 = np.abs(dev1 - host1) / host1, np.abs(dev2 - host2) / host2
    return float(r1.max()), float(r2.max()), int(np.argmax(r1)) + 1, int(np.argmax(r2)) + 1


def adam_inputs(n, seed, moments):
    """(p, g, m, v) f32 numpy: |g| log-uniform over 1e-9 .. 1e3, |p| over 1e-4 .. 10 with exact zeros, moments zero or non-zero
    (v >= 0).  No f32 subnormal anywhere (g^2 (1 - b2) >= 1e-21)."""
    r = np.random.default_rng(seed)

    def logu(lo, hi, signed=True):
        x = 10.0 ** r.uniform(lo, hi, n)
        return (x * (r.choice([-1.0, 1.0], n) if signed else 1.0)).astype(f32)
    g = logu(-9, 3)
    p = logu(-4, 1)
    p[r.integers(0, 5, n) == 0] = 0.0
    if moments:
        m, v = logu(-9, 2), logu(-16, 4, signed=False)
    else:
        m, v = np.zeros(n, f32), np.zeros(n, f32)
    return p, g, m, v


def _fma(a, b, c):
    return (a.astype(f64) * b.astype(f64) + c.astype(f64)).astype(f32)       # the product of two f32 is exact in f64


def adam_model32(p, g, m, v, h, contract=0, mut=None):
    """The kernel text in numpy float32.  contract: 0 none, 1 / 2 the two ways a compiler may fuse each a*b + c*d (fma(a, b, c d) or
    fma(c, d, a b)).  h: float32 hyper vector with bc1 / bc2s in slots 6, 7.  mut: a modelled fault.  -> (p', m', v')."""
    lr, b1, b2, eps, wd, gs, bc1, bc2s = (f32(x) for x in h[:8])
    one = f32(1.0)
    p, g, m, v = (np.asarray(x, dtype=f32) for x in (p, g, m, v))
    if mut == "wd_before_scale":
        G = (g + wd * p) * gs
    elif wd == 0 or mut == "decoupled":
        G = g * gs
    elif contract == 1:
        G = _fma(np.broadcast_to(wd, p.shape), p, g * gs)
    elif contract == 2:
        G = _fma(g, np.broadcast_to(gs, g.shape), wd * p)
    else:
        G = g * gs + wd * p
    w1, w2 = one - b1, one - b2
    B1, B2, W1 = (np.broadcast_to(x, p.shape) for x in (b1, b2, w1))
    if mut == "w1_on_m":
        mk = w1 * m + b1 * G
    elif contract == 1:
        mk = _fma(B1, m, w1 * G)
    elif contract == 2:
        mk = _fma(W1, G, b1 * m)
    else:
        mk = b1 * m + w1 * G
    sq = (w2 * G) if mut == "v_with_G" else (w2 * G) * G
    if contract == 1:
        vk = _fma(B2, v, sq)
    elif contract == 2 and mut != "v_with_G":
        vk = _fma(w2 * G, G, b2 * v)
    else:
        vk = b2 * v + sq
    if mut == "eps_in_sqrt":
        denom = np.sqrt(vk + eps) / bc2s
    elif mut == "bc2_multiplied":
        denom = np.sqrt(vk) * bc2s + eps
    else:
        denom = np.sqrt(vk) / bc2s + eps
    step = lr if mut == "no_bc1" else lr / bc1
    q = mk / denom
    pk = _fma(np.broadcast_to(-step, q.shape), q, p) if contract else p - step * q
    if mut == "decoupled" and wd != 0:
        pk = pk - lr * wd * p
    return pk.astype(f32), mk.astype(f32), vk.astype(f32)


def adam_refs(p, g, m, v, h):
    """Float64 M, V and their magnitudes from the float32 inputs and the float32 hyper vector (widened)."""
    lr, b1, b2, eps, wd, gs = (f64(f32(x)) for x in h[:6])
    p, g, m, v = (np.asarray(x, dtype=f32).astype(f64) for x in (p, g, m, v))
    G, Gm = g * gs + wd * p, np.abs(g * gs) + np.abs(wd * p)
    M, Mm = b1 * m + (1 - b1) * G, b1 * np.abs(m) + (1 - b1) * Gm
    V, Vm = b2 * v + (1 - b2) * G * G, b2 * np.abs(v) + (1 - b2) * Gm * Gm
    return M, Mm, V, Vm


def adam_p_ref(p, m_dev, v_dev, h):
    """P = p - U from the device's own m', v' and the bias corrections it holds; -> (P, |p| + |U|, |U|)."""
    lr, eps, bc1, bc2s = (f64(f32(h[i])) for i in (0, 3, 6, 7))
    p, md, vd = (np.asarray(x, dtype=f32).astype(f64) for x in (p, m_dev, v_dev))
    Uv = (lr / bc1) * md / (np.sqrt(vd) / bc2s + eps)
    return p - Uv, np.abs(p) + np.abs(Uv), np.abs(Uv)


def check_bounded(name, got, ref, mag, ops):
    """|got - ref| <= ops u mag at EVERY element (numpy; got f32, ref / mag f64).  -> (worst err / bound, its index).  A zero bound
    demands equality; NaN is a violation."""
    got = np.asarray(got, dtype=f32).astype(f64)
    err = np.abs(got - ref)
    bound = ops * U * mag
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    ratio = np.where(np.isnan(ratio), np.inf, ratio)
    w = int(np.argmax(ratio))
    bad = ~(err <= bound)
    if bad.any():
        f = int(np.nonzero(bad)[0][0])
        raise AssertionError("%s: element %d got %r, float64 reference %r, |err| %.3e > bound %.3e (worst err/bound %.3f at %d)" % (
            name, f, float(got[f]), float(ref[f]), float(err[f]), float(bound[f]), float(ratio[w]), w))
    return float(ratio[w]), w


def check_adam(tag, got, p, g, m, v, h):
    """got = (p', m', v') as numpy f32; every element against the bounds of the module docstring.
    -> [(worst err / bound, index)] for m', v', p'.  Raises AssertionError on the first violation."""
    gp, gm, gv = (np.asarray(x, dtype=f32) for x in got)
    M, Mm, V, Vm = adam_refs(p, g, m, v, h)
    P, PUm, Um = adam_p_ref(p, gm, gv, h)
    return [check_bounded(tag + " m'", gm, M, Mm, M_OPS), check_bounded(tag + " v'", gv, V, Vm, V_OPS),
            check_bounded(tag + " p'", gp, P, PUm + U_OPS * Um, 1)]


def check_adam_slice(tag, before, after, s, e, h, g_inside=None):
    """before / after: dicts p, g, m, v of whole f32 numpy buffers around one update of [s, e).  Outside the slice every buffer is
    bit-unchanged; the gradient inside is bit-equal to g_inside (default: unchanged); inside, check_adam."""
    for k in "pgmv":
        b, a = bits32(before[k]), bits32(after[k])
        assert a.shape == b.shape
        out = np.ones(b.shape, dtype=bool)
        out[s:e] = False
        bad = np.nonzero((a != b) & out)[0]
        assert len(bad) == 0, "%s: %s changed outside [%d, %d) at %d" % (tag, k, s, e, int(bad[0]))
    gi = before["g"][s:e] if g_inside is None else g_inside
    assert np.array_equal(bits32(after["g"][s:e]), bits32(gi)), "%s: gradient inside the slice is not what it should be" % tag
    return check_adam(tag, (after["p"][s:e], after["m"][s:e], after["v"][s:e]), before["p"][s:e], gi, before["m"][s:e], before["v"][s:e], h)


class Worst(object):
    """Collects the worst err / bound of m', v', p' over the sub-cases of one test, with where it occurred."""

    def __init__(self):
        self.w = {k: (-1.0, "") for k in ("m'", "v'", "p'")}

    def add(self, res, where, base=0):
        for k, (r, i) in zip(("m'", "v'", "p'"), res):
            if r > self.w[k][0]:
                self.w[k] = (r, "%s i=%d" % (where, base + i))

    def lines(self, tag):
        out = []
        for k in ("m'", "v'", "p'"):
            r, where = self.w[k]
            out.append("%-58s %-4s worst err/bound=%.3f at %s  %s%s" % (tag, k, r, where, "OK" if r <= 1 else "FAIL",
                                                                     "  (above 0.8)" if r > 0.8 else ""))
        return out


ADAM_FAULTS = ("eps_in_sqrt", "bc2_multiplied", "no_bc1", "wd_before_scale", "decoupled", "w1_on_m", "v_with_G")
