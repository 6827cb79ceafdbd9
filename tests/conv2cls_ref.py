"""Float64 references, per-element bounds, case tables and modelled faults of the conv2 position-class kernels (csrc/conv2cls.hip),
shared by tests/test_conv2cls_parity_gpu.py (which compares the kernels with them) and tests/test_conv2cls_parity_cpu.py (which anchors
the references to the plain operation and shows that the bounds accept fp32 models of the kernels and reject the faults).  Test-side
only; plain torch on the CPU.

Everything here comes from the DEFINITION, not from the kernels' lookup tables: tap r of output row s i + a reads up-sampled row
s i + a + r - 1, which lies in low-resolution row floor((s i + a + r - 1) / s); the frame index u is that row minus i, plus 1
(`frame_of`); the class of a is first (0) if a == 0, last (2) if a == s - 1, else mid (1) (`cls_of`).  `frame_table` asserts that every
offset of a class has the same frames, for s = 8 and s = 4 alike.

Every sum is described as a list of TERMS (tensors of the output's shape, zero where the term is absent, and the mask of where it is
present); `reduce_terms` gives the float64 sum, the magnitude sum |t|, the number n of terms present per element and the sequential
fp32 sum in the order asked for.  Bounds (u = 2^-24, helpers.check_elementwise through `check_sum`; nothing fitted):
    any fp32 summation of n terms, in any order or tree:   (n - 1) u sum |t|     (n - 1 additions, each off by at most u |partial|)
    + half a spacing of the output type where the result is stored in 16 bits
    elements with n <= 1 (combine, f32 expand: n <= 2, one correctly rounded add) must be bit-equal to the fp32 value
The chain dy -> pool -> tapsum adds, as extra_abs, half a spacing of every stored P term that enters the element.

Storage contract of the backward (`pool_store`, `g_scale`; csrc/conv2cls.hip): bf16 / f32 store P and G in the compute type; fp16 stores P
in f32 and G as G / s^2, and both consumers of G (the 1x1 input-gradient launch, fold) multiply by s^2 in f32 behind their contraction.

The last section is conv2's WHOLE backward (`bwd_case`): a float64 reference per member from the definition — autograd of
conv2d(cat(up8(q5), up4(q4), up2(q3), q2), W, pad 1) — on input sets that span the fp16 range, the structural per-element bound of the
class route and of the plain route (`bwd_specs`), and fp32 models of both routes and of the faults the bound must reject (`class_model`)."""
import functools
import math

import torch
import torch.nn.functional as F

from helpers import check_elementwise, report, rng_normal, ulp_out
from stream_ref import exact, roundings

BF, H16, F32 = torch.bfloat16, torch.float16, torch.float32
F64 = torch.float64
TYPES = (BF, H16, F32)


def dn(dtype):
    return {BF: "bf16", H16: "f16", F32: "f32"}[dtype]


# ------------------------------------------------------------------------------------------------ the definition
def cls_of(a, s):
    return 0 if a == 0 else (2 if a == s - 1 else 1)


def frame_of(a, r, s):
    return (a + r - 1) // s + 1                      # floor division: a + r - 1 = -1 -> row i - 1 -> frame 0


def frame_table(s):
    """FR[class][r] = frame index of original tap r, the same for every offset of the class."""
    tab = {}
    for a in range(s):
        row = tuple(frame_of(a, r, s) for r in range(3))
        assert tab.setdefault(cls_of(a, s), row) == row, (s, a)
    return tuple(tab[k] for k in range(3))


FR = frame_table(8)
FR_FIRST_TAKES_01 = ((0, 0, 1),) + FR[1:]            # the fault "first collects taps {0, 1} in frame 0"


def cls_vec(n, s, last_at=None):
    """class of every coordinate 0 .. n - 1 of an image of s-pixel blocks (last_at: the modelled fault's offset of `last`)."""
    la = s - 1 if last_at is None else last_at
    a = torch.arange(n) % s
    return torch.where(a == 0, 0, torch.where(a == la, 2, 1))


def lowres_src(n, a, r, s):
    """For low-resolution rows i = 0 .. n - 1: the low-resolution row that tap r of output row s i + a reads, and whether it is inside."""
    idx = torch.div(s * torch.arange(n) + a + r - 1, s, rounding_mode="floor")
    return idx, (idx >= 0) & (idx < n)


REP = (0, 1, 3)                                      # one offset of each class at s = 4 (frame_table: every other one agrees)


# ------------------------------------------------------------------------------------------------ sums of terms
class Sum(object):
    __slots__ = ("ref", "mag", "n", "f32")


def reduce_terms(terms, order=None):
    """terms: thunks -> (float64 values, bool presence).  order: indices (default 0 .. len - 1) of the sequential fp32 sum."""
    S = Sum()
    S.ref = None
    for k in (range(len(terms)) if order is None else order):
        v, on = terms[k]()
        if S.ref is None:
            S.ref, S.mag, S.n, S.f32 = torch.zeros_like(v), torch.zeros_like(v), torch.zeros(v.shape, dtype=torch.int32), torch.zeros(v.shape, dtype=F32)
        S.ref += v
        S.mag += v.abs()
        S.n += on
        S.f32 = S.f32 + v.float()                    # every term is an fp32 (or narrower) value: the cast is exact
    return S


def bound_of(S, out_dtype, got=None):
    """The bound check_sum applies (for the generator conditions)."""
    v = S.ref.abs() if got is None else torch.maximum(S.ref.abs(), got.double().abs())
    return 0.5 * ulp_out(v, out_dtype) + (S.n - 1).clamp(min=0).double() * 2.0 ** -24 * S.mag


def check_sum(name, got, S, out_dtype, route="", names="bhwko", exact_n=1, extra_abs=None):
    """got against a Sum: (n - 1) roundings on sum |t| (+ half an output spacing, + extra_abs); where n <= exact_n bit-equal to the fp32
    value stored in out_dtype.  One report line each."""
    got = got.detach().cpu()
    assert got.shape == S.ref.shape, (name, got.shape, S.ref.shape)
    w = check_elementwise(name, got, S.ref, S.mag * (S.n - 1).clamp(min=0).double(), out_dtype, route=route, names=names,
                          extra_abs=extra_abs, **roundings(1))
    m = S.n <= exact_n
    if exact_n >= 0 and bool(m.any()):
        want = S.f32.to(out_dtype)
        ok = torch.equal(got[m], want[m])
        report("%-58s %-52s %d elements of <= %d terms exact  %s" % (name, route, int(m.sum()), exact_n, "OK" if ok else "FAIL"))
        if not ok:
            bad = torch.nonzero(m & ~(got == want))[0].tolist()
            raise AssertionError("%s: element %s of %d term(s) is %r, not the fp32 value %r" % (
                name, bad, int(S.n[tuple(bad)]), float(got[tuple(bad)]), float(want[tuple(bad)])))
    return w


# ------------------------------------------------------------------------------------------------ combine
def comb_sizes(O, C):
    """(nm, nc, nt): elements of Wm [O][3][3][2C], of one frame-filter set [9 O][3][3][C], of one per-tap set [9 O][C]."""
    return O * 9 * 2 * C, 9 * O * 9 * C, 9 * O * C


def frame_terms(w, m, fr_rows=FR, fr_cols=FR):
    """Frame filters [9 (class)][O][3 (u)][3 (v)][C] of member m of w [O][3][3][4 C]: one term per original tap (r, s), landing in frame
    (FR[ca][r], FR[cc][s]) of every class (ca, cc)."""
    O, C = w.shape[0], w.shape[3] // 4
    wm = w[..., m * C: (m + 1) * C].double()

    def term(r, s):
        def f():
            v, on = torch.zeros(9, O, 3, 3, C, dtype=F64), torch.zeros(9, 1, 3, 3, 1, dtype=torch.bool)
            for k in range(9):
                u, vv = fr_rows[k // 3][r], fr_cols[k % 3][s]
                v[k, :, u, vv] = wm[:, r, s]
                on[k, 0, u, vv, 0] = True
            return v, on.expand_as(v)
        return f
    return [term(r, s) for r in range(3) for s in range(3)]


def combine_parts(w, mut=None, order=None):
    """w f32 [O][3][3][4 C] (members q5, q4, q3, q2 along the input channels) -> dict wm (f32 [O][3][3][2C]), wc (two Sums), wtap (two
    f32 [9][O][C]: row t * O + o is tap t of output channel o).  mut: 'first01' | 'members' | 'tap_rows'."""
    O, C = w.shape[0], w.shape[3] // 4
    mem = (1, 0) if mut == "members" else (0, 1)
    fr_rows = FR_FIRST_TAKES_01 if mut == "first01" else FR
    wt = []
    for m in mem:
        t = w[..., m * C: (m + 1) * C].reshape(O, 9, C)
        wt.append(t.reshape(9, O, C) if mut == "tap_rows" else t.permute(1, 0, 2).contiguous())
    return dict(wm=w[..., 2 * C:].contiguous(), wc=[reduce_terms(frame_terms(w, m, fr_rows), order) for m in mem], wtap=wt)


def comb_flat(parts, model=False):
    """The comb vector a combine with these parts would write (frame filters: the float64 sum rounded once, or the sequential fp32 one)."""
    wc = [(S.f32 if model else S.ref.float()).reshape(-1) for S in parts["wc"]]
    return torch.cat([parts["wm"].reshape(-1)] + wc + [t.reshape(-1) for t in parts["wtap"]])


def check_combine(tag, comb, w, route=""):
    O, C = w.shape[0], w.shape[3] // 4
    nm, nc, nt = comb_sizes(O, C)
    comb = comb.detach().cpu()
    assert comb.numel() == nm + 2 * nc + 2 * nt, (tag, comb.numel())
    P = combine_parts(w)
    exact(tag + " Wm", comb[:nm], P["wm"].reshape(-1), route)
    worst = 0.0
    for m in range(2):
        worst = max(worst, check_sum("%s Wc%d" % (tag, 8 >> m), comb[nm + m * nc: nm + (m + 1) * nc].reshape(9, O, 3, 3, C), P["wc"][m], F32,
                                     route, "kouvc", exact_n=2))
        exact("%s Wtap%d" % (tag, 8 >> m), comb[nm + 2 * nc + m * nt: nm + 2 * nc + (m + 1) * nt], P["wtap"][m].reshape(-1), route)
    return worst


# ------------------------------------------------------------------------------------------------ expand
def expand_terms(m8, m4, H, W, mut=None):
    """m8 [B, H/8, W/8, 9, O], m4 [B, H/4, W/4, 9, O] -> the two terms of E [B, H, W, O].  mut: 'transposed' | 'last_s2' | 'm8_shift2'."""
    y, x = torch.arange(H), torch.arange(W)

    def member(m, s, shift):
        la = s - 2 if mut == "last_s2" else None
        ky, kx = cls_vec(H, s, la)[:, None], cls_vec(W, s, la)[None, :]
        k = kx * 3 + ky if mut == "transposed" else ky * 3 + kx
        sh = 2 if (mut == "m8_shift2" and s == 8) else shift
        B, h, w_, _, O = m.shape
        flat = (((y >> sh)[:, None] * w_ + (x >> sh)[None, :]) * 9 + k) % (h * w_ * 9)     # (the fault's overrun wraps inside the image)
        return lambda: (m.double().reshape(B, h * w_ * 9, O)[:, flat], torch.ones(B, H, W, O, dtype=torch.bool))
    return [member(m8, 8, 3), member(m4, 4, 2)]


# ------------------------------------------------------------------------------------------------ classsum
def classsum_terms(t, mut=None):
    """t [B, h, w, 9 (tap), O] per-tap products -> terms of M [B, h, w, 9 (class), O]: class (ca, cc) at (i, j) is the output at an
    up-sampled pixel of that class, whose tap (r, s) reads the low-resolution pixel lowres_src gives; zero outside.
    mut: 'clamp' | 'uv'."""
    B, h, w, _, O = t.shape
    t = t.double()

    def term(r, s):
        def f():
            v, on = torch.zeros(B, h, w, 9, O, dtype=F64), torch.zeros(1, h, w, 9, 1, dtype=torch.bool)
            for k in range(9):
                ca, cc = k // 3, k % 3
                if mut == "uv":          # the row displacement taken from the column's frame and the other way round
                    ii, vi = lowres_src(h, REP[cc], s, 4)
                    jj, vj = lowres_src(w, REP[ca], r, 4)
                else:
                    ii, vi = lowres_src(h, REP[ca], r, 4)
                    jj, vj = lowres_src(w, REP[cc], s, 4)
                if mut == "clamp":
                    vi, vj = vi | True, vj | True
                ok = vi[:, None] & vj[None, :]
                src = t[:, ii.clamp(0, h - 1)][:, :, jj.clamp(0, w - 1)][:, :, :, r * 3 + s]
                v[:, :, :, k] = src * ok[None, :, :, None]
                on[0, :, :, k, 0] = ok
            return v, on.expand_as(v)
        return f
    return [term(r, s) for r in range(3) for s in range(3)]


# ------------------------------------------------------------------------------------------------ pool
def pool_terms(dy, s):
    """dy [B, H, W, O] -> terms of P_s [B, H/s, W/s, 9, O]: one per offset (a, c) of the block, in its class's plane."""
    B, H, W, O = dy.shape
    dy = dy.double()

    def term(a, c):
        def f():
            v, on = torch.zeros(B, H // s, W // s, 9, O, dtype=F64), torch.zeros(1, 1, 1, 9, 1, dtype=torch.bool)
            k = cls_of(a, s) * 3 + cls_of(c, s)
            v[:, :, :, k] = dy[:, a::s, c::s]
            on[..., k, 0] = True
            return v, on.expand_as(v)
        return f
    return [term(a, c) for a in range(s) for c in range(s)]


def pool_threads(B, H, W, O):
    return B * (H // 8) * (W // 8) * (O // 4) * 4


def pool_tree(dy, dtype=F32, mut=None):
    """Model of conv2cls_pool_kernel's summation: per 4 x 4 quadrant nine sequential class sums (= P4), then per 8 x 8 class the
    quadrant's own classes selected by (rsel, csel), then lanes ^ 1 and ^ 2.  mut: 'mid_rows' (P8 mid misses rows 4..6) | 'swap'
    (quadrants qa / qc swapped when loading) | 'one_step' (the ^ 2 step missing).  -> (p8, p4) in `dtype`."""
    B, H, W, O = dy.shape
    q = dy.to(dtype).reshape(B, H // 4, 4, W // 4, 4, O)
    c4 = (0, 1, 1, 2)
    s4 = [torch.zeros(B, H // 4, W // 4, O, dtype=dtype) for _ in range(9)]
    for a in range(4):
        for c in range(4):
            k = c4[a] * 3 + c4[c]
            s4[k] = s4[k] + q[:, :, a, :, c]
    p4 = torch.stack(s4, 3)
    quad = p4.reshape(B, H // 8, 2, W // 8, 2, 9, O)

    def sel(R, qd, rows):       # quadrant classes (first, mid, last) that belong to block class R
        if R == 0:
            return (qd == 0, False, False)
        if R == 2:
            return (False, False, qd == 1)
        if qd == 0:
            return (False, True, True)
        return (False, False, False) if (rows and mut == "mid_rows") else (True, True, False)
    planes = []
    for R in range(3):
        for Cc in range(3):
            part = {}
            for qa in range(2):
                for qc in range(2):
                    src = quad[:, :, qc, :, qa] if mut == "swap" else quad[:, :, qa, :, qc]
                    rs, cs = sel(R, qa, True), sel(Cc, qc, False)
                    acc = torch.zeros(B, H // 8, W // 8, O, dtype=dtype)
                    for ra in range(3):
                        for rc in range(3):
                            if rs[ra] and cs[rc]:
                                acc = acc + src[:, :, :, ra * 3 + rc]
                    part[qa, qc] = acc
            lane0 = part[0, 0] + part[0, 1]
            planes.append(lane0 if mut == "one_step" else lane0 + (part[1, 0] + part[1, 1]))
    return torch.stack(planes, 3), p4


# ------------------------------------------------------------------------------------------------ tapsum
TAP_ORDER = ((1, 2, 0), (0, 1, 2), (2, 0, 1))        # the classes in the order the kernel's comment lists them per tap: M L F | F M L | L F M


def tapsum_terms(P, mut=None):
    """P [B, h, w, 9 (class), O] -> terms of G [B, h, w, 9 (tap), O]: the pixels of row class ca of block i' read, through tap r, the
    low-resolution row i' + FR[ca][r] - 1; G[i] collects the blocks for which that is i (inside the image only).  Term (a, c) takes the
    a-th / c-th class of TAP_ORDER per axis.  mut: 'r02' | 'wrap' | 'drop'."""
    B, h, w, _, O = P.shape
    P = P.double()

    def axis(n, cl, r):
        i = torch.arange(n) - FR[cl][2 - r if mut == "r02" else r] + 1
        return (i % n, torch.ones(n, dtype=torch.bool)) if mut == "wrap" else (i.clamp(0, n - 1), (i >= 0) & (i < n))

    def term(a, c):
        def f():
            v, on = torch.zeros(B, h, w, 9, O, dtype=F64), torch.zeros(1, h, w, 9, 1, dtype=torch.bool)
            for t in range(9):
                r, s = t // 3, t % 3
                ca, cc = TAP_ORDER[r][a], TAP_ORDER[s][c]
                if mut == "drop" and ca == 0:
                    continue
                ii, vi = axis(h, ca, r)
                jj, vj = axis(w, cc, s)
                ok = vi[:, None] & vj[None, :]
                v[:, :, :, t] = P[:, ii][:, :, jj][:, :, :, ca * 3 + cc] * ok[None, :, :, None]
                on[0, :, :, t, 0] = ok
            return v, on.expand_as(v)
        return f
    return [term(a, c) for a in range(3) for c in range(3)]


def tap_direct(dy, s):
    """G_s straight from dy [B, H, W, O] in float64: per tap (r, s') the sum of dy over the output pixels (y, x) whose up-sampled source
    (y + r - 1, x + s' - 1) is inside the image and lies in the low-resolution pixel.  -> Sum (f32 unused)."""
    B, H, W, O = dy.shape
    h, w = H // s, W // s

    def fold_axis(t, dim, n, r):
        pos = torch.arange(n) + r - 1
        ok = (pos >= 0) & (pos < n)
        shape = list(t.shape)
        shape[dim] = n // s
        return torch.zeros(shape, dtype=F64).index_add_(dim, pos[ok] // s, t.index_select(dim, torch.nonzero(ok).reshape(-1)))
    S = Sum()
    out = []
    for src in (dy.double(), dy.double().abs(), torch.ones(dy.shape, dtype=F64)):
        out.append(torch.stack([fold_axis(fold_axis(src, 1, H, t // 3), 2, W, t % 3) for t in range(9)], 3))
    S.ref, S.mag, S.n, S.f32 = out[0], out[1], out[2].round().to(torch.int32), None
    return S


def pool_store(dtype):
    """The type P is stored in: f32 for an fp16 backward (36 fp16 values of one sign pass 65504 from |dy| ~ 1820), else the type itself."""
    return F32 if dtype == H16 else dtype


def g_scale(dtype, s):
    """The factor G_s is stored with: 1 / s^2 in fp16 (G_s sums up to s^2 dy: the mean is never above max |dy|), else 1."""
    return 1.0 / (s * s) if dtype == H16 else 1.0


def scaled(S, k):
    """The Sum of k * terms, k a power of two (every part scales exactly)."""
    T = Sum()
    T.ref, T.mag, T.n, T.f32 = S.ref * k, S.mag * k, S.n, None if S.f32 is None else S.f32 * k
    return T


def chain_extra(P_stored, dtype):
    """Half a spacing of every stored P term that enters an element of G (the intermediate rounding of the chain)."""
    return reduce_terms(tapsum_terms(0.5 * ulp_out(P_stored.double(), dtype))).ref


# ------------------------------------------------------------------------------------------------ fold
def fold_scale(dtype):
    """What fold multiplies the two per-tap slices of dcomb by: 1 / g_scale (the launches that made them contracted G * g_scale)."""
    return (1.0 / g_scale(dtype, 8), 1.0 / g_scale(dtype, 4))


def fold_ref(dcomb, dw0, O, C, mut=None, scale=(1.0, 1.0)):
    """dw0 [O][9][4 C] + g in fp32 (one correctly rounded add), g from dcomb = dWm [O][9][2C] | dWtap8 [9][O][C] | dWtap4 [9][O][C]: the
    gradient of row t * O + o of a per-tap set belongs to tap t of output channel o, times scale[member] (a power of two: exact in
    fp32).  mut: 'tap_rows' | 'members' | 'assign'."""
    nm, _, nt = comb_sizes(O, C)
    g = torch.empty(O, 9, 4 * C, dtype=F32)
    g[..., 2 * C:] = dcomb[:nm].reshape(O, 9, 2 * C)
    for m in range(2):
        src = dcomb[nm + m * nt: nm + (m + 1) * nt] * scale[m]
        dst = (1 - m) if mut == "members" else m
        g[..., dst * C: (dst + 1) * C] = src.reshape(O, 9, C) if mut == "tap_rows" else src.reshape(9, O, C).permute(1, 0, 2)
    return g if mut == "assign" else dw0.reshape(O, 9, 4 * C) + g


def fold_inputs(O, C):
    """dcomb with every (o, t, c) distinct (a ramp of distinct fp32 integers below 2^24, shuffled signs) and a non-zero dw0."""
    nm, _, nt = comb_sizes(O, C)
    n = nm + 2 * nt
    dcomb = (torch.arange(1, n + 1, dtype=F32)) * torch.where(torch.arange(n) % 3 == 0, -1.0, 1.0)
    assert n < 2 ** 24 and dcomb.abs().unique().numel() == n
    dw0 = rng_normal(7000 + O + C, O * 9 * 4 * C) * 100.0 + 0.5
    return dcomb, dw0


# ------------------------------------------------------------------------------------------------ operands (host slicing)
def operands_ref(comb32, O, C, dtype):
    """What ops.Conv2ClsOperands must hold, from the device's comb32: the RNE copy and its slices, and the transposes by definition."""
    nm, nc, nt = comb_sizes(O, C)
    comb = comb32.to(dtype)
    wtap = [comb[nm + 2 * nc + m * nt: nm + 2 * nc + (m + 1) * nt] for m in range(2)]
    return dict(comb=comb, wm=comb[:nm], wc=[comb[nm + m * nc: nm + (m + 1) * nc] for m in range(2)], wtap=wtap,
                wm_t=comb[:nm].reshape(O, 9, 2 * C).permute(2, 1, 0).reshape(2 * C, 3, 3, O).contiguous(),
                wtap_t=[t.reshape(9 * O, C).t().reshape(C, 1, 1, 9 * O).contiguous() for t in wtap])


# ------------------------------------------------------------------------------------------------ inputs and case tables
def qnormal(seed, dtype, *shape):
    """Unit normals quantised through the storage type (f32 tensor holding exactly the values the kernel reads)."""
    return rng_normal(seed, *shape).to(dtype).float()


COMBINE_CASES = {          # (O, C)
    "8x4": ((8, 4), "the smallest"),
    "5x3": ((5, 3), "odd sizes (a wrong % or / shows), total no multiple of 256"),
    "256x128": ((256, 128), "the product's own size (6.5 M floats)"),
}
EXPAND_CASES = {           # (B, H, W, O)
    "1x8x8x8": ((1, 8, 8, 8), "one x8 block: every class on an image border"),
    "2x8x24x8": ((2, 8, 24, 8), "non-square, three blocks in a row, two images"),
    "1x16x8x24": ((1, 16, 8, 24), "og = 6, two blocks in a column"),
}
POOL_CASES = dict(EXPAND_CASES)
POOL_CASES["2x16x24x24"] = ((2, 16, 24, 24), "288 threads: two workgroups, the second with 32 live and 224 dead lanes")
POOL_THREADS = {"1x8x8x8": 8, "2x8x24x8": 48, "1x16x8x24": 48, "2x16x24x24": 288}
LOW_CASES = {              # (B, h, w, O) at low resolution
    "1x1x1x8": ((1, 1, 1, 8), "every neighbour outside"),
    "2x1x3x8": ((2, 1, 3, 8), "h = 1: no row neighbour; left, inner and right column"),
    "1x3x1x8": ((1, 3, 1, 8), "w = 1: no column neighbour"),
    "2x2x5x24": ((2, 2, 5, 24), "non-power-of-two, og = 6, 540 threads (three workgroups, the last ragged)"),
    "1x3x3x8": ((1, 3, 3, 8), "the smallest with an interior pixel"),
}
CLASSSUM_CASES = dict(LOW_CASES)
CLASSSUM_CASES["1x3x3x4"] = ((1, 3, 3, 4), "O = 4: one channel group (the entry point accepts O % 4)")
CLASSSUM_CASES["2x2x5x12"] = ((2, 2, 5, 12), "O = 12: og = 3")
CHAIN_CASES = {
    "2x8x24x8": ((2, 8, 24, 8), "one block row: P8 has no row neighbour, P4 has"),
    "1x16x16x8": ((1, 16, 16, 8), "2 x 2 blocks of 8: every P8 neighbour once"),
}


def case_seed(kind, name):
    return 1000 * (1 + ["combine", "expand", "classsum", "pool", "tapsum", "fold", "chain"].index(kind)) + sum(ord(c) for c in name)


def combine_input(name):
    O, C = COMBINE_CASES[name][0]
    return rng_normal(case_seed("combine", name), O, 3, 3, 4 * C)


def expand_input(name):
    B, H, W, O = EXPAND_CASES[name][0]
    s = case_seed("expand", name)
    return rng_normal(s, B, H // 8, W // 8, 9, O), rng_normal(s + 1, B, H // 4, W // 4, 9, O)


def low_input(kind, name, dtype):
    B, h, w, O = (CLASSSUM_CASES if kind == "classsum" else LOW_CASES)[name][0]
    return qnormal(case_seed(kind, name), dtype, B, h, w, 9, O)


def pool_input(kind, name, dtype):
    B, H, W, O = (POOL_CASES if kind == "pool" else CHAIN_CASES)[name][0]
    return qnormal(case_seed(kind, name), dtype, B, H, W, O)


# ------------------------------------------------------------------------------------------------ generator condition
def assert_decided(tag, S, alt64, out_dtype, plane=-2):
    """A pass is never luck: where the value another class or neighbour would give (alt64) differs from the reference at all, it
    differs by more than twice the bound — at EVERY such element of an f32 result; for 16-bit results (whose spacing 2^-8 |v| makes
    near-coincidences among thousands of unit normals certain) in every plane of dim `plane` that the alternative touches."""
    plane = plane % S.ref.dim()
    d = (S.ref - alt64).abs()
    far = d > 2 * bound_of(S, out_dtype)
    touched = d > 0
    if out_dtype == F32:
        assert bool((far | ~touched).all()), "%s: %d elements within the bound of the alternative" % (tag, int((touched & ~far).sum()))
    else:
        dims = [i for i in range(d.dim()) if i != plane]
        assert bool((far.sum(dims) > 0)[touched.sum(dims) > 0].all()), "%s: a plane the alternative touches has no decided element" % tag
    return int(touched.sum()), int((touched & ~far).sum())


# ================================================================================================ conv2's backward as a whole
O2, C2 = 256, 128                                    # the production sizes (Engine.conv2cls_begin takes nothing else)
U24 = 2.0 ** -24
BWD_SHAPES = {             # (B, H, W)
    "1x16x16": ((1, 16, 16), "two 8-blocks per axis: every block touches a border"),
    "2x24x16": ((2, 24, 16), "an interior 8-block with both neighbours on one axis; pool runs 3072 threads = 12 full workgroups"),
}
BWD_SETS = {
    "nominal": "unit normals, random signs",
    "scaled1536": "dy = 1536 (1 + u / 4) sgn(o): G8 and the mid class of P8 pass 65504, G4 does not",
    "scaled6144": "dy = 6144 (1 + u / 4) sgn(o), below 7680: G4 passes 65504 too",
    "tiny": "|dy| in [2^-14, 2^-10], around fp16's smallest normal",
}
BWD_OUTPUTS = ("dq5", "dq4", "dW5", "dW4", "dWm", "db")          # what the GPU test compares
BWD_STORED16 = ("dq5", "dq4", "dx32", "dq3", "dq2")              # what a 16-bit run stores in 16 bits (dx32: the q3 / q2 gradient at H x W)
# log2 of the weight scale per (set, shape, type): the largest power of two for which every BWD_STORED16 reference stays below 2^15
# (tests/test_conv2cls_parity_cpu.py::test_bwd_inputs_are_fair asserts that it is).  f32 runs nominal only, with bf16's scale.
# In fp16 the tiny set stops where the weights themselves leave the type (2^14 x a 4-sigma normal > 65504), not at the outputs.
BWD_WLOG2 = {
    ("nominal", "1x16x16", "bf16"): 4, ("nominal", "1x16x16", "f16"): 4, ("nominal", "2x24x16", "bf16"): 4, ("nominal", "2x24x16", "f16"): 4,
    ("scaled1536", "1x16x16", "bf16"): -9, ("scaled1536", "1x16x16", "f16"): -9, ("scaled1536", "2x24x16", "bf16"): -9, ("scaled1536", "2x24x16", "f16"): -9,
    ("scaled6144", "1x16x16", "bf16"): -11, ("scaled6144", "1x16x16", "f16"): -11, ("scaled6144", "2x24x16", "bf16"): -11, ("scaled6144", "2x24x16", "f16"): -11,
    ("tiny", "1x16x16", "bf16"): 15, ("tiny", "1x16x16", "f16"): 13, ("tiny", "2x24x16", "bf16"): 16, ("tiny", "2x24x16", "f16"): 13,
}


def bwd_dy(setname, seed, dtype, B, H, W):
    g = torch.Generator().manual_seed(seed)
    if setname == "nominal":
        dy = torch.randn(B, H, W, O2, generator=g)
    elif setname.startswith("scaled"):
        u = (2.0 * torch.rand(B, H, W, O2, generator=g) - 1.0) * (1.0 - 2.0 ** -6)      # (so that bf16's rounding cannot reach 1.25 A)
        sgn = torch.where(torch.arange(O2) % 2 == 0, 1.0, -1.0)
        dy = float(setname[6:]) * (1.0 + u / 4.0) * sgn
    else:
        mag = torch.exp2(-14.0 + 4.0 * torch.rand(B, H, W, O2, generator=g)).clamp(2.0 ** -14, 2.0 ** -10)
        dy = mag * torch.where(torch.rand(B, H, W, O2, generator=g) < 0.5, -1.0, 1.0)
    return dy.to(dtype).float()


def bwd_inputs(shape, setname, dtype, wlog2=None):
    """q5 .. q2 (NHWC), W [O][3][3][4 C] and dy [B, H, W, O] as f32 tensors holding exactly the values the device reads (quantised
    through the storage type; the weights AFTER their scale)."""
    (B, H, W), _ = BWD_SHAPES[shape]
    seed = 8000 + 100 * list(BWD_SHAPES).index(shape) + 10 * list(BWD_SETS).index(setname)
    if wlog2 is None:
        wlog2 = BWD_WLOG2[setname, shape, dn(BF if dtype == F32 else dtype)]
    q = [qnormal(seed + 1 + m, dtype, B, H >> sh, W >> sh, C2) for m, sh in enumerate((3, 2, 1, 0))]
    w = (rng_normal(seed + 5, O2, 3, 3, 4 * C2) * 2.0 ** wlog2).to(dtype).float()
    return q, w, bwd_dy(setname, seed + 6, dtype, B, H, W)


def _block_sum(t, s):
    B, H, W, K = t.shape
    return t.reshape(B, H // s, s, W // s, s, K).sum((2, 4))


def conv2_bwd_f64(q, w, dy):
    """Float64 autograd of sum(conv2d(cat(up8(q5), up4(q4), up2(q3), q2), W, pad 1) * dy).  -> dict: dq5 .. dq2 (NHWC at the member's
    resolution), dx32 [B, H, W, 2 C] (the gradient of cat(up2(q3), q2)), dx [B, H, W, 4 C], dW5 / dW4 [O][3][3][C], dWm [O][3][3][2 C], db."""
    qs = [t.double().permute(0, 3, 1, 2).contiguous().requires_grad_(True) for t in q]
    wd = w.double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    x = torch.cat([F.interpolate(t, scale_factor=f, mode="nearest") if f > 1 else t for t, f in zip(qs, (8, 4, 2, 1))], 1)
    x.retain_grad()
    (F.conv2d(x, wd, padding=1) * dy.double().permute(0, 3, 1, 2)).sum().backward()
    dw = wd.grad.permute(0, 2, 3, 1)
    dx = x.grad.permute(0, 2, 3, 1)
    out = {"dq%d" % (5 - m): qs[m].grad.permute(0, 2, 3, 1).contiguous() for m in range(4)}
    out.update(dx=dx.contiguous(), dx32=dx[..., 2 * C2:].contiguous(), dW5=dw[..., :C2].contiguous(), dW4=dw[..., C2: 2 * C2].contiguous(),
               dWm=dw[..., 2 * C2:].contiguous(), db=dy.double().sum((0, 1, 2)))
    return out


class BwdCase(object):
    """Inputs, float64 reference and magnitudes (the same operation on absolute values) of one (shape, set, type)."""

    def __init__(self, shape, setname, dtype, wlog2=None):
        self.shape, self.set, self.dtype = shape, setname, dtype
        (self.B, self.H, self.W), _ = BWD_SHAPES[shape]
        self.q, self.w, self.dy = bwd_inputs(shape, setname, dtype, wlog2)
        self.ref = conv2_bwd_f64(self.q, self.w, self.dy)
        self._mag = None

    @property
    def mag(self):
        if self._mag is None:
            self._mag = conv2_bwd_f64([t.abs() for t in self.q], self.w.abs(), self.dy.abs())
        return self._mag

    def stored16_max(self):
        return max(float(self.ref[k].abs().max()) for k in BWD_STORED16)


@functools.lru_cache(maxsize=None)
def bwd_case(shape, setname, dtype):
    return BwdCase(shape, setname, dtype)


def _slices(P):
    """Split-K slices of a weight-gradient launch over P pixels: at most one per 512 pixels (mpn_conv_wgrad_chunks), each one more add."""
    return max(1, -(-P // 512))


def class_allowance(case, p_store, gs):
    """Per member m (s = 8, 4): E [B, h, w, 9, O] = what the STORED intermediates may be off in an element of G_s — half a spacing (of the
    storage type at that magnitude, subnormal-aware; nothing for f32) of every stored P term that enters it, plus half a spacing of
    the stored G itself (stored as gs[s] G: the spacing of gs[s] |G|, divided by gs[s]).  Magnitudes are upper bounds of what the
    device holds: |reference| + the fp32 summation error + the allowances already made."""
    out = []
    for s in (8, 4):
        P = reduce_terms(pool_terms(case.dy, s))
        p_up = P.ref.abs() + (P.n - 1).clamp(min=0).double() * U24 * P.mag
        EP = reduce_terms(tapsum_terms(0.5 * ulp_out(p_up, p_store))).ref
        G = tap_direct(case.dy, s)
        g_up = G.ref.abs() + EP + (G.n - 1).clamp(min=0).double() * U24 * G.mag
        out.append(EP + 0.5 * ulp_out(g_up * gs[s], case.dtype) / gs[s])
    return out


def bwd_specs(case, route, p_store=None, gs=None):
    """name -> check_elementwise arguments (ref64, mag64, out_dtype, k_step, K, extra_terms, extra_abs, names) for every BWD_OUTPUTS
    entry of the class route or the plain route.  Nothing fitted:
      accumulation: the convolution launches at their real contraction length (K / k_step + k_step + 2 roundings on the magnitude;
        k_step 32 for the 16-bit MFMA, 4 for the exact-fp32 one), + one per split-K slice of a weight gradient, + the s^2 - 1 fp32
        additions of pool and tapsum behind an element of G (class route) or of the block sum of the up-sampled member's slice
        (plain route);  db: P - 1 additions in any order;
      stored intermediates: class route — `class_allowance` carried through |W| (input gradients) or |q| (filter gradients);
        plain route — half a spacing of every stored element of the full-resolution input gradient in the block;
      + half a spacing of the stored output (16-bit input gradients; the filter gradients are f32)."""
    dt = case.dtype
    ks = 4 if dt == F32 else 32
    B, H, W = case.B, case.H, case.W
    P = B * H * W
    specs = {}
    if route == "class":
        p_store = pool_store(dt) if p_store is None else p_store
        gs = {8: g_scale(dt, 8), 4: g_scale(dt, 4)} if gs is None else gs
        E = class_allowance(case, p_store, gs)
        for m, s in ((0, 8), (1, 4)):
            wm = case.w[..., m * C2: (m + 1) * C2].double().abs().reshape(O2, 9, C2)
            n = "%d" % (5 - m)
            specs["dq" + n] = dict(out_dtype=dt, k_step=ks, K=9 * O2, extra_terms=s * s - 1, names="bhwc",
                                   extra_abs=torch.einsum("bijto,otc->bijc", E[m], wm))
            specs["dW" + n] = dict(out_dtype=F32, k_step=ks, K=P // (s * s), extra_terms=s * s - 1 + _slices(P // (s * s)), names="orsc",
                                   extra_abs=torch.einsum("bijto,bijc->otc", E[m], case.q[m].double().abs()).reshape(O2, 3, 3, C2))
    else:
        dx_up = case.ref["dx"].abs() + (9 * O2 / float(ks) + ks + 2) * U24 * case.mag["dx"]
        half = 0.5 * ulp_out(dx_up, dt)
        for m, s in ((0, 8), (1, 4)):
            n = "%d" % (5 - m)
            specs["dq" + n] = dict(out_dtype=dt, k_step=ks, K=9 * O2, extra_terms=s * s - 1, names="bhwc",
                                   extra_abs=_block_sum(half[..., m * C2: (m + 1) * C2], s))
            specs["dW" + n] = dict(out_dtype=F32, k_step=ks, K=P, extra_terms=_slices(P), extra_abs=None, names="orsc")
    specs["dWm"] = dict(out_dtype=F32, k_step=ks, K=P, extra_terms=_slices(P), extra_abs=None, names="orsc")
    specs["db"] = dict(out_dtype=F32, k_step=1, K=P, extra_terms=_slices(P), extra_abs=None, names="o")
    for k, v in specs.items():
        v["ref64"], v["mag64"] = case.ref[k], case.mag[k]
    return specs


def check_bwd(tag, got, specs, route=""):
    """Every BWD_OUTPUTS entry of `got` element by element (one report line each; an element that is not finite where the reference is
    fails whatever the bound says: check_elementwise counts NaN and an infinite error as violations).  -> {name: worst err / bound}."""
    worst = {}
    for k in BWD_OUTPUTS:
        g = got[k].detach().cpu()
        assert bool(torch.isfinite(specs[k]["ref64"]).all())
        worst[k] = check_elementwise("%s %s" % (tag, k), g, route=route, **specs[k])
        assert bool(torch.isfinite(g.double()).all()), "%s %s: non-finite element" % (tag, k)
    return worst


def error_ratio(got_a, got_b, ref):
    """Element-wise errors of two results against the same float64 reference: (rms a / rms b, max a / max b)."""
    ea, eb = (got_a.double().cpu() - ref).abs(), (got_b.double().cpu() - ref).abs()
    rms = lambda e: float(e.pow(2).mean().sqrt())
    div = lambda a, b: a / b if b > 0 else (0.0 if a == 0 else float("inf"))
    return div(rms(ea), rms(eb)), div(float(ea.max()), float(eb.max()))


# fp32 models of the two routes.  `fault` (class route): None | 'parent' (P and G in the compute type, unscaled: what the kernels did
# before P went to f32 in fp16) | 'dgrad' (the input-gradient launch without its s^2) | 'fold' (fold without its s^2) | 'swapped' (the
# consumers take 16 for s = 8 and 64 for s = 4)
BWD_FAULTS = ("parent", "dgrad", "fold", "swapped")


def class_model(case, fault=None):
    """The class route in fp32 under the storage contract: pool (quadrant tree) -> P stored -> tapsum (the kernel's order) times the G
    factor -> G stored -> fp32 contractions -> the consumers' factors -> outputs rounded once."""
    dt = case.dtype
    ps = dt if fault == "parent" else pool_store(dt)
    out = {}
    for m, s, P in zip((0, 1), (8, 4), pool_tree(case.dy, F32)):
        gk = 1.0 if fault == "parent" else g_scale(dt, s)
        back = 1.0 / gk
        if fault == "swapped" and gk != 1.0:
            back = 1.0 / g_scale(dt, 12 - s)
        G = (reduce_terms(tapsum_terms(P.to(ps).float())).f32 * gk).to(dt).float()
        wm = case.w[..., m * C2: (m + 1) * C2].reshape(O2, 9, C2)
        n = "%d" % (5 - m)
        out["dq" + n] = (torch.einsum("bijto,otc->bijc", G, wm) * (1.0 if fault == "dgrad" else back)).to(dt)
        out["dW" + n] = (torch.einsum("bijto,bijc->otc", G, case.q[m]) * (1.0 if fault == "fold" else back)).reshape(O2, 3, 3, C2)
    out["dWm"], out["db"] = case.ref["dWm"].float(), case.ref["db"].float()      # (these two are plain launches in both routes)
    return out


def plain_model(case):
    """The plain route as fp32 accumulation of W dy rounded once: the float64 reference through f32 into the output type."""
    return {k: case.ref[k].float().to(case.dtype if k.startswith("dq") else F32) for k in BWD_OUTPUTS}
