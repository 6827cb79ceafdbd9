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
The chain dy -> pool -> tapsum adds, as extra_abs, half a spacing of every stored P term that enters the element."""
import torch

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


def chain_extra(P_stored, dtype):
    """Half a spacing of every stored P term that enters an element of G (the intermediate rounding of the chain)."""
    return reduce_terms(tapsum_terms(0.5 * ulp_out(P_stored.double(), dtype))).ref


# ------------------------------------------------------------------------------------------------ fold
def fold_ref(dcomb, dw0, O, C, mut=None):
    """dw0 [O][9][4 C] + g in fp32 (one correctly rounded add), g from dcomb = dWm [O][9][2C] | dWtap8 [9][O][C] | dWtap4 [9][O][C]: the
    gradient of row t * O + o of a per-tap set belongs to tap t of output channel o.  mut: 'tap_rows' | 'members' | 'assign'."""
    nm, _, nt = comb_sizes(O, C)
    g = torch.empty(O, 9, 4 * C, dtype=F32)
    g[..., 2 * C:] = dcomb[:nm].reshape(O, 9, 2 * C)
    for m in range(2):
        src = dcomb[nm + m * nt: nm + (m + 1) * nt]
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
