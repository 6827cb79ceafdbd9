"""CPU tier of the conv2 position-class parity tests (csrc/conv2cls.hip; references, bounds and cases in tests/conv2cls_ref.py).

1. Anchoring: the definition-built references against the plain operation in float64 — conv3x3 of the nearest-up-sampled member, its
   autograd gradient — and against oracle/posenet_oracle.py: _conv2_position_classes (its class table and its un-rounded output).
2. Teeth: for every kernel and every case of the GPU tier, an fp32 model of the kernel's arithmetic in the kernel's own summation
   order and in another one must be ACCEPTED by the bound (worst err / bound goes to the parity report), and every modelled fault
   (MUTANTS) must be REJECTED — by the bound or by the exact comparison — except at the cases SURVIVES names, with the reason.
3. Generator conditions: where another class or neighbour would give a different value, it is further than the bound away
   (conv2cls_ref.assert_decided); the launch sizes are the stated ones; pool's one-pixel classes hold one pixel.
4. The ops.conv2cls_* wrappers refuse a non-dense operand, a channel width the kernel would misread and a dtype the entry point rejects,
   before they allocate anything.
5. conv2's whole backward (conv2cls_ref.bwd_case; the GPU tier drives the engine's own composition against it): the input sets are fair
   — the weight scale of every set is the largest power of two for which the float64 reference of everything a 16-bit run stores in
   16 bits stays below 2^15, and an fp32-accumulate, round-once model of the plain route passes the bound with finite outputs — the
   loss-scaled sets really take the unscaled 16-bit intermediates past 65504, the bound accepts the fp32 model of the class route
   under the storage contract (fp16: P in f32, G / s^2, the s^2 back behind both contractions) and rejects the kernels' former
   behaviour (inf on the loss-scaled sets), a compensation factor missing from either consumer, and swapped s = 8 / s = 4 factors."""
import pytest
import torch
import torch.nn.functional as F

import conv2cls_ref as R
from conv2cls_ref import BF, F32, F64, H16, TYPES, dn
from helpers import rng_normal


@pytest.fixture(scope="module", autouse=True)
def _threads():
    n = torch.get_num_threads()
    torch.set_num_threads(min(n, 16))
    yield
    torch.set_num_threads(n)


def rejected(fn, *a, **k):
    try:
        fn(*a, **k)
    except AssertionError:
        return True
    return False


def close(a, b, tol=1e-12):
    assert a.shape == b.shape, (a.shape, b.shape)
    err = float((a - b).abs().max())
    assert err <= tol * max(1.0, float(b.abs().max())), err


def up(x, s):
    return F.interpolate(x, scale_factor=s, mode="nearest")


# ====================================================================================================== 1. anchoring
ANCHOR_SHAPES = [(1, 8, 8), (2, 8, 24), (2, 16, 8)]          # B, H, W;  O = 8, C = 4


def test_frame_tables_of_both_scales_are_identical():
    assert R.frame_table(8) == R.frame_table(4) == R.FR
    w = rng_normal(1, 8, 3, 3, 16)
    for m in range(2):
        a = R.reduce_terms(R.frame_terms(w, m, R.frame_table(8), R.frame_table(8))).ref
        b = R.reduce_terms(R.frame_terms(w, m, R.frame_table(4), R.frame_table(4))).ref
        assert torch.equal(a, b)


def _member(seed, B, H, W, s, O=8, C=4):
    q = rng_normal(seed, B, C, H // s, W // s).double()
    w = rng_normal(seed + 1, O, 3, 3, 4 * C)                                    # KRSC, four members
    return q, w


@pytest.mark.parametrize("B,H,W", ANCHOR_SHAPES)
@pytest.mark.parametrize("s", [8, 4])
def test_expanded_class_maps_equal_the_convolution_of_the_upsampled_member(B, H, W, s):
    """conv3x3(q_s, Wc_s) expanded by class == conv3x3(nearest_up_s(q_s), W_member), pad 1 — through the frame filters and, separately,
    through the per-tap products and the class sums (the f32 route)."""
    O, C = 8, 4
    m = 0 if s == 8 else 1
    q, w = _member(10 * s + H + W, B, H, W, s)
    wm = w[..., m * C: (m + 1) * C].double().permute(0, 3, 1, 2)               # OIHW
    plain = F.conv2d(up(q, s), wm, padding=1).permute(0, 2, 3, 1)               # [B, H, W, O]
    frames = R.reduce_terms(R.frame_terms(w, m)).ref                            # [9, O, 3, 3, C]
    maps = F.conv2d(q, frames.reshape(9 * O, 3, 3, C).permute(0, 3, 1, 2), padding=1).permute(0, 2, 3, 1).reshape(B, H // s, W // s, 9, O)
    taps = torch.einsum("bcij,otc->bijto", q, wm.permute(0, 2, 3, 1).reshape(O, 9, C))       # the nine 1x1 convolutions
    zero8, zero4 = torch.zeros(B, H // 8, W // 8, 9, O, dtype=F64), torch.zeros(B, H // 4, W // 4, 9, O, dtype=F64)
    for M in (maps, R.reduce_terms(R.classsum_terms(taps)).ref):
        e = R.reduce_terms(R.expand_terms(M if s == 8 else zero8, M if s == 4 else zero4, H, W)).ref
        close(e, plain, 1e-13)


@pytest.mark.parametrize("B,H,W", ANCHOR_SHAPES)
@pytest.mark.parametrize("s", [8, 4])
def test_tap_sums_are_the_gradient_of_the_upsampled_convolution(B, H, W, s):
    """G_s[t] straight from dy == the kernel comment's F / M / L formula on the class sums P_s, and sum_t G_t W_t == autograd's gradient
    with respect to q_s of conv3x3(nearest_up_s(q_s), W_member)."""
    O, C = 8, 4
    m = 0 if s == 8 else 1
    q, w = _member(20 * s + H + W, B, H, W, s)
    dy = rng_normal(30 * s + H + W, B, H, W, O).double()
    wm = w[..., m * C: (m + 1) * C].double()                                    # [O, 3, 3, C]
    q.requires_grad_(True)
    (F.conv2d(up(q, s), wm.permute(0, 3, 1, 2), padding=1) * dy.permute(0, 3, 1, 2)).sum().backward()
    G = R.tap_direct(dy, s)
    close(torch.einsum("bijto,otc->bcij", G.ref, wm.reshape(O, 9, C)), q.grad, 1e-13)
    P = R.reduce_terms(R.pool_terms(dy, s)).ref
    Gp = R.reduce_terms(R.tapsum_terms(P))
    close(Gp.ref, G.ref, 1e-13)
    # the same through the comment's formula, written out per axis:  r = 0: M + L + F[i + 1]   r = 1: F + M + L   r = 2: L[i - 1] + F + M
    h, w_ = H // s, W // s
    Pp = F.pad(P.reshape(B, h, w_, 3, 3, O), (0, 0, 0, 0, 0, 0, 1, 1, 1, 1))     # zero blocks around
    ax = {0: ((0, 1), (0, 2), (1, 0)), 1: ((0, 0), (0, 1), (0, 2)), 2: ((-1, 2), (0, 0), (0, 1))}      # (block offset, class)
    for t in range(9):
        acc = 0
        for di, ci in ax[t // 3]:
            for dj, cj in ax[t % 3]:
                acc = acc + Pp[:, 1 + di: 1 + di + h, 1 + dj: 1 + dj + w_, ci, cj]
        close(acc, G.ref[:, :, :, t], 1e-13)
    # the float64 quadrant tree is the same sum
    p8, p4 = R.pool_tree(dy, F64)
    close(p8 if s == 8 else p4, P, 1e-13)


def test_frame_filters_equal_the_oracles():
    """The oracle's class table gives the same frame filters (bit for bit in float64), and its position-class model without rounding is
    relu(expand(conv3x3(q, frames))) of these references."""
    from oracle import posenet_oracle as po
    O, C, B, H, W = 8, 128, 1, 8, 16
    g = torch.Generator().manual_seed(5)
    w = torch.randn(O, 3, 3, 4 * C, generator=g).double()                         # KRSC
    for m in range(2):
        wm = w[..., m * C: (m + 1) * C]
        mine = R.reduce_terms(R.frame_terms(w, m)).ref
        for k in range(9):
            for u in range(3):
                for v in range(3):
                    taps = [wm[:, r, s] for r in po._CLS_ROWS[k // 3][u] for s in po._CLS_ROWS[k % 3][v]]
                    assert torch.equal(mine[k, :, u, v], sum(taps) if taps else torch.zeros(O, C, dtype=F64)), (m, k, u, v)
    assert po._QUANT is None
    q5, q4 = torch.randn(B, C, H // 8, W // 8, generator=g).double(), torch.randn(B, C, H // 4, W // 4, generator=g).double()
    sd = {"conv2.weight": w.permute(0, 3, 1, 2).contiguous(), "conv2.bias": torch.zeros(O, dtype=F64)}
    got = po._conv2_position_classes(sd, q5, q4, torch.zeros(B, C, H // 2, W // 2, dtype=F64), torch.zeros(B, C, H, W, dtype=F64))
    maps = []
    for m, q in ((0, q5), (1, q4)):
        fr = R.reduce_terms(R.frame_terms(w, m)).ref.reshape(9 * O, 3, 3, C).permute(0, 3, 1, 2)
        maps.append(F.conv2d(q, fr, padding=1).permute(0, 2, 3, 1).reshape(B, q.shape[2], q.shape[3], 9, O))
    e = R.reduce_terms(R.expand_terms(maps[0], maps[1], H, W)).ref
    close(got.permute(0, 2, 3, 1), F.relu(e), 1e-12)


# ====================================================================================================== 2. teeth
# kernel -> the modelled faults (names are conv2cls_ref's `mut` arguments)
MUTANTS = {
    "combine": {"first01": "`first` row collecting taps {0, 1} instead of {0}", "members": "members swapped", "tap_rows": "Wtap row o * 9 + t"},
    "expand": {"transposed": "row / column class transposed", "last_s2": "`last` taken at a == s - 2", "m8_shift2": "m8 indexed with >> 2"},
    "classsum": {"clamp": "border clamped instead of zero", "uv": "u / v swapped"},
    "pool": {"mid_rows": "P8 mid missing rows 4..6", "swap": "quadrants qa / qc swapped", "one_step": "one shuffle step dropped"},
    "tapsum": {"r02": "r = 0 and r = 2 swapped", "wrap": "border wrapped around", "drop": "one of the three axis terms dropped"},
    "fold": {"tap_rows": "o * 9 + t row index", "members": "members swapped", "assign": "= instead of +="},
}
# (kernel, fault, case) -> why the fault computes the right values there; every other (fault, case) must be rejected
SURVIVES = {
    ("expand", "m8_shift2", "1x8x8x8"): "m8 has one pixel: every index inside it is the right one (the overrun itself is not modelled)",
    ("classsum", "uv", "1x1x1x8"): "h = w = 1: a displaced row and a displaced column are both outside, whichever axis displaces",
}


def _judge(kernel, case, results):
    """results: {fault: rejected?}.  Every fault is rejected unless SURVIVES names the case; a named survivor must really survive."""
    for mut, rej in results.items():
        why = SURVIVES.get((kernel, mut, case))
        assert rej == (why is None), "%s / %s at %s: %s" % (kernel, MUTANTS[kernel][mut], case, "not rejected" if not rej else "listed as surviving (%s) but rejected" % why)


def _accept(tag, check, models):
    """models: {name of the summation order: result}: each must pass `check`."""
    for order, got in models.items():
        check("%s [fp32 model, %s]" % (tag, order), got)


REV9 = list(range(8, -1, -1))


@pytest.mark.parametrize("name", list(R.COMBINE_CASES))
def test_combine_bound_accepts_fp32_models_and_rejects_faults(name):
    w = R.combine_input(name)
    (O, C), _ = R.COMBINE_CASES[name]
    assert sum(R.comb_sizes(O, C)) + sum(R.comb_sizes(O, C)[1:]) == O * 9 * 2 * C + 2 * 81 * O * C + 2 * 9 * O * C
    _accept("combine " + name, lambda t, g: R.check_combine(t, g, w, "cpu"),
            {"(r, s) order": R.comb_flat(R.combine_parts(w), model=True), "reversed": R.comb_flat(R.combine_parts(w, order=REV9), model=True)})
    n = R.combine_parts(w)["wc"][0].n
    assert sorted(n.unique().tolist()) == [0, 1, 2, 3, 4, 6, 9]                  # structural zeros, copies, pairs and real sums all occur
    if name != "256x128":                                                        # (the faults move whole planes: the small cases decide them)
        _judge("combine", name, {m: rejected(R.check_combine, "mutant", R.comb_flat(R.combine_parts(w, mut=m), model=True), w, "cpu")
                                 for m in MUTANTS["combine"]})


@pytest.mark.parametrize("dtype", TYPES, ids=dn)
@pytest.mark.parametrize("name", list(R.EXPAND_CASES))
def test_expand_bound_accepts_fp32_models_and_rejects_faults(name, dtype):
    (B, H, W, O), _ = R.EXPAND_CASES[name]
    m8, m4 = R.expand_input(name)
    S = R.reduce_terms(R.expand_terms(m8, m4, H, W))
    chk = lambda t, g: R.check_sum(t, g, S, dtype, "cpu", "bhwo", exact_n=2 if dtype == F32 else 1)
    _accept("expand %s %s" % (name, dn(dtype)), chk,
            {"m8 + m4": S.f32.to(dtype), "m4 + m8": R.reduce_terms(R.expand_terms(m8, m4, H, W), order=[1, 0]).f32.to(dtype)})
    res = {}
    for m in MUTANTS["expand"]:
        alt = R.reduce_terms(R.expand_terms(m8, m4, H, W, mut=m))
        R.assert_decided("expand %s %s vs %s" % (name, dn(dtype), m), S, alt.ref, dtype, plane=0)
        res[m] = rejected(chk, "mutant", alt.f32.to(dtype))
    _judge("expand", name, res)


@pytest.mark.parametrize("name", list(R.CLASSSUM_CASES))
def test_classsum_bound_accepts_fp32_models_and_rejects_faults(name):
    (B, h, w, O), _ = R.CLASSSUM_CASES[name]
    t = R.low_input("classsum", name, F32)
    S = R.reduce_terms(R.classsum_terms(t))
    chk = lambda tag, g: R.check_sum(tag, g, S, F32, "cpu")
    _accept("classsum " + name, chk, {"(r, s) order": S.f32, "reversed": R.reduce_terms(R.classsum_terms(t), order=REV9).f32})
    assert int(S.n.min()) >= 1 and int(S.n.max()) == 9                           # (mid, mid) reads the pixel itself nine times
    res = {}
    for m in MUTANTS["classsum"]:
        alt = R.reduce_terms(R.classsum_terms(t, mut=m))
        R.assert_decided("classsum %s vs %s" % (name, m), S, alt.ref, F32)
        res[m] = rejected(chk, "mutant", alt.f32)
    _judge("classsum", name, res)


@pytest.mark.parametrize("dtype", TYPES, ids=dn)
@pytest.mark.parametrize("name", list(R.POOL_CASES))
def test_pool_bound_accepts_fp32_models_and_rejects_faults(name, dtype):
    (B, H, W, O), _ = R.POOL_CASES[name]
    assert R.pool_threads(B, H, W, O) == R.POOL_THREADS[name]
    dy = R.pool_input("pool", name, dtype)
    S8, S4 = R.reduce_terms(R.pool_terms(dy, 8)), R.reduce_terms(R.pool_terms(dy, 4))
    # one-pixel classes hold one pixel (the corners), the others 2 / 4 and 6 / 36
    assert S4.n[0, 0, 0, :, 0].tolist() == [1, 2, 1, 2, 4, 2, 1, 2, 1] and S8.n[0, 0, 0, :, 0].tolist() == [1, 6, 1, 6, 36, 6, 1, 6, 1]
    for k, (a, c) in zip((0, 2, 6, 8), ((0, 0), (0, 1), (1, 0), (1, 1))):
        for S, s in ((S8, 8), (S4, 4)):
            assert torch.equal(S.f32[:, :, :, k], dy[:, a * (s - 1)::s, c * (s - 1)::s])
    tag = "pool %s %s " % (name, dn(dtype))
    pt = R.pool_store(dtype)                                                     # fp16: P is stored in f32 — no output spacing to allow for
    assert pt == (F32 if dtype == H16 else dtype)
    c8 = lambda t, g: R.check_sum(t, g, S8, pt, "cpu")
    c4 = lambda t, g: R.check_sum(t, g, S4, pt, "cpu")
    p8, p4 = R.pool_tree(dy, F32)
    _accept(tag + "P8", c8, {"quadrant / shuffle tree": p8.to(pt), "sequential": S8.f32.to(pt)})
    _accept(tag + "P4", c4, {"quadrant order": p4.to(pt), "reversed": R.reduce_terms(R.pool_terms(dy, 4), order=REV9 + list(range(15, 8, -1))).f32.to(pt)})
    if dtype == H16:                                                             # ... so a P rounded to fp16 on the way is outside the bound
        assert rejected(c8, "P8 through fp16", p8.to(H16).float()) and rejected(c4, "P4 through fp16", p4.to(H16).float())
    res = {}
    for m in MUTANTS["pool"]:
        a8, a4 = R.pool_tree(dy, F64, mut=m)
        assert torch.equal(a4, R.pool_tree(dy, F64)[1])                          # (all three faults live in the 8 x 8 part)
        R.assert_decided(tag + "vs " + m, S8, a8, pt)
        res[m] = rejected(c8, "mutant", R.pool_tree(dy, F32, mut=m)[0].to(pt))
    _judge("pool", name, res)


@pytest.mark.parametrize("dtype", TYPES, ids=dn)
@pytest.mark.parametrize("name", list(R.LOW_CASES))
def test_tapsum_bound_accepts_fp32_models_and_rejects_faults(name, dtype):
    (B, h, w, O), _ = R.LOW_CASES[name]
    P = R.low_input("tapsum", name, R.pool_store(dtype))                         # the values the kernel reads: f32 class sums in fp16
    for s in ((8, 4) if dtype == H16 else (8,)):                                 # (the member's scale only matters where G is stored scaled)
        k = R.g_scale(dtype, s)
        assert k == (1.0 / (s * s) if dtype == H16 else 1.0)
        S = R.scaled(R.reduce_terms(R.tapsum_terms(P)), k)                       # a scaled G is referenced as the scaled sum
        chk = lambda t, g: R.check_sum(t, g, S, dtype, "cpu")
        _accept("tapsum %s %s x %g" % (name, dn(dtype), k), chk,
                {"the kernel's order": S.f32.to(dtype), "reversed": (R.reduce_terms(R.tapsum_terms(P), order=REV9).f32 * k).to(dtype)})
        assert int(S.n.min()) >= 4 and int(S.n.max()) == 9                       # r = 1 / s = 1 read the block's own three classes; r = 0 at least M and L
        if k != 1.0:                                                             # the unscaled sum, and the other member's factor, are outside
            assert rejected(chk, "unscaled", (S.f32 / k).to(dtype)) and rejected(chk, "the other member's factor", (S.f32 / k * R.g_scale(dtype, 12 - s)).to(dtype))
        res = {}
        for m in MUTANTS["tapsum"]:
            alt = R.scaled(R.reduce_terms(R.tapsum_terms(P, mut=m)), k)
            R.assert_decided("tapsum %s %s vs %s" % (name, dn(dtype), m), S, alt.ref, dtype)
            res[m] = rejected(chk, "mutant", alt.f32.to(dtype))
        _judge("tapsum", name, res)


@pytest.mark.parametrize("name", list(R.COMBINE_CASES))
def test_fold_reference_rejects_faults(name):
    (O, C), _ = R.COMBINE_CASES[name]
    dcomb, dw0 = R.fold_inputs(O, C)
    ref = R.fold_ref(dcomb, dw0, O, C)
    assert ref.dtype == F32
    # against the definition in float64: the add is one rounding
    g64 = ref.double() - dw0.reshape(O, 9, 4 * C).double()
    assert float((g64.abs() - g64.abs().round()).abs().max()) <= 2.0 ** -24 * float(ref.abs().max())
    _judge("fold", name, {m: not torch.equal(R.fold_ref(dcomb, dw0, O, C, mut=m), ref) for m in MUTANTS["fold"]})
    # fp16: the per-tap slices come back times 64 / 16 (exact: the ramp stays below 2^30 with 24 significant bits); a factor missing
    # from fold, or the two swapped, moves every element of those slices
    assert R.fold_scale(H16) == (64.0, 16.0) and R.fold_scale(BF) == R.fold_scale(F32) == (1.0, 1.0)
    ref16 = R.fold_ref(dcomb, dw0, O, C, scale=R.fold_scale(H16))
    g16 = ref16.double() - dw0.reshape(O, 9, 4 * C).double()
    assert torch.equal(ref16[..., 2 * C:], ref[..., 2 * C:])
    for m, k in ((0, 64.0), (1, 16.0)):
        assert float(((g16 - k * g64)[..., m * C: (m + 1) * C].abs() / (k * g64[..., m * C: (m + 1) * C].abs())).max()) <= 2.0 ** -23
    for wrong in ((1.0, 1.0), (16.0, 64.0)):
        assert bool((R.fold_ref(dcomb, dw0, O, C, scale=wrong) != ref16)[..., : 2 * C].all())
    for m in ("tap_rows", "members"):                                            # an index fault moves (nearly) every element it can
        moved = (R.fold_ref(dcomb, dw0, O, C, mut=m) != ref)[..., : 2 * C]
        assert float(moved.double().mean()) > 0.7, (m, float(moved.double().mean()))


@pytest.mark.parametrize("dtype", TYPES, ids=dn)
@pytest.mark.parametrize("name", list(R.CHAIN_CASES))
def test_chain_bound_accepts_the_fp32_model(name, dtype):
    """dy -> pool -> (stored in pool_store(dtype)) -> tapsum (times g_scale) against G straight from dy: the bound holds for the fp32 model
    of both kernels, and is missed by a chain whose pool is faulty."""
    (B, H, W, O), _ = R.CHAIN_CASES[name]
    dy = R.pool_input("chain", name, dtype)
    pt = R.pool_store(dtype)
    for mut, want_reject in ((None, False), ("one_step", True), ("mid_rows", True)):
        p8, p4 = R.pool_tree(dy, F32, mut=mut)
        for s, P in ((8, p8), (4, p4)):
            k = R.g_scale(dtype, s)
            Pst = P.to(pt).float()
            G = (R.reduce_terms(R.tapsum_terms(Pst)).f32 * k).to(dtype)
            D = R.scaled(R.tap_direct(dy, s), k)
            chk = lambda: R.check_sum("chain %s %s G%d [fp32 model]" % (name, dn(dtype), s), G, D, dtype, "cpu", exact_n=-1, extra_abs=k * R.chain_extra(Pst, pt))
            if mut is None:
                chk()
            elif s == 8:
                assert rejected(chk) == want_reject


# ====================================================================================================== 4. wrapper argument checks
class _NoAlloc(object):
    """ops.torch replaced so that any allocation inside the wrapper fails the test."""

    def __getattr__(self, k):
        if k in ("empty", "empty_like", "zeros", "zeros_like", "full"):
            raise RuntimeError("the wrapper allocated before it checked its operand")
        return getattr(torch, k)


@pytest.fixture
def ops_noalloc():
    from multiposenet.pytorch_amd import ops
    ops.torch = _NoAlloc()
    yield ops
    ops.torch = torch


def test_wrappers_refuse_what_the_kernels_would_misread(ops_noalloc):
    ops = ops_noalloc
    from multiposenet.pytorch_amd._lib import MpnError
    A = ops.Act

    def bad(fn, *a):
        with pytest.raises(MpnError):
            fn(*a)
    dense = torch.zeros(1, 2, 2, 72)
    # non-contiguous: a channel slice of a wider tensor, and a permuted view
    wide = torch.zeros(1, 2, 2, 80)[..., :72]
    perm = torch.zeros(1, 2, 72, 2).permute(0, 1, 3, 2)
    for t in (wide, perm):
        assert not t.is_contiguous()
        bad(ops.conv2cls_classsum, A(t, 72))
        bad(ops.conv2cls_tapsum, A(t, 72), 8, F32)
    bad(ops.conv2cls_pool, A(torch.zeros(1, 8, 8, 16)[..., :8], 8))
    bad(ops.conv2cls_expand, A(wide, 72), A(torch.zeros(1, 4, 4, 72), 72), 1, 16, 16, 8, torch.float32)
    # widths the kernel would misread
    bad(ops.conv2cls_classsum, A(torch.zeros(1, 2, 2, 64), 64))                 # not 9 planes
    bad(ops.conv2cls_classsum, A(torch.zeros(1, 2, 2, 54), 54))                 # O = 6: no multiple of 4
    bad(ops.conv2cls_tapsum, A(torch.zeros(1, 2, 2, 64), 64), 8, F32)
    bad(ops.conv2cls_tapsum, A(torch.zeros(1, 2, 2, 36), 36), 8, F32)           # O = 4: tapsum's entry point needs O % 8
    bad(ops.conv2cls_tapsum, A(dense, 72), 2, F32)                               # the member's scale is 8 or 4
    bad(ops.conv2cls_pool, A(torch.zeros(1, 8, 8, 12), 12))                     # O % 8
    bad(ops.conv2cls_pool, A(torch.zeros(1, 8, 12, 8), 8))                      # W % 8
    bad(ops.conv2cls_expand, A(dense, 72), A(torch.zeros(1, 4, 4, 72), 72), 1, 16, 16, 16, torch.float32)      # O is not Cs / 9
    bad(ops.conv2cls_expand, A(dense, 72), A(torch.zeros(1, 2, 2, 72), 72), 1, 16, 16, 8, torch.float32)       # m4 at the wrong resolution
    # dtypes the entry points reject
    bad(ops.conv2cls_classsum, A(dense.to(BF), 72))                              # classsum is f32 only
    bad(ops.conv2cls_tapsum, A(dense.double(), 72), 8, F64)
    bad(ops.conv2cls_tapsum, A(dense.to(H16), 72), 8, H16)                       # fp16's class sums are f32 (conv2cls_pool writes them so)
    bad(ops.conv2cls_tapsum, A(dense, 72), 4, BF)                                # bf16's are bf16
    bad(ops.conv2cls_pool, A(torch.zeros(1, 8, 8, 8, dtype=F64), 8))
    bad(ops.conv2cls_expand, A(dense.to(H16), 72), A(torch.zeros(1, 4, 4, 72), 72), 1, 16, 16, 8, torch.float32)   # class maps are f32
    bad(ops.conv2cls_expand, A(dense, 72), A(torch.zeros(1, 4, 4, 72), 72), 1, 16, 16, 8, F64)
    # a well-formed operand passes the checks and reaches the allocation
    for fn, a in ((ops.conv2cls_classsum, (A(dense, 72),)), (ops.conv2cls_tapsum, (A(dense.to(BF), 72), 8, BF)), (ops.conv2cls_tapsum, (A(dense, 72), 4, H16)),
                  (ops.conv2cls_pool, (A(torch.zeros(1, 8, 8, 8), 8),)), (ops.conv2cls_pool, (A(torch.zeros(1, 8, 8, 8, dtype=H16), 8),))):
        with pytest.raises(RuntimeError, match="allocated"):
            fn(*a)


# ====================================================================================================== 5. conv2's whole backward
BWD_CASES = [(sh, st, dt) for dt in TYPES for sh in R.BWD_SHAPES for st in R.BWD_SETS if dt != F32 or st == "nominal"]
BWD_IDS = ["%s-%s-%s" % (dn(dt), st, sh) for sh, st, dt in BWD_CASES]


def test_bwd_reference_is_the_definition():
    """conv2cls_ref.conv2_bwd_f64 against the explicit transposed sums, and the class formulation against it: the member's input gradient
    is the block sum of the full-resolution one, sum_t G_t W_t is that block sum, sum_pixels G_t q is the member's filter gradient."""
    c = R.bwd_case("1x16x16", "nominal", BF)
    dy, w = c.dy.double().permute(0, 3, 1, 2), c.w.double().permute(0, 3, 1, 2)
    close(F.conv_transpose2d(dy, w, padding=1).permute(0, 2, 3, 1), c.ref["dx"], 1e-12)
    x = torch.cat([up(t.double().permute(0, 3, 1, 2), f) if f > 1 else t.double().permute(0, 3, 1, 2) for t, f in zip(c.q, (8, 4, 2, 1))], 1)
    dw = torch.nn.grad.conv2d_weight(x, w.shape, dy, padding=1).permute(0, 2, 3, 1)
    close(dw, torch.cat([c.ref["dW5"], c.ref["dW4"], c.ref["dWm"]], 3), 1e-12)
    for m, s in ((0, 8), (1, 4)):
        n = "%d" % (5 - m)
        close(R._block_sum(c.ref["dx"][..., m * 128: (m + 1) * 128], s), c.ref["dq" + n], 1e-12)
        G = R.tap_direct(c.dy, s).ref
        close(torch.einsum("bijto,otc->bijc", G, c.w[..., m * 128: (m + 1) * 128].double().reshape(256, 9, 128)), c.ref["dq" + n], 1e-12)
        close(torch.einsum("bijto,bijc->otc", G, c.q[m].double()).reshape(256, 3, 3, 128), c.ref["dW" + n], 1e-12)
    close(R._block_sum(c.ref["dx32"][..., :128], 2), c.ref["dq3"], 1e-12)
    assert torch.equal(c.ref["dx32"][..., 128:], c.ref["dq2"])


@pytest.mark.parametrize("shape,setname,dtype", [c for c in BWD_CASES if c[2] != F32], ids=[i for i, c in zip(BWD_IDS, BWD_CASES) if c[2] != F32])
def test_bwd_inputs_are_fair(shape, setname, dtype):
    """The inputs are the stated ones (quantised through the storage type, the stated ranges), the weight scale is the LARGEST power of
    two that keeps every reference of a 16-bit stored output below 2^15 (one more doubling does not: an output reaches 2^15, or — the
    tiny set in fp16 — the weights themselves leave the type), and the round-once model of the plain route passes the plain bound,
    finite.  So whatever fails on these inputs is the class route's own doing."""
    c = R.bwd_case(shape, setname, dtype)
    for t in c.q + [c.w, c.dy]:
        assert torch.equal(t, t.to(dtype).float()) and bool(torch.isfinite(t).all())
    a = c.dy.abs()
    if setname.startswith("scaled"):
        A = float(setname[6:])
        sgn = torch.where(torch.arange(256) % 2 == 0, 1.0, -1.0)
        assert bool((c.dy * sgn > 0).all()) and 0.75 * A <= float(a.min()) and float(a.max()) < 1.25 * A <= 7680
    elif setname == "tiny":
        assert 2.0 ** -14 <= float(a.min()) and float(a.max()) <= 2.0 ** -10 and 0.4 < float((c.dy > 0).double().mean()) < 0.6
    top = c.stored16_max()
    assert top < 2.0 ** 15, top
    k = R.BWD_WLOG2[setname, shape, dn(dtype)]
    q, w2, dy = R.bwd_inputs(shape, setname, dtype, wlog2=k + 1)
    if bool(torch.isfinite(w2).all()):
        r2 = R.conv2_bwd_f64(q, w2, dy)
        assert max(float(r2[n].abs().max()) for n in R.BWD_STORED16) >= 2.0 ** 15
    else:
        assert dtype == H16 and setname == "tiny"
    got = R.plain_model(c)
    assert all(bool(torch.isfinite(v).all()) for v in got.values())
    R.check_bwd("conv2 bwd %s %s %s [round-once model of the plain route]" % (shape, setname, dn(dtype)), got, R.bwd_specs(c, "plain"), "cpu")


@pytest.mark.parametrize("shape", list(R.BWD_SHAPES))
def test_bwd_loss_scaled_sets_pass_fp16_where_stated(shape):
    """What each amplitude is for: at 1536 the unscaled G8 (64 dy) passes 65504 while G4 and both P do not (the mid class of P8, 36 dy
    of mean 1536, reaches 6.0e4: it passes from |dy| ~ 1820); at 6144 G4 and the mid class of P8 pass as well (P4's mid class of four
    pixels cannot); G / s^2 and dy itself stay inside the type."""
    top = {}
    for st in ("scaled1536", "scaled6144"):
        c = R.bwd_case(shape, st, H16)
        for s in (8, 4):
            top[st, "P", s] = float(R.reduce_terms(R.pool_terms(c.dy, s)).ref.abs().max())
            top[st, "G", s] = float(R.tap_direct(c.dy, s).ref.abs().max())
        assert float(c.dy.abs().max()) < 7680 and top[st, "G", 8] / 64 < 7680 and top[st, "G", 4] / 16 < 7680
    assert top["scaled1536", "G", 8] > 65504 > max(top["scaled1536", "P", 8], top["scaled1536", "G", 4], top["scaled1536", "P", 4])
    assert min(top["scaled6144", "G", 8], top["scaled6144", "G", 4], top["scaled6144", "P", 8]) > 65504 > top["scaled6144", "P", 4]


@pytest.mark.parametrize("shape,setname,dtype", BWD_CASES, ids=BWD_IDS)
def test_bwd_bound_accepts_the_fp32_model_and_rejects_faults(shape, setname, dtype):
    c = R.bwd_case(shape, setname, dtype)
    specs = R.bwd_specs(c, "class")
    tag = "conv2 bwd %s %s %s " % (shape, setname, dn(dtype))
    R.check_bwd(tag + "[fp32 model of the class route]", R.class_model(c), specs, "cpu")
    if dtype != H16:
        # nothing is scaled outside fp16: the faulty contracts are the contract itself
        for f in R.BWD_FAULTS:
            m, g = R.class_model(c, f), R.class_model(c)
            assert all(torch.equal(m[k], g[k]) for k in R.BWD_OUTPUTS), f
        return
    for f in R.BWD_FAULTS:
        got = R.class_model(c, f)
        assert rejected(R.check_bwd, tag + f, got, specs, "cpu"), "%s not rejected" % f
        if f == "parent" and setname.startswith("scaled"):
            bad = [k for k in R.BWD_OUTPUTS if not bool(torch.isfinite(got[k]).all())]
            assert bad == (["dq5", "dW5"] if setname == "scaled1536" else ["dq5", "dq4", "dW5", "dW4"]), bad
