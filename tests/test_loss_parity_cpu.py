"""CPU tier of the loss-kernel parity tests (csrc/losses.hip; bounds and references in tests/loss_ref.py).

1. Anchoring: the float64 references of loss_ref.py against independent sources — oracle.posenet_oracle.keypoint_loss / focal_loss /
   prn_loss with their autograd gradients, torch.softmax, and the recorded reference outputs g4_focal.npz / g16_focal_mc.npz.
2. Generator conditions of every GPU-tier case: no undecided anchor, grid-family exactness (the fp32 mirror of assign_anchor equals
   the float64 IoU rounded once), every planted edge present, positive / negative / ignored anchors present.
3. Teeth: an fp32 numpy model of each kernel's arithmetic on the GPU tier's own inputs must be ACCEPTED by the bounds — contracted
   and uncontracted, in the kernel's summation tree and in another order — and each modelled fault (the mutants named in the tests
   below) must be REJECTED."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import loss_ref as L
from helpers import gold
from loss_ref import f32, f64


@pytest.fixture(scope="module", autouse=True)
def _threads():
    n = torch.get_num_threads()
    torch.set_num_threads(min(n, 16))
    yield
    torch.set_num_threads(n)


def rejects(fn, *a, **k):
    with pytest.raises(AssertionError):
        fn(*a, **k)


def t64(x, grad=False):
    return torch.from_numpy(np.ascontiguousarray(x)).double().requires_grad_(grad)


def close(a, b, rtol=1e-9, atol=0.0):
    a, b = np.asarray(a, dtype=f64), np.asarray(b, dtype=f64)
    assert a.shape == b.shape, (a.shape, b.shape)
    err = np.abs(a - b)
    lim = rtol * np.abs(b) + atol
    assert (err <= lim).all(), "max err %.3e over limit at %s" % (err.max(), np.unravel_index(np.argmax(err - lim), a.shape))


# ====================================================================================================== 1. anchoring
@pytest.mark.parametrize("name", ["227px last partial chunk", "228px second chunk of 8"])
def test_mse_reference_equals_the_oracle_keypoint_loss(name):
    from oracle import posenet_oracle as po
    case = L.mse_case(name)
    ref = L.mse_ref(case)
    preds = [t64(s[..., :C].transpose(0, 3, 1, 2), True) for s, C in zip(case["store"], L.MSE_C)]
    total, log = po.keypoint_loss(preds, t64(case["gt"].transpose(0, 3, 1, 2)), t64(case["w"].transpose(0, 3, 1, 2)))
    (total * float(f64(case["gs"]))).backward()
    close(ref["total"], total.item())
    close(ref["loss"], list(log.values())[:5])
    assert log["max_ht"] == ref["max"] and log["min_ht"] == ref["min"]
    for j in range(5):
        close(ref["grad"][j], preds[j].grad.permute(0, 2, 3, 1).numpy(), rtol=1e-9, atol=1e-18)


@pytest.mark.parametrize("name", list(L.TRAIN_CASES))
def test_one_pass_reference_equals_the_oracle_on_upsampled_levels(name):
    from oracle import posenet_oracle as po
    case = L.train_case(name)
    ref = L.train_ref(case)
    leaves = [t64(x[..., :C], True) for x, C in zip(case["lv"], L.MSE_C)]
    up = [F.interpolate(x.permute(0, 3, 1, 2), size=(case["H"], case["W"]), mode="nearest") for x in leaves]      # posenet.py:243-257
    total, log = po.keypoint_loss(up, t64(case["heat"]), t64(case["w"]))
    (total * float(f64(case["gs"]))).backward()
    close(ref["loss"], list(log.values())[:5])
    assert log["max_ht"] == ref["max"] and log["min_ht"] == ref["min"]
    for j in range(5):
        close(ref["cgrad"][j], leaves[j].grad.numpy()[..., :18], rtol=1e-9, atol=1e-18)


def _no_edges(case):
    """The oracle clamps at the double constants 1e-4 and 1 - 1e-4, the kernels at the float ones (1 - HI differs by 1.7e-4 relative
    between the two): every value the clamp touches, the planted edges included, goes."""
    c = dict(case)
    c["cls"] = np.where((case["cls"] < 1.5e-4) | (case["cls"] > 1 - 1.5e-4), f32(0.3), case["cls"])
    return c


ANCHOR_KEYS = [("grid", 257, 3, 3, 2), ("grid", 256, 1, 8, 4), ("real", 256, 1, 8, 4), ("real", 600, 5, 3, 4), ("real", 1, 3, 8, 4)]


@pytest.mark.parametrize("key", ANCHOR_KEYS, ids=L.focal_tag)
def test_focal_reference_equals_the_oracle_focal_loss(key):
    from oracle import posenet_oracle as po
    case = _no_edges(L.make_focal(key))
    case["anno"] = np.where(case["anno"][..., 4:5] >= case["K"], f32(-1), case["anno"])       # the oracle cannot index a class id >= K
    ref = L.focal_eval(case)
    cls, reg = t64(case["cls"], True), t64(case["reg"], True)
    c, r = po.focal_loss(cls, reg, t64(case["anchors"])[None], t64(case["anno"]))
    (c * float(f64(L.FOCAL_GS[0])) + r * float(f64(L.FOCAL_GS[1]))).sum().backward()
    close(ref["out"], [c.item(), r.item()], rtol=1e-9)
    close(ref["dcls"], cls.grad.numpy(), rtol=1e-6, atol=1e-12)
    close(ref["dreg"], reg.grad.numpy(), rtol=1e-6, atol=1e-12)


@pytest.mark.parametrize("which", ["g4", "k3", "k80"])
def test_focal_reference_equals_the_recorded_reference_outputs(which):
    g = gold("g4_focal.npz" if which == "g4" else "g16_focal_mc.npz")
    p = "" if which == "g4" else which + "_"
    # the records come from an fp32 run of the reference and carry anchors whose IoU sits on 0.4: the fp32 mirror of the assignment
    # (family "grid") decides them as that run did; the tolerances are those of an fp32 record, not of the float64 reference
    case = dict(family="grid", cls=g[p + "cls"], reg=g[p + "reg"], anchors=g[p + "anchors"].reshape(-1, 4), anno=g[p + "anno"],
                gs=(f32(1), f32(1)))
    case.update(A=case["cls"].shape[1], K=case["cls"].shape[2])
    ref = L.focal_eval(case)
    close(ref["out"], g[p + "loss"], rtol=2e-6)
    for k in ("dcls", "dreg"):
        r = g[p + k].astype(f64)
        # dreg: the record's quadratic branch is 9 kr (r - t) with t from fp32 (|t| up to 3, a few roundings: ~1e-6) and max |dreg| = kr
        assert (np.abs(ref[k] - r) <= 2e-5 * np.abs(r) + (2e-5 if k == "dreg" else 1e-7) * np.abs(r).max()).all(), k


@pytest.mark.parametrize("cols", [17, 1000])
@pytest.mark.parametrize("relu", [1, 0])
def test_softmax_and_bce_references_equal_torch(cols, relu):
    from oracle import posenet_oracle as po
    c = L.softmax_case(cols, True)
    ref, _ = L.softmax_ref(c["a"], c["res"], cols, relu)
    a = t64(c["a"][:, :cols], True)
    res = t64(c["res"])
    out = torch.softmax((F.relu(a) if relu else a) + res, dim=1)
    close(ref, out.detach().numpy(), rtol=1e-12, atol=1e-300)
    # backward with the ReLU mask: autograd through relu -> softmax against check_softmax_bwd's reference (a bound of 0 elsewhere)
    dp = t64(c["dp"])
    (out * dp).sum().backward()
    p32 = ref.astype(f32)
    got = p32.astype(f64) * (c["dp"].astype(f64) - (p32.astype(f64) * c["dp"]).sum(1, keepdims=True))
    pre = c["a"] if relu else None
    if relu:
        got = np.where(c["a"][:, :cols] > 0, got, 0.0)
    L.check_softmax_bwd("anchor softmax bwd cols=%d relu=%d" % (cols, relu), got, p32, c["dp"], pre, cols)
    close(got, a.grad.numpy(), rtol=1e-5, atol=1e-6)              # p32 is the rounded probability
    p, y = L.bce_case(4097)
    Lr, _ = L.bce_ref(p, y)
    pt = t64(p, True)
    lt = po.prn_loss(pt, t64(y))
    (lt * L.BCE_GS).backward()
    close(Lr, lt.item(), rtol=1e-12)
    gref, _ = L.bce_bwd_ref(p, y, L.BCE_GS)
    inner = (p > 0) & (p < 1) & (p.astype(f64) * (1 - p.astype(f64)) > 1e-12)
    close(gref[inner], pt.grad.numpy()[inner], rtol=1e-6)


# ====================================================================================================== 2. generator conditions
@pytest.fixture(scope="module")
def focal_all():
    return {k: L.make_focal(k) for k in L.focal_cases()}


def test_focal_generator_conditions(focal_all):
    seen_maxn, seen = set(), set()
    for key, case in focal_all.items():
        fam, A, K, maxN, B = key
        L.check_focal_conditions(case)                                           # no undecided anchor / the grid / the switch / the clamp
        states = L.focal_state(case)
        st = np.concatenate([s[0] for s in states])
        if A >= 8:
            assert (st >= 0).any() and (st == -2).any() and (st == -1).any(), key
            live = np.stack([s[0] != -1 for s in states])
            for v in L.EDGE_P:                                                   # every clamp edge sits on an element that counts
                assert (case["cls"][live] == v).any(), (key, v)
        nvalid = [s[2] for s in states]
        npos = [int((s[0] >= 0).sum()) for s in states]
        if B >= 4:
            assert nvalid[2] == 0 and nvalid[1] > 0 and nvalid[3] > 0            # the empty image sits in the middle
            assert nvalid[3] > 0 and npos[3] == 0                                # annotations but no positive anchor
        if maxN >= 3:
            v = case["anno"][0, :, 4] != -1
            assert not v[1] and v[0] and v[2]                                    # a -1 row between valid ones
        seen_maxn.add((K, maxN)); seen.add((A, maxN))
        if fam == "grid":
            anc, ann = case["anchors"], case["anno"][0]
            i32, i64 = L.iou_matrix(anc, ann, f32), L.iou_matrix(anc, ann, f64)
            assert i32.dtype == np.float32 and (i32 == i64.astype(f32)).all(), key    # every operation exact up to the one division
            best, arg, second = L.assign(anc, ann, f32)
            at = case["planted_at"]
            assert best[at[0]] == f32(0.5) and states[0][0][at[0]] >= 0 and arg[at[0]] == 0      # exactly 1/2: positive, the first wins
            if maxN >= 3:
                assert second[at[0]] == best[at[0]]                              # a bit-equal second annotation
            if A > 6:
                assert best[at[1]] == L.T04 and states[0][0][at[1]] == -1        # exactly 2/5: ignored, not negative
                assert best[at[2]] == 1.0
                if maxN == 8:
                    assert best[at[3]] == 1.0 and ann[arg[at[3]], 2] - ann[arg[at[3]], 0] < 1     # the box narrower than a pixel
                    assert (ann[0, :4] == ann[3, :4]).all()                      # a duplicate annotation (the first wins)
    assert len(seen_maxn) == 15 and len({x for x in seen if x[0] != 64}) == 15       # every maxN meets every K and every A


def test_mse_and_head_generators_carry_their_edges():
    for name, (B, H, W, need) in L.MSE_CASES.items():
        c = L.mse_case(name)
        assert abs((c["w"] == 0).mean() - 0.1) < 0.1 or B * H * W == 1
        assert ((c["w"] != 0) & (c["w"] != 1)).any()
    assert [-(-B * H * W * 18 // L.MSE_CHUNK) for B, H, W, _ in L.MSE_CASES.values()] == [1, 1, 2, 257]
    assert 227 * 18 == 4086 and 228 * 18 == 4096 + 8
    p, y = L.bce_case(L.BCE_N[-1])
    assert -(-p.size // 4096) == 257 and (p == 0).any() and (p == 1).any() and ((y > 0) & (y < 1)).any()
    assert ((p.astype(f64) * (1 - p.astype(f64)) < 1e-12)).any()
    x, _, _ = L.sigmoid_case(257)
    assert x.min() == -100 and x.max() == 100 and np.isinf(np.exp(-x.astype(f32))).any()
    c = L.softmax_case(257, True)
    assert (c["a"][1, :257] < 0).all() and c["stride"] == 288 and (c["pre"][:, :257] == 0).any()
    assert np.ptp(c["a"][2, :257] + c["res"][2]) > 88                           # exponentials underflow
    assert L.mix64(0) == 0xE220A8397B1DCDAF                                      # splitmix64's first output for state 0


# ====================================================================================================== 3. teeth: fp32 models
def wave_tree(v):
    """v [..., 256] f32 -> block sum as the kernels form it: xor butterflies over 64 lanes, then ((s0 + s1) + s2) + s3."""
    v = v.reshape(v.shape[:-1] + (4, 64)).astype(f32)
    idx = np.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        v = v + v[..., idx ^ m]
    s = v[..., 0]
    return ((s[..., 0] + s[..., 1]) + s[..., 2]) + s[..., 3]


def chunk_sum(x, order, iters=16):
    """x [n] f32 -> per-chunk (256 * iters elements) f32 sums -> their float64 sum."""
    chunk = 256 * iters
    n = -(-x.size // chunk)
    x = np.concatenate([x, np.zeros(n * chunk - x.size, f32)]).reshape(n, iters, 256)
    if order == "tree":
        acc = np.zeros((n, 256), f32)
        for it in range(iters):
            acc = acc + x[:, it]
        part = wave_tree(acc)
    else:
        part = x.reshape(n, -1)[:, ::-1].sum(1, dtype=f32)
    return part.astype(f64).sum(), part


def fma(a, b, c):
    return (a.astype(f64) * b.astype(f64) + c.astype(f64)).astype(f32)


def mse_model(case, contract=False, order="tree", mut=None):
    npix = case["B"] * case["H"] * case["W"]
    N = npix * 18.0
    w, g = case["w"].reshape(-1), case["gt"].reshape(-1)
    out = np.zeros(8, f32)
    grads = []
    k = f32(case["gs"]) * f32(2) / f32(N)
    for j in range(5):
        p = np.ascontiguousarray(case["store"][j][..., :18]).reshape(-1)
        b = w * g
        d = fma(p, w, -b) if contract else p * w - b
        sq = d * d
        if mut == "last partial chunk dropped" and sq.size % L.MSE_CHUNK:
            sq = sq[: sq.size // L.MSE_CHUNK * L.MSE_CHUNK]
        s, _ = chunk_sum(sq, order)
        out[j] = f32(s / (npix if mut == "mean over pixels" else N))
        gr = np.zeros(case["store"][j].shape[:3] + (L.MSE_C[j],), f32)
        kw = k if mut == "gradient weighted by w once" else k * w
        gr[..., :18] = (kw * (p * w - b)).reshape(gr.shape[:3] + (18,))      # mse_grad: contraction off
        if mut == "channel 18 gradient not zero" and gr.shape[-1] > 18:
            gr[..., 18] = gr[..., 17]
        grads.append(gr if case["need"][j] else None)
    out[5] = (((out[0] + out[1]) + out[2]) + out[3]) + out[4]
    src = case["store"][4][..., :19] if mut == "max over channel 18 too" else case["store"][3][..., :18] if mut == "max from another level" \
        else case["store"][4][..., :18]
    out[6], out[7] = src.max(), src.min()
    return out, grads


def check_mse_model(case, ref, **kw):
    out, grads = mse_model(case, **kw)
    L.check_mse_out("model mse " + case["name"], out, ref, L.MSE_FWD_LEVELS, route=str(kw))
    L.check_mse_grads("model mse " + case["name"], grads, ref, case["need"], route=str(kw))


@pytest.mark.parametrize("name", list(L.MSE_CASES))
def test_mse_bounds_accept_the_fp32_model(name):
    case = L.mse_case(name)
    ref = L.mse_ref(case)
    for contract in (False, True):
        for order in ("tree", "flat"):
            check_mse_model(case, ref, contract=contract, order=order)


@pytest.mark.parametrize("mut", ["mean over pixels", "gradient weighted by w once", "last partial chunk dropped", "max over channel 18 too",
                                 "max from another level", "channel 18 gradient not zero"])
def test_mse_bounds_reject(mut):
    case = L.mse_case("228px second chunk of 8")
    case["need"] = [True] * 5
    rejects(check_mse_model, case, L.mse_ref(case), mut=mut)


def train_model(case, dtype, order="kernel", mut=None):
    """mse_train_kernel: full-resolution gradients by mse_grad (uncontracted), coarse levels summed over their children in the row-major
    walk of the 8x8 cell; losses per lane over its 64 pixels."""
    m = L.train_as_mse(case)
    B, H, W = case["B"], case["H"], case["W"]
    if mut == "level 2 indexed with px >> 1":
        x = case["lv"][2].repeat(4, axis=1)                                      # rows right, columns: (x0 >> 2) + (px >> 1)
        xi = (np.arange(W) // 8) * 2 + (np.arange(W) % 8) // 2
        m["store"][2] = x[:, :, np.minimum(xi, x.shape[2] - 1)]
    if mut == "rows and columns of the cell swapped":
        def tr(x):
            Bx, Hx, Wx, C = x.shape
            return x.reshape(Bx, Hx // 8, 8, Wx // 8, 8, C).transpose(0, 1, 4, 3, 2, 5).reshape(x.shape)
        m["store"][0], m["store"][4] = tr(m["store"][0]), tr(m["store"][4])
    m["need"], m["name"] = [True] * 5, case["name"]
    out, full = mse_model(m, order="flat")
    # losses: lane-sequential over the cell, then the block tree
    w, g = m["w"], m["gt"]
    for j in range(5):
        p = m["store"][j][..., :18]
        e = p * w - w * g
        sq = (e * e).reshape(B, H // 8, 8, W // 8, 8, 18).transpose(0, 1, 3, 5, 2, 4).reshape(-1, 64)        # [cell * channel, 64]
        lane = np.zeros(sq.shape[0], f32)
        for i in range(64):
            lane = lane + sq[:, i]
        out[j] = f32(lane.astype(f64).sum() / (B * H * W * 18.0)) if order == "kernel" else f32(sq.sum(dtype=f64) / (B * H * W * 18.0))
    out[5] = (((out[0] + out[1]) + out[2]) + out[3]) + out[4]
    grads = []
    for j, s in enumerate((0, 1, 2, 3, 0)):
        gfull = full[j][..., :18]
        f = 1 << s
        c = gfull.reshape(B, H // f, f, W // f, f, 18)
        acc = np.zeros((B, H // f, W // f, 18), f32)
        kids = [(r, q) for r in range(f) for q in range(f)]
        if order != "kernel":
            kids = kids[::-1]
        if mut == "one child missing" and s == 3:
            kids = kids[:-1]
        for r, q in kids:
            acc = acc + c[:, :, r, :, q]
        st = np.zeros(acc.shape[:3] + (32,), f32)
        st[..., :18] = acc
        grads.append(torch.from_numpy(st).to(dtype).double().numpy())
    return out, grads


@pytest.mark.parametrize("name", list(L.TRAIN_CASES))
@pytest.mark.parametrize("dtype", [L.F32, L.BF, L.H16])
def test_one_pass_bounds_accept_the_fp32_model(name, dtype):
    case = L.train_case(name)
    ref = L.train_ref(case)
    for order in ("kernel", "other"):
        out, grads = train_model(case, dtype, order)
        L.check_train("model train %s %s" % (name, dtype), out, grads, ref, dtype, route=order)


@pytest.mark.parametrize("dtype", [L.F32, L.BF])
@pytest.mark.parametrize("mut", ["one child missing", "level 2 indexed with px >> 1", "rows and columns of the cell swapped"])
def test_one_pass_bounds_reject(mut, dtype):
    case = L.train_case("2x16x40")
    ref = L.train_ref(case)
    out, grads = train_model(case, dtype, mut=mut)
    rejects(L.check_train, "mutant train", out, grads, ref, dtype)


def seq_sum(x):
    """Another order: fp32 pairwise from the far end."""
    return x.reshape(-1)[::-1].sum(dtype=f32)


def test_focal_bounds_accept_the_fp32_model(focal_all):
    for key, case in focal_all.items():
        ref = L.focal_eval(case)
        variants = [dict(), dict(contract=True, fsum=seq_sum)] if key[4] < 200 else [dict()]
        for kw in variants:
            got = L.focal_eval(case, ft=f32, **kw)
            L.check_focal("model " + L.focal_tag(key), got, ref, route="contract=%s" % kw.get("contract", False))


FOCAL_MUTANTS = [
    ("> at 0.5", ("grid", 257, 3, 8, 4)), ("<= at 0.4", ("grid", 257, 3, 8, 4)), ("last maximum wins", ("grid", 257, 3, 8, 4)),
    ("last maximum wins", ("grid", 255, 1, 3, 4)), ("alpha exchanged", ("real", 256, 1, 8, 4)), ("npos not clamped", ("grid", 255, 1, 3, 4)),
    ("factor 4 missing", ("real", 257, 2, 3, 4)), ("clamp passes gradient outside", ("grid", 256, 1, 8, 4)),
    ("clamp passes gradient outside", ("real", 600, 80, 8, 4)), ("upstream gradients swapped", ("real", 255, 3, 1, 4)),
    ("empty image contributes", ("grid", 600, 5, 3, 4)), ("gw clamped before the centre", ("grid", 257, 3, 8, 4)),
    ("positive column off by one across a row seam", ("real", 257, 3, 3, 2)), ("head element skipped", ("grid", 257, 3, 3, 2)),
    ("head element skipped", ("real", 257, 3, 3, 2)),
]


@pytest.mark.parametrize("mut,key", FOCAL_MUTANTS, ids=lambda v: v if isinstance(v, str) else L.focal_tag(v))
def test_focal_bounds_reject(mut, key, focal_all):
    case = focal_all[key]
    ref = L.focal_eval(case)
    rejects(L.check_focal, "mutant " + mut, L.focal_eval(case, mut=mut), ref)


def softmax_model(c, relu, order="tree", mut=None):
    cols = c["cols"]
    a, res = c["a"][:, :cols], c["res"]
    ra = np.maximum(a, f32(0)) if relu else a
    t = ra + res
    mx = ((a + res) if mut == "maximum before the ReLU" else t).max(1, keepdims=True)
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(t - mx).astype(f32)
        s = e.sum(1, keepdims=True, dtype=f32) if order == "flat" else np.stack([chunk_sum(r, "tree", -(-cols // 256))[1][0] for r in e])[:, None]
        return e * (f32(1) / s.astype(f32))


def softmax_bwd_model(p, dp, pre, cols, mut=None, contract=False):
    n = cols - 1 if mut == "tail column missing" else cols
    prod = p[:, :n].astype(f64) * dp[:, :n] if contract else (p[:, :n] * dp[:, :n])
    dot = prod.sum(1, keepdims=True, dtype=prod.dtype).astype(f32)
    g = p * (dp - dot)
    if pre is not None:
        g = np.where(pre[:, :cols] >= 0 if mut == "mask >= 0" else pre[:, :cols] > 0, g, f32(0))
    return g


@pytest.mark.parametrize("cols", L.SM_COLS)
def test_softmax_bounds_accept_the_fp32_model_and_reject_the_faults(cols):
    for padded in (0, 1):
        c = L.softmax_case(cols, padded)
        for relu in (1, 0):
            for order in ("tree", "flat"):
                p = softmax_model(c, relu, order)
                L.check_softmax("model softmax cols=%d" % cols, p, c["a"], c["res"], cols, relu, route="relu=%d %s" % (relu, order))
            for pre in (c["pre"], None):
                for contract in (False, True):
                    g = softmax_bwd_model(p, c["dp"], pre, cols, contract=contract)
                    L.check_softmax_bwd("model softmax bwd cols=%d" % cols, g, p, c["dp"], pre, cols)
    c = L.softmax_case(cols, 1)
    rejects(L.check_softmax, "mutant", softmax_model(c, 1, mut="maximum before the ReLU"), c["a"], c["res"], cols, 1)
    p = softmax_model(c, 1)
    if cols > 1:                                                                 # one column: the gradient is 0 whatever the mask
        rejects(L.check_softmax_bwd, "mutant", softmax_bwd_model(p, c["dp"], c["pre"], cols, mut="mask >= 0"), p, c["dp"], c["pre"], cols)
        rejects(L.check_softmax_bwd, "mutant", softmax_bwd_model(p, c["dp"], c["pre"], cols, mut="tail column missing"), p, c["dp"], c["pre"], cols)


def bce_model(p, y, order="tree", contract=False):
    with np.errstate(divide="ignore"):
        lp, lq = np.maximum(np.log(p), f32(-100)), np.maximum(np.log(f32(1) - p), f32(-100))
    term = -(fma(y, lp, (f32(1) - y) * lq) if contract else y * lp + (f32(1) - y) * lq)
    return f32(chunk_sum(term.astype(f32), order)[0] / p.size)


def check_bce(got, p, y):
    ref, bound = L.bce_ref(p, y)
    return L.chk("bce n=%d" % p.size, got, ref, [], extra_abs=bound)


@pytest.mark.parametrize("n", L.BCE_N)
def test_bce_bounds_accept_the_fp32_model_and_reject_the_faults(n):
    p, y = L.bce_case(n)
    for order in ("tree", "flat"):
        for contract in (False, True):
            got = bce_model(p, y, order, contract)
            assert np.isfinite(got)
            check_bce(got, p, y)
    rejects(check_bce, L.bce_ref(p, y, "no -100 clamp")[0], p, y)
    if n > 4096:
        rejects(check_bce, L.bce_ref(p, y, "divided by the chunk count")[0], p, y)
    ref, terms = L.bce_bwd_ref(p, y, L.BCE_GS)
    gs = f32(L.BCE_GS) / f32(n)
    got = gs * (p - y) / np.maximum(p * (f32(1) - p), L.BCE_EPS)
    assert np.isfinite(got).all()
    L.chk("model bce bwd n=%d" % n, got, ref, terms)
    rejects(L.chk, "mutant bce bwd (no 1e-12 clamp)", np.nan_to_num(gs * (p - y) / (p * (f32(1) - p)), posinf=3e38, neginf=-3e38), ref, terms)


@pytest.mark.parametrize("n", L.SIG_N)
def test_sigmoid_bounds_accept_the_fp32_model(n):
    x, dp, p = L.sigmoid_case(n)
    with np.errstate(over="ignore"):
        y = f32(1) / (f32(1) + np.exp(-x))
    L.check_sigmoid("model sigmoid n=%d" % n, y, x)
    L.check_sigmoid_bwd("model sigmoid bwd n=%d" % n, dp * p * (f32(1) - p), dp, p)
    rejects(L.check_sigmoid_bwd, "mutant sigmoid bwd", dp * p * (f32(1) + p), dp, p)


def test_dropout_mirror_and_step_log_reference():
    x = torch.arange(1, 5001, dtype=torch.float32) / 7
    for dt in (L.F32, L.BF, L.H16):
        y0, k0 = L.dropout_ref(x.to(dt), 123, 0.0)
        assert k0.all() and torch.equal(y0, x.to(dt))                            # p = 0 is the identity
        y, k = L.dropout_ref(x.to(dt), 123, 0.5)
        assert abs(float(k.float().mean()) - 0.5) < 0.03
        assert torch.equal(y[k], (x.to(dt).float() * 2).to(dt)[k]) and (y[~k] == 0).all()
    assert not np.array_equal(L.dropout_keep(5000, 123, 0.5), L.dropout_keep(5000, 124, 0.5))
    assert abs(L.dropout_keep(5000, 9, 0.9).mean() - 0.1) < 0.02
    kp8, det2 = np.arange(1, 9, dtype=f32) / 3, np.array([0.7, 0.2], f32)
    before = np.full(13, -5.0, f32)
    both = L.step_log_ref(kp8, det2, before)
    assert both[12] == -5 and both[11] == f32(kp8[5]) + (det2[0] + det2[1]) and (both[:8] == kp8).all()
    only = L.step_log_ref(None, det2, before)
    assert (only[:8] == -5).all() and only[11] == only[8] == det2[0] + det2[1]
    assert (L.step_log_ref(kp8, None, before)[8:11] == -5).all()


def test_one_pass_loss_refuses_weights_it_cannot_read():
    """mse_train_raw reads wgt with heat's strides and both with 16-byte loads: a broadcast, half-precision, differently shaped or
    misaligned weight tensor is refused by mse_train_supported(levels, heat, wgt), and mse_train_raw raises before any launch."""
    from multiposenet.pytorch_amd import ops
    from multiposenet.pytorch_amd._lib import MpnError
    from multiposenet.pytorch_amd.network import losses
    B, H, W = 2, 16, 24
    lv = [ops.Act(torch.zeros(B, H >> s, W >> s, 32), c) for s, c in ((0, 19), (1, 19), (2, 19), (3, 19), (0, 18))]
    heat, wgt = torch.zeros(B, 18, H, W), torch.ones(B, 18, H, W)
    assert losses.mse_train_supported(lv, heat) and losses.mse_train_supported(lv, heat, wgt)
    odd = torch.ones(B * 18 * H * W + 1)[1:].reshape(B, 18, H, W)               # contiguous f32, 4 bytes off a 16-byte boundary
    bad = [torch.ones(B, 1, H, W).expand(B, 18, H, W), wgt.half(), wgt.double(), torch.ones(B, 18, H, W + 8)[..., :W], wgt[:1], odd]
    for w in bad:
        assert not losses.mse_train_supported(lv, heat, w), (w.shape, w.dtype, w.stride())
        with pytest.raises(MpnError):
            losses.mse_train_raw(lv, heat, w, torch.ones(2), torch.float32)
    assert not losses.mse_train_supported(lv, heat.half(), wgt.half())          # the heat-map's dtype counts too
