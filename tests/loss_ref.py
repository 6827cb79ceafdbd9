"""Float64 references, per-element bounds and input generators of the loss and PRN head kernels (csrc/losses.hip), shared by
tests/test_loss_parity_gpu.py (which compares the kernels with them) and tests/test_loss_parity_cpu.py (which anchors the references
to independent sources and shows that the bounds reject modelled faults).  Test-side only; numpy on the CPU.

References: build_keypoint_loss posenet.py:367-403, calc_iou losses.py:5-22, FocalLoss losses.py:27-137, PRN softmax
posenet.py:343-347, BCELoss posenet.py:427-445 — each written plainly in float64 on exactly the float32 operand values (and the
float32 constants: 1e-4f, 1 - 1e-4f, 0.1f, 0.2f, 1/9f, 0.5f/9f, 0.4f, 1e-8f, 1e-12f) the kernel reads.

Bounds.  u = 2^-24.  Every fp32 rounding on the path of an element is charged u times the magnitude of what is rounded (the "same
operation on absolute values" rule of helpers.check_elementwise, through which every comparison here goes: `terms` is a list of
(number of roundings, magnitude) pairs).  Sums are charged (levels of the summation tree the kernel has) * u * sum |terms|; the level
counts are the constants below.  logf / expf: no HIP math accuracy table ships with the ROCm installation, so the OpenCL full-profile
limit of 3 ulp is used for both (ULP_LOG, ULP_EXP; 1 ulp <= 2^-23 relative = 2 u).  Division and sqrt are correctly rounded (no
fast-math in the Makefile).  Second-order terms (u^2) are covered by the factor (1 + 2^-10) on the bounds of sums of squares.  Two
absolute terms: logf(1 - p) carries 2^-25 / (1 - p) from the rounding of 1 - p (p < 1/2; for p >= 1/2 the subtraction is exact), and a
softmax exponential carries u (|relu(a)| + |res| + |max| + |arg|) relative from its rounded argument.  Results below the smallest
normal float (2^-126) may be flushed: TINY is added where an exponential can underflow.  No bound is tuned against a kernel."""
import numpy as np
import torch

from helpers import U24, check_elementwise, report, round_up
from stream_ref import exact, roundings

F32, BF, H16 = torch.float32, torch.bfloat16, torch.float16
f32, f64 = np.float32, np.float64
U = U24
ULP_LOG = ULP_EXP = 3                   # OpenCL full profile (no HIP accuracy table under the ROCm installation)
R_LOG, R_EXP = 2 * ULP_LOG, 2 * ULP_EXP  # in units of u
TINY = 2.0 ** -126
SQ = 1.0 + 2.0 ** -10                   # second-order cover for squared differences

# summation trees (losses.hip)
WAVE_LEVELS = 6                         # wave_sum: 6 shuffle steps
BLOCK_LEVELS = WAVE_LEVELS + 3          # + sh[0] + sh[1] + sh[2] + sh[3]
MSE_CHUNK = 4096
MSE_FWD_LEVELS = 16 + BLOCK_LEVELS      # 16 sequential adds per lane, then the block; double precision after that
MSE_TRAIN_LEVELS = 64 + BLOCK_LEVELS    # one lane walks the 64 pixels of its cell
BCE_LEVELS = 16 + BLOCK_LEVELS
FMC_TILE = 256

LO, HI = f32(1e-4), f32(1) - f32(1e-4)
C01, C02 = f32(0.1), f32(0.2)
NINTH, HALF9 = f32(1) / f32(9), f32(0.5) / f32(9)
T04, T05 = f32(0.4), f32(0.5)
UA_MIN, BCE_EPS = f32(1e-8), f32(1e-12)


def T(a):
    return torch.from_numpy(np.ascontiguousarray(np.atleast_1d(np.asarray(a, dtype=f64))))


def chk(name, got, ref, terms, out_dtype=F32, extra_abs=None, route="", names="i"):
    """check_elementwise with bound 0.5 ulp_out + u * sum n_i mag_i [+ extra_abs]."""
    ref = np.atleast_1d(np.asarray(ref, dtype=f64))
    mag = np.zeros_like(ref)
    for n, m in terms:
        mag = mag + n * np.abs(np.asarray(m, dtype=f64))
    got = got.detach().cpu() if torch.is_tensor(got) else torch.from_numpy(np.ascontiguousarray(np.atleast_1d(np.asarray(got))))
    got = got.reshape(ref.shape)
    ea = None if extra_abs is None else T(np.array(np.broadcast_to(np.asarray(extra_abs, dtype=f64), ref.shape)))
    nm = names if len(names) >= ref.ndim else "".join("ijklm"[: ref.ndim])
    return check_elementwise(name, got, T(ref), T(mag), out_dtype, route=route, names=nm, extra_abs=ea, **roundings(1))


def same(name, got, ref, route=""):
    got = got.detach().cpu() if torch.is_tensor(got) else torch.from_numpy(np.ascontiguousarray(np.atleast_1d(np.asarray(got))))
    ref = torch.from_numpy(np.ascontiguousarray(np.atleast_1d(np.asarray(ref)))).to(got.dtype).reshape(got.shape)
    exact(name, got, ref, route)


def rng(seed):
    return np.random.RandomState(seed)


# ====================================================================================================== heat-map MSE
MSE_C = (19, 19, 19, 19, 18)            # live channels of the five predictions
MSE_STRIDE = (19, 32, 19, 32, 32)       # pixel strides: dense and Act storage mixed in one call
MSE_CASES = {                           # name -> (B, H, W, need)
    "1px": (1, 1, 1, [True] * 5),
    "227px last partial chunk": (1, 1, 227, [True] * 5),
    "228px second chunk of 8": (1, 12, 19, [True, True, None, True, True]),
    "241x242 257 chunks": (1, 241, 242, [True] * 5),
}
MSE_GS = 1.7
PLANT = 1e3                             # larger than any live value: planted where max / min must not look
PLANT_LIVE = 50.0                       # a live value of another level, larger than any of the final prediction


def mse_case(name):
    """Five prediction storages [B,H,W,stride_j] (f32; lanes >= C_j zero except the planted ones), pixel-major targets."""
    B, H, W, need = MSE_CASES[name]
    r = rng(len(name) * 7 + B * H * W)
    store = []
    for C, S in zip(MSE_C, MSE_STRIDE):
        x = np.zeros((B, H, W, S), f32)
        x[..., :C] = r.standard_normal((B, H, W, C)).astype(f32)
        store.append(x)
    store[4][..., 18] = f32(PLANT)      # the 19th lane of the final prediction's storage: not a heat-map channel
    store[4][..., 19] = f32(-PLANT)
    store[3][0, 0, 0, 0] = f32(PLANT_LIVE)   # another level
    store[0][0, 0, 0, 18] = f32(-PLANT)  # channel 18 of a 19-channel level
    gt = r.random_sample((B, H, W, 18)).astype(f32)
    w = (r.random_sample((B, H, W, 18)) * (r.random_sample((B, H, W, 18)) > 0.1)).astype(f32)
    return dict(name=name, B=B, H=H, W=W, need=need, store=store, gt=gt, w=w, gs=f32(MSE_GS))


def _mse_terms(p, w, g):
    a, b = p * w, w * g
    d = a - b
    return a, b, d


def mse_ref(case):
    """float64: losses[5], total, max, min, grads (list of [B,H,W,C_j], channel 18 zero) and their bounds."""
    npix = case["B"] * case["H"] * case["W"]
    N = npix * 18.0
    w, g = case["w"].astype(f64), case["gt"].astype(f64)
    k = f64(case["gs"]) * 2.0 / N
    ref = dict(loss=[], loss_b=[], grad=[], grad_terms=[])
    for j in range(5):
        p = case["store"][j][..., :18].astype(f64)
        a, b, d = _mse_terms(p, w, g)
        L = (d * d).sum() / N
        # a, b, a - b rounded: |delta d| <= u (|a| + |b| + |d|); d * d: 2 |d| |delta d| + u d^2; tree; (float)(double / N)
        per = 2 * np.abs(d) * (np.abs(a) + np.abs(b) + np.abs(d)) + d * d
        ref["loss"].append(L)
        ref["loss_b"].append((per.sum(), (d * d).sum(), N, L))
        gr = np.zeros(case["store"][j].shape[:3] + (MSE_C[j],), f64)
        gr[..., :18] = k * w * d
        ref["grad"].append(gr)
        ta, tb = np.zeros_like(gr), np.zeros_like(gr)
        ta[..., :18] = np.abs(k * w) * (np.abs(a) + np.abs(b))      # roundings of a and b
        tb[..., :18] = np.abs(k * w * d)                             # a - b, k (cast of N, division), k * w, the product
        ref["grad_terms"].append([(2, ta), (5, tb)])
    ref["total"] = sum(ref["loss"])
    p4 = case["store"][4][..., :18]
    ref["max"], ref["min"] = p4.max(), p4.min()
    return ref


def mse_loss_bound(per_sum, sq_sum, N, L, levels):
    return SQ * U * (per_sum + levels * sq_sum) / N + U * abs(L)


def check_mse_out(tag, out8, ref, levels, route=""):
    out8 = np.asarray(out8, dtype=f64).reshape(-1)
    bs = [mse_loss_bound(*b, levels=levels) for b in ref["loss_b"]]
    w = chk(tag + " five level losses", out8[:5], np.array(ref["loss"]), [], extra_abs=np.array(bs), route=route, names="j")
    # total: four fp32 additions of the five stored losses
    w = max(w, chk(tag + " total", out8[5], ref["total"], [(4, sum(abs(x) for x in ref["loss"]))], extra_abs=sum(bs), route=route))
    same(tag + " max / min over channels < 18 of the final prediction", out8[6:8].astype(f32), np.array([ref["max"], ref["min"]], f32), route)
    assert out8[6] < PLANT_LIVE and out8[7] > -PLANT_LIVE
    return w


def check_mse_grads(tag, grads, ref, need, route=""):
    w = 0.0
    for j in range(5):
        if not need[j]:
            assert grads[j] is None, "%s: level %d was not needed but got a gradient" % (tag, j)
            continue
        g = np.asarray(grads[j], dtype=f64)
        w = max(w, chk("%s d/d pred %d" % (tag, j), g, ref["grad"][j], ref["grad_terms"][j], route=route, names="bhwc"))
        if g.shape[-1] > 18:
            assert (g[..., 18:] == 0).all(), "%s: channel 18 of level %d's gradient is not exactly 0" % (tag, j)
    return w


# ------------------------------------------------------------------------------------------------ one-pass mse_train_kernel
TRAIN_CASES = {"1x8x8 one cell": (1, 8, 8), "1x24x24 nine cells": (1, 24, 24), "2x16x40": (2, 16, 40)}
TRAIN_GS = 0.6


def train_case(name):
    B, H, W = TRAIN_CASES[name]
    r = rng(B * 1000 + H * 10 + W)
    lv = []
    for s, C in ((0, 19), (1, 19), (2, 19), (3, 19), (0, 18)):
        x = np.zeros((B, H >> s, W >> s, 32), f32)
        x[..., :C] = r.standard_normal((B, H >> s, W >> s, C)).astype(f32)
        lv.append(x)
    lv[4][..., 18] = f32(PLANT)
    lv[2][0, 0, 0, 0] = f32(PLANT_LIVE)
    lv[0][..., 18] = f32(-PLANT)
    heat = r.random_sample((B, 18, H, W)).astype(f32)
    w = (r.random_sample((B, 18, H, W)) * (r.random_sample((B, 18, H, W)) > 0.1)).astype(f32)
    return dict(name=name, B=B, H=H, W=W, lv=lv, heat=heat, w=w, gs=f32(TRAIN_GS))


def upsample(x, s):
    """[B,h,w,C] -> [B,h<<s,w<<s,C]: full-resolution pixel (y, x) reads (y >> s, x >> s) (posenet.py:243-257, nearest)."""
    return x.repeat(1 << s, axis=1).repeat(1 << s, axis=2) if s else x


def sum_cells(x, s):
    if not s:
        return x
    B, H, W, C = x.shape
    f = 1 << s
    return x.reshape(B, H // f, f, W // f, f, C).sum((2, 4))


def train_as_mse(case):
    """The same operands as a five-prediction full-resolution MSE case (the levels up-sampled by indexing)."""
    shifts = (0, 1, 2, 3, 0)
    store = [upsample(x, s) for x, s in zip(case["lv"], shifts)]
    return dict(B=case["B"], H=case["H"], W=case["W"], store=store, gs=case["gs"],
                gt=np.ascontiguousarray(case["heat"].transpose(0, 2, 3, 1)), w=np.ascontiguousarray(case["w"].transpose(0, 2, 3, 1)))


def train_ref(case):
    ref = mse_ref(train_as_mse(case))
    ref["cgrad"], ref["cgrad_terms"] = [], []
    for j, s in enumerate((0, 1, 2, 3, 0)):
        g = ref["grad"][j][..., :18]
        n = 4 ** s
        # sum over the 4^s children: every child's own bound, plus n - 1 additions on sum |child|
        ta, tb = [sum_cells(t[..., :18], s) for _, t in ref["grad_terms"][j]]
        ref["cgrad"].append(sum_cells(g, s))
        ref["cgrad_terms"].append([(2, ta), (5, tb), (n - 1, sum_cells(np.abs(g), s))])
    return ref


def check_train(tag, out8, grads, ref, dtype, route=""):
    """grads: five [B,h,w,32] arrays (as float64 of the stored type)."""
    w = check_mse_out(tag, out8, ref, MSE_TRAIN_LEVELS, route)
    for j in range(5):
        g = np.asarray(grads[j], dtype=f64)
        assert g.shape[-1] == 32
        w = max(w, chk("%s level %d gradient (%d children)" % (tag, j, 4 ** (0, 1, 2, 3, 0)[j]), g[..., :18], ref["cgrad"][j],
                       ref["cgrad_terms"][j], out_dtype=dtype, route=route, names="bhwc"))
        assert (g[..., 18:] == 0).all(), "%s: lanes 18..31 of level %d's gradient are not exactly 0" % (tag, j)
    return w


# ====================================================================================================== focal loss
FOCAL_GS = (f32(1.7), f32(0.3))
EDGE_P = [LO, HI, np.nextafter(LO, f32(0)), np.nextafter(HI, f32(2)), f32(0), f32(1)]
FOCAL_A = (1, 255, 256, 257, 600)
FOCAL_K = (1, 2, 3, 5, 80)
FOCAL_MAXN = (1, 3, 8)


def iou_matrix(anc, ann, ft):
    """losses.py:5-22 in the dtype ft: [A, N]."""
    a, g = anc.astype(ft), ann[:, :4].astype(ft)
    area_a = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    area_b = (g[:, 2] - g[:, 0]) * (g[:, 3] - g[:, 1])
    iw = np.minimum(a[:, None, 2], g[None, :, 2]) - np.maximum(a[:, None, 0], g[None, :, 0])
    ih = np.minimum(a[:, None, 3], g[None, :, 3]) - np.maximum(a[:, None, 1], g[None, :, 1])
    iw, ih = np.maximum(iw, ft(0)), np.maximum(ih, ft(0))
    inter = iw * ih
    ua = np.maximum(area_a[:, None] + area_b[None, :] - inter, ft(UA_MIN))
    return inter / ua


def assign(anc, ann, ft, mut=None):
    """assign_anchor: (iou_max, arg, second-best IoU) per anchor; the first maximum wins (losses.py:59).  ft = float32 is the mirror
    of the kernel's operations (bit-exact on the grid family), ft = float64 the reference of the real-anchor family."""
    iou = iou_matrix(anc, ann, ft)
    A = anc.shape[0]
    best, arg, second = np.full(A, -1.0, ft), np.full(A, -1, np.int64), np.full(A, -1.0, ft)
    for n in range(ann.shape[0]):
        if ann[n, 4] == -1:
            continue
        v = iou[:, n]
        better = v >= best if mut == "last maximum wins" else v > best
        second = np.where(better, best, np.maximum(second, v))
        best, arg = np.where(better, v, best), np.where(better, n, arg)
    return best, arg, second


def focal_state(case, mut=None):
    """Per image: state [A] (-1 ignored, -2 negative, >= 0 the class, K for a class outside [0, K)), arg [A], nvalid, nbad."""
    K = case["cls"].shape[2]
    ft = f32 if case["family"] == "grid" else f64
    out = []
    for b in range(case["cls"].shape[0]):
        ann = case["anno"][b]
        valid = ann[:, 4] != -1
        cid = np.trunc(ann[:, 4])
        cid = np.where((cid >= 0) & (cid < K), cid, K).astype(np.int64)
        nvalid, nbad = int(valid.sum()), int((valid & (cid == K)).sum())
        A = case["anchors"].shape[0]
        st, arg = np.full(A, -1, np.int64), np.zeros(A, np.int64)
        if nvalid:
            best, arg, _ = assign(case["anchors"], ann, ft, mut)
            pos = best > ft(T05) if mut == "> at 0.5" else best >= ft(T05)
            neg = best <= ft(T04) if mut == "<= at 0.4" else best < ft(T04)
            st = np.where(pos, cid[np.maximum(arg, 0)], np.where(neg, -2, -1))
        out.append((st, np.maximum(arg, 0), nvalid, nbad))
    return out


def undecided(case):
    """Real-anchor family: anchors whose float64 assignment the kernel's fp32 one might not share."""
    n = 0
    for b in range(case["cls"].shape[0]):
        ann = case["anno"][b]
        if not (ann[:, 4] != -1).any():
            continue
        best, _, second = assign(case["anchors"], ann, f64)
        n += int(((np.abs(best - 0.4) < 1e-6) | (np.abs(best - 0.5) < 1e-6) | ((best != second) & (best - second < 1e-6))).sum())
    return n


def reg_targets(anc, g, ft, mut=None):
    """losses.py:97-121: targets [.., 4] and the bound of their fp32 evaluation (float64 only)."""
    a = anc.astype(ft)
    g = g.astype(ft)
    half = ft(0.5)
    aw, ah = a[..., 2] - a[..., 0], a[..., 3] - a[..., 1]
    acx, acy = a[..., 0] + half * aw, a[..., 1] + half * ah
    gw, gh = g[..., 2] - g[..., 0], g[..., 3] - g[..., 1]
    if mut == "gw clamped before the centre":
        gw, gh = np.maximum(gw, ft(1)), np.maximum(gh, ft(1))
    gcx, gcy = g[..., 0] + half * gw, g[..., 1] + half * gh
    gwc, ghc = np.maximum(gw, ft(1)), np.maximum(gh, ft(1))
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.stack([((gcx - acx) / aw) / ft(C01), ((gcy - acy) / ah) / ft(C01), np.log(gwc / aw) / ft(C02), np.log(ghc / ah) / ft(C02)], -1)
        if ft is not f64:
            return t, None
        # centres: a.x + 0.5 aw with aw rounded, likewise the box; their difference, two divisions
        dx = (0.5 * np.abs(gw) + np.abs(gcx) + 0.5 * np.abs(aw) + np.abs(acx) + np.abs(gcx - acx)) / np.abs(aw) / f64(C01)
        dy = (0.5 * np.abs(gh) + np.abs(gcy) + 0.5 * np.abs(ah) + np.abs(acy) + np.abs(gcy - acy)) / np.abs(ah) / f64(C01)
        # gw / aw carries 3 roundings into the logarithm's argument; logf; the division by 0.2f
        dw = np.full_like(dx, 3.0 / f64(C02))
        bt = U * (np.stack([dx, dy, dw, dw], -1) + np.array([3, 3, R_LOG + 1, R_LOG + 1]) * np.abs(t))
    return t, bt


def focal_eval(case, ft=f64, mut=None, fsum=None, contract=False):
    """The focal loss and its gradients in the dtype ft (float64: the reference, with bounds; float32: the arithmetic model).
    mut: a modelled fault.  fsum(x): the summation used for the per-image sums (model tier)."""
    cls, reg = case["cls"], case["reg"]
    B, A, K = cls.shape
    fsum = fsum or (lambda x: x.sum(dtype=ft))
    g2 = case.get("gs", FOCAL_GS)
    gs, gsr = [ft(v) for v in (g2[::-1] if mut == "upstream gradients swapped" else g2)]
    states = focal_state(case, mut)
    ref = ft is f64
    per_img, bad = np.zeros((B, 4), f64), np.zeros(B, f64)
    per_b = np.zeros((B, 2), f64)
    dcls, dreg = np.zeros((B, A, K), ft), np.zeros((B, A, 4), ft)
    dcls_t = [np.zeros((B, A, K)) for _ in range(2)]
    dreg_t = [np.zeros((B, A, 4)) for _ in range(2)]
    cols = np.arange(K)[None, :]
    # K > 1: a lane of stream_rows adds its head element, ceil(quads / 256) float4s and its tail element before the block tree
    lane_terms = 1 if K == 1 else 4 * -(-(-(-(min(A, FMC_TILE) * K) // 4)) // 256) + 2
    pb = {}
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for b in range(B):
            st, arg, nvalid, nbad = states[b]
            bad[b] = nbad
            per_img[b, 3] = nvalid
            if nvalid == 0 and mut != "empty image contributes":
                continue
            if nvalid == 0:
                st = np.full(A, -2, np.int64)
            praw = cls[b].astype(ft)
            p = np.clip(praw, ft(LO), ft(HI))
            inr = np.ones_like(praw, bool) if mut == "clamp passes gradient outside" else (praw >= ft(LO)) & (praw <= ft(HI))
            live = (st != -1)[:, None] & np.ones((1, K), bool)
            pcol = st
            if mut == "positive column off by one across a row seam" and K > 1:
                pcol = np.where(st >= 0, (st + 1) % K, st)
            posm = live & (pcol[:, None] == cols)
            negm = live & ~posm
            om, lp, lq = ft(1) - p, np.log(p), np.log(ft(1) - p)
            al, be = (ft(0.75), ft(0.25)) if mut == "alpha exchanged" else (ft(0.25), ft(0.75))
            cl = np.where(posm, al * om * om * -lp, np.where(negm, be * p * p * -lq, ft(0)))
            if mut == "head element skipped" and K > 1 and b > 0 and ((b * A * K) % 4):
                cl = cl.copy()
                cl.reshape(-1)[0] = 0
            pos = st >= 0
            npos = int(pos.sum())
            t, bt = reg_targets(case["anchors"], case["anno"][b][arg][:, :4], ft, mut)
            r = reg[b].astype(ft)
            d = np.abs(t - r)
            quad = d <= ft(NINTH)
            rl = np.where(pos[:, None], np.where(quad, ft(4.5) * d * d, d - ft(HALF9)), ft(0))
            csum, rsum = fsum(cl), fsum(rl)
            per_img[b, :3] = csum, rsum, npos
            nd = npos if mut == "npos not clamped" else max(npos, 1)
            lc = f64(f32(csum)) / nd if ft is f32 else csum / nd
            lr = 0.0
            if npos > 0:
                lr = (f64(f32(rsum)) if ft is f32 else rsum) / ((1.0 if mut == "factor 4 missing" else 4.0) * npos)
            per_b[b] = lc, lr
            # gradients
            kc = gs / (ft(B) * ft(nd))
            if contract:                    # the sums of the brackets as fused multiply-adds
                gp = kc * al * (f64(ft(2) * om) * f64(lp) - f64(om * om / p)).astype(ft)
                gn = kc * be * (f64(ft(-2) * p) * f64(lq) + f64(p * p / (ft(1) - p))).astype(ft)
            else:
                gp = kc * al * (ft(2) * om * lp - om * om / p)
                gn = kc * be * (ft(-2) * p * lq + p * p / (ft(1) - p))
            dcls[b] = np.where(inr, np.where(posm, gp, np.where(negm, gn, ft(0))), ft(0))
            kr = gsr / (ft(B) * ft(4) * ft(npos)) if npos else ft(0)
            e = r - t
            dr = kr * np.where(np.abs(e) <= ft(NINTH), ft(9) * e, np.sign(e))
            dreg[b] = np.where(pos[:, None], dr, ft(0))
            if not ref or mut:
                continue
            assert not np.isnan(np.where(pos[:, None], t, 0)).any()
            # ---- bounds (float64 reference only)
            qa = np.where(p < 0.5, 2.0 ** -25 / (1 - p), 0.0)                  # the rounding of 1 - p, carried into logf(1 - p)
            # positive: 1 - p (twice), two products, logf.  negative: 0.75 p, p, the product with the logarithm, logf, + the absolute term
            cb = U * np.where(posm, (4 + R_LOG) * np.abs(cl), np.where(negm, (3 + R_LOG) * np.abs(cl), 0)) + np.where(negm, 0.75 * p * p * qa, 0)
            bt = np.where(pos[:, None], bt, 0)
            # |t - r|: delta t + u d; quadratic branch 4.5 d^2: 9 d delta d + 2 roundings; linear: delta d + 1 rounding
            dd = bt + U * d
            rb = np.where(pos[:, None], np.where(quad, 9 * d * dd + 2 * U * rl, dd + U * np.abs(rl)), 0)
            per_img_b = (cb.sum() + (lane_terms + BLOCK_LEVELS) * U * np.abs(cl).sum() + U * abs(csum),
                         rb.sum() + (4 + BLOCK_LEVELS) * U * np.abs(rl).sum() + U * abs(rsum))
            pb[b] = per_img_b
            # dcls.  kc: one division.  positive: 2 om logf(p) [om, product, logf] and om^2 / p [om twice, product, division] have the
            # same sign; kc * 0.25, the product: <= (3 + R_LOG) + 3 roundings on the sum of magnitudes.  negative: the same count plus
            # 0.75 (not a power of two) and the absolute term through 2 p logf(1 - p); p^2 / (1 - p) carries the rounding of 1 - p.
            T1p, T2p = np.abs(2 * om * lp), om * om / p
            T1n, T2n = np.abs(2 * p * lq), p * p / (1 - p)
            mp, mn = np.abs(kc) * 0.25 * (T1p + T2p), np.abs(kc) * 0.75 * (T1n + T2n)
            dcls_t[0][b] = np.where(inr, np.where(posm, (6 + R_LOG) * mp, np.where(negm, (7 + R_LOG) * mn, 0)), 0)
            dcls_t[1][b] = np.where(inr & negm, np.abs(kc) * 0.75 * 2 * p * qa, 0)
            # dreg.  quadratic: kr * 9 * (r - t): |kr| 9 (delta t + u |e|), kr, two products.  linear: kr alone.
            qe = np.abs(e) <= f64(NINTH)
            dreg_t[0][b] = np.where(pos[:, None], np.where(qe, 4, 1) * np.abs(dr), 0)
            dreg_t[1][b] = np.where(pos[:, None] & qe, np.abs(kr) * 9 * bt, 0)
    valid = per_img[:, 3] > 0 if mut != "empty image contributes" else np.ones(B, bool)
    out = np.array([per_b[valid, 0].sum() / B, per_b[valid, 1].sum() / B])
    res = dict(out=out, per_img=per_img, bad=bad, dcls=dcls, dreg=dreg, states=states)
    if ref and not mut:
        pib = np.zeros((B, 2))
        ob = np.zeros(2)
        for b, (c_b, r_b) in pb.items():
            pib[b] = c_b, r_b
            n = max(per_img[b, 2], 1)
            # (float) sum, the division, in double after that
            ob[0] += (c_b + 2 * U * abs(per_img[b, 0])) / n / B
            if per_img[b, 2] > 0:
                ob[1] += (r_b + 2 * U * abs(per_img[b, 1])) / (4 * n) / B
        res.update(per_img_b=pib, out_b=ob + U * np.abs(out), dcls_t=dcls_t, dreg_t=dreg_t)
    return res


def check_focal(tag, got, ref, route=""):
    """got: dict(out [2], per_img [B,4], bad [B] or None, dcls [B,A,K], dreg [B,A,4])."""
    K = ref["dcls"].shape[2]
    w = chk(tag + " cls / reg loss", got["out"], ref["out"], [], extra_abs=ref["out_b"], route=route, names="j")
    pi = np.asarray(got["per_img"], dtype=f64)
    w = max(w, chk(tag + " per_img sums", pi[:, :2], ref["per_img"][:, :2], [], extra_abs=ref["per_img_b"], route=route, names="bj"))
    same(tag + " npos, nvalid", pi[:, 2:], ref["per_img"][:, 2:], route)
    if K > 1:
        same(tag + " bad", got["bad"], ref["bad"], route)
    w = max(w, chk(tag + " dcls", got["dcls"], ref["dcls"], [(1, ref["dcls_t"][0])], extra_abs=ref["dcls_t"][1], route=route, names="bak"))
    w = max(w, chk(tag + " dreg", got["dreg"], ref["dreg"], [(1, ref["dreg_t"][0])], extra_abs=ref["dreg_t"][1], route=route, names="bak"))
    assert np.isfinite(np.asarray(got["dreg"], dtype=f64)).all() and np.isfinite(np.asarray(got["dcls"], dtype=f64)).all()
    return w


# ------------------------------------------------------------------------------------------------ focal generators
def _q(x):
    return np.round(np.asarray(x, dtype=f64) * 4) / 4


def _anno_rows(boxes, maxN, r, K, spread):
    """maxN rows with the boxes placed in order, -1 rows between them where there is room (not only at the end)."""
    rows = np.full((maxN, 5), -1.0, f32)
    n = min(len(boxes), maxN if maxN < 3 else maxN - (1 if maxN == 3 else 2))
    slots = list(range(maxN))
    if maxN >= 3:
        slots.remove(1)                 # a -1 row between valid ones
    if maxN >= 8:
        slots.remove(5)
    for i in range(n):
        rows[slots[i], :4] = boxes[i]
        rows[slots[i], 4] = (i * 2 + spread) % K
    return rows


def focal_case(family, A, K, maxN, B=4, seed=0):
    """Image 0 carries the planted boxes, image 1 generic ones, image 2 (the middle of the batch) no valid annotation, image 3
    annotations that no anchor reaches (npos = 0); further images cycle through the four kinds."""
    r = rng(seed * 7919 + A * 131 + K * 17 + maxN)
    if family == "grid":
        s = 4.0 * r.randint(2, 9)
        x, y = _q(r.uniform(130, 180)), _q(r.uniform(130, 180))    # the planted square: clear of the free anchors and boxes
        g0, g1 = [x, y, x + s, y + s / 2], [x, y + s / 2, x + s, y + s]          # halves of the square S: both IoU 1/2 with it
        thin = [230.0, 100.0, 230.5, 120.0]
        planted = [[x, y, x + s, y + s],            # IoU exactly 1/2 (a tie where g1 is present): positive, the first wins
                   [x, y, x + s, y + 1.25 * s],     # IoU exactly 2/5: ignored
                   g0, thin,                        # IoU 1
                   [236.0, 200.0, 252.0, 232.0], [240.0, 0.0, 250.0, 30.0]]     # IoU 0
        lo = _q(np.stack([r.uniform(0, 80, A), r.uniform(0, 80, A)], 1))
        anc = np.concatenate([lo, lo + _q(r.uniform(4, 40, (A, 2)))], 1)
        def extra():                        # a copy of an anchor (IoU 1) or a free box
            if r.rand() < 0.5:
                return list(anc[r.randint(0, A)])
            c = _q(r.uniform(0, 80, 2))
            return list(np.concatenate([c, c + _q(r.uniform(2, 40, 2))]))
        far = [250.0, 250.0, 250.25, 250.25]
    else:
        from oracle.posenet_oracle import anchors_for_image
        allanc = anchors_for_image(64, 64)[0]
        anc = allanc[np.linspace(0, len(allanc) - 1, A).astype(np.int64)].astype(f64) if A > 1 else allanc[40:41].astype(f64)
        pick = lambda: anc[r.randint(0, A)]
        jit = lambda a: a + r.uniform(-0.04, 0.04, 4) * (a[2] - a[0])
        a0, a1 = pick(), pick()
        g0 = jit(a0)
        g1 = jit(a1)
        thin = [a0[0], a0[1], a0[0] + 0.6, a0[3]]
        planted = []
        extra = lambda: jit(pick()) if r.rand() < 0.5 else [a1[0], a1[1], a1[0] + 0.45 * (a1[2] - a1[0]), a1[3]]
        far = [300.0, 300.0, 300.3, 300.2]
    kinds = []
    img0 = [g0, g1, g0, thin] + [extra() for _ in range(4)]                  # g0 again: a duplicate annotation
    anno = np.zeros((B, maxN, 5), f32)
    for b in range(B):
        kind = b % 4
        if kind == 0:
            anno[b] = _anno_rows(img0, maxN, r, K, 0)
        elif kind == 1:
            anno[b] = _anno_rows([extra() for _ in range(8)], maxN, r, K, 1)
            if K > 1 and maxN == 8:
                anno[b, 0, 4] = K + 2                                            # a class id outside [0, K)
        elif kind == 2:
            anno[b] = -1.0
        else:
            anno[b] = _anno_rows([far], maxN, r, K, 0)
        kinds.append(kind)
    if B == 2:
        anno[1] = _anno_rows([extra() for _ in range(8)], maxN, r, K, 1)
    anc = np.asarray(anc, f64)
    used, planted_at = set(), []
    for i, pl in enumerate(planted):                                             # spread over the anchor range, block seams included
        at = (0, A // 2, A - 1, 255, 256, A // 3)[i]
        if i and A <= 6:
            break
        at = at if at < A else i
        while at in used:
            at = (at + 1) % A
        used.add(at)
        anc[at] = pl
        planted_at.append(at)
    u = r.random_sample((B, A, K))
    kind_p = r.randint(0, 10, (B, A, K))
    p = np.where(kind_p < 6, 2e-4 + u * (1 - 4e-4), np.where(kind_p < 8, 2e-4 * 10 ** (2 * u), np.where(kind_p < 9, 1e-6 + u * 5e-5, 1 - 1e-6 - u * 5e-5)))
    case = dict(family=family, A=A, K=K, maxN=maxN, B=B, anchors=anc.astype(f32), anno=anno, cls=p.astype(f32),
                reg=np.zeros((B, A, 4), f32), planted_at=planted_at)
    # regressions: on positives both branches of the smooth-L1 and both signs, clear of the switch; generic elsewhere
    reg = (0.5 * r.standard_normal((B, A, 4))).astype(f32)
    states = focal_state(case)
    deltas = np.array([0.03, -0.07, 0.5, -1.3, 0.1, -0.1105, 0.0])
    edges = {"pos": [], "neg": []}
    for b in range(B):
        st, arg, nvalid, _ = states[b]
        if not nvalid:
            continue
        t, _ = reg_targets(case["anchors"], anno[b][arg][:, :4], f64)
        pos = np.nonzero(st >= 0)[0]
        for i, a in enumerate(pos):
            reg[b, a] = (t[a] + deltas[(i + np.arange(4)) % len(deltas)]).astype(f32)
        for a in range(A):
            for k in range(K):
                if st[a] == k:
                    edges["pos"].append((b, a, k))
                elif st[a] != -1:
                    edges["neg"].append((b, a, k))
    case["reg"] = reg
    case["planted_edges"] = 0
    for key in ("pos", "neg"):                                                   # the clamp edges on elements that count
        el = edges[key]
        step = max(1, len(el) // 6)
        for i, v in enumerate(EDGE_P):
            if i * step < len(el):
                case["cls"][el[i * step]] = v
                case["planted_edges"] += 1
    case["cls"][case["cls"] != case["cls"]] = 0.5
    check_focal_conditions(case)
    return case


def check_focal_conditions(case):
    """The generator conditions, on the reference alone."""
    A, K = case["A"], case["K"]
    if case["family"] == "grid":
        for arr in (case["anchors"], case["anno"][..., :4][case["anno"][..., 4] != -1]):
            assert (arr * 4 == np.round(arr * 4)).all() and arr.min() >= 0 and arr.max() <= 256, "grid family: a coordinate is off the grid"
    else:
        assert undecided(case) == 0, "real-anchor family: %d undecided anchor(s); choose another seed" % undecided(case)
    p = case["cls"].astype(f64)
    generic = ~np.isin(case["cls"], np.array(EDGE_P, f32))
    assert (np.abs(p[generic] - f64(LO)) >= 1e-6).all() and (np.abs(p[generic] - f64(HI)) >= 1e-6).all()
    for b, (st, arg, nvalid, _) in enumerate(focal_state(case)):
        if not nvalid:
            continue
        t, _ = reg_targets(case["anchors"], case["anno"][b][arg][:, :4], f64)
        d = np.abs(t - case["reg"][b].astype(f64))[st >= 0]
        assert (np.abs(d - f64(NINTH)) > 1e-4).all(), "a positive sits on the smooth-L1 switch"


FOCAL_SEEDS = {}        # (family, A, K, maxN, B) -> seed, where the default 0 leaves an undecided anchor


def focal_cases():
    """(family, A, K, maxN, B): K x A with maxN rotating so that every maxN meets every K and every A, plus the two batch shapes."""
    out = []
    for fam in ("grid", "real"):
        for i, K in enumerate(FOCAL_K):
            for j, A in enumerate(FOCAL_A):
                out.append((fam, A, K, FOCAL_MAXN[(i + j) % 3], 4))
        out.append((fam, 257, 3, 3, 2))             # the second image's slice starts 12 bytes into a 16-byte group: head = 1
        out.append((fam, 64, 1, 3, 257))            # the finalize's loop over images wraps
        out.append((fam, 64, 3, 8, 257))
    return out


def make_focal(key):
    fam, A, K, maxN, B = key
    return focal_case(fam, A, K, maxN, B, FOCAL_SEEDS.get(key, 0))


def focal_tag(key):
    return "focal %s A=%d K=%d maxN=%d B=%d" % key


# ====================================================================================================== sigmoid
SIG_N = (1, 255, 257)


def sigmoid_case(n):
    r = rng(n)
    x = r.uniform(-100, 100, n).astype(f32)
    sp = np.array([-100, 100, -88.5, -89, 88.5, 0, -20, 20, 1e-3, -99.5], f32)
    x[: min(n, len(sp))] = sp[:n] if n < len(sp) else sp
    if n == 1:
        x[0] = -100.0                   # expf(100) overflows
    return x, r.standard_normal(n).astype(f32), r.random_sample(n).astype(f32)


def check_sigmoid(tag, y, x, route=""):
    x = x.astype(f64)
    with np.errstate(over="ignore"):
        e = np.exp(-x)
        ref = 1.0 / (1.0 + e)
    # expf, the addition, the division; a result below 2^-126 may be flushed
    return chk(tag, y, ref, [(R_EXP + 2, ref)], extra_abs=TINY, route=route)


def check_sigmoid_bwd(tag, dl, dp, p, route=""):
    dp, p = dp.astype(f64), p.astype(f64)
    ref = dp * p * (1 - p)
    return chk(tag, dl, ref, [(3, ref)], route=route)


# ====================================================================================================== PRN softmax
SM_COLS = (1, 17, 255, 256, 257, 1000)
SM_ROWS = 3


def softmax_case(cols, padded):
    """a [3, a_stride] (row 1 negative everywhere, row 2 spread over +-30), res [3, cols], dp, pre with exact zeros."""
    r = rng(cols * 2 + padded)
    stride = round_up(cols, 32) if padded else cols
    a = np.full((SM_ROWS, stride), 777.0, f32)                                  # pad lanes hold a value that would win the maximum
    a[:, :cols] = r.standard_normal((SM_ROWS, cols)).astype(f32) * 2
    a[1, :cols] = -50 * np.abs(a[1, :cols]) - f32(100)                          # negative everywhere, far below the ReLU
    a[2, :cols] = r.uniform(-30, 30, cols).astype(f32)
    res = r.standard_normal((SM_ROWS, cols)).astype(f32)
    res[2] = r.uniform(-30, 30, cols).astype(f32)
    dp = r.standard_normal((SM_ROWS, cols)).astype(f32)
    pre = np.full((SM_ROWS, stride), 1.0, f32)
    pre[:, :cols] = r.standard_normal((SM_ROWS, cols)).astype(f32)
    pre[:, 0:cols:5] = 0.0                                                      # exactly 0: masked (the test is a strict >)
    return dict(cols=cols, stride=stride, a=a, res=res, dp=dp, pre=pre)


def softmax_ref(a, res, cols, relu):
    A = a[:, :cols].astype(f64)
    ra = np.maximum(A, 0) if relu else A
    t = ra + res.astype(f64)
    mx = t.max(1, keepdims=True)
    arg = t - mx
    e = np.exp(arg)
    s = e.sum(1, keepdims=True)
    out = e / s
    darg = U * (np.abs(ra) + np.abs(res) + np.abs(mx) + np.abs(arg))           # relative to each exponential
    levels = -(-cols // 256) + BLOCK_LEVELS
    rel_s = (e * (darg + R_EXP * U)).sum(1, keepdims=True) / s + levels * U
    rel = darg + R_EXP * U + rel_s + 2 * U                                      # + 1 / s and the product
    return out, rel


def check_softmax(tag, got, a, res, cols, relu, route=""):
    ref, rel = softmax_ref(a, res, cols, relu)
    w = chk(tag, got, ref, [], extra_abs=rel * ref + TINY, route=route, names="rc")
    g = np.asarray(got, dtype=f64)
    w = max(w, chk(tag + " rows sum to 1", g.sum(1), np.ones(g.shape[0]), [], extra_abs=(rel * ref + TINY).sum(1), route=route, names="r"))
    return w


def check_softmax_bwd(tag, got, p, dp, pre, cols, route=""):
    """p: the f32 probabilities the kernel read; pre: [rows, pre_stride] or None."""
    p, dp = p.astype(f64), dp.astype(f64)
    dot = (p * dp).sum(1, keepdims=True)
    levels = -(-cols // 256) + BLOCK_LEVELS
    dot_b = (levels + 1) * U * np.abs(p * dp).sum(1, keepdims=True)
    g = p * (dp - dot)
    bound = np.abs(p) * dot_b + 2 * U * np.abs(p) * (np.abs(dp) + np.abs(dot)) + TINY       # an underflowed probability's product
    if pre is not None:
        m = pre[:, :cols] > 0
        g, bound = np.where(m, g, 0.0), np.where(m, bound, 0.0)
    return chk(tag, got, g, [], extra_abs=bound, route=route, names="rc")


# ====================================================================================================== BCE
BCE_N = (1, 4095, 4096, 4097, 256 * 4096 + 1)
BCE_GS = 1.3


def bce_case(n):
    r = rng(n % 9973)
    p = r.uniform(1e-3, 1 - 1e-3, n).astype(f32)
    y = (r.random_sample(n) > 0.5).astype(f32)
    soft = r.random_sample(n) < 0.3
    y[soft] = r.random_sample(int(soft.sum())).astype(f32)
    sp_p = np.array([0, 0, 1, 1, 1e-13, 1e-7, 1 - 2.0 ** -24, 0.5], f32)
    sp_y = np.array([0, 1, 0, 1, 0.25, 1, 0, 0.5], f32)
    if n >= 4095:
        p[-8:], y[-8:] = sp_p, sp_y                                             # the -100 clamp, in the last (partial) chunk
        p[:8], y[:8] = sp_p[::-1], sp_y[::-1]
    else:
        p[0], y[0] = 0.0, 1.0
    return p, y


def bce_ref(p, y, mut=None):
    p, y = p.astype(f64), y.astype(f64)
    n = p.size
    with np.errstate(divide="ignore"):
        lp, lq = np.log(p), np.log(1 - p)
    if mut != "no -100 clamp":
        lp, lq = np.maximum(lp, -100.0), np.maximum(lq, -100.0)
    with np.errstate(invalid="ignore"):
        t1, t2 = np.where(y == 0, 0.0, y * lp), np.where(y == 1, 0.0, (1 - y) * lq)
    term = -(t1 + t2)
    L = term.sum() / (-(-n // 4096) if mut == "divided by the chunk count" else n)
    qa = np.where((p < 0.5) & (lq > -100), 2.0 ** -25 / np.maximum(1 - p, 1e-300), 0.0)
    # logf (each), 1 - y, two products, the sum: <= (R_LOG + 3) roundings on |y lp| + |(1 - y) lq|; the absolute term on lq
    per = (R_LOG + 3) * U * (np.abs(t1) + np.abs(t2)) + np.abs(1 - y) * qa
    bound = (per.sum() + BCE_LEVELS * U * np.abs(term).sum()) / n + U * abs(L)
    return L, bound


def bce_bwd_ref(p, y, gs):
    p, y = p.astype(f64), y.astype(f64)
    den = np.maximum(p * (1 - p), f64(BCE_EPS))
    ref = f64(f32(gs)) / p.size * (p - y) / den
    # gs / n, p - y, 1 - p, p (1 - p), the product, the division
    return ref, [(6, ref)]


# ====================================================================================================== dropout
M64 = (1 << 64) - 1
DROP_N = (1, 255, 257, 5000)
DROP_P = (0.0, 0.5, 0.9)


def mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def dropout_keep(n, seed, p):
    """keep[i]: (float)(h >> 40) * 2^-24 >= p with h = mix64(mix64(seed) ^ i); both sides exact in Python floats."""
    ms = mix64(seed & M64)
    pf = float(f32(p))
    return np.array([(mix64(ms ^ i) >> 40) * 2.0 ** -24 >= pf for i in range(n)], bool)


def dropout_ref(x, seed, p):
    """x: torch tensor of the storage type (CPU).  Survivors are round_to_dtype(float32(x) * float32(1 / (1 - p)))."""
    keep = torch.from_numpy(dropout_keep(x.numel(), seed, p))
    scale = f32(1) / (f32(1) - f32(p))
    y = (x.float() * torch.tensor(scale, dtype=F32)).to(x.dtype)
    return torch.where(keep, y, torch.zeros_like(y)), keep


# ====================================================================================================== step log
def step_log_ref(kp8, det2, before):
    """The fp32 additions written out; slots the call does not own keep `before`."""
    out = np.array(before, f32).copy()
    kt = dt = f32(0)
    if kp8 is not None:
        out[:8] = kp8
        kt = f32(kp8[5])
    if det2 is not None:
        dt = f32(det2[0]) + f32(det2[1])
        out[8], out[9], out[10] = dt, det2[0], det2[1]
    out[11] = kt + dt if (kp8 is not None and det2 is not None) else (kt if kp8 is not None else dt)
    return out
