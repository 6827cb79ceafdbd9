"""Launch-plan mirrors and float64 references of the streaming kernels (csrc/bn.hip, csrc/resample.hip), shared by
tests/test_stream_parity_gpu.py (which compares the kernels with them) and tests/test_stream_parity_cpu.py (which shows that the
bounds used there reject modelled faults).  Test-side only; plain torch on the CPU."""
import torch
import torch.nn.functional as F

from helpers import U24, check_elementwise, report

BF, H16, F32 = torch.bfloat16, torch.float16, torch.float32
U53 = 2.0 ** -53
BN_BLOCKS = 8192                    # bn.hip pick_iters: blocks per launch
EPS32 = float(torch.tensor(1e-5, dtype=F32))
MOM32 = float(torch.tensor(0.1, dtype=F32))


# ------------------------------------------------------------------------------------------------ launch plans (bn.hip)
def vec(dtype):
    return 4 if dtype == F32 else 8


def geo(Cs, dtype):
    """Geo<T>: (G, GB, lanes, grid.y)."""
    V = vec(dtype)
    G = Cs // V
    assert Cs % V == 0 and G > 0 and G & (G - 1) == 0, (Cs, dtype)
    GB = min(G, 256)
    return G, GB, 256 // GB, (1 if G <= 256 else G // 256)


def pick_iters(P, lanes):
    return max(1, min(32, P // (lanes * BN_BLOCKS)))


def reduce_chunk(P, lanes):
    c = max(4 * lanes, min(4096, P // 512))
    return (c + lanes - 1) // lanes * lanes


def plan(P, Cs, dtype):
    """(lanes, iters, grid.x of bn_act / bn_bwd_apply, grid.y, chunks of bn_bwd_reduce)."""
    _, _, lanes, gy = geo(Cs, dtype)
    it = pick_iters(P, lanes)
    ch = reduce_chunk(P, lanes)
    return lanes, it, (P + lanes * it - 1) // (lanes * it), gy, (P + ch - 1) // ch


def roundings(n):
    """check_elementwise arguments for `n` fp32 roundings on mag64 and no summation: K / k_step + k_step + extra_terms + 2 = n."""
    return dict(k_step=1, K=0, extra_terms=n - 3)


# ------------------------------------------------------------------------------------------------ BN references (float64)
def slice_sums(part):
    """[n, C, 2] f32 partials -> float64 (S1, S2, sum |s1|, sum |s2|) per channel."""
    p = part.double()
    return p[..., 0].sum(0), p[..., 1].sum(0), p[..., 0].abs().sum(0), p[..., 1].abs().sum(0)


def finalize_train_ref(part, count, eps=EPS32):
    """mean, var (clamped at 0), invstd in float64 and their fp64-noise allowances (n 2^-53 sum|partials| / count, carried through
    var = s2 / count - mu^2 relative to var + eps for invstd)."""
    n = part.shape[0]
    S1, S2, A1, A2 = slice_sums(part)
    mu = S1 / count
    var = (S2 / count - mu * mu).clamp(min=0.0)
    istd = 1.0 / torch.sqrt(var + eps)
    d_mu = (n + 2) * U53 * A1 / count
    d_var = (n + 4) * U53 * (A2 / count + 2 * mu.abs() * A1 / count + mu * mu)
    d_is = 0.5 * istd * d_var / (var + eps) + 4 * U53 * istd
    return mu, var, istd, d_mu, d_var, d_is


def unpack_mask(mask, dtype):
    """uint8 [P, Cs / V] sign bytes of bn_act -> bool [P, Cs]: bit k of byte g is channel g * V + k."""
    V = vec(dtype)
    m = mask.to(torch.int32)
    return torch.stack([(m >> k) & 1 for k in range(V)], -1).reshape(m.shape[0], -1).bool()


def pack_mask(pos, dtype, G=None):
    """bool [P, Cs] -> uint8 [P, G] in bn_act's layout (G defaults to Cs / V)."""
    V = vec(dtype)
    P, Cs = pos.shape
    G = Cs // V if G is None else G
    w = torch.tensor([1 << k for k in range(V)], dtype=torch.int32)
    return (pos.reshape(P, Cs // V, V).to(torch.int32) * w).sum(-1).to(torch.uint8).reshape(-1)[: P * G].reshape(P, G)


def chunk_sums(t, chunk):
    """[P, C] float64 -> [chunks, C] sums over each chunk's own pixel range (last chunk ragged)."""
    P, C = t.shape
    n = (P + chunk - 1) // chunk
    if n * chunk != P:
        t = torch.cat([t, torch.zeros(n * chunk - P, C, dtype=t.dtype)], 0)
    return t.reshape(n, chunk, C).sum(1)


# ------------------------------------------------------------------------------------------------ max-pool 3x3 / s2 / p1
def pool_taps(x_nchw):
    """[B, C, H, W] float64 -> ([B, C, 9, Ho * Wo] taps in window order r * 3 + s, out-of-range taps -inf, Ho, Wo)."""
    B, C, H, W = x_nchw.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xp = F.pad(x_nchw, (1, 1, 1, 1), value=float("-inf"))
    return F.unfold(xp, 3, stride=2).reshape(B, C, 9, Ho * Wo), Ho, Wo


def pool_first_max(x_nchw, last=False):
    """Window maximum and the window position r * 3 + s of its first (last=True: last) occurrence in scan order; and the share of
    windows whose maximum is tied.  No argmax: the position is 9 - max over the maximal taps of (9 - k)."""
    taps, Ho, Wo = pool_taps(x_nchw)
    B, C = taps.shape[:2]
    m = taps.amax(2, keepdim=True)
    eq = taps == m
    k = torch.arange(9).reshape(1, 1, 9, 1)
    idx = (eq * (k + 1)).amax(2) - 1 if last else 9 - (eq * (9 - k)).amax(2)
    tied = (eq.sum(2) > 1).double().mean().item()
    return m.reshape(B, C, Ho, Wo), idx.reshape(B, C, Ho, Wo), tied


def pool_scatter(dy_nchw, idx, H, W):
    """float64 scatter of dy by window position idx -> (dx, sum |dy| routed) [B, C, H, W]."""
    B, C, Ho, Wo = dy_nchw.shape
    hot = (idx.reshape(B, C, 1, Ho * Wo) == torch.arange(9).reshape(1, 1, 9, 1)).double()
    out = []
    for d in (dy_nchw, dy_nchw.abs()):
        cols = (hot * d.reshape(B, C, 1, Ho * Wo)).reshape(B, C * 9, Ho * Wo)
        out.append(F.fold(cols, (H + 2, W + 2), 3, stride=2)[:, :, 1:H + 1, 1:W + 1])
    return out


# ------------------------------------------------------------------------------------------------ nearest resampling
def nearest_map(n_out, n_src):
    """The kernels' integer rule: source index floor(o * n_src / n_out) of every output index."""
    return (torch.arange(n_out, dtype=torch.int64) * n_src) // n_out


def torch_nearest_map(n_out, n_src):
    """torch's CPU nearest rule, read off F.interpolate on an index ramp."""
    r = torch.arange(n_src, dtype=torch.float32).reshape(1, 1, n_src, 1)
    return F.interpolate(r, size=(n_out, 1), mode="nearest").reshape(-1).to(torch.int64)


def children(n_out, n_src, floor_rule=False):
    """Per source index the [lo, hi) range of outputs that read it: ceil_div(s * n_out, n_src) (floor_rule: the modelled fault)."""
    s = torch.arange(n_src + 1, dtype=torch.int64) * n_out
    e = s // n_src if floor_rule else (s + n_src - 1) // n_src
    return e[:-1], e[1:].clamp(max=n_out)


def gather_nearest(src, Ho, Wo):
    """[B, Hs, Ws, C] -> [B, Ho, Wo, C] by the integer rule."""
    return src[:, nearest_map(Ho, src.shape[1])][:, :, nearest_map(Wo, src.shape[2])]


def sum_children(fine, Hc, Wc):
    """[B, Hf, Wf, C] float64 -> [B, Hc, Wc, C] sums over each coarse pixel's children (the transpose of gather_nearest)."""
    B, Hf, Wf, C = fine.shape
    t = torch.zeros(B, Hc, Wf, C, dtype=fine.dtype).index_add_(1, nearest_map(Hf, Hc), fine)
    return torch.zeros(B, Hc, Wc, C, dtype=fine.dtype).index_add_(2, nearest_map(Wf, Wc), t)


def max_children(n_out, n_src):
    lo, hi = children(n_out, n_src)
    return int((hi - lo).max())


# ------------------------------------------------------------------------------------------------ the checks (bounds live here)
def check_rows(name, got, ref, mag, out_dtype, route="", names="pc", extra_abs=None, **kw):
    """check_elementwise over dim-0 pieces of at most 2^25 elements (the float64 temporaries of the largest cases stay small)."""
    n = got.shape[0]
    per = max(1, (1 << 25) // max(1, got[0].numel())) if got.dim() > 1 else n
    worst = 0.0
    for i in range(0, n, per):
        s = slice(i, min(n, i + per))
        tag = name if per >= n else "%s [%d:%d]" % (name, s.start, s.stop)
        worst = max(worst, check_elementwise(tag, got[s], ref[s], mag[s], out_dtype, route=route, names=names,
                                             extra_abs=None if extra_abs is None else extra_abs[s], **kw))
    return worst


def exact(name, got, ref, route=""):
    got, ref = got.cpu(), ref.cpu()
    ok = got.shape == ref.shape and torch.equal(got, ref)
    report("%-58s %-52s exact  %s" % (name, route, "OK" if ok else "FAIL"))
    if not ok:
        bad = torch.nonzero((got != ref) | (got != got)) if got.shape == ref.shape else None
        raise AssertionError("%s: not bit-equal to the reference; first differing index %s" % (
            name, None if bad is None or not len(bad) else (bad[0].tolist(), float(got[tuple(bad[0])]), float(ref[tuple(bad[0])]))))


def pad_zero(name, t, C):
    """Lanes [C, Cs) of a [..., Cs] tensor are exactly 0."""
    if C < t.shape[-1]:
        assert bool((t[..., C:].cpu() == 0).all()), "%s: pad lanes [%d, %d) are not all zero" % (name, C, t.shape[-1])


def check_finalize_train(tag, part, count, gamma, beta, rm0, rv0, got, route):
    """got: dict of the device's mean, invstd, scale, shift (and rm, rv when rm0 / rv0 are given).  scale, shift and running_mean are
    referenced from the device's own mean / invstd; running_var from the float64 variance with its noise allowance."""
    mu, var, istd, d_mu, d_var, d_is = finalize_train_ref(part, count)
    C = part.shape[1]
    gm = gamma.double() if gamma is not None else torch.ones(C, dtype=torch.float64)
    bt = beta.double() if beta is not None else torch.zeros(C, dtype=torch.float64)
    mean_d, is_d, sc_d = got["mean"].cpu().double(), got["invstd"].cpu().double(), got["scale"].cpu().double()
    m = MOM32
    w = [check_rows(tag + "mean", got["mean"], mu, mu.abs(), F32, route, "c", extra_abs=d_mu, **roundings(1)),
         check_rows(tag + "invstd", got["invstd"], istd, istd, F32, route, "c", extra_abs=d_is, **roundings(1)),
         check_rows(tag + "scale", got["scale"], gm * is_d, (gm * is_d).abs(), F32, route, "c", **roundings(1)),
         check_rows(tag + "shift", got["shift"], bt - mean_d * sc_d, bt.abs() + (mean_d * sc_d).abs(), F32, route, "c", **roundings(2))]
    if rm0 is not None:
        w.append(check_rows(tag + "running_mean", got["rm"], (1 - m) * rm0.double() + m * mean_d,
                            (1 - m) * rm0.double().abs() + m * mean_d.abs(), F32, route, "c", **roundings(4)))
    if rv0 is not None:
        f = count / (count - 1.0) if count > 1 else 1.0          # unbiased into running_var; count == 1 keeps the biased one
        w.append(check_rows(tag + "running_var", got["rv"], (1 - m) * rv0.double() + m * var * f, (1 - m) * rv0.double().abs() + m * var * f,
                            F32, route, "c", extra_abs=m * d_var * f, **roundings(5)))
    return max(w)


def bwd_coef_ref(part, count, gamma, mean, istd, k3_sign=-1.0):
    """float64 (S1, S2, k1, k2, k3, |k3| magnitude, noise1, noise2) from the partials.  k3_sign = +1 models the wrong sign on a."""
    n = part.shape[0]
    S1, S2, A1, A2 = slice_sums(part)
    n1, n2 = (n + 2) * U53 * A1, (n + 2) * U53 * A2
    gm, mu, is_ = gamma.double(), mean.double(), istd.double()
    a, b = S1 / count, S2 / count
    return (S1, S2, gm * is_, -gm * is_ * is_ * b, gm * is_ * (mu * is_ * b + k3_sign * a),
            (gm * is_).abs() * ((mu * is_ * b).abs() + a.abs()), n1, n2)


def check_bwd_finalize(tag, part, count, gamma, mean, istd, dg0, db0, train, dgamma, dbeta, coef, route):
    """coef None: a frozen finalize that returns no coefficient tensor (the conv epilogue's: k1 is the forward scale) — dgamma / dbeta only."""
    S1, S2, k1, k2, k3, k3mag, n1, n2 = bwd_coef_ref(part, count, gamma, mean, istd)
    gi = k1.abs()
    is_, mu = istd.double(), mean.double()
    w = [check_rows(tag + "dbeta", dbeta, db0.double() + S1, db0.double().abs() + S1.abs(), F32, route, "c", extra_abs=n1, **roundings(2)),
         check_rows(tag + "dgamma", dgamma, dg0.double() + S2, dg0.double().abs() + S2.abs(), F32, route, "c", extra_abs=n2, **roundings(2))]
    if coef is None:
        assert not train
        return max(w)
    w.append(check_rows(tag + "k1", coef[0], k1, k1.abs(), F32, route, "c", **roundings(1)))
    if train:
        w.append(check_rows(tag + "k2", coef[1], k2, k2.abs(), F32, route, "c", extra_abs=gi * is_ * n2 / count, **roundings(4)))
        w.append(check_rows(tag + "k3", coef[2], k3, k3mag, F32, route, "c", extra_abs=gi * ((mu * is_).abs() * n2 + n1) / count,
                            **roundings(7)))
    else:
        exact(tag + "k2 = k3 = 0", coef[1:], torch.zeros(2, part.shape[1]), route)
    return max(w)


def check_act(tag, z, y, sc, sf, res, relu, C, dtype, route):
    """z, y, res: [P, Cs] in the storage type; sc, sf: the device's f32 scale / shift.  Returns (worst ratio, float64 reference)."""
    yl = y[:, :C].double()
    sc, sf = sc.double(), sf.double()
    ref, mag = yl * sc + sf, (yl * sc).abs() + sf.abs()
    del yl
    if res is not None:
        r = res[:, :C].double()
        ref, mag = ref + r, mag + r.abs()
        del r
    if relu:
        ref = ref.clamp(min=0.0)
    w = check_rows(tag, z[:, :C], ref, mag, dtype, route, **roundings(3))
    pad_zero(tag, z, C)
    return w, ref


def check_mask(tag, mask, z, dtype, route):
    """The sign bytes [P][Cs / V] equal (stored z > 0) bit for bit."""
    assert tuple(mask.shape) == (z.shape[0], z.shape[1] // vec(dtype)), (tag, mask.shape)
    exact(tag + " sign bytes [P][Cs/V]", unpack_mask(mask.cpu(), dtype), z.cpu() > 0, route)


def relu_pos(mode, z, y, sc, sf, C):
    """(float64 0/1 ReLU mask over the live channels, ambiguity mask or None).  'z' / 'bits': the stored z > 0; 'remask': the float64
    sign of y * scale + shift, either sign accepted within 3 roundings of zero; 'none': no ReLU."""
    if mode == "none":
        return None, None
    if mode in ("z", "bits"):
        return (z[:, :C] > 0).double(), None
    yl, sc, sf = y[:, :C].double(), sc.double(), sf.double()
    x = yl * sc + sf
    amb = x.abs() <= 3 * U24 * ((yl * sc).abs() + sf.abs())
    return (x > 0).double(), amb.double()


def check_reduce(tag, part, dz, y, pos, amb, mean, istd, chunk, lanes, C, route):
    dzl = dz[:, :C].double()
    g = dzl if pos is None else dzl * pos
    mu, is_ = mean.double(), istd.double()
    yl = y[:, :C].double()
    xh, xa = (yl - mu) * is_, (yl.abs() + mu.abs()) * is_
    del yl
    K = (chunk + lanes - 1) // lanes + lanes
    e1 = e2 = None
    if amb is not None:
        e1, e2 = chunk_sums(dzl.abs() * amb, chunk), chunk_sums(dzl.abs() * amb * xa, chunk)
    w1 = check_rows(tag + "sum g", part[..., 0], chunk_sums(g, chunk), chunk_sums(g.abs(), chunk), F32, route, "nc",
                    extra_abs=e1, k_step=1, K=K)
    w2 = check_rows(tag + "sum g*xhat", part[..., 1], chunk_sums(g * xh, chunk), chunk_sums(g.abs() * xa, chunk), F32, route, "nc",
                    extra_abs=e2, k_step=1, K=K, extra_terms=3)
    return max(w1, w2)


def check_apply(tag, dy, dres, dres0, dres_mode, dz, y, pos, amb, k, C, dtype, route):
    """dy / dres: [P, Cs] results (or None); dres0: the prefill of the accumulate mode; k = (k1, k2, k3) f32 vectors, k2 = k3 = None
    for the frozen form."""
    dzl = dz[:, :C].double()
    g = dzl if pos is None else dzl * pos
    w = 0.0
    if dy is not None:
        k1 = k[0].double()
        ref, mag = k1 * g, (k1 * g).abs()
        if k[1] is not None:
            k2, k3 = k[1].double(), k[2].double()
            yl = y[:, :C].double()
            ref, mag = ref + k2 * yl + k3, mag + (k2 * yl).abs() + k3.abs()
            del yl
        w = check_rows(tag + "dy", dy[:, :C], ref, mag, dtype, route, extra_abs=None if amb is None else (k1 * dzl).abs() * amb,
                       **roundings(4))
        pad_zero(tag + "dy", dy, C)
    if dres is not None:
        if dres_mode == "acc":
            r0 = dres0[:, :C].double()
            w = max(w, check_rows(tag + "dres+=", dres[:, :C], r0 + g, r0.abs() + g.abs(), dtype, route,
                                  extra_abs=None if amb is None else dzl.abs() * amb, **roundings(1)))
            assert torch.equal(dres[:, C:].cpu(), dres0[:, C:]), "%s: dres += changed a pad lane" % tag
        else:
            if amb is None:
                exact(tag + "dres", dres[:, :C].cpu().double(), g, route)
            else:
                check_rows(tag + "dres", dres[:, :C], g, g.abs(), dtype, route, extra_abs=dzl.abs() * amb, **roundings(0))
            pad_zero(tag + "dres", dres, C)
    return w


def check_pool(tag, y_nchw, idx_nchw, x_nchw, route):
    """Forward: bit-equal to float64 F.max_pool2d, idx the first maximum in window coordinates.  Returns (idx reference, tied share)."""
    m, idx, tied = pool_first_max(x_nchw)
    assert torch.equal(m, F.max_pool2d(x_nchw, 3, 2, 1))
    exact("maxpool_forward %s y" % tag, y_nchw.double(), m, route)
    exact("maxpool_forward %s idx" % tag, idx_nchw.to(torch.int64), idx, route)
    return idx, tied


def check_pool_bwd(tag, dx_nchw, dy_nchw, idx, dtype, route):
    H, W = dx_nchw.shape[2:]
    ref, mag = pool_scatter(dy_nchw.double(), idx, H, W)
    return check_rows("maxpool_backward %s" % tag, dx_nchw, ref, mag, dtype, route, "bchw", k_step=1, K=4)


def check_children_sum(name, got, fine, Hc, Wc, dtype, route, base=None):
    """got [B, Hc, Wc, C] = (base +) the sum over each coarse pixel's children of fine [B, Hf, Wf, C]."""
    f = fine.double()
    ref, mag = sum_children(f, Hc, Wc), sum_children(f.abs(), Hc, Wc)
    K = max_children(f.shape[1], Hc) * max_children(f.shape[2], Wc)
    if base is not None:
        ref, mag, K = ref + base.double(), mag + base.double().abs(), K + 1
    return check_rows(name, got, ref, mag, dtype, route, "bhwc", k_step=1, K=K)
