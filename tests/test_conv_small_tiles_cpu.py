"""CPU tier of tests/test_conv_small_tiles_gpu.py: its routes pinned without a GPU, and teeth for its checks.

Route pin: for every case of the GPU file the ConvParams block is built as ops.conv_forward / conv_forward_seg / the class path fill it
(the block builders of tests/test_kernel_names_cpu.py) and mpn_conv_kernel_name must return the route the case names — a later pick_tc
change cannot silently move a case off the tile it is there for.

Teeth: the GPU file's references and checks are plain CPU functions; here they are fed fp32 / bf16 models of the arithmetic.  They must
accept the float64 reference rounded to the output type, a permuted fp32 blocked sum and the two-rounding model of the residual stage,
and reject the faults the tier is there to catch: res_mask ignored, the bit order inside a mask byte reversed, the mask byte of the
neighbouring pixel, a recomputed ReLU mask taken from y > 0, a parity class stored at the wrong offset, a one-tap class that also
writes its neighbours, a stride-2 gather shifted by one input row, the last live row of the 17-of-32 tile zeroed, a sigmoid that leaves
0.5 in a pad lane, and a finalize that adds sum g to dgamma."""
import pytest
import torch
import torch.nn.functional as F

import stream_ref
import test_conv_small_tiles_gpu as st
import test_kernel_names_cpu as kn
from helpers import round_up
from test_conv_tiles_gpu import BF, F32, H16, TP, _pad_lanes_zero, _tile_sums

CASES = {c[0]: c for c in st.CASES}


# ----------------------------------------------------------------------------------------------------------------- route pin
def _blocks(runner, f):
    if runner is st._conv_case:
        return [kn.conv_block(**f)]
    if runner is st._pyramid_case:
        return [kn.pyramid_block(**f)]
    if runner is st._onetap_case:
        return [kn.class_block(**f)]
    assert runner is st._class_case
    return [kn.class_block(a=a, c=c, **f) for a in (0, 1) for c in (0, 1)]


@pytest.mark.parametrize("case", st.CASES, ids=[c[0].replace(" ", "_") for c in st.CASES])
def test_small_tile_case_route(case):
    cid, route, runner, f = case
    names = set(kn._name("mpn_conv_kernel_name", p) for p in _blocks(runner, f))
    assert names == {route}, (cid, names)
    assert route.endswith("true>") == st._needs_ext(f), cid


def test_small_tile_table_reaches_every_required_route():
    assert len(st.REQUIRED_ROUTES) == len(set(st.REQUIRED_ROUTES)) == 15
    reached = set()
    for cid, route, runner, f in st.CASES:
        reached |= set(kn._name("mpn_conv_kernel_name", p) for p in _blocks(runner, f))
    assert not [r for r in st.REQUIRED_ROUTES if r not in reached], [r for r in st.REQUIRED_ROUTES if r not in reached]
    assert all(r.split(", ")[1] in ("32", "64") for r in st.REQUIRED_ROUTES)
    # the one case that sits on the 128-row tile on purpose: too many pixel tiles for the in-launch finalize
    big = [c[0] for c in st.CASES if c[1].split(", ")[1] not in ("32", "64")]
    assert big == ["bf16 dgrad 1x1 64->256 B24 res mask bnb mask"], big


# ----------------------------------------------------------------------------------------------------------------- models of the arithmetic
def _rnd(t, dt):
    return t.to(dt).double()


def _blocked_sum(x, w, k_step, perm_seed, **conv):
    """fp32 blocked summation of F.conv2d(x, w) over input-channel blocks of k_step, the blocks visited in a permuted order."""
    Cin = x.shape[1]
    blocks = list(range(0, Cin, k_step))
    order = torch.randperm(len(blocks), generator=torch.Generator().manual_seed(perm_seed)).tolist()
    acc = None
    for i in order:
        c0 = blocks[i]
        part = F.conv2d(x[:, c0:c0 + k_step], w[:, c0:c0 + k_step], **conv).float()
        acc = part if acc is None else acc + part
    return acc


def _staged_f32(R, f, core):
    """The epilogue up to the staged value, in fp32, from the fp32 accumulator `core`."""
    v = core.float()
    if R.scale is not None:
        v = v * R.scale.view(1, -1, 1, 1)
    if R.bias is not None:
        v = v + R.bias.view(1, -1, 1, 1)
    if f.get("act") == 1:
        v = v.clamp(min=0)
    if f.get("act") == 2:
        v = torch.sigmoid(v)
    return v


def _core(R, f, perm_seed=None):
    """The convolution itself: float64, or the permuted fp32 blocked sum."""
    if f.get("mode", 0) == 1:
        assert f.get("stride", 1) == 1 and f["k"] == 1
        w = R.wf.transpose(0, 1).contiguous()
        conv = dict()
    else:
        w, conv = R.wv, dict(stride=f.get("stride", 1), padding=R.pad)
    if perm_seed is None:
        return F.conv2d(R.x, w, **conv)
    return _blocked_sum(R.x, w, R.k_step, perm_seed, **conv)


def _two_rounding(R, f, core, res_term=None):
    """Staged value rounded to the output type, the residual stage added in fp32, rounded again."""
    v = _staged_f32(R, f, core).to(R.odt).float()
    if R.res is not None:
        r = st._upsample(R.res, R.Ho, R.Wo)
        if R.zr is not None:
            r = r * (R.zr > 0)
        v = v + (r if res_term is None else res_term).float()
    if R.prev is not None:
        v = v + R.prev.float()
    if f.get("act") == 3:
        v = v.clamp(min=0)
    return _rnd(v, R.odt)


def _reject(fn, *a, **k):
    with pytest.raises(AssertionError):
        fn(*a, **k)


# ----------------------------------------------------------------------------------------------------------------- teeth
def test_bounds_accept_correct_results_of_every_plain_case_kind():
    """The float64 reference rounded to the output type, and a permuted fp32 blocked sum through the fp32 epilogue, pass."""
    for cid in ("bf16 1x1 s2 256->500 bias", "bf16 3x3 256->17 bias f32out", "f32 3x3 s2 128->128 bias", "f16 1x1 256->128 bias res2 from 15x14",
                "bf16 s3 3x3 256->36 bias sigmoid f32out"):
        _, route, _, f = CASES[cid]
        R = st._ref(cid, f)
        assert st._check_out("cpu teeth exact " + cid, route, f, R, _rnd(R.ref, R.odt)) <= 1.0
        assert st._check_out("cpu teeth permuted " + cid, route, f, R, _two_rounding(R, f, _core(R, f, perm_seed=3))) <= 1.0


def test_res_mask_bound_accepts_the_two_rounding_model_and_rejects_mask_faults():
    cid = "bf16 dgrad 1x1 64->256 res mask bnb mask"
    _, route, _, f = CASES[cid]
    R = st._ref(cid, f)
    core = _core(R, f, perm_seed=5)
    good = _two_rounding(R, f, core)
    assert st._check_out("cpu teeth two roundings " + cid, route, f, R, good) <= 1.0
    assert st._check_out("cpu teeth exact " + cid, route, f, R, _rnd(R.ref, R.odt)) <= 1.0

    # the device's mask bytes, as the test packs them: [P][Cs / 8], bit e = z > 0
    B, C, Ho, Wo = R.zr.shape
    zs = torch.zeros(B, Ho, Wo, round_up(C, 32))
    zs[..., :C] = R.zr.permute(0, 2, 3, 1)
    bits = st.pack_bits(zs.to(R.odt), R.odt)
    assert torch.equal(bits, stream_ref.pack_mask(zs.reshape(-1, zs.shape[-1]) > 0, R.odt))

    def masked(byte_of):
        m = stream_ref.unpack_mask(byte_of, R.odt)[:, :C].reshape(B, Ho, Wo, C).permute(0, 3, 1, 2)
        return R.res * m

    assert torch.equal(masked(bits), R.res * (R.zr > 0))
    rev = torch.zeros_like(bits)
    for e in range(8):
        rev |= ((bits >> e) & 1) << (7 - e)
    faults = {"res_mask ignored": R.res,
              "bit order inside a mask byte reversed": masked(rev),
              "mask byte of the neighbouring pixel": masked(torch.roll(bits, 1, 0))}
    for tag, term in faults.items():
        _reject(st._check_out, "cpu teeth %s" % tag, route, f, R, _two_rounding(R, f, core, res_term=term))


def test_bnb_partials_accept_the_device_order_and_reject_a_mask_from_y():
    cid = "bf16 dgrad 1x1 256->64 bnb recompute"
    _, route, _, f = CASES[cid]
    R = st._ref(cid, f)
    got = _two_rounding(R, f, _core(R, f, perm_seed=7))
    pos, amb = st.relu_mask("re", R)
    assert float(amb.mean()) <= st.AMBIGUOUS_MAX

    def partials(mask):
        # fp32 sums in another order than the reference's: pixels of a tile in reverse
        xh = ((R.yb.float() - R.mean.view(1, -1, 1, 1)) * R.invstd.view(1, -1, 1, 1))
        g = (got * mask).float()
        P = g.numel() // g.shape[1]
        tiles = (P + TP - 1) // TP
        out = torch.zeros(tiles, g.shape[1], 2)
        gp, xp = st._pc(g), st._pc(xh)
        for t in range(tiles):
            for p in reversed(range(t * TP, min(P, (t + 1) * TP))):
                out[t, :, 0] += gp[p]
                out[t, :, 1] += gp[p] * xp[p]
        return out

    # the epilogue's own fp32 recomputation of the sign
    dev = (R.yb.float() * R.bscale.view(1, -1, 1, 1) + R.bshift.view(1, -1, 1, 1)) > 0
    st._check_bnb("cpu teeth " + cid, route, f, R, got, partials(dev.double()))
    _reject(st._check_bnb, "cpu teeth mask from y > 0", route, f, R, got, partials((R.yb > 0).double()))


def test_bnb_finalize_rejects_sum_g_added_to_dgamma():
    from multiposenet.pytorch_amd.ops import BNBackwardResult
    cid = "f32 dgrad 1x1 256->64 bnb recompute finalize train"
    _, route, _, f = CASES[cid]
    R = st._ref(cid, f)
    got = _rnd(R.ref, R.odt)
    pos, _ = st.relu_mask("re", R)
    xh = (R.yb - st._c(R.mean)) * st._c(R.invstd)
    gz = got * pos
    part = _tile_sums(gz, [gz, gz * xh])[0].float()
    count = float(got.numel() // got.shape[1])
    S1, S2, k1, k2, k3, _, _, _ = stream_ref.bwd_coef_ref(part, count, R.gamma, R.mean, R.invstd)
    fused = BNBackwardResult(None, torch.stack([k1, k2, k3]).float(), False)
    st._check_bnb_fin("cpu teeth " + cid, route, f, R, part, (R.dg0.double() + S2).float(), (R.db0.double() + S1).float(), fused, count)
    _reject(st._check_bnb_fin, "cpu teeth dgamma += sum g", route, f, R, part, (R.dg0.double() + S1).float(), (R.db0.double() + S1).float(), fused, count)
    # frozen statistics: no coefficients, dgamma / dbeta still accumulated
    ff = dict(f, bnb_fin="frozen")
    frozen = BNBackwardResult(None, None, True)
    st._check_bnb_fin("cpu teeth frozen", route, ff, R, part, (R.dg0.double() + S2).float(), (R.db0.double() + S1).float(), frozen, count)
    _reject(st._check_bnb_fin, "cpu teeth frozen, dgamma untouched", route, ff, R, part, R.dg0, (R.db0.double() + S1).float(), frozen, count)


def test_class_checks_reject_a_wrong_offset_and_a_wrong_table_row():
    cid = "bf16 dgrad s2 classes 128->128 acc bnb mask"
    _, route, _, f = CASES[cid]
    R = st._class_ref(cid, f)
    B, Cx, Hx, Wx = R.ref.shape
    # two-rounding model per class: the class's sum rounded, the previous dx added in fp32, rounded again
    good = _rnd(R.ref.float().to(R.odt).float() + R.prev.float(), R.odt)
    from multiposenet.pytorch_amd.ops import dgrad_s2_class_plan
    plan = dgrad_s2_class_plan(B, Hx, Wx)
    pos, _ = st.relu_mask("mask", R)
    xh = (R.yb - st._c(R.mean)) * st._c(R.invstd)

    def table(got):
        rows = []
        for a, c, ho, wo, t, tile0 in plan:
            gz = (got * pos)[:, :, a::2, c::2]
            rows.append(_tile_sums(gz, [gz, gz * xh[:, :, a::2, c::2]])[0])
        return torch.cat(rows).float()

    st._check_classes("cpu teeth " + cid, route, f, R, good, table(good))
    # class (0, 1) stored at the offset of class (1, 0) and the reverse (both 15x13 / 14x14 grids differ: swap the common part)
    bad = good.clone()
    h, w = min(good[:, :, 0::2, 1::2].shape[2], good[:, :, 1::2, 0::2].shape[2]), min(good[:, :, 0::2, 1::2].shape[3], good[:, :, 1::2, 0::2].shape[3])
    bad[:, :, 0::2, 1::2][:, :, :h, :w] = good[:, :, 1::2, 0::2][:, :, :h, :w]
    bad[:, :, 1::2, 0::2][:, :, :h, :w] = good[:, :, 0::2, 1::2][:, :, :h, :w]
    _reject(st._check_classes, "cpu teeth class stored at the wrong offset", route, f, R, bad)
    # the classes' table rows in the wrong place: class (0, 1) and (1, 0) have the same number of tiles here
    t = table(good)
    (_, _, _, _, t1, r1), (_, _, _, _, t2, r2) = plan[1], plan[2]
    assert t1 == t2
    sw = t.clone()
    sw[r1:r1 + t1], sw[r2:r2 + t2] = t[r2:r2 + t2], t[r1:r1 + t1]
    _reject(st._check_classes, "cpu teeth class partials in another class's rows", route, f, R, good, sw)


def test_onetap_check_rejects_written_neighbours():
    cid = "bf16 dgrad 1x1 s2 one-tap class 512->256 existing dx"
    _, route, _, f = CASES[cid]
    R = st._class_ref(cid, f)
    prefill = R.prev.permute(0, 2, 3, 1).to(R.odt).contiguous()
    good = (R.ref.float().to(R.odt).float() + R.prev.float()).permute(0, 2, 3, 1).to(R.odt).contiguous()
    assert torch.equal(good[:, 1::2], prefill[:, 1::2]) and torch.equal(good[:, :, 1::2], prefill[:, :, 1::2])
    st._check_onetap("cpu teeth " + cid, route, f, R, good, prefill)
    bad = good.clone()
    bad[:, ::2, 1::2] = (good[:, ::2, 1::2].float() + 0.0).to(R.odt)            # rewritten with the same values: still fine
    st._check_onetap("cpu teeth neighbours rewritten unchanged", route, f, R, bad, prefill)
    bad = good.clone()
    bad[:, 0::2, 1::2] = good[:, 0::2, 0::2][:, :, : good[:, 0::2, 1::2].shape[2]]  # the class value also lands on its right neighbour
    _reject(st._check_onetap, "cpu teeth one-tap class writes its neighbours", route, f, R, bad, prefill)
    bad = good.clone()
    bad[:, 1, 1, 0] = 0.0                                                        # one neighbour zeroed
    _reject(st._check_onetap, "cpu teeth one neighbour zeroed", route, f, R, bad, prefill)


def test_gather_checks_reject_a_shifted_input_row():
    cid = "bf16 dgrad 1x1 s2 gather 512->256 fresh"
    _, route, _, f = CASES[cid]
    R = st._ref(cid, f)
    good = _rnd(R.ref, R.odt)
    st._check_out("cpu teeth " + cid, route, f, R, good)
    st._gather_zeros("cpu teeth " + cid, route, good)
    shifted = torch.roll(good, 1, 2)                     # every output row reads the input row above
    _reject(st._gather_zeros, "cpu teeth gather shifted by one input row (zeros)", route, shifted)
    _reject(st._check_out, "cpu teeth gather shifted by one input row", route, f, R, shifted)
    # the same fault in the forward stride-2 gather: output row ho reads input rows 2 ho - 1 .. instead of 2 ho ..
    cid = "bf16 3x3 s2 128->128 stats"
    _, route, _, f = CASES[cid]
    R = st._ref(cid, f)
    st._check_out("cpu teeth " + cid, route, f, R, _rnd(R.ref, R.odt))
    wrong = F.conv2d(torch.roll(R.x, 1, 2), R.wv, stride=2, padding=1)
    _reject(st._check_out, "cpu teeth forward s2 gather shifted by one input row", route, f, R, _rnd(wrong, R.odt))


def test_partial_tile_checks_reject_a_zeroed_last_row_and_a_sigmoid_pad_lane():
    cid = "bf16 3x3 256->17 bias f32out"
    _, route, _, f = CASES[cid]
    R = st._ref(cid, f)
    good = _rnd(R.ref, R.odt)
    st._check_out("cpu teeth " + cid, route, f, R, good)
    bad = good.clone()
    bad[:, 16] = 0.0
    _reject(st._check_out, "cpu teeth last live row of the 17-of-32 tile zeroed", route, f, R, bad)

    cid = "bf16 s3 3x3 256->36 bias sigmoid f32out"
    _, route, _, f = CASES[cid]
    R = st._ref(cid, f)
    B, C, Ho, Wo = R.ref.shape

    class Out(object):          # the storage view _pad_lanes_zero reads
        def __init__(self, pad):
            self.C, self.Cs = C, round_up(C, 32)
            self.t = torch.full((B, Ho, Wo, self.Cs), pad)
            self.t[..., :C] = R.ref.permute(0, 2, 3, 1).float()
    _pad_lanes_zero("cpu teeth " + cid, Out(0.0))
    _reject(_pad_lanes_zero, "cpu teeth sigmoid leaves 0.5 in a pad lane", Out(0.5))
    # and sigmoid of the un-biased accumulator is not sigmoid of the pre-activation
    _reject(st._check_out, "cpu teeth sigmoid before the bias", route, f, R, torch.sigmoid(R.pre - st._c(R.bias)))
