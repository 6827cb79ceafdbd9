"""Teeth of the parameter-path tier (no GPU): tests/param_ref.py's references are anchored to independent restatements, its Adam bounds
accept the float32 model of the kernel text in every contraction a compiler may choose and reject each modelled fault, and its
bit-exact references reject the modelled faults of the casts, the transpose, the stem packings and the unpack.  The GPU file
(tests/test_param_path_gpu.py) applies exactly these checks to the kernels."""
import numpy as np
import pytest
import torch

import param_ref as R

f32, f64 = np.float32, np.float64


def u16(t):
    return R.ibits(t).numpy().view(np.uint16)


# ====================================================================================================== 1. anchoring
def test_cast_edge_set_holds_every_edge_the_tier_names():
    e = R.cast_edge_values()
    x = e[:-1]
    b = R.bits32(x)
    bf = R.rne_bf16_bits(x)
    ties_bf = (b & 0xFFFF) == 0x8000
    lower = (b >> 16) & 1
    assert (ties_bf & (lower == 0)).sum() >= 4 and (ties_bf & (lower == 1)).sum() >= 4
    ties_h = ((b & 0x1FFF) == 0x1000) & (np.abs(x) >= 2.0 ** -14) & (np.abs(x) < 65520)
    lower = (b >> 13) & 1
    assert (ties_h & (lower == 0)).sum() >= 4 and (ties_h & (lower == 1)).sum() >= 4
    for p in b[ties_bf | ties_h]:                                     # one spacing above and below each tie
        assert (b == p - 1).any() and (b == p + 1).any()
    assert (b == 0).any() and (b == 0x80000000).any() and np.isinf(x).sum() == 2 and np.isnan(e[-1])
    assert (b == 0x7F7FFFFF).any() and bf[b == 0x7F7FFFFF][0] == 0x7F80          # the largest finite f32 rounds to +inf in bf16
    h = R.rne_f16_bits(x)
    assert h[x == f32(65504.0)][0] == 0x7BFF and h[x == f32(65520.0)][0] == 0x7C00 and h[b == R.bits32(f32(65520.0))[0] - 1][0] == 0x7BFF
    sub = (np.abs(x) >= 6e-8) & (np.abs(x) <= 6e-5)
    assert sub.sum() >= 60 and ((h[sub] & 0x7C00) == 0).sum() >= 60              # land on f16 subnormals
    assert h[b == 0x33000000][0] == 0 and h[b == 0x33000001][0] == 1 and h[b == 0x33C00000][0] == 2
    for n in R.CAST_SIZES:
        assert len(R.cast_input(n)) == n


@pytest.mark.parametrize("dtype", [R.BF, R.H16])
def test_torch_cpu_conversion_is_the_bit_level_round_to_nearest_even(dtype):
    x = R.cast_edge_values()[:-1]
    r = np.random.default_rng(3)
    more = R.from_bits(r.integers(0x00800000, 0x7F800000, 50000).astype(np.uint32) | (r.integers(0, 2, 50000).astype(np.uint32) << 31))
    x = np.concatenate([x, more])
    want = R.rne_bf16_bits(x) if dtype == R.BF else R.rne_f16_bits(x)
    assert np.array_equal(u16(R.cast_ref(x, dtype)), want)


def test_transpose_reference_is_the_permutation_with_zero_pad_columns():
    for O, RS, I, opad in R.TRANSPOSE_GEOMS:
        w = R.weights(O + RS, O * RS * I)
        for dtype in R.TYPES:
            ref = R.transpose_ref(w, O, RS, I, opad, dtype)
            assert ref.shape == (I, RS, opad)
            for (i, rs, o) in ((0, 0, 0), (I - 1, RS - 1, O - 1), (I // 2, RS // 2, O // 2)):
                assert ref[i, rs, o] == w[(o * RS + rs) * I + i].to(dtype)
            assert bool((R.ibits(ref[..., O:]) == 0).all())
    rows, src, dst, blk = R.wt_layout(R.TRANSPOSE_GEOMS)
    assert all(r[1] % 64 == 0 and r[0] % 64 == 0 for r in rows) and rows[3][1] - rows[2][1] == R.round_up(3 * 49 * 32, 64)
    assert blk == sum(((I + 31) // 32) * ((p + 31) // 32) * RS for _, RS, I, p in R.TRANSPOSE_GEOMS)


def test_stem_references_follow_the_indexing():
    Cout = 3
    w = R.weights(5, Cout * 147)
    pk = R.stem_pack_weight_ref(w, Cout, R.F32)
    for co in range(Cout):
        for r in range(7):
            for slot in range(32):
                s, c = slot >> 2, slot & 3
                want = w[((co * 7 + r) * 7 + s) * 3 + c] if (s < 7 and c < 3) else 0.0
                assert pk[co, r, slot] == want
    dp = torch.full((Cout, 7, 32), 1e30)
    dp.view(Cout, 7, 8, 4)[:, :, :7, :3] = R.weights(6, Cout * 147).view(Cout, 7, 7, 3)
    dw = R.weights(7, Cout * 147) * 3 + 1
    out = R.stem_unpack_ref(dw, dp, Cout)
    assert bool(out.abs().max() < 10) and out[4] == dw[4] + dp.reshape(-1)[(0 * 7 + 0) * 32 + 1 * 4 + 1]
    x = torch.randn(2, 3, 7, 5)
    im = R.stem_pack_image_ref(x, R.F32)
    assert im.shape == (2, 13, 13, 4) and im[1, 3 + 6, 3 + 4, 2] == x[1, 2, 6, 4]
    assert im[:, :3].abs().sum() == 0 and im[:, -3:].abs().sum() == 0 and im[:, :, :3].abs().sum() == 0 and im[:, :, -5:].abs().sum() == 0
    assert im[..., 3].abs().sum() == 0


# ====================================================================================================== 2. Adam: the bounds accept
def _hyper(wd, gs, t, betas=(0.9, 0.999)):
    h = R.hyper_vector(wd=wd, gs=gs, b1=betas[0], b2=betas[1], step=t)
    h[6], h[7] = R.bias_corrections(h[1], h[2], t)
    return h


@pytest.mark.parametrize("contract", [0, 1, 2])
def test_adam_bounds_accept_every_contraction_of_the_kernel_text(contract):
    worst = R.Worst()
    for wd, gs in R.ADAM_SETTINGS:
        for t in R.ADAM_STEPS + (100000,):
            for moments in (False, True):
                h = _hyper(wd, gs, t)
                p, g, m, v = R.adam_inputs(20000, 17 * t + int(1000 * wd) + moments, moments)
                got = R.adam_model32(p, g, m, v, h, contract)
                worst.add(R.check_adam("model", got, p, g, m, v, h), "wd=%g gs=%g t=%d mom=%d" % (wd, gs, t, moments))
    for line in worst.lines("adam model contract=%d" % contract):
        print(line)
    # m' and v' sit well inside (the deepest paths carry 5 and 8 roundings of the 6 and 11 allowed).  p' comes close to 1 by
    # construction, not by accident: where |U| << |p| and |p| lies just above a power of two, half a spacing of p' IS u 2^k ~ u |p|.
    assert worst.w["m'"][0] <= 0.75 and worst.w["v'"][0] <= 0.75 and worst.w["p'"][0] <= 1.0, worst.w


def test_adam_neutral_elements_stay_plus_zero_in_the_model():
    z = np.zeros(8, f32)
    for wd in (0.0, 1e-2):
        got = R.adam_model32(z, z, z, z, _hyper(wd, 0.37, 3))
        for x in got:
            assert not R.bits32(x).any()
        R.check_adam("neutral", got, z, z, z, z, _hyper(wd, 0.37, 3))


# ====================================================================================================== 3. Adam: the bounds reject
@pytest.mark.parametrize("fault", R.ADAM_FAULTS)
def test_adam_bounds_reject_the_fault(fault):
    """At every tested step count, with zero and with non-zero moments, in the settings where the fault changes anything."""
    needs_wd = fault in ("wd_before_scale", "decoupled")
    hit = 0
    for wd, gs in R.ADAM_SETTINGS:
        if needs_wd and (wd == 0 or (fault == "wd_before_scale" and gs == 1.0)):
            continue                                                  # the fault is the identity there
        for t in R.ADAM_STEPS:
            for moments in (False, True):
                h = _hyper(wd, gs, t)
                if fault == "no_bc1" and h[6] == 1.0:
                    continue                                          # t = 1000: 0.9^t is below half a spacing of 1, bc1 is 1
                p, g, m, v = R.adam_inputs(4099, 5 * t + moments, moments)
                with np.errstate(invalid="ignore"):                   # v_with_G makes v' negative: NaN, a violation
                    got = R.adam_model32(p, g, m, v, h, 0, fault)
                with pytest.raises(AssertionError), np.errstate(invalid="ignore"):
                    R.check_adam(fault, got, p, g, m, v, h)
                hit += 1
    assert hit >= 8


@pytest.mark.parametrize("fault", ["skips_last", "one_past_n"])
@pytest.mark.parametrize("n", [5, 1023, 4099])
def test_adam_slice_check_rejects_a_wrong_tail(fault, n):
    h = _hyper(1e-2, 0.37, 2)
    s = 64
    tot = s + R.round_up(n, 4) + 64
    p, g, m, v = R.adam_inputs(tot, n, True)
    before = dict(p=p, g=g, m=m, v=v)

    def run(e):
        after = {k: x.copy() for k, x in before.items()}
        after["p"][s:e], after["m"][s:e], after["v"][s:e] = R.adam_model32(p[s:e], g[s:e], m[s:e], v[s:e], h)
        return after
    R.check_adam_slice("good", before, run(s + n), s, s + n, h)
    with pytest.raises(AssertionError):
        R.check_adam_slice(fault, before, run(s + n - 1 if fault == "skips_last" else s + n + 1), s, s + n, h)


# ====================================================================================================== 4. bit-exact references reject
@pytest.mark.parametrize("mode", ["half_up", "trunc"])
def test_cast_reference_rejects_another_rounding_rule(mode):
    for n in (9, 2049):
        x = R.cast_input(n)
        good = torch.from_numpy(R.rne_bf16_bits(np.where(np.isnan(x), f32(0), x)).view(np.int16)).view(R.BF).clone()
        good[torch.from_numpy(np.isnan(x))] = float("nan")
        R.check_cast("rne", good, x, R.BF)
        bad = torch.from_numpy(R.rne_bf16_bits(np.where(np.isnan(x), f32(0), x), mode).view(np.int16)).view(R.BF).clone()
        bad[torch.from_numpy(np.isnan(x))] = float("nan")
        with pytest.raises(AssertionError):
            R.check_cast(mode, bad, x, R.BF)
    # half-up differs from ties-to-even exactly at the ties with an even lower neighbour
    e = R.cast_edge_values()[:-1]
    d = R.rne_bf16_bits(e) != R.rne_bf16_bits(e, "half_up")
    b = R.bits32(e)
    assert np.array_equal(d, ((b & 0xFFFF) == 0x8000) & (((b >> 16) & 1) == 0))


def test_transpose_reference_rejects_stale_pad_columns():
    O, RS, I, opad = 3, 1, 40, 96
    w = R.weights(1, O * RS * I)
    for dtype in R.TYPES:
        prev = torch.full((I * RS * opad,), 0.5).to(dtype)
        good, bad = R.transpose_ref(w, O, RS, I, opad, dtype), R.transpose_ref(w, O, RS, I, opad, dtype, prev=prev)
        assert torch.equal(R.ibits(good[..., :O]), R.ibits(bad[..., :O])) and not torch.equal(R.ibits(good), R.ibits(bad))
    # and a pad of -0.0 is not +0
    neg = R.transpose_ref(w, O, RS, I, opad, R.F32, prev=torch.full((I * RS * opad,), -0.0))
    assert torch.equal(neg, R.transpose_ref(w, O, RS, I, opad, R.F32)) and not torch.equal(R.ibits(neg), R.ibits(R.transpose_ref(w, O, RS, I, opad, R.F32)))


def test_stem_references_reject_the_next_pixel_and_an_overwriting_unpack():
    for B, H, W in R.IMAGE_SHAPES:
        x = torch.randn(B, 3, H, W) + 2.0
        for dtype in R.TYPES:
            assert not torch.equal(R.ibits(R.stem_pack_image_ref(x, dtype)), R.ibits(R.stem_pack_image_ref(x, dtype, mut="next_pixel")))
    Cout = 3
    dp = R.weights(8, Cout * 7 * 32).view(Cout, 7, 32)
    dw = R.weights(9, Cout * 147) + 1.0
    assert not torch.equal(R.stem_unpack_ref(dw, dp, Cout), R.stem_unpack_ref(dw, dp, Cout, mut="assign"))


# ====================================================================================================== 5. the betas the device uses
def test_device_bias_corrections_differ_from_the_host_doubles_by_the_documented_amount():
    """Finding: adam_advance_kernel widens the FLOAT betas; torch.optim.Adam raises the Python doubles.  The figures below are the ones
    DESIGN.md, weight_prep.hip and optim.py quote."""
    r1, r2, t1, t2 = R.beta_rounding_distance()
    print("bc1: largest relative difference %.3e at t=%d; bc2s: %.3e at t=%d" % (r1, t1, r2, t2))
    assert 2.3e-7 < r1 < 2.4e-7 and t1 == 2
    assert 6.4e-6 < r2 < 6.6e-6 and t2 == 4
    bc1, _ = R.bias_corrections(0.9, 0.999, 1)
    assert R.spacings_apart(bc1, f32(0.1)) == 3                       # 1 - 0.9f = 0.10000002384, three spacings above 0.1f
    assert R.bias_corrections(0.9, 0.999, 100000) == (f32(1.0), f32(1.0))
    assert R.bias_corrections(0.8, 0.99, 100000) == (f32(1.0), f32(1.0))
