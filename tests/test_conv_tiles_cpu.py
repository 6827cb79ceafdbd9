"""Teeth for helpers.check_elementwise (CPU tier): the per-element bound the route-pinned conv tests use
(tests/test_conv_tiles_gpu.py) must accept every correct result — the float64 reference rounded to the output type, and an fp32
blocked summation in a different order — and reject the bugs those tests are there to catch: a k-step lost in the last partial
pixel tile, one input channel missing from one output channel, the last live channel row of a partial channel tile left at
zero, an image column shifted at the right border, and a double rounding of the output."""
import pytest
import torch
import torch.nn.functional as F

from helpers import check_elementwise, rng_normal, ulp_out

B, CIN, H, W, COUT = 2, 64, 13, 11, 200          # K = 576; P = 286: pixel tiles of 128, 128 and 30; channel tiles 128 + 72 (partial)
TP = 128


def _operands(dtype):
    x = rng_normal(71, B, CIN, H, W).to(dtype).double()
    w = (rng_normal(72, COUT, CIN, 3, 3) / (CIN * 9) ** 0.5).to(dtype).double()
    return x, w


def _step_partials(x, w, kc):
    """fp32-rounded partial sums of the k-steps of the implicit GEMM: [(tap, c0)] -> [B, Cout, H, W] (kc channels of one tap)."""
    cols = F.unfold(x, 3, padding=1).view(B, CIN, 9, H * W)
    wt = w.reshape(COUT, CIN, 9)
    out = {}
    for t in range(9):
        for c0 in range(0, CIN, kc):
            part = torch.einsum("oc,bcl->bol", wt[:, c0:c0 + kc, t], cols[:, c0:c0 + kc, t])
            out[(t, c0)] = part.view(B, COUT, H, W)
    return out


def _blocked(parts, order):
    acc = torch.zeros(B, COUT, H, W, dtype=torch.float32)
    for k in order:
        acc = acc + parts[k].float()
    return acc


def _last_tile_mask():
    p = torch.arange(B * H * W).view(B, 1, H, W)
    return p >= (B * H * W - 1) // TP * TP


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_elementwise_bound_accepts_correct_results_and_rejects_kernel_bugs(dtype):
    x, w = _operands(dtype)
    ref64 = F.conv2d(x, w, padding=1)
    mag64 = F.conv2d(x.abs(), w.abs(), padding=1)
    k_step = 32 if dtype != torch.float32 else 4
    kc = 32 if dtype != torch.float32 else 16                  # channels per k-step of the kernel's operand ring
    K = CIN * 9
    out_dt = dtype

    def rnd(t):
        return t.to(out_dt).double()

    def check(tag, got):
        return check_elementwise("cpu teeth %s %s" % (str(dtype), tag), got, ref64, mag64, out_dt, k_step, K)

    # correct results pass
    assert check("exact", rnd(ref64)) <= 1.0
    parts = _step_partials(x, w, k_step)
    keys = list(parts)
    perm = torch.randperm(len(keys), generator=torch.Generator().manual_seed(5)).tolist()
    acc_rev = _blocked(parts, keys[::-1])
    acc_perm = _blocked(parts, [keys[i] for i in perm])
    check("reversed fp32 order", rnd(acc_rev))
    check("permuted fp32 order", rnd(acc_perm))

    # mutations fail
    mutations = {}
    drop = sum(parts[(4, c)] for c in range(kc, 2 * kc, k_step)).float()          # channels [kc, 2 kc) of the centre tap
    mutations["k-step dropped in the last partial pixel tile"] = acc_perm - drop * _last_tile_mask()
    m = acc_perm.clone()
    m[:, 7] -= F.conv2d(x[:, 13:14], w[7:8, 13:14], padding=1)[:, 0].float()
    mutations["input channel 13 missing from output channel 7"] = m
    m = acc_perm.clone()
    m[:, COUT - 1] = 0.0
    mutations["last live row of the partial channel tile zeroed"] = m
    m = acc_perm.clone()
    m[B - 1, :, :, W - 1] = acc_perm[B - 1, :, :, W - 2]
    mutations["right-border column shifted by one pixel"] = m
    for tag, mut in mutations.items():
        with pytest.raises(AssertionError):
            check(tag, rnd(mut))
    if dtype == torch.bfloat16:
        with pytest.raises(AssertionError):
            check("rounded twice (f16, then bf16)", acc_perm.half().float().to(out_dt).double())


def test_ulp_out_spacing():
    v = torch.tensor([1.0, 1.5, 2.0, 3.0, 0.0, 2.0 ** -20, -6.0], dtype=torch.float64)
    assert ulp_out(v, torch.float32).eq(0).all()
    assert ulp_out(v, torch.bfloat16).tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -6, 0.0, 2.0 ** -27, 2.0 ** -5]
    assert ulp_out(v, torch.float16).tolist() == [2.0 ** -10, 2.0 ** -10, 2.0 ** -9, 2.0 ** -9, 2.0 ** -24, 2.0 ** -24, 2.0 ** -8]
    # the spacing is what the output types really have: neighbours of a value differ by exactly it
    for dt in (torch.bfloat16, torch.float16):
        t = torch.tensor([1.0, 3.0, 1000.0], dtype=dt)
        nxt = (t.view(torch.int16) + 1).view(dt)                                        # the next representable value up
        assert torch.equal((nxt.double() - t.double()), ulp_out(t.double(), dt))
