"""Shared helpers for the parity tests (test-side only)."""
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
REPORT = os.path.join(ROOT, "gpurun_out", "parity_report.txt")


def report(line):
    os.makedirs(os.path.dirname(REPORT), exist_ok=True)
    with open(REPORT, "a") as f:
        f.write(line + "\n")


def round_up(v, m):
    return (v + m - 1) // m * m


def to_act(x_nchw, dtype, device="cuda"):
    from multiposenet.pytorch_amd.ops import Act
    B, C, H, W = x_nchw.shape
    t = torch.zeros(B, H, W, round_up(C, 32), dtype=torch.float32)
    t[..., :C] = x_nchw.permute(0, 2, 3, 1)
    return Act(t.to(dtype).to(device), C)


def from_act(a):
    return a.t[..., : a.C].float().cpu().permute(0, 3, 1, 2).contiguous()


def w_krsc(w_oihw, dtype, device="cuda"):
    return w_oihw.permute(0, 2, 3, 1).contiguous().to(dtype).to(device)


def rnd(dtype, x):
    """Round a f32 CPU tensor through `dtype` (so the CPU reference sees the same operand values)."""
    return x.to(dtype).float()


def tol(dtype):
    return 2e-4 if dtype == torch.float32 else 2e-2


def check_close(name, got, ref, dtype, scale=None, factor=1.0):
    got = got.double()
    ref = ref.double()
    s = ref.abs().max().item() if scale is None else scale
    err = (got - ref).abs().max().item()
    lim = tol(dtype) * factor * max(s, 1e-6)
    report("%-60s err=%.3e  lim=%.3e  refmax=%.3e  %s" % (name, err, lim, s, "OK" if err <= lim else "FAIL"))
    assert err <= lim, "%s: max err %.3e > %.3e (ref max %.3e)" % (name, err, lim, s)


U24 = 2.0 ** -24          # unit roundoff of fp32


def ulp_out(v, out_dtype):
    """Spacing of `out_dtype` at |v| (float64 tensor): 0 for f32 outputs (no output rounding to allow for), 2^-7 * 2^floor(log2|v|) for
    bf16 (8-bit significand), 2^-10 * 2^floor(log2|v|) for f16 with a floor of 2^-24 (f16 subnormals)."""
    v = v.abs().double()
    if out_dtype == torch.float32:
        return torch.zeros_like(v)
    bits = 7 if out_dtype == torch.bfloat16 else 10
    _, e = torch.frexp(v)                                       # v = m * 2^e, m in [0.5, 1): floor(log2 v) = e - 1
    u = torch.ldexp(torch.ones_like(v), (e - 1 - bits).to(torch.int64).clamp(min=-1074))
    u = torch.where(v > 0, u, torch.zeros_like(v))
    if out_dtype == torch.float16:
        u = u.clamp(min=2.0 ** -24)
    return u


def _loc(shape, flat, names):
    idx = []
    for n in reversed(shape):
        idx.append(flat % n)
        flat //= n
    return "(%s)" % ", ".join("%s=%d" % (k, i) for k, i in zip(names, reversed(idx)))


def check_elementwise(name, got, ref64, mag64, out_dtype, k_step, K, extra_terms=0, extra_abs=None, route="", names="bchw"):
    """Per-element parity of a kernel result against its float64 reference.

    ref64: the operation in float64 on exactly the operand values the kernel sees; mag64: the same operation on absolute values
    (conv(|x|, |w|) |scale| + |bias| + |res| ...).  Every element must satisfy
        |got - ref64| <= 0.5 ulp_out(max(|ref64|, |got|)) + (K / k_step + k_step + extra_terms + 2) 2^-24 mag64 [+ extra_abs]
    — half a spacing of the output type (the kernels store by round-to-nearest-even) plus the linear worst-case bound of an fp32
    blocked summation of K terms in steps of k_step (32 for the 16-bit MFMA, 4 for the exact-fp32 one; per-tile statistics use
    k_step 1 with K = the pixels summed).  extra_abs: an absolute allowance derived by the caller from an intermediate rounding
    (the staged value of a residual epilogue).  Writes the worst err / bound and its location to the parity report; fails on the
    first violating element (in index order), naming it."""
    got = got.double().cpu()
    ref64 = ref64.double().cpu()
    mag64 = mag64.double().cpu()
    assert got.shape == ref64.shape == mag64.shape, (name, got.shape, ref64.shape, mag64.shape)
    err = (got - ref64).abs()
    bound = 0.5 * ulp_out(torch.maximum(ref64.abs(), got.abs().nan_to_num(0.0)), out_dtype) \
        + (K / float(k_step) + k_step + extra_terms + 2) * U24 * mag64
    if extra_abs is not None:
        bound = bound + extra_abs.double().cpu()
    bad = ~(err <= bound)                                       # NaN in got is a violation
    ratio = torch.where(bound > 0, err / bound, torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    names = list(names)[: got.dim()] if len(names) >= got.dim() else ["i%d" % d for d in range(got.dim())]
    wf = int(torch.argmax(ratio.reshape(-1)))
    worst = float(ratio.reshape(-1)[wf])
    report("%-58s %-52s worst err/bound=%.3f at %s  %s" % (name, route, worst, _loc(got.shape, wf, names), "OK" if not bool(bad.any()) else "FAIL"))
    if bool(bad.any()):
        f = int(torch.nonzero(bad.reshape(-1))[0])
        raise AssertionError("%s: element %s got %r, float64 reference %r, |err| %.3e > bound %.3e (worst err/bound %.3f at %s)" % (
            name, _loc(got.shape, f, names), float(got.reshape(-1)[f]), float(ref64.reshape(-1)[f]), float(err.reshape(-1)[f]),
            float(bound.reshape(-1)[f]), worst, _loc(got.shape, wf, names)))
    return worst


def rng_normal(seed, *shape):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g)


def gold(name):
    return np.load(os.path.join(GOLD, name), allow_pickle=False)
