#!/usr/bin/env python3
"""Time the PRN training step through the recorded launch list next to the eager step, and the one-launch loss head next to the
kernel chain it replaces.

    python tools/prn_step_bench.py [--out profiles/r12_prn_recorded_step.txt]

On an MI355X: poseNet(50, prn_node_count=1024, prn_coeff=2), everything but the PRN frozen, bf16 and fp32, B = 8 / 64 / 256, on
batches rendered by DevicePRNBatcher from a seeded synthetic annotation set.

  * step: host-clock time per step over windows of steps that end in a device synchronise, after warm-up; windows of
    batch_processor.train_step (the Python tape with autograd, host-seeded dropout: the path before the recorded PRN step) and of
    replay.ReplayedTrainStep alternate inside one process, so both see the same machine state.  Median [min .. max] over windows.
  * head: HIP-event time per call over blocks of calls, the chain mpn_add_softmax_rows -> mpn_bce_mean_forward ->
    mpn_bce_mean_backward -> mpn_softmax_rows_backward -> mpn_cast_f32 (bf16 only) against mpn_prn_head_train on the same
    operands ([B, 34272] float32), blocks alternating.
Nothing is gated on these numbers."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from prn_batch_bench import synthetic_annotations  # noqa: E402


def fmt(t):
    return "%9.1f us [%.1f .. %.1f]" % (statistics.median(t), min(t), max(t))


def alternate(fns, per_window, windows, warmup, clock):
    """Windows of `per_window` calls of each fn in turn (A B A B ..); returns one list of per-call microseconds per fn."""
    for fn in fns:
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(windows):
        for k, fn in enumerate(fns):
            if clock == "host":
                t0 = time.perf_counter()
                for _ in range(per_window):
                    fn()
                torch.cuda.synchronize()
                out[k].append((time.perf_counter() - t0) * 1e6 / per_window)
            else:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(per_window):
                    fn()
                b.record()
                b.synchronize()
                out[k].append(a.elapsed_time(b) * 1e3 / per_window)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--windows", type=int, default=11)
    ap.add_argument("--sizes", type=int, nargs="+", default=[8, 64, 256])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("prn_step_bench needs the MI355X: there is nothing to time on a CPU")
    from multiposenet.pytorch_amd import _lib, ops
    from multiposenet.pytorch_amd._lib import call
    from multiposenet.pytorch_amd.datasets import DevicePRNBatcher, PRNSampleSet
    from multiposenet.pytorch_amd.network.posenet import poseNet
    from multiposenet.pytorch_amd.optim import FusedAdam
    from multiposenet.pytorch_amd.replay import ReplayedTrainStep
    from multiposenet.pytorch_amd.training.batch_processor import train_step

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    ss = PRNSampleSet(synthetic_annotations(400))
    bt = DevicePRNBatcher()
    say("# prn_step_bench: library %s, device %s, torch %s" % (_lib.lib().mpn_version().decode(), torch.cuda.get_device_name(0), torch.__version__))
    say("# poseNet(50, prn_node_count=1024, prn_coeff=2), PRN parameters trainable only; medians over %d alternating windows [min .. max]" % a.windows)
    model = poseNet(50, compute_dtype=torch.float32).cuda()
    for n, p in model.named_parameters():
        p.requires_grad = n.startswith("prn.")
    model.train()
    rs = np.random.RandomState(1)
    n = 56 * 36 * 17
    for B in a.sizes:
        idx = rs.permutation(len(ss))[:B].tolist()
        inp, lab = bt(ss, idx)
        torch.cuda.synchronize()
        per = max(5, min(30, 240 // B))
        for dt, name in ((torch.bfloat16, "bf16"), (torch.float32, "fp32")):
            model.compute_dtype = dt
            opt = FusedAdam(model, lr=1e-5)
            step = ReplayedTrainStep(model, opt)
            inputs, gts = [[inp, "prn_subnet"]], ["prn_subnet", lab]
            for _ in range(2):                                   # the eager pass and the recording
                step(inputs, gts)
            te, tr = alternate([lambda: train_step(model, opt, inputs, gts), lambda: step(inputs, gts)], per, a.windows, per, "host")
            assert step.replays >= per * a.windows
            nl = len(next(iter(step._entries.values())).tape)
            say("step B=%-4d %s  eager train_step %s   recorded (%d list entries) %s   recorded / eager = %.3f" % (
                B, name, fmt(te), nl, fmt(tr), statistics.median(tr) / statistics.median(te)))
            step._drop(next(iter(step._entries)))
            del step, opt
        # ---- loss head: the chain against the one launch, on [B, n] operands
        g = torch.Generator(device="cuda").manual_seed(B)
        o = torch.randn((B, n), device="cuda", generator=g) * 2
        res, y = inp.reshape(B, n).contiguous(), lab.reshape(B, n).contiguous()
        ones = torch.ones(1, device="cuda")
        p, dp, dl = (torch.empty((B, n), device="cuda") for _ in range(3))
        chunks = call("mpn_bce_chunks", B * n)
        part, out1 = torch.empty(max(chunks, B), device="cuda"), torch.empty(1, device="cuda")
        for dt, name in ((torch.bfloat16, "bf16"), (torch.float32, "fp32")):
            d = torch.empty((B, n), dtype=dt, device="cuda")
            st, code = ops.stream_ptr(), ops.dtype_code(dt)

            def chain():
                call("mpn_add_softmax_rows", ops.ptr(o), n, ops.ptr(res), ops.ptr(p), B, n, 1, st)
                call("mpn_bce_mean_forward", ops.ptr(p), ops.ptr(y), B * n, ops.ptr(part), chunks, ops.ptr(out1), st)
                call("mpn_bce_mean_backward", ops.ptr(p), ops.ptr(y), ops.ptr(dp), B * n, ops.ptr(ones), st)
                call("mpn_softmax_rows_backward", ops.ptr(p), ops.ptr(dp), ops.ptr(o), n, ops.ptr(dl), B, n, st)
                if dt != torch.float32:
                    ops.cast_lowp(dl, d)

            def head():
                call("mpn_prn_head_train", ops.ptr(o), n, ops.ptr(res), ops.ptr(y), ops.ptr(ones), ops.ptr(d), B, n, n, code,
                     ops.ptr(part), ops.ptr(out1), st)
            tc, th = alternate([chain, head], 20, a.windows, 20, "events")
            say("head B=%-4d %s  chain (%d launches) %s   mpn_prn_head_train (2 launches) %s   head / chain = %.3f" % (
                B, name, 5 if dt == torch.float32 else 6, fmt(tc), fmt(th), statistics.median(th) / statistics.median(tc)))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
