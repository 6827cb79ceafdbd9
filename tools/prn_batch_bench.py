#!/usr/bin/env python3
"""Time the device rendering of PRN training batches (mpn_prn_train_maps) next to the eager PRN training step.

    python tools/prn_batch_bench.py [--out profiles/r07_prn_batch_bench.txt]

On an MI355X, for B = 8, 64 and 256 at coeff 2, on a seeded synthetic annotation set (images of 1..8 people):
  * device time of the ONE launch, by HIP events around blocks of launches on resident inputs (median over blocks, after warm-up);
  * host-clock time of a whole DevicePRNBatcher call (pack + copy + launch), the device drained at the end of every block;
  * the eager 'prn_subnet' training step (forward, BCE, backward, FusedAdam over the PRN's parameters) on the same batch, fp32 and
    bf16, by HIP events, so that the data share of a step is a ratio of two measured times.
Nothing is gated on these numbers.  There is no earlier device implementation to compare against; the host figure quoted in the
output (the reference's get_data under real scikit-image) was taken once on a build machine and is labelled as such.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def synthetic_annotations(n_img, seed=7):
    rs = np.random.RandomState(seed)
    anns = []
    for im in range(n_img):
        for _ in range(int(rs.randint(1, 9))):
            x, y, w, h = rs.uniform(0, 500), rs.uniform(0, 300), rs.uniform(20, 140), rs.uniform(60, 180)
            kp = np.zeros((17, 3))
            kp[:, 0], kp[:, 1] = x + w * rs.uniform(-0.1, 1.1, 17), y + h * rs.uniform(-0.1, 1.1, 17)
            kp[:, 2] = rs.choice([0, 1, 2], 17, p=[0.2, 0.3, 0.5])
            anns.append({"bbox": [x, y, w, h], "keypoints": np.round(kp, 2).reshape(-1).tolist(), "image_id": im, "iscrowd": 0,
                         "num_keypoints": int((kp[:, 2] > 0).sum())})
    return anns


def event_blocks(fn, per_block, blocks, warmup):
    """Median, min, max over `blocks` of (HIP-event time of `per_block` calls) / per_block, in microseconds."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(blocks):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(per_block):
            fn()
        b.record()
        b.synchronize()
        t.append(a.elapsed_time(b) * 1e3 / per_block)
    return statistics.median(t), min(t), max(t)


def host_blocks(fn, per_block, blocks, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(blocks):
        t0 = time.perf_counter()
        for _ in range(per_block):
            fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e6 / per_block)
    return statistics.median(t), min(t), max(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--blocks", type=int, default=21)
    ap.add_argument("--sizes", type=int, nargs="+", default=[8, 64, 256])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("prn_batch_bench needs the MI355X: there is nothing to time on a CPU")
    from multiposenet.pytorch_amd import _lib
    from multiposenet.pytorch_amd.datasets import DevicePRNBatcher, PRNSampleSet
    from multiposenet.pytorch_amd.network.posenet import poseNet
    from multiposenet.pytorch_amd.optim import FusedAdam
    from multiposenet.pytorch_amd.training.batch_processor import train_step

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    ss = PRNSampleSet(synthetic_annotations(400))
    bt = DevicePRNBatcher()
    say("# prn_batch_bench: library %s, device %s, torch %s" % (_lib.lib().mpn_version().decode(), torch.cuda.get_device_name(0), torch.__version__))
    say("# %d samples of %d annotations, coeff 2 (56 x 36 x 17 float32 x 2 tensors = %.3f MB written per sample); medians over %d blocks [min .. max]"
        % (len(ss), ss.bbox.shape[0], 2 * 56 * 36 * 17 * 4 / 1e6, a.blocks))
    say("# host reference, not measured here: the reference's get_data under scikit-image 0.18.3, one CPU thread of a build machine, "
        "six synthetic samples in one run: 2.6 ms per sample")
    model = poseNet(50, compute_dtype=torch.float32).cuda()
    for n, p in model.named_parameters():
        p.requires_grad = n.startswith("prn.")
    model.train()
    opt = FusedAdam(model, lr=1e-4)
    rs = np.random.RandomState(1)
    for B in a.sizes:
        idx = rs.permutation(len(ss))[:B].tolist()
        stage, _, P = bt.pack(ss, idx)
        packed = stage.cuda()
        inp, lab, err = bt.launch(packed, B, P)
        torch.cuda.synchronize()
        assert not err.any()
        k = max(20, 2000 // B)
        dev = event_blocks(lambda: bt.launch(packed, B, P), k, a.blocks, 2 * k)
        host = host_blocks(lambda: bt(ss, idx), k, a.blocks, k)
        say("B=%-4d P=%-5d launch (device, events): %8.1f us [%.1f .. %.1f]   %.2f us/sample   %.1f GB/s written" % (
            B, P, dev[0], dev[1], dev[2], dev[0] / B, B * 2 * 56 * 36 * 17 * 4 / dev[0] / 1e3))
        say("B=%-4d         batcher call (host clock, drained per block of %d): %8.1f us [%.1f .. %.1f]   %.2f us/sample" % (
            B, k, host[0], host[1], host[2], host[0] / B))
        for dt, name in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
            model.compute_dtype = dt
            ks = 10
            st = event_blocks(lambda: train_step(model, opt, [[inp, "prn_subnet"]], ["prn_subnet", lab]), ks, a.blocks, 2 * ks)
            say("B=%-4d         eager prn_subnet train step %s (device, events): %8.1f us [%.1f .. %.1f]   launch / step = %.4f" % (
                B, name, st[0], st[1], st[2], dev[0] / st[0]))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
