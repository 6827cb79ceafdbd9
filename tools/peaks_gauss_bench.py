#!/usr/bin/env python3
"""Cost of the smoothed peak refinement (NMS(..., bool_gaussian_filt=True)) next to the plain one (run on the GPU box).

The two workloads of profiles/r06_peaks_microbench.txt: 64 x 18 x 160 x 160 channels-last heat-maps, factor 4, "people" (4 Gaussian
blobs per joint plane) and "noise" (uniform noise thresholded so that about 300 cells per plane are peaks).  HIP-event times of the
whole call (flags + compaction + refinement) in ALTERNATING blocks of the two forms in one process, so that clocks and cache state
drift over both alike; the median block is reported, with the spread.  No pass / fail threshold.  Optionally the host cost of the
reference's own form, scipy.ndimage.gaussian_filter on one 20 x 20 float32 patch (the reference quotes 0.8 ms per peak).

    python tools/peaks_gauss_bench.py [--blocks 9] [--iters 20] > profiles/r14_peaks_gauss_bench.txt
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from multiposenet.pytorch_amd import _lib
from multiposenet.pytorch_amd.network import joint_utils as ju


def block(pred, thre, cap, smooth, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        pk, cnt = ju._peaks_device(pred, thre, 4.0, True, cap, smooth)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000 / iters, cnt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    print("library %s on %s" % (_lib.lib().mpn_version().decode(), torch.cuda.get_device_name(0)))
    B, J, H, W = 64, 18, 160, 160
    yy, xx = torch.meshgrid(torch.arange(H, device="cuda").float(), torch.arange(W, device="cuda").float(), indexing="ij")
    gen = torch.Generator(device="cuda").manual_seed(5)
    people = torch.zeros((B, J, H, W), device="cuda")
    for _ in range(4):
        cx = torch.rand((B, J, 1, 1), device="cuda", generator=gen) * (W - 1)
        cy = torch.rand((B, J, 1, 1), device="cuda", generator=gen) * (H - 1)
        people = torch.maximum(people, torch.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * 2.5 ** 2)))
    people += 0.02 * torch.rand((B, J, H, W), device="cuda", generator=gen)
    noise = torch.rand((B, J, H, W), device="cuda", generator=gen)
    for name, t, thre in (("people (4 blobs / plane)", people, 0.1), ("noise, ~300 peaks / plane", noise, 0.988)):
        pred = t.contiguous(memory_format=torch.channels_last)
        cap = 256
        _, cnt = block(pred, thre, cap, False, 1)
        most, total = int(cnt.max()), int(cnt.sum())
        if most > cap:
            cap = 1 << (most - 1).bit_length()
        for smooth in (False, True):                                  # warm-up of both forms
            block(pred, thre, cap, smooth, 3)
        times = {False: [], True: []}
        for _ in range(a.blocks):
            for smooth in (False, True):
                times[smooth].append(block(pred, thre, cap, smooth, a.iters)[0])
        med = {k: float(np.median(v)) for k, v in times.items()}
        print("64x18x160x160 channels_last f=4 %s: %d peaks (max %d / plane), cap %d, %d alternating blocks of %d calls" % (name, total, most, cap, a.blocks, a.iters))
        for smooth in (False, True):
            v = times[smooth]
            print("    %-8s median %9.1f us/call   (min %9.1f, max %9.1f)" % ("smoothed" if smooth else "plain", med[smooth], min(v), max(v)))
        print("    smoothed / plain = %.2f;  extra cost per peak = %.2f ns" % (med[True] / med[False], (med[True] - med[False]) * 1000.0 / max(total, 1)))
    try:
        from scipy.ndimage import gaussian_filter
    except ImportError:
        print("host form: scipy is not installed")
        return
    patch = np.random.RandomState(0).uniform(0, 1, (20, 20)).astype(np.float32)
    for _ in range(100):
        gaussian_filter(patch, sigma=3)
    n = 5000
    t0 = time.perf_counter()
    for _ in range(n):
        gaussian_filter(patch, sigma=3)
    print("host form: scipy.ndimage.gaussian_filter(20x20 float32, sigma=3) %.1f us per peak (one core)" % ((time.perf_counter() - t0) / n * 1e6))


if __name__ == "__main__":
    main()
