#!/usr/bin/env python3
"""What the ``segmentations`` path of the detection loader costs next to the ``instances`` path (datasets/augment.py:
DeviceBBoxAugmenter; datasets/segm.py; csrc/segm.hip).  Synthetic batch: B = 32 samples of 480 x 480, 8 polygon instances each
(24-vertex outlines, the size of a COCO person polygon), one RLE crowd-sized instance in every fourth sample.

Reports, as one JSON line:
  * the HOST time of ``DeviceBBoxAugmenter.__call__`` on either kind of sample: a host clock around the call alone (what the
    loader's thread is busy for; the call returns when everything is enqueued) and around the call plus a device synchronise; the
    two kinds alternate, medians of ``--calls`` after warm-up.  ``--instances-module`` names another module that holds a
    DeviceBBoxAugmenter for the ``instances`` leg (a copy of an earlier revision's augment.py, to time that revision in the same run);
  * the bytes each kind uploads for the objects (the images and the geometry tables are the same for both);
  * the time of one ``rasterize_packed`` call (its allocations, the one H2D copy of the tables, two memsets, the toggle launches,
    the fill launch), median over blocks of back-to-back calls between two HIP events.  With ``--trace-calls N`` the tool only
    issues N such calls and exits: run it under ``rocprofv3 --kernel-trace --stats`` for the per-kernel times.

The dense masks of the ``instances`` leg come from the rasteriser itself (setup, not timed), so both legs describe the same objects.
There is no pass / fail threshold.  Needs the MI355X; there is no CPU path.
"""
import argparse
import importlib
import json
import math
import os
import random
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.augment_bench import time_launches  # noqa: E402


def make_batch(B, H, W, n_inst, seed):
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    img = np.stack([125 + 80 * np.sin(xx / (11.0 + 3 * c)) * np.cos(yy / (17.0 - 2 * c) - c) for c in range(3)], 2)
    samples = []
    for b in range(B):
        im = np.clip(img + rs.uniform(-25, 25, size=img.shape), 0, 255).astype(np.uint8)
        segms = []
        for _ in range(n_inst):                                        # person-sized wobbly ellipses, two decimals as in COCO
            cy, cx = rs.uniform(0.2, 0.8) * H, rs.uniform(0.2, 0.8) * W
            ry, rx = rs.uniform(0.1, 0.35) * H, rs.uniform(0.05, 0.2) * W
            poly = []
            for j in range(24):
                a, r = 2 * math.pi * j / 24, rs.uniform(0.75, 1.0)
                poly += [round(float(cx + r * rx * math.cos(a)), 2), round(float(cy + r * ry * math.sin(a)), 2)]
            segms.append([poly])
        if b % 4 == 0:                                                 # an RLE instance: a band of columns with a ragged edge
            runs, pos = [], 0
            for x in range(W // 3, W // 3 + 60):
                top, bot = int(rs.randint(40, 120)), int(rs.randint(300, 440))
                runs += [x * H + top - pos, bot - top]
                pos = x * H + bot
            segms[-1] = {"size": [H, W], "counts": runs + [H * W - pos]}
        samples.append({"img": torch.from_numpy(im), "objpos": (rs.uniform(0.2 * W, 0.8 * W), rs.uniform(0.2 * H, 0.8 * H)),
                        "scale_provided": float(rs.uniform(0.3, 1.0)), "segmentations": segms, "iscrowd": [0] * n_inst})
    return samples


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=480)
    ap.add_argument("--src", type=int, nargs=2, default=(480, 480), metavar=("H", "W"))
    ap.add_argument("--instances", type=int, default=8)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=20)
    ap.add_argument("--per-block", type=int, default=20)
    ap.add_argument("--instances-module", default=None)
    ap.add_argument("--trace-calls", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("segm_bench needs the MI355X; nothing was measured")
    from multiposenet.pytorch_amd.datasets import augment as aug, segm

    B, S, (H, W) = a.batch, a.size, a.src
    dev = torch.device("cuda", torch.cuda.current_device())
    by_segm = make_batch(B, H, W, a.instances, 1)
    pack = segm.concat_packs([segm.pack_segmentations(s["segmentations"], H, W) for s in by_segm])

    def raster():
        return segm.rasterize_packed(pack, dev)

    if a.trace_calls:
        for _ in range(a.trace_calls):
            raster()
        torch.cuda.synchronize()
        return
    by_inst = []
    for s in by_segm:
        masks = segm.rasterize_segmentations(s["segmentations"], H, W).cpu().numpy()
        assert all(m.any() for m in masks)
        by_inst.append(dict({k: v for k, v in s.items() if k != "segmentations"}, instances=list(masks)))
    rng = random.Random(1)
    dice = np.stack([aug.draw_dice(rng) for _ in range(B)])
    da_s = aug.DeviceBBoxAugmenter(S, 4, row_multiple=8)
    inst_mod = importlib.import_module(a.instances_module) if a.instances_module else aug
    da_i = inst_mod.DeviceBBoxAugmenter(S, 4, row_multiple=8)
    ref = da_i(by_inst, dice=dice)
    got = da_s(by_segm, dice=dice)
    torch.cuda.synchronize()
    same = bool(torch.equal(ref[0], got[0]) and torch.equal(ref[1], got[1]))
    host = {"instances": [], "segmentations": []}
    e2e = {"instances": [], "segmentations": []}
    for it in range(3 + a.calls):                                      # three warm-up rounds, the two kinds alternating
        for kind, da, samples in (("instances", da_i, by_inst), ("segmentations", da_s, by_segm)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            da(samples, dice=dice)
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            if it >= 3:
                host[kind].append((t1 - t0) * 1e3)
                e2e[kind].append((t2 - t0) * 1e3)
    rect_bytes = aug._aligned_offsets([r[3] * r[4] for g in ref[2] for r in g["rects"]])[1]
    h2d_segm = raster()[2]
    med, lo, hi = time_launches(raster, a.blocks, a.per_block, 3)
    # this figure includes the allocation and the one small H2D copy of every call; the per-kernel times come from the trace run
    out = {"what": "segm_raster_stages", "batch": B, "size": S, "src": [H, W], "instances_per_sample": a.instances, "n_instances": pack.n,
           "vertices": int(pack.verts.shape[0]), "outline_steps": int(pack.estart[-1]), "rle_toggles": int(pack.toggles.shape[0]),
           "bitmap_bytes": pack.words * 8, "outputs_equal": same, "calls": a.calls,
           "instances_module": a.instances_module or "this revision",
           "host_ms_instances_median": statistics.median(host["instances"]), "host_ms_segmentations_median": statistics.median(host["segmentations"]),
           "host_ms_instances_min_max": [min(host["instances"]), max(host["instances"])],
           "host_ms_segmentations_min_max": [min(host["segmentations"]), max(host["segmentations"])],
           "call_plus_sync_ms_instances_median": statistics.median(e2e["instances"]),
           "call_plus_sync_ms_segmentations_median": statistics.median(e2e["segmentations"]),
           "object_h2d_bytes_instances": int(rect_bytes), "object_h2d_bytes_segmentations": int(h2d_segm),
           "rasterize_call_ms_median_min_max": [med, lo, hi], "device": torch.cuda.get_device_name(0)}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
