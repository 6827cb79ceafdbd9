#!/usr/bin/env python3
"""Timing of the device augmentation (datasets/augment.py) at the benchmark batch: B = 32, 480 x 480 from 640 x 480 sources.

Reports, as one JSON line:
  * the three device stages separately — mpn_augment_image, mpn_augment_mask, mpn_gt_heatmaps — each as the median over blocks of
    back-to-back launches between two HIP events (per-launch time = block time / launches per block), on data already resident;
  * their sum against the budget of 3 % of the training step (--step-ms, default the 36.06 ms of profiles/r06_bench.json);
  * the whole DeviceAugmenter call (host geometry, packing into pinned staging, three H2D copies, the launches) as the median of a
    host clock around calls that end in a device synchronise;
  * the traffic floor computed from the shapes: every source byte read once, every output byte written once, over the HBM peak.

Needs the MI355X; there is no CPU path.
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12          # bytes/s, MI355X


def make_batch(B, H, W, seed):
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    samples = []
    for b in range(B):
        img = np.stack([125 + 80 * np.sin(xx / (11.0 + 3 * c) + b) * np.cos(yy / (17.0 - 2 * c) - c) for c in range(3)], 2)
        img += rs.uniform(-25, 25, size=img.shape)
        mask = np.full((H, W), 255, dtype=np.uint8)
        mask[rs.randint(0, H // 2):H // 2 + rs.randint(0, H // 2), rs.randint(0, W // 2):W // 2] = 0
        n = int(rs.randint(0, 6))
        j = np.zeros((1 + n, 17, 3))
        j[..., 0], j[..., 1] = rs.uniform(0, W, (1 + n, 17)), rs.uniform(0, H, (1 + n, 17))
        j[..., 2] = rs.choice([0.0, 1.0, 2.0], (1 + n, 17))
        samples.append({"img": torch.from_numpy(np.clip(img, 0, 255).astype(np.uint8)), "mask_miss": torch.from_numpy(mask),
                        "objpos": (rs.uniform(0.2 * W, 0.8 * W), rs.uniform(0.2 * H, 0.8 * H)),
                        "scale_provided": float(rs.uniform(0.3, 1.0)), "joint_self": j[0], "joint_others": j[1:]})
    return samples


def time_launches(fn, blocks, per_block, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(blocks):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(per_block):
            fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / per_block)
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=480)
    ap.add_argument("--stride", type=int, default=4)
    ap.add_argument("--src", type=int, nargs=2, default=(480, 640), metavar=("H", "W"))
    ap.add_argument("--blocks", type=int, default=200)
    ap.add_argument("--per-block", type=int, default=20)
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--step-ms", type=float, default=36.06)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("augment_bench needs the MI355X; nothing was measured")
    from multiposenet.pytorch_amd.datasets import augment as aug
    from multiposenet.pytorch_amd.datasets.heatmap import put_gaussian_maps

    B, S, H, W = a.batch, a.size, a.src[0], a.src[1]
    samples = make_batch(B, H, W, 1)
    rng = random.Random(1)
    dice = np.stack([aug.draw_dice(rng) for _ in range(B)])
    da = aug.DeviceAugmenter(S, a.stride)
    grid = S // a.stride

    # resident copies of exactly what one call uploads
    metas = da.geometry(samples, dice)
    ioff, moff, rows = 0, 0, []
    for g in metas:
        rows.append(aug.table_row(g, H, W, ioff, W * 3, moff, W))
        ioff += H * W * 3
        moff += H * W
    d_img = torch.cat([s["img"].view(-1) for s in samples]).cuda()
    d_mask = torch.cat([s["mask_miss"].view(-1) for s in samples]).cuda()
    d_table = torch.from_numpy(np.stack(rows)).cuda()
    maxP = max(1 + g["joint_others_out"].shape[0] for g in metas)
    joints = np.zeros((B, maxP, 18, 3))
    num = np.zeros(B, dtype=np.int32)
    for b, g in enumerate(metas):
        n = g["joint_others_out"].shape[0]
        joints[b, 0], joints[b, 1:1 + n], num[b] = g["joint_self_out"], g["joint_others_out"], 1 + n
    d_joints, d_num = torch.from_numpy(joints).cuda(), torch.from_numpy(num).cuda()

    stages = {
        "augment_image_ms": lambda: aug.augment_image(d_img, d_table, S, S),
        "augment_mask_ms": lambda: aug.augment_mask(d_mask, d_table, grid, grid, a.stride, S),
        "gt_heatmaps_ms": lambda: put_gaussian_maps(d_joints, d_num, S, S, a.stride, 7.0),
    }
    res = {"batch": B, "size": S, "src": [H, W], "stride": a.stride}
    total = 0.0
    for name, fn in stages.items():
        med, lo, hi = time_launches(fn, a.blocks, a.per_block, 20)
        res[name] = round(med, 5)
        res[name.replace("_ms", "_range_ms")] = [round(lo, 5), round(hi, 5)]
        total += med
    res["device_total_ms"] = round(total, 5)
    res["budget_ms"] = round(0.03 * a.step_ms, 4)
    res["within_budget"] = bool(total <= 0.03 * a.step_ms)

    for _ in range(3):
        da(samples, dice=dice)
    torch.cuda.synchronize()
    wall = []
    for _ in range(a.calls):
        t0 = time.perf_counter()
        da(samples, dice=dice)
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    res["whole_call_ms"] = round(statistics.median(wall), 3)
    res["whole_call_range_ms"] = [round(min(wall), 3), round(max(wall), 3)]
    t0 = time.perf_counter()
    for _ in range(a.calls):
        da.geometry(samples, dice)
    res["host_geometry_ms"] = round((time.perf_counter() - t0) * 1e3 / a.calls, 3)

    src_bytes = B * H * W * 4
    out_bytes = B * (3 * S * S + 2 * 18 * grid * grid) * 4
    res["traffic_bytes"] = src_bytes + out_bytes
    res["h2d_bytes"] = src_bytes + d_table.numel() * 8 + d_joints.numel() * 8 + B * 4
    res["traffic_floor_ms"] = round((src_bytes + out_bytes) / HBM_PEAK * 1e3, 5)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if res["within_budget"] else 1


if __name__ == "__main__":
    sys.exit(main())
