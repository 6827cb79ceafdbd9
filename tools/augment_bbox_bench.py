#!/usr/bin/env python3
"""Timing of the detection loader's device augmentation (datasets/augment.py: DeviceBBoxAugmenter) at the benchmark batch: B = 32,
480 x 480 from 640 x 480 sources, 5 instances per image.  Sibling of tools/augment_bench.py, same method.

Reports, as one JSON line:
  * mpn_augment_boxes on resident data as the median over blocks of back-to-back calls between two HIP events: the scan launch
    alone (the entry point with n_rows = 0 issues only that launch), both launches, and their difference as the finalize launch;
    next to mpn_augment_image measured in the same run;
  * the whole DeviceBBoxAugmenter call (host geometry, the np.any scans, packing into pinned staging, three H2D copies, the three
    launches) as the median of a host clock around calls that end in a device synchronise, and the host geometry + scans alone;
  * the bytes: rectangles uploaded against full masks, the partial records.

There is no pass / fail threshold: the output is the figure DESIGN.md section 3 quotes.  Needs the MI355X; there is no CPU path.
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

from tools.augment_bench import time_launches  # noqa: E402


def make_batch(B, H, W, n_inst, seed):
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    img = np.stack([125 + 80 * np.sin(xx / (11.0 + 3 * c)) * np.cos(yy / (17.0 - 2 * c) - c) for c in range(3)], 2)
    samples = []
    for b in range(B):
        im = np.clip(img + rs.uniform(-25, 25, size=img.shape), 0, 255).astype(np.uint8)
        masks = []
        for _ in range(n_inst):                                        # person-sized ellipses
            cy, cx = rs.uniform(0.2, 0.8) * H, rs.uniform(0.2, 0.8) * W
            ry, rx = rs.uniform(0.1, 0.35) * H, rs.uniform(0.05, 0.2) * W
            masks.append((((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 < 1.0).astype(np.uint8))
        samples.append({"img": torch.from_numpy(im), "objpos": (rs.uniform(0.2 * W, 0.8 * W), rs.uniform(0.2 * H, 0.8 * H)),
                        "scale_provided": float(rs.uniform(0.3, 1.0)), "instances": masks, "iscrowd": [0] * n_inst})
    return samples


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=480)
    ap.add_argument("--src", type=int, nargs=2, default=(480, 640), metavar=("H", "W"))
    ap.add_argument("--instances", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=100)
    ap.add_argument("--per-block", type=int, default=20)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("augment_bbox_bench needs the MI355X; nothing was measured")
    from multiposenet.pytorch_amd import ops
    from multiposenet.pytorch_amd._lib import call
    from multiposenet.pytorch_amd.datasets import augment as aug

    B, S, H, W = a.batch, a.size, a.src[0], a.src[1]
    samples = make_batch(B, H, W, a.instances, 1)
    rng = random.Random(1)
    dice = np.stack([aug.draw_dice(rng) for _ in range(B)])
    da = aug.DeviceBBoxAugmenter(S, 4, row_multiple=8)
    metas = da.geometry(samples, dice)

    # resident copies of exactly what one call uploads
    rows, irows, rects, rowmap = [], [], [], []
    ioff = roff = 0
    N = (max(len(g["rects"]) for g in metas) + 7) // 8 * 8
    for b, g in enumerate(metas):
        rows.append(aug.table_row(g, H, W, ioff, W * 3))
        ioff += H * W * 3
        rm = [-1] * N
        for r, (m, rx0, ry0, rw, rh) in enumerate(g["rects"]):
            row = np.zeros(aug.TB_COLS)
            row[:aug.T_COLS] = aug.table_row(g, H, W, 0, 0, roff, rw)
            row[aug.TB_RX0:] = (rx0, ry0, rw, rh)
            rm[r] = len(irows)
            irows.append(row)
            rects.append(torch.from_numpy(np.ascontiguousarray(m[ry0:ry0 + rh, rx0:rx0 + rw])).view(-1))
            roff += rw * rh
        rowmap += rm
    d_img = torch.cat([s["img"].view(-1) for s in samples]).cuda()
    d_table = torch.from_numpy(np.stack(rows)).cuda()
    d_rect = torch.cat(rects).cuda()
    d_itable = torch.from_numpy(np.stack(irows)).cuda()
    d_rowmap = torch.tensor(rowmap, dtype=torch.int32).cuda()
    n_inst = len(irows)
    ws_bytes = int(call("mpn_augment_boxes_workspace_bytes", n_inst, S, S))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    out = torch.empty((B, N, 5), dtype=torch.float32, device="cuda")

    def boxes(n_rows):
        call("mpn_augment_boxes", ops.ptr(d_rect), d_rect.numel(), ops.ptr(d_itable), n_inst, ops.ptr(d_rowmap), n_rows, ops.ptr(out), S, S,
             ops.ptr(ws), ops.stream_ptr())

    res = {"batch": B, "size": S, "src": [H, W], "instances_per_image": a.instances, "rows": n_inst, "N": N}
    for name, fn in (("augment_image_ms", lambda: aug.augment_image(d_img, d_table, S, S)),
                     ("box_scan_ms", lambda: boxes(0)), ("box_scan_plus_finalize_ms", lambda: boxes(B * N))):
        med, lo, hi = time_launches(fn, a.blocks, a.per_block, 20)
        res[name] = round(med, 5)
        res[name.replace("_ms", "_range_ms")] = [round(lo, 5), round(hi, 5)]
    res["box_finalize_ms_by_difference"] = round(res["box_scan_plus_finalize_ms"] - res["box_scan_ms"], 5)

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
    res["host_geometry_and_scans_ms"] = round((time.perf_counter() - t0) * 1e3 / a.calls, 3)

    res["rect_bytes"] = int(d_rect.numel())
    res["full_mask_bytes"] = n_inst * H * W
    res["partial_bytes"] = ws_bytes
    res["frame_pixels_per_instance"] = (S + 1) * (S + 1)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
