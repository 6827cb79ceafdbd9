#!/usr/bin/env python3
"""What building ``mask_miss`` on the device from ``person_anns`` costs next to handing ``DeviceAugmenter`` ready ``mask_miss``
planes (datasets/augment.py; datasets/segm.py: mask_miss_batch; csrc/segm.hip).  Synthetic batch: B = 32 images of 480 x 640,
8 person annotations each (24-vertex outlines, the size of a COCO person polygon), among them one without keypoints and one RLE
crowd, the crowd in the middle of the list so that the people before it are rasterised and the people after it are dropped.

Reports, as one JSON line:
  * the HOST time of ``DeviceAugmenter.__call__`` on either kind of sample: a host clock around the call alone (what the loader's
    thread is busy for; the call returns when everything is enqueued) and around the call plus a device synchronise; the two kinds
    alternate, medians of ``--calls`` after warm-up.  ``--planes-module`` names another module that holds a DeviceAugmenter for the
    ``mask_miss`` leg (a copy of an earlier revision's augment.py, to time that revision in the same run);
  * the bytes each kind uploads for the masks (the images, joints and geometry tables are the same for both);
  * with ``--trace-calls N`` the tool only issues N ``mask_miss_batch`` calls and exits: run it under
    ``rocprofv3 --kernel-trace --stats`` for the per-kernel times; ``--summarise DB`` prints the medians of the segm kernels of such
    a run's rocpd database.

The planes of the ``mask_miss`` leg come from ``mask_miss_batch`` itself (setup, not timed), so both legs describe the same masks
and their outputs are compared.  There is no pass / fail threshold.  Needs the MI355X; there is no CPU path.
"""
import argparse
import importlib
import json
import os
import random
import sqlite3
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.segm_bench import make_batch  # noqa: E402


def make_samples(B, H, W, n_ann, seed):
    rs = np.random.RandomState(seed + 100)
    samples = []
    for s in make_batch(B, H, W, n_ann, seed):
        segms = [g for g in s["segmentations"] if not isinstance(g, dict)]
        while len(segms) < n_ann:                                      # make_batch turns one polygon into an RLE in every fourth sample
            segms.append(segms[0])
        runs, pos = [], 0                                              # the crowd: a band of columns with a ragged edge
        for x in range(W // 3, W // 3 + 90):
            top, bot = int(rs.randint(40, 120)), int(rs.randint(300, 440))
            runs += [x * H + top - pos, bot - top]
            pos = x * H + bot
        anns = [{"segmentation": g, "iscrowd": 0, "num_keypoints": 9} for g in segms]
        anns[1]["num_keypoints"] = 0
        anns[n_ann // 2] = {"segmentation": {"size": [H, W], "counts": runs + [H * W - pos]}, "iscrowd": 1, "num_keypoints": 0}
        j = np.zeros((17, 3))
        j[:, 0], j[:, 1], j[:, 2] = rs.uniform(0, W, 17), rs.uniform(0, H, 17), rs.choice([0.0, 1.0, 2.0], 17)
        samples.append({"img": s["img"], "objpos": s["objpos"], "scale_provided": s["scale_provided"], "joint_self": j,
                        "person_anns": anns})
    return samples


def summarise(db):
    cur = sqlite3.connect(db).cursor()
    rows = cur.execute("select name, (end - start) / 1e3 from kernels").fetchall()
    out = {}
    for name in sorted(set(r[0] for r in rows)):
        if "segm_" in name or "fillBuffer" in name:
            t = sorted(r[1] for r in rows if r[0] == name)
            short = name.replace("(anonymous namespace)::", "").split("(")[0]
            out[short] = {"dispatches": len(t), "us_median_min_max": [statistics.median(t), t[0], t[-1]]}
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=480)
    ap.add_argument("--src", type=int, nargs=2, default=(480, 640), metavar=("H", "W"))
    ap.add_argument("--annotations", type=int, default=8)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--planes-module", default=None)
    ap.add_argument("--trace-calls", type=int, default=0)
    ap.add_argument("--summarise", default=None, metavar="DB")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    if a.summarise:
        return summarise(a.summarise)
    if not torch.cuda.is_available():
        raise SystemExit("mask_miss_bench needs the MI355X; nothing was measured")
    from multiposenet.pytorch_amd.datasets import augment as aug, segm

    B, S, (H, W) = a.batch, a.size, a.src
    by_anns = make_samples(B, H, W, a.annotations, 1)
    lists, sizes = [s["person_anns"] for s in by_anns], [(H, W)] * B
    if a.trace_calls:
        for _ in range(a.trace_calls):
            segm.mask_miss_batch(lists, sizes)
        torch.cuda.synchronize()
        return
    pack, kinds, imgs, offsets, nbytes = segm.pack_mask_miss_batch(lists, sizes)
    buf = segm.mask_miss_batch(lists, sizes)[0].cpu()
    by_plane = []
    for s, off in zip(by_anns, offsets):
        plane = buf[off: off + H * W].view(H, W).clone()
        assert bool((plane == 0).any()) and bool((plane == 255).any())
        by_plane.append(dict({k: v for k, v in s.items() if k != "person_anns"}, mask_miss=plane))
    rng = random.Random(1)
    dice = np.stack([aug.draw_dice(rng) for _ in range(B)])
    da_a = aug.DeviceAugmenter(S, 4)
    da_p = (importlib.import_module(a.planes_module) if a.planes_module else aug).DeviceAugmenter(S, 4)
    ref = da_p(by_plane, dice=dice)
    got = da_a(by_anns, dice=dice)
    torch.cuda.synchronize()
    same = all(bool(torch.equal(x, y)) for x, y in zip(ref[:3], got[:3]))
    host = {"mask_miss": [], "person_anns": []}
    e2e = {"mask_miss": [], "person_anns": []}
    for it in range(3 + a.calls):                                      # three warm-up rounds, the two kinds alternating
        for kind, da, samples in (("mask_miss", da_p, by_plane), ("person_anns", da_a, by_anns)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            da(samples, dice=dice)
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            if it >= 3:
                host[kind].append((t1 - t0) * 1e3)
                e2e[kind].append((t2 - t0) * 1e3)
    t_pack = []
    for _ in range(a.calls):
        t0 = time.perf_counter()
        segm.pack_mask_miss_batch(lists, sizes)
        t_pack.append((time.perf_counter() - t0) * 1e3)
    h2d_anns = sum((x.nbytes + 7) // 8 * 8 for x in (pack.insts, pack.parts, pack.verts, pack.vpart, pack.estart, pack.toggles, imgs, kinds))
    out = {"what": "mask_miss_stages", "batch": B, "size": S, "src": [H, W], "annotations_per_image": a.annotations,
           "n_instances_rasterised": pack.n, "kinds_rasterised": [int((kinds == k).sum()) for k in range(3)],
           "vertices": int(pack.verts.shape[0]), "outline_steps": int(pack.estart[-1]), "rle_toggles": int(pack.toggles.shape[0]),
           "bitmap_bytes": pack.words * 8, "outputs_equal": same, "calls": a.calls, "planes_module": a.planes_module or "this revision",
           "host_ms_mask_miss_median": statistics.median(host["mask_miss"]), "host_ms_person_anns_median": statistics.median(host["person_anns"]),
           "host_ms_mask_miss_min_max": [min(host["mask_miss"]), max(host["mask_miss"])],
           "host_ms_person_anns_min_max": [min(host["person_anns"]), max(host["person_anns"])],
           "call_plus_sync_ms_mask_miss_median": statistics.median(e2e["mask_miss"]),
           "call_plus_sync_ms_person_anns_median": statistics.median(e2e["person_anns"]),
           "host_ms_pack_mask_miss_batch_median": statistics.median(t_pack),
           "mask_h2d_bytes_mask_miss": int(aug._aligned_offsets([H * W] * B)[1]), "mask_h2d_bytes_person_anns": int(h2d_anns),
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
