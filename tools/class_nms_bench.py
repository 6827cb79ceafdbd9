#!/usr/bin/env python3
"""Stage times of the class-wise post-processing of a K-class head (ops.detect_batched_classwise) at the batch-64 inference shape:
B = 64 images of 640x640 (A = 76 725 anchors), K = 80 classes, synthetic scores with about 1 000 and about 10 000 (anchor, class)
pairs per image above the 0.05 threshold.  HIP-event medians of 20 launches for the count pass, the fill pass, the class-aware NMS and
the gathers; mpn_class_max on the same tensor is the yardstick of the two filter passes (each reads the bytes it reads once), and the
class-maximum chain (mpn_class_max + ops.detect_batched, what detect_padded runs without class_wise) the yardstick of the whole.
Run on the GPU box; --out writes the JSON (profiles/class_nms_stages.json)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from multiposenet.pytorch_amd import _lib, ops
from multiposenet.pytorch_amd._lib import call

REPS = 20


def timed(fn, reps=REPS, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms))}


def make_inputs(B, A, K, per_image, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    xy = torch.rand((B, A, 2), device="cuda", generator=g) * 600
    wh = torch.rand((B, A, 2), device="cuda", generator=g) * 180 + 16
    boxes = torch.cat([xy, xy + wh], -1).contiguous()
    cls = torch.full((B, A * K), 0.01, dtype=torch.float32, device="cuda")
    idx = torch.randint(0, A * K, (B, per_image), device="cuda", generator=g)
    cls.scatter_(1, idx, torch.rand((B, per_image), device="cuda", generator=g) * 0.9 + 0.06)
    return boxes, cls.view(B, A, K)


def run_set(B, A, K, per_image):
    boxes, cls = make_inputs(B, A, K, per_image, per_image)
    dev = cls.device
    thr, iou = 0.05, 0.5
    out = {"B": B, "A": A, "K": K, "target_candidates_per_image": per_image, "reps": REPS, "cls_bytes": cls.numel() * 4}
    score = torch.empty((B, A), dtype=torch.float32, device=dev)
    cls_id = torch.empty((B, A), dtype=torch.int64, device=dev)
    out["class_max"] = timed(lambda: call("mpn_class_max", ops.ptr(cls), B, A, K, ops.ptr(score), ops.ptr(cls_id), ops.stream_ptr()))
    table = torch.empty((call("mpn_class_filter_workspace_bytes", B, A, K) // 4,), dtype=torch.int32, device=dev)
    counts = torch.empty((B,), dtype=torch.int32, device=dev)
    out["count_pass"] = timed(lambda: call("mpn_class_filter_count", ops.ptr(cls), B, A, K, thr, ops.ptr(table), ops.ptr(counts), ops.stream_ptr()))
    cnt = counts.tolist()
    n = max(cnt)
    out["candidates_per_image"] = {"min": min(cnt), "max": n, "mean": float(np.mean(cnt))}
    out["chunks_per_image"] = table.numel() // B
    dets = torch.empty((B, n, 5), dtype=torch.float32, device=dev)
    ccls = torch.empty((B, n), dtype=torch.int32, device=dev)
    canc = torch.empty((B, n), dtype=torch.int32, device=dev)
    out["fill_pass"] = timed(lambda: call("mpn_class_filter_fill", ops.ptr(boxes), ops.ptr(cls), B, A, K, thr, ops.ptr(table), n, ops.ptr(dets), n * 5,
                                          ops.ptr(ccls), ops.ptr(canc), n, ops.ptr(counts), ops.stream_ptr()))
    keep = torch.empty((B, n), dtype=torch.int64, device=dev)
    num = torch.empty((B,), dtype=torch.int64, device=dev)
    ws_bytes = call("mpn_nms_batched_classes_workspace_bytes", B, n)
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    out["nms_workspace_bytes"] = int(ws_bytes)
    out["class_nms"] = timed(lambda: call("mpn_nms_batched_classes", ops.ptr(dets), n * 5, ops.ptr(ccls), n, ops.ptr(counts), B, n, 0, iou, 0,
                                          ops.ptr(keep), n, ops.ptr(num), ops.ptr(ws), ops.stream_ptr()))
    ob = torch.empty((B, n, 4), dtype=torch.float32, device=dev)
    osc = torch.empty((B, n), dtype=torch.float32, device=dev)
    oc = torch.empty((B, n), dtype=torch.int64, device=dev)

    def gathers():
        call("mpn_gather_dets_batched", ops.ptr(dets), n * 5, ops.ptr(keep), n, ops.ptr(num), B, n, ops.ptr(ob), ops.ptr(osc), n, ops.stream_ptr())
        call("mpn_gather_cand_class", ops.ptr(ccls), None, n, ops.ptr(keep), n, ops.ptr(num), B, n, ops.ptr(oc), None, n, ops.stream_ptr())
    out["gathers"] = timed(gathers)
    out["kept_per_image_mean"] = float(num.float().mean().item())
    # whole chains, host reads included
    out["chain_class_wise"] = timed(lambda: ops.detect_batched_classwise(boxes, cls, thr, iou, padded=True), warm=2)

    def parent():
        s, ci = ops.class_max(cls)
        return ops.detect_batched(boxes, s, thr, iou, padded=True, cls_id=ci)
    out["chain_class_max"] = timed(parent, warm=2)
    out["chain_class_max_kept_per_image_mean"] = float(np.mean(parent()[2]))
    for k in ("count_pass", "fill_pass"):
        out[k + "_over_class_max"] = out[k]["median_ms"] / out["class_max"]["median_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--anchors", type=int, default=76725)
    ap.add_argument("--classes", type=int, default=80)
    ap.add_argument("--candidates", type=int, nargs="+", default=[1000, 10000])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"library": _lib.lib().mpn_version().decode(), "chunk": call("mpn_class_filter_chunk"),
           "sets": [run_set(a.batch, a.anchors, a.classes, c) for c in a.candidates]}
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
