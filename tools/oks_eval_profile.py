#!/usr/bin/env python
"""Device time of the three keypoint-evaluation stages (csrc/coco_eval.hip) at validation-set scale, next to the host time of the
numpy restatement (tests/oks_eval_ref.py) on a subset.

    python tools/oks_eval_profile.py --out profiles/oks_eval_stages.json [--images 5000] [--subset 200] [--reps 20]

Synthetic data from a seed: --images images, 0..5 ground truths (2.5 on average) and 6..20 detections each.  Every stage is timed
with device events around its launches, after a warm-up of the same shapes; the figure is the median over --reps, the spread is
recorded.  The rank sort of stage 3 is K^2 score compares for K kept detections; its share is reported separately."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--subset", type=int, default=200)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import oks_eval_ref as R
    from multiposenet.pytorch_amd import _lib, ops
    from multiposenet.pytorch_amd.evaluate.oks_eval import KeypointEval

    anns, res = R.random_set(11, args.images, (0, 5), (6, 20), tie_scores=False)
    ids = sorted(set(a['image_id'] for a in anns) | set(r['image_id'] for r in res))
    sub = set(ids[:args.subset])
    t0 = time.time()
    ref = R.evaluate([a for a in anns if a['image_id'] in sub], [r for r in res if r['image_id'] in sub], sorted(sub))
    host_ref_s = time.time() - t0
    ev = KeypointEval(anns)
    t0 = time.time()
    _, gsel, det_kp, det_score, tab = ev.pack(res, ids)
    pack_s = time.time() - t0
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: the stage times are device measurements (host restatement on %d images: %.2f s)" % (len(sub), host_ref_s))
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    c = ev._device_arrays(dev)
    d_kp, d_score, tab_d = torch.from_numpy(det_kp).to(dev), torch.from_numpy(det_score).to(dev), torch.from_numpy(tab).to(dev)
    T, Rn, A = len(ev.iou_thrs), len(ev.rec_thrs), len(ev.area_rng)
    out = torch.empty((T * Rn * A + T * A,), dtype=torch.float64, device=dev)
    K, G = int(tab[-1, 2]), int(tab[-1, 1])

    def stage1():
        return ops.oks_matrix(d_kp, d_score, c['gt_kp'], c['gt_area'], c['gt_bbox'], tab, tab_d, ev.max_dets, c['var'])

    kept_src, kept_score, kept_area, oks = stage1()

    def stage2():
        return ops.oks_match(oks, kept_area, c['gt_area'], c['gt_flags'], tab, tab_d, ev.max_dets, c['area_rng'], c['iou'])

    det_match, det_ig, gt_ig, gt_match = stage2()

    def stage3():
        return ops.oks_accumulate(kept_score, det_match, det_ig, gt_ig, c['rec'], out)

    order = torch.empty((K,), dtype=torch.int32, device=dev)
    ws = ops.workspace(_lib.call("mpn_oks_eval_workspace_bytes", K, A, T), dev, slot=9)

    def rank_only():           # stage 3 with one (area range, threshold): the rank sort and a thirtieth of the scans
        _lib.call("mpn_oks_accumulate", ops.ptr(kept_score), ops.ptr(det_match), ops.ptr(det_ig), ops.ptr(gt_ig), K, G, 1, 1, ops.ptr(c['rec']),
                  Rn, ops.ptr(order), ops.ptr(out), ops.ptr(out[T * Rn * A:]), ops.ptr(ws), ops.stream_ptr())

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        ms = np.asarray(ms)
        return {"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max())}

    rec = {"images": len(ids), "detections": int(tab[-1, 0]), "kept": K, "ground_truths": G, "oks_elements": int(tab[-1, 3]),
           "reps": args.reps, "library": _lib.lib().mpn_version().decode(),
           "stage1_oks_matrix": timed(stage1), "stage2_oks_match": timed(stage2), "stage3_oks_accumulate": timed(stage3),
           "stage3_rank_sort_with_one_scan": timed(rank_only), "rank_sort_compares": K * K}
    t0 = time.time()
    full = ev.evaluate(res, ids)
    rec["evaluate_wall_s_with_packing_and_uploads"] = time.time() - t0
    rec["host_pack_s"] = pack_s
    rec["stats"] = full["stats"].tolist()
    rec["host_restatement"] = {"images": len(sub), "kept": int(ref['det_match'].shape[2]), "seconds": host_ref_s}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
