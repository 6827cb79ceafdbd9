#!/usr/bin/env python
"""Device time of the box-evaluation stages (csrc/coco_eval.hip) at validation-set scale, next to
the host time of the numpy restatement (tests/box_eval_ref.py) on a subset.

    python tools/box_eval_profile.py --out profiles/box_eval_stages.json [--images 5000] [--subset 50] [--reps 20]

Two synthetic sets from a seed: ``coco80`` — --images images, 80 categories of which every image shows 1..6 (low ids more often),
1..4 ground truths and 0..12 detections per (image, category) pair — and ``person`` — one category with as many detections spread
over the same images, where the whole set is ONE segment of the rank sort (K^2 compares; with 80 categories the segments share
them out).  Every stage is timed with device events around its launches, after a warm-up of the same shapes; the figure is the
median over --reps, the spread is recorded."""
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


def synthetic(seed, n_img, n_cat, per_img, n_gt, n_det):
    """Per image ``per_img`` = (lo, hi) categories out of n_cat, per pair n_gt ground truths and n_det detections (ranges)."""
    import box_eval_ref as R
    rs = np.random.RandomState(seed)
    weight = 1.0 / np.arange(1, n_cat + 1)
    weight /= weight.sum()
    anns, res = [], []
    for img in range(1, n_img + 1):
        k = min(n_cat, rs.randint(per_img[0], per_img[1] + 1))
        for c in rs.choice(n_cat, size=k, replace=False, p=weight) + 1:
            boxes = []
            for _ in range(rs.randint(n_gt[0], n_gt[1] + 1)):
                w, h = np.exp(rs.uniform(np.log(8), np.log(300), 2))
                box = [round(float(v), 2) for v in (rs.uniform(0, 632), rs.uniform(0, 472), w, h)]
                anns.append(R.ann(img, int(c), box, area=round(box[2] * box[3] * rs.uniform(.4, 1.0), 1), crowd=int(rs.uniform() < .03)))
                boxes.append(box)
            for d in range(rs.randint(n_det[0], n_det[1] + 1)):
                if d < len(boxes) and rs.uniform() < .8:
                    j, b = rs.normal(0, .08, 4), boxes[d]
                    box = [b[0] + j[0] * b[2], b[1] + j[1] * b[3], b[2] * np.exp(j[2]), b[3] * np.exp(j[3])]
                else:
                    w, h = np.exp(rs.uniform(np.log(8), np.log(300), 2))
                    box = [rs.uniform(0, 632), rs.uniform(0, 472), w, h]
                res.append(R.det(img, int(c), [round(float(v), 2) for v in box], rs.uniform(.05, 1)))
    return anns, res


def profile(name, anns, res, n_cat, args, dev):
    import box_eval_ref as R
    from multiposenet.pytorch_amd import _lib, ops
    from multiposenet.pytorch_amd.evaluate.box_eval import BoxEval
    cats = list(range(1, n_cat + 1))
    ids = sorted(set(a['image_id'] for a in anns) | set(r['image_id'] for r in res))
    sub = set(ids[:args.subset])
    t0 = time.time()
    ref = R.evaluate([a for a in anns if a['image_id'] in sub], [r for r in res if r['image_id'] in sub], sorted(sub), cats)
    host_ref_s = time.time() - t0
    ev = BoxEval(anns, categories=cats)
    t0 = time.time()
    _, rows, gsel, det_box, det_score, tab, cat_tab = ev.pack(res, ids)
    pack_s = time.time() - t0
    c = ev._device_arrays(dev)
    up = lambda a: torch.from_numpy(a).to(dev)
    d_box, d_score, tab_d, cat_tab_d = up(det_box), up(det_score), up(tab), up(cat_tab)
    md = np.asarray(ev.max_dets, dtype=np.int32)
    T, Rn, A, M, C = len(ev.iou_thrs), len(ev.rec_thrs), len(ev.area_rng), len(md), len(cats)
    out = torch.empty((T * Rn * C * A * M + T * C * A * M,), dtype=torch.float64, device=dev)
    K, G = int(tab[-1, 2]), int(tab[-1, 1])

    def stage1():
        return ops.box_iou_matrix(d_box, d_score, c['gt_box'], c['gt_flags'], tab, tab_d, ev.max_dets[-1])

    kept_src, kept_score, kept_area, kept_rank, iou = stage1()

    def stage2():
        return ops.oks_match(iou, kept_area, c['gt_area'], c['gt_flags'], tab, tab_d, ev.max_dets[-1], c['area_rng'], c['iou'])

    det_match, det_ig, gt_ig, gt_match = stage2()

    def stage3():
        return ops.box_accumulate(kept_score, kept_rank, det_match, det_ig, gt_ig, cat_tab, cat_tab_d, md, c['rec'], out)

    order = torch.empty((max(K, 1),), dtype=torch.int32, device=dev)
    ws = ops.workspace(_lib.call("mpn_box_eval_workspace_bytes", K, A, M, T), dev, slot=9)
    one = np.asarray(ev.max_dets[-1:], dtype=np.int32)
    import ctypes

    def rank_only():           # stage 3 with one (area range, maxDets entry, threshold): the segmented rank sort and 1/120 of the scans
        _lib.call("mpn_box_accumulate", ops.ptr(kept_score), ops.ptr(kept_rank), ops.ptr(det_match), ops.ptr(det_ig), ops.ptr(gt_ig),
                  ctypes.c_void_p(cat_tab.ctypes.data), ops.ptr(cat_tab_d), C, K, G, 1, 1, ctypes.c_void_p(one.ctypes.data), 1, ops.ptr(c['rec']),
                  Rn, ops.ptr(order), ops.ptr(out), ops.ptr(out[Rn * C:]), ops.ptr(ws), ops.stream_ptr())

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

    seg = np.diff(cat_tab[:, 0])
    rec = {"set": name, "images": len(ids), "categories": C, "rows": int(len(rows)), "detections": int(tab[-1, 0]), "kept": K,
           "ground_truths": G, "iou_elements": int(tab[-1, 3]), "largest_category_kept": int(seg.max()),
           "rank_sort_compares": int((seg.astype(np.float64) ** 2).sum()), "accumulate_workgroups": C * A * M * T,
           "workspace_bytes": int(_lib.call("mpn_box_eval_workspace_bytes", K, A, M, T)), "reps": args.reps,
           "stage1_box_iou_matrix": timed(stage1), "stage2_oks_match": timed(stage2), "stage3_box_accumulate": timed(stage3),
           "stage3_rank_sort_with_one_scan": timed(rank_only)}
    t0 = time.time()
    full = ev.evaluate(res, ids)
    rec["evaluate_wall_s_with_packing_and_uploads"] = time.time() - t0
    rec["host_pack_s"] = pack_s
    rec["stats"] = full["stats"].tolist()
    rec["host_restatement"] = {"images": len(sub), "kept": int(ref['det_match'].shape[2]), "seconds": host_ref_s}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--subset", type=int, default=50)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    from multiposenet.pytorch_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: the stage times are device measurements")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    rec = {"library": _lib.lib().mpn_version().decode(), "sets": []}
    coco = synthetic(11, args.images, 80, (1, 6), (1, 4), (0, 12))
    rec["sets"].append(profile("coco80", coco[0], coco[1], 80, args, dev))
    per = max(1, int(round(rec["sets"][0]["detections"] / float(args.images))))
    person = synthetic(12, args.images, 1, (1, 1), (0, 8), (max(0, per - 4), per + 4))
    rec["sets"].append(profile("person", person[0], person[1], 1, args, dev))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
