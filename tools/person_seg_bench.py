#!/usr/bin/env python3
"""Cost of the person-segmentation channel: the recorded train_both step with and without ``mask_all``, and the two new launches
next to their ``mask_miss`` counterparts.

    python tools/person_seg_bench.py [--out profiles/person_seg_step.json]

On an MI355X, the README's headline configuration: poseNet(101), 480 x 480, 32 images, bf16, batch-statistics BatchNorm,
train_both through replay.ReplayedTrainStep.

  * step: host-clock time per step over windows of steps that end in a device synchronise, after warm-up; for ``person_seg`` False
    and True, windows of the step without ``mask_all`` and with it alternate inside one process (tools/prn_step_bench.py's scheme).
    Both run the one-pass loss kernel, the second in its seg-aware instantiation.
  * launches: HIP-event time per call, blocks alternating, tables uploaded beforehand: mpn_segm_mask_miss against
    mpn_segm_person_masks (each: workspace memset, toggle launches, compose launch) on 32 synthetic 480 x 640 images with 8
    annotations each, in two batches: "crowd last" (a crowd closes every list, so pack_mask_miss drops nobody and both entry points
    get the same tables) and "no crowd" (as most COCO images: mask_miss rasterises the keypoint-less people only, mask_all
    everyone); the whole host calls (packing and upload included) next to them; mpn_augment_mask against mpn_augment_plane on a
    [32, ., 120, 120] grid.
Nothing is gated on these numbers."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from prn_step_bench import alternate  # noqa: E402


def stats(t):
    return {"median_us": statistics.median(t), "min_us": min(t), "max_us": max(t), "windows": len(t)}


def device_call(segm, ops, call, lists, sizes, two):
    """The entry point alone on tables uploaded once -> a closure that issues its launches (memset, toggles, compose)."""
    dev = torch.device("cuda", torch.cuda.current_device())
    pack, kinds, imgs, offsets, nbytes = segm.pack_mask_miss_batch(lists, sizes, keep_all=two)
    outs = [torch.empty((nbytes + 15) // 16 * 16, dtype=torch.uint8, device=dev) for _ in range(2 if two else 1)]
    (insts, parts, verts, vpart, estart, toggles, d_imgs, d_kinds), _ = segm._upload(pack, dev, (imgs, kinds))
    ws = torch.empty(int(call("mpn_segm_workspace_bytes", pack.words)), dtype=torch.uint8, device=dev)
    n, npt, nv, nt = pack.n, int(pack.parts.shape[0]), int(pack.verts.shape[0]), int(pack.toggles.shape[0])
    args = [ops.ptr(d_imgs), int(imgs.shape[0]), ops.ptr(insts) if n else None, ops.ptr(d_kinds) if n else None, n,
            ops.ptr(parts) if npt else None, npt, ops.ptr(verts) if nv else None, ops.ptr(vpart) if nv else None, ops.ptr(estart), nv,
            int(pack.estart[-1]), ops.ptr(toggles) if nt else None, nt, int(imgs[:, segm.M_W].max()), int(imgs[:, segm.M_H].max())] \
        + [ops.ptr(o) for o in outs] + [outs[0].numel(), ops.ptr(ws), ws.numel(), ops.stream_ptr()]
    name = "mpn_segm_person_masks" if two else "mpn_segm_mask_miss"
    keep = (outs, insts, parts, verts, vpart, estart, toggles, d_imgs, d_kinds, ws)
    return (lambda: call(name, *args)), n, keep


def person_annotations(rs, H, W, n, crowds=True):
    """n person annotations of one image: polygons; every fourth has no keypoints, and with ``crowds`` every fourth (the last one
    among them) is a crowd."""
    anns = []
    for i in range(n):
        cx, cy, r = rs.uniform(0.2, 0.8) * W, rs.uniform(0.2, 0.8) * H, rs.uniform(0.05, 0.25) * min(H, W)
        ang = np.sort(rs.uniform(0, 2 * np.pi, 24))
        rad = r * rs.uniform(0.6, 1.0, 24)
        poly = np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], 1).round(2).reshape(-1).tolist()
        anns.append({"segmentation": [poly], "iscrowd": 1 if crowds and i % 4 == 3 else 0, "num_keypoints": 0 if i % 4 == 1 else 9})
    return anns


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--per-window", type=int, default=8)
    ap.add_argument("--layers", type=int, default=101)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=480)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("person_seg_bench needs the MI355X: there is nothing to time on a CPU")
    from multiposenet.pytorch_amd import _lib, ops, synthetic as weightgen
    from multiposenet.pytorch_amd._lib import call
    from multiposenet.pytorch_amd.datasets import augment as aug, segm
    from multiposenet.pytorch_amd.network.posenet import poseNet
    from multiposenet.pytorch_amd.optim import FusedAdam
    from multiposenet.pytorch_amd.replay import ReplayedTrainStep

    res = {"library": _lib.lib().mpn_version().decode(), "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "config": {"layers": a.layers, "batch": a.batch, "size": a.size, "dtype": "bf16", "subnet": "train_both"}, "step": {}, "launches": {}}
    B, S = a.batch, a.size
    img = torch.from_numpy(weightgen.gen_images(7, B, S, S)).cuda()
    heat, wgt = (torch.from_numpy(x).cuda() for x in weightgen.gen_keypoint_gt(8, B, S // 4, S // 4))
    anno = torch.from_numpy(weightgen.gen_boxes_gt(9, B, S)).cuda()
    mask = (torch.rand((B, 1, S // 4, S // 4), generator=torch.Generator().manual_seed(3)) > 0.6).float().cuda()
    for person_seg in (False, True):
        m = poseNet(a.layers, compute_dtype=torch.bfloat16, person_seg=person_seg).cuda()
        shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
        sd = weightgen.gen_state_dict(shapes, seed=0, flavour="he", skip_prefixes=("prn.",))
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
        for p in m.prn.parameters():
            p.requires_grad = False
        m.train()
        opt = FusedAdam(m, lr=1e-5)
        step = ReplayedTrainStep(m, opt)
        inputs = [[img, "train_both"]]
        plain, seg = ["train_both", heat, wgt, anno], ["train_both", heat, wgt, anno, mask]
        for g in (plain, seg):
            for _ in range(2):                                   # the eager pass and the recording
                step(inputs, g)
        t0, t1 = alternate([lambda: step(inputs, plain), lambda: step(inputs, seg)], a.per_window, a.windows, a.per_window, "host")
        key = "person_seg=%s" % person_seg
        res["step"][key] = {"without_mask_all": stats(t0), "with_mask_all": stats(t1),
                            "with / without": statistics.median(t1) / statistics.median(t0)}
        print("step %s: without %.1f us, with mask_all %.1f us, ratio %.4f" % (key, statistics.median(t0), statistics.median(t1),
                                                                               statistics.median(t1) / statistics.median(t0)), flush=True)
        for k in list(step._entries):
            step._drop(k)
        del step, opt, m
        torch.cuda.empty_cache()

    # ---- the two launches against their mask_miss counterparts
    rs = np.random.RandomState(1)
    H, W = 480, 640
    sizes = [(H, W)] * B
    for tag, crowds in (("crowd last", True), ("no crowd", False)):
        lists = [person_annotations(rs, H, W, 8, crowds) for _ in range(B)]
        f1, n1, k1 = device_call(segm, ops, call, lists, sizes, False)
        f2, n2, k2 = device_call(segm, ops, call, lists, sizes, True)
        tm, tb = alternate([f1, f2], 20, a.windows, 20, "events")
        res["launches"]["%s: mpn_segm_mask_miss, %d instances rasterised (device)" % (tag, n1)] = stats(tm)
        res["launches"]["%s: mpn_segm_person_masks, %d instances rasterised (device)" % (tag, n2)] = stats(tb)
        tm, tb = alternate([lambda: segm.mask_miss_batch(lists, sizes), lambda: segm.person_masks_batch(lists, sizes)], 5, a.windows, 3, "events")
        res["launches"]["%s: mask_miss_batch (host pack + upload + launches)" % tag] = stats(tm)
        res["launches"]["%s: person_masks_batch (host pack + upload + launches)" % tag] = stats(tb)
        del k1, k2
    miss, every, offs = segm.person_masks_batch(lists, sizes)
    da = aug.DeviceAugmenter(S, 4)
    samples = [{"img": torch.zeros((H, W, 3), dtype=torch.uint8), "objpos": (0.5 * W, 0.5 * H), "scale_provided": 0.6,
                "joint_self": np.ones((17, 3)), "person_anns": lists[b]} for b in range(B)]
    metas = da.geometry(samples, rng=__import__("random").Random(2))
    table = torch.from_numpy(np.stack([aug.table_row(g, H, W, 0, W * 3, off, W) for g, off in zip(metas, offs)])).cuda()
    grid = S // 4
    tw, tp = alternate([lambda: aug.augment_mask(miss, table, grid, grid, 4, S), lambda: aug.augment_plane(every, table, grid, grid, 4, S, 0.0)],
                       20, a.windows, 20, "events")
    res["launches"]["mpn_augment_mask [32,18,120,120]"] = stats(tw)
    res["launches"]["mpn_augment_plane [32,1,120,120]"] = stats(tp)
    for k, v in res["launches"].items():
        print("%-86s %9.1f us [%.1f .. %.1f]" % (k, v["median_us"], v["min_us"], v["max_us"]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
