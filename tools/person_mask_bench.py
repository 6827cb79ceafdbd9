#!/usr/bin/env python3
"""Person masks at inference (csrc/seg_infer.hip; Tester return_masks / seg_eval): what the three kernels cost next to the composed
chains of existing kernels they replace, and what ``return_masks`` costs the fused test-time augmentation — run on the GPU box.

Kernel legs: HIP events around each call on the stream, medians of ``--calls`` after three warm-up calls, with min .. max.
  * ``mpn_seg_masks`` at B = 64, 480 x 640 images, S = 640 (160 x 160 maps) against the composed chain per image (``resize`` to the
    D x D square, slice, compare, scale to 0 / 255) on the same maps; the masks are compared.
  * ``mpn_tta_merge_mask`` at 480 x 640 with the five scales of inp_size 480 against its composed chain (per pass and scale: slice,
    resize to the image, multiply, float64 add; then flip, add, halve, round, compare) on the same seg pair maps; masks compared.
  * ``mpn_mask_iou`` at B = 64, 480 x 640, against the composed torch expression (three boolean reductions per image).
Tester leg: the rig and alternating-window method of tools/tta_bench.py (R101 fp16, inp_size 480, synthetic 480 x 640 images) with a
``person_seg`` model: fused, pipelined images/s with and without ``return_masks``, medians of ``--windows`` windows with min .. max.
No pass / fail threshold: the numbers are the product.

    python tools/person_mask_bench.py [--calls 20] [--windows 7] [--images 6] [--out profiles/person_mask_stages.json]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch


def timed(fn, calls):
    """Median, min, max of the device time of fn() in microseconds (HIP events on the current stream)."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        t.append(e0.elapsed_time(e1) * 1e3)
    return {"median_us": float(np.median(t)), "min_us": float(min(t)), "max_us": float(max(t))}


def stat(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)), "spread": float(max(v) - min(v))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--images", type=int, default=6)
    ap.add_argument("--layers", type=int, default=101)
    ap.add_argument("--skip-tester", action="store_true")
    ap.add_argument("--out", default=os.path.join("profiles", "person_mask_stages.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("person_mask_bench needs the MI355X; nothing was measured")
    from multiposenet.pytorch_amd import _lib
    from multiposenet.pytorch_amd.evaluate import tester as T
    from multiposenet.pytorch_amd.evaluate.seg_eval import mask_iou_counts
    torch.cuda.set_device(0)
    B, H, W = a.batch, a.height, a.width
    D, thr = max(H, W), 0.5
    g = torch.Generator().manual_seed(1)
    out = {"library": _lib.lib().mpn_version().decode(), "device": torch.cuda.get_device_name(0), "calls": a.calls,
           "image": [H, W], "batch": B}

    # ---- mpn_seg_masks against resize / slice / compare, image by image
    hq = 160
    heat = torch.rand((B, 19, hq, hq), generator=g).cuda()
    sizes = [(H, W)] * B

    def chain_single():
        return [(T.resize(heat[b, 18][:, :, None], (D, D), cubic=True)[:H, :W, 0] > thr).to(torch.uint8) * 255 for b in range(B)]
    fused_masks, chain_masks = T.seg_masks(heat, sizes, thr), chain_single()
    out["seg_masks"] = {"map": [hq, hq], "fused": timed(lambda: T.seg_masks(heat, sizes, thr), a.calls), "chain": timed(chain_single, a.calls),
                        "launches_fused": 1, "launches_chain": 4 * B, "equal": all(bool(torch.equal(x, y)) for x, y in zip(fused_masks, chain_masks)),
                        "chain_intermediate_bytes_per_image": 4 * D * D + H * W + H * W}

    # ---- mpn_tta_merge_mask against its chain
    mult =[x * 480 / float(H) for x in [0.5, 1., 1.5, 2, 2.5]]
    maps = []
    for s in mult:
        _, h, w, hp, wp = T.scale_geometry(H, W, s * H, 32)
        maps.append(T.tta_seg_upsample(torch.rand((2, 19, hp // 4, wp // 4), generator=g).cuda(), min(h, hp), min(w, wp)))

    def chain_merge():
        acc = []
        for p in range(2):
            acc_p = torch.zeros((H, W, 1), dtype=torch.float64, device="cuda")
            for u in maps:
                acc_p = acc_p + T.resize(u[:, :, p:p + 1], (H, W), cubic=True) / len(maps)
            acc.append(acc_p)
        return (((acc[0] + acc[1].flip(1)) / 2.).float()[:, :, 0] > thr).to(torch.uint8) * 255
    out["tta_merge_mask"] = {"scales": len(maps), "fused": timed(lambda: T.tta_merge_mask(maps, H, W, thr), a.calls), "chain": timed(chain_merge, a.calls),
                             "launches_fused": 1, "equal": bool(torch.equal(T.tta_merge_mask(maps, H, W, thr), chain_merge())),
                             "chain_accumulator_bytes": 2 * 8 * H * W}

    # ---- mpn_mask_iou against three boolean reductions per image
    pred = (torch.rand((B, H, W), generator=g) > 0.5).to(torch.uint8).cuda() * 255
    gt = (torch.rand((B, H, W), generator=g) > 0.7).to(torch.uint8).cuda() * 255
    table = np.array([(H, W, b * H * W, W, b * H * W, W) for b in range(B)], dtype=np.int64)
    counts = torch.empty((B, 3), dtype=torch.int64, device="cuda")

    def chain_iou():
        p, q = pred != 0, gt != 0
        return torch.stack([(p & q).sum((1, 2)), p.sum((1, 2)), q.sum((1, 2))], 1)
    out["mask_iou"] = {"fused": timed(lambda: mask_iou_counts(pred.view(-1), gt.view(-1), table, out=counts), a.calls), "chain": timed(chain_iou, a.calls),
                       "equal": bool(torch.equal(mask_iou_counts(pred.view(-1), gt.view(-1), table), chain_iou())),
                       "bytes_read": 2 * B * H * W, "note": "the fused figure includes the upload of the 3 KB image table"}

    # ---- fused TTA images/s with and without return_masks
    if not a.skip_tester:
        from multiposenet.pytorch_amd import synthetic as weightgen
        from multiposenet.pytorch_amd.network.posenet import poseNet
        import bench
        m = poseNet(a.layers, compute_dtype=torch.float16, person_seg=True).cuda()
        bench.he_weights(m)
        sd = weightgen.gen_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items() if k.startswith("prn.")}, seed=3, flavour="he")
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
        m.eval()
        tp = T.TestParams()
        tp.ckpt, tp.inp_size = None, 480
        tester = T.Tester(m, tp)
        rs = np.random.RandomState(7)
        images = [rs.uniform(0, 255, (H, W, 3)).astype(np.float32) for _ in range(a.images)]
        with torch.no_grad():                                        # the calibration of tools/tta_bench.py: 8 anchors above 0.5, 4 people's worth of peaks
            img0 = T._to_device_image(images[0], tester.dev)
            im_scale, h, w, hp, wp = T.scale_geometry(H, W, tester._get_multiplier(img0)[1] * H, 32)
            _, (cls, _, _) = m([T.tta_input(img0, h, w, hp, wp, 1.0 / im_scale)[:1].contiguous(), "detection_subnet"])
            s_ = cls.float().flatten().clamp(1e-6, 1 - 1e-6)
            q = torch.topk(s_, 8).values[-1]
            m.classificationModel.output.bias.data += float(-torch.log(q / (1 - q)))
            hv = tester._tta_enqueue(img0)[1].flatten()
            qh = torch.quantile(hv[torch.randperm(hv.numel(), device=hv.device)[:2000000]], 1.0 - 4.0 * 12.0 / (H * W))
            m.convfin.bias.data[:18] += float(0.1 - qh)
        configs = {"fused_pipelined": lambda: tester.infer_images_multiscale(images),
                   "fused_pipelined_with_masks": lambda: tester.infer_images_multiscale(images, return_masks=True)}
        res = {}
        for name, fn in configs.items():
            res[name] = fn()
            torch.cuda.synchronize()
        rates = {k: [] for k in configs}
        for _ in range(a.windows):
            for name, fn in configs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                rates[name].append(a.images / (time.perf_counter() - t0))
        out["tta"] = {"setup": {"trunk": "resnet%d" % a.layers, "dtype": "float16", "inp_size": 480, "images_per_window": a.images, "windows": a.windows,
                                "people_per_image": sum(len(r) for r in res["fused_pipelined"]) / float(a.images)},
                      "results_identical": bool(res["fused_pipelined"] == res["fused_pipelined_with_masks"][0]),
                      "mask_on_share": float(torch.stack([(x != 0).float().mean() for x in res["fused_pipelined_with_masks"][1]]).mean()),
                      "images_per_s": {k: stat(v) for k, v in rates.items()}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
