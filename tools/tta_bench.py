#!/usr/bin/env python3
"""Multi-scale + flip test-time augmentation: the unfused Tester.infer_image_multiscale against the fused, flip-paired path
(infer_images_multiscale, csrc/tta.hip) — run on the GPU box.

R101, fp16, inp_size 480, synthetic 480 x 640 images (random weights; the detector bias shifted so that a few people per image pass
0.5: the post-processing load of a COCO image, not of noise).  The three configurations — unfused, fused with pipeline=False, fused with pipeline=True — run in ALTERNATING windows in one
process, so that clocks and cache state drift over all alike; images/s is the median window, with the window-to-window spread
(max - min) of each.  One further instrumented pass of the fused path brackets its sections with HIP events on the stream: device
time per image in the network, the input kernels, the x4 up-sampling and the merge, and the host time of enqueueing an image and of
finishing it (detections, peaks, PRN assignment with their reads).  No pass / fail threshold: the numbers are the product.

    python tools/tta_bench.py [--windows 7] [--images 6] [--out profiles/tta_fused_stages.json]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--images", type=int, default=6)
    ap.add_argument("--layers", type=int, default=101)
    ap.add_argument("--inp-size", type=int, default=480)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--people", type=int, default=8, help="anchors of the first image above 0.5 at scale index 1, before NMS")
    ap.add_argument("--joints", type=float, default=4.0, help="people's worth of cells above 0.1 per joint plane of the first image's averaged maps")
    ap.add_argument("--out", default=os.path.join("profiles", "tta_fused_stages.json"))
    a = ap.parse_args()
    assert a.windows >= 5
    from multiposenet.pytorch_amd import _lib, synthetic as weightgen
    from multiposenet.pytorch_amd.evaluate import tester as T
    from multiposenet.pytorch_amd.network.posenet import poseNet
    import bench
    torch.cuda.set_device(0)
    m = poseNet(a.layers, compute_dtype=torch.float16).cuda()
    bench.he_weights(m)
    sd = weightgen.gen_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items() if k.startswith("prn.")}, seed=3, flavour="he")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    m.eval()
    tp = T.TestParams()
    tp.ckpt, tp.inp_size = None, a.inp_size
    tester = T.Tester(m, tp)
    rs = np.random.RandomState(7)
    images = [rs.uniform(0, 255, (a.height, a.width, 3)).astype(np.float32) for _ in range(a.images)]
    names, ids = ["s%d.jpg" % i for i in range(a.images)], list(range(a.images))
    with torch.no_grad():
        # calibrate the detector's output bias on the input whose boxes are used (scale index 1 of the first image): a uniform logit
        # shift that puts the a.people-th best anchor at 0.5
        img0 = T._to_device_image(images[0], tester.dev)
        im_scale, h, w, hp, wp = T.scale_geometry(a.height, a.width, tester._get_multiplier(img0)[1] * a.height, 32)
        _, (cls, _, _) = m([T.tta_input(img0, h, w, hp, wp, 1.0 / im_scale)[:1].contiguous(), "detection_subnet"])
        s_ = cls.float().flatten().clamp(1e-6, 1 - 1e-6)
        q = torch.topk(s_, int(a.people)).values[-1]
        m.classificationModel.output.bias.data += float(-torch.log(q / (1 - q)))
        # ... and the keypoint head's output bias, so that about 12 cells per person and joint plane of the first image's AVERAGED maps
        # exceed the peak threshold 0.1 (random weights give noise maps: thousands of peaks per image for the host to walk, or, once
        # ten passes are averaged, none).  A bias shift moves every resized and averaged value by the same amount.
        hv = tester._tta_enqueue(img0)[1].flatten()
        qh = torch.quantile(hv[torch.randperm(hv.numel(), device=hv.device)[:2000000]], 1.0 - a.joints * 12.0 / (a.height * a.width))
        m.convfin.bias.data += float(0.1 - qh)

    configs = {
        "unfused": lambda: [tester.infer_image_multiscale(images[i], names[i], ids[i]) for i in range(a.images)],
        "fused_serial": lambda: tester.infer_images_multiscale(images, names, ids, pipeline=False),
        "fused_pipelined": lambda: tester.infer_images_multiscale(images, names, ids, pipeline=True),
    }
    results = {}
    for name, fn in configs.items():                                 # warm-up of every form (conv plans, allocator pools)
        results[name] = fn()
        torch.cuda.synchronize()
    same = results["unfused"] == results["fused_serial"] == results["fused_pipelined"]
    joints = float(np.mean([len(T.get_joint_list(item[0], {'thre1': 0.1}, item[1], 1)) for item in [tester._tta_enqueue(im) for im in images[:2]]]))
    rates = {k: [] for k in configs}
    for _ in range(a.windows):
        for name, fn in configs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            rates[name].append(a.images / (time.perf_counter() - t0))

    # ---- instrumented pass of the fused path: sections bracketed by events on the stream (not part of the windows above)
    marks = {"network": [], "input": [], "upsample": [], "merge": []}
    host = {"enqueue": [], "finish": []}

    def bracket(key, fn):
        def wrapped(*args, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(*args, **kw)
            e1.record()
            marks[key].append((e0, e1))
            return out
        return wrapped
    split = {"detections": [], "peaks": [], "prn": []}

    def clocked(key, fn):
        def wrapped(*args, **kw):
            t0 = time.perf_counter()
            out = fn(*args, **kw)
            split[key].append((time.perf_counter() - t0) * 1e3)
            return out
        return wrapped
    saved = (T.tta_input, T.tta_upsample, T.tta_merge, m.forward_heat, m.forward_padded_begin, T.get_joint_list)
    m.detect_padded, T.get_joint_list, tester.prn_process = clocked("detections", m.detect_padded), clocked("peaks", T.get_joint_list), clocked("prn", tester.prn_process)
    T.tta_input, T.tta_upsample, T.tta_merge = bracket("input", saved[0]), bracket("upsample", saved[1]), bracket("merge", saved[2])
    m.forward_heat, m.forward_padded_begin = bracket("network", saved[3]), bracket("network", saved[4])
    try:
        for i in range(a.images):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            item = tester._tta_enqueue(images[i])
            t1 = time.perf_counter()
            tester._tta_finish(item, names[i], ids[i])
            torch.cuda.synchronize()
            host["enqueue"].append((t1 - t0) * 1e3)
            host["finish"].append((time.perf_counter() - t1) * 1e3)
    finally:
        T.tta_input, T.tta_upsample, T.tta_merge = saved[:3]
        T.get_joint_list = saved[5]
        del m.forward_heat, m.forward_padded_begin, m.detect_padded, tester.prn_process
    torch.cuda.synchronize()
    device_ms = {k: sum(e0.elapsed_time(e1) for e0, e1 in v) / a.images for k, v in marks.items()}

    def stat(v):
        return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)), "spread": float(max(v) - min(v))}
    out = {
        "library": _lib.lib().mpn_version().decode(), "device": torch.cuda.get_device_name(0),
        "setup": {"trunk": "resnet%d" % a.layers, "dtype": "float16", "inp_size": a.inp_size, "image": [a.height, a.width],
                  "images_per_window": a.images, "windows": a.windows, "people_per_image": sum(len(r) for r in results["unfused"]) / float(a.images), "joints_per_image": joints},
        "results_identical": bool(same),
        "images_per_s": {k: stat(v) for k, v in rates.items()},
        "fused_device_ms_per_image": device_ms,
        "fused_host_ms_per_image": {"enqueue": float(np.median(host["enqueue"])), "finish_incl_waiting": float(np.median(host["finish"])),
                                    "finish_split": {k: float(np.median(v)) for k, v in split.items()}},
        "unfused_host_ms_per_image": 1e3 / float(np.median(rates["unfused"])),
    }
    u, f = out["images_per_s"]["unfused"], out["images_per_s"]["fused_pipelined"]
    out["fused_pipelined_over_unfused"] = f["median"] / u["median"]
    out["beats_unfused_by_more_than_the_larger_spread"] = bool(f["median"] - u["median"] > max(f["spread"], u["spread"]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
