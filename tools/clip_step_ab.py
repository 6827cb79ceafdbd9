#!/usr/bin/env python3
"""Cost of gradient clipping (the Trainer's max_grad_norm) on the headline training step (R101 480x480 B=32 bf16, train_both,
batch statistics, FusedAdam), variants alternated in rounds on one model:

  replay            recorded step, no clipping (what bench.py times)
  replay_clip       recorded step with the device clip, a max_norm that clips every step (1e-8)
  replay_clip_noop  recorded step with the device clip, a max_norm that never clips (1e30: coef = 1, the multiply still runs)
  eager_clip        the eager path the Trainer took before (training/trainer.py _Stepper, launch='eager'): autograd tape,
                    torch.nn.utils.clip_grad_norm_(..., inf) and its host sync, then FusedAdam.step()

Per variant and round: ms per step (host clock around K steps ending in a device synchronise) and the host time to enqueue
them.  Prints a table; --out writes it too.

    python tools/clip_step_ab.py [--steps 30] [--warmup 5] [--rounds 2] [--out profiles/r07_clip_step_ab.txt]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=101)
    ap.add_argument("--size", type=int, default=480)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--variants", default="replay,replay_clip,replay_clip_noop,eager_clip")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from bench import he_weights, synth
    from multiposenet.pytorch_amd import _lib
    from multiposenet.pytorch_amd.network import losses
    from multiposenet.pytorch_amd.network.posenet import poseNet
    from multiposenet.pytorch_amd.optim import FusedAdam
    from multiposenet.pytorch_amd.replay import ReplayedTrainStep
    from multiposenet.pytorch_amd.training.trainer import TrainParams, _Stepper

    assert torch.cuda.is_available(), "clip_step_ab.py measures on the MI355X"
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    losses.set_lazy_log(True)
    model = poseNet(args.layers, compute_dtype=torch.bfloat16).to(dev)
    for p in model.prn.parameters():
        p.requires_grad = False
    model.train()
    img, heat, wgt, anno = synth(args.batch, args.size, dev, seed=100)
    inputs, gts = [[img, "train_both"]], ["train_both", heat, wgt, anno]

    def make(variant, opt):
        if variant == "replay":
            return ReplayedTrainStep(model, opt), 2
        if variant == "replay_clip":
            return ReplayedTrainStep(model, opt, max_grad_norm=1e-8), 2
        if variant == "replay_clip_noop":
            return ReplayedTrainStep(model, opt, max_grad_norm=1e30), 2
        if variant == "eager_clip":
            return _Stepper(model, opt, TrainParams(max_grad_norm=1e-8, launch="eager")), 1
        raise ValueError(variant)

    variants = args.variants.split(",")
    rows = []
    for rnd in range(args.rounds):
        for variant in variants:
            he_weights(model)
            for p in model.parameters():
                p.grad = None
            opt = FusedAdam(model, lr=1e-4, weight_decay=0.0)
            step, setup = make(variant, opt)
            last = None
            for _ in range(setup + args.warmup):
                _, last = step(inputs, gts)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                _, last = step(inputs, gts)
            t_enq = time.perf_counter() - t0
            torch.cuda.synchronize()
            el = time.perf_counter() - t0
            mg = last.get("max_grad")
            rows.append((rnd, variant, el / args.steps * 1e3, t_enq / args.steps * 1e3, None if mg is None else float(mg)))
            print("round %d %-17s %8.3f ms/step  enqueue %7.3f ms/step  max_grad %s" % rows[-1], flush=True)
            del step, opt
            torch.cuda.synchronize()
            torch.cuda.empty_cache()

    lines = ["clip_step_ab: R%d %dx%d B=%d bf16 train_both, batch statistics, FusedAdam; %d timed steps after %d warm-up, %d rounds; %s"
             % (args.layers, args.size, args.size, args.batch, args.steps, args.warmup, args.rounds, _lib.lib().mpn_version().decode()),
             "%-17s %s   %s" % ("variant", "ms/step per round".ljust(24), "enqueue ms/step per round")]
    for variant in variants:
        ms = ["%.3f" % r[2] for r in rows if r[1] == variant]
        enq = ["%.3f" % r[3] for r in rows if r[1] == variant]
        lines.append("%-17s %s   %s" % (variant, " ".join(ms).ljust(24), " ".join(enq)))
    base = [r[2] for r in rows if r[1] == "replay"]
    if base:
        b = min(base)
        for variant in variants[1:] if variants[0] == "replay" else variants:
            v = [r[2] for r in rows if r[1] == variant]
            if v:
                lines.append("%-17s best %+.3f ms/step vs replay (best of rounds)" % (variant, min(v) - b))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
