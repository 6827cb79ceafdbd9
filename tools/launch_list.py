#!/usr/bin/env python3
"""The launch list of one step, one line per entry: what the engine enqueues, on which stream, with which arguments.

``_lib.TAPE`` collects every C-ABI launch and every stream / event / collective operation of a step (replay.py re-issues that
list).  This tool prints it in a form two trees can be compared by: two revisions that print the same text enqueue the same
work in the same order on the same streams with the same aliasing between their buffers.

  * the entry-point name, or ``gpu_op:<qualname>`` (with the bound object) for a gpu_op;
  * for mpn_conv_forward / mpn_conv_wgrad*: the library's kernel name for the recorded parameter block and every field of the block;
  * integers and floats as they are;
  * pointers, streams and events as p<k>, s<k>, e<k> in order of first appearance (the last argument of an entry point is its stream).

Cases (--case): recorded (ReplayedTrainStep, the default), eager (train_step: autograd node, export / import_grad), infer ('both').

    python tools/launch_list.py --layers 50 --size 128 --batch 2 --subnet train_both --dtype bf16 [--case eager] [--out FILE] [--histogram]

Prints the entry count and the SHA-256 of the dump; --out writes the dump, --histogram the entry points by count instead.
"""
import argparse
import collections
import ctypes
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


class Names(object):
    """p<k> / s<k> / e<k> in order of first appearance."""

    def __init__(self):
        self.seen = {"p": {}, "s": {}, "e": {}}
        self.keep = []          # objects whose id() is a key

    def name(self, kind, key, obj=None):
        table = self.seen[kind]
        if key not in table:
            table[key] = "%s%d" % (kind, len(table))
            self.keep.append(obj)
        return table[key]

    def ptr(self, v):
        return "null" if not v else self.name("p", int(v))

    def value(self, a, stream=False):
        if isinstance(a, ctypes.c_void_p):
            return self.name("s", int(a.value or 0)) if stream else self.ptr(a.value)
        if isinstance(a, torch.cuda.Stream):
            return self.name("s", int(a.cuda_stream))
        if isinstance(a, torch.cuda.Event):
            return self.name("e", id(a), a)
        if isinstance(a, torch.Tensor):
            return self.ptr(a.data_ptr())
        if isinstance(a, bool) or a is None or isinstance(a, (int, float, str)):
            return repr(a)
        if isinstance(a, dict) and "start" in a and "end" in a:          # a reducer bucket
            return "bucket[%d:%d]" % (a["start"], a["end"])
        if hasattr(a, "_obj"):          # ctypes.byref(parameter block)
            return self.block(a._obj)
        if isinstance(a, ctypes.Array):
            return "[%s]" % ",".join(self.ptr(x) if a._type_ is ctypes.c_void_p else repr(x) for x in a)
        if hasattr(a, "value"):          # other ctypes scalars
            return repr(a.value)
        if callable(a):
            return "fn:" + getattr(a, "__qualname__", type(a).__name__)
        return type(a).__name__

    def block(self, p):
        out = []
        for field, ctype in p._fields_:
            v = getattr(p, field)
            if ctype is ctypes.c_void_p:
                out.append("%s=%s" % (field, self.ptr(v)))
            elif isinstance(v, ctypes.Array):
                out.append("%s=%s" % (field, self.value(v)))
            else:
                out.append("%s=%r" % (field, v))
        return "{" + " ".join(out) + "}"


def render(tape):
    from multiposenet.pytorch_amd import ops
    names = Names()
    lines = []
    for fn, args, is_c in tape:
        if is_c:
            name = fn.__name__
            parts = [name]
            if name == "mpn_conv_forward":
                parts.append(ops._kernel_name("mpn_conv_kernel_name", args[0]._obj))
            elif name.startswith("mpn_conv_wgrad"):
                parts.append(ops._kernel_name("mpn_conv_wgrad_kernel_name", args[0]._obj))
            for i, (a, ctype) in enumerate(zip(args, fn.argtypes)):
                if ctype is ctypes.c_void_p and isinstance(a, int):          # an address passed as a plain integer
                    a = ctypes.c_void_p(a)
                parts.append(names.value(a, stream=(i == len(args) - 1)))
        else:
            parts = ["gpu_op:" + getattr(fn, "__qualname__", type(fn).__name__)]
            owner = getattr(fn, "__self__", None)
            if isinstance(owner, (torch.cuda.Stream, torch.cuda.Event, torch.Tensor)):
                parts.append("self=" + names.value(owner))
            parts += [names.value(a) for a in args]
        lines.append(" ".join(parts))
    return lines


def record(args):
    import bench
    from multiposenet.pytorch_amd import _lib
    from multiposenet.pytorch_amd.network import losses
    from multiposenet.pytorch_amd.network.posenet import poseNet
    from multiposenet.pytorch_amd.optim import FusedAdam
    from multiposenet.pytorch_amd.replay import ReplayedTrainStep
    from multiposenet.pytorch_amd.training.batch_processor import train_step
    losses.set_lazy_log(True)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    torch.manual_seed(0)
    dtype = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}[args.dtype]
    m = poseNet(args.layers, compute_dtype=dtype).to(dev)
    bench.he_weights(m)
    for p in m.prn.parameters():
        p.requires_grad = False
    img, heat, wgt, anno = bench.synth(args.batch, args.size, dev, seed=100)
    if args.case == "infer":
        m.eval()
        with torch.no_grad():
            m([img, "both"])          # fills the host-side caches (anchors)
            _lib.TAPE = tape = []
            try:
                m([img, "both"])
            finally:
                _lib.TAPE = None
        torch.cuda.synchronize()
        return tape
    m.train()
    gts = {"train_both": [heat, wgt, anno], "keypoint_subnet": [heat, wgt], "detection_subnet": [anno]}[args.subnet]
    inputs, gts = [[img, args.subnet]], [args.subnet] + gts
    opt = FusedAdam(m, lr=1e-4)
    if args.case == "recorded":
        step = ReplayedTrainStep(m, opt)
        for _ in range(step.eager_steps + 1):
            step(inputs, gts)
        torch.cuda.synchronize()
        (ent,) = step._entries.values()
        return ent.tape
    train_step(m, opt, inputs, gts)
    _lib.TAPE = tape = []
    try:
        train_step(m, opt, inputs, gts)
    finally:
        _lib.TAPE = None
    torch.cuda.synchronize()
    return tape


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="recorded", choices=("recorded", "eager", "infer"))
    ap.add_argument("--layers", type=int, default=101)
    ap.add_argument("--size", type=int, default=480)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--subnet", default="train_both", choices=("train_both", "keypoint_subnet", "detection_subnet"))
    ap.add_argument("--dtype", default="bf16", choices=("bf16", "f16", "f32"))
    ap.add_argument("--out", default=None)
    ap.add_argument("--histogram", action="store_true")
    args = ap.parse_args()
    tape = record(args)
    if args.histogram:
        c = collections.Counter((fn.__name__ if is_c else "gpu_op:" + getattr(fn, "__qualname__", type(fn).__name__)) for fn, _, is_c in tape)
        for k, v in c.most_common():
            print("%6d  %s" % (v, k))
    text = "\n".join(render(tape)) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    print("entries %d sha256 %s" % (len(tape), hashlib.sha256(text.encode()).hexdigest()))


if __name__ == "__main__":
    main()
