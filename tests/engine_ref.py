"""Sections, configurations, references, seed table and checks of the engine tier: the backward COMPOSITION of
multiposenet/pytorch_amd/engine.py (which launch carries which statistics, which gradient is deferred, which parameter is reported
when) against the project's oracle in float64, per trainable set and BatchNorm mode.  Shared by tests/test_engine_parity_gpu.py (the
comparison) and tests/test_engine_parity_cpu.py (conditions on the reference alone, and teeth).  Test-side only; plain torch on the
CPU.  The arithmetic is the oracle's (oracle/posenet_oracle.py): this file composes its functions section by section, as the two
teacher-forced bf16 tests do, and never restates them.

A SECTION is a piece of R50 that the engine runs through its own composition method on leaf inputs and given output gradients:

  S1            stem -> max-pool -> layer1.0 (projection shortcut) -> layer1.1 (identity shortcut); image [2, 3, 16, 12]
  S2 / S3 / S4  layerL.0 (projection, stride 2) -> layerL.1 (identity); inputs [2, 256, 6, 5], [2, 512, 5, 4], [2, 1024, 4, 3]
  S5            layer4.2 -> keypoint pyramid AND detection pyramid; leaves [2, 2048, 2, 1], c4 [2, 1024, 4, 2], c3 [2, 512, 8, 4],
                c2 [2, 256, 16, 8]
  S6            keypoint head with the intermediate heads on four 256-channel leaves at 16x8, 8x4, 4x2, 2x1
  S7K1 / S7K3   detection head on five 256-channel leaves (8x4, 4x2, 2x1, 1x1, 1x1), K = 1 / K = 3 classes

Every level of those is exactly twice the next.  The ODD sections run the same composition (parameters, units, trainable sets,
configurations, routes and exact properties are those of their BASE section: ``base``) at the sizes an image that is no multiple of
32 gives, where the top-down up-sample goes to the lateral's exact size (factor not 2), conv6 / conv7 give ceil-sized levels and the
max-pool windows hang over the edges.  Detection path only: the reference's keypoint head needs exact x2 / x4 / x8 maps.

  S1o           S1 on an image [2, 3, 19, 13]: stem 10x7, pool 5x4
  S5o           S5 on the stage sizes of a 75x40 image: leaves [2, 2048, 3, 2], c4 [2, 1024, 5, 3], c3 [2, 512, 10, 5],
                c2 [2, 256, 19, 10]; up-samples 3->5->10->19 by 2->3->5->10; p6 2x1, p7 1x1
  S7K1o         S7K1 on the five levels S5o's detection pyramid gives: 10x5, 5x3, 3x2, 2x1, 1x1 (74 cells, 666 anchors per image)

A CONFIGURATION is a trainable set plus a BatchNorm mode (CONFIGS).  S6 / S7 hold no BatchNorm layer, so A (batch statistics) and C
(BatchNorm affine frozen) are the same run as B there and are not listed twice.

fp32 measure, per tensor:  e = max|T - T64| / max|T64|  over EVERY element; allowance 16 x the same measure of the same oracle run
in float32 on the CPU (the yardstick), clamped below at 4 * 2^-24.  No element is excluded, which is possible because the stored
seeds satisfy the MARGIN CONDITION (margins): every ReLU input of the float64 run is at least 16 x its tensor's float32 deviation
away from zero, every max-pool window's two largest values are at least that far apart.  One max-pool clause follows from the ReLU
clause instead of the gap: a window whose maximum is the ReLU's exact zero (every input robustly negative) ties by construction in
every arithmetic, and whichever position receives its gradient, the ReLU behind it multiplies that gradient by zero."""
import contextlib

import numpy as np
import torch
import torch.nn.functional as F

from helpers import report

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
FACTOR = 16.0
FLOOR = 4.0 * 2.0 ** -24
BF16_GATES = {"out": 2e-3, "dx": 3e-2, "dx_towers": 8e-2, "dw": 5e-2}       # the gates of the two teacher-forced bf16 tests, unchanged

SECTIONS = ("S1", "S2", "S3", "S4", "S5", "S6", "S7K1", "S7K3", "S1o", "S5o", "S7K1o")
_BASE = {"S1o": "S1", "S5o": "S5", "S7K1o": "S7K1"}
B = 2


def base(section):
    """The section whose composition ``section`` runs: itself, or for an odd-size section the one it re-sizes."""
    return _BASE.get(section, section)


def _with_odd(table):
    """``table`` (keyed by section) with every odd-size section given its base section's entry."""
    table.update({o: table[b] for o, b in _BASE.items() if b in table})
    return table


# ------------------------------------------------------------------------------------------------ parameters of a section
def _bn_names(p, c):
    return [(p + ".weight", (c,)), (p + ".bias", (c,)), (p + ".running_mean", (c,)), (p + ".running_var", (c,))]


def _block(p, cin, planes, down):
    out = [(p + ".conv1.weight", (planes, cin, 1, 1))] + _bn_names(p + ".bn1", planes)
    out += [(p + ".conv2.weight", (planes, planes, 3, 3))] + _bn_names(p + ".bn2", planes)
    out += [(p + ".conv3.weight", (4 * planes, planes, 1, 1))] + _bn_names(p + ".bn3", 4 * planes)
    if down:
        out += [(p + ".downsample.0.weight", (4 * planes, cin, 1, 1))] + _bn_names(p + ".downsample.1", 4 * planes)
    return out


def _conv(p, cout, cin, k):
    return [(p + ".weight", (cout, cin, k, k)), (p + ".bias", (cout,))]


def _tower(p, cout):
    out = []
    for i in (1, 2, 3, 4):
        out += _conv("%s.conv%d" % (p, i), 256, 256, 3)
    return out + _conv(p + ".output", cout, 256, 3)


def section_shapes(section):
    """Ordered state-dict entries (name, shape) the section reads."""
    section = base(section)
    if section == "S1":
        return [("fpn.conv1.weight", (64, 3, 7, 7))] + _bn_names("fpn.bn1", 64) + _block("fpn.layer1.0", 64, 64, True) \
            + _block("fpn.layer1.1", 256, 64, False)
    if section in ("S2", "S3", "S4"):
        L = int(section[1])
        planes = 64 * 2 ** (L - 1)
        return _block("fpn.layer%d.0" % L, 2 * planes, planes, True) + _block("fpn.layer%d.1" % L, 4 * planes, planes, False)
    if section == "S5":
        out = _block("fpn.layer4.2", 2048, 512, False)
        out += _conv("fpn.toplayer", 256, 2048, 1) + _conv("fpn.flatlayer1", 256, 1024, 1) + _conv("fpn.flatlayer2", 256, 512, 1)
        out += _conv("fpn.flatlayer3", 256, 256, 1) + _conv("fpn.smooth1", 256, 256, 3) + _conv("fpn.smooth2", 256, 256, 3)
        out += _conv("fpn.smooth3", 256, 256, 3) + _conv("fpn.conv6", 256, 2048, 3) + _conv("fpn.conv7", 256, 256, 3)
        out += _conv("fpn.latlayer1", 256, 2048, 1) + _conv("fpn.latlayer2", 256, 1024, 1) + _conv("fpn.latlayer3", 256, 512, 1)
        return out + _conv("fpn.toplayer0", 256, 256, 3) + _conv("fpn.toplayer1", 256, 256, 3) + _conv("fpn.toplayer2", 256, 256, 3)
    if section == "S6":
        out = []
        for i in (2, 3, 4, 5):
            out += _conv("convfin_k%d" % i, 19, 256, 1)
        for i in (1, 2, 3, 4):
            out += _conv("convt%d" % i, 128, 256, 3) + _conv("convs%d" % i, 128, 128, 3)
        return out + _conv("conv2", 256, 512, 3) + _conv("convfin", 18, 256, 1)
    if section in ("S7K1", "S7K3"):
        return _tower("regressionModel", 36) + _tower("classificationModel", 9 * num_classes(section))
    raise KeyError(section)


def num_classes(section):
    return 3 if base(section) == "S7K3" else 1


def is_stat(name):
    return name.endswith(("running_mean", "running_var"))


def is_bn_affine(name):
    return (".bn" in name or "downsample.1" in name) and not is_stat(name)


def param_names(section):
    return [n for n, _ in section_shapes(section) if not is_stat(n)]


def has_bn(section):
    return base(section) in ("S1", "S2", "S3", "S4", "S5")


def gen_state(section, dtype=F64):
    """The section's entries of the 'he' state dict (synthetic.gen_param, seed 0: what test_model_gpu.load_he loads), in ``dtype``."""
    from multiposenet.pytorch_amd import synthetic
    return {n: torch.from_numpy(synthetic.gen_param(0, n, s, "he")).to(dtype) for n, s in section_shapes(section)}


# ------------------------------------------------------------------------------------------------ configurations
CONFIGS = {
    #      trainable   statistics   leaf inputs need grad
    "A": ("all", "batch", True),
    "B": ("all", "frozen", True),
    "C": ("conv", "frozen", True),
    "D": ("last", "frozen", False),
    "E": ("first", "frozen", True),
    "F": ("none", "frozen", True),
    "G": ("all", "frozen", True),          # ... and some outputs get no gradient (G_VARIANTS)
}
G_VARIANTS = _with_odd({"S5": ("kp", "det"), "S6": ("pred",), "S7K1": ("reg", "cls"), "S7K3": ("reg", "cls")})

_UNITS = {
    "S1": (("fpn.conv1.", "fpn.bn1."), ("fpn.layer1.1.",)),
    "S2": (("fpn.layer2.0.",), ("fpn.layer2.1.",)),
    "S3": (("fpn.layer3.0.",), ("fpn.layer3.1.",)),
    "S4": (("fpn.layer4.0.",), ("fpn.layer4.1.",)),
    "S5": (("fpn.layer4.2.",), ("fpn.smooth1.", "fpn.smooth2.", "fpn.smooth3.", "fpn.toplayer0.", "fpn.toplayer1.", "fpn.toplayer2.",
                                "fpn.conv7.")),
    "S6": (("convt1.", "convt2.", "convt3.", "convt4."), ("conv2.", "convfin.")),
    "S7K1": (("regressionModel.conv1.", "classificationModel.conv1."), ("regressionModel.output.", "classificationModel.output.")),
}
_UNITS["S7K3"] = _UNITS["S7K1"]
_with_odd(_UNITS)


def trainable_set(section, cfg):
    """Names of the section's parameters with requires_grad under configuration ``cfg``."""
    kind = CONFIGS[cfg][0]
    names = param_names(section)
    if kind == "all":
        return set(names)
    if kind == "conv":
        return {n for n in names if not is_bn_affine(n)}
    if kind == "none":
        return set()
    first, last = _UNITS[section]
    return {n for n in names if n.startswith(first if kind == "first" else last)}


def batch_stats(cfg):
    return CONFIGS[cfg][1] == "batch"


def leaf_grad(cfg):
    return CONFIGS[cfg][2]


def apply_config(model, section, cfg):
    """Put ``model`` (anything with named_parameters / train / freeze_bn) into configuration ``cfg`` for ``section``: every parameter
    outside the trainable set — the other sections' as well — is frozen."""
    want = trainable_set(section, cfg)
    for n, p in model.named_parameters():
        p.requires_grad = n in want
    model.train()
    if not batch_stats(cfg):
        model.freeze_bn()


# ------------------------------------------------------------------------------------------------ case table
# Seeds: the first seed (from 0) at which the float64 run of (section, statistics) satisfies the margin condition — find_seed;
# tests/test_engine_parity_cpu.py asserts every entry.  bf16 runs the same inputs rounded to bf16 (no margin condition applies there).
SEEDS = {
    ("S1", "batch"): 5, ("S1", "frozen"): 3,
    ("S2", "batch"): 5, ("S2", "frozen"): 0,
    ("S3", "batch"): 0, ("S3", "frozen"): 1,
    ("S4", "batch"): 1, ("S4", "frozen"): 0,
    ("S5", "batch"): 3, ("S5", "frozen"): 0,
    ("S6", "frozen"): 0,
    ("S7K1", "frozen"): 36, ("S7K3", "frozen"): 11,
    ("S1o", "batch"): 8, ("S1o", "frozen"): 0,
    ("S5o", "batch"): 2, ("S5o", "frozen"): 1,
    ("S7K1o", "frozen"): 216,
}


def _case_table():
    rows = []
    for dtype in ("fp32", "bf16"):
        for s in SECTIONS:
            for cfg in "ABCDEFG":
                if cfg in "AC" and not has_bn(s):
                    continue          # no BatchNorm layer in the section: the same run as B
                if cfg == "A" and dtype == "bf16":
                    continue          # the two teacher-forced bf16 tests are this configuration
                variants = G_VARIANTS.get(s, ()) if cfg == "G" else (None,)
                for v in variants:
                    rows.append((dtype, s, cfg, v))
    return rows


CASES = _case_table()


def case_id(case):
    dtype, s, cfg, v = case
    return "%s-%s-%s%s" % (dtype, s, cfg, "-" + v if v else "")


def case_seed(case):
    return SEEDS[(case[1], CONFIGS[case[2]][1])]


# ------------------------------------------------------------------------------------------------ inputs
_LEAVES = {
    "S1": ((3, 16, 12),),
    "S2": ((256, 6, 5),), "S3": ((512, 5, 4),), "S4": ((1024, 4, 3),),
    "S5": ((2048, 2, 1), (1024, 4, 2), (512, 8, 4), (256, 16, 8)),          # input of layer4.2, c4, c3, c2
    "S6": ((256, 16, 8), (256, 8, 4), (256, 4, 2), (256, 2, 1)),
    "S7K1": ((256, 8, 4), (256, 4, 2), (256, 2, 1), (256, 1, 1), (256, 1, 1)),
    "S1o": ((3, 19, 13),),
    "S5o": ((2048, 3, 2), (1024, 5, 3), (512, 10, 5), (256, 19, 10)),
    "S7K1o": ((256, 10, 5), (256, 5, 3), (256, 3, 2), (256, 2, 1), (256, 1, 1)),
}
_LEAVES["S7K3"] = _LEAVES["S7K1"]


def _half(n):
    """Extent after a stride-2 layer whose padding is half its kernel (7x7 / 3, 3x3 / 1, the max-pool): ceil(n / 2)."""
    return (n + 1) // 2


def out_shapes(section):
    """Output shapes, from the section's leaves (the sizes the layers of its base section give at any extent)."""
    leaves, kind = _LEAVES[section], base(section)
    if kind == "S1":          # stem (stride 2), max-pool (stride 2), layer1
        _, h, w = leaves[0]
        return [(256, _half(_half(h)), _half(_half(w)))]
    if kind in ("S2", "S3", "S4"):
        c, h, w = leaves[0]
        return [(2 * c, _half(h), _half(w))]
    if kind == "S5":          # fp2s, fp3s, fp4s, fp5, p3s, p4s, p5s, p6, p7: each level has its lateral's size, p6 / p7 halve c5 (ceil)
        (_, h5, w5), (_, h4, w4), (_, h3, w3), (_, h2, w2) = leaves
        h6, w6 = _half(h5), _half(w5)
        return [(256, h2, w2), (256, h3, w3), (256, h4, w4), (256, h5, w5), (256, h3, w3), (256, h4, w4), (256, h5, w5), (256, h6, w6),
                (256, _half(h6), _half(w6))]
    if kind == "S6":          # k2, k3, k4, k5 (API tensors at the output resolution), pred
        _, h, w = leaves[0]
        return [(19, h, w)] * 4 + [(18, h, w)]
    cells = sum(h * w for _, h, w in leaves)
    return [("A", 9 * cells, num_classes(section)), ("A", 9 * cells, 4)]          # cls [B, A, K], reg [B, A, 4]


OUT_NAMES = _with_odd({
    "S1": ("c2",), "S2": ("out",), "S3": ("out",), "S4": ("out",),
    "S5": ("fp2s", "fp3s", "fp4s", "fp5", "p3s", "p4s", "p5s", "p6", "p7"),
    "S6": ("k2", "k3", "k4", "k5", "pred"), "S7K1": ("cls", "reg"), "S7K3": ("cls", "reg"),
})


def outputs_with_gradient(section, variant):
    """Indices of the section outputs that receive a gradient (all, or the G case's subset)."""
    n = len(OUT_NAMES[section])
    if variant is None:
        return list(range(n))
    return {"kp": [0, 1, 2, 3], "det": [4, 5, 6, 7, 8], "pred": [4], "cls": [0], "reg": [1]}[variant]


def gen_inputs(section, seed, dtype=F32):
    """(leaves, output gradients) as float32 CPU tensors holding values of ``dtype`` (so that every arithmetic sees the same operands).
    Backbone feature leaves are post-ReLU (as in the network); the head gradients of S6 / S7 are float32 API tensors in any dtype."""
    g = torch.Generator().manual_seed(100003 * SECTIONS.index(section) + seed)
    leaves = []
    for shp in _LEAVES[section]:
        x = torch.randn(B, *shp, generator=g)
        if base(section) in ("S2", "S3", "S4", "S5"):
            x = torch.relu(x)
        leaves.append(x.to(dtype).float())
    grads = []
    for shp in out_shapes(section):
        full = (B,) + tuple(shp[1:]) if shp[0] == "A" else (B,) + tuple(shp)
        d = torch.randn(*full, generator=g) * 0.05
        grads.append(d if base(section) in ("S6", "S7K1", "S7K3") else d.to(dtype).float())
    return leaves, grads


# ------------------------------------------------------------------------------------------------ shim around the oracle's torch calls
class Fault(object):
    """A modelled fault: a substitution for single calls of the oracle run.  Each hook returns None to leave the call alone."""

    def relu(self, i, v, orig):
        return None

    def batch_norm(self, i, args, kwargs, orig):
        return None

    def conv2d(self, i, args, kwargs, orig, sd):
        return None

    def interpolate(self, i, args, kwargs, orig):
        return None

    def sigmoid(self, i, v, orig):
        return None


class Shim(object):
    """While entered, F.relu / F.max_pool2d / F.batch_norm / F.conv2d / F.interpolate / torch.sigmoid — the oracle looks them up at call
    time — record their inputs (``relu``, ``pool``: detached) and let ``fault`` substitute single calls."""

    def __init__(self, fault=None, sd=None):
        self.fault, self.sd = fault, sd
        self.relu, self.pool = [], []
        self.n = {}

    def _count(self, k):
        i = self.n.get(k, 0)
        self.n[k] = i + 1
        return i

    def __enter__(self):
        self.saved = (F.relu, F.max_pool2d, F.batch_norm, F.conv2d, F.interpolate, torch.sigmoid)
        o_relu, o_pool, o_bn, o_conv, o_int, o_sig = self.saved
        ft = self.fault

        def relu(v, *a, **k):
            i = self._count("relu")
            self.relu.append(v.detach())
            r = ft.relu(i, v, o_relu) if ft is not None else None
            return o_relu(v, *a, **k) if r is None else r

        def max_pool2d(v, *a, **k):
            self._count("pool")
            self.pool.append((v.detach(), a, k))
            return o_pool(v, *a, **k)

        def batch_norm(*a, **k):
            i = self._count("bn")
            r = ft.batch_norm(i, a, k, o_bn) if ft is not None else None
            return o_bn(*a, **k) if r is None else r

        def conv2d(*a, **k):
            i = self._count("conv")
            r = ft.conv2d(i, a, k, o_conv, self.sd) if ft is not None else None
            return o_conv(*a, **k) if r is None else r

        def interpolate(*a, **k):
            i = self._count("interp")
            r = ft.interpolate(i, a, k, o_int) if ft is not None else None
            return o_int(*a, **k) if r is None else r

        def sigmoid(v):
            i = self._count("sigmoid")
            r = ft.sigmoid(i, v, o_sig) if ft is not None else None
            return o_sig(v) if r is None else r
        F.relu, F.max_pool2d, F.batch_norm, F.conv2d, F.interpolate, torch.sigmoid = relu, max_pool2d, batch_norm, conv2d, interpolate, sigmoid
        return self

    def __exit__(self, *exc):
        F.relu, F.max_pool2d, F.batch_norm, F.conv2d, F.interpolate, torch.sigmoid = self.saved


# ------------------------------------------------------------------------------------------------ the oracle, section by section
def oracle_forward(section, sd, xs, bn_train):
    """The section through the oracle's own functions -> list of outputs in OUT_NAMES order (NCHW; S7: [B, A, K] / [B, A, 4])."""
    from oracle import posenet_oracle as po
    xs = [po._q(x) for x in xs]
    section = base(section)
    if section == "S1":
        c1 = po._q(F.relu(po._bn(sd, "fpn.bn1", po._conv(sd, "fpn.conv1", xs[0], stride=2, padding=3), bn_train)))
        c1 = F.max_pool2d(c1, kernel_size=3, stride=2, padding=1)
        c = po.bottleneck(sd, "fpn.layer1.0", c1, 1, True, bn_train)
        return [po.bottleneck(sd, "fpn.layer1.1", c, 1, False, bn_train)]
    if section in ("S2", "S3", "S4"):
        p = "fpn.layer%s" % section[1]
        c = po.bottleneck(sd, p + ".0", xs[0], 2, True, bn_train)
        return [po.bottleneck(sd, p + ".1", c, 1, False, bn_train)]
    if section == "S5":
        x, c4, c3, c2 = xs
        c5 = po.bottleneck(sd, "fpn.layer4.2", x, 1, False, bn_train)
        fp5 = po._conv(sd, "fpn.toplayer", c5)
        fp4 = po.upsample_add(fp5, po._conv(sd, "fpn.flatlayer1", c4))
        fp3 = po.upsample_add(fp4, po._conv(sd, "fpn.flatlayer2", c3))
        fp2 = po.upsample_add(fp3, po._conv(sd, "fpn.flatlayer3", c2))
        kp = [po._conv(sd, "fpn.smooth3", fp2, padding=1), po._conv(sd, "fpn.smooth2", fp3, padding=1),
              po._conv(sd, "fpn.smooth1", fp4, padding=1), fp5]
        p6 = po._conv(sd, "fpn.conv6", c5, stride=2, padding=1)
        p7 = po._conv(sd, "fpn.conv7", F.relu(p6), stride=2, padding=1)
        p5 = po._conv(sd, "fpn.latlayer1", c5)
        p4 = po.upsample_add(p5, po._conv(sd, "fpn.latlayer2", c4))
        p3 = po.upsample_add(p4, po._conv(sd, "fpn.latlayer3", c3))
        return kp + [po._conv(sd, "fpn.toplayer2", p3, padding=1), po._conv(sd, "fpn.toplayer1", p4, padding=1),
                     po._conv(sd, "fpn.toplayer0", p5, padding=1), p6, p7]
    if section == "S6":
        return po.keypoint_head(sd, xs, True)[1]
    K = num_classes(section)
    cls = torch.cat([po.classification_model(sd, f, K) for f in xs], dim=1)
    reg = torch.cat([po.regression_model(sd, f) for f in xs], dim=1)
    return [cls, reg]


def run_oracle(section, seed, dtype, bn_train, variant=None, fault=None, state=None, quant=None, conv2_classes=False, times=1):
    """One forward + backward of the section in ``dtype`` (F64: the reference; F32: the yardstick) with every parameter and every leaf
    asking for a gradient.  ``quant``: run under the oracle's storage-rounding model (the bf16 reference; dtype F32).  ``state``:
    name -> tensor to use instead of gen_state.  -> dict(outs, leaf_grads, param_grads, running, relu, pool); a gradient is None where
    nothing flowed (the G cases).  ``times``: that many identical passes, their parameter gradients summed (the accumulation cases)."""
    from oracle import posenet_oracle as po
    src = state if state is not None else gen_state(section, F32)
    sd = {n: v.detach().to(dtype).clone() for n, v in src.items()}
    names = [n for n in sd if not is_stat(n)]
    for n in names:
        sd[n].requires_grad_(True)
    xs0, gs0 = gen_inputs(section, seed, quant if quant is not None else F32)
    image = base(section) == "S1"
    xs = [x.to(dtype).requires_grad_(not image) for x in xs0]
    shim = Shim(fault, sd)
    saved_cls = po.CONV2_CLASSES
    try:
        po.CONV2_CLASSES = bool(conv2_classes)
        with shim, (po.rounding(quant) if quant is not None else contextlib.nullcontext()):
            for _ in range(times):          # (batch statistics: the running averages move once per pass)
                outs = oracle_forward(section, sd, xs, bn_train)
            idx = outputs_with_gradient(section, variant)
            wrt = ([] if image else xs) + [sd[n] for n in names]
            got = torch.autograd.grad([outs[i] for i in idx], wrt, [gs0[i].to(dtype) for i in idx], allow_unused=True)
    finally:
        po.CONV2_CLASSES = saved_cls
    nl = 0 if image else len(xs)          # (a leaf's gradient buffer belongs to its pass; only the parameter arena accumulates)
    got = [g if (g is None or i < nl) else g * float(times) for i, g in enumerate(got)]
    return {"outs": [o.detach() for o in outs], "leaf_grads": [None] if image else list(got[:nl]),
            "param_grads": dict(zip(names, got[nl:])), "running": {n: v for n, v in sd.items() if is_stat(n)},
            "relu": shim.relu, "pool": shim.pool}


def view_for(run, section, cfg):
    """What configuration ``cfg`` leaves of a full run: gradients of frozen parameters and of leaves without needs_grad are absent
    (a gradient does not depend on which OTHER tensors ask for one)."""
    tr = trainable_set(section, cfg)
    out = dict(run)
    out["param_grads"] = {n: (g if n in tr else None) for n, g in run["param_grads"].items()}
    if not leaf_grad(cfg):
        out["leaf_grads"] = [None] * len(run["leaf_grads"])
    return out


# ------------------------------------------------------------------------------------------------ margin condition
def _pool_windows(x, k=3, s=2, p=1):
    xp = F.pad(x, (p, p, p, p), value=float("-inf"))
    return xp.unfold(2, k, s).unfold(3, k, s).reshape(x.shape[0], x.shape[1], -1, k * k)


def margins(run64, run32):
    """-> (ok, worst): worst = the smallest margin / (16 x deviation) over every ReLU tensor and max-pool tensor (>= 1 passes)."""
    worst = float("inf")
    assert len(run64["relu"]) == len(run32["relu"]) and len(run64["pool"]) == len(run32["pool"])
    for v64, v32 in zip(run64["relu"], run32["relu"]):
        dev = float((v32.double() - v64).abs().max())
        worst = min(worst, float(v64.abs().min()) / max(FACTOR * dev, 1e-300))
    for (x64, _, _), (x32, _, _) in zip(run64["pool"], run32["pool"]):
        dev = float((x32.double() - x64).abs().max())
        top = _pool_windows(x64).topk(2, dim=-1).values
        gap = top[..., 0] - top[..., 1]
        gap = torch.where(top[..., 0] == 0, torch.full_like(gap, float("inf")), gap)      # the ReLU's exact zero: see the module docstring
        worst = min(worst, float(gap.min()) / max(FACTOR * dev, 1e-300))
    return worst >= 1.0, worst


def find_seed(section, stats, limit=400):
    """The committed search: the first seed from 0 whose float64 run satisfies the margin condition."""
    for seed in range(limit):
        r64 = run_oracle(section, seed, F64, stats == "batch")
        r32 = run_oracle(section, seed, F32, stats == "batch")
        if margins(r64, r32)[0]:
            return seed
    raise AssertionError("no seed below %d satisfies the margin condition for %s / %s" % (limit, section, stats))


# ------------------------------------------------------------------------------------------------ checks
def measure(got, ref64):
    """max|T - T64| / max|T64| over every element (0 / inf when the reference is identically zero)."""
    got, ref64 = got.detach().double().cpu(), ref64.detach().double().cpu()
    assert got.shape == ref64.shape, (tuple(got.shape), tuple(ref64.shape))
    err = (got - ref64).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
    m = float(ref64.abs().max())
    e = float(err.max())
    at = int(torch.argmax(err.reshape(-1)))
    if m == 0.0:
        return (0.0 if e == 0.0 else float("inf")), at
    return e / m, at


def _tensors(run, batch):
    """(kind, name, tensor or None) of everything a case compares."""
    out = [("out", "out%d" % i, t) for i, t in enumerate(run["outs"])]
    out += [("dx", "leaf%d" % i, t) for i, t in enumerate(run["leaf_grads"])]
    out += [("dw", n, t) for n, t in run["param_grads"].items()]
    if batch:
        out += [("stat", n, t) for n, t in run["running"].items()]
    return out


def compare_fp32(case, got, ref64, yard32, log=True):
    """Every output, leaf gradient, trainable parameter gradient (and in A the updated running statistics) of ``got`` against the
    float64 run under 16 x the float32 yardstick; a gradient is absent in ``got`` exactly where it is absent in the reference view.
    -> worst ratio e_got / max(e_yardstick, FLOOR / 16) (<= 16 passes).  One report line (``log``)."""
    _, section, cfg, _ = case
    batch = batch_stats(cfg)
    worst, where, fails = 0.0, "", []
    for (kind, name, t), (_, _, r), (_, _, y) in zip(_tensors(got, batch), _tensors(ref64, batch), _tensors(yard32, batch)):
        if r is None or t is None:
            if (r is None) != (t is None):
                fails.append("%s: gradient %s but the reference's is %s" % (name, "absent" if t is None else "present", "absent" if r is None else "present"))
            continue
        e, at = measure(t, r)
        unit = max(measure(y, r)[0], FLOOR / FACTOR)
        ratio = e / unit
        if ratio > worst:
            worst, where = ratio, "%s[%d]" % (name, at)
        if not ratio <= FACTOR:
            fails.append("%s: e = %.3e at flat index %d, yardstick %.3e, ratio %.1f > %g" % (name, e, at, unit, ratio, FACTOR))
    if log:
        report("engine %-18s worst device / yardstick = %7.3f (limit %g) at %s  %s" % (case_id(case), worst, FACTOR, where, "FAIL" if fails else "OK"))
    assert not fails, "%s:\n  %s" % (case_id(case), "\n  ".join(fails))
    return worst


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-12))


def compare_bf16(case, got, ref):
    """rel-L2 of outputs / leaf gradients / parameter gradients against the rounding oracle under BF16_GATES.  One report line."""
    _, section, cfg, _ = case
    lim = {"out": BF16_GATES["out"], "dx": BF16_GATES["dx_towers" if base(section).startswith("S7") else "dx"], "dw": BF16_GATES["dw"]}
    worst, fails = {"out": (0.0, ""), "dx": (0.0, ""), "dw": (0.0, "")}, []
    for (kind, name, t), (_, _, r) in zip(_tensors(got, False), _tensors(ref, False)):
        if r is None or t is None:
            if (r is None) != (t is None):
                fails.append("%s: gradient %s but the reference's is %s" % (name, "absent" if t is None else "present", "absent" if r is None else "present"))
            continue
        e = rel_l2(t, r)
        if e > worst[kind][0]:
            worst[kind] = (e, name)
        if not e <= lim[kind]:
            fails.append("%s: rel-L2 %.3e > %.1e" % (name, e, lim[kind]))
    report("engine %-18s out %.2e (lim %.0e)  dx %.2e (lim %.0e)  dparam %.2e (lim %.0e, %s)  %s" % (
        case_id(case), worst["out"][0], lim["out"], worst["dx"][0], lim["dx"], worst["dw"][0], lim["dw"], worst["dw"][1], "FAIL" if fails else "OK"))
    assert not fails, "%s:\n  %s" % (case_id(case), "\n  ".join(fails))
    return worst


def check_exact(case, obs):
    """The exact properties.  ``obs``: frozen_nonzero (names of frozen parameters whose arena slice is not all zero bits), stats_changed
    (names of running statistics whose bits changed), ready (name -> param_ready calls), uses_left (names whose ctx.uses count is not 0),
    leftovers (what ctx.grads / ctx.lazy_res / ctx.bnb still held when the tape ended, beyond the leaf gradients), leaf_buffers
    (per leaf: a gradient buffer exists), began / finished (calls of the schedule)."""
    _, section, cfg, _ = case
    tr = trainable_set(section, cfg)
    assert not obs["frozen_nonzero"], "frozen parameters were written to: %s" % sorted(obs["frozen_nonzero"])
    if not batch_stats(cfg):
        assert not obs["stats_changed"], "frozen running statistics changed: %s" % sorted(obs["stats_changed"])
    ready = obs["ready"]
    wrong = {n: c for n, c in ready.items() if c != (1 if n in tr else 0)}
    missing = [n for n in tr if n not in ready]
    assert not wrong and not missing, "param_ready: wrong counts %s, never reported %s" % (wrong, missing)
    assert not obs["uses_left"], "ctx.uses did not end at 0 for %s" % sorted(obs["uses_left"])
    assert not obs["leftovers"], "left behind after the pass: %s" % obs["leftovers"]
    if not leaf_grad(cfg):
        assert not any(obs["leaf_buffers"]), "a leaf without needs_grad got a gradient buffer"
    assert obs["began"] == 1 and obs["finished"] == 1, (obs["began"], obs["finished"])


def expected_routes(section, cfg):
    """For the activation z between the two blocks of S1 - S4 (bn3 + shortcut + ReLU of the first), with the engine's default switches:
    (the identity shortcut's share of its gradient was deferred into conv1's input-gradient launch, the BatchNorm-backward statistics
    of the bn3 behind z rode in that launch) — what the two-block chains exist to reach.  The share is deferred whenever z needs a
    gradient at all; the statistics ride when that bn3 has any to form (batch statistics, or a trainable affine pair)."""
    if base(section) not in ("S1", "S2", "S3", "S4"):
        return None
    tr = trainable_set(section, cfg)
    section = base(section)
    first = {n for n in param_names(section) if n.startswith(_UNITS[section][0])} if section != "S1" else \
        {n for n in param_names(section) if not n.startswith("fpn.layer1.1.")}
    z_needs = (leaf_grad(cfg) and section != "S1") or bool(tr & first)
    bn3 = "fpn.layer%s.0.bn3." % ("1" if section == "S1" else section[1])
    stats = batch_stats(cfg) or (bn3 + "weight") in tr or (bn3 + "bias") in tr
    return z_needs, z_needs and stats


def obs_of_reference(case, view):
    """What a faultless engine would show for ``case``, built from a reference view (the CPU tier drives check_exact with it)."""
    _, section, cfg, _ = case
    tr = trainable_set(section, cfg)
    return {"frozen_nonzero": {n for n, g in view["param_grads"].items() if n not in tr and g is not None},
            "stats_changed": set(), "ready": {n: (1 if n in tr else 0) for n in param_names(section)}, "uses_left": set(), "leftovers": [],
            "leaf_buffers": [g is not None for g in view["leaf_grads"]], "began": 1, "finished": 1}


def np_bits_nonzero(t):
    return bool(np.any(t.detach().cpu().contiguous().view(torch.int32).numpy() != 0))
