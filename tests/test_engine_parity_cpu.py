"""Engine tier, CPU half (tests/engine_ref.py): conditions on the reference alone, and teeth.  No GPU and no product code runs here:
the oracle in float64 is the reference, the same oracle in float32 stands for "a correct implementation in another arithmetic", and
each modelled fault is a small autograd substitution in that float32 run.  The checks the GPU half applies to the device must accept
the faultless float32 run of every fp32 case and reject every fault."""
import pytest
import torch

import engine_ref as er
from engine_ref import F32, F64

_runs = {}


def runs(section, stats, variant=None):
    """(float64 run, float32 run) of a section at its stored seed, computed once."""
    key = (section, stats, variant)
    if key not in _runs:
        seed = er.SEEDS[(section, stats)]
        _runs[key] = tuple(er.run_oracle(section, seed, dt, stats == "batch", variant) for dt in (F64, F32))
    return _runs[key]


def faulty(section, stats, fault, variant=None):
    return er.run_oracle(section, er.SEEDS[(section, stats)], F32, stats == "batch", variant, fault=fault)


def rejected(case, got, r64, r32):
    _, section, cfg, _ = case
    with pytest.raises(AssertionError):
        er.compare_fp32(case, er.view_for(got, section, cfg), er.view_for(r64, section, cfg), er.view_for(r32, section, cfg), log=False)


# ------------------------------------------------------------------------------------------------ the table, the seeds, the margins
def test_case_table_lists_every_section_configuration_and_dtype():
    ids = [er.case_id(c) for c in er.CASES]
    assert len(ids) == len(set(ids))
    for dtype in ("fp32", "bf16"):
        for s in er.SECTIONS:
            want = "BDEFG" if not er.has_bn(s) else ("ABCDEF" + ("G" if s in er.G_VARIANTS else ""))
            if dtype == "bf16":
                want = want.replace("A", "")
            have = sorted({c[2] for c in er.CASES if c[0] == dtype and c[1] == s})
            assert have == sorted(want), (dtype, s, have)
    for s, vs in er.G_VARIANTS.items():
        assert {c[3] for c in er.CASES if c[1] == s and c[2] == "G"} == set(vs)
    assert all(er.case_seed(c) is not None for c in er.CASES)
    assert len([c for c in er.CASES if c[0] == "fp32"]) == 69 and len([c for c in er.CASES if c[0] == "bf16"]) == 62


@pytest.mark.parametrize("key", sorted(er.SEEDS), ids=lambda k: "%s-%s" % k)
def test_stored_seed_satisfies_the_margin_condition_and_is_the_first(key):
    """Zero exceptions: every ReLU input at least 16 x its tensor's float32 deviation from zero, every max-pool window's top two at
    least that far apart; and the table holds what the committed search returns."""
    section, stats = key
    r64, r32 = runs(section, stats)
    ok, worst = er.margins(r64, r32)
    assert ok, "%s / %s seed %d: margin / (16 x deviation) = %.3f" % (section, stats, er.SEEDS[key], worst)
    n_relu = {"S1": 7, "S2": 6, "S3": 6, "S4": 6, "S5": 4, "S6": 1, "S7K1": 40, "S7K3": 40}[er.base(section)]
    assert len(r64["relu"]) == n_relu and len(r64["pool"]) == (1 if er.base(section) == "S1" else 0)
    if er.SEEDS[key] <= 12:
        assert er.find_seed(section, stats, limit=er.SEEDS[key] + 1) == er.SEEDS[key]


def test_margin_condition_rejects_a_near_zero_relu_input_and_a_tied_pool_window():
    r64, r32 = runs("S1", "frozen")
    bad = dict(r64)
    v = r64["relu"][2].clone()
    v.view(-1)[5] = 1e-9
    bad["relu"] = r64["relu"][:2] + [v] + r64["relu"][3:]
    assert not er.margins(bad, r32)[0]
    x = r64["pool"][0][0].clone()
    x[0, 0, 0, 0] = x[0, 0, 0, 1] = float(x.max()) + 1.0          # a tie above zero inside the first window
    bad = dict(r64)
    bad["pool"] = [(x,) + tuple(r64["pool"][0][1:])]
    assert not er.margins(bad, r32)[0]


# ------------------------------------------------------------------------------------------------ configurations
class _Stub(torch.nn.Module):
    """Parameters and BatchNorm layers under the state-dict names of a section (no arithmetic)."""

    def __init__(self, section):
        super(_Stub, self).__init__()
        for n, shape in er.section_shapes(section):
            if er.is_stat(n):
                continue
            mod = self
            *path, leaf = n.split(".")
            for part in path:
                if part not in mod._modules:
                    is_bn = part.startswith("bn") or (part == "1" and "downsample" in n)
                    mod.add_module(part, torch.nn.BatchNorm2d(shape[0]) if is_bn else torch.nn.Module())
                mod = mod._modules[part]
            if leaf not in mod._parameters:
                mod.register_parameter(leaf, torch.nn.Parameter(torch.zeros(shape)))

    def freeze_bn(self):
        for layer in self.modules():
            if isinstance(layer, torch.nn.BatchNorm2d):
                layer.eval()


@pytest.mark.parametrize("section", er.SECTIONS)
def test_every_configuration_produces_the_pattern_it_names(section):
    stub = _Stub(section)
    names = [n for n, _ in stub.named_parameters()]
    assert sorted(names) == sorted(er.param_names(section))
    bns = [m for m in stub.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    assert bool(bns) == er.has_bn(section)
    first, last = er._UNITS[section]
    for cfg in "ABCDEFG":
        er.apply_config(stub, section, cfg)
        on = {n for n, p in stub.named_parameters() if p.requires_grad}
        assert on == er.trainable_set(section, cfg)
        assert all(m.training == (cfg == "A") for m in bns) and stub.training
        if cfg in "ABG":
            assert on == set(names)
        elif cfg == "C":
            assert on and all(not er.is_bn_affine(n) for n in on) and all(n in on for n in names if not er.is_bn_affine(n))
            assert not er.has_bn(section) or len(on) < len(names)
        elif cfg in "DE":
            unit = last if cfg == "D" else first
            assert on and on == {n for n in names if n.startswith(unit)} and len(on) < len(names)
        else:
            assert not on
        assert er.leaf_grad(cfg) == (cfg != "D")


def test_expected_routes_of_the_two_block_chains():
    T, N = True, False
    assert [er.expected_routes("S2", c) for c in "ABCDEFG"] == [(T, T), (T, T), (T, N), (N, N), (T, T), (T, N), (T, T)]
    assert [er.expected_routes("S1", c) for c in "ABCDEF"] == [(T, T), (T, T), (T, N), (N, N), (T, N), (N, N)]
    assert er.expected_routes("S5", "B") is None and er.expected_routes("S7K1", "B") is None


# ------------------------------------------------------------------------------------------------ the checks accept the float32 run
@pytest.mark.parametrize("case", [c for c in er.CASES if c[0] == "fp32"], ids=er.case_id)
def test_checks_accept_the_float32_cpu_run(case):
    _, section, cfg, variant = case
    r64, r32 = runs(section, er.CONFIGS[cfg][1], variant)
    v64, v32 = er.view_for(r64, section, cfg), er.view_for(r32, section, cfg)
    worst = er.compare_fp32(case, v32, v64, v32, log=False)
    assert worst <= 1.0 + 1e-12
    er.check_exact(case, er.obs_of_reference(case, v32))
    tr = er.trainable_set(section, cfg)
    for n in tr:          # the reference reaches every trainable parameter unless the G case cuts its branch off
        assert variant is not None or v64["param_grads"][n] is not None, n
    if variant is not None:
        assert any(g is None for g in v64["param_grads"].values()), "the G case leaves no parameter without a gradient"


def test_yardstick_is_where_the_issue_measured_it():
    """The float32 deviations of the two-block chains were measured at 2e-7 .. 1.7e-6; the allowance rests on that scale."""
    for s in ("S2", "S3", "S4"):
        for stats in ("batch", "frozen"):
            r64, r32 = runs(s, stats)
            e = max(er.measure(y, r)[0] for (_, _, y), (_, _, r) in zip(er._tensors(r32, stats == "batch"), er._tensors(r64, stats == "batch")))
            assert 2.0 ** -26 < e < 2e-5, (s, stats, e)


# ------------------------------------------------------------------------------------------------ modelled faults
class _Sub(torch.autograd.Function):
    """y = fwd(x) with a chosen backward: ``bwd(g, x)``."""

    @staticmethod
    def forward(ctx, x, y, bwd):
        ctx.bwd, ctx.x = bwd, x.detach()
        return y.detach().clone()

    @staticmethod
    def backward(ctx, g):
        return ctx.bwd(g, ctx.x), None, None


class FlipOneRelu(er.Fault):
    """1. One ReLU decision flipped, at the element of the whole run closest to zero."""

    def __init__(self, r64):
        mins = [float(v.abs().min()) for v in r64["relu"]]
        self.call = mins.index(min(mins))

    def relu(self, i, v, orig):
        if i != self.call:
            return None
        mask = (v.detach() > 0)
        j = int(torch.argmin(v.detach().abs().reshape(-1)))
        mask.view(-1)[j] = ~mask.view(-1)[j]
        return v * mask.to(v.dtype)


class Shortcut(er.Fault):
    """2. / 3. relu(bn3(.) + x) of the identity block: the sum's gradient g * (z > 0) reaches the BatchNorm branch as it should, the
    shortcut gets ``to_shortcut(g, mask)`` instead — g without the mask, or nothing."""

    def __init__(self, bn_call, relu_call, to_shortcut):
        self.bn_call, self.relu_call, self.to_shortcut = bn_call, relu_call, to_shortcut
        self.h = {}

    def batch_norm(self, i, args, kwargs, orig):
        if i != self.bn_call:
            return None
        out = orig(*args, **kwargs)
        return _Sub.apply(out, out, lambda g, x: self.h["right"] - self.h["wrong"] + g)      # g arrives as "wrong": replace it by "right"

    def relu(self, i, v, orig):
        if i != self.relu_call:
            return None

        def bwd(g, x):
            mask = (x > 0).to(g.dtype)
            self.h["right"], self.h["wrong"] = g * mask, self.to_shortcut(g, mask)
            return self.h["wrong"]          # reaches both addends; the BatchNorm branch corrects its own above
        return _Sub.apply(v, orig(v), bwd)


def _bn_parts(args, kwargs):
    x, rm, rv, w, b = args[:5]
    return x, rm, rv, w, b, kwargs.get("eps", 1e-5)


class BatchCoefficientsOnFrozen(er.Fault):
    """4. A frozen layer's BatchNorm backward computed as if the layer had normalised with batch statistics."""

    def __init__(self, call):
        self.call = call

    def batch_norm(self, i, args, kwargs, orig):
        if i != self.call:
            return None
        assert not kwargs["training"]
        x, rm, rv, w, b, eps = _bn_parts(args, kwargs)
        y = orig(*args, **kwargs)

        def bwd(g, xd):
            with torch.enable_grad():
                x_ = xd.clone().requires_grad_(True)
                yb = orig(x_, None, None, w.detach(), b.detach(), training=True, momentum=0.0, eps=eps)
                return torch.autograd.grad(yb, x_, g)[0]
        # dgamma / dbeta through the true graph (y), dx from the batch-statistics formula
        return _BnDx.apply(x, w, b, y, bwd)


class _BnDx(torch.autograd.Function):
    """Value and parameter gradients of a frozen BatchNorm, input gradient from ``dx(g, x)``."""

    @staticmethod
    def forward(ctx, x, w, b, y, dx):
        ctx.dx = dx
        ctx.save_for_backward(x.detach(), y.detach(), w.detach(), b.detach())
        return y.detach().clone()

    @staticmethod
    def backward(ctx, g):
        x, y, w, b = ctx.saved_tensors
        xhat = (y - b.view(1, -1, 1, 1)) / w.view(1, -1, 1, 1)
        return ctx.dx(g, x), (g * xhat).sum((0, 2, 3)), g.sum((0, 2, 3)), None, None


class GammaFromOtherMode(er.Fault):
    """5. dgamma = sum g * xhat with the xhat of the mode the layer is NOT in (batch-normalised on a frozen layer)."""

    def __init__(self, call):
        self.call = call

    def batch_norm(self, i, args, kwargs, orig):
        if i != self.call:
            return None
        assert not kwargs["training"]
        x, rm, rv, w, b, eps = _bn_parts(args, kwargs)
        y = orig(*args, **kwargs)

        class Fn(torch.autograd.Function):
            @staticmethod
            def forward(ctx, x_, w_, b_):
                ctx.save_for_backward(x_.detach(), w_.detach())
                return y.detach().clone()

            @staticmethod
            def backward(ctx, g):
                xd, wd = ctx.saved_tensors
                inv = 1.0 / torch.sqrt(rv + eps)
                mu, var = xd.mean((0, 2, 3)), xd.var((0, 2, 3), unbiased=False)
                other = (xd - mu.view(1, -1, 1, 1)) / torch.sqrt(var + eps).view(1, -1, 1, 1)
                return g * (wd * inv).view(1, -1, 1, 1), (g * other).sum((0, 2, 3)), g.sum((0, 2, 3))
        return Fn.apply(x, w, b)


class UpsampleAddThreeOfFour(er.Fault):
    """6. The up-sample-add backward sums three of the four fine pixels of each coarse one."""

    def interpolate(self, i, args, kwargs, orig):
        if i != 0:
            return None
        x = args[0]
        y = orig(*args, **kwargs)
        assert y.shape[2] == 2 * x.shape[2] and y.shape[3] == 2 * x.shape[3]
        return _Sub.apply(x, y, lambda g, xd: g[:, :, 0::2, 0::2] + g[:, :, 0::2, 1::2] + g[:, :, 1::2, 0::2])


class InputGradOf(er.Fault):
    """7. / 8. The input gradient of the convolution with weight ``name`` replaced by ``edit(g)`` (its weight gradient is right)."""

    def __init__(self, name, edit):
        self.name, self.edit, self.hits = name, edit, 0

    def conv2d(self, i, args, kwargs, orig, sd):
        if args[1] is not sd[self.name]:
            return None
        self.hits += 1
        x = _Sub.apply(args[0], args[0], lambda g, xd: self.edit(g))
        return orig(x, *args[1:], **kwargs)


def _zero_odd_odd(g):
    g = g.clone()
    g[:, :, 1::2, 1::2] = 0
    return g


class NoSigmoidDerivative(er.Fault):
    """9. The sigmoid derivative omitted at the detection edge."""

    def sigmoid(self, i, v, orig):
        return _Sub.apply(v, orig(v), lambda g, x: g)


B_S2 = ("fp32", "S2", "B", None)


def test_teeth_1_one_flipped_relu_decision():
    r64, r32 = runs("S2", "frozen")
    for case, (a, b) in ((B_S2, (r64, r32)), (("fp32", "S2", "A", None), runs("S2", "batch"))):
        rejected(case, faulty("S2", er.CONFIGS[case[2]][1], FlipOneRelu(a)), a, b)


def test_teeth_2_identity_shortcut_gradient_without_the_relu_mask():
    r64, r32 = runs("S2", "frozen")
    # S2: BatchNorm calls 0-3 are block 0 (bn1, bn2, bn3, downsample), 4-6 block 1; ReLU calls 0-2 / 3-5
    rejected(B_S2, faulty("S2", "frozen", Shortcut(6, 5, lambda g, mask: g)), r64, r32)


def test_teeth_3_identity_shortcut_gradient_dropped():
    r64, r32 = runs("S2", "frozen")
    rejected(B_S2, faulty("S2", "frozen", Shortcut(6, 5, lambda g, mask: torch.zeros_like(g))), r64, r32)
    # the substitution itself is sound: handing the shortcut what it should get reproduces the faultless run
    same = faulty("S2", "frozen", Shortcut(6, 5, lambda g, mask: g * mask))
    er.compare_fp32(B_S2, same, r64, r32, log=False)


def test_teeth_4_batch_statistics_coefficients_on_a_frozen_layer():
    r64, r32 = runs("S2", "frozen")
    rejected(B_S2, faulty("S2", "frozen", BatchCoefficientsOnFrozen(1)), r64, r32)
    rejected(("fp32", "S2", "F", None), faulty("S2", "frozen", BatchCoefficientsOnFrozen(5)), r64, r32)


def test_teeth_5_dgamma_with_the_other_modes_xhat():
    r64, r32 = runs("S2", "frozen")
    rejected(B_S2, faulty("S2", "frozen", GammaFromOtherMode(1)), r64, r32)
    # ... and only dgamma moves: with the BatchNorm affine frozen (C) the same run is accepted
    c = ("fp32", "S2", "C", None)
    got = faulty("S2", "frozen", GammaFromOtherMode(1))
    er.compare_fp32(c, er.view_for(got, "S2", "C"), er.view_for(r64, "S2", "C"), er.view_for(r32, "S2", "C"), log=False)


def test_teeth_6_upsample_add_backward_over_three_of_four_pixels():
    r64, r32 = runs("S5", "frozen")
    rejected(("fp32", "S5", "B", None), faulty("S5", "frozen", UpsampleAddThreeOfFour()), r64, r32)


def test_teeth_7_c5_gradient_missing_one_consumer():
    r64, r32 = runs("S5", "frozen")
    for name in ("fpn.latlayer1.weight", "fpn.conv6.weight", "fpn.toplayer.weight"):
        f = InputGradOf(name, torch.zeros_like)
        got = faulty("S5", "frozen", f)
        assert f.hits == 1
        rejected(("fp32", "S5", "B", None), got, r64, r32)
        rejected(("fp32", "S5", "F", None), got, r64, r32)


def test_teeth_8_one_parity_class_of_a_stride_2_input_gradient_zeroed():
    r64, r32 = runs("S2", "frozen")
    f = InputGradOf("fpn.layer2.0.conv2.weight", _zero_odd_odd)
    got = faulty("S2", "frozen", f)
    assert f.hits == 1
    rejected(B_S2, got, r64, r32)
    f = InputGradOf("fpn.layer2.0.downsample.0.weight", _zero_odd_odd)          # 1x1 / stride 2: the class (1, 1) holds zeros anyway
    er.compare_fp32(B_S2, faulty("S2", "frozen", f), r64, r32, log=False)


@pytest.mark.parametrize("section", ["S7K1", "S7K3"])
def test_teeth_9_sigmoid_derivative_omitted(section):
    r64, r32 = runs(section, "frozen")
    rejected(("fp32", section, "B", None), faulty(section, "frozen", NoSigmoidDerivative()), r64, r32)
    r64, r32 = runs(section, "frozen", "reg")          # ... which only the class tower can show
    er.compare_fp32(("fp32", section, "G", "reg"), faulty(section, "frozen", NoSigmoidDerivative(), "reg"), r64, r32, log=False)


def test_teeth_10_a_frozen_parameter_receives_its_gradient():
    case = ("fp32", "S2", "D", None)
    r64, r32 = runs("S2", "frozen")
    v64, v32 = er.view_for(r64, "S2", "D"), er.view_for(r32, "S2", "D")
    leaked = dict(v32)
    leaked["param_grads"] = dict(v32["param_grads"])
    leaked["param_grads"]["fpn.layer2.0.bn2.weight"] = r32["param_grads"]["fpn.layer2.0.bn2.weight"]
    with pytest.raises(AssertionError):
        er.compare_fp32(case, leaked, v64, v32, log=False)
    with pytest.raises(AssertionError):
        er.check_exact(case, er.obs_of_reference(case, leaked))
    obs = er.obs_of_reference(case, v32)
    er.check_exact(case, obs)
    for key, bad in (("ready", dict(obs["ready"], **{"fpn.layer2.0.bn2.weight": 1})), ("ready", dict(obs["ready"], **{"fpn.layer2.1.conv3.weight": 2})),
                     ("ready", {n: c for n, c in obs["ready"].items() if n != "fpn.layer2.1.bn3.bias"}), ("uses_left", {"fpn.layer2.1.conv1.weight"}),
                     ("leftovers", ["lazy_res: 1"]), ("leaf_buffers", [True]), ("stats_changed", {"fpn.layer2.0.bn1.running_var"}), ("finished", 0)):
        with pytest.raises(AssertionError):
            er.check_exact(case, dict(obs, **{key: bad}))


def test_teeth_11_an_unused_heads_gradient_zero_filled():
    """A G case equals the reference with the unused outputs' gradients ABSENT: what only they reach has no gradient at all.  Zero-filling
    them (and running the backward of the unused branch, statistics sums included, on zeros) gives zero TENSORS there instead."""
    for section, variant in (("S5", "kp"), ("S5", "det"), ("S6", "pred"), ("S7K1", "reg"), ("S7K3", "cls")):
        case = ("fp32", section, "G", variant)
        r64, r32 = runs(section, "frozen", variant)
        absent = [n for n, g in r64["param_grads"].items() if g is None]
        assert absent
        full = runs(section, "frozen")[1]
        filled = dict(r32)
        filled["param_grads"] = {n: (torch.zeros_like(full["param_grads"][n]) if g is None else g) for n, g in r32["param_grads"].items()}
        filled["leaf_grads"] = [torch.zeros_like(f) if g is None else g for g, f in zip(r32["leaf_grads"], full["leaf_grads"])]
        with pytest.raises(AssertionError):
            er.compare_fp32(case, filled, r64, r32, log=False)
        er.compare_fp32(case, r32, r64, r32, log=False)
    r64 = runs("S5", "frozen", "det")[0]
    assert r64["leaf_grads"][3] is None and r64["leaf_grads"][0] is not None          # c2 feeds the keypoint pyramid only


# ------------------------------------------------------------------------------------------------ the odd-size sections
def test_odd_sections_have_the_shapes_of_an_image_that_is_no_multiple_of_32():
    """S1o: image 19x13 -> stem 10x7 -> pool 5x4.  S5o: the stage sizes of a 75x40 image, every pyramid level at its lateral's size,
    p6 / p7 ceil-sized.  S7K1o: those five levels, 74 cells, 666 anchors per image, 100 / 30 / 12 / 4 / 2 pixels per level for B = 2.
    The even sections keep the shapes they had."""
    assert er.out_shapes("S1o") == [(256, 5, 4)] and er.out_shapes("S1") == [(256, 4, 3)]
    assert er.out_shapes("S5o") == [(256, 19, 10), (256, 10, 5), (256, 5, 3), (256, 3, 2), (256, 10, 5), (256, 5, 3), (256, 3, 2), (256, 2, 1), (256, 1, 1)]
    assert er.out_shapes("S5") == [(256, 16, 8), (256, 8, 4), (256, 4, 2), (256, 2, 1), (256, 8, 4), (256, 4, 2), (256, 2, 1), (256, 1, 1), (256, 1, 1)]
    assert er.out_shapes("S6") == [(19, 16, 8)] * 4 + [(18, 16, 8)]
    assert er.out_shapes("S7K1o") == [("A", 666, 1), ("A", 666, 4)] and er.out_shapes("S7K1") == [("A", 396, 1), ("A", 396, 4)]
    assert [er.B * h * w for _, h, w in er._LEAVES["S7K1o"]] == [100, 30, 12, 4, 2]
    assert [tuple(s[1:]) for s in er._LEAVES["S7K1o"]] == [tuple(s[1:]) for s in er.out_shapes("S5o")[4:]]      # what S5o's detection pyramid gives
    h, w = 75, 40
    sizes = []
    for _ in range(5):
        h, w = (h + 1) // 2, (w + 1) // 2
        sizes.append((h, w))
    assert [tuple(s[1:]) for s in er._LEAVES["S5o"]] == sizes[:0:-1]
    for o, b in (("S1o", "S1"), ("S5o", "S5"), ("S7K1o", "S7K1")):
        assert er.base(o) == b and er.section_shapes(o) == er.section_shapes(b) and er.G_VARIANTS.get(o) == er.G_VARIANTS.get(b)
        assert [er.trainable_set(o, c) for c in "ABCDEFG"] == [er.trainable_set(b, c) for c in "ABCDEFG"]
        assert [er.expected_routes(o, c) for c in "ABCDEFG"] == [er.expected_routes(b, c) for c in "ABCDEFG"]
        assert er.gen_inputs(o, 0)[0][0].shape[2:] != er.gen_inputs(b, 0)[0][0].shape[2:]
    r64 = runs("S5o", "frozen")[0]
    assert [tuple(o.shape[1:]) for o in r64["outs"]] == er.out_shapes("S5o")          # the oracle sizes by the lateral, conv6 / conv7 by ceil
    assert [tuple(o.shape[1:]) for o in runs("S1o", "frozen")[0]["outs"]] == er.out_shapes("S1o")
    assert tuple(r64["pool"]) == () and tuple(runs("S1o", "frozen")[0]["pool"][0][0].shape[2:]) == (10, 7)


def _halving(n_out, n_in):
    """The 2x-only rule: source index i // 2, clamped to the last row / column."""
    return (torch.arange(n_out) // 2).clamp(max=n_in - 1)


def _pixel_centres(n_out, n_in):
    """The other nearest convention: the source pixel under the CENTRE of the destination pixel, floor((i + 1/2) * n_in / n_out)."""
    return (((2 * torch.arange(n_out) + 1) * n_in) // (2 * n_out)).clamp(max=n_in - 1)


class NearestBy(er.Fault):
    """12. / 13. Every nearest up-sample-to-size of the run replaced by a gather under another index rule (forward, and through the
    gather's own backward the enumeration of each coarse pixel's children)."""

    def __init__(self, rule):
        self.rule, self.hits = rule, 0

    def interpolate(self, i, args, kwargs, orig):
        x, (H, W) = args[0], kwargs["size"]
        assert kwargs["mode"] == "nearest"
        self.hits += 1
        return x[:, :, self.rule(H, x.shape[2])][:, :, :, self.rule(W, x.shape[3])]


def _failed_names(case, got, r64, r32):
    """The tensors compare_fp32 rejects (names as in its report: out<i>, leaf<i>, parameter names)."""
    with pytest.raises(AssertionError) as e:
        er.compare_fp32(case, got, r64, r32, log=False)
    return {line.strip().split(":")[0] for line in str(e.value).splitlines()[1:]}


def _nearest(n_out, n_in):
    x = torch.arange(n_in, dtype=F64).view(1, 1, n_in, 1)
    return torch.nn.functional.interpolate(x, size=(n_out, 1), mode="nearest").view(-1).long()


def test_teeth_12_upsample_by_the_halving_rule():
    """Source index i // 2 (clamped) in place of nearest-to-size.  On S5 every level is exactly twice the next and the rule IS the
    nearest rule, so the faulty run is accepted: S5 cannot see it.  It is accepted on S5o as well, and on every size the network can
    produce: a lateral of extent L sits over a coarse level of extent n = ceil(L / 2), so L is 2n or 2n - 1, and for L = 2n - 1
    floor(i * n / (2n - 1)) = floor(i / 2 + i / (2 (2n - 1))) = i // 2 because the second term stays below 1/2 (checked below for
    every n up to 64).  What S5o can see of an index rule that S5 cannot is the next test's."""
    for n in range(1, 65):
        for L in (2 * n - 1, 2 * n):
            assert torch.equal(_nearest(L, n), _halving(L, n)), (L, n)
    for section in ("S5", "S5o"):
        r64, r32 = runs(section, "frozen")
        f = NearestBy(_halving)
        got = faulty(section, "frozen", f)
        assert f.hits == 5
        er.compare_fp32(("fp32", section, "B", None), got, r64, r32, log=False)
        assert all(torch.equal(a, b) for a, b in zip(got["outs"], r32["outs"]))          # not merely accepted: the same forward, bit for bit


def test_teeth_13_upsample_by_pixel_centres():
    """The source pixel under the destination pixel's centre (the "nearest-exact" convention) in place of nearest-to-size's
    floor(i * n_in / n_out).  At an exact factor 2 the two agree — floor((2i + 1) / 4) = i // 2 — so S5 accepts the run: the reason
    S5o exists.  At 3 -> 5 they part (sources 0 0 1 2 2 against 0 0 1 1 2), as at every odd extent above 1, and S5o rejects the run:
    every output below the first non-2x level, the gradient of layer4.2's input, and the parameter gradients of the two 1x1
    convolutions whose outputs are up-sampled first; what lies above that level (fp5, p5s, p6, p7 and their parameters) is untouched."""
    for n in range(1, 65):
        assert torch.equal(_nearest(2 * n, n), _pixel_centres(2 * n, n))
        assert n == 1 or not torch.equal(_nearest(2 * n - 1, n), _pixel_centres(2 * n - 1, n))
    r64, r32 = runs("S5", "frozen")
    got = faulty("S5", "frozen", NearestBy(_pixel_centres))
    er.compare_fp32(("fp32", "S5", "B", None), got, r64, r32, log=False)
    assert all(torch.equal(a, b) for a, b in zip(got["outs"], r32["outs"]))
    r64, r32 = runs("S5o", "frozen")
    f = NearestBy(_pixel_centres)
    got = faulty("S5o", "frozen", f)
    assert f.hits == 5
    names = er.OUT_NAMES["S5o"]
    bad = _failed_names(("fp32", "S5o", "B", None), got, r64, r32)
    for n in ("fp4s", "fp3s", "fp2s", "p4s", "p3s"):
        assert "out%d" % names.index(n) in bad, (n, sorted(bad))
    for n in ("fp5", "p5s", "p6", "p7"):
        assert "out%d" % names.index(n) not in bad, (n, sorted(bad))
    assert "leaf0" in bad          # the input of layer4.2
    for n in ("fpn.toplayer.weight", "fpn.latlayer1.weight"):
        assert n in bad, (n, sorted(bad))
    # (their bias gradients are sums over every pixel, and under either rule every fine pixel has exactly one parent: unchanged)
    assert not bad & {"fpn.toplayer.bias", "fpn.latlayer1.bias"}
    assert not bad & {"fpn.conv6.weight", "fpn.conv7.weight", "fpn.toplayer0.weight"}
    # ... with nothing trainable (F) the outputs and the leaf gradient still show it
    rejected(("fp32", "S5o", "F", None), got, r64, r32)


class FloorSizedP6(er.Fault):
    """14. conv6 sized by floor(H / 2) x floor(W / 2): the stride-2 convolution loses its last output row / column where the extent is
    odd.  ``refill``: the level keeps its ceil-sized buffer and the lost row / column is never written (zeros)."""

    def __init__(self, refill):
        self.refill, self.hits = refill, 0

    def conv2d(self, i, args, kwargs, orig, sd):
        if args[1] is not sd["fpn.conv6.weight"]:
            return None
        self.hits += 1
        x = args[0]
        y = orig(*args, **kwargs)
        h, w = max(x.shape[2] // 2, 1), max(x.shape[3] // 2, 1)
        cut = y[:, :, :h, :w]
        if self.refill:
            cut = torch.nn.functional.pad(cut, (0, y.shape[3] - w, 0, y.shape[2] - h))
        return cut


def test_teeth_14_p6_sized_by_floor():
    """S5o: c5 is 3x2, p6 must be 2x1 (ceil).  Sized by floor it is 1x1: rejected by the shape check (the unused-detection G case, so
    that the run needs no gradient of that shape); kept at 2x1 with the second row never written: rejected element by element in p6,
    p7 and conv6's gradients.  S5's c5 is 2x1, where floor and ceil agree: the same fault is accepted there."""
    r64, r32 = runs("S5o", "frozen", "kp")
    f = FloorSizedP6(False)
    got = faulty("S5o", "frozen", f, "kp")
    assert f.hits == 1 and tuple(got["outs"][7].shape[2:]) == (1, 1) and tuple(r64["outs"][7].shape[2:]) == (2, 1)
    with pytest.raises(AssertionError) as e:
        er.compare_fp32(("fp32", "S5o", "G", "kp"), got, r64, r32, log=False)
    assert "(2, 256, 1, 1)" in str(e.value) and "(2, 256, 2, 1)" in str(e.value)          # measure's shape check, not an element
    r64, r32 = runs("S5o", "frozen")
    bad = _failed_names(("fp32", "S5o", "B", None), faulty("S5o", "frozen", FloorSizedP6(True)), r64, r32)
    assert {"out7", "out8", "fpn.conv6.weight", "fpn.conv6.bias", "leaf0"} <= bad and "out6" not in bad, sorted(bad)
    r64, r32 = runs("S5", "frozen")
    assert er.compare_fp32(("fp32", "S5", "B", None), faulty("S5", "frozen", FloorSizedP6(True)), r64, r32, log=False) <= 1.0 + 1e-12
