"""Tensor-level wrappers over the C-ABI (``include/mpn.h``).

torch is used only as the device-memory allocator and stream provider: every function here passes
raw device pointers, sizes and the current ``hipStream_t`` to ``libmpn_hip.so``.
"""
import ctypes
import os
from collections import namedtuple

import torch

from . import _lib
from ._lib import BF16, F16, F32, ConvParams, WgradParams, call


def round_up(v, m):
    return (v + m - 1) // m * m


def dtype_code(dt):
    if dt == torch.float32:
        return F32
    if dt == torch.bfloat16:
        return BF16
    if dt == torch.float16:
        return F16
    raise _lib.MpnError("unsupported dtype %s" % dt)


# Launch stream.  Kernels go to torch's current stream unless the engine has pushed an explicit one (the weight-gradient
# side stream): switching torch's current stream with `torch.cuda.stream(...)` costs ~20 us of Python per use, and
# torch.cuda.current_stream() ~8 us per launch; the raw-handle query below is two C calls.
_STREAM_OVERRIDE = []          # stack of (raw handle, torch.cuda.Stream)


def push_stream(stream):
    _STREAM_OVERRIDE.append((stream.cuda_stream, stream))


def pop_stream():
    _STREAM_OVERRIDE.pop()


def stream_handle():
    if _STREAM_OVERRIDE:
        return _STREAM_OVERRIDE[-1][0]
    return torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice())


def check_device(t):
    """Kernels are enqueued on the CURRENT device's stream: refuse tensors that live on another GPU (the reference selects
    the device with params.gpus[0] and never calls set_device; training/batch_processor.py here does)."""
    if not t.is_cuda:
        raise _lib.MpnError("tensor is on %s; the HIP path has no CPU fallback" % t.device)
    cur = torch._C._cuda_getDevice()
    if t.device.index != cur:
        raise _lib.MpnError("tensor is on cuda:%d but the current device is cuda:%d — call torch.cuda.set_device(%d) "
                            "(or run under torch.cuda.device) first" % (t.device.index, cur, t.device.index))


def stream_obj():
    """torch.cuda.Stream to record events on (None = torch's current stream)."""
    return _STREAM_OVERRIDE[-1][1] if _STREAM_OVERRIDE else None


def launch_stream(device):
    """torch.cuda.Stream our launches go to right now: the pushed override, else torch's current stream."""
    return _STREAM_OVERRIDE[-1][1] if _STREAM_OVERRIDE else torch.cuda.current_stream(device)


def stream_ptr():
    return ctypes.c_void_p(stream_handle())


def is16(dt):
    """bf16 / f16: 32 elements per 64-byte K chunk, 8 per 16-byte vector."""
    return dt == torch.bfloat16 or dt == torch.float16


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


class Act(object):
    """Dense pixel-major activation: storage ``t`` is [B, H, W, Cs] contiguous, ``C`` logical channels.

    Cs (channel storage) is a multiple of 32; lanes [C, Cs) hold zeros (see include/mpn.h).
    """
    __slots__ = ("t", "B", "H", "W", "C", "Cs", "needs_grad", "tag", "seg", "cons", "bn_src", "mask", "conv_cons")

    def __init__(self, t, C, needs_grad=False, tag=""):
        self.t = t
        self.B, self.H, self.W, self.Cs = t.shape
        self.C = C
        self.needs_grad = needs_grad
        self.tag = tag
        self.seg = None          # (flat buffer, index) when this activation is one level of a pyramid group (alloc_seg)
        self.cons = 0            # gradient contributions still to come in backward (engine: last-contributor detection)
        self.bn_src = None       # output of a BatchNorm: the BNSource that produced it
        self.conv_cons = 0       # how many of the pending contributions are input gradients of plain convolutions (engine.conv)
        self.mask = None         # sign bits of this tensor (uint8 [P, Cs / V]) when bn_act produced them for the backward pass

    @staticmethod
    def empty(B, H, W, C, dtype, device, needs_grad=False, tag=""):
        return Act(torch.empty((B, H, W, round_up(C, 32)), dtype=dtype, device=device), C, needs_grad, tag)

    @property
    def P(self):
        return self.B * self.H * self.W

    @property
    def dtype(self):
        return self.t.dtype

    def nchw(self):
        """Logical [B, C, H, W] view (channels_last strides) — the shape the reference API exposes."""
        return self.t[..., : self.C].permute(0, 3, 1, 2)


class _KernelEvents(object):
    """Optional live timing of conv launches with HIP events on the launch stream (bench.py roofline).

    Each instrumented launch is bracketed by two events recorded on the SAME stream the kernel is
    enqueued on (torch's current stream); durations are read after the timed region."""

    def __init__(self):
        self.on = False
        self.detail = False          # name launches by shape (tools/shape_report.py)
        self.rec = []

    def enable(self):
        self.on = True
        self.rec = []

    def disable(self):
        self.on = False

    def begin(self):
        e = torch.cuda.Event(enable_timing=True)
        e.record(stream_obj())
        return e

    def end(self, name, flops, e0):
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record(stream_obj())
        self.rec.append((name, flops, e0, e1))

    def summary(self):
        out = {}
        for name, flops, e0, e1 in self.rec:
            d = out.setdefault(name, {"ms": 0.0, "flops": 0.0, "n": 0})
            d["ms"] += e0.elapsed_time(e1)
            d["flops"] += flops
            d["n"] += 1
        return out


KERNEL_EVENTS = _KernelEvents()

_ws = {}
WS_EPOCH = 0          # replay.py sets a unique value while it records: the recorded launches then own their scratch buffers


def take_epoch_workspaces(epoch):
    """Remove and return the scratch buffers allocated under capture epoch `epoch` (the graph keeps them alive; nothing
    outside the graph may re-grow or free them)."""
    keys = [k for k in _ws if k[3] == epoch]
    return [_ws.pop(k) for k in keys]


def workspace(nbytes, device, slot=0):
    """Persistent scratch (grown geometrically); one buffer per (device, slot)."""
    # one buffer per stream as well: launches on different streams must not share (or re-grow) a scratch area
    key = (device, slot, stream_handle() if device.type == "cuda" else 0, WS_EPOCH)
    buf = _ws.get(key)
    if buf is None or buf.numel() < nbytes:
        so = stream_obj()
        if buf is not None and so is not None:
            buf.record_stream(so)        # the outgoing buffer may still be read by launches queued on the pushed stream
        buf = torch.empty(int(nbytes * 1.25) + 1024, dtype=torch.uint8, device=device)
        if so is not None:
            buf.record_stream(so)
        _ws[key] = buf
    return buf


def _kernel_name(query, p):
    """The instantiation the library launches for the parameter block p, as rocprofv3 spells it (`query`: mpn_conv_kernel_name or
    mpn_conv_wgrad_kernel_name — the launcher's own routing decision; nothing here re-derives it)."""
    buf = ctypes.create_string_buffer(128)
    n = call(query, ctypes.byref(p), buf, len(buf))
    if n < 0:
        raise _lib.MpnError("%s failed with status %d" % (query, n))
    return buf.value.decode()


def _launch_conv(p, flops, label):
    """The one mpn_conv_forward call site.  flops() / label() (algorithmic FLOPs; the shape label of tools/shape_report.py) are only
    evaluated while KERNEL_EVENTS brackets the launch."""
    events = KERNEL_EVENTS.on
    if events:
        # KERNEL_EVENTS classes keep the five-argument spelling bench.py's pmc_traffic keys on: the library's name without its last (EXT) argument
        name = label() if KERNEL_EVENTS.detail else _kernel_name("mpn_conv_kernel_name", p).rsplit(", ", 1)[0] + ">"
        e0 = KERNEL_EVENTS.begin()
    call("mpn_conv_forward", ctypes.byref(p), stream_ptr())
    if events:
        KERNEL_EVENTS.end(name, flops(), e0)


def _launch_wgrad(p, dev, db, flops, label, plan="mpn_conv_wgrad_chunks"):
    """The one weight-gradient call site: splits the contraction (`plan`: mpn_conv_wgrad_chunks, or mpn_conv_wgrad_seg_plan for a pyramid),
    attaches the partial-sum workspaces and the bias gradient db the launch fuses (None: not fused), and launches.  flops() / label(chunks)
    as in _launch_conv."""
    p.chunks = 1
    chunks = call(plan, ctypes.byref(p))
    if chunks < 1:
        raise _lib.MpnError("%s failed with status %d" % (plan, chunks))
    p.chunks = chunks
    if chunks > 1:
        p.ws = workspace(chunks * p.Cout * p.R * p.S * p.Cin * 4, dev, slot=1).data_ptr()
    if db is not None:
        p.db = db.data_ptr()
        if chunks > 1:
            p.db_ws = workspace(chunks * p.Cout * 4, dev, slot=4).data_ptr()
    events = KERNEL_EVENTS.on
    if events:
        name = label(chunks) if KERNEL_EVENTS.detail else _kernel_name("mpn_conv_wgrad_kernel_name", p)
        e0 = KERNEL_EVENTS.begin()
    # under events the MFMA kernel is bracketed alone (the partial-sum reduction is launched separately) so the class time matches the
    # kernel's own row in a rocprofv3 trace
    call("mpn_conv_wgrad_partials" if events and chunks > 1 else "mpn_conv_wgrad", ctypes.byref(p), stream_ptr())
    if events:
        KERNEL_EVENTS.end(name, flops(), e0)
        if chunks > 1:          # the reduction mpn_conv_wgrad runs (same kernels and order: the same bits as without events)
            call("mpn_conv_wgrad_reduce", ctypes.byref(p), stream_ptr())


def alloc_seg(like, C, dtype):
    """One buffer holding an activation per pyramid level (geometry of the Acts in `like`, C channels): the levels are views
    of a single flat tensor, so element-wise kernels can treat the whole pyramid as one array."""
    Cs = round_up(C, 32)
    sizes = [a.B * a.H * a.W * Cs for a in like]
    flat = torch.empty(sum(sizes), dtype=dtype, device=like[0].t.device)
    out, off = [], 0
    for i, (a, n) in enumerate(zip(like, sizes)):
        v = Act(flat[off: off + n].view(a.B, a.H, a.W, Cs), C)
        v.seg = (flat, i)
        out.append(v)
        off += n
    return out


def seg_flat(acts):
    """The flat tensor behind a complete pyramid group (None if `acts` is not exactly one group in order)."""
    if not acts or acts[0].seg is None:
        return None
    flat = acts[0].seg[0]
    for i, a in enumerate(acts):
        if a.seg is None or a.seg[0] is not flat or a.seg[1] != i:
            return None
    return flat if sum(a.t.numel() for a in acts) == flat.numel() else None


def conv_forward_seg(xs, w, Cout, R, S, pad, bias=None, act=0, out_f32=False, mode=0, outs=None, accumulate=False, cin=None):
    """The same convolution (stride 1, same-size output) over every level of a pyramid in ONE launch — the shared RetinaNet
    towers of posenet.py:327-328.  xs: Acts with equal B / C / dtype.  Returns the per-level outputs (views of one buffer)."""
    x0 = xs[0]
    dt = x0.t.dtype
    odt = torch.float32 if out_f32 else dt
    if outs is None:
        outs = alloc_seg(xs, Cout, odt)
    p = ConvParams()
    p.w = w.data_ptr()
    p.bias = bias.data_ptr() if bias is not None else None
    p.B = x0.B
    p.Cin = cin if cin is not None else round_up(x0.C, 32 if is16(dt) else 16)
    p.Cout, p.Cout_store = Cout, outs[0].Cs
    p.x_sW, p.y_sP = x0.Cs, outs[0].Cs
    p.R, p.S, p.stride, p.pad = R, S, 1, pad
    p.mode, p.act, p.accumulate = mode, act, 1 if accumulate else 0
    p.dtype = dtype_code(dt)
    p.out_f32 = 1 if (out_f32 and dt != torch.float32) else 0
    p.nseg = len(xs)
    tile0 = 0
    for l, (x, o) in enumerate(zip(xs, outs)):
        assert (x.B, x.Cs, x.t.dtype) == (x0.B, x0.Cs, dt) and (o.H, o.W, o.Cs, o.t.dtype) == (x.H, x.W, outs[0].Cs, odt)
        p.seg_x[l], p.seg_y[l] = x.t.data_ptr(), o.t.data_ptr()
        p.seg_H[l], p.seg_W[l] = x.H, x.W
        p.seg_tile0[l] = tile0
        tile0 += (x.B * x.H * x.W + 127) // 128
    p.seg_tile0[len(xs)] = tile0
    _launch_conv(p, lambda: sum(2.0 * x.B * x.H * x.W * Cout * R * S * min(p.Cin, x.C) for x in xs),
                 lambda: "%s %dx%d %d->%d pyramid(%s)|0" % ("dgrad" if mode == 1 else "fwd", R, S, p.Cin, Cout, ",".join(str(x.H) for x in xs)))
    return outs


def conv_wgrad_seg(xs, dys, dw, Cout, R, S, pad, db=None):
    """dw += sum over the pyramid levels of wgrad(x_l, dy_l) in ONE launch (LDS-DMA kernel).  Returns (handled, fused_db)."""
    x0 = xs[0]
    dev, dt = x0.t.device, x0.t.dtype
    p = WgradParams()
    p.dw = dw.data_ptr()
    p.x_sW, p.dy_sP = x0.Cs, dys[0].Cs
    p.B, p.Cin, p.Cout = x0.B, x0.C, Cout
    p.R, p.S, p.stride, p.pad = R, S, 1, pad
    p.dtype = dtype_code(dt)
    p.nseg = len(xs)
    for l, (x, d) in enumerate(zip(xs, dys)):
        p.seg_x[l], p.seg_dy[l] = x.t.data_ptr(), d.t.data_ptr()
        p.seg_H[l], p.seg_W[l] = x.H, x.W
    if not (call("mpn_conv_wgrad_kernel_id", ctypes.byref(p)) & 1):
        return False, False
    _launch_wgrad(p, dev, db, lambda: sum(2.0 * x.B * x.H * x.W * Cout * R * S * x.C for x in xs),
                  lambda chunks: "wgrad %dx%d %d->%d pyramid(%s) chunks=%d|0" % (R, S, x0.C, Cout, ",".join(str(x.H) for x in xs), chunks),
                  plan="mpn_conv_wgrad_seg_plan")
    return True, db is not None


def _kseg_fill(p, srcs, H, W):
    """Describe the virtual concatenation cat_s(nearest_upsample(srcs[s])) (MpnConvParams / MpnWgradParams kseg_*)."""
    c = srcs[0].Cs
    p.kseg_n, p.kseg_c = len(srcs), c
    for i, a in enumerate(srcs):
        sh = (H // a.H).bit_length() - 1
        if a.Cs != c or a.C != c or (a.H << sh) != H or (a.W << sh) != W or a.B != srcs[0].B or a.t.dtype != srcs[0].t.dtype:
            raise _lib.MpnError("virtual concatenation: member %d does not up-sample to %dx%d by a power of two" % (i, H, W))
        p.kseg_shift[i] = sh
        p.kseg_x[i] = a.t.data_ptr()


def cat_supported(srcs, H, W):
    """True when conv_forward_cat / conv_wgrad_cat serve cat(up(srcs)) at H x W: 16-bit members of 128 channels, power-of-two ratios."""
    if not srcs or len(srcs) > 4 or not is16(srcs[0].t.dtype):
        return False
    for a in srcs:
        sh = (H // max(a.H, 1)).bit_length() - 1
        if a.C != 128 or a.Cs != 128 or (a.H << sh) != H or (a.W << sh) != W or a.t.dtype != srcs[0].t.dtype:
            return False
    return True


def conv_forward_cat(srcs, H, W, w, Cout, bias=None, act=0, tag="", res=None):
    """3x3 / stride 1 / pad 1 convolution over torch.cat([nearest_upsample(s) for s in srcs], 1) WITHOUT materialising it
    (posenet.py:311-315: the 512-channel input of conv2).  w: [Cout][3][3][len(srcs) * 128].  res: same-size tensor added in the
    epilogue (act 3 = ReLU after it): the expanded class maps of the members conv2cls_* serve."""
    x0 = srcs[0]
    dt, dev = x0.t.dtype, x0.t.device
    out = Act.empty(x0.B, H, W, Cout, dt, dev, False, tag)
    p = ConvParams()
    _kseg_fill(p, srcs, H, W)
    p.w, p.y = w.data_ptr(), out.t.data_ptr()
    p.bias = bias.data_ptr() if bias is not None else None
    p.B, p.H, p.W, p.Ho, p.Wo = x0.B, H, W, H, W
    p.Cin, p.Cout, p.Cout_store = p.kseg_n * p.kseg_c, Cout, out.Cs
    p.x_sW, p.x_sH, p.x_sB = p.Cin, W * p.Cin, H * W * p.Cin          # geometry of the virtual tensor (not dereferenced)
    p.y_sB, p.y_sP = H * W * out.Cs, out.Cs
    p.R, p.S, p.stride, p.pad = 3, 3, 1, 1
    p.act, p.dtype = act, dtype_code(dt)
    if res is not None:
        assert res.t.dtype == dt and (res.B, res.H, res.W, res.Cs) == (out.B, H, W, out.Cs)
        p.res, p.res_mode = res.t.data_ptr(), 1
        p.res_sB, p.res_sP = H * W * res.Cs, res.Cs
        p.res_H, p.res_W = H, W
    _launch_conv(p, lambda: 2.0 * x0.B * H * W * Cout * 9 * p.Cin,
                 lambda: "fwd 3x3 %d->%d @%dx%d s1 virtual-cat%s%s|%d" % (p.Cin, Cout, H, W, " bias" if bias is not None else "", " act%d" % act if act else "",
                                                                         sum(a.t.numel() for a in srcs) * 2 + out.t.numel() * 2))
    return out


def conv_wgrad_cat(srcs, H, W, dy, dw, Cout, db=None):
    """dw += wgrad of the convolution of conv_forward_cat (x = the virtual concatenation); db fused as in conv_wgrad."""
    x0 = srcs[0]
    dev, dt = x0.t.device, x0.t.dtype
    p = WgradParams()
    _kseg_fill(p, srcs, H, W)
    Cin = p.kseg_n * p.kseg_c
    p.dy, p.dw = dy.t.data_ptr(), dw.data_ptr()
    p.dy_sP = dy.Cs
    p.x_sW, p.x_sH, p.x_sB = Cin, W * Cin, H * W * Cin
    p.B, p.H, p.W, p.Cin = x0.B, H, W, Cin
    p.Ho, p.Wo, p.Cout = H, W, Cout
    p.R, p.S, p.stride, p.pad = 3, 3, 1, 1
    p.dtype = dtype_code(dt)
    _launch_wgrad(p, dev, db, lambda: 2.0 * x0.B * H * W * Cout * 9 * Cin,
                  lambda chunks: "wgrad 3x3 %d->%d @%dx%d s1 virtual-cat chunks=%d|%d" % (Cin, Cout, H, W, chunks,
                                                                                       sum(a.t.numel() for a in srcs) * 2 + dy.t.numel() * 2))
    return db is not None


# ---- conv2 of the keypoint head by position classes (csrc/conv2cls.hip) -------------------------------------------------------------
def conv2cls_supported(srcs, H, W):
    """The class formulation serves exactly posenet.py:311-315's geometry: four dense 128-channel members of one element type at 1/8,
    1/4, 1/2, 1/1 of an H x W (multiples of 8) output."""
    if len(srcs) != 4 or H % 8 or W % 8:
        return False
    if any(a.C != 128 or a.Cs != 128 or a.t.dtype != srcs[0].t.dtype or a.B != srcs[0].B for a in srcs):
        return False
    return [(a.H * f, a.W * f) for a, f in zip(srcs, (8, 4, 2, 1))] == [(H, W)] * 4


_CONST_F32 = {}


def _const_f32(dev, value, n):
    """A constant f32 vector on ``dev``, filled once (on the launch stream of its first user) and kept for the life of the process."""
    key = (str(dev), value, n)
    t = _CONST_F32.get(key)
    if t is None:
        t = _CONST_F32[key] = torch.empty(n, dtype=torch.float32, device=dev)
        call("mpn_fill_f32", ptr(t), value, n, stream_ptr())
    return t


class Conv2ClsOperands(object):
    """Per-forward operands of the class formulation, all derived from the f32 master filter [O][3][3][4 C] in four launches: the
    combined filters (f32), their compute-dtype copies, and the transposed (input-gradient) copies when a backward pass will follow.
    tap_unscale[m] (fp16 only, else None): the per-channel epilogue multiplier s^2 (s = 8, 4) of the tap input-gradient launch, which
    contracts conv2cls_tapsum's G / s^2 there (include/mpn.h)."""

    def __init__(self, w_master, O, C, dtype, want_t):
        dev = w_master.device
        n = call("mpn_conv2cls_comb_elems", O, C)
        self.O, self.C = O, C
        self.nm, self.nc, self.nt = O * 9 * 2 * C, 9 * O * 9 * C, 9 * O * C
        comb32 = torch.empty(n, dtype=torch.float32, device=dev)
        call("mpn_conv2cls_combine", ptr(w_master), ptr(comb32), O, C, stream_ptr())
        nf = self.nm + 2 * self.nc                                              # main filter + the two frame-filter sets
        if is16(dtype):
            self.comb = torch.empty(n, dtype=dtype, device=dev)
            cast_lowp(comb32, self.comb)
        else:
            self.comb = comb32                                                  # f32 kernels read the f32 filters in place
        self.wm = self.comb[: self.nm]                                         # [O][3][3][2C]
        self.wc = [self.comb[self.nm + m * self.nc: self.nm + (m + 1) * self.nc] for m in range(2)]      # [9 O][3][3][C], members q5 / q4
        self.wtap = [self.comb[nf + m * self.nt: nf + (m + 1) * self.nt] for m in range(2)]              # [9 O][C]: nine 1x1 filters
        self.wm_t = self.wtap_t = None
        self.tap_unscale = [None, None]
        if want_t:
            if dtype == torch.float16:
                self.tap_unscale = [_const_f32(dev, 64.0, C), _const_f32(dev, 16.0, C)]
            self.wm_t = torch.empty((2 * C, 3, 3, O), dtype=dtype, device=dev)
            weight_transpose(comb32[: self.nm], self.wm_t, O, 9, 2 * C, O)
            self.wtap_t = []                                                    # [C][1][1][9 O]: the member as nine 1x1 convolutions, transposed
            for m in range(2):
                t = torch.empty((C, 1, 1, 9 * O), dtype=dtype, device=dev)
                weight_transpose(comb32[nf + m * self.nt: nf + (m + 1) * self.nt], t, 9 * O, 1, C, 9 * O)
                self.wtap_t.append(t)
        self.keep = comb32


def _cls_operand(name, a, dtypes, groups, per_class=True):
    """The conv2cls_* kernels read their operand as dense NHWC and take O from its channel storage: refuse, before anything is allocated,
    what they would misread (a non-contiguous tensor, a width that is not 9 O or an O the vector width does not divide, an element type
    the entry point rejects).  Returns O."""
    if a.t.dtype not in dtypes:
        raise _lib.MpnError("%s: unsupported dtype %s" % (name, a.t.dtype))
    if not a.t.is_contiguous():
        raise _lib.MpnError("%s: the operand must be dense NHWC (strides %s of shape %s)" % (name, tuple(a.t.stride()), tuple(a.t.shape)))
    if per_class and a.Cs % 9:
        raise _lib.MpnError("%s: %d stored channels are not nine class / tap planes" % (name, a.Cs))
    O = a.Cs // 9 if per_class else a.Cs
    if O <= 0 or O % groups:
        raise _lib.MpnError("%s: %d channels per plane (need a positive multiple of %d)" % (name, O, groups))
    return O


_CLS_TYPES = (torch.float32, torch.bfloat16, torch.float16)


def conv2cls_expand(m8, m4, B, H, W, O, dtype):
    code = dtype_code(dtype)
    if H <= 0 or W <= 0 or H % 8 or W % 8:
        raise _lib.MpnError("conv2cls_expand: %d x %d is not a positive multiple of 8 x 8" % (H, W))
    for a, s in ((m8, 8), (m4, 4)):
        if _cls_operand("conv2cls_expand", a, (torch.float32,), 8) != O or tuple(a.t.shape[:3]) != (B, H // s, W // s):
            raise _lib.MpnError("conv2cls_expand: class maps %s do not belong to a [%d, %d, %d, %d] output at 1/%d" % (tuple(a.t.shape), B, H, W, O, s))
    e = Act(torch.empty((B, H, W, O), dtype=dtype, device=m8.t.device), O)
    call("mpn_conv2cls_expand", ptr(m8.t), ptr(m4.t), ptr(e.t), B, H, W, O, code, stream_ptr())
    return e


def pool_dtype(dtype):
    """Storage type of the class sums of a dy of type ``dtype``: sums of up to 36 fp16 values do not fit fp16 (csrc/conv2cls.hip)."""
    return torch.float32 if dtype == torch.float16 else dtype


def conv2cls_pool(dy):
    """(P8 [B, H/8, W/8, 9 O], P4 [B, H/4, W/4, 9 O]): per-class sums of dy over 8 x 8 / 4 x 4 blocks (one pass over dy), in pool_dtype(dy's
    type): f32 for an fp16 dy."""
    B, H, W = dy.B, dy.H, dy.W
    O = _cls_operand("conv2cls_pool", dy, _CLS_TYPES, 8, per_class=False)
    if H <= 0 or W <= 0 or H % 8 or W % 8:
        raise _lib.MpnError("conv2cls_pool: %d x %d is not a positive multiple of 8 x 8" % (H, W))
    pt = pool_dtype(dy.t.dtype)
    p8 = Act(torch.empty((B, H // 8, W // 8, 9 * O), dtype=pt, device=dy.t.device), 9 * O)
    p4 = Act(torch.empty((B, H // 4, W // 4, 9 * O), dtype=pt, device=dy.t.device), 9 * O)
    call("mpn_conv2cls_pool", ptr(dy.t), ptr(p8.t), ptr(p4.t), B, H, W, O, dtype_code(dy.t.dtype), stream_ptr())
    return p8, p4


def conv2cls_classsum(t):
    """Per-tap products (f32 [B, h, w, 9 O]) -> class maps of the same shape (csrc/conv2cls.hip: conv2cls_classsum_kernel)."""
    O = _cls_operand("conv2cls_classsum", t, (torch.float32,), 4)
    m = Act(torch.empty_like(t.t), t.C)
    call("mpn_conv2cls_classsum", ptr(t.t), ptr(m.t), t.B, t.H, t.W, O, stream_ptr())
    return m


def conv2cls_tapsum(pc, s=None, dtype=None):
    """Class sums [B, h, w, 9 O] (conv2cls_pool's, of the member up-sampled by s = 8 or 4, for a dy of type ``dtype``; default: pc's own
    type) -> per-tap sums of the same shape in ``dtype``; fp16: divided by s^2, so s must be given there (csrc/conv2cls.hip:
    conv2cls_tapsum_kernel)."""
    dtype = pc.t.dtype if dtype is None else dtype
    if dtype not in _CLS_TYPES:
        raise _lib.MpnError("conv2cls_tapsum: unsupported dtype %s" % dtype)
    if s is None and dtype != torch.float16:
        s = 8                                                                   # (nothing is scaled: either member's value does)
    if s not in (8, 4):
        raise _lib.MpnError("conv2cls_tapsum: the member is up-sampled by 8 or 4, not %r" % (s,))
    O = _cls_operand("conv2cls_tapsum", pc, (pool_dtype(dtype),), 8)
    g = Act(torch.empty(pc.t.shape, dtype=dtype, device=pc.t.device), pc.C)
    call("mpn_conv2cls_tapsum", ptr(pc.t), ptr(g.t), pc.B, pc.H, pc.W, O, s, dtype_code(dtype), stream_ptr())
    return g


def conv_out_hw(H, W, R, S, stride, pad):
    return (H + 2 * pad - R) // stride + 1, (W + 2 * pad - S) // stride + 1


def conv_forward(x, w, Cout, R, S, stride, pad, bias=None, scale=None, act=0, res=None, res_mode=0,
                 want_stats=False, out_f32=False, out=None, accumulate=False, mode=0, out_hw=None,
                 cin=None, x_geom=None, y_geom=None, cout_store=None, needs_grad=False, tag="", bnb=None, bn_fin=None, res_mask=None,
                 _cls=None):
    """Implicit-GEMM convolution.  x: Act.  w: compute-dtype tensor laid out [Cout][R][S][Cin].

    mode 0 = forward gather, mode 1 = dgrad gather (then ``out_hw`` is the input-gradient size and
    ``w`` is the transposed copy).  x_geom=(H, W, sB, sH, sW) overrides the source geometry (stem).
    y_geom=(ptr_tensor, sB, sP) writes into a slice of a larger buffer.

    Returns (Act|None, second).  ``second`` is None unless one of these was asked for:
    want_stats: the forward statistics table [tiles, Cout, 2] — or, with ``bn_fin`` (a BNFinalize) when the launch finalized in
    place (fin_in_launch), the finished BNState;
    bnb (a BNBackward; this launch completes dz of that BatchNorm): a BNBackwardResult.
    """
    dev = x.t.device
    dt = x.t.dtype
    if (DGRAD_S2_CLASSES and _cls is None and mode == 1 and stride == 2 and not out_f32
            and res is None and not want_stats and bias is None and scale is None and act == 0 and x_geom is None and y_geom is None
            and out_hw is not None and cout_store is None):
        if R == 3 and S == 3 and pad == 1:
            return _conv_dgrad_s2_classes(x, w, Cout, out_hw, cin, out, accumulate, bnb, needs_grad, tag)
        if R == 1 and S == 1 and pad == 0 and accumulate and bnb is None and out is not None:
            # 1x1 / stride 2 (the ResNet down-sampling shortcut): only the pixels (2 i, 2 j) of dx receive anything — one class, one tap.  Needs an
            # existing dx to add to (the other three quarters keep what they hold) and no epilogue statistics (they would need every pixel).
            conv_forward(x, w, Cout, 1, 1, 1, 0, out=out, accumulate=True, mode=0, out_hw=((out_hw[0] + 1) // 2, (out_hw[1] + 1) // 2), cin=cin,
                         _cls=ParityClass(0, 0, None, 0, one_tap=True))
            return out, None
    Cin = cin if cin is not None else round_up(x.C, 32 if is16(dt) else 16)
    if x_geom is None:
        H, W = x.H, x.W
        sB, sH, sW = x.H * x.W * x.Cs, x.W * x.Cs, x.Cs
    else:
        H, W, sB, sH, sW = x_geom
    if out_hw is None:
        Ho, Wo = conv_out_hw(H, W, R, S, stride, pad)
    else:
        Ho, Wo = out_hw
    odt = torch.float32 if out_f32 else dt
    p = ConvParams()
    if y_geom is None:
        if out is None:
            out = Act.empty(x.B, Ho, Wo, Cout, odt, dev, needs_grad, tag)
        if _cls is None:
            assert out.t.dtype == odt and (out.B, out.H, out.W) == (x.B, Ho, Wo), "conv output geometry mismatch"
            p.y_sB, p.y_sP = Ho * Wo * out.Cs, out.Cs
        else:       # parity class (a, c) of a stride-2 input gradient (mpn.h: y_step): output pixel (i, j) -> (2 i + a, 2 j + c) of `out`
            ca, cc_, p.y_H, p.y_W = _cls.a, _cls.c, out.H, out.W
            assert out.t.dtype == odt and out.B == x.B and out.Cs == round_up(Cout, 32) and cout_store is None, "class launch: output tensor mismatch"
            assert 2 * (Ho - 1) + ca < out.H and 2 * (Wo - 1) + cc_ < out.W, "class launch: class grid exceeds the output"
            p.y_step, p.y_oh, p.y_ow = 2, ca, cc_
            if _cls.one_tap:                            # 1x1 filter: its only tap
                p.w_taps, p.wtap0, p.wtap_dr, p.wtap_ds = 1, 0, 0, 0
            else:                                       # 3x3, pad 1: tap (t_r, t_s) of the class is filter tap (a + 1 - 2 t_r, c + 1 - 2 t_s)
                p.w_taps, p.wtap0, p.wtap_dr, p.wtap_ds = 9, (ca + 1) * 3 + (cc_ + 1), -6, -2
            p.y_sB, p.y_sP = out.H * out.W * out.Cs, out.Cs
        p.y = out.t.data_ptr()
        p.Cout_store = out.Cs if cout_store is None else cout_store
    else:
        yt, ysB, ysP = y_geom
        p.y = yt.data_ptr()
        p.y_sB, p.y_sP = ysB, ysP
        p.Cout_store = cout_store if cout_store is not None else round_up(Cout, 4)
    p.x = x.t.data_ptr()
    p.w = w.data_ptr()
    p.bias = bias.data_ptr() if bias is not None else None
    p.scale = scale.data_ptr() if scale is not None else None
    p.x_sB, p.x_sH, p.x_sW = sB, sH, sW
    p.B, p.H, p.W, p.Cin = x.B, H, W, Cin
    p.Ho, p.Wo, p.Cout = Ho, Wo, Cout
    p.R, p.S, p.stride, p.pad = R, S, stride, pad
    p.mode, p.act, p.accumulate = mode, act, 1 if accumulate else 0
    p.dtype = dtype_code(dt)
    p.out_f32 = 1 if (out_f32 and dt != torch.float32) else 0
    if res is not None:
        assert res.t.dtype == odt
        p.res = res.t.data_ptr()
        p.res_mode = res_mode
        p.res_sB, p.res_sP = res.H * res.W * res.Cs, res.Cs
        p.res_H, p.res_W = res.H, res.W
        if res_mask is not None:          # residual * mask bits (bn_act(want_mask=True) layout): res_mode 1 only
            assert res_mode == 1
            p.res_mask = res_mask.data_ptr()
    stats = None
    keep = None
    if want_stats:
        tiles = call("mpn_conv_stats_tiles", ctypes.byref(p))
        stats = torch.empty((tiles, Cout, 2), dtype=torch.float32, device=dev)
        p.stats = stats.data_ptr()
        if bn_fin is not None and fin_in_launch(tiles, Cout):
            # the last workgroup of every channel tile turns the tile partials into the BatchNorm coefficients (no finalize launch):
            # the BNState comes back in the stats slot
            keep, stats = stats, BNState(Cout, dev)
            p.fin_counters = fin_counters(dev).data_ptr()
            p.fin_gamma, p.fin_beta = bn_fin.gamma.data_ptr(), bn_fin.beta.data_ptr()
            p.fin_rm = bn_fin.running_mean.data_ptr() if bn_fin.running_mean is not None else None
            p.fin_rv = bn_fin.running_var.data_ptr() if bn_fin.running_var is not None else None
            p.fin_out = stats.mean.data_ptr()
            p.fin_count, p.fin_momentum, p.fin_eps = float(x.B * Ho * Wo), bn_fin.momentum, bn_fin.eps
    if bnb is not None:
        # this launch completes dz of a BatchNorm: its backward statistics ride in the epilogue (a BNBackwardResult in the stats slot)
        by, bz, st = bnb.y, bnb.z, bnb.state
        assert y_geom is None and not out_f32 and by.t.shape == out.t.shape and by.t.dtype == out.t.dtype
        tiles = call("mpn_conv_stats_tiles", ctypes.byref(p))
        if _cls is None:
            stats = torch.empty((tiles, Cout, 2), dtype=torch.float32, device=dev)
            p.bnb_partial = stats.data_ptr()
        else:       # rows [tile0, tile0 + tiles) of the table the four class launches share
            stats = _cls.table
            assert _cls.tile0 + tiles <= stats.shape[0]
            p.bnb_partial = stats.data_ptr() + _cls.tile0 * Cout * 2 * 4
        p.bnb_y = by.t.data_ptr()
        p.bnb_z = bz.t.data_ptr() if bz is not None else None
        if bz is not None and bz.mask is not None:          # the ReLU mask as bits (bn_act(want_mask=True)): z itself is not read
            p.bnb_mask, p.bnb_z = bz.mask.data_ptr(), None
        p.bnb_mean, p.bnb_invstd = st.mean.data_ptr(), st.invstd.data_ptr()
        p.bnb_scale, p.bnb_shift = st.scale.data_ptr(), st.shift.data_ptr()
        p.bnb_relu = 1 if bnb.relu else 0
        fin = bnb.fin
        if _cls is None and fin is not None and fin_in_launch(tiles, Cout):
            # ... and the last workgroup of every channel tile finishes the reduction: dgamma / dbeta and the (k1, k2, k3) of
            # dy = k1*g + k2*y + k3 (mpn_bn_bwd_finalize's work); the partial table dies with this call (keep), the coefficients
            # (frozen statistics: none, k1 is the forward scale) come back
            keep, coef = stats, (torch.empty((3, Cout), dtype=torch.float32, device=dev) if fin.train else None)
            p.fin_counters = fin_counters(dev).data_ptr()
            p.fin_gamma = fin.gamma.data_ptr()
            p.fin_out = coef.data_ptr() if coef is not None else None
            p.fin_dgamma = fin.dgamma.data_ptr() if fin.dgamma is not None else None
            p.fin_dbeta = fin.dbeta.data_ptr() if fin.dbeta is not None else None
            p.fin_count, p.fin_train = float(x.B * Ho * Wo), 1 if fin.train else 0
            stats = BNBackwardResult(None, coef, coef is None)
        else:
            stats = BNBackwardResult(stats, None, False)

    def flops():
        # algorithmic FLOPs: 2 * output pixels * Cout * taps * Cin; a stride-s dgrad only has 1/s^2 live taps
        live = (R * S) / float(stride * stride) if mode == 1 else R * S
        return 2.0 * x.B * Ho * Wo * Cout * live * min(Cin, x.C if x_geom is None else Cin)

    def label():
        es = 2 if is16(dt) else 4
        byts = x.B * H * W * Cin * es + x.B * Ho * Wo * p.Cout_store * (4 if out_f32 else es) * (2 if accumulate else 1) \
            + (x.B * Ho * Wo * p.Cout_store * es if res is not None and res_mode == 1 else 0)
        return "%s %dx%d %d->%d @%dx%d s%d%s%s%s%s%s|%d" % (
            ("dgrad s2 class(%d,%d)" % (_cls.a, _cls.c)) if _cls is not None else ("dgrad" if mode == 1 else "fwd"), R, S, Cin, Cout, Ho, Wo, stride,
            " stats" if want_stats else "",
            " bias" if bias is not None else "", " act%d" % act if act else "", " res%d" % res_mode if res is not None else "",
            " acc" if accumulate else "", byts)

    _launch_conv(p, flops, label)
    return out, stats


DGRAD_S2_CLASSES = os.environ.get("MPN_DGRAD_S2_CLASSES", "1") != "0"


def _conv_dgrad_s2_classes(dy, wt, Cout, out_hw, cin, out, accumulate, bnb, needs_grad, tag):
    """Input gradient of a 3x3 / stride 2 / pad 1 convolution as four parity-class launches (mpn.h: y_step): the pixel (h, w) of dx only
    receives the taps with r = (h + 1) mod 2 (+ 2), s likewise — 1, 2, 2 or 4 of the nine — so each class is a small stride-1 gather over
    dy written to every second row / column of dx; together 2.25 taps per pixel instead of the 9 (6.75 of them against zeros) of the
    strided gather.  The BatchNorm-backward statistics of the epilogue (bnb) fill consecutive row ranges of ONE partial table."""
    H, W = out_hw
    dev, dt = dy.t.device, dy.t.dtype
    if out is None:
        out = Act.empty(dy.B, H, W, Cout, dt, dev, needs_grad, tag)
    plan = dgrad_s2_class_plan(dy.B, H, W)
    rows = sum(t for _, _, _, _, t, _ in plan)
    part = torch.empty((rows, Cout, 2), dtype=torch.float32, device=dev) if bnb is not None else None
    for a, c, ho, wo, t, tile0 in plan:
        if t > 0:
            conv_forward(dy, wt, Cout, 1 + a, 1 + c, 1, 0, out=out, accumulate=accumulate, mode=0, out_hw=(ho, wo), cin=cin, bnb=bnb,
                         _cls=ParityClass(a, c, part, tile0))
    return out, (BNBackwardResult(part, None, False) if bnb is not None else None)


def dgrad_s2_class_plan(B, H, W, tile_pixels=128):
    """The four parity classes of a 3x3 / stride 2 / pad 1 input gradient over a [B][H][W] dx: (a, c, class rows, class columns, pixel tiles,
    first row of the class in the shared statistics table).  Class (a, c) owns the pixels (2 i + a, 2 j + c); its launch has (1 + a) x (1 + c)
    taps, tap (t_r, t_s) being filter tap (a + 1 - 2 t_r, c + 1 - 2 t_s) applied to dy[i + t_r][j + t_s]."""
    plan, tile0 = [], 0
    for a in (0, 1):
        for c in (0, 1):
            ho, wo = (H - a + 1) // 2, (W - c + 1) // 2
            t = (B * ho * wo + tile_pixels - 1) // tile_pixels
            plan.append((a, c, ho, wo, t, tile0))
            tile0 += t
    return plan


def conv_wgrad(x, dy, dw, Cout, R, S, stride, pad, cin=None, x_geom=None, db=None):
    """dw (f32 view laid out [Cout][R][S][Cin], contiguous) += wgrad(x, dy).  db (f32 [Cout], optional) += column sums of
    dy, fused into the same kernel where the LDS-DMA path serves the launch; returns True if db was taken care of."""
    dev = x.t.device
    dt = x.t.dtype
    p = WgradParams()
    if x_geom is None:
        H, W = x.H, x.W
        sB, sH, sW = x.H * x.W * x.Cs, x.W * x.Cs, x.Cs
        Cin = cin if cin is not None else x.C
    else:
        H, W, sB, sH, sW = x_geom
        Cin = cin
    p.x, p.dy, p.dw = x.t.data_ptr(), dy.t.data_ptr(), dw.data_ptr()
    p.x_sB, p.x_sH, p.x_sW = sB, sH, sW
    p.dy_sP = dy.Cs
    p.B, p.H, p.W, p.Cin = x.B, H, W, Cin
    p.Ho, p.Wo, p.Cout = dy.H, dy.W, Cout
    p.R, p.S, p.stride, p.pad = R, S, stride, pad
    p.dtype = dtype_code(dt)
    fused_db = db is not None and bool(call("mpn_conv_wgrad_kernel_id", ctypes.byref(p)) & 1)
    _launch_wgrad(p, dev, db if fused_db else None, lambda: 2.0 * x.B * dy.H * dy.W * Cout * R * S * Cin,
                  lambda chunks: "wgrad %dx%d %d->%d @%dx%d s%d chunks=%d|%d" % (R, S, Cin, Cout, dy.H, dy.W, stride, chunks,
                                                                               (x.B * H * W * Cin + x.B * dy.H * dy.W * dy.Cs) * (2 if is16(dt) else 4)))
    return fused_db


def bias_grad(dy, db, C):
    """db[C] (f32) += column sums of dy."""
    v = 4 if dy.t.dtype == torch.float32 else 8
    g = dy.Cs // v
    if dy.P <= 256 or dy.Cs % v != 0 or (g & (g - 1)) != 0:
        call("mpn_colsum_rows", ptr(dy.t), dtype_code(dy.t.dtype), dy.P, C, dy.Cs, ptr(db), stream_ptr())
        return
    chunks = call("mpn_channel_sum_chunks", dy.P, dy.Cs, dtype_code(dy.t.dtype))
    ws = workspace(chunks * C * 4, dy.t.device, slot=2)
    call("mpn_channel_sum", ptr(dy.t), dtype_code(dy.t.dtype), dy.P, C, dy.Cs, ptr(ws), chunks, stream_ptr())
    call("mpn_reduce_partials", ptr(ws), chunks, C, ptr(db), 1, stream_ptr())


def weight_transpose(w_master, wt, Cout, RS, Cin, Cout_pad):
    call("mpn_weight_transpose", ptr(w_master), ptr(wt), Cout, RS, Cin, Cout_pad, dtype_code(wt.dtype), stream_ptr())


def cast_lowp(src, dst):
    """f32 -> bf16 / f16 copy (dst's dtype decides)."""
    call("mpn_cast_f32", ptr(src), ptr(dst), src.numel(), dtype_code(dst.dtype), stream_ptr())


_fin_counters = {}
# In-launch BatchNorm finalize (mpn.h: fin_*).  Up to FIN_MAX_TILES pixel tiles one workgroup per channel tile does the whole
# reduction; beyond that a single reader behind an acquire is slower than the separate (wide) finalize launch (round 2: +0.85 ms at
# <= 256 tiles), and so were the two-level form and the finalize inside the bn_act launch (round 3: +0.26 / +0.2 ms; both removed).
FIN_MAX_TILES = int(os.environ.get("MPN_BN_FIN_MAX_TILES", "64"))
FIN_COUNTERS = 64


def fin_in_launch(tiles, Cout=2):
    """The in-launch finalize reads the partial table as float4 pairs of channels: even widths only (every BatchNorm of the network is;
    an odd width takes the separate finalize launch instead of failing with BADARG — ADVICE r5)."""
    return tiles <= FIN_MAX_TILES and Cout % 2 == 0


def fin_counters(device):
    """Ticket counters of the in-launch BatchNorm finalize (mpn.h: fin_counters): zero between launches.  One buffer per
    (device, launch stream): launches of one stream run one after another, launches of different streams (a second model or a
    Tester beside training) must not draw tickets from the same counters."""
    key = (device, stream_handle() if device.type == "cuda" else 0)
    t = _fin_counters.get(key)
    if t is None:
        t = _fin_counters[key] = torch.zeros(FIN_COUNTERS, dtype=torch.int32, device=device)
    return t


class BNState(object):
    __slots__ = ("mean", "invstd", "scale", "shift")

    def __init__(self, C, device):
        buf = torch.empty((4, C), dtype=torch.float32, device=device)
        self.mean, self.invstd, self.scale, self.shift = buf[0], buf[1], buf[2], buf[3]


# What travels between the engine and conv_forward when BatchNorm work rides in a convolution launch (plain records, read by name).
# conv_forward(bn_fin=): the in-launch forward finalize of train-mode statistics
BNFinalize = namedtuple("BNFinalize", "gamma beta running_mean running_var momentum eps")
# BNBackward.fin: the in-launch backward finalize (train: batch statistics; dgamma / dbeta: the gradient slices to add to, or None)
BNBackwardFinalize = namedtuple("BNBackwardFinalize", "gamma train dgamma dbeta")
# conv_forward(bnb=): the BatchNorm whose dz the launch completes — y its input, z its output (only when the ReLU mask must be read
# from it, else None), state its BNState
BNBackward = namedtuple("BNBackward", "y z state relu fin", defaults=(None,))
# Act.bn_src: the BatchNorm that produced the activation
BNSource = namedtuple("BNSource", "y state relu has_res wants_stats layer train_stats")
# conv_forward(_cls=): parity class (a, c) of a stride-2 input gradient; its statistics go to rows [tile0, ...) of the shared table
ParityClass = namedtuple("ParityClass", "a c table tile0 one_tap", defaults=(False,))
# What a launch given bnb= returns, exactly one of: the per-tile partial table [tiles, C, 2] (reduced, not finalized); coef [3, C]
# = k1, k2, k3 (finalized in the launch, batch statistics); frozen (finalized in the launch, frozen statistics: k1 is the forward
# scale, no tensor).  A finalized launch never hands its partial table out: partial is None then.
BNBackwardResult = namedtuple("BNBackwardResult", "partial coef frozen")


def bn_finalize_train(stats, count, gamma, beta, rm, rv, momentum=0.1, eps=1e-5):
    C = stats.shape[1]
    st = BNState(C, stats.device)
    call("mpn_bn_finalize_train", ptr(stats), stats.shape[0], C, count, ptr(gamma), ptr(beta), ptr(rm), ptr(rv),
         momentum, eps, ptr(st.mean), ptr(st.invstd), ptr(st.scale), ptr(st.shift), stream_ptr())
    return st


def bn_finalize_eval(gamma, beta, rm, rv, eps=1e-5):
    C = gamma.numel()
    st = BNState(C, gamma.device)
    call("mpn_bn_finalize_eval", C, ptr(gamma), ptr(beta), ptr(rm), ptr(rv), eps, ptr(st.mean), ptr(st.invstd),
         ptr(st.scale), ptr(st.shift), stream_ptr())
    return st


def bn_act(y, st, relu, res=None, needs_grad=False, tag="", want_mask=False):
    """z = act(y * scale + shift [+ res]).  want_mask (with relu): also the sign bits of z, one byte per 16-byte chunk — all the
    backward of relu(bn(.) + shortcut) needs of z (the ReLU mask), at 1/16 of z's bytes (z.mask)."""
    z = Act(torch.empty_like(y.t), y.C, needs_grad, tag)
    if want_mask and relu:
        z.mask = torch.empty((y.P, y.Cs // (4 if y.t.dtype == torch.float32 else 8)), dtype=torch.uint8, device=y.t.device)
    call("mpn_bn_act_forward", ptr(y.t), ptr(res.t) if res is not None else None, ptr(z.t), ptr(st.scale), ptr(st.shift),
         y.P, y.C, y.Cs, 1 if relu else 0, dtype_code(y.t.dtype), ptr(z.mask), stream_ptr())
    return z


def masked_copy(dz, mask_bits, out):
    """out = dz * mask (mask bits in bn_act's layout): the shortcut gradient of relu(bn(.) + shortcut), materialised."""
    call("mpn_bn_bwd_apply", ptr(dz.t), None, None, None, None, None, None, None, None, ptr(out.t), 0, dz.P, dz.C, dz.Cs, 1,
         dtype_code(dz.t.dtype), ptr(mask_bits), stream_ptr())
    return out


def bn_backward(dz, z, y, st, gamma, relu, train, dgamma=None, dbeta=None, want_dy=True, dres=None, dres_acc=False, remask=False,
                fused=None):
    """Returns dy (Act or None).  dres (Act) receives/accumulates g = dz*(z>0).  remask=True (forward without a
    residual input): the ReLU mask is recomputed from y and the forward's scale/shift instead of reading z.
    fused: the BNBackwardResult of the launch that wrote dz (conv_forward(bnb=...)): with its per-tile (sum g, sum g*xhat)
    the reduction pass over dz / y / z is skipped, with its coefficients (or frozen) the finalize as well."""
    dev = y.t.device
    P, C, Cs = y.P, y.C, y.Cs
    dc = dtype_code(y.t.dtype)
    k1, k2, k3 = st.scale, None, None        # frozen BN, no parameter gradients: dy = g * gamma * invstd
    if fused is not None and fused.partial is None:
        # reduction AND finalize already happened in the launch that completed dz (BNBackward.fin): dgamma / dbeta are in place,
        # coef = [3][C] k1, k2, k3 (frozen: none, k1 = gamma * invstd = the forward scale)
        if not fused.frozen:
            k1, k2, k3 = fused.coef[0], fused.coef[1], fused.coef[2]
    elif train or dgamma is not None or dbeta is not None:
        if fused is not None:
            part, chunks = fused.partial, fused.partial.shape[0]
        else:
            chunks = call("mpn_bn_bwd_chunks", P, Cs, dc)
            part = workspace(chunks * C * 2 * 4, dev, slot=3)
            call("mpn_bn_bwd_reduce", ptr(dz.t), ptr(z.t) if (relu and not remask) else None, ptr(y.t), ptr(st.mean), ptr(st.invstd),
                 ptr(st.scale) if remask else None, ptr(st.shift) if remask else None, ptr(part),
                 chunks, P, C, Cs, 1 if relu else 0, dc, stream_ptr())
        coef = torch.empty((3, C), dtype=torch.float32, device=dev) if train else None
        call("mpn_bn_bwd_finalize", ptr(part), chunks, C, P, ptr(gamma), ptr(st.mean), ptr(st.invstd), 1 if train else 0,
             ptr(dgamma), ptr(dbeta), ptr(coef), stream_ptr())
        if train:
            k1, k2, k3 = coef[0], coef[1], coef[2]
    dy = None
    if want_dy or dres is not None:
        if want_dy:
            dy = Act(torch.empty_like(y.t), C)
        bits = z.mask if (relu and not remask) else None
        call("mpn_bn_bwd_apply", ptr(dz.t), ptr(z.t) if (relu and not remask and bits is None) else None, ptr(y.t), ptr(k1), ptr(k2), ptr(k3),
             ptr(st.scale) if remask else None, ptr(st.shift) if remask else None,
             ptr(dy.t) if dy is not None else None, ptr(dres.t) if dres is not None else None,
             1 if dres_acc else 0, P, C, Cs, 1 if relu else 0, dc, ptr(bits), stream_ptr())
    return dy


def maxpool_forward(x, needs_grad=False):
    Ho, Wo = (x.H + 2 - 3) // 2 + 1, (x.W + 2 - 3) // 2 + 1
    y = Act(torch.empty((x.B, Ho, Wo, x.Cs), dtype=x.t.dtype, device=x.t.device), x.C, needs_grad)
    idx = torch.empty((x.B, Ho, Wo, x.Cs), dtype=torch.uint8, device=x.t.device) if needs_grad else None
    call("mpn_maxpool3x3s2_forward", ptr(x.t), ptr(y.t), ptr(idx), x.B, x.H, x.W, x.Cs, Ho, Wo, dtype_code(x.t.dtype), stream_ptr())
    return y, idx


def maxpool_backward(dy, idx, x_like):
    dx = Act(torch.empty_like(x_like.t), x_like.C)
    call("mpn_maxpool3x3s2_backward", ptr(dy.t), ptr(idx), ptr(dx.t), x_like.B, x_like.H, x_like.W, x_like.Cs, dy.H, dy.W,
         dtype_code(dy.t.dtype), stream_ptr())
    return dx


def upsample_backward(dfine, dcoarse, accumulate):
    call("mpn_upsample_nearest_backward", ptr(dfine.t), ptr(dcoarse.t), dfine.B, dfine.H, dfine.W, dcoarse.H, dcoarse.W,
         dfine.Cs, 1 if accumulate else 0, dtype_code(dfine.t.dtype), stream_ptr())


def upsample_slice(src, dst, c_off):
    call("mpn_upsample_nearest_slice", ptr(src.t), ptr(dst.t), src.B, src.H, src.W, src.Cs, dst.H, dst.W, dst.Cs, c_off,
         dtype_code(src.t.dtype), stream_ptr())


def upsample_slice_backward(ddst, dsrc, c_off):
    call("mpn_upsample_nearest_slice_backward", ptr(ddst.t), ptr(dsrc.t), dsrc.B, dsrc.H, dsrc.W, dsrc.Cs, ddst.H, ddst.W,
         ddst.Cs, c_off, dtype_code(dsrc.t.dtype), stream_ptr())


def export_f32(src, C, Ho, Wo):
    """Internal padded [B,h,w,Cs] -> exact f32 tensor of logical shape [B,C,Ho,Wo] (channels_last)."""
    out = torch.empty((src.B, Ho, Wo, C), dtype=torch.float32, device=src.t.device)
    call("mpn_export_f32", ptr(src.t), dtype_code(src.t.dtype), ptr(out), src.B, src.H, src.W, src.Cs, C, Ho, Wo,
         Ho * Wo * C, C, stream_ptr())
    return out.permute(0, 3, 1, 2)


def import_grad(g_nchw, like, dtype):
    """f32 gradient w.r.t. an exported tensor (logical [B,C,Ho,Wo], any strides w/ channel stride 1
    after permute) -> internal padded gradient Act shaped like ``like`` (sums nearest children)."""
    B, C, Ho, Wo = g_nchw.shape
    g = g_nchw.permute(0, 2, 3, 1)
    if g.stride(3) != 1 or g.stride(1) != Wo * g.stride(2):
        g = g.contiguous()
    d = Act(torch.empty((like.B, like.H, like.W, like.Cs), dtype=dtype, device=like.t.device), like.C)
    call("mpn_import_grad", ptr(g), g.stride(0), g.stride(2), ptr(d.t), dtype_code(dtype), like.B, like.H, like.W, like.Cs,
         like.C, Ho, Wo, stream_ptr())
    return d


def relu_forward(x, needs_grad=False):
    y = Act(torch.empty_like(x.t), x.C, needs_grad)
    call("mpn_relu_forward", ptr(x.t), ptr(y.t), x.t.numel(), dtype_code(x.t.dtype), stream_ptr())
    return y


def relu_backward(dz, z, dx=None, accumulate=False):
    if dx is None:
        dx = Act(torch.empty_like(z.t), z.C)
        accumulate = False
    call("mpn_relu_backward", ptr(dz.t), ptr(z.t), ptr(dx.t), z.t.numel(), 1 if accumulate else 0, dtype_code(z.t.dtype), stream_ptr())
    return dx


def copy_act(dst, src):
    """dst <- src for two activations of identical storage geometry."""
    call("mpn_copy_bytes", ptr(dst.t), ptr(src.t), src.t.numel() * src.t.element_size(), stream_ptr())


def add_inplace(dst, src):
    call("mpn_add_inplace", ptr(dst.t), ptr(src.t), dst.t.numel(), dtype_code(dst.t.dtype), stream_ptr())


def nchw_to_nhwc_f32(t):
    """Arbitrary-strided f32 [B,C,H,W] -> dense [B,H,W,C] f32."""
    B, C, H, W = t.shape
    out = torch.empty((B, H, W, C), dtype=torch.float32, device=t.device)
    call("mpn_nchw_to_nhwc_f32", ptr(t), t.stride(0), t.stride(1), t.stride(2), t.stride(3), ptr(out), B, C, H, W, stream_ptr())
    return out


def nms(dets, thresh, mode=0):
    """dets: f32 [N,5] device tensor.  Returns int64 device tensor of kept ORIGINAL indices (one D2H of the count)."""
    n = dets.shape[0]
    dev = dets.device
    if n == 0:
        return torch.empty((0,), dtype=torch.int64, device=dev)
    dets = dets.contiguous()
    keep = torch.empty((n,), dtype=torch.int64, device=dev)
    num = torch.empty((1,), dtype=torch.int64, device=dev)
    ws = workspace(call("mpn_nms_workspace_bytes", n), dev, slot=4)
    call("mpn_nms", ptr(dets), n, float(thresh), mode, ptr(keep), ptr(num), ptr(ws), stream_ptr())
    k = int(num.item())
    return keep[:k]


def box_decode_clip(anchors, deltas, img_w, img_h, clip=True, mean_std=None):
    """mean_std: None = the reference defaults (mean 0, std .1 .1 .2 .2), or the eight floats (mean[0..3], std[0..3]) of
    BBoxTransform(mean, std) (network/utils.py:8-17)."""
    B, A, _ = deltas.shape
    boxes = torch.empty((B, A, 4), dtype=torch.float32, device=deltas.device)
    w, h = (float(img_w), float(img_h)) if clip else (-1.0, -1.0)
    if mean_std is None:
        call("mpn_box_decode_clip", ptr(anchors), ptr(deltas), ptr(boxes), B, A, w, h, stream_ptr())
    else:
        ms = (ctypes.c_float * 8)(*[float(v) for v in mean_std])
        call("mpn_box_decode_clip_ms", ptr(anchors), ptr(deltas), ptr(boxes), B, A, w, h, ms, stream_ptr())
    return boxes


def clip_boxes_(boxes, img_w, img_h):
    if not boxes.is_contiguous():
        raise _lib.MpnError("clip_boxes_ needs a contiguous [B,A,4] tensor")
    call("mpn_clip_boxes", ptr(boxes), boxes.numel() // 4, float(img_w), float(img_h), stream_ptr())
    return boxes


def gather_dets(dets, keep):
    k = keep.numel()
    boxes = torch.empty((k, 4), dtype=torch.float32, device=dets.device)
    scores = torch.empty((k,), dtype=torch.float32, device=dets.device)
    if k > 0:
        call("mpn_gather_dets", ptr(dets), ptr(keep), k, ptr(boxes), ptr(scores), stream_ptr())
    return boxes, scores


_NMS_WARNED = []


def nms_pre_topn_env():
    """MPN_NMS_PRE_TOPN, read at CALL time: cap of candidates per image entering NMS when the caller passes none.  Unset / 0 = no cap —
    the reference's behaviour (posenet.py:269-285 hands every candidate above the score threshold to nms); there is NO default cap."""
    try:
        return max(0, int(os.environ.get("MPN_NMS_PRE_TOPN", "0")))
    except ValueError:
        return 0


def class_max(cls):
    """cls [B,A,K] f32 contiguous -> (score [B,A] f32, cls_id [B,A] int64): the maximum over the classes and the index of its first
    occurrence (torch.max(dim=2); posenet.py:267,283)."""
    B, A, K = cls.shape
    score = torch.empty((B, A), dtype=torch.float32, device=cls.device)
    cls_id = torch.empty((B, A), dtype=torch.int64, device=cls.device)
    call("mpn_class_max", ptr(cls), B, A, K, ptr(score), ptr(cls_id), stream_ptr())
    return score, cls_id


def gather_class(cls_id0, src, keep):
    """Class ids [k] int64 of the detections keep[k] selected from the candidates of score_filter(..., src) of one image."""
    k = keep.numel()
    out = torch.empty((k,), dtype=torch.int64, device=cls_id0.device)
    if k > 0:
        call("mpn_gather_class", ptr(cls_id0), ptr(src), cls_id0.numel(), ptr(keep), 0, None, 1, k, ptr(out), k, stream_ptr())
    return out


def _pre_nms_top_n(pre_nms_top_n, ncand):
    """Cap of candidates per image entering NMS: the caller's pre_nms_top_n, else MPN_NMS_PRE_TOPN (nms_pre_topn_env), else 0 = none.
    ncand: the most candidates of one image; above 32 768 of them and with no cap, warns once per process."""
    if pre_nms_top_n is None and nms_pre_topn_env() > 0:
        pre_nms_top_n = nms_pre_topn_env()
    top = int(pre_nms_top_n) if pre_nms_top_n else 0
    if top == 0 and ncand > 32768 and not _NMS_WARNED:
        # the reference's behaviour (every candidate above the score threshold enters the suppression) costs the upper triangle of an
        # N x N / 64 mask per image: 67 MB at 32 768 candidates, 0.6 GB at 100 000 — say so once instead of silently taking seconds
        import warnings
        _NMS_WARNED.append(True)
        warnings.warn("NMS over %d candidates in one image (upper-triangle N x N / 128 mask = %.0f MB per image); pass pre_nms_top_n or set "
                      "MPN_NMS_PRE_TOPN to bound it (not in the reference)" % (ncand, ncand * float(ncand) / 128 * 8 / 1e6))
    return top


def _no_detections(B, dev, padded, with_cls):
    """What detect_batched / detect_batched_classwise return when no image of the batch has a candidate."""
    if not padded:
        return [(None, None, None) if with_cls else (None, None)] * B
    out = (torch.zeros((B, 0, 4), dtype=torch.float32, device=dev), torch.zeros((B, 0), dtype=torch.float32, device=dev), [0] * B)
    return out + (torch.zeros((B, 0), dtype=torch.int64, device=dev),) if with_cls else out


def _suppress_and_gather(dets, dets_stride, counts, cnt, ncand, cand_cls, cls_stride, top, iou_thresh, mode, ws_limit, padded, gather_cls):
    """The tail of detect_batched / detect_batched_classwise: per-image NMS over the candidate rows dets (dets_stride floats between
    images, counts [B] int32 on the device = cnt on the host, ncand = max(cnt) > 0), class-wise when cand_cls (int32, cls_stride between
    images) is given; then the gathers and host round trip 2, and the results in the shape the two functions document.
    gather_cls: None, or a callable (keep, num, nmax, out) that enqueues the class gather into out [B,nmax] int64."""
    B, dev = len(cnt), dets.device
    nmax = min(ncand, top) if top > 0 else ncand       # rows of the sort / mask scratch and of the outputs
    keep = torch.empty((B, nmax), dtype=torch.int64, device=dev)
    num = torch.empty((B,), dtype=torch.int64, device=dev)
    per_img = call("mpn_nms_batched_classes_workspace_bytes" if cand_cls is not None else "mpn_nms_batched_workspace_bytes", 1, nmax)
    group = max(1, min(B, int(ws_limit // per_img)))   # bound the N x N/64 mask scratch; groups of images per launch set
    for b0 in range(0, B, group):
        nb = min(group, B - b0)
        ws = workspace(per_img * nb, dev, slot=4)
        rows = (ctypes.c_void_p(dets.data_ptr() + b0 * dets_stride * 4), dets_stride)
        head = (ctypes.c_void_p(counts.data_ptr() + b0 * 4), nb, ncand)
        tail = (float(iou_thresh), mode, ctypes.c_void_p(keep.data_ptr() + b0 * nmax * 8), nmax, ctypes.c_void_p(num.data_ptr() + b0 * 8),
                ptr(ws), stream_ptr())
        if cand_cls is not None:
            call("mpn_nms_batched_classes", *(rows + (ctypes.c_void_p(cand_cls.data_ptr() + b0 * cls_stride * 4), cls_stride) + head + (top,) + tail))
        elif top > 0:
            call("mpn_nms_batched_topk", *(rows + head + (top,) + tail))
        else:
            call("mpn_nms_batched", *(rows + head + tail))
    outs = (torch.empty((B, nmax, 4), dtype=torch.float32, device=dev), torch.empty((B, nmax), dtype=torch.float32, device=dev))
    call("mpn_gather_dets_batched", ptr(dets), dets_stride, ptr(keep), nmax, ptr(num), B, nmax, ptr(outs[0]), ptr(outs[1]), nmax, stream_ptr())
    if gather_cls is not None:
        outs += (torch.empty((B, nmax), dtype=torch.int64, device=dev),)
        gather_cls(keep, num, nmax, outs[2])
    kept = num.tolist()                                # host round trip 2
    if padded:
        return outs[:2] + ([k if cnt[b] > 0 else 0 for b, k in enumerate(kept)],) + outs[2:]
    return [tuple(o[b, :k] for o in outs) if cnt[b] > 0 else (None,) * len(outs) for b, k in enumerate(kept)]


def detect_batched(boxes, scores, score_thresh, iou_thresh, mode=0, ws_limit=4 << 30, padded=False, pre_nms_top_n=None, cls_id=None):
    """Score filter + per-image NMS + gather for EVERY image of a batch with two host round trips per batch (the candidate
    counts size the NMS launches, the kept counts size the returned tensors) instead of two per image.
    boxes [B,A,4], scores [B,A] (f32, contiguous).  Returns per image (boxes[k,4], scores[k]) device tensors (views); with
    padded=True the batch-wide tensors themselves: (boxes [B,nmax,4], scores [B,nmax] in descending order, kept counts list).
    pre_nms_top_n (not in the reference; None = every candidate, as posenet.py:269-285): only that many best-scored candidates of
    an image enter the suppression, which bounds its N x N/64 mask.
    cls_id (optional, [B,A] int64, from class_max): the class id of every kept detection travels along (its anchor index passes the
    score filter): each result gains it as a last item, (boxes, scores, classes [k] int64) / (..., kept, classes [B,nmax] int64)."""
    B, A = scores.shape[0], scores.shape[1]
    dev = scores.device
    dets = torch.empty((B, A, 5), dtype=torch.float32, device=dev)
    counts = torch.empty((B,), dtype=torch.int32, device=dev)
    src = torch.empty((B, A), dtype=torch.int32, device=dev) if cls_id is not None else None
    call("mpn_score_filter_batched", ptr(boxes), ptr(scores), B, A, float(score_thresh), ptr(dets), ptr(src) if src is not None else None,
         ptr(counts), stream_ptr())
    cnt = counts.tolist()                              # host round trip 1
    ncand = max(cnt)
    if ncand == 0:
        return _no_detections(B, dev, padded, cls_id is not None)
    gather_cls = None
    if cls_id is not None:
        def gather_cls(keep, num, nmax, out):
            call("mpn_gather_class", ptr(cls_id), ptr(src), A, ptr(keep), nmax, ptr(num), B, nmax, ptr(out), nmax, stream_ptr())
    return _suppress_and_gather(dets, A * 5, counts, cnt, ncand, None, 0, _pre_nms_top_n(pre_nms_top_n, ncand), iou_thresh, mode, ws_limit,
                                padded, gather_cls)


def detect_batched_classwise(boxes, cls, score_thresh, iou_thresh, mode=0, ws_limit=4 << 30, padded=False, pre_nms_top_n=None):
    """Class-wise post-processing of a K-class head (NOT the reference's, which thresholds the maximum over the classes and suppresses
    across them, posenet.py:267-281): every (anchor, class) score of cls [B,A,K] above score_thresh is a candidate, the suppression runs
    among candidates of the same class only, and the kept rows come out in descending score across classes (ties: lower a*K + c first)
    — include/mpn.h, "Class-wise candidates and NMS".  boxes [B,A,4], cls [B,A,K] (f32, contiguous).
    Returns what detect_batched(..., cls_id=...) returns: per image (boxes[k,4], scores[k], classes[k] int64) device tensors (views), or
    with padded=True (boxes [B,nmax,4], scores [B,nmax], kept counts list, classes [B,nmax] int64).  Two host reads per batch: the
    candidate counts after the count pass, the kept counts at the end.  pre_nms_top_n / MPN_NMS_PRE_TOPN, the warning above 32 768
    candidates and ws_limit are detect_batched's; the cap counts the candidates of an image, not of a class.  With K == 1 every result
    equals detect_batched's byte for byte."""
    B, A, K = cls.shape
    dev = cls.device
    if not (boxes.is_contiguous() and cls.is_contiguous()):
        raise _lib.MpnError("detect_batched_classwise needs contiguous boxes [B,A,4] and cls [B,A,K]")
    chunk_bytes = call("mpn_class_filter_workspace_bytes", B, A, K)
    if chunk_bytes < 0:
        raise _lib.MpnError("detect_batched_classwise: B=%d A=%d K=%d is out of range (A*K must stay below 2^31)" % (B, A, K))
    chunk_cnt = torch.empty((chunk_bytes // 4,), dtype=torch.int32, device=dev)
    counts = torch.empty((B,), dtype=torch.int32, device=dev)
    call("mpn_class_filter_count", ptr(cls), B, A, K, float(score_thresh), ptr(chunk_cnt), ptr(counts), stream_ptr())
    cnt = counts.tolist()                              # host round trip 1
    ncand = max(cnt)
    if ncand == 0:
        return _no_detections(B, dev, padded, True)
    dets = torch.empty((B, ncand, 5), dtype=torch.float32, device=dev)
    cand_cls = torch.empty((B, ncand), dtype=torch.int32, device=dev)
    cand_anchor = torch.empty((B, ncand), dtype=torch.int32, device=dev)
    call("mpn_class_filter_fill", ptr(boxes), ptr(cls), B, A, K, float(score_thresh), ptr(chunk_cnt), ncand, ptr(dets), ncand * 5, ptr(cand_cls),
         ptr(cand_anchor), ncand, ptr(counts), stream_ptr())

    def gather_cls(keep, num, nmax, out):
        call("mpn_gather_cand_class", ptr(cand_cls), None, ncand, ptr(keep), nmax, ptr(num), B, nmax, ptr(out), None, nmax, stream_ptr())
    return _suppress_and_gather(dets, ncand * 5, counts, cnt, ncand, cand_cls, ncand, _pre_nms_top_n(pre_nms_top_n, ncand), iou_thresh, mode,
                                ws_limit, padded, gather_cls)


def score_filter(boxes0, scores0, thresh):
    """Image-0 candidates with score > thresh: returns (dets[n,5], src_idx[n]) (one D2H of n)."""
    A = scores0.numel()
    dev = scores0.device
    dets = torch.empty((A, 5), dtype=torch.float32, device=dev)
    src = torch.empty((A,), dtype=torch.int32, device=dev)
    cnt = torch.empty((1,), dtype=torch.int32, device=dev)
    call("mpn_score_filter", ptr(boxes0), ptr(scores0), A, float(thresh), ptr(dets), ptr(src), ptr(cnt), stream_ptr())
    n = int(cnt.item())
    return dets[:n], src[:n]


# ---------------------------------------------------------------- keypoint and box AP / AR (csrc/coco_eval.hip; evaluate/oks_eval.py and
# evaluate/box_eval.py pack the arrays)
def _stage1_outputs(tab_host, tab, ranked):
    """Buffers of a stage 1 over the rows of tab_host: kept_src i32, kept_score, kept_area (, kept_rank i32 if ranked) [K] and the
    similarity blocks [sum kept x G], none of them empty, and their views of the true lengths."""
    check_device(tab)
    K, n_sim = int(tab_host[-1, 2]), int(tab_host[-1, 3])
    kinds = [(K, torch.int32), (K, torch.float64), (K, torch.float64)] + [(K, torch.int32)] * ranked + [(n_sim, torch.float64)]
    bufs = [torch.empty((max(n, 1),), dtype=dt, device=tab.device) for n, dt in kinds]
    return bufs, tuple(b[:n] for b, (n, _) in zip(bufs, kinds))


def _or_spare(dev):
    """p(t): the address of t, or of a spare allocation if t is empty and has none to hand over."""
    one = torch.empty((2,), dtype=torch.float64, device=dev)
    return lambda t: ptr(t) if t.numel() else ptr(one)


def _stage3_buffers(out, K, ws_bytes):
    """(order buffer i32 [max(K, 1)], workspace, p as _or_spare) of an accumulate into ``out``."""
    check_device(out)
    return torch.empty((max(K, 1),), dtype=torch.int32, device=out.device), workspace(ws_bytes, out.device, slot=9), _or_spare(out.device)


def oks_matrix(det_kp, det_score, gt_kp, gt_area, gt_bbox, tab_host, tab, max_dets, var):
    """Stage 1: (kept_src i32 [K], kept_score [K], kept_area [K], oks [sum kept x G]).  tab_host: contiguous int64 numpy
    [n_img + 1, 4]; tab: the same table on the device."""
    bufs, res = _stage1_outputs(tab_host, tab, ranked=False)
    call("mpn_oks_matrix", ptr(det_kp), ptr(det_score), ptr(gt_kp), ptr(gt_area), ptr(gt_bbox), ctypes.c_void_p(tab_host.ctypes.data),
         ptr(tab), tab_host.shape[0] - 1, int(max_dets), ptr(var), *[ptr(b) for b in bufs], stream_ptr())
    return res


def box_iou_matrix(det_box, det_score, gt_box, gt_flags, tab_host, tab, max_dets):
    """Stage 1: (kept_src i32 [K], kept_score [K], kept_area [K], kept_rank i32 [K], iou [sum kept x G]).  tab_host: contiguous int64
    numpy [n_row + 1, 4], one row per (category, image) pair; tab: the same table on the device.  The matching of stage 2 is
    ``oks_match`` on these IoU blocks."""
    bufs, res = _stage1_outputs(tab_host, tab, ranked=True)
    call("mpn_box_iou_matrix", ptr(det_box), ptr(det_score), ptr(gt_box), ptr(gt_flags), ctypes.c_void_p(tab_host.ctypes.data), ptr(tab),
         tab_host.shape[0] - 1, int(max_dets), *[ptr(b) for b in bufs], stream_ptr())
    return res


def oks_match(oks, kept_area, gt_area, gt_flags, tab_host, tab, max_dets, area_rng, iou_thrs):
    """Stage 2, on OKS or IoU blocks: (det_match [A, T, K], det_ig [A, T, K], gt_ig [A, G], gt_match [A, T, G]), int32."""
    check_device(tab)
    dev = tab.device
    n_img = tab_host.shape[0] - 1
    G, K = int(tab_host[-1, 1]), int(tab_host[-1, 2])
    A, T = area_rng.shape[0], iou_thrs.numel()
    det_match = torch.empty((A, T, K), dtype=torch.int32, device=dev)
    det_ig = torch.empty((A, T, K), dtype=torch.int32, device=dev)
    gt_ig = torch.empty((A, G), dtype=torch.int32, device=dev)
    gt_match = torch.empty((A, T, G), dtype=torch.int32, device=dev)
    p = _or_spare(dev)
    call("mpn_oks_match", p(oks), p(kept_area), ptr(gt_area), ptr(gt_flags), ctypes.c_void_p(tab_host.ctypes.data), ptr(tab), n_img,
         int(max_dets), ptr(area_rng), A, ptr(iou_thrs), T, p(det_match), p(det_ig), p(gt_ig), p(gt_match), stream_ptr())
    return det_match, det_ig, gt_ig, gt_match


def oks_accumulate(kept_score, det_match, det_ig, gt_ig, rec_thrs, out):
    """Stage 3: fills out = float64 [T*R*A + T*A] (precision [T, R, A] then recall [T, A]) and returns the order [K] of the stable
    descending-score sort over all images."""
    A, T, K = det_match.shape
    G, R = gt_ig.shape[1], rec_thrs.numel()
    order, ws, p = _stage3_buffers(out, K, call("mpn_oks_eval_workspace_bytes", K, A, T))
    call("mpn_oks_accumulate", p(kept_score), p(det_match), p(det_ig), p(gt_ig), K, G, A, T, ptr(rec_thrs), R, ptr(order), ptr(out),
         ctypes.c_void_p(out.data_ptr() + 8 * T * R * A), ptr(ws), stream_ptr())
    return order[:K]


def box_accumulate(kept_score, kept_rank, det_match, det_ig, gt_ig, cat_tab_host, cat_tab, max_dets_host, rec_thrs, out):
    """Stage 3: fills out = float64 [T*R*C*A*M + T*C*A*M] (precision [T, R, C, A, M] then recall [T, C, A, M]) and returns the order
    [K] of every category's stable descending-score sort.  cat_tab_host: contiguous int64 numpy [C + 1, 2]; max_dets_host:
    contiguous int32 numpy [M]."""
    A, T, K = det_match.shape
    G, R = gt_ig.shape[1], rec_thrs.numel()
    C, M = cat_tab_host.shape[0] - 1, max_dets_host.shape[0]
    order, ws, p = _stage3_buffers(out, K, call("mpn_box_eval_workspace_bytes", K, A, M, T))
    call("mpn_box_accumulate", p(kept_score), p(kept_rank), p(det_match), p(det_ig), p(gt_ig), ctypes.c_void_p(cat_tab_host.ctypes.data),
         ptr(cat_tab), C, K, G, A, T, ctypes.c_void_p(max_dets_host.ctypes.data), M, ptr(rec_thrs), R, ptr(order), ptr(out),
         ctypes.c_void_p(out.data_ptr() + 8 * T * R * C * A * M), ptr(ws), stream_ptr())
    return order[:K]
