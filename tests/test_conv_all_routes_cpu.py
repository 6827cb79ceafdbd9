"""CPU tier of tests/test_conv_all_routes_gpu.py: its routes pinned on the host, the census of the built library, and teeth.

Route pins: for every case of the GPU file the parameter block is built as the ops.py wrappers fill it (the builders of
tests/test_kernel_names_cpu.py) and mpn_conv_kernel_name / mpn_conv_wgrad_kernel_name must return the route the case names; for the
weight gradients mpn_conv_wgrad_chunks must also give the slice count and the last slice's length the case asserts.  Every shape is
proven here before a GPU is touched.

Census: the conv_igemm / conv_wgrad kernels of the built production library (tools/codeobj.py reads them from the code objects) are
parsed into their route spelling and each must be named by a case of the four GPU files — 138 of 138, minus EXCLUDED.  A conv kernel
name the parser does not recognise fails: a new family cannot slip by.

Teeth: the one new reference (_generic_ref / _check_generic of the register-staged weight gradient) is fed fp32 blocked models of the
kernel's loop.  It accepts the exact result and blocked sums in other step and slice orders, and rejects a dropped tap, two cin tiles
stored in each other's place, the last four cin lanes of the ragged tile left unwritten, one missing k-step and a slice partial
missing."""
import ctypes
import os
import re
import sys

import pytest
import torch
import torch.nn.functional as F

import test_conv_all_routes_gpu as ar
import test_conv_small_tiles_gpu as st
import test_conv_tiles_gpu as ct
import test_kernel_names_cpu as kn
import test_wgrad_parity_gpu as wt
from helpers import ROOT, report, round_up

F32 = torch.float32
CASES = {c[0]: c for c in ar.CASES}


@pytest.fixture(scope="module", autouse=True)
def _threads():
    from multiposenet.pytorch_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    n = torch.get_num_threads()
    torch.set_num_threads(min(n, 16))
    yield
    torch.set_num_threads(n)


# ----------------------------------------------------------------------------------------------------------------- route pins
def _spread_block(f):
    """ops.conv_wgrad through x_geom as _generic_case calls it: the dense block with the batch stride of _spread_act."""
    p = kn.wgrad_block(**f)
    es = 4 if f["dtype"] == F32 else 2
    p.x_sB = round_up(((1 << 31) + f["B"] * es - 1) // (f["B"] * es), 32)
    return p


BUILD = {st._conv_case: (kn.conv_block, "mpn_conv_kernel_name"), ct._kseg_case: (kn.kseg_block, "mpn_conv_kernel_name"),
         st._pyramid_case: (kn.pyramid_block, "mpn_conv_kernel_name"), wt._conv_case: (kn.wgrad_block, "mpn_conv_wgrad_kernel_name"),
         wt._seg_case: (kn.wseg_block, "mpn_conv_wgrad_kernel_name")}


def _block(runner, f):
    if runner is ar._generic_case:
        return _spread_block(f), "mpn_conv_wgrad_kernel_name"
    build, query = BUILD[runner]
    return build(**f), query


@pytest.mark.parametrize("case", ar.CASES, ids=[c[0].replace(" ", "_") for c in ar.CASES])
def test_all_routes_case_route(case):
    from multiposenet.pytorch_amd import _lib
    cid, route, runner, f = case
    p, query = _block(runner, f)
    assert kn._name(query, p) == route, cid
    if query == "mpn_conv_kernel_name":
        assert route.endswith("true>") == ct._needs_ext(f), cid
        return
    if runner is wt._seg_case and "slices" in f:
        c = _lib.lib().mpn_conv_wgrad_seg_plan(ctypes.byref(p))
        assert f["slices"][0] <= c <= f["slices"][1] and c == p.chunks, (cid, c)
    if "chunks" in f:           # the slice plan the case asserts on the device
        p.chunks = 1
        chunks = _lib.lib().mpn_conv_wgrad_chunks(ctypes.byref(p))
        assert chunks == f["chunks"], (cid, chunks)
        if "last_slice" in f:
            P = p.B * p.Ho * p.Wo
            kp = 16 if f["dtype"] == F32 else 32
            cp = P if chunks == 1 else round_up((P + chunks - 1) // chunks, kp)
            assert P - (chunks - 1) * cp == f["last_slice"], (cid, P, cp)


def test_generic_cases_need_the_spread_batch_stride():
    """The same blocks over a dense x take an LDS-DMA kernel: only the operand's extent sends a launch the C ABI accepts to the generic
    kernel.  And the extent is exactly the descriptor limit, held in an allocation half that size."""
    for cid, route, runner, f in ar.WGRAD_GENERIC:
        dense = kn._name("mpn_conv_wgrad_kernel_name", kn.wgrad_block(**f))
        assert dense.startswith("conv_wgrad_dma"), (cid, dense)
        p = _spread_block(f)
        es = 4 if f["dtype"] == F32 else 2
        assert f["Cin"] % 8 == 0 and p.B * p.x_sB * es >= (1 << 31) - 1 and (p.B - 1) * p.x_sB * es <= (1 << 30) + 4096, cid


# ----------------------------------------------------------------------------------------------------------------- census
TYPE = {"t": "bf16", "DF16_": "_Float16", "f": "float"}
_T = r"(t|DF16_|f)"
_B = {"0": "false", "1": "true"}
# Routes left without a parity case, each with its reason (a launch that faulted or hung and whose cause is not found).  Empty.
EXCLUDED = {}


def _codeobj():
    tools = os.path.join(ROOT, "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import codeobj
    return codeobj


def parse_conv_kernel(mangled):
    """Mangled name of a conv_igemm / conv_wgrad instantiation -> the route spelling of the GPU files' CASES (the profiling flag of the
    igemm kernels dropped: a production library holds PROF = false only).  ValueError for anything else."""
    m = re.match(r"^_ZN12_GLOBAL__N_1(\d+)", mangled)
    if not m:
        raise ValueError(mangled)
    n = int(m.group(1))
    base, rest = mangled[m.end(): m.end() + n], mangled[m.end() + n:]
    if base in ("conv_igemm_kernel", "conv_igemm_s3_kernel"):
        a = re.match(r"^I%sLi(\d+)ELi(\d+)ELb([01])ELb([01])ELb([01])ELb0EEEv13MpnConvParamsi$" % _T, rest)
        if a:
            return "%s<%s, %s, %s, %s, %s, %s>" % (base, TYPE[a.group(1)], a.group(2), a.group(3), _B[a.group(4)], _B[a.group(5)], _B[a.group(6)])
    elif base == "conv_wgrad_kernel":
        a = re.match(r"^I%sLi(\d+)ELi(\d+)EEEv14MpnWgradParamsl$" % _T, rest)
        if a:
            return "%s<%s, %s, %s>" % (base, TYPE[a.group(1)], a.group(2), a.group(3))
    elif re.match(r"^conv_wgrad_dma(_lin|_seg)?(_f16|_f32)?_kernel$", base):
        a = re.match(r"^ILi(\d+)ELi(\d+)EEEv14MpnWgradParamsl$", rest)
        if a:
            return "%s<%s, %s>" % (base, a.group(1), a.group(2))
    raise ValueError(mangled)


def test_parser_spells_routes_as_the_cases_do_and_refuses_the_rest():
    mangled = _codeobj().mangled
    assert parse_conv_kernel("_ZN12_GLOBAL__N_1" + mangled("conv_igemm_s3_kernel", "t", 256, 128, True, False, False, False)
                             + "Ev13MpnConvParamsi") == ct._inst(ct.BF, 256, s3=True, out_f32=True)
    assert parse_conv_kernel("_ZN12_GLOBAL__N_1" + mangled("conv_igemm_kernel", "DF16_", 32, 128, False, True, True, False)
                             + "Ev13MpnConvParamsi") == ct._inst(ct.H16, 32, ext=True)
    assert parse_conv_kernel("_ZN12_GLOBAL__N_1" + mangled("conv_wgrad_dma_lin_f16_kernel", 64, 128) + "Ev14MpnWgradParamsl") == wt._lin(ct.H16, 64, 128)
    assert parse_conv_kernel("_ZN12_GLOBAL__N_1" + mangled("conv_wgrad_kernel", "f", 32, 128) + "Ev14MpnWgradParamsl") == "conv_wgrad_kernel<float, 32, 128>"
    for bad in ("_ZN12_GLOBAL__N_1" + mangled("conv_igemm_kernel", "t", 128, 128, False, False, False, True) + "Ev13MpnConvParamsi",      # PROF
                "_ZN12_GLOBAL__N_1" + mangled("conv_igemm_s4_kernel", "t", 128, 128, False, False, False, False) + "Ev13MpnConvParamsi",  # a new family
                "_ZN12_GLOBAL__N_1" + mangled("conv_wgrad_dma_prof_kernel", 128, 128) + "Ev14MpnWgradParamslPy",
                "_ZN12_GLOBAL__N_1" + mangled("conv_wgrad_kernel", "d", 32, 128) + "Ev14MpnWgradParamsl"):
        with pytest.raises(ValueError):
            parse_conv_kernel(bad)


def test_census_every_compiled_conv_kernel_has_a_parity_case():
    from multiposenet.pytorch_amd import _lib
    codeobj = _codeobj()
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    names = [k["name"] for k in codeobj.kernels(_lib.LIB_PATH)]
    conv = sorted(n for n in names if "conv_igemm" in n or "conv_wgrad" in n)
    routes = [parse_conv_kernel(n) for n in conv]           # an unknown family raises here
    assert len(routes) == len(set(routes)) == 138, len(routes)
    files = (("tests/test_conv_tiles_gpu.py", ct.CASES), ("tests/test_conv_small_tiles_gpu.py", st.CASES), ("tests/test_wgrad_parity_gpu.py", wt.CASES),
             ("tests/test_conv_all_routes_gpu.py", ar.CASES))
    cover = {}
    for fname, cases in files:
        for c in cases:
            cover.setdefault(c[1], fname)
    assert not (set(EXCLUDED) & set(cover)) and set(EXCLUDED) <= set(routes), EXCLUDED
    missing = [r for r in routes if r not in cover and r not in EXCLUDED]
    for r in routes:
        report("census %-64s %s" % (r, cover.get(r) or ("EXCLUDED: " + EXCLUDED[r] if r in EXCLUDED else "NO PARITY CASE")))
    report("census: %d of %d compiled conv kernels have a float64 element-wise case (%d before tests/test_conv_all_routes_gpu.py)" % (
        len(routes) - len(missing) - len(EXCLUDED), len(routes), sum(1 for r in routes if cover.get(r) not in (None, files[3][0]))))
    assert not missing, "compiled conv kernels without a parity case: %s" % missing
    # and no case names a kernel the library does not hold (the one non-kernel entry: the f32 pyramid's per-level fallback)
    ghosts = sorted(r for r in cover if r not in routes and r != "per-level fallback")
    assert not ghosts, ghosts
    assert sum(1 for r in routes if cover[r] != files[3][0]) == 56 and sum(1 for r in routes if cover[r] == files[3][0]) == 82


# ----------------------------------------------------------------------------------------------------------------- teeth
def _model(R, chunks, step_order=1, slice_order=None, skip_step=None, skip_slice=None, drop_tap=None):
    """fp32 model of conv_wgrad_kernel: per slice one accumulator per element over k-steps of R.k_step pixels (each step's exact sum
    rounded to fp32), then dw0 += the slice partials in order.  Returns [Cout][R][S][Cin] float64."""
    B, C, H, W = R.x.shape
    O, taps = R.dy.shape[1], R.k * R.k
    cols = F.unfold(R.x, R.k, padding=R.pad, stride=R.stride).transpose(1, 2).reshape(R.P, C * taps)       # columns in (c, r, s) order
    dy = R.dy.permute(0, 2, 3, 1).reshape(R.P, O)
    cp = ar._slice_len(R, chunks)
    parts = []
    for si in range(chunks):
        s0, s1 = min(si * cp, R.P), min((si + 1) * cp, R.P)
        acc = torch.zeros(O, C * taps, dtype=F32)
        for j, p0 in enumerate(list(range(s0, s1, R.k_step))[::step_order]):
            if skip_step == (si, j):
                continue
            acc = acc + (dy[p0:min(p0 + R.k_step, s1)].t() @ cols[p0:min(p0 + R.k_step, s1)]).float()
        acc = acc.view(O, C, R.k, R.k).permute(0, 2, 3, 1).contiguous()
        if drop_tap is not None:
            acc[:, drop_tap[0], drop_tap[1]] = 0
        parts.append(acc)
    out = R.dw0.clone()
    for si in (range(chunks) if slice_order is None else slice_order):
        if si != skip_slice:
            out = out + parts[si]
    return out.double()


def _reject(cid, route, R, dw, chunks, what):
    with pytest.raises(AssertionError):
        ar._check_generic("cpu teeth REJECT %s: %s" % (what, cid), route, R, dw, chunks)


@pytest.mark.parametrize("cid", ["bf16 generic 3x3 200->200 B2 30x30", "f32 generic 3x3 valid 40->19 B2 20x22", "f16 generic 3x3 s2 72->36 B2 61x59 db"])
def test_generic_reference_accepts_blocked_sums_and_rejects_modelled_faults(cid):
    _, route, _, f = CASES[cid]
    R = ar._generic_ref(cid, f)
    chunks = f["chunks"]
    assert chunks > 1 and R.P - (chunks - 1) * ar._slice_len(R, chunks) == f["last_slice"]
    assert ar._check_generic("cpu teeth exact " + cid, route, R, (R.ref + R.dw0.double()).float(), chunks) <= 1.0
    assert ar._check_generic("cpu teeth blocked " + cid, route, R, _model(R, chunks), chunks) <= 1.0
    perm = torch.randperm(chunks, generator=torch.Generator().manual_seed(3)).tolist()
    assert ar._check_generic("cpu teeth blocked reversed, permuted slices " + cid, route, R, _model(R, chunks, step_order=-1, slice_order=perm), chunks) <= 1.0

    Cin = f["Cin"]
    _reject(cid, route, R, _model(R, chunks, skip_step=(1, 2)), chunks, "one k-step missing in slice 1")
    _reject(cid, route, R, _model(R, chunks, skip_step=(chunks - 1, 0)), chunks, "first k-step of the short last slice missing")
    _reject(cid, route, R, _model(R, chunks, skip_slice=chunks - 1), chunks, "last slice's partial missing")
    _reject(cid, route, R, _model(R, chunks, drop_tap=(R.k - 1, 0)), chunks, "tap (k - 1, 0) dropped")
    good = _model(R, chunks)
    bad = good.clone()                                       # the ragged tile's last four cin lanes (one lane's float4) never stored
    bad[..., Cin - 4:] = R.dw0.double()[..., Cin - 4:]
    _reject(cid, route, R, bad, chunks, "tail float4 of the ragged cin tile unwritten")
    bad = good.clone()                                       # two 16-channel cin blocks (the MFMA row blocks of a tile) in each other's place
    bad[..., 0:16], bad[..., 16:32] = good[..., 16:32], good[..., 0:16]
    _reject(cid, route, R, bad, chunks, "cin blocks swapped")
    bad = good.clone()                                       # ... and two output channels
    bad[0], bad[1] = good[1], good[0]
    _reject(cid, route, R, bad, chunks, "cout rows swapped")
    _reject(cid, route, R, good - R.dw0.double(), chunks, "dw overwritten")
