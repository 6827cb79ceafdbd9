"""The recorded PRN training step, the parts that need no GPU: the new C-ABI entry points exist in the header, the library and the
ctypes table and refuse bad arguments before any HIP call; the host mirror of the device dropout seed word reproduces the eager
seed sequence; the float32 model of the one-launch loss head passes the check the GPU test applies to the kernel, and four modelled
faults do not.  The kernels themselves are checked on the device in tests/test_prn_replay_gpu.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import loss_ref as L
import prn_head_ref as H
from helpers import ROOT

NEW = ("mpn_dropout_dev", "mpn_dropout_advance", "mpn_prn_pack", "mpn_prn_head_train")
M64 = (1 << 64) - 1


def _badarg():
    src = open(os.path.join(ROOT, "include", "mpn.h")).read()
    return int(re.search(r"#define\s+MPN_E_BADARG\s+\(?(-?\d+)\)?", src).group(1))


def test_prn_step_entry_points_agree_across_header_library_and_ctypes_table():
    from multiposenet.pytorch_amd import _lib
    _lib.build()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mpn.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(mpn_[a-z0-9_]+)\s*\(", src))
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    exported = set(l.split()[-1] for l in out.splitlines() if " T mpn_" in l)
    for name in NEW:
        assert name in declared, name
        assert name in exported, name
        assert name in _lib.SIGNATURES, name
        assert name not in _lib._COUNT_FUNCS, name
    # the eager dropout keeps its host-seeded entry point
    assert _lib.SIGNATURES["mpn_dropout"][1][3] is ctypes.c_uint64


def test_prn_step_entry_points_reject_bad_arguments_without_touching_the_gpu():
    from multiposenet.pytorch_amd import _lib
    Lb = _lib.lib()
    BAD = _badarg()
    nul = ctypes.c_void_p(None)
    a = ctypes.c_void_p(0x1000)          # 16-byte aligned, never dereferenced: validation fails first
    m4 = ctypes.c_void_p(0x1004)         # 4-byte aligned only
    m2 = ctypes.c_void_p(0x1002)         # 2-byte aligned only
    m1 = ctypes.c_void_p(0x1001)
    F32, BF16 = _lib.F32, _lib.BF16
    # dropout seeded from device memory
    assert Lb.mpn_dropout_dev(nul, a, 8, a, 1, 0.5, F32, nul) == BAD
    assert Lb.mpn_dropout_dev(a, nul, 8, a, 1, 0.5, F32, nul) == BAD
    assert Lb.mpn_dropout_dev(a, a, 8, nul, 1, 0.5, F32, nul) == BAD
    assert Lb.mpn_dropout_dev(a, a, 0, a, 1, 0.5, F32, nul) == BAD
    assert Lb.mpn_dropout_dev(a, a, -8, a, 1, 0.5, F32, nul) == BAD
    assert Lb.mpn_dropout_dev(a, a, 8, a, 1, 1.0, F32, nul) == BAD          # p outside [0, 1)
    assert Lb.mpn_dropout_dev(a, a, 8, a, 1, -0.1, F32, nul) == BAD
    assert Lb.mpn_dropout_dev(a, a, 8, a, 1, float("nan"), F32, nul) == BAD
    assert Lb.mpn_dropout_dev(a, a, 8, a, 1, 0.5, 7, nul) == BAD            # unknown dtype
    assert Lb.mpn_dropout_dev(a, a, 8, m4, 1, 0.5, F32, nul) == BAD         # the state word is 8 bytes
    assert Lb.mpn_dropout_dev(m2, a, 8, a, 1, 0.5, F32, nul) == BAD
    assert Lb.mpn_dropout_dev(a, m1, 8, a, 1, 0.5, BF16, nul) == BAD
    assert Lb.mpn_dropout_advance(nul, 2, nul) == BAD
    assert Lb.mpn_dropout_advance(m4, 2, nul) == BAD
    # input packing
    assert Lb.mpn_prn_pack(nul, a, 3, 24, 32, BF16, nul) == BAD
    assert Lb.mpn_prn_pack(a, nul, 3, 24, 32, BF16, nul) == BAD
    assert Lb.mpn_prn_pack(a, a, 0, 24, 32, BF16, nul) == BAD
    assert Lb.mpn_prn_pack(a, a, 3, 0, 32, BF16, nul) == BAD
    assert Lb.mpn_prn_pack(a, a, 3, -24, 32, BF16, nul) == BAD
    assert Lb.mpn_prn_pack(a, a, 3, 24, 16, BF16, nul) == BAD               # npad < n
    assert Lb.mpn_prn_pack(a, a, 3, 24, 32, 9, nul) == BAD
    assert Lb.mpn_prn_pack(m2, a, 3, 24, 32, BF16, nul) == BAD
    assert Lb.mpn_prn_pack(a, m1, 3, 24, 32, BF16, nul) == BAD
    assert Lb.mpn_prn_pack(a, m2, 3, 24, 32, F32, nul) == BAD
    # loss head
    ok = [a, 32, a, a, nul, a, 3, 24, 32, BF16, a, a, nul]

    def head(**kw):
        args = list(ok)
        for k, v in kw.items():
            args[int(k[1:])] = v
        return Lb.mpn_prn_head_train(*args)
    for i in (0, 2, 3, 5, 10, 11):                                          # o, res, label, dl, partial, loss
        assert head(**{"i%d" % i: nul}) == BAD, i
    assert head(i6=0) == BAD and head(i6=-3) == BAD                         # rows
    assert head(i7=0) == BAD and head(i7=-24) == BAD                        # cols
    assert head(i8=16) == BAD                                               # npad < cols
    assert head(i1=16) == BAD                                               # row stride < cols
    assert head(i9=5) == BAD                                                # unknown dtype
    for i in (0, 2, 3, 4, 10, 11):
        assert head(**{"i%d" % i: m2}) == BAD, i                            # float operands are 4-byte aligned
    assert head(i5=m1) == BAD
    assert head(i5=m2, i9=F32) == BAD


# ------------------------------------------------------------------------------------------------ dropout seed word
class _SeedWorld(object):
    """The eager formula on one side (Engine.dropout: the j-th call ever is seeded initial_seed * 1000003 + j), a device word
    driven by engine.drop_state_step on the other."""

    def __init__(self, initial_seed, calls=0):
        self.seed, self.calls = initial_seed, calls
        self.word, self.mirror, self.uploads = 0xDEAD, None, 0          # the device word starts as garbage

    def eager(self, d=2):
        out = []
        for _ in range(d):
            self.calls += 1
            out.append((self.seed * 1000003 + self.calls) & M64)
        return out

    def recorded(self, d=2):
        from multiposenet.pytorch_amd.engine import drop_state_step
        upload, self.mirror = drop_state_step(self.mirror, self.seed, self.calls, d)
        if upload is not None:
            assert 0 <= upload <= M64
            self.word, self.uploads = upload, self.uploads + 1
        out = [(self.word + k) & M64 for k in range(1, d + 1)]          # mpn_dropout_dev, k = 1 .. d
        self.word = (self.word + d) & M64                               # mpn_dropout_advance
        self.calls += d
        assert self.mirror == self.word
        return out


def test_seed_word_mirror_reproduces_the_eager_seed_sequence():
    plan = ["r", "r", "r", "e", "r", "r", ("seed", 99), "r", "e", "e", "r", ("eval", 0), "r", "r"]
    a, b = _SeedWorld(1234567), _SeedWorld(1234567)
    uploads = []
    for op in plan:
        if isinstance(op, tuple) and op[0] == "seed":
            a.seed = b.seed = op[1]
        elif isinstance(op, tuple):                                     # a recorded step in eval mode: no dropout, no launch
            assert b.recorded(0) == a.eager(0) == []
        elif op == "e":
            assert a.eager() == b.eager()
        else:
            assert b.recorded() == a.eager(), op
        uploads.append(b.uploads)
    # uploaded at the first recorded step, after the eager forward, after manual_seed, after the two eager steps — never otherwise
    assert uploads == [1, 1, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4, 4]
    assert a.calls == b.calls


@pytest.mark.parametrize("gap", [0, 1, 2, 3])
def test_seed_word_mirror_wraps_at_2_to_the_64(gap):
    seed = 0x1234567
    calls = (M64 - gap - seed * 1000003) % (1 << 64)                    # the word before the step is 2^64 - 1 - gap
    a, b = _SeedWorld(seed, calls), _SeedWorld(seed, calls)
    for _ in range(3):
        got = b.recorded()
        assert got == a.eager() and all(0 <= s <= M64 for s in got)
    assert b.uploads == 1 and b.word == (M64 - gap + 6) & M64 and b.word < 8


def test_seed_word_upload_fits_the_signed_storage():
    """The engine keeps the word in an int64 tensor: values with the top bit set go up as their two's complement."""
    from multiposenet.pytorch_amd.engine import drop_state_step
    up, after = drop_state_step(None, (1 << 63) // 1000003 + 5, 0, 2)
    assert up >> 63 == 1 and after == (up + 2) & M64
    t = torch.tensor([up - (1 << 64)], dtype=torch.int64)
    assert int(t.view(torch.uint8).numpy().view(np.uint64)[0]) == up
    assert drop_state_step(up, (1 << 63) // 1000003 + 5, 0, 2) == (None, after)


# ------------------------------------------------------------------------------------------------ loss head model
def _bytes(dl, dtype):
    t = torch.from_numpy(np.ascontiguousarray(dl)).to(dtype).contiguous()
    return t.view(torch.uint8).numpy().reshape(dl.shape[0], -1)


_CASES = {}


def _case(name):
    if name not in _CASES:
        if name == "saturating 3x8568":
            c = H.saturating_case()
        else:
            c = L.softmax_case(257, True)
            c["y"] = H.softmax_label(c)
        npad = L.round_up(c["cols"], 32)
        chain_dl, p = H.chain_model(c["a"], c["res"], c["y"], c["cols"], npad)
        _CASES[name] = (c, npad, chain_dl, p)
    return _CASES[name]


@pytest.mark.parametrize("name", ["257 padded", "saturating 3x8568"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_head_model_passes_the_check(name, dtype):
    c, npad, chain_dl, p = _case(name)
    dl, loss = H.head_model(c["a"], c["res"], c["y"], c["cols"], npad)
    err, bound = H.check_head("model " + name, _bytes(dl, dtype), loss, _bytes(chain_dl, dtype), p, c["y"], c["cols"], npad)
    assert bound < 1e-5 * max(1.0, abs(float(loss)))                     # the bound is not vacuous
    if name.startswith("saturating"):
        # the case does what it is there for: clamped and saturated probabilities, exact-zero pre-activations, rare ones
        assert (p * (1 - p) < 1e-12).sum() > 100 and (p == 0).sum() > 1000 and (p == 1).sum() >= 1
        assert (c["a"][:, :c["cols"]] == 0).sum() > 1000 and 0.005 < c["y"].mean() < 0.02
        assert npad - c["cols"] == 8


@pytest.mark.parametrize("mut", ["ReLU mask dropped", "dot product of the neighbouring row", "1/N omitted", "non-zero pad lane"])
@pytest.mark.parametrize("name", ["257 padded", "saturating 3x8568"])
def test_head_check_rejects_modelled_faults(name, mut):
    c, npad, chain_dl, p = _case(name)
    dl, loss = H.head_model(c["a"], c["res"], c["y"], c["cols"], npad, mut=mut)
    for dtype in (torch.float32, torch.bfloat16):
        with pytest.raises(AssertionError):
            H.check_head("fault", _bytes(dl, dtype), loss, _bytes(chain_dl, dtype), p, c["y"], c["cols"], npad)


def test_head_loss_bound_rejects_a_loss_divided_by_the_row_count():
    c, npad, chain_dl, p = _case("257 padded")
    dl, loss = H.head_model(c["a"], c["res"], c["y"], c["cols"], npad)
    with pytest.raises(AssertionError):
        H.check_head("fault", _bytes(dl, torch.float32), loss * c["cols"], _bytes(chain_dl, torch.float32), p, c["y"], c["cols"], npad)
    with pytest.raises(AssertionError):
        H.check_head("fault", _bytes(dl, torch.float32), np.float32(loss) * np.float32(1 + 2e-5), _bytes(chain_dl, torch.float32), p,
                     c["y"], c["cols"], npad)
