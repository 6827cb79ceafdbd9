"""Gradient clipping by the infinity norm (FusedAdam.clip_grad_norm_inf_, ReplayedTrainStep(max_grad_norm=...)): the C-ABI
entry points exist in the header, the library and the ctypes table, and refuse bad arguments before any HIP call (no GPU here).
The numerics are checked on the device in tests/test_grad_clip_gpu.py."""
import ctypes
import os
import re
import subprocess

from helpers import ROOT

NEW = ("mpn_grad_absmax_workspace_bytes", "mpn_grad_absmax_partial", "mpn_grad_clip_finalize", "mpn_adam_step_clip_dev",
       "mpn_scale_by_dev")


def _badarg():
    src = open(os.path.join(ROOT, "include", "mpn.h")).read()
    return int(re.search(r"#define\s+MPN_E_BADARG\s+\(?(-?\d+)\)?", src).group(1))


def test_clip_entry_points_agree_across_header_library_and_ctypes_table():
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
    # the existing optimizer entry points keep their signatures
    assert _lib.SIGNATURES["mpn_adam_step_dev"] == (ctypes.c_int, [ctypes.c_void_p] * 4 + [ctypes.c_int64] + [ctypes.c_void_p] * 2)
    assert "mpn_grad_absmax_workspace_bytes" in _lib._COUNT_FUNCS


def test_clip_entry_points_reject_bad_arguments_without_touching_the_gpu():
    from multiposenet.pytorch_amd import _lib
    L = _lib.lib()
    BAD = _badarg()
    nul = ctypes.c_void_p(None)
    a = ctypes.c_void_p(0x1000)          # 16-byte aligned, never dereferenced: validation fails first
    mis = ctypes.c_void_p(0x1004)        # 4-byte aligned only
    # workspace size: one partial per workgroup, at most 1024 per run
    assert L.mpn_grad_absmax_workspace_bytes(0) == BAD and L.mpn_grad_absmax_workspace_bytes(-5) == BAD
    assert L.mpn_grad_absmax_workspace_bytes(1) == 4
    assert L.mpn_grad_absmax_workspace_bytes(4096) == 4 and L.mpn_grad_absmax_workspace_bytes(4097) == 8
    assert L.mpn_grad_absmax_workspace_bytes(61 * 10 ** 6) == 4096
    # max-abs partials
    assert L.mpn_grad_absmax_partial(nul, 16, a, nul) == BAD
    assert L.mpn_grad_absmax_partial(a, 16, nul, nul) == BAD
    assert L.mpn_grad_absmax_partial(a, 0, a, nul) == BAD
    assert L.mpn_grad_absmax_partial(a, -1, a, nul) == BAD
    assert L.mpn_grad_absmax_partial(mis, 16, a, nul) == BAD
    # finalize
    assert L.mpn_grad_clip_finalize(nul, 4, a, a, a, nul) == BAD
    assert L.mpn_grad_clip_finalize(a, 4, nul, a, a, nul) == BAD
    assert L.mpn_grad_clip_finalize(a, 4, a, nul, a, nul) == BAD
    assert L.mpn_grad_clip_finalize(a, 4, a, a, nul, nul) == BAD
    assert L.mpn_grad_clip_finalize(a, 0, a, a, a, nul) == BAD
    assert L.mpn_grad_clip_finalize(a, -3, a, a, a, nul) == BAD
    assert L.mpn_grad_clip_finalize(a, 4, ctypes.c_void_p(0x1002), a, a, nul) == BAD
    # clipped Adam
    assert L.mpn_adam_step_clip_dev(a, a, a, a, 64, a, nul, nul) == BAD
    assert L.mpn_adam_step_clip_dev(a, a, a, a, 64, nul, a, nul) == BAD
    assert L.mpn_adam_step_clip_dev(nul, a, a, a, 64, a, a, nul) == BAD
    assert L.mpn_adam_step_clip_dev(a, nul, a, a, 64, a, a, nul) == BAD
    assert L.mpn_adam_step_clip_dev(a, a, a, a, 0, a, a, nul) == BAD
    assert L.mpn_adam_step_clip_dev(a, a, a, a, -64, a, a, nul) == BAD
    assert L.mpn_adam_step_clip_dev(a, mis, a, a, 64, a, a, nul) == BAD
    assert L.mpn_adam_step_clip_dev(a, a, a, mis, 64, a, a, nul) == BAD
    # in-place scale
    assert L.mpn_scale_by_dev(nul, 8, a, nul) == BAD
    assert L.mpn_scale_by_dev(a, 8, nul, nul) == BAD
    assert L.mpn_scale_by_dev(a, 0, a, nul) == BAD
    assert L.mpn_scale_by_dev(a, -8, a, nul) == BAD
    assert L.mpn_scale_by_dev(mis, 8, a, nul) == BAD


def test_stepper_records_clipping_steps_and_keeps_the_prn_on_the_eager_path():
    """Host logic of the Trainer's stepper: with FusedAdam and launch='replay' a finite max_grad_norm goes to the recorded step
    (before, it forced the eager tape); the recorded step refuses an unrecorded subnet instead of skipping its clip."""
    import math
    import pytest
    import torch
    from multiposenet.pytorch_amd.replay import ReplayedTrainStep
    from multiposenet.pytorch_amd.training import trainer

    class FusedAdam(torch.optim.SGD):          # the stepper chooses by type name; nothing here runs a kernel
        clip_grad_norm_inf_ = begin_bucketed = None

    model = torch.nn.Linear(2, 2)
    model._engine = None
    opt = FusedAdam(model.parameters(), lr=0.1)
    P = trainer.TrainParams(max_grad_norm=0.5, launch='replay')
    st = trainer._Stepper(model, opt, P)
    assert isinstance(st.fast, ReplayedTrainStep) and st.fast.max_grad_norm == 0.5 and st.clip == 0.5
    assert st.fast.bucketed_update is False
    with pytest.raises(ValueError):
        st.fast([[torch.zeros(1), 'prn_subnet']], ['prn_subnet', torch.zeros(1)])
    assert trainer._Stepper(model, opt, trainer.TrainParams(max_grad_norm=math.inf, launch='replay')).fast.max_grad_norm is None
    assert trainer._Stepper(model, opt, trainer.TrainParams(max_grad_norm=0.5, launch='eager')).fast is None
    with pytest.raises(TypeError):
        ReplayedTrainStep(model, torch.optim.SGD(model.parameters(), lr=0.1), max_grad_norm=1.0)
