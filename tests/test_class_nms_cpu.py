"""Class-wise candidates and NMS for K-class heads, the parts that need no GPU: the two numpy formulations of tests/class_nms_ref.py
agree on every case, each modelled fault is rejected by the reference alone, and the new C-ABI entry points exist in the header, the
library and the ctypes table and refuse bad arguments before any HIP call.  The kernels are checked in tests/test_class_nms_gpu.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import class_nms_ref as C
from helpers import ROOT, report

NEW = ("mpn_class_filter_chunk", "mpn_class_filter_workspace_bytes", "mpn_class_filter_count", "mpn_class_filter_fill",
       "mpn_nms_batched_classes_workspace_bytes", "mpn_nms_batched_classes", "mpn_gather_cand_class")
CAP = 150
MODEL_CHUNK = 256          # the model's chunk length on the CPU tier: the chain case (1 500 flat indices) then spans six chunks


def _cases():
    """(name, boxes, cls, thr, iou, mode, cap, chunk)"""
    boxes, cls, thr, iou = C.chain_case()
    yield "chain", boxes, cls, thr, iou, 0, None, MODEL_CHUNK
    yield "chain mode 1", boxes, cls, thr, iou, 1, None, MODEL_CHUNK
    yield "chain cap %d" % CAP, boxes, cls, thr, iou, 0, CAP, MODEL_CHUNK
    yield "chain one chunk", boxes, cls, thr, iou, 0, None, 16384
    yield "chain K=1", boxes, np.ascontiguousarray(cls[:, :, :1]), thr, iou, 0, None, MODEL_CHUNK
    b2, c2, thr, iou = C.chunk_case(512)
    yield "four chunks", b2, c2, thr, iou, 0, None, 512
    yield "four chunks cap 100", b2, c2, thr, iou, 1, 100, 512


def test_reference_and_kernel_model_agree_on_every_case():
    rows = 0
    for name, boxes, cls, thr, iou, mode, cap, chunk in _cases():
        ref = C.reference(boxes, cls, thr, iou, mode, cap)
        got = C.model(boxes, cls, thr, iou, mode, cap, chunk)
        assert C.same(got, ref), name
        rows += sum(len(r["scores"]) for r in ref if r is not None)
    report("class nms cpu: per-class oracle NMS + union sort and the one-sort / class-mask / one-scan model agree on %d kept rows" % rows)


def test_chain_case_loses_a_tenth_of_every_image_to_suppression_and_has_ties_and_threshold_scores():
    boxes, cls, thr, iou = C.chain_case()
    ref = C.chain_reference()
    assert ref[2] is None and all(ref[b] is not None for b in (0, 1, 3))
    for b in (0, 1, 3):
        n, k = ref[b]["ncand"], len(ref[b]["scores"])
        assert n > CAP, "image %d: %d candidates, the capped cases need more than %d" % (b, n, CAP)
        assert k <= 0.9 * n, "image %d keeps %d of %d candidates" % (b, k, n)
        assert len(np.unique(ref[b]["scores"])) < k                                   # ties among the kept rows
    assert (cls == thr).sum() > 50 and int(((cls > thr).sum(-1) > 1).sum()) > 50          # scores AT the threshold; anchors with two classes
    report("class nms cpu: chain case candidates %s kept %s" % ([r["ncand"] if r else 0 for r in ref], [len(r["scores"]) if r else 0 for r in ref]))


@pytest.mark.parametrize("mut", C.MUTANTS)
def test_each_modelled_fault_is_rejected_by_the_reference(mut):
    rejected = []
    for name, boxes, cls, thr, iou, mode, cap, chunk in _cases():
        ref = C.reference(boxes, cls, thr, iou, mode, cap)
        assert C.same(C.model(boxes, cls, thr, iou, mode, cap, chunk), ref), name       # the unmutated model passes
        if not C.same(C.model(boxes, cls, thr, iou, mode, cap, chunk, mut=mut), ref):
            rejected.append(name)
    assert rejected, "no case rejects '%s'" % mut
    if mut in C.MUTANTS[:5]:
        assert "chain" in rejected, "the uncapped chain case must reject '%s'" % mut
    if mut == "cap applied per class":
        assert "chain cap %d" % CAP in rejected
    report("class nms cpu: fault '%s' rejected by %s" % (mut, rejected))


def _badarg():
    src = open(os.path.join(ROOT, "include", "mpn.h")).read()
    return int(re.search(r"#define\s+MPN_E_BADARG\s+\(?(-?\d+)\)?", src).group(1))


def test_class_nms_entry_points_agree_across_header_library_and_ctypes_table():
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
    for name in ("mpn_class_filter_chunk", "mpn_class_filter_workspace_bytes", "mpn_nms_batched_classes_workspace_bytes"):
        assert name in _lib._COUNT_FUNCS
    # the existing NMS entry points keep their signatures
    i, i64, f, vp = ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p
    assert _lib.SIGNATURES["mpn_nms_batched"] == (i, [vp, i64, vp, i, i64, f, i, vp, i64, vp, vp, vp])
    assert _lib.SIGNATURES["mpn_nms_batched_topk"] == (i, [vp, i64, vp, i, i64, i64, f, i, vp, i64, vp, vp, vp])


def test_class_nms_entry_points_size_their_buffers_and_reject_bad_arguments_without_touching_the_gpu():
    from multiposenet.pytorch_amd import _lib
    L = _lib.lib()
    BAD = _badarg()
    nul = ctypes.c_void_p(None)
    a = ctypes.c_void_p(0x1000)          # 16-byte aligned, never dereferenced: validation fails first
    mis4 = ctypes.c_void_p(0x1004)       # 4-byte aligned only
    mis2 = ctypes.c_void_p(0x1002)
    chunk = L.mpn_class_filter_chunk()
    assert chunk > 0 and chunk % 1024 == 0
    # chunk table: one int32 per (image, chunk)
    assert L.mpn_class_filter_workspace_bytes(1, 1, 1) == 4
    assert L.mpn_class_filter_workspace_bytes(3, chunk, 1) == 12 and L.mpn_class_filter_workspace_bytes(3, chunk + 1, 1) == 24
    assert L.mpn_class_filter_workspace_bytes(64, 76725, 80) == 64 * ((76725 * 80 + chunk - 1) // chunk) * 4
    for bad in ((0, 5, 5), (1, 0, 5), (1, 5, 0), (1, -5, 5), (1, 1 << 26, 32), (1, 76725, 27990)):       # the last two: A*K >= 2^31
        assert L.mpn_class_filter_workspace_bytes(*bad) == BAD, bad
    assert L.mpn_class_filter_workspace_bytes(1, (1 << 26) - 1, 32) > 0
    # count pass
    assert L.mpn_class_filter_count(nul, 1, 5, 5, 0.05, a, a, nul) == BAD
    assert L.mpn_class_filter_count(a, 1, 5, 5, 0.05, nul, a, nul) == BAD
    assert L.mpn_class_filter_count(a, 1, 5, 5, 0.05, a, nul, nul) == BAD
    assert L.mpn_class_filter_count(mis2, 1, 5, 5, 0.05, a, a, nul) == BAD
    for bad in ((0, 5, 5), (1, 0, 5), (1, 5, 0), (1, 1 << 26, 32)):
        assert L.mpn_class_filter_count(a, bad[0], bad[1], bad[2], 0.05, a, a, nul) == BAD, bad
    # fill pass: (boxes, cls, B, A, K, thresh, chunk_cnt, nmax, dets, dets_stride, cand_cls, cand_anchor, idx_stride, counts, stream)
    good = [a, mis4, 2, 5, 5, 0.05, a, 7, a, 35, a, a, 7, a, nul]
    for pos in (0, 1, 6, 8, 10, 11, 13):
        args = list(good); args[pos] = nul
        assert L.mpn_class_filter_fill(*args) == BAD, pos
    for pos, val in ((0, mis4), (1, mis2), (2, 0), (3, 0), (4, 0), (3, 1 << 30), (7, 0), (7, 1 << 30), (9, 34), (12, 6)):
        args = list(good); args[pos] = val
        assert L.mpn_class_filter_fill(*args) == BAD, (pos, val)
    # class NMS: (dets, dets_stride, cand_cls, cls_stride, counts, B, nmax, top_k, thresh, mode, keep, keep_stride, num, ws, stream)
    assert L.mpn_nms_batched_classes_workspace_bytes(0, 10) == 256 and L.mpn_nms_batched_classes_workspace_bytes(2, 0) == 256
    for n in (1, 64, 65, 700):
        assert L.mpn_nms_batched_classes_workspace_bytes(3, n) == 3 * (L.mpn_nms_batched_workspace_bytes(1, n) + (n * 4 + 255) // 256 * 256)
    good = [a, 35, a, 7, a, 2, 7, 0, 0.5, 0, a, 7, a, a, nul]
    for pos in (0, 2, 4, 10, 12, 13):
        args = list(good); args[pos] = nul
        assert L.mpn_nms_batched_classes(*args) == BAD, pos
    for pos, val in ((1, 34), (3, 6), (5, 0), (6, 0), (6, 1 << 30), (7, -1), (9, 2), (9, -1), (11, 6)):
        args = list(good); args[pos] = val
        assert L.mpn_nms_batched_classes(*args) == BAD, (pos, val)
    args = list(good); args[7] = 4; args[11] = 3                  # top_k = 4: keep_stride must hold min(nmax, top_k) rows
    assert L.mpn_nms_batched_classes(*args) == BAD
    # class gather: (cand_cls, cand_anchor, idx_stride, keep, keep_stride, num, B, kmax, classes, anchors, out_stride, stream)
    good = [a, a, 7, a, 7, a, 2, 7, a, a, 7, nul]
    for pos in (0, 3, 5, 8):
        args = list(good); args[pos] = nul
        assert L.mpn_gather_cand_class(*args) == BAD, pos
    for pos, val in ((1, nul), (2, 0), (6, 0), (7, 0), (10, 6)):      # anchors asked for without cand_anchor; sizes
        args = list(good); args[pos] = val
        assert L.mpn_gather_cand_class(*args) == BAD, (pos, val)


def test_pre_nms_cap_is_the_argument_then_the_environment_at_call_time_and_only_an_uncapped_dense_image_warns_once(monkeypatch):
    import warnings
    from multiposenet.pytorch_amd import ops
    monkeypatch.setattr(ops, "_NMS_WARNED", [])          # the once-per-process latch, fresh for this test
    monkeypatch.delenv("MPN_NMS_PRE_TOPN", raising=False)
    assert ops._pre_nms_top_n(None, 100) == 0 and ops._pre_nms_top_n(70, 100) == 70
    monkeypatch.setenv("MPN_NMS_PRE_TOPN", "300")
    assert ops._pre_nms_top_n(None, 100) == 300
    assert ops._pre_nms_top_n(50, 100) == 50 and ops._pre_nms_top_n(0, 100) == 0          # an explicit value, 0 = no cap included, wins
    monkeypatch.delenv("MPN_NMS_PRE_TOPN")
    assert ops._pre_nms_top_n(None, 100) == 0                                             # read at call time, not at import
    for junk in ("", "many", "1.5", "-5"):
        monkeypatch.setenv("MPN_NMS_PRE_TOPN", junk)
        assert ops._pre_nms_top_n(None, 100) == 0, junk
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        monkeypatch.setenv("MPN_NMS_PRE_TOPN", "1000")
        assert ops._pre_nms_top_n(None, 100000) == 1000 and ops._pre_nms_top_n(2000, 100000) == 2000
        monkeypatch.delenv("MPN_NMS_PRE_TOPN")
        assert ops._pre_nms_top_n(None, 32768) == 0
        assert not seen and not ops._NMS_WARNED, "a capped call, or 32 768 candidates, must neither warn nor use up the one warning"
        assert ops._pre_nms_top_n(None, 32769) == 0
        assert len(seen) == 1 and "32769 candidates" in str(seen[0].message) and "MPN_NMS_PRE_TOPN" in str(seen[0].message)
        assert ops._pre_nms_top_n(None, 100000) == 0 and ops._pre_nms_top_n(None, 32769) == 0
        assert len(seen) == 1, "the warning fires once per process"


def test_public_interface_carries_the_opt_in_arguments_with_their_defaults():
    import inspect
    from multiposenet.pytorch_amd import ops
    from multiposenet.pytorch_amd.evaluate.tester import TestParams
    from multiposenet.pytorch_amd.network.posenet import poseNet
    sig = inspect.signature(ops.detect_batched_classwise)
    assert list(sig.parameters) == ["boxes", "cls", "score_thresh", "iou_thresh", "mode", "ws_limit", "padded", "pre_nms_top_n"]
    assert [sig.parameters[k].default for k in ("mode", "ws_limit", "padded", "pre_nms_top_n")] == [0, 4 << 30, False, None]
    for fn in (poseNet.detect_padded, poseNet.forward_all_images_padded, poseNet.forward_all_images):
        assert inspect.signature(fn).parameters["class_wise"].default is False, fn
    assert TestParams.nms_per_class is False
