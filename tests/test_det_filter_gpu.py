"""GPU tier of the detection filter / gather tests: mpn_score_filter(_batched), mpn_gather_dets(_batched), mpn_gather_class and
ops.detect_batched against numpy masks, fancy indexing and the oracle NMS (tests/det_filter_ref.py).  Every comparison is exact."""
import numpy as np
import pytest
import torch

import det_filter_ref as D
from helpers import report

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()            # a copy: the cached inputs are read-only


def full(shape, value, dtype):
    return torch.full(shape, value, dtype=dtype, device="cuda")


@pytest.mark.parametrize("A", D.A_SIZES)
def test_score_filter_equals_the_numpy_mask(A):
    from multiposenet.pytorch_amd import _lib, ops
    from multiposenet.pytorch_amd._lib import call
    L = _lib.lib()
    rows = cases = 0
    for name in D.CASES:
        if name == "beyond 1024" and A <= 1024:
            continue
        boxes, scores, thr = D.filter_case(A, name)
        ref = D.ref_filter(boxes, scores, thr)
        d_boxes, d_scores = dev(boxes), dev(scores)
        # every image in one launch, with and without the src list
        for with_src in (True, False):
            dets, src, cnt = full((D.B, A, 5), float(D.SENT_F), torch.float32), full((D.B, A), D.SENT_I, torch.int32), full((D.B,), D.SENT_I, torch.int32)
            call("mpn_score_filter_batched", ops.ptr(d_boxes), ops.ptr(d_scores), D.B, A, float(thr), ops.ptr(dets), ops.ptr(src) if with_src else None,
                 ops.ptr(cnt), ops.stream_ptr())
            rows += D.check_filter(ref, cnt.cpu().numpy(), dets.cpu().numpy(), src.cpu().numpy() if with_src else None)
            assert with_src or (src.cpu().numpy() == D.SENT_I).all()
        # the single-image entry on each image in turn
        for b in range(D.B):
            dets, src, cnt = full((1, A, 5), float(D.SENT_F), torch.float32), full((1, A), D.SENT_I, torch.int32), full((1,), D.SENT_I, torch.int32)
            call("mpn_score_filter", ops.ptr(d_boxes[b]), ops.ptr(d_scores[b]), A, float(thr), ops.ptr(dets), ops.ptr(src), ops.ptr(cnt), ops.stream_ptr())
            rows += D.check_filter(tuple(r[b:b + 1] for r in ref), cnt.cpu().numpy(), dets.cpu().numpy(), src.cpu().numpy())
        cases += 1
    # src == NULL: rejected by the single-image entry before any launch
    dets, cnt = full((1, A, 5), float(D.SENT_F), torch.float32), full((1,), D.SENT_I, torch.int32)
    assert L.mpn_score_filter(ops.ptr(d_boxes), ops.ptr(d_scores), A, float(thr), ops.ptr(dets), None, ops.ptr(cnt), ops.stream_ptr()) == -2
    torch.cuda.synchronize()
    assert int(cnt.item()) == D.SENT_I and (dets.cpu().numpy() == D.SENT_F).all()
    report("det_filter gpu: score filter A=%-4d %d cases x (batched with src, batched without, 3 single images): %d passing rows equal "
           "np.nonzero order, every other row keeps the sentinel" % (A, cases, rows))


@pytest.mark.parametrize("kmax", D.KMAX)
def test_gathers_equal_fancy_indexing(kmax):
    from multiposenet.pytorch_amd import ops
    from multiposenet.pytorch_amd._lib import call
    c = D.gather_case(kmax)
    ref = D.ref_gather(c)
    nb, os_ = c["nb"], c["out_stride"]
    d_dets, d_keep, d_num, d_src, d_cls = dev(c["dets"]), dev(c["keep"]), dev(c["num"]), dev(c["src"]), dev(c["cls_id"])
    boxes, scores, cls = full((nb, os_, 4), float(D.SENT_F), torch.float32), full((nb, os_), float(D.SENT_F), torch.float32), full((nb, os_), D.SENT_I, torch.int64)
    call("mpn_gather_dets_batched", ops.ptr(d_dets), c["dets_stride"], ops.ptr(d_keep), c["keep_stride"], ops.ptr(d_num), nb, kmax, ops.ptr(boxes),
         ops.ptr(scores), os_, ops.stream_ptr())
    call("mpn_gather_class", ops.ptr(d_cls), ops.ptr(d_src), c["A"], ops.ptr(d_keep), c["keep_stride"], ops.ptr(d_num), nb, kmax, ops.ptr(cls), os_,
         ops.stream_ptr())
    rows = D.check_gather(ref, boxes.cpu().numpy(), scores.cpu().numpy(), cls.cpu().numpy())
    # the single-image entries (k rows from the host, num == NULL) on every image that keeps something
    for b in range(nb):
        k = int(c["num"][b])
        if k == 0:
            continue
        b1, s1, c1 = full((os_, 4), float(D.SENT_F), torch.float32), full((os_,), float(D.SENT_F), torch.float32), full((os_,), D.SENT_I, torch.int64)
        call("mpn_gather_dets", ops.ptr(d_dets[b]), ops.ptr(d_keep[b]), k, ops.ptr(b1), ops.ptr(s1), ops.stream_ptr())
        call("mpn_gather_class", ops.ptr(d_cls[b]), ops.ptr(d_src[b]), c["A"], ops.ptr(d_keep[b]), 0, None, 1, k, ops.ptr(c1), os_, ops.stream_ptr())
        want_c = ref[2][b].copy()
        want_c[k:] = D.SENT_I                                        # kmax == k here: no padding rows
        D.check_gather((ref[0][b:b + 1], ref[1][b:b + 1], want_c[None]), b1.cpu().numpy()[None], s1.cpu().numpy()[None], c1.cpu().numpy()[None])
        rows += os_
    report("det_filter gpu: gathers kmax=%-3d num %s: %d output rows equal the indexed rows / class ids, padding ids 0, the rest untouched" % (
        kmax, c["num"].tolist(), rows))


@pytest.mark.parametrize("with_cls", [True, False], ids=["classes", "no classes"])
@pytest.mark.parametrize("padded", [True, False], ids=["padded", "views"])
def test_detect_batched_equals_numpy_filter_oracle_nms_numpy_gather(padded, with_cls):
    from multiposenet.pytorch_amd import ops
    from multiposenet.pytorch_amd._lib import call
    boxes, scores, cls_id, thr, iou = D.chain_case()
    ref, counts = D.ref_chain(boxes, scores, cls_id, thr, iou)
    d_boxes, d_scores, d_cls = dev(boxes), dev(scores), dev(cls_id)
    per_img = call("mpn_nms_batched_workspace_bytes", 1, int(counts.max()))
    rows = 0
    for ws_limit in (4 << 30, per_img * 2 + 1, per_img):              # one launch set; groups of two images; one image at a time
        res = ops.detect_batched(d_boxes, d_scores, float(thr), float(iou), mode=0, ws_limit=ws_limit, padded=padded, cls_id=d_cls if with_cls else None)
        torch.cuda.synchronize()
        if padded:
            ob, osc, kept = res[0].cpu().numpy(), res[1].cpu().numpy(), res[2]
            oc = res[3].cpu().numpy() if with_cls else None
            assert ob.shape[1] == counts.max() and len(res) == (4 if with_cls else 3)
            per = [(ob[b, :kept[b]], osc[b, :kept[b]], oc[b, :kept[b]] if with_cls else None) if kept[b] else None for b in range(len(kept))]
            if with_cls:
                for b in range(len(kept)):
                    assert (oc[b, kept[b]:] == 0).all()              # class padding up to nmax
        else:
            assert all(len(r) == (3 if with_cls else 2) for r in res)
            per = [None if r[0] is None else tuple(x.cpu().numpy() for x in r) + ((None,) if not with_cls else ()) for r in res]
        for b, (got, want) in enumerate(zip(per, ref)):
            assert (got is None) == (want is None), "image %d" % b
            if want is None:
                continue
            assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), "image %d" % b
            if with_cls:
                assert got[2].dtype == np.int64 and np.array_equal(got[2], want[2]), "image %d" % b
            rows += len(want[1])
    report("det_filter gpu: detect_batched padded=%s classes=%s: %d kept rows equal numpy filter + oracle NMS + numpy gather over 3 workspace "
           "limits (1, 2 and 4 NMS groups); candidates %s" % (padded, with_cls, rows, counts.tolist()))
