"""GPU tier of the class-wise post-processing of K-class heads: mpn_class_filter_count / _fill, mpn_nms_batched_classes,
mpn_gather_cand_class through the C ABI, ops.detect_batched_classwise, poseNet.detect_padded(class_wise=True) and
Tester.detect_images / coco_eval_bbox with params.nms_per_class, each against tests/class_nms_ref.py's reference (np.nonzero, the
oracle NMS on every class's rows separately, the union sorted by score).  Every comparison is an equality of bytes."""
import ctypes

import numpy as np
import pytest
import torch

import class_nms_ref as C
from helpers import report

pytestmark = pytest.mark.gpu

f32 = np.float32
SCORE_CASES = ("mixed", "all", "none", "equal to the threshold", "nan", "last chunk only", "empty image between")


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()


def full(shape, value, dtype):
    return torch.full(shape, value, dtype=dtype, device="cuda")


def _chunk():
    from multiposenet.pytorch_amd._lib import call
    return call("mpn_class_filter_chunk")


def _scores(A, K, name, chunk):
    """boxes [3,A,4], cls [3,A,K]: det_filter_ref's score cases over the flat (anchor, class) index."""
    rs = np.random.RandomState(A * 7 + K * 131 + SCORE_CASES.index(name))
    nb, n = 3, A * K
    boxes = rs.uniform(0, 500, (nb, A, 4)).astype(f32)
    lo = rs.uniform(0.0, 0.049, (nb, n)).astype(f32)
    hi = rs.uniform(0.051, 1.0, (nb, n)).astype(f32)
    mixed = np.where(rs.rand(nb, n) < np.array([0.5, 0.05, 0.9])[:, None], hi, lo)
    idx = np.arange(n)[None, :]
    if name == "mixed":
        s = mixed
    elif name == "all":
        s = hi
    elif name == "none":
        s = lo
    elif name == "equal to the threshold":
        s = np.where(rs.rand(nb, n) < 0.34, C.THR, mixed)
        s[:, 0] = C.THR
    elif name == "nan":
        s = np.where(rs.rand(nb, n) < 0.34, f32(np.nan), mixed)
        s[:, n - 1] = np.nan
    elif name == "last chunk only":
        s = np.where(idx >= (n - 1) // chunk * chunk, np.where(rs.rand(nb, n) < 0.7, hi, lo), lo)
        s[:, n - 1] = hi[:, n - 1]
    elif name == "empty image between":
        s = mixed.copy()
        s[1] = lo[1]
    return boxes, np.ascontiguousarray(s, dtype=f32).reshape(nb, A, K)


def _ref_filter(boxes, cls, thr, nmax, dets_stride, idx_stride):
    nb, A, K = cls.shape
    counts = np.zeros(nb, dtype=np.int32)
    dets = np.full((nb, dets_stride), C.SENT_F, dtype=f32)
    ccls = np.full((nb, idx_stride), C.SENT_I, dtype=np.int32)
    canc = np.full((nb, idx_stride), C.SENT_I, dtype=np.int32)
    for b in range(nb):
        f, rows = C.ref_candidates(boxes[b], cls[b], thr)
        counts[b] = len(f)
        dets[b, :len(f) * 5] = rows.reshape(-1)
        ccls[b, :len(f)] = f % K
        canc[b, :len(f)] = f // K
    return counts, dets, ccls, canc


def _run_filter(d_boxes, d_cls, thr, pad=0):
    """count pass, host read of the counts, fill pass into sentinel-filled outputs with `pad` spare rows per image."""
    from multiposenet.pytorch_amd import ops
    from multiposenet.pytorch_amd._lib import call
    nb, A, K = d_cls.shape
    words = call("mpn_class_filter_workspace_bytes", nb, A, K) // 4
    assert words == nb * ((A * K + _chunk() - 1) // _chunk())
    table = full((words + 4,), C.SENT_I, torch.int32)
    counts = full((nb,), C.SENT_I, torch.int32)
    call("mpn_class_filter_count", ops.ptr(d_cls), nb, A, K, float(thr), ops.ptr(table), ops.ptr(counts), ops.stream_ptr())
    cnt = counts.cpu().numpy()
    tab = table.cpu().numpy()
    assert (tab[words:] == C.SENT_I).all() and np.array_equal(tab[:words].reshape(nb, -1).sum(1), cnt)
    nmax = max(int(cnt.max()), 1)
    ds, is_ = (nmax + pad) * 5 + (3 if pad else 0), nmax + pad
    dets, ccls, canc = full((nb, ds), float(C.SENT_F), torch.float32), full((nb, is_), C.SENT_I, torch.int32), full((nb, is_), C.SENT_I, torch.int32)
    counts2 = full((nb,), C.SENT_I, torch.int32)
    call("mpn_class_filter_fill", ops.ptr(d_boxes), ops.ptr(d_cls), nb, A, K, float(thr), ops.ptr(table), nmax, ops.ptr(dets), ds, ops.ptr(ccls),
         ops.ptr(canc), is_, ops.ptr(counts2), ops.stream_ptr())
    return cnt, counts2.cpu().numpy(), dets.cpu().numpy(), ccls.cpu().numpy(), canc.cpu().numpy(), nmax, ds, is_


def _check_filter(boxes, cls, got, thr=C.THR):
    cnt, cnt2, dets, ccls, canc, nmax, ds, is_ = got
    rc, rd, rk, ra = _ref_filter(boxes, cls, thr, nmax, ds, is_)
    assert np.array_equal(cnt, rc) and np.array_equal(cnt2, rc), "counts %s / %s, expected %s" % (cnt.tolist(), cnt2.tolist(), rc.tolist())
    assert np.array_equal(dets.view(np.uint32), rd.view(np.uint32)), "dets (or a row that should keep its sentinel) differ"
    assert np.array_equal(ccls, rk), "classes differ at %s" % np.argwhere(ccls != rk)[:4].tolist()
    assert np.array_equal(canc, ra), "anchors differ at %s" % np.argwhere(canc != ra)[:4].tolist()
    return int(rc.sum())


def _filter_sizes():
    for A in (1, 63, 65, 1025):
        for K in (1, 3, 5, 80):
            yield A, K
    ch = 16384                                   # asserted against mpn_class_filter_chunk() in the test
    for n in (ch - 1, ch, ch + 1, 2 * ch + 1):
        yield n, 1
    yield (ch + 1) // 5, 5                       # A*K = chunk length + 1 with K = 5
    yield (2 * ch + 1) // 3, 3                   # A*K = 2 * chunk length + 1 with K = 3


@pytest.mark.parametrize("A,K", list(_filter_sizes()), ids=lambda v: str(v))
def test_class_filter_equals_np_nonzero_over_the_flat_scores(A, K):
    chunk = _chunk()
    assert chunk == 16384, "the sizes of this test are placed around a chunk length of 16 384"
    rows = cases = 0
    for name in SCORE_CASES:
        boxes, cls = _scores(A, K, name, chunk)
        d_boxes, d_cls = dev(boxes), dev(cls)
        first = _run_filter(d_boxes, d_cls, C.THR)
        rows += _check_filter(boxes, cls, first)
        if name == "mixed":
            # a second launch pair writes the same bytes; larger strides leave the spare rows untouched
            again = _run_filter(d_boxes, d_cls, C.THR)
            assert all(np.array_equal(x.view(np.uint32) if x.dtype == f32 else x, y.view(np.uint32) if y.dtype == f32 else y)
                       for x, y in zip(first[:5], again[:5]))
            _check_filter(boxes, cls, _run_filter(d_boxes, d_cls, C.THR, pad=5))
            # cls one float past a 16-byte boundary: every image's base moves through the four alignments
            buf = torch.zeros((cls.size + 8,), dtype=torch.float32, device="cuda")
            for off in (1, 2, 3):
                view = buf[off:off + cls.size].view(3, A, K)
                view.copy_(d_cls)
                _check_filter(boxes, cls, _run_filter(d_boxes, view, C.THR))
            # the same image at batch position 0 and 2
            swapped = np.ascontiguousarray(cls[[2, 1, 0]]), np.ascontiguousarray(boxes[[2, 1, 0]])
            sw = _run_filter(dev(swapped[1]), dev(swapped[0]), C.THR)
            _check_filter(swapped[1], swapped[0], sw)
            n0 = int(first[0][0])
            assert sw[0][2] == n0 and np.array_equal(sw[2][2, :n0 * 5].view(np.uint32), first[2][0, :n0 * 5].view(np.uint32))
            assert np.array_equal(sw[3][2, :n0], first[3][0, :n0]) and np.array_equal(sw[4][2, :n0], first[4][0, :n0])
        cases += 1
    report("class nms gpu: filter A=%-5d K=%-2d (%d flat scores, %d chunks) %d score cases: %d candidate rows equal np.nonzero order, every "
           "other row keeps the sentinel" % (A, K, A * K, (A * K + chunk - 1) // chunk, cases, rows))


# ---------------------------------------------------------------------------------------------- class NMS through the C ABI
def _run_nms(dets_list, cls_list, iou, mode, top_k=0, pad=0):
    """mpn_nms_batched_classes on images of different candidate counts -> per image the kept rows (int64)."""
    from multiposenet.pytorch_amd import ops
    from multiposenet.pytorch_amd._lib import call
    nb = len(dets_list)
    nmax = max(max(len(d) for d in dets_list), 1)
    live = min(nmax, top_k) if top_k > 0 else nmax
    ds, cs, ks = (nmax + pad) * 5 + (2 if pad else 0), nmax + pad, live + pad
    dets = np.full((nb, ds), C.SENT_F, dtype=f32)
    ccls = np.full((nb, cs), C.SENT_I, dtype=np.int32)
    for b in range(nb):
        dets[b, :len(dets_list[b]) * 5] = np.asarray(dets_list[b], dtype=f32).reshape(-1)
        ccls[b, :len(cls_list[b])] = cls_list[b]
    counts = dev(np.array([len(d) for d in dets_list], dtype=np.int32))
    d_dets, d_cls = dev(dets), dev(ccls)
    keep, num = full((nb, ks), C.SENT_I, torch.int64), full((nb,), C.SENT_I, torch.int64)
    ws = torch.empty((call("mpn_nms_batched_classes_workspace_bytes", nb, live),), dtype=torch.uint8, device="cuda")
    call("mpn_nms_batched_classes", ops.ptr(d_dets), ds, ops.ptr(d_cls), cs, ops.ptr(counts), nb, nmax, top_k, float(iou), mode, ops.ptr(keep),
         ks, ops.ptr(num), ops.ptr(ws), ops.stream_ptr())
    keep, num = keep.cpu().numpy(), num.cpu().numpy()
    out = []
    for b in range(nb):
        assert (keep[b, num[b]:] == C.SENT_I).all(), "image %d: keep rows past the count were written" % b
        out.append(keep[b, :num[b]].copy())
    return out


def _rand_rows(rs, n, K, span=120.0, levels=32):
    xy = rs.uniform(0, span, (n, 2))
    wh = rs.uniform(15, 60, (n, 2))
    sc = np.ceil(rs.uniform(0.06, 1.0, (n, 1)) * levels) / levels          # ties
    return np.concatenate([xy, xy + wh, sc], 1).astype(f32), rs.randint(0, K, n).astype(np.int32)


@pytest.mark.parametrize("mode", [0, 1])
def test_class_nms_equals_the_oracle_run_on_every_class_separately(mode):
    rs = np.random.RandomState(77 + mode)
    sizes = (1, 63, 64, 65, 129, 700, 0)
    dets, ccls = zip(*[_rand_rows(rs, n, 5, span=60.0 + n / 4.0) for n in sizes])
    rows = 0
    for top_k, pad in ((0, 0), (0, 3), (100, 0), (64, 2), (5000, 0)):
        got = _run_nms(dets, ccls, C.IOU, mode, top_k, pad)
        for b, n in enumerate(sizes):
            want = C.reference_rows(dets[b], ccls[b], C.IOU, mode, top_k or None)
            assert np.array_equal(got[b], want), "n=%d top_k=%d: kept rows differ" % (n, top_k)
            if n == 700 and top_k == 0:
                assert len(want) < 0.9 * n                                   # the suppression does something here
            rows += len(want)
    report("class nms gpu: mode %d, n in %s, top_k in (none, 100, 64, 5000): %d kept rows equal the per-class oracle" % (mode, list(sizes), rows))


def test_class_nms_identical_boxes_ties_and_pairs_exactly_at_the_threshold():
    from test_nms_ref_gpu import _near_threshold_pairs
    box = [10.0, 20.0, 50.0, 80.0]
    # the same box four times: classes 0 0 1 2 -> one row of class 0 (the better score), and the rows of classes 1 and 2
    d = np.array([box + [0.5], box + [0.9], box + [0.7], box + [0.7]], dtype=f32)
    for mode in (0, 1):
        got = _run_nms([d], [np.array([0, 0, 1, 2], dtype=np.int32)], C.IOU, mode)[0]
        assert got.tolist() == [1, 2, 3]                      # descending score; the tie between rows 2 and 3 by position (lower f)
        assert _run_nms([d], [np.zeros(4, dtype=np.int32)], C.IOU, mode)[0].tolist() == [1]
    # equal scores across classes, disjoint boxes: the order is the order of the candidate list whatever the classes are
    n = 130
    d = np.array([[40.0 * i, 0, 40.0 * i + 20, 20, 0.25] for i in range(n)], dtype=f32)
    for cl in (np.arange(n) % 3, (n - np.arange(n)) % 7):
        assert _run_nms([d], [cl.astype(np.int32)], C.IOU, 0)[0].tolist() == list(range(n))
    # top_k with ties straddling the cut: rows 0..9 score .5 (disjoint), the cut at 6 keeps rows 0..5
    assert _run_nms([d[:10]], [np.arange(10, dtype=np.int32) % 2], C.IOU, 0, top_k=6)[0].tolist() == list(range(6))
    # pairs whose IoU is exactly 1/2 (the existing NMS tests' construction, the exact tenth of it), each pair far from the others
    p = _near_threshold_pairs(np.random.RandomState(3), 400)
    h = p.shape[0] // 2
    exact = np.nonzero((p[:h, :4] == np.floor(p[:h, :4])).all(1) & (p[h:, :4] == np.floor(p[h:, :4])).all(1))[0][:20]
    assert len(exact) >= 10
    a, b = p[exact].copy(), p[exact + h].copy()
    shift = (np.arange(len(exact)) * 4096.0).astype(f32)
    for q in (a, b):
        q[:, 0] += shift
        q[:, 2] += shift
    d = np.concatenate([a, b], 0)
    m = len(exact)
    same_cls = np.concatenate([np.arange(m) % 3, np.arange(m) % 3]).astype(np.int32)
    other_cls = np.concatenate([np.zeros(m), np.ones(m)]).astype(np.int32)
    for mode, kept in ((0, 2 * m), (1, m)):
        got = _run_nms([d], [same_cls], f32(0.5), mode)[0]
        assert len(got) == kept and np.array_equal(got, C.reference_rows(d, same_cls, f32(0.5), mode)), "mode %d" % mode
        assert len(_run_nms([d], [other_cls], f32(0.5), mode)[0]) == 2 * m       # different classes: nothing is suppressed
    report("class nms gpu: identical boxes, ties across classes, top_k ties, %d pairs at IoU == 1/2 (mode 0 keeps both, mode 1 one)" % m)


@pytest.mark.parametrize("top_k", [0, 90])
def test_class_nms_with_one_class_equals_nms_batched_byte_for_byte(top_k):
    from multiposenet.pytorch_amd import ops
    from multiposenet.pytorch_amd._lib import call
    rs = np.random.RandomState(9)
    sizes = (700, 0, 1, 129, 64)
    rows = [_rand_rows(rs, n, 1, span=80.0)[0] for n in sizes]
    nb, nmax = len(sizes), max(sizes)
    live = min(nmax, top_k) if top_k else nmax
    dets = np.zeros((nb, nmax, 5), dtype=f32)
    for b, r in enumerate(rows):
        dets[b, :len(r)] = r
    d_dets, counts = dev(dets), dev(np.array(sizes, dtype=np.int32))
    zeros = torch.zeros((nb, nmax), dtype=torch.int32, device="cuda")
    for mode in (0, 1):
        k0, n0 = full((nb, live), C.SENT_I, torch.int64), full((nb,), C.SENT_I, torch.int64)
        k1, n1 = full((nb, live), C.SENT_I, torch.int64), full((nb,), C.SENT_I, torch.int64)
        ws = torch.empty((call("mpn_nms_batched_classes_workspace_bytes", nb, live),), dtype=torch.uint8, device="cuda")
        head = (ops.ptr(d_dets), nmax * 5, ops.ptr(counts), nb, nmax)
        tail = (float(C.IOU), mode, ops.ptr(k0), live, ops.ptr(n0), ops.ptr(ws), ops.stream_ptr())
        if top_k:
            call("mpn_nms_batched_topk", *(head + (top_k,) + tail))
        else:
            call("mpn_nms_batched", *(head + tail))
        call("mpn_nms_batched_classes", ops.ptr(d_dets), nmax * 5, ops.ptr(zeros), nmax, ops.ptr(counts), nb, nmax, top_k, float(C.IOU), mode,
             ops.ptr(k1), live, ops.ptr(n1), ops.ptr(ws), ops.stream_ptr())
        assert torch.equal(n0, n1) and torch.equal(k0, k1) and int(n0.max()) > 1


def test_gather_cand_class_pads_with_zeros_and_gathers_the_anchor():
    from multiposenet.pytorch_amd import ops
    from multiposenet.pytorch_amd._lib import call
    rs = np.random.RandomState(4)
    nb, n, kmax, istr, kstr, ostr = 4, 300, 257, 310, 260, 263
    ccls = rs.randint(0, 80, (nb, istr)).astype(np.int32)
    canc = rs.randint(0, 1 << 20, (nb, istr)).astype(np.int32)
    keep = np.stack([rs.permutation(n)[:kstr] for _ in range(nb)]).astype(np.int64)
    num = np.array([0, 1, kmax - 1, kmax], dtype=np.int64)
    d_cls, d_anc, d_keep, d_num = dev(ccls), dev(canc), dev(keep), dev(num)
    for with_anchor in (True, False):
        oc, oa = full((nb, ostr), C.SENT_I, torch.int64), full((nb, ostr), C.SENT_I, torch.int64)
        call("mpn_gather_cand_class", ops.ptr(d_cls), ops.ptr(d_anc) if with_anchor else None, istr, ops.ptr(d_keep), kstr, ops.ptr(d_num),
             nb, kmax, ops.ptr(oc), ops.ptr(oa) if with_anchor else None, ostr, ops.stream_ptr())
        wc, wa = np.full((nb, ostr), C.SENT_I, dtype=np.int64), np.full((nb, ostr), C.SENT_I, dtype=np.int64)
        for b in range(nb):
            k = int(num[b])
            wc[b, :k], wa[b, :k] = ccls[b, keep[b, :k]], canc[b, keep[b, :k]]
            wc[b, k:kmax] = wa[b, k:kmax] = 0
        assert np.array_equal(oc.cpu().numpy(), wc)
        assert np.array_equal(oa.cpu().numpy(), wa if with_anchor else np.full((nb, ostr), C.SENT_I, dtype=np.int64))


# ---------------------------------------------------------------------------------------------- the chain
def _check_rows(got, want, what):
    """got: (boxes, scores, classes) numpy or None; want: class_nms_ref.reference's entry."""
    assert (got is None) == (want is None), what
    if want is None:
        return 0
    assert np.array_equal(got[0].view(np.uint32), want["boxes"].view(np.uint32)), what
    assert np.array_equal(got[1].view(np.uint32), want["scores"].view(np.uint32)), what
    assert got[2].dtype == np.int64 and np.array_equal(got[2], want["classes"]), what
    return len(want["scores"])


@pytest.mark.parametrize("cap", [None, 150], ids=["no cap", "pre_nms_top_n 150"])
@pytest.mark.parametrize("padded", [True, False], ids=["padded", "views"])
def test_detect_batched_classwise_equals_the_reference(padded, cap):
    """Two host reads per batch, by construction of ops.detect_batched_classwise: ``counts.tolist()`` after the count pass and
    ``num.tolist()`` after the gathers (the existing detect tests do not count transfers either); here the host objects it returns are
    checked: the kept counts are a list of Python ints and every tensor is still on the device."""
    from multiposenet.pytorch_amd import ops
    from multiposenet.pytorch_amd._lib import call
    boxes, cls, thr, iou = C.chain_case()
    d_boxes, d_cls = dev(boxes), dev(cls)
    rows = 0
    for mode in (0, 1):
        ref = C.chain_reference(mode, cap)
        ncand = max(r["ncand"] for r in ref if r is not None)
        per_img = call("mpn_nms_batched_classes_workspace_bytes", 1, min(ncand, cap) if cap else ncand)
        for ws_limit in (4 << 30, per_img * 2 + 1, per_img):          # one launch set; groups of two images; one image at a time
            res = ops.detect_batched_classwise(d_boxes, d_cls, float(thr), float(iou), mode=mode, ws_limit=ws_limit, padded=padded, pre_nms_top_n=cap)
            if padded:
                ob, osc, kept, oc = res
                assert all(t_.is_cuda for t_ in (ob, osc, oc)) and isinstance(kept, list) and all(type(k) is int for k in kept)
                assert ob.shape == (4, min(ncand, cap) if cap else ncand, 4) and oc.dtype == torch.int64
                ob, osc, oc = ob.cpu().numpy(), osc.cpu().numpy(), oc.cpu().numpy()
                per = [(ob[b, :k], osc[b, :k], oc[b, :k]) if ref[b] is not None else None for b, k in enumerate(kept)]
                assert kept[2] == 0 and all((oc[b, k:] == 0).all() for b, k in enumerate(kept))
            else:
                assert len(res) == 4 and all(len(r) == 3 for r in res)
                per = [None if r[0] is None else tuple(x.cpu().numpy() for x in r) for r in res]
            for b in range(4):
                rows += _check_rows(per[b], ref[b], "mode %d image %d" % (mode, b))
    report("class nms gpu: detect_batched_classwise padded=%s cap=%s: %d kept rows equal the reference over 2 modes x 3 workspace limits" % (padded, cap, rows))


def test_detect_batched_classwise_with_one_class_equals_detect_batched():
    from multiposenet.pytorch_amd import ops
    import det_filter_ref as D
    boxes, scores, _, thr, iou = D.chain_case()
    d_boxes, d_scores = dev(boxes), dev(scores)
    for cap in (None, 200):
        a = ops.detect_batched(d_boxes, d_scores, float(thr), float(iou), padded=True, pre_nms_top_n=cap)
        b = ops.detect_batched_classwise(d_boxes, d_scores.reshape(4, -1, 1), float(thr), float(iou), padded=True, pre_nms_top_n=cap)
        assert a[2] == b[2] and a[0].shape == b[0].shape and max(a[2]) > 0 and int(b[3].abs().sum()) == 0
        for i, k in enumerate(a[2]):
            assert torch.equal(a[0][i, :k], b[0][i, :k]) and torch.equal(a[1][i, :k], b[1][i, :k])


# ---------------------------------------------------------------------------------------------- model
def test_k3_detect_padded_class_wise_equals_the_reference_on_the_models_own_outputs():
    from multiposenet.pytorch_amd import synthetic as weightgen
    from test_multiclass_gpu import model_k, t
    K, B = 3, 2
    m, _ = model_k(50, torch.float32, K, seed=5, swap=False)
    m.eval()
    img = t(weightgen.gen_images(11, B, 128, 96)).cuda()
    with torch.no_grad():
        heat, boxes_all, cls, keep = m.forward_padded_begin(img)
        plain = m.detect_padded(boxes_all, cls, return_class=True)
        off = m.detect_padded(boxes_all, cls, return_class=True, class_wise=False)
        pb, ps, kept, pc = m.detect_padded(boxes_all, cls, return_class=True, class_wise=True)
        three = m.detect_padded(boxes_all, cls, class_wise=True)
        hp, fb, fs, fkept, fc = m.forward_all_images_padded(img, return_class=True, class_wise=True)
        _, per_img = m.forward_all_images(img, class_wise=True)
    torch.cuda.synchronize()
    # class_wise=False is the call without the argument
    assert plain[2] == off[2] and torch.equal(plain[3], off[3])
    for b, k in enumerate(plain[2]):                            # rows past the kept count of the padded tensors are not defined
        assert torch.equal(plain[0][b, :k], off[0][b, :k]) and torch.equal(plain[1][b, :k], off[1][b, :k])
    ref = C.reference(boxes_all.cpu().numpy(), cls.cpu().numpy(), f32(0.05), f32(0.5))
    assert len(three) == 3 and three[2] == kept and fkept == kept and torch.equal(hp, heat)
    rows = 0
    for b in range(B):
        k = kept[b]
        assert k > 0 and len(set(ref[b]["classes"].tolist())) > 1
        rows += _check_rows((pb[b, :k].cpu().numpy(), ps[b, :k].cpu().numpy(), pc[b, :k].cpu().numpy()), ref[b], "image %d" % b)
        _check_rows((fb[b, :k].cpu().numpy(), fs[b, :k].cpu().numpy(), fc[b, :k].cpu().numpy()), ref[b], "forward_all_images_padded, image %d" % b)
        _check_rows((per_img[b][2].cpu().numpy(), per_img[b][0].cpu().numpy(), per_img[b][1].cpu().numpy()), ref[b], "forward_all_images, image %d" % b)
        assert int(pc[b, k:].abs().sum()) == 0
    assert sum(kept) > sum(plain[2]), "every anchor yields one candidate on the class-maximum path: the class-wise one must keep more here"
    report("class nms gpu: K=3 R50 128x96 detect_padded(class_wise=True): %d kept rows equal the reference (class-maximum path: %d)" % (rows, sum(plain[2])))


def test_single_class_detect_padded_class_wise_is_byte_identical():
    from multiposenet.pytorch_amd import synthetic as weightgen
    from test_multiclass_gpu import model_k, t
    m, _ = model_k(50, torch.float32, 1, swap=False)
    m.eval()
    img = t(weightgen.gen_images(11, 2, 128, 96)).cuda()
    with torch.no_grad():
        heat, boxes_all, cls, keep = m.forward_padded_begin(img)
        a = m.detect_padded(boxes_all, cls, return_class=True)
        b = m.detect_padded(boxes_all, cls, return_class=True, class_wise=True)
    assert a[2] == b[2] and max(a[2]) > 0 and a[0].shape == b[0].shape and int(b[3].abs().sum()) == 0 and b[3].shape == a[3].shape
    for i, k in enumerate(a[2]):
        assert torch.equal(a[0][i, :k], b[0][i, :k]) and torch.equal(a[1][i, :k], b[1][i, :k])


# ---------------------------------------------------------------------------------------------- Tester
def test_tester_nms_per_class_keeps_two_categories_on_the_same_anchors():
    """A 3-class R50 fp32 head at inp_size 96 whose class 1 is class 0 with a slightly lower bias: both fire on the same anchors, class 1
    never is an anchor's arg-max.  With params.nms_per_class the tester returns the reference's rows (both categories on the same
    boxes); the default path returns no row of class 1 at all."""
    import box_eval_ref as R
    from multiposenet.pytorch_amd.evaluate.tester import Tester, TestParams
    from test_box_eval_gpu import _lift_scores, _network_input
    from test_multiclass_gpu import model_k
    S, K = 96, 3
    model, _ = model_k(50, torch.float32, K, swap=False)
    model.eval()
    model.freeze_bn()
    out = model.classificationModel.output
    with torch.no_grad():
        w = out.weight.data.view(9, K, 256, 3, 3)               # output channel = anchor * K + class
        w[:, 1].copy_(w[:, 0].clone())
        bias = out.bias.data.view(9, K)
        bias[:, 1].copy_(bias[:, 0] - 0.25)
    _lift_scores(model, S)
    params = TestParams()
    params.ckpt, params.inp_size = None, S
    params.category_ids = [11, 4, 30]
    assert params.nms_per_class is False
    tester = Tester(model, params)
    rs = np.random.RandomState(1)
    images = [(5, "a.jpg", rs.uniform(0, 255, (64, 96, 3)).astype(np.float32)), (9, "b.jpg", rs.uniform(0, 255, (64, 48, 3)).astype(np.float32))]
    default = tester.detect_images(images)
    params.nms_per_class = True
    dets = tester.detect_images(images)
    # the reference on the model's own decoded boxes and class scores
    with torch.no_grad():
        x = torch.stack([_network_input(tester, img) for _, _, img in images])
        _, boxes_all, cls, keep = model.forward_padded_begin(x)
    torch.cuda.synchronize()
    cls_h = cls.cpu().numpy()
    both = (cls_h[..., 0] > 0.05) & (cls_h[..., 1] > 0.05)
    assert (cls_h[..., 1] < cls_h[..., 0]).all() and both.any(1).all(), "class 1 must fire below class 0 on the same anchors"
    ref = C.reference(boxes_all.cpu().numpy(), cls_h, f32(0.05), f32(0.5))

    def rows_of(limit=None):
        want = []
        for li, (image_id, name, img) in enumerate(images):
            scale = np.float32(float(max(img.shape[0], img.shape[1])) / S)
            r = ref[li]
            for j in range(len(r["scores"]) if limit is None else min(limit, len(r["scores"]))):
                b = (r["boxes"][j] * scale).astype(np.float64)
                want.append({'image_id': image_id, 'file_name': name, 'category_id': params.category_ids[int(r["classes"][j])],
                             'bbox': [b[0], b[1], b[2] - b[0], b[3] - b[1]], 'score': float(r["scores"][j])})
        return want

    assert dets == rows_of()
    assert tester.detect_images(images, max_per_image=5) == rows_of(5)                     # the first five across classes
    # image 5: the best row of category 11 and the row of category 4 on the same box are two ground truths at IoU 1
    top = next(d for d in dets if d['image_id'] == 5 and d['category_id'] == 11)
    twin = [d for d in dets if d['image_id'] == 5 and d['category_id'] == 4 and d['bbox'] == top['bbox']]
    assert len(twin) == 1, "the per-class path must keep the box of category 4 that lies on the best box of category 11"
    assert not [d for d in default if d['category_id'] == 4], "the class-maximum path never yields class 1 here"
    anns = [R.ann(5, 11, top['bbox']), R.ann(5, 4, top['bbox']), R.ann(9, 30, [4, 6, 20, 24])]
    got = tester.coco_eval_bbox(images, anns)
    assert got == dets and tester.last_box_eval is not None and tester.last_box_eval['stats'][0] > 0
    per_class = tester.last_box_eval
    params.nms_per_class = False
    assert tester.coco_eval_bbox(images, anns) == default
    k4 = sorted(params.category_ids).index(4)                                             # categories are evaluated in ascending id
    line = "Tester nms_per_class: %d rows (default path %d), AP of category 4 %.4f against %.4f with the class-maximum path" % (
        len(dets), len(default), per_class['per_category_ap'][k4], tester.last_box_eval['per_category_ap'][k4])
    print(line)
    report(line)
    # category 4's ground truth is found by the per-class path only
    assert per_class['per_category_ap'][k4] > 0 and tester.last_box_eval['per_category_ap'][k4] == 0
