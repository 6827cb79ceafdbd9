"""Inputs and two independent numpy formulations of the class-wise post-processing of a K-class detection head (csrc/nms.hip:
class_filter_count_kernel / class_filter_fill_kernel, nms_rank_kernel<true> / nms_mask_kernel<true>, gather_cand_class_kernel;
ops.detect_batched_classwise).  The contract (include/mpn.h, "Class-wise candidates and NMS"):

  1. every flat index f = a*K + c with cls[b,a,c] > thr (strict; NaN fails) is a candidate, listed in ascending f;
  2. optionally only the `cap` best-scored candidates of the IMAGE enter the suppression (ties: lower f);
  3. candidates are visited in descending score (ties lower f first); a kept one suppresses a later one iff both have the same class
     and devIoU > iou (mode 0) / >= iou (mode 1);
  4. kept rows come out in descending score across classes, ties lower f first, each with box, score, class and anchor.

``reference``: np.nonzero, then oracle.nms_oracle.nms on each class's rows separately, then the union sorted by (-score, f).
``model``: what the kernels do — a chunked two-pass filter, ONE global sort, a class-equality AND in the IoU mask, one greedy scan —
with the modelled faults of MUTANTS.  Every comparison is an equality of bytes."""
import functools

import numpy as np

f32 = np.float32
THR = f32(0.05)
IOU = f32(0.5)
SENT_F = f32(-555.5)
SENT_I = -555

MUTANTS = ("suppression across classes", "arg-max candidates only", ">= at the score threshold", "class taken as (f / K) % K",
           "ties ordered class-major", "cap applied per class", "class read at the unsorted index", "chunk carry dropped")


# ---------------------------------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def chain_case():
    """Four images, A = 300 anchors, K = 5 classes: overlapping boxes, scores quantised to multiples of 1/64 (many ties, within and
    across classes), about 12 % of the (anchor, class) pairs above the threshold, 3 % exactly AT it and the rest 0.01; image 2 has
    nothing above the threshold."""
    rs = np.random.RandomState(21)
    nb, A, K = 4, 300, 5
    xy = rs.uniform(0, 70, (nb, A, 2))
    wh = rs.uniform(15, 60, (nb, A, 2))
    boxes = np.concatenate([xy, xy + wh], -1).astype(f32)
    hi = (np.ceil(rs.uniform(0.07, 1.0, (nb, A, K)) * 64) / 64).astype(f32)
    u = rs.rand(nb, A, K)
    cls = np.where(u < 0.12, hi, np.where(u < 0.15, THR, f32(0.01))).astype(f32)
    cls[2] = np.minimum(cls[2], THR)
    cls = np.ascontiguousarray(cls)
    boxes.setflags(write=False)
    cls.setflags(write=False)
    return boxes, cls, THR, IOU


@functools.lru_cache(maxsize=None)
def chunk_case(chunk):
    """Two images whose A*K spans three chunks of ``chunk`` flat indices and a partial fourth (K = 3), candidates in every chunk."""
    rs = np.random.RandomState(chunk)
    K = 3
    A = (3 * chunk + 7 * K) // K + 1
    nb = 2
    xy = rs.uniform(0, 300, (nb, A, 2))
    wh = rs.uniform(15, 60, (nb, A, 2))
    boxes = np.concatenate([xy, xy + wh], -1).astype(f32)
    hi = (np.ceil(rs.uniform(0.07, 1.0, (nb, A, K)) * 64) / 64).astype(f32)
    cls = np.where(rs.rand(nb, A, K) < 300.0 / (A * K), hi, f32(0.01)).astype(f32)
    cls = np.ascontiguousarray(cls)
    flat, hflat = cls.reshape(nb, -1), hi.reshape(nb, -1)
    for c in range(4):                                          # at least two candidates in each chunk of each image
        for d in (1, 5):
            flat[:, c * chunk + d] = hflat[:, c * chunk + d]
    boxes.setflags(write=False)
    cls.setflags(write=False)
    return boxes, cls, THR, IOU


# ---------------------------------------------------------------------------------------------- reference
def ref_candidates(boxes_b, cls_b, thr):
    """(f [n] int64 ascending, dets [n,5]) of one image from np.nonzero."""
    K = cls_b.shape[-1]
    with np.errstate(invalid="ignore"):
        f = np.nonzero(cls_b.reshape(-1) > thr)[0]
    dets = np.concatenate([boxes_b[f // K], cls_b.reshape(-1)[f][:, None]], 1).astype(f32).reshape(-1, 5)
    return f, dets


def reference(boxes, cls, thr, iou, mode=0, cap=None):
    """Per image None (no candidate) or dict(boxes [k,4], scores [k], classes [k] i64, anchors [k] i64, f [k] i64, ncand)."""
    from oracle import nms_oracle
    nb, A, K = cls.shape
    out = []
    for b in range(nb):
        f, dets = ref_candidates(boxes[b], cls[b], thr)
        n = len(f)
        if n == 0:
            out.append(None)
            continue
        live = np.arange(n)
        if cap is not None and cap > 0 and n > cap:
            live = np.sort(np.lexsort((f, -dets[:, 4].astype(np.float64)))[:cap])
        kept = []
        for c in range(K):
            rows = live[f[live] % K == c]                      # ascending f: the oracle's tie rule (lower row first) is lower f first
            if len(rows):
                kept.append(rows[nms_oracle.nms(dets[rows], float(iou), mode="gpu" if mode == 0 else "cpu")])
        kept = np.concatenate(kept)
        kept = kept[np.lexsort((f[kept], -dets[kept, 4].astype(np.float64)))]
        out.append(dict(boxes=dets[kept, :4], scores=dets[kept, 4], classes=(f[kept] % K).astype(np.int64),
                        anchors=(f[kept] // K).astype(np.int64), f=f[kept], ncand=n))
    return out


def reference_rows(dets, ccls, iou, mode=0, cap=None):
    """Steps 2 - 4 on a given candidate list (dets [n,5], ccls [n]; row order = ascending f): the kept rows, int64, in output order."""
    from oracle import nms_oracle
    n = dets.shape[0]
    if n == 0:
        return np.zeros((0,), dtype=np.int64)
    sc = dets[:, 4].astype(np.float64)
    live = np.arange(n)
    if cap is not None and cap > 0 and n > cap:
        live = np.sort(np.lexsort((np.arange(n), -sc))[:cap])
    kept = [np.zeros((0,), dtype=np.int64)]
    for c in np.unique(ccls[live]):
        rows = live[ccls[live] == c]
        kept.append(rows[nms_oracle.nms(dets[rows], float(iou), mode="gpu" if mode == 0 else "cpu")])
    kept = np.concatenate(kept)
    return kept[np.lexsort((kept, -sc[kept]))].astype(np.int64)


# ---------------------------------------------------------------------------------------------- kernel model
def model_filter(boxes_b, cls_b, thr, chunk, mut=None):
    """The two passes over one image: per-chunk counts, then each chunk writes its passing elements from the sum of the counts ahead
    of it.  -> (dets [n,5], cand_cls [n] i32, cand_anchor [n] i32, n)."""
    A, K = cls_b.shape
    flat = cls_b.reshape(-1)
    with np.errstate(invalid="ignore"):
        ok = (flat >= thr) if mut == ">= at the score threshold" else (flat > thr)
    if mut == "arg-max candidates only":
        first = np.zeros((A, K), dtype=bool)
        first[np.arange(A), np.argmax(np.where(np.isnan(cls_b), -np.inf, cls_b), 1)] = True
        ok &= first.reshape(-1)
    nchunks = (A * K + chunk - 1) // chunk
    cnt = np.array([int(ok[c * chunk:(c + 1) * chunk].sum()) for c in range(nchunks)], dtype=np.int64)
    n = int(cnt.sum())
    dets = np.full((n, 5), SENT_F, dtype=f32)
    ccls = np.full((n,), SENT_I, dtype=np.int32)
    canc = np.full((n,), SENT_I, dtype=np.int32)
    for c in range(nchunks):
        base = (int(cnt[c - 1]) if c else 0) if mut == "chunk carry dropped" else int(cnt[:c].sum())
        f = c * chunk + np.nonzero(ok[c * chunk:(c + 1) * chunk])[0]
        pos = base + np.arange(len(f))
        a = f // K
        dets[pos, :4], dets[pos, 4] = boxes_b[a], flat[f]
        ccls[pos] = (a % K) if mut == "class taken as (f / K) % K" else (f - a * K)
        canc[pos] = a
    return dets, ccls, canc, n


def dev_iou_matrix(d):
    """devIoU (nms_kernel.cu:16-24) of every row pair, each operation a separately rounded float32 one."""
    one = f32(1)
    a = d[:, None, :4]
    b = d[None, :, :4]
    w = np.maximum(np.minimum(a[..., 2], b[..., 2]) - np.maximum(a[..., 0], b[..., 0]) + one, f32(0))
    h = np.maximum(np.minimum(a[..., 3], b[..., 3]) - np.maximum(a[..., 1], b[..., 1]) + one, f32(0))
    inter = w * h
    sa = (a[..., 2] - a[..., 0] + one) * (a[..., 3] - a[..., 1] + one)
    sb = (b[..., 2] - b[..., 0] + one) * (b[..., 3] - b[..., 1] + one)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (inter / (sa + sb - inter)).astype(f32)


def model_nms(dets, ccls, iou, mode=0, cap=None, mut=None, K=None):
    """One global rank sort (descending score, ties lower row first), the cap, the IoU mask ANDed with class equality, one greedy
    scan.  -> kept rows of the candidate list, in the order of the sort."""
    n = dets.shape[0]
    sc = dets[:, 4].astype(np.float64)
    if mut == "ties ordered class-major":
        order = np.lexsort((np.arange(n), ccls, -sc))
    else:
        order = np.lexsort((np.arange(n), -sc))
    if cap is not None and cap > 0 and n > cap:
        if mut == "cap applied per class":
            seen = {}
            sel = []
            for i in order:
                seen[int(ccls[i])] = seen.get(int(ccls[i]), 0) + 1
                if seen[int(ccls[i])] <= cap:
                    sel.append(i)
            order = np.array(sel, dtype=np.int64)
        else:
            order = order[:cap]
    m = len(order)
    srt = dets[order]
    scls = ccls[np.arange(m)] if mut == "class read at the unsorted index" else ccls[order]
    ov = dev_iou_matrix(srt)
    hit = (ov > iou) if mode == 0 else (ov >= iou)
    if mut != "suppression across classes":
        hit &= scls[:, None] == scls[None, :]
    removed = np.zeros(m, dtype=bool)
    kept = []
    for i in range(m):
        if removed[i]:
            continue
        kept.append(order[i])
        removed[i + 1:] |= hit[i, i + 1:]
    return np.array(kept, dtype=np.int64)


def model(boxes, cls, thr, iou, mode=0, cap=None, chunk=16384, mut=None):
    """The kernels' chain in the form of ``reference``'s result (without 'f')."""
    nb, A, K = cls.shape
    out = []
    for b in range(nb):
        dets, ccls, canc, n = model_filter(boxes[b], cls[b], thr, chunk, mut)
        if n == 0:
            out.append(None)
            continue
        kept = model_nms(dets, ccls, iou, mode, cap, mut)
        out.append(dict(boxes=dets[kept, :4], scores=dets[kept, 4], classes=ccls[kept].astype(np.int64), anchors=canc[kept].astype(np.int64),
                        ncand=n))
    return out


def same(got, want):
    """True when two per-image result lists are equal byte for byte (boxes, scores, classes, anchors, candidate counts)."""
    if len(got) != len(want):
        return False
    for g, w in zip(got, want):
        if (g is None) != (w is None):
            return False
        if g is None:
            continue
        if g["ncand"] != w["ncand"] or g["scores"].shape != w["scores"].shape:
            return False
        if not (np.array_equal(g["boxes"].view(np.uint32), w["boxes"].view(np.uint32)) and
                np.array_equal(g["scores"].view(np.uint32), w["scores"].view(np.uint32)) and
                np.array_equal(g["classes"], w["classes"]) and np.array_equal(g["anchors"], w["anchors"])):
            return False
    return True


@functools.lru_cache(maxsize=None)
def chain_reference(mode=0, cap=None):
    """``reference`` on chain_case(), computed once."""
    boxes, cls, thr, iou = chain_case()
    return reference(boxes, cls, thr, iou, mode, cap)
