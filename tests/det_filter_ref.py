"""Inputs, references, comparisons and numpy models for the detection score filter and the gathers around NMS (csrc/nms.hip:
score_filter_kernel, gather_dets_kernel, gather_class_kernel).  The references are numpy boolean masks and fancy indexing; every
comparison is an equality of bytes.  The ``check_*`` functions serve the GPU tier (kernels) and the CPU tier (models and mutants)."""
import functools

import numpy as np

f32 = np.float32
SENT_F = f32(-555.5)
SENT_I = -555
A_SIZES = (1, 63, 64, 65, 1023, 1024, 1025, 2500)
B = 3
THR = f32(0.05)
CASES = ("mixed", "all", "none", "equal to the threshold", "nan", "last partial wave", "beyond 1024")


@functools.lru_cache(maxsize=None)
def filter_case(A, name):
    """boxes [3,A,4], scores [3,A] float32 and the threshold.  'mixed': about 50 % / 5 % / 90 % of the candidates pass in the three
    images; 'equal to the threshold' / 'nan': a third of the scores are exactly THR / NaN (neither passes), the rest mixed;
    'last partial wave': only indices of the last, partial 64-lane wave pass; 'beyond 1024': only indices >= 1024."""
    rs = np.random.RandomState(A * 7 + CASES.index(name))
    boxes = rs.uniform(0, 500, (B, A, 4)).astype(f32)
    lo = rs.uniform(0.0, 0.049, (B, A)).astype(f32)
    hi = rs.uniform(0.051, 1.0, (B, A)).astype(f32)
    frac = np.array([0.5, 0.05, 0.9])[:, None]
    mixed = np.where(rs.rand(B, A) < frac, hi, lo)
    idx = np.arange(A)[None, :]
    if name == "mixed":
        s = mixed
    elif name == "all":
        s = hi
    elif name == "none":
        s = lo
    elif name == "equal to the threshold":
        s = np.where(rs.rand(B, A) < 0.34, THR, mixed)
        s[:, 0] = THR
    elif name == "nan":
        s = np.where(rs.rand(B, A) < 0.34, f32(np.nan), mixed)
        s[:, A - 1] = np.nan
    elif name == "last partial wave":
        s = np.where(idx >= (A - 1) // 64 * 64, np.where(rs.rand(B, A) < 0.7, hi, lo), lo)
        s[:, A - 1] = hi[:, A - 1]
    elif name == "beyond 1024":
        s = np.where(idx >= 1024, np.where(rs.rand(B, A) < 0.6, hi, lo), lo)
        s[:, A - 1] = hi[:, A - 1]
    s = np.ascontiguousarray(s, dtype=f32)
    boxes.setflags(write=False)
    s.setflags(write=False)
    return boxes, s, THR


def ref_filter(boxes, scores, thr):
    """counts [B] int32, dets [B,A,5] and src [B,A] (sentinels at and beyond the count) from np.nonzero(scores > thr)."""
    nb, A = scores.shape
    counts = np.zeros(nb, dtype=np.int32)
    dets = np.full((nb, A, 5), SENT_F, dtype=f32)
    src = np.full((nb, A), SENT_I, dtype=np.int32)
    with np.errstate(invalid="ignore"):
        for b in range(nb):
            i = np.nonzero(scores[b] > thr)[0]
            counts[b] = len(i)
            dets[b, :len(i), :4] = boxes[b, i]
            dets[b, :len(i), 4] = scores[b, i]
            src[b, :len(i)] = i
    return counts, dets, src


def check_filter(ref, counts, dets, src=None):
    rc, rd, rsrc = ref
    assert np.array_equal(counts, rc), "counts %s, expected %s" % (counts.tolist(), rc.tolist())
    assert dets.dtype == f32 and np.array_equal(dets.view(np.uint32), rd.view(np.uint32)), \
        "dets (or a row that should keep its sentinel) differs at (image, row) %s" % np.argwhere((dets.view(np.uint32) != rd.view(np.uint32)).any(-1))[:4].tolist()
    if src is not None:
        assert np.array_equal(src, rsrc), "src differs at %s" % np.argwhere(src != rsrc)[:4].tolist()
    return int(rc.sum())


def model_filter(boxes, scores, thr, mut=None):
    """score_filter_kernel: 1024 lanes in 16 waves per chunk, ballot + prefix inside a wave, wave offsets, carry between chunks."""
    nb, A = scores.shape
    counts = np.zeros(nb, dtype=np.int32)
    dets = np.full((nb, A, 5), SENT_F, dtype=f32)
    src = np.full((nb, A), SENT_I, dtype=np.int32)
    with np.errstate(invalid="ignore"):
        for b in range(nb):
            base = 0
            for a0 in range(0, A, 1024):
                a = a0 + np.arange(1024)
                ok = a < A
                sc = np.where(ok, scores[b, np.minimum(a, A - 1)], f32(0))
                passed = ok & ((sc >= thr) if mut == ">=" else (sc > thr))
                wave_cnt = passed.reshape(16, 64).sum(1)
                for wv in range(16):
                    off = base + (wave_cnt[1:wv + 1].sum() if mut == "wrong waves" else wave_cnt[:wv].sum())
                    lanes = np.nonzero(passed[wv * 64:(wv + 1) * 64])[0]
                    for k, lane in enumerate(lanes):
                        i = a0 + wv * 64 + lane
                        pos = int(off + k)
                        if pos < A:
                            dets[b, pos, :4], dets[b, pos, 4] = boxes[b, i], scores[b, i]
                            src[b, pos] = i - a0 if mut == "src chunk base" else i
                if mut == "no carry":
                    base = int(wave_cnt.sum())
                else:
                    base += int(wave_cnt.sum())
            counts[b] = base
    return counts, dets, src


# ---------------------------------------------------------------------------------------------- gathers
KMAX = (1, 255, 256, 257)


@functools.lru_cache(maxsize=None)
def gather_case(kmax):
    """Four images with num = (0, 1, kmax - 1, kmax); candidate blocks of A = kmax + 40 rows, dets_stride and keep_stride and
    out_stride all larger than they need to be; keep = distinct candidate rows in random order; src = a random permutation."""
    rs = np.random.RandomState(kmax)
    nb, A = 4, kmax + 40
    c = dict(nb=nb, A=A, kmax=kmax, dets_stride=A * 5 + 15, keep_stride=kmax + 3, out_stride=kmax + 7,
             num=np.array([0, 1, kmax - 1, kmax], dtype=np.int64))
    c["dets"] = rs.uniform(-10, 500, (nb, c["dets_stride"])).astype(f32)
    c["keep"] = np.stack([np.concatenate([rs.permutation(A)[:kmax], rs.randint(0, A, 3)]) for _ in range(nb)]).astype(np.int64)
    c["src"] = np.stack([rs.permutation(A) for _ in range(nb)]).astype(np.int32)
    c["cls_id"] = rs.randint(1, 80, (nb, A)).astype(np.int64)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def ref_gather(c):
    """boxes [nb,out_stride,4], scores [nb,out_stride], classes [nb,out_stride] int64 with sentinels wherever nothing is written."""
    nb, os_ = c["nb"], c["out_stride"]
    boxes = np.full((nb, os_, 4), SENT_F, dtype=f32)
    scores = np.full((nb, os_), SENT_F, dtype=f32)
    cls = np.full((nb, os_), SENT_I, dtype=np.int64)
    for b in range(nb):
        n = int(c["num"][b])
        rows = c["dets"][b, :c["A"] * 5].reshape(c["A"], 5)[c["keep"][b, :n]]
        boxes[b, :n], scores[b, :n] = rows[:, :4], rows[:, 4]
        cls[b, :n] = c["cls_id"][b, c["src"][b, c["keep"][b, :n]]]
        cls[b, n:c["kmax"]] = 0
    return boxes, scores, cls


def check_gather(ref, boxes, scores, cls=None):
    rb, rs_, rc = ref
    assert np.array_equal(boxes.view(np.uint32), rb.view(np.uint32)), "boxes differ at (image, row) %s" % np.argwhere((boxes != rb).any(-1))[:4].tolist()
    assert np.array_equal(scores.view(np.uint32), rs_.view(np.uint32)), "scores differ at %s" % np.argwhere(scores != rs_)[:4].tolist()
    if cls is not None:
        assert cls.dtype == np.int64 and np.array_equal(cls, rc), "class ids differ at %s" % np.argwhere(cls != rc)[:4].tolist()
    return int(rb.shape[0] * rb.shape[1])


def model_gather(c, mut=None):
    """gather_dets_kernel and gather_class_kernel, thread by thread."""
    nb, os_ = c["nb"], c["out_stride"]
    boxes = np.full((nb * os_ * 4,), SENT_F, dtype=f32)
    scores = np.full((nb * os_,), SENT_F, dtype=f32)
    cls = np.full((nb * os_,), SENT_I, dtype=np.int64)
    dets, keep = c["dets"].reshape(-1), c["keep"].reshape(-1)
    for b in range(nb):
        k = int(c["num"][b])
        for i in range((c["kmax"] + 255) // 256 * 256):
            if i < k:
                s = b * c["dets_stride"] + int(keep[b * c["keep_stride"] + i]) * 5
                boxes[(b * os_ + i) * 4:(b * os_ + i) * 4 + 4] = dets[s:s + 4]
                scores[b * os_ + i] = dets[s + 4]
            if i >= c["kmax"] or (mut == "class padding unwritten" and i >= k):
                continue
            cls[b * os_ + i] = c["cls_id"][b, c["src"][b, keep[b * c["keep_stride"] + i]]] if i < k else 0
    return boxes.reshape(nb, os_, 4), scores.reshape(nb, os_), cls.reshape(nb, os_)


# ---------------------------------------------------------------------------------------------- the chain
@functools.lru_cache(maxsize=None)
def chain_case():
    """Four images of 700 overlapping candidate boxes with distinct scores; image 2 has no score above the threshold."""
    rs = np.random.RandomState(21)
    nb, A = 4, 700
    xy = rs.uniform(0, 160, (nb, A, 2))
    wh = rs.uniform(15, 60, (nb, A, 2))
    boxes = np.concatenate([xy, xy + wh], -1).astype(f32)
    scores = np.stack([rs.permutation(A) for _ in range(nb)]).astype(f32) / f32(A) * np.array([1.0, 0.4, 0.04, 0.15], dtype=f32)[:, None]
    scores = np.ascontiguousarray(scores, dtype=f32)
    cls_id = rs.randint(0, 80, (nb, A)).astype(np.int64)
    return boxes, scores, cls_id, THR, f32(0.5)


def ref_chain(boxes, scores, cls_id, thr, iou):
    """numpy filter -> oracle NMS -> numpy gather: per image (boxes [k,4], scores [k], classes [k]) or None without candidates."""
    from oracle import nms_oracle
    counts, dets, src = ref_filter(boxes, scores, thr)
    res = []
    for b in range(scores.shape[0]):
        n = int(counts[b])
        if n == 0:
            res.append(None)
            continue
        keep = nms_oracle.nms(dets[b, :n], float(iou), mode="gpu")
        res.append((dets[b, keep, :4], dets[b, keep, 4], cls_id[b, src[b, keep]]))
    return res, counts
