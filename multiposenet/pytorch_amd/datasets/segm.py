"""COCO ``segmentation`` fields rasterised on the GPU: ``annToMask`` without pycocotools (csrc/segm.hip).

The rule is COCO's maskApi.c: ``rleFrPoly`` (the polygon outline walked on a 5x grid, its crossings of the pixel columns turned into
toggles on the column-major flat index), ``rleMerge`` as a union of an annotation's parts, ``rleDecode`` and ``rleFrString`` for crowds.

The host side here is O(vertices): :func:`pack_segmentations` upsamples the vertices, counts the steps of every edge and gives
every instance a rectangle that is certain to contain its ON cells; no pixel is touched.  The device side flips one bit per
crossing (mpn_segm_rasterize's toggle launch) and turns the bits into uint8 cells by prefix parity (its fill launch), either as the
packed rectangles ``mpn_augment_boxes`` reads (:func:`rasterize_packed`) or as dense masks (:func:`rasterize_segmentations`).

``mask_miss`` — the uint8 [H, W] image that takes unlabelled people and crowds out of the heat-map loss, which the reference reads
as a PNG written by a MATLAB step (``COCO_data_pipeline.py:244-250``) — comes from the same toggle launch and ONE compose launch
(mpn_segm_mask_miss) over an image's person annotations in json order, with ``M_p`` the ``annToMask`` of annotation ``p``::

    all = 0; miss = 0
    for p in order:
        if iscrowd(p):            miss |= M_p & ~all          # "all" as accumulated SO FAR, not the final union
        else:                     all  |= M_p
                                  if num_keypoints(p) <= 0: miss |= M_p
    mask_miss = 255 where miss == 0, else 0

With at most one crowd per image this is what the known scripts compute; they refuse, or leave undefined, more than one crowd, and
here every crowd contributes as above.  No instance mask is ever in memory (:func:`mask_miss_batch`).

``mask_all`` — the target of the keypoint subnet's person-segmentation channel, which the reference would have read from the same
MATLAB step — is the plain union: 255 where ANY person annotation (with keypoints, without, or a crowd) covers the pixel, else 0;
independent of the order, all 0 for an empty list.  The compose launch's second instantiation (mpn_segm_person_masks) writes both
planes from the registers it holds (:func:`person_masks_batch`).
"""
import math

import numpy as np
import torch

from .._lib import MpnError, call
from .. import ops

SCALE = 5.0
MAX_COORD = float(1 << 20)                  # |x|, |y| of a vertex: far beyond any image, keeps (int)(5 x + 0.5) and the step counts small
MAX_INSTANCES = 65535

# columns of the int64 instance table and of the int64 part table (include/mpn.h: MPN_SEGI_*, MPN_SEGP_*)
I_H, I_W, I_RX0, I_RY0, I_RW, I_RH, I_OUT_OFF, I_OUT_PITCH, I_P0, I_P1, I_COLS = range(11)
P_INST, P_V0, P_V1, P_BM, P_COLS = range(5)
# columns of mpn_segm_mask_miss's int64 image table (MPN_SEGM_*) and the kinds of a person annotation (MPN_SEGK_*)
M_H, M_W, M_I0, M_I1, M_OUT_OFF, M_OUT_PITCH, M_COLS = range(7)
KIND_KEYPOINTS, KIND_NO_KEYPOINTS, KIND_CROWD = 0, 1, 2


def string_counts(s):
    """The compressed ``counts`` of an RLE (str or bytes) -> list of run lengths.  Each run length is a group of characters read as
    ``c - 48``: five data bits each (low group first), 0x20 = the group continues, the last character's 0x10 sign-extends; from the
    fourth count on the value is a difference to the count two places back."""
    if isinstance(s, str):
        try:
            s = s.encode("ascii")
        except UnicodeEncodeError:
            raise MpnError("compressed RLE counts must be ASCII")
    counts, p, n = [], 0, len(s)
    while p < n:
        x, k = 0, 0
        while True:
            if p >= n:
                raise MpnError("compressed RLE counts end inside a group")
            c = s[p] - 48
            if c < 0 or c > 63 or k > 12:
                raise MpnError("compressed RLE counts hold a character outside '0'..'o' or an overlong group")
            x |= (c & 0x1f) << (5 * k)
            p += 1
            k += 1
            if not c & 0x20:
                if c & 0x10:
                    x |= -1 << (5 * k)
                break
        if len(counts) > 2:
            x += counts[-2]
        counts.append(x)
    return counts


class SegmPack(object):
    """The tables mpn_segm_rasterize reads for ``n`` instances, as numpy arrays on the host:

    ``insts`` int64 [n, 10] (H, W, the rectangle rx0, ry0, rw, rh, byte offset and row pitch of its output, its parts [p0, p1));
    ``parts`` int64 [P, 4] (instance, its vertices [v0, v1), word offset of its toggle bitmap in the workspace) — an RLE instance
    has one part without vertices; ``verts`` int32 [V, 2] the upsampled vertices (edge e runs from vertex e to the next of its part,
    the last one back to the first); ``vpart`` int32 [V] the part of each; ``estart`` int32 [V + 1] the prefix table of per-edge step
    counts max(|dX|, |dY|); ``toggles`` int32 [T, 2] (part, flat index) of the RLE instances; ``words`` the bitmap words in all."""

    def __init__(self, insts, parts, verts, vpart, estart, toggles, words):
        self.insts, self.parts, self.verts, self.vpart, self.estart, self.toggles, self.words = insts, parts, verts, vpart, estart, toggles, words

    @property
    def n(self):
        return int(self.insts.shape[0])

    def rects(self):
        """[(rx0, ry0, rw, rh)] per instance."""
        return [tuple(int(v) for v in r[I_RX0:I_RH + 1]) for r in self.insts]

    def packed_layout(self):
        """Row-major rectangles, each starting on a 16-byte boundary in instance order (the layout of boxes_from_rects) -> bytes."""
        size = self.insts[:, I_RW] * self.insts[:, I_RH]
        step = (size + 15) // 16 * 16
        self.insts[:, I_OUT_OFF] = np.cumsum(step) - step
        self.insts[:, I_OUT_PITCH] = self.insts[:, I_RW]
        return int(step.sum())

    def dense_layout(self):
        """Rectangle i inside plane i of a [n, H, W] tensor (every instance must have one H, W) -> bytes."""
        H, W = int(self.insts[0, I_H]), int(self.insts[0, I_W])
        if np.any(self.insts[:, I_H] != H) or np.any(self.insts[:, I_W] != W):
            raise MpnError("a dense layout needs one image size")
        self.insts[:, I_OUT_OFF] = np.arange(self.n, dtype=np.int64) * (H * W) + self.insts[:, I_RY0] * W + self.insts[:, I_RX0]
        self.insts[:, I_OUT_PITCH] = W
        return self.n * H * W


def _numbers(seq, what):
    try:
        a = np.asarray(seq, dtype=np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise MpnError("%s must be a flat list of numbers" % what)
    if not np.all(np.isfinite(a)):
        raise MpnError("%s holds a number that is not finite" % what)
    return a


def _rle_toggles(segm, H, W):
    """RLE dict -> (toggles below H * W with the cancelled pairs still in, rectangle)."""
    size = segm.get("size")
    if size is None or [int(v) for v in size] != [H, W]:
        raise MpnError("the RLE size %s is not the image's [%d, %d]" % (size, H, W))
    counts = segm.get("counts")
    if isinstance(counts, (str, bytes)):
        counts = string_counts(counts)
    c = _numbers(counts, "RLE counts")
    if c.size == 0 or np.any(c < 0) or np.any(c != np.floor(c)) or c.sum() != H * W:
        raise MpnError("RLE counts must be non-negative integers that sum to H * W")
    ends = np.cumsum(c.astype(np.int64))
    on = np.flatnonzero(c[1::2] > 0) * 2 + 1                              # the ON runs that are not empty
    if on.size == 0:
        return np.zeros(0, dtype=np.int64), (0, 0, 1, 1)
    c0, c1 = int(ends[on[0] - 1]) // H, (int(ends[on[-1]]) - 1) // H       # columns of the first and of the last ON cell
    return ends[ends < H * W], (c0, 0, c1 - c0 + 1, H)


def pack_segmentations(segms, H, W, strict=True):
    """The ``segmentation`` fields of ``n`` annotations of one H x W image -> :class:`SegmPack` (packed-rectangle layout).

    A segmentation is a list of polygon parts ``[x0, y0, x1, y1, ...]`` (their union is the instance), an uncompressed RLE dict
    ``{"size": [H, W], "counts": [...]}`` or a compressed one (``counts`` a str or bytes).  MpnError for an RLE of another size, counts
    that do not sum to H * W, a number that is not finite, a vertex beyond +-2^20, and for a part with an odd length or fewer than 6
    numbers.  With ``strict=False`` such a part is DROPPED instead (an instance that loses every part rasterises empty).  pycocotools
    would read a 4-number list as a box; that is not reproduced.

    The rectangle of an instance contains its ON cells and need not be tight: for polygons the vertex extents widened by one pixel
    and clipped to the image, for an RLE the columns from the first ON run to the last at full height; an instance that cannot
    have an ON cell gets the cell (0, 0)."""
    H, W = int(H), int(W)
    if not (1 <= H <= 65536 and 1 <= W <= 65536 and H * W < 2 ** 31):
        raise MpnError("H and W must lie in 1..65536 with H * W < 2^31")
    if len(segms) > MAX_INSTANCES:
        raise MpnError("at most %d instances" % MAX_INSTANCES)
    cw = H // 64 + 1                                                      # 64-bit words of a column's H + 1 toggle slots
    insts = np.zeros((len(segms), I_COLS), dtype=np.int64)
    parts, verts, vpart, steps, toggles, words = [], [], [], [], [], 0
    for i, segm in enumerate(segms):
        p0 = len(parts)
        if isinstance(segm, dict):
            tg, rect = _rle_toggles(segm, H, W)
            toggles.append(np.stack([np.full(tg.size, p0, dtype=np.int64), tg], axis=1))
            parts.append([i, 0, 0, 0])
        else:
            if isinstance(segm, (str, bytes)) or not hasattr(segm, "__len__"):
                raise MpnError("a segmentation must be a list of polygon parts or an RLE dict")
            lo, hi = np.full(2, np.inf), np.full(2, -np.inf)
            for part in segm:
                xy = _numbers(part, "a polygon part")
                if xy.size % 2 or xy.size < 6:
                    if strict:
                        raise MpnError("a polygon part needs an even count of at least 6 numbers, got %d" % xy.size)
                    continue
                if np.any(np.abs(xy) > MAX_COORD):
                    raise MpnError("a vertex lies beyond +-2^20")
                xy = xy.reshape(-1, 2)
                up = np.trunc(SCALE * xy + 0.5).astype(np.int64)             # (int)(5 x + 0.5), one rounding per operation
                d = np.abs(np.roll(up, -1, axis=0) - up)
                v0 = sum(v.shape[0] for v in verts)
                verts.append(up)
                vpart.append(np.full(up.shape[0], len(parts), dtype=np.int64))
                steps.append(np.maximum(d[:, 0], d[:, 1]))
                parts.append([i, v0, v0 + up.shape[0], 0])
                lo, hi = np.minimum(lo, xy.min(axis=0)), np.maximum(hi, xy.max(axis=0))
            x0, y0 = max(int(math.floor(lo[0])) - 1, 0) if lo[0] < np.inf else 0, max(int(math.floor(lo[1])) - 1, 0) if lo[1] < np.inf else 0
            x1, y1 = min(int(math.ceil(hi[0])) + 1, W - 1) if hi[0] > -np.inf else -1, min(int(math.ceil(hi[1])) + 1, H - 1) if hi[1] > -np.inf else -1
            rect = (x0, y0, x1 - x0 + 1, y1 - y0 + 1) if x1 >= x0 and y1 >= y0 else (0, 0, 1, 1)
        for p in parts[p0:]:
            p[P_BM] = words
            words += cw * rect[2]
        insts[i] = (H, W) + rect + (0, 0, p0, len(parts))
    nv = sum(v.shape[0] for v in verts)
    estart = np.zeros(nv + 1, dtype=np.int64)
    if nv:
        np.cumsum(np.concatenate(steps), out=estart[1:])
    if estart[-1] >= 2 ** 31 or words >= 2 ** 31:
        raise MpnError("the outlines are too long for one launch")
    pack = SegmPack(insts,
                    np.asarray(parts, dtype=np.int64).reshape(-1, P_COLS),
                    (np.concatenate(verts) if nv else np.zeros((0, 2))).astype(np.int32),
                    (np.concatenate(vpart) if nv else np.zeros(0)).astype(np.int32),
                    estart.astype(np.int32),
                    (np.concatenate(toggles) if toggles else np.zeros((0, 2))).astype(np.int32),
                    int(words))
    pack.packed_layout()
    return pack


def concat_packs(packs):
    """The packs of a batch's samples as one (instances in order, packed-rectangle layout)."""
    ni = npt = nv = nw = 0
    insts, parts, verts, vpart, steps, toggles = [], [], [], [], [], []
    for k in packs:
        i, p = k.insts.copy(), k.parts.copy()
        i[:, I_P0:I_P1 + 1] += npt
        p[:, P_INST] += ni
        p[:, P_V0:P_V1 + 1] += nv
        p[:, P_BM] += nw
        t = k.toggles.astype(np.int64)
        t[:, 0] += npt
        insts.append(i); parts.append(p); verts.append(k.verts); vpart.append(k.vpart.astype(np.int64) + npt)
        steps.append(np.diff(k.estart.astype(np.int64))); toggles.append(t)
        ni, npt, nv, nw = ni + k.n, npt + p.shape[0], nv + k.verts.shape[0], nw + k.words
    estart = np.zeros(nv + 1, dtype=np.int64)
    np.cumsum(np.concatenate(steps), out=estart[1:])
    if ni > MAX_INSTANCES or estart[-1] >= 2 ** 31 or nw >= 2 ** 31:
        raise MpnError("too many instances or too long outlines for one launch")
    pack = SegmPack(np.concatenate(insts), np.concatenate(parts), np.concatenate(verts), np.concatenate(vpart).astype(np.int32),
                    estart.astype(np.int32), np.concatenate(toggles).astype(np.int32), nw)
    pack.packed_layout()
    return pack


def _upload(pack, dev, extra=()):
    """Every table (and the arrays of ``extra`` after them) in ONE pinned block and one H2D copy, each starting on an 8-byte
    boundary -> (device views, bytes uploaded)."""
    arrs = [pack.insts, pack.parts, pack.verts, pack.vpart, pack.estart, pack.toggles] + list(extra)
    sizes = [(a.nbytes + 7) // 8 * 8 for a in arrs]
    stage = torch.empty(max(sum(sizes), 8), dtype=torch.uint8, pin_memory=True)
    off, offs = 0, []
    for a, s in zip(arrs, sizes):
        if a.nbytes:
            stage[off: off + a.nbytes] = torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8))
        offs.append(off)
        off += s
    d = stage.to(dev, non_blocking=True)
    return [d[o: o + max(a.nbytes, 0)] for o, a in zip(offs, arrs)], stage.numel()


def _rasterize(pack, out_bytes, dense, dev):
    """mpn_segm_rasterize on an uploaded pack -> (uint8 [out_bytes], int32 [n] 'any cell ON', bytes uploaded)."""
    n = pack.n
    out = torch.empty(max(out_bytes, 16), dtype=torch.uint8, device=dev)
    anyon = torch.empty(n, dtype=torch.int32, device=dev)
    (insts, parts, verts, vpart, estart, toggles), h2d = _upload(pack, dev)
    ws_bytes = int(call("mpn_segm_workspace_bytes", pack.words))
    if ws_bytes <= 0:
        raise MpnError("mpn_segm_workspace_bytes refused %d words" % pack.words)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    nv, nt = int(pack.verts.shape[0]), int(pack.toggles.shape[0])
    call("mpn_segm_rasterize", ops.ptr(insts), n, ops.ptr(parts), int(pack.parts.shape[0]),
         ops.ptr(verts) if nv else None, ops.ptr(vpart) if nv else None, ops.ptr(estart), nv, int(pack.estart[-1]),
         ops.ptr(toggles) if nt else None, nt, int(pack.insts[:, I_RW].max()), int(pack.insts[:, I_H].max()),
         ops.ptr(out), out.numel(), 1 if dense else 0, ops.ptr(anyon), ops.ptr(ws), ws_bytes, ops.stream_ptr())
    return out, anyon, h2d


def rasterize_packed(pack, dev=None):
    """The instances of ``pack`` as row-major uint8 rectangles at 16-byte-aligned offsets, as mpn_augment_boxes reads them
    -> (uint8 device buffer, int32 [n] 'any cell ON' on the device, bytes uploaded).  Nothing waits for the device."""
    dev = _device() if dev is None else dev
    if pack.n == 0:
        raise MpnError("nothing to rasterise")
    return _rasterize(pack, pack.packed_layout(), False, dev)


def rasterize_segmentations(segms, H, W, strict=True):
    """``annToMask`` of a list of annotations' ``segmentation`` fields on one H x W image -> uint8 [n, H, W] on the device."""
    dev = _device()
    pack = pack_segmentations(segms, H, W, strict)
    if pack.n == 0:
        return torch.zeros((0, int(H), int(W)), dtype=torch.uint8, device=dev)
    out, _, _ = _rasterize(pack, pack.dense_layout(), True, dev)
    return out[:pack.n * int(H) * int(W)].view(pack.n, int(H), int(W))


def annotation_kind(ann):
    """KIND_CROWD if ``iscrowd`` is truthy (whatever its ``num_keypoints``), KIND_NO_KEYPOINTS if ``num_keypoints <= 0``, else
    KIND_KEYPOINTS.  Without ``num_keypoints`` it is the count of ``v > 0`` entries of ``keypoints``; MpnError without both."""
    if ann.get("iscrowd"):
        return KIND_CROWD
    n = ann.get("num_keypoints")
    if n is None:
        kp = ann.get("keypoints")
        if kp is None:
            raise MpnError("a person annotation needs 'num_keypoints' or 'keypoints'")
        n = int(np.count_nonzero(_numbers(kp, "keypoints")[2::3] > 0))
    return KIND_NO_KEYPOINTS if n <= 0 else KIND_KEYPOINTS


def pack_mask_miss(anns, H, W, strict=True, keep_all=False):
    """The person annotations of one H x W image, in json order -> (:class:`SegmPack`, ``kinds`` int32 [n]) for mpn_segm_mask_miss.

    A KIND_KEYPOINTS annotation after the image's last crowd cannot change the result (``all`` is read by crowds only) and is
    dropped here, before anything is uploaded: most COCO images have no crowd, so only their KIND_NO_KEYPOINTS annotations get
    rasterised.  ``keep_all`` (the two-plane form, mpn_segm_person_masks) drops nothing: everyone is part of ``mask_all``.
    Refusals: those of :func:`pack_segmentations`, an annotation without ``segmentation``, and the one of
    :func:`annotation_kind`."""
    kinds = [annotation_kind(a) for a in anns]
    last_crowd = max([i for i, k in enumerate(kinds) if k == KIND_CROWD] or [-1])
    keep = [i for i, k in enumerate(kinds) if keep_all or k != KIND_KEYPOINTS or i < last_crowd]
    segms = []
    for i in keep:
        if anns[i].get("segmentation") is None:
            raise MpnError("a person annotation needs a 'segmentation'")
        segms.append(anns[i]["segmentation"])
    return pack_segmentations(segms, H, W, strict), np.asarray([kinds[i] for i in keep], dtype=np.int32)


def pack_mask_miss_batch(list_of_anns, sizes, offsets=None, strict=True, keep_all=False):
    """The host side of :func:`mask_miss_batch`: the images' packs as one, their kinds, and the int64 image table [B, 6] (H, W, the
    image's instances [i0, i1), byte offset of its plane, row pitch W) -> (pack, kinds, imgs, offsets, bytes of the output).
    ``keep_all``: as for :func:`pack_mask_miss` (the host side of :func:`person_masks_batch`)."""
    if len(list_of_anns) == 0 or len(list_of_anns) != len(sizes) or len(sizes) > MAX_INSTANCES:
        raise MpnError("a batch needs 1..%d images and one (H, W) for each" % MAX_INSTANCES)
    sizes = [(int(H), int(W)) for H, W in sizes]
    packed = [pack_mask_miss(anns, H, W, strict, keep_all) for anns, (H, W) in zip(list_of_anns, sizes)]
    if offsets is None:
        from .augment import _aligned_offsets
        offsets = _aligned_offsets([H * W for H, W in sizes])[0]
    offsets = [int(o) for o in offsets]
    if len(offsets) != len(sizes) or min(offsets) < 0:
        raise MpnError("one non-negative byte offset per image")
    imgs = np.zeros((len(sizes), M_COLS), dtype=np.int64)
    i0 = 0
    for b, ((H, W), (pk, _), off) in enumerate(zip(sizes, packed, offsets)):
        imgs[b] = (H, W, i0, i0 + pk.n, off, W)
        i0 += pk.n
    nbytes = max(off + H * W for (H, W), off in zip(sizes, offsets))
    return concat_packs([pk for pk, _ in packed]), np.concatenate([k for _, k in packed]), imgs, offsets, nbytes


def _compose(list_of_anns, sizes, offsets, strict, dev, two):
    """The device side of :func:`mask_miss_batch` (``two`` False) and :func:`person_masks_batch` (True): one pinned upload, the
    toggle launches and one compose launch -> ([plane buffers], offsets)."""
    dev = _device() if dev is None else dev
    pack, kinds, imgs, offsets, nbytes = pack_mask_miss_batch(list_of_anns, sizes, offsets, strict, keep_all=two)
    outs = [torch.empty(max((nbytes + 15) // 16 * 16, 16), dtype=torch.uint8, device=dev) for _ in range(2 if two else 1)]
    (insts, parts, verts, vpart, estart, toggles, d_imgs, d_kinds), _ = _upload(pack, dev, (imgs, kinds))
    ws_bytes = int(call("mpn_segm_workspace_bytes", pack.words))
    if ws_bytes <= 0:
        raise MpnError("mpn_segm_workspace_bytes refused %d words" % pack.words)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    n, npt, nv, nt = pack.n, int(pack.parts.shape[0]), int(pack.verts.shape[0]), int(pack.toggles.shape[0])
    call("mpn_segm_person_masks" if two else "mpn_segm_mask_miss",
         ops.ptr(d_imgs), int(imgs.shape[0]), ops.ptr(insts) if n else None, ops.ptr(d_kinds) if n else None, n,
         ops.ptr(parts) if npt else None, npt, ops.ptr(verts) if nv else None, ops.ptr(vpart) if nv else None, ops.ptr(estart), nv,
         int(pack.estart[-1]), ops.ptr(toggles) if nt else None, nt, int(imgs[:, M_W].max()), int(imgs[:, M_H].max()),
         *([ops.ptr(o) for o in outs] + [outs[0].numel(), ops.ptr(ws), ws_bytes, ops.stream_ptr()]))
    return outs, offsets


def mask_miss_batch(list_of_anns, sizes, offsets=None, strict=True, dev=None):
    """``mask_miss`` of every image of a batch (``list_of_anns[b]`` the person annotations of image ``b`` in json order, an empty
    list allowed; ``sizes[b]`` its (H, W)) -> (uint8 device buffer, byte offsets): image ``b`` is the row-major H x W plane at
    ``offsets[b]`` (default: consecutive planes, each starting on a 16-byte boundary, the layout ``mpn_augment_mask`` reads); the
    bytes between planes hold nothing.  One pinned upload and two launches for the whole batch; nothing waits for the device."""
    outs, offsets = _compose(list_of_anns, sizes, offsets, strict, dev, False)
    return outs[0], offsets


def person_masks_batch(list_of_anns, sizes, offsets=None, strict=True, dev=None):
    """``mask_miss`` AND ``mask_all`` of every image of a batch, arguments as for :func:`mask_miss_batch`
    -> (miss buffer, all buffer, byte offsets): two uint8 device buffers with image ``b``'s planes at ``offsets[b]`` of both.

    ``mask_all`` is the target of the keypoint subnet's person-segmentation channel: 255 where ANY of the image's person
    annotations covers the pixel — people with keypoints, people without, crowds — else 0; a plain union, independent of the
    order; all 0 for an empty list.  Both planes leave the ONE compose launch (mpn_segm_person_masks) from the registers it
    holds, so every annotation is packed here: the dropping rule of :func:`pack_mask_miss` does not apply.  The ``mask_miss``
    bytes are those of :func:`mask_miss_batch`."""
    outs, offsets = _compose(list_of_anns, sizes, offsets, strict, dev, True)
    return outs[0], outs[1], offsets


def mask_miss_from_annotations(anns, H, W):
    """``mask_miss`` of one H x W image from its person annotations in json order -> uint8 [H, W] on the device."""
    out, _ = mask_miss_batch([anns], [(H, W)])
    return out[:int(H) * int(W)].view(int(H), int(W))


def mask_all_from_annotations(anns, H, W):
    """``mask_all`` of one H x W image from its person annotations -> uint8 [H, W] on the device (:func:`person_masks_batch`)."""
    _, out, _ = person_masks_batch([anns], [(H, W)])
    return out[:int(H) * int(W)].view(int(H), int(W))


def _device():
    if not torch.cuda.is_available():
        raise MpnError("segmentations are rasterised on the MI355X only; there is no CPU path")
    return torch.device("cuda", torch.cuda.current_device())
