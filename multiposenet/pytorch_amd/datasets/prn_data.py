"""PRN training batches on the GPU, from raw COCO annotations.

Device replacement for the reference's ``PRN_CocoDataset`` (``datasets/coco_data/prn_data_pipeline.py:10-123``), whose
``get_data`` builds every ``(input, label)`` pair on the host: a Python triple loop over people x joints, 17 skimage gaussians and
one multichannel gaussian per sample.

* :class:`PRNSampleSet` holds the ``annotations`` list of a ``person_keypoints_*.json`` as flat arrays: the samples in
  ``get_anns`` order (:113-123), every image's annotations in file order, and the samples for which the reference would raise.
* :class:`DevicePRNBatcher` packs a batch into one pinned buffer, copies it once and renders both tensors with ONE launch of
  csrc/prn_targets.hip (``mpn_prn_train_maps``): float32 ``[B, 28 coeff, 18 coeff, 17]``, the reference's float64 arithmetic
  rounded once.
* :class:`PRNDeviceLoader` iterates over a sample set in batches, as the ``DataLoader`` of ``training/multipose_prn_train.py`` does.

Reading the json file stays with the caller; pycocotools is not needed.
"""
import random

import numpy as np
import torch

from .._lib import MpnError, call
from .. import ops

ERR_INDEX, ERR_ZERODIV, ERR_NONFINITE = 1, 2, 4           # include/mpn.h: MPN_PRN_ERR_*
_ERR_NAMES = ((ERR_ZERODIV, "ZeroDivisionError"), (ERR_NONFINITE, "ValueError"), (ERR_INDEX, "IndexError"))


def gaussian_taps(sigma, truncate=4.0):
    """The normalised kernel of ``scipy.ndimage._gaussian_kernel1d(sigma, 0, int(truncate * sigma + 0.5))``, computed the same way
    (float64; skimage's gaussian passes truncate 4)."""
    radius = int(truncate * float(sigma) + 0.5)
    x = np.arange(-radius, radius + 1)
    phi_x = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    return phi_x / phi_x.sum()


TAPS9 = gaussian_taps(1.0)          # the input's blur: skimage's default sigma 1, 'nearest'
TAPS17 = gaussian_taps(2.0)         # the label's blur: sigma 2, 'constant'


def _ranges(start, count):
    """Concatenated ``arange(start[k], start[k] + count[k])`` and the k of every element."""
    owner = np.repeat(np.arange(len(count)), count)
    first = np.cumsum(count) - count
    return start[owner] + (np.arange(int(count.sum())) - first[owner]), owner


class PRNSampleSet(object):
    """``PRNSampleSet(annotations, num_of_keypoints=3)``: the samples of ``PRN_CocoDataset`` over plain COCO annotation dicts
    (``bbox``, ``keypoints``, ``image_id``, ``iscrowd``, ``num_keypoints``).

    ``order``        positions (into ``annotations``) of the reference's samples: ``iscrowd == 0 and num_keypoints >
                     num_of_keypoints``, sorted by ``num_keypoints`` descending and stable, as ``sorted(..., reverse=True)`` is.
    ``would_raise``  the sample numbers (into ``order``) for which the reference's ``get_data`` raises at this ``coeff`` and
                     ``threshold`` (``IndexError`` of the clamp chain, ``ZeroDivisionError`` of an empty box, a non-finite
                     number), found once, vectorised; ``raise_names`` gives the exception's name.  They are skipped:
                     ``len(set)`` counts and a batch index addresses the remaining samples (``valid``).  ``strict=True`` raises
                     ``ValueError`` naming them instead.

    Every annotation of an image — the own one, crowds, people with few keypoints — contributes to the inputs of that image's
    samples, in file order (pycocotools' ``imgToAnns``)."""

    def __init__(self, annotations, num_of_keypoints=3, coeff=2, threshold=0.21, strict=False):
        n = len(annotations)
        if n == 0:
            raise MpnError("no annotations")
        if int(coeff) not in (1, 2, 3):
            raise MpnError("coeff must be 1, 2 or 3")
        try:
            self.bbox = np.array([a["bbox"] for a in annotations], dtype=np.float64).reshape(n, -1)
            self.kp = np.array([a["keypoints"] for a in annotations], dtype=np.float64).reshape(n, -1)
            image_id = np.array([a["image_id"] for a in annotations])
            iscrowd = np.array([a["iscrowd"] for a in annotations])
            num_kp = np.array([a["num_keypoints"] for a in annotations])
        except (KeyError, ValueError, TypeError) as e:
            raise MpnError("annotations must be COCO person-keypoint dicts (bbox[4], keypoints[51], image_id, iscrowd, num_keypoints): %r" % (e,))
        if self.bbox.shape != (n, 4) or self.kp.shape != (n, 51):
            raise MpnError("every annotation needs bbox[4] and keypoints[51]")
        self.kp = np.ascontiguousarray(self.kp.reshape(n, 17, 3))
        self.coeff, self.threshold, self.num_of_keypoints = int(coeff), float(threshold), num_of_keypoints
        keep = np.nonzero((iscrowd == 0) & (num_kp > num_of_keypoints))[0]
        self.order = keep[np.argsort(-num_kp[keep].astype(np.int64), kind="stable")]
        # an image's annotations, grouped with a stable sort so that they keep their file order
        _, img = np.unique(image_id, return_inverse=True)
        rows = np.argsort(img, kind="stable")
        count = np.bincount(img)
        self.img_kp = np.ascontiguousarray(self.kp[rows])                     # [N, 17, 3], grouped by image
        self.img_start = (np.cumsum(count) - count)[img[self.order]]           # per sample: its image's rows of img_kp
        self.img_count = count[img[self.order]]
        self.codes = self._raise_codes()
        self.would_raise = [int(s) for s in np.nonzero(self.codes)[0]]
        self.raise_names = {s: next(nm for bit, nm in _ERR_NAMES if self.codes[s] & bit) for s in self.would_raise}
        self.valid = np.nonzero(self.codes == 0)[0]
        if strict and self.would_raise:
            raise ValueError("the reference raises for %d sample(s) (sample number, annotation position, exception): %s" % (
                len(self.would_raise), [(s, int(self.order[s]), self.raise_names[s]) for s in self.would_raise]))

    def __len__(self):
        return int(self.valid.shape[0])

    def _raise_codes(self, chunk=4096):
        """MPN_PRN_ERR_* per sample, by the kernel's own rules (csrc/prn_targets.hip), in numpy float64."""
        H, W, thr = 28.0 * self.coeff, 18.0 * self.coeff, self.threshold
        S = self.order.shape[0]
        codes = np.zeros(S, dtype=np.int32)
        with np.errstate(all="ignore"):
            for s0 in range(0, S, chunk):
                sl = slice(s0, min(S, s0 + chunk))
                b = self.bbox[self.order[sl]]
                finite = np.isfinite(b).all(axis=1)
                cw, ch = np.ceil(b[:, 2]), np.ceil(b[:, 3])
                zero = finite & ((cw == 0) | (ch == 0))
                code = np.where(finite, np.where(zero, ERR_ZERODIV, 0), ERR_NONFINITE).astype(np.int32)
                x, y, xs, ys = np.trunc(b[:, 0]), np.trunc(b[:, 1]), W / cw, H / ch

                def cells(kp, who):
                    fx, fy = (kp[..., 0] - x[who]) * xs[who], (kp[..., 1] - y[who]) * ys[who]
                    return np.isfinite(fx) & np.isfinite(fy), np.trunc(fx), np.trunc(fy)

                own = self.kp[self.order[sl]]                                       # [s, 17, 3]
                who = np.arange(own.shape[0])[:, None]
                vis = own[..., 2] > 0
                fin, x0, y0 = cells(own, who)
                kcode = np.where((vis & ~fin).any(axis=1), ERR_NONFINITE, 0)
                kcode |= np.where((vis & fin & (x0 >= W) & (y0 < -H)).any(axis=1), ERR_INDEX, 0)
                rows, who = _ranges(self.img_start[sl], self.img_count[sl])
                kp = self.img_kp[rows]                                              # [r, 17, 3]
                who = who[:, None]
                bb = b[who[:, 0]][:, None, :]
                one_t = 1 + thr
                inside = (kp[..., 2] > 0) & (kp[..., 0] > bb[..., 0] - bb[..., 2] * thr) & (kp[..., 0] < bb[..., 0] + bb[..., 2] * one_t) \
                    & (kp[..., 1] > bb[..., 1] - bb[..., 3] * thr) & (kp[..., 1] < bb[..., 1] + bb[..., 3] * one_t)
                fin, x0, y0 = cells(kp, who)
                bad_f = (inside & ~fin).any(axis=1)
                bad_i = (inside & fin & (((x0 >= W) & (y0 < -H)) | ((y0 >= H) & (x0 < -W)))).any(axis=1)
                ns = own.shape[0]
                kcode |= np.where(np.bincount(who[:, 0], weights=bad_f, minlength=ns) > 0, ERR_NONFINITE, 0)
                kcode |= np.where(np.bincount(who[:, 0], weights=bad_i, minlength=ns) > 0, ERR_INDEX, 0)
                codes[sl] = np.where(code != 0, code, kcode)
        return codes


class DevicePRNBatcher(object):
    """``DevicePRNBatcher(coeff=2, threshold=0.21, device=None)(sampleset, indices) -> (input, label)``: float32
    ``[B, 28 coeff, 18 coeff, 17]`` on the device — the reference's ``weights`` / ``output`` after ``batch_processor``'s
    ``.float()``.  ``indices`` address the set's valid samples (``raw=True``: the full ``get_anns`` order, raising samples included).

    One pinned staging buffer, one host-to-device copy, one launch; nothing in the call waits for the device.  ``render`` returns
    the per-sample error words as a third (int32, device) tensor, and ``__call__`` keeps them in ``self.err``: 0, or
    MPN_PRN_ERR_* where the reference raises — both maps of such a sample are zero.  There is no CPU path."""

    def __init__(self, coeff=2, threshold=0.21, device=None):
        if int(coeff) not in (1, 2, 3):
            raise MpnError("coeff must be 1, 2 or 3")
        dev = torch.device("cuda" if device is None else device)
        if dev.type != "cuda" or not torch.cuda.is_available():
            raise MpnError("DevicePRNBatcher runs on the MI355X only; there is no CPU path")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.coeff, self.threshold, self.device = int(coeff), float(threshold), dev
        self.H, self.W = 28 * self.coeff, 18 * self.coeff
        self.taps = torch.from_numpy(np.concatenate([TAPS9, TAPS17])).to(dev)      # resident: 26 doubles
        self.err = None

    def pack(self, sampleset, indices, raw=False):
        """Host half: the batch in one pinned float64 buffer, laid out as box [B][4] | own_kp [B][51] | img_kp [P][51] |
        person_off [B + 1] int32.  Returns (buffer, B, P)."""
        ss = sampleset
        if ss.coeff != self.coeff or ss.threshold != self.threshold:
            raise MpnError("the sample set was checked for coeff %d, threshold %r; this batcher renders coeff %d, threshold %r"
                           % (ss.coeff, ss.threshold, self.coeff, self.threshold))
        idx = np.asarray(indices, dtype=np.int64).reshape(-1)
        B = int(idx.shape[0])
        limit = ss.order.shape[0] if raw else len(ss)
        if B == 0 or idx.min() < 0 or idx.max() >= limit:
            raise MpnError("batch indices must be a non-empty list within 0..%d" % (limit - 1))
        s = idx if raw else ss.valid[idx]
        rows, _ = _ranges(ss.img_start[s], ss.img_count[s])
        P = int(rows.shape[0])
        o_own, o_img, o_off = 4 * B, 55 * B, 55 * B + 51 * P
        stage = torch.empty(o_off + (B + 2) // 2, dtype=torch.float64, pin_memory=True)
        host = stage.numpy()
        host[:o_own] = ss.bbox[ss.order[s]].reshape(-1)
        host[o_own:o_img] = ss.kp[ss.order[s]].reshape(-1)
        host[o_img:o_off] = ss.img_kp[rows].reshape(-1)
        off = host[o_off:].view(np.int32)
        off[0] = 0
        off[1:B + 1] = np.cumsum(ss.img_count[s])
        return stage, B, P

    def launch(self, packed, B, P):
        """Device half: ``packed`` is the buffer of :meth:`pack` on the device.  One launch; returns (input, label, err)."""
        o_own, o_img, o_off = 4 * B, 55 * B, 55 * B + 51 * P
        inp = torch.empty((B, self.H, self.W, 17), dtype=torch.float32, device=self.device)
        lab = torch.empty_like(inp)
        err = torch.empty(B, dtype=torch.int32, device=self.device)
        call("mpn_prn_train_maps", ops.ptr(packed), ops.ptr(packed[o_own:]), ops.ptr(packed[o_img:]), ops.ptr(packed[o_off:]), B, P,
             self.coeff, self.threshold, ops.ptr(self.taps), ops.ptr(self.taps[9:]), ops.ptr(inp), ops.ptr(lab), ops.ptr(err),
             ops.stream_ptr())
        return inp, lab, err

    def render(self, sampleset, indices, raw=False):
        stage, B, P = self.pack(sampleset, indices, raw)
        with torch.cuda.device(self.device):
            # the pinned buffer may go out of scope after this call: torch's caching host allocator hands a block out again only
            # after the copy recorded on this stream has finished
            return self.launch(stage.to(self.device, non_blocking=True), B, P)

    def __call__(self, sampleset, indices, raw=False):
        inp, lab, self.err = self.render(sampleset, indices, raw)
        return inp, lab


class PRNDeviceLoader(object):
    """Iterable over ``(input, label)`` batches already on the device; ``len()`` is the number of batches.

    ``batch_processor``'s ``'prn_subnet'`` branch (``.to(dev).float()``) returns these tensors without copying, so
    ``Trainer(model, params, batch_processor, loader, ...)`` works unchanged.  With ``shuffle`` the order of every pass is a
    permutation drawn by ``random.Random(seed)``: one generator, seeded at construction, shuffled once per pass — two loaders with
    the same seed give the same sequence of passes.  ``indices`` (default: all valid samples of the set) lets a data-parallel
    caller pass its shard."""

    def __init__(self, sampleset, batcher, batch_size, shuffle=True, seed=0, drop_last=False, indices=None):
        if int(batch_size) <= 0:
            raise MpnError("batch_size must be positive")
        self.sampleset, self.batcher, self.batch_size = sampleset, batcher, int(batch_size)
        self.shuffle, self.drop_last = bool(shuffle), bool(drop_last)
        self.indices = list(range(len(sampleset))) if indices is None else [int(i) for i in indices]
        if any(i < 0 or i >= len(sampleset) for i in self.indices):
            raise MpnError("indices must lie within the set's %d valid samples" % len(sampleset))
        self._rng = random.Random(seed)

    def __len__(self):
        n = len(self.indices)
        return n // self.batch_size if self.drop_last else (n + self.batch_size - 1) // self.batch_size

    def index_batches(self):
        """The index lists of one pass (advances the generator when shuffling)."""
        order = list(self.indices)
        if self.shuffle:
            self._rng.shuffle(order)
        return [order[k * self.batch_size:(k + 1) * self.batch_size] for k in range(len(self))]

    def __iter__(self):
        for idx in self.index_batches():
            yield self.batcher(self.sampleset, idx)
