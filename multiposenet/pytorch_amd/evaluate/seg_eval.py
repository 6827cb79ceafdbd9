"""Score of predicted person masks against ``mask_all`` (csrc/seg_infer.hip: mpn_mask_iou; include/mpn.h states the definitions).

    counts = mask_iou_counts(pred_buf, gt_buf, table)      # int64 [n, 3] on the device: inter, pred, gt of every image
    summary = summarize_counts(counts.cpu().numpy(), sizes) # float64 on the host, from the exact integers

A byte is ON when it is non-zero; ``union = pred + gt - inter``.  ``Tester.seg_eval`` uses both."""
import numpy as np
import torch

from .. import ops
from .._lib import MpnError, call

MIOU_COLS = 6               # H, W, offset and pitch in the prediction buffer, offset and pitch in the ground-truth buffer


def mask_iou_counts(pred_buf, gt_buf, table, out=None):
    """mpn_mask_iou: ``pred_buf`` / ``gt_buf`` are uint8 CUDA buffers, ``table`` an int64 [n, 6] host array (H, W, byte offset and row
    pitch of the image's plane in ``pred_buf``, then in ``gt_buf``) -> int64 CUDA [n, 3] = (inter, pred, gt) per image.  ``out``: a
    contiguous int64 [n, 3] CUDA tensor to write instead of a new one.  One launch (and the zeroing of the counts) on the current
    stream; nothing waits for the device."""
    table = np.ascontiguousarray(np.asarray(table, dtype=np.int64))
    if table.ndim != 2 or table.shape[1] != MIOU_COLS or table.shape[0] < 1:
        raise MpnError("mask_iou_counts: an int64 [n >= 1, %d] table expected" % MIOU_COLS)
    for buf in (pred_buf, gt_buf):
        if not buf.is_cuda or buf.dtype != torch.uint8 or not buf.is_contiguous():
            raise MpnError("mask_iou_counts: contiguous uint8 CUDA buffers expected")
    n = int(table.shape[0])
    if out is None:
        out = torch.empty((n, 3), dtype=torch.int64, device=pred_buf.device)
    elif out.dtype != torch.int64 or tuple(out.shape) != (n, 3) or not out.is_contiguous() or not out.is_cuda:
        raise MpnError("mask_iou_counts: out must be a contiguous int64 [%d, 3] CUDA tensor" % n)
    d_table = torch.from_numpy(table).to(pred_buf.device)
    call("mpn_mask_iou", ops.ptr(pred_buf), pred_buf.numel(), ops.ptr(gt_buf), gt_buf.numel(), ops.ptr(d_table), n,
         int(table[:, 0].max()), ops.ptr(out), ops.stream_ptr())
    return out


def summarize_counts(counts, sizes):
    """The float64 summary of int64 ``counts`` [n, 3] = (inter, pred, gt) and ``sizes`` [n] = pixels per image -> dict with ``iou``,
    ``mean_iou``, ``n_empty``, ``precision``, ``recall``, ``pixel_acc`` and ``n_images``.  A ratio whose denominator is 0 is nan."""
    c = np.asarray(counts, dtype=np.int64).reshape(-1, 3)
    npx = np.asarray(sizes, dtype=np.int64).reshape(-1)
    if c.shape[0] != npx.shape[0]:
        raise MpnError("summarize_counts: one pixel count per image")
    inter, pred, gt = c[:, 0], c[:, 1], c[:, 2]
    union = pred + gt - inter

    def ratio(a, b):
        return float(a) / float(b) if b > 0 else float('nan')
    full = union > 0
    per = inter[full].astype(np.float64) / union[full].astype(np.float64)
    return {'iou': ratio(inter.sum(), union.sum()),
            'mean_iou': float(per.mean()) if per.size else float('nan'),
            'n_empty': int((~full).sum()),
            'precision': ratio(inter.sum(), pred.sum()),
            'recall': ratio(inter.sum(), gt.sum()),
            'pixel_acc': ratio((npx - union + inter).sum(), npx.sum()),
            'n_images': int(c.shape[0])}
