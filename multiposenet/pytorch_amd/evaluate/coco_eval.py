"""What KeypointEval (oks_eval.py) and BoxEval (box_eval.py) share: COCOeval's threshold tables, the choice of the evaluated
images, the cached upload of the ground truths, the "mean over the entries > -1" of COCOeval._summarize and its summary lines.
Stage 1 and ``pack()`` are each class's own; matching and accumulation are the same kernels for both (csrc/coco_eval.hip)."""
import logging

import numpy as np
import torch

from .._lib import MpnError

logger = logging.getLogger("multiposenet")


def iou_thrs():
    return np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)


def rec_thrs():
    return np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)


def mean_valid(s):
    return float(np.mean(s[s > -1])) if len(s[s > -1]) else -1.0


class CocoEval(object):
    """A subclass sets GT (names of its per-ground-truth arrays), CONST (cache key -> name of a constant array), ``gt_img_ids``,
    ``max_dets`` and ``stat_rows()`` = (ap, IoU threshold or None, area label, maxDets) of every summary line."""

    def __init__(self, area_rng):
        self.iou_thrs, self.rec_thrs = iou_thrs(), rec_thrs()
        self.area_rng = np.asarray(area_rng, dtype=np.float64)
        self._dev = None
        self.last = None
        self.debug = None

    def image_ids(self, results, img_ids):
        """Ascending ids of the evaluated images: the annotated ones, or ``img_ids``.  Every result must be of one of either."""
        ids = self.gt_img_ids if img_ids is None else np.unique(np.asarray(list(img_ids), dtype=np.int64))
        known = set(self.gt_img_ids.tolist()) | set(ids.tolist())
        for r in results:
            if r['image_id'] not in known:
                raise MpnError("result for image %r, which is neither annotated nor in img_ids" % (r['image_id'],))
        return ids

    def _device_arrays(self, dev):
        if self._dev is None or self._dev['dev'] != dev:
            names = dict({k: k for k in self.GT}, iou='iou_thrs', rec='rec_thrs', area_rng='area_rng', **self.CONST)
            self._dev = {k: torch.from_numpy(np.ascontiguousarray(getattr(self, v))).to(dev) for k, v in names.items()}
            self._dev['dev'] = dev
        return self._dev

    def device_inputs(self, dev, gsel, *dets):
        """(cache of uploaded arrays, [the GT arrays' rows ``gsel``], [``dets`` uploaded]); no tensor is empty (one zero row)."""
        c = self._device_arrays(dev)
        gts = [c[k] for k in self.GT]
        if len(gsel) != len(self.gt_area):
            sel = torch.from_numpy(gsel).to(dev)
            gts = [g[sel] for g in gts]
        pad = lambda t: t if t.shape[0] else torch.zeros((1,) + tuple(t.shape[1:]), dtype=t.dtype, device=dev)
        return c, [pad(g) for g in gts], [pad(torch.from_numpy(d).to(dev)) for d in dets]

    def summary_lines(self, stats):
        """COCOeval.summarize's lines for ``stats``."""
        fmt = ' {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}'
        lines = []
        for (ap, thr, area, md), v in zip(self.stat_rows(), stats):
            title, typ = ('Average Precision', '(AP)') if ap else ('Average Recall', '(AR)')
            iou = '{:0.2f}:{:0.2f}'.format(self.iou_thrs[0], self.iou_thrs[-1]) if thr is None else '{:0.2f}'.format(thr)
            lines.append(fmt.format(title, typ, iou, area, md, v))
        return lines

    def summarize(self):
        """COCOeval.summarize: the lines of the last evaluate(), logged."""
        if self.last is None:
            raise MpnError("summarize() before evaluate()")
        lines = self.summary_lines(self.last['stats'])
        for line in lines:
            logger.info(line)
        return lines
