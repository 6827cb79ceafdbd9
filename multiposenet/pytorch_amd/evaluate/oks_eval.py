"""KeypointEval — COCO keypoint AP / AR (object keypoint similarity) on the device.

    ev = KeypointEval(annotations)                 # the json's ``annotations`` list (what PRNSampleSet takes), category 1
    out = ev.evaluate(results, img_ids=None)       # the result dicts Tester produces
    out['stats']                                   # the ten COCO keypoint numbers: AP, AP.5, AP.75, AP-M, AP-L, AR, AR.5, AR.75, AR-M, AR-L
    ev.summarize()                                 # logs them in COCO's wording

Stands in for ``COCOeval(coco, coco.loadRes(file), 'keypoints')`` + evaluate / accumulate / summarize of the reference
(evaluate/tester.py:179-186).  pycocotools is not used: the published algorithm is restated, OKS, matching and accumulation run in
csrc/oks_eval.hip (three stages, four launches), and only the two result arrays come back to the host, in one read.  The constant
tables are built here exactly as COCOeval's Params builds them with numpy and handed to the kernels.
"""
import logging

import numpy as np
import torch

from .. import ops
from .._lib import MpnError

logger = logging.getLogger("multiposenet")

SIGMAS = np.array([.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89]) / 10.0
AREA_RNG = [[0 ** 2, 1e5 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]            # all, medium, large
NAMES = ['AP', 'AP50', 'AP75', 'APm', 'APl', 'AR', 'AR50', 'AR75', 'ARm', 'ARl']


def iou_thrs():
    return np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)


def rec_thrs():
    return np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)


def summarize_stats(precision, recall, thrs):
    """COCOeval._summarizeKps on precision [T, R, A] / recall [T, A]: mean over the entries > -1, or -1."""
    def one(ap, thr, a):
        s = precision if ap else recall
        if thr is not None:
            s = s[np.where(thr == thrs)[0]]
        s = s[:, :, a] if ap else s[:, a]
        return float(np.mean(s[s > -1])) if len(s[s > -1]) else -1.0
    return np.array([one(ap, thr, a) for ap in (1, 0) for thr, a in ((None, 0), (.5, 0), (.75, 0), (None, 1), (None, 2))], dtype=np.float64)


class KeypointEval(object):
    def __init__(self, annotations, max_dets=20, sigmas=None):
        if not 1 <= int(max_dets) <= 128:
            raise MpnError("max_dets must be in 1..128")
        self.max_dets = int(max_dets)
        sig = SIGMAS if sigmas is None else np.asarray(sigmas, dtype=np.float64)
        if sig.shape != (17,):
            raise MpnError("sigmas must hold 17 values")
        self.var = (sig * 2) ** 2
        self.iou_thrs, self.rec_thrs = iou_thrs(), rec_thrs()
        self.area_rng = np.asarray(AREA_RNG, dtype=np.float64)
        # ground truths of category 1, grouped by image (ascending id), annotation order inside an image
        anns = [a for a in annotations if a.get('category_id', 1) == 1]
        ids = np.asarray([a['image_id'] for a in anns], dtype=np.int64)
        order = np.argsort(ids, kind='stable')
        self.gt_img_ids, counts = np.unique(ids, return_counts=True)
        self.gt_start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        n = len(anns)
        self.gt_kp = np.zeros((n, 17, 3), dtype=np.float64)
        self.gt_area = np.zeros((n,), dtype=np.float64)
        self.gt_bbox = np.zeros((n, 4), dtype=np.float64)
        self.gt_flags = np.zeros((n,), dtype=np.int32)
        for row, j in enumerate(order):
            a = anns[j]
            self.gt_kp[row] = np.asarray(a['keypoints'], dtype=np.float64).reshape(17, 3)
            self.gt_area[row] = a['area']
            self.gt_bbox[row] = a['bbox']
            crowd = 1 if a.get('iscrowd', 0) else 0
            nk = a['num_keypoints'] if 'num_keypoints' in a else int((self.gt_kp[row, :, 2] > 0).sum())
            self.gt_flags[row] = (1 if (crowd or nk == 0) else 0) | (crowd << 1)
        self._dev = None
        self.last = None
        self.debug = None

    # ------------------------------------------------------------------ host packing
    def pack(self, results, img_ids=None):
        """Host arrays of one evaluation: (image ids, ground-truth row index, det_kp [D, 17, 3], det_score [D], img_tab [I + 1, 4])."""
        known = set(self.gt_img_ids.tolist())
        if img_ids is None:
            ids = self.gt_img_ids
        else:
            ids = np.unique(np.asarray(list(img_ids), dtype=np.int64))
            known |= set(ids.tolist())
        pos = {int(v): i for i, v in enumerate(ids)}
        per = [[] for _ in ids]
        for r in results:
            if r['image_id'] not in known:
                raise MpnError("result for image %r, which is neither annotated nor in img_ids" % (r['image_id'],))
            if r.get('category_id', 1) != 1:
                continue
            i = pos.get(int(r['image_id']))
            if i is not None:
                per[i].append(r)
        D = sum(len(p) for p in per)
        det_kp = np.zeros((D, 17, 3), dtype=np.float64)
        det_score = np.zeros((D,), dtype=np.float64)
        tab = np.zeros((len(ids) + 1, 4), dtype=np.int64)
        gsel = []
        gpos = {int(v): i for i, v in enumerate(self.gt_img_ids)}
        d = 0
        for i, img in enumerate(ids):
            for r in per[i]:
                det_kp[d] = np.asarray(r['keypoints'], dtype=np.float64).reshape(17, 3)
                det_score[d] = r['score']
                d += 1
            g = gpos.get(int(img))
            ng = 0
            if g is not None:
                gsel.append(np.arange(self.gt_start[g], self.gt_start[g + 1]))
                ng = int(self.gt_start[g + 1] - self.gt_start[g])
            nk = min(len(per[i]), self.max_dets)
            tab[i + 1] = tab[i] + (len(per[i]), ng, nk, nk * ng)
        if not np.isfinite(det_score).all():
            raise MpnError("detection scores must be finite")
        gsel = np.concatenate(gsel).astype(np.int64) if gsel else np.zeros((0,), dtype=np.int64)
        return ids, gsel, det_kp, det_score, tab

    # ------------------------------------------------------------------ device
    def _device_arrays(self, dev):
        if self._dev is None or self._dev['dev'] != dev:
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
            self._dev = {'dev': dev, 'gt_kp': up(self.gt_kp), 'gt_area': up(self.gt_area), 'gt_bbox': up(self.gt_bbox),
                         'gt_flags': up(self.gt_flags), 'var': up(self.var), 'iou': up(self.iou_thrs), 'rec': up(self.rec_thrs),
                         'area_rng': up(self.area_rng)}
        return self._dev

    def evaluate(self, results, img_ids=None, keep_intermediates=False):
        """Returns {'stats': float64[10], 'precision' [T, R, A], 'recall' [T, A], 'names'}.  With keep_intermediates the device
        results of the three stages stay in ``self.debug`` (tests read them)."""
        if not torch.cuda.is_available():
            raise MpnError("KeypointEval needs the MI355X HIP kernels (no CPU fallback)")
        dev = torch.device('cuda', torch.cuda.current_device())
        ids, gsel, det_kp, det_score, tab = self.pack(results, img_ids)
        T, R, A = len(self.iou_thrs), len(self.rec_thrs), len(self.area_rng)
        if len(ids) == 0:
            raise MpnError("no image to evaluate")
        c = self._device_arrays(dev)
        if len(gsel) == len(self.gt_area):
            gt_kp, gt_area, gt_bbox, gt_flags = c['gt_kp'], c['gt_area'], c['gt_bbox'], c['gt_flags']
        else:
            sel = torch.from_numpy(gsel).to(dev)
            gt_kp, gt_area, gt_bbox, gt_flags = c['gt_kp'][sel], c['gt_area'][sel], c['gt_bbox'][sel], c['gt_flags'][sel]
        pad = lambda t: t if t.shape[0] else torch.zeros((1,) + tuple(t.shape[1:]), dtype=t.dtype, device=dev)
        gt_kp, gt_area, gt_bbox, gt_flags = pad(gt_kp), pad(gt_area), pad(gt_bbox), pad(gt_flags)
        d_kp, d_score = pad(torch.from_numpy(det_kp).to(dev)), pad(torch.from_numpy(det_score).to(dev))
        tab_d = torch.from_numpy(tab).to(dev)
        out = torch.empty((T * R * A + T * A,), dtype=torch.float64, device=dev)
        kept_src, kept_score, kept_area, oks = ops.oks_matrix(d_kp, d_score, gt_kp, gt_area, gt_bbox, tab, tab_d, self.max_dets, c['var'])
        det_match, det_ig, gt_ig, gt_match = ops.oks_match(oks, kept_area, gt_area, gt_flags, tab, tab_d, self.max_dets, c['area_rng'],
                                                           c['iou'])
        order = ops.oks_accumulate(kept_score, det_match, det_ig, gt_ig, c['rec'], out)
        host = out.cpu().numpy()                                 # the one host read
        precision, recall = host[:T * R * A].reshape(T, R, A), host[T * R * A:].reshape(T, A)
        self.last = {'stats': summarize_stats(precision, recall, self.iou_thrs), 'precision': precision, 'recall': recall,
                     'names': list(NAMES)}
        self.debug = None
        if keep_intermediates:
            self.debug = {'img_ids': ids, 'tab': tab, 'kept_src': kept_src, 'kept_score': kept_score, 'kept_area': kept_area, 'oks': oks,
                          'det_match': det_match, 'det_ig': det_ig, 'gt_ig': gt_ig, 'gt_match': gt_match, 'order': order}
        return self.last

    def summarize(self):
        """COCOeval.summarize for keypoints: the ten lines, logged."""
        if self.last is None:
            raise MpnError("summarize() before evaluate()")
        fmt = ' {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}'
        rows = [(None, 'all'), (.5, 'all'), (.75, 'all'), (None, 'medium'), (None, 'large')]
        lines = []
        for k, v in enumerate(self.last['stats']):
            thr, area = rows[k % 5]
            title, typ = ('Average Precision', '(AP)') if k < 5 else ('Average Recall', '(AR)')
            iou = '{:0.2f}:{:0.2f}'.format(self.iou_thrs[0], self.iou_thrs[-1]) if thr is None else '{:0.2f}'.format(thr)
            lines.append(fmt.format(title, typ, iou, area, self.max_dets, v))
            logger.info(lines[-1])
        return lines
