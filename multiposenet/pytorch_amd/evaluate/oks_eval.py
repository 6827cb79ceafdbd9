"""KeypointEval — COCO keypoint AP / AR (object keypoint similarity) on the device.

    ev = KeypointEval(annotations)                 # the json's ``annotations`` list (what PRNSampleSet takes), category 1
    out = ev.evaluate(results, img_ids=None)       # the result dicts Tester produces
    out['stats']                                   # the ten COCO keypoint numbers: AP, AP.5, AP.75, AP-M, AP-L, AR, AR.5, AR.75, AR-M, AR-L
    ev.summarize()                                 # logs them in COCO's wording

Stands in for ``COCOeval(coco, coco.loadRes(file), 'keypoints')`` + evaluate / accumulate / summarize of the reference
(evaluate/tester.py:179-186).  pycocotools is not used: the published algorithm is restated, OKS, matching and accumulation run in
csrc/coco_eval.hip (three stages, four launches), and only the two result arrays come back to the host, in one read.  The constant
tables are built here exactly as COCOeval's Params builds them with numpy and handed to the kernels.  What the box metric needs as
well is CocoEval's (coco_eval.py).
"""
import numpy as np
import torch

from .. import ops
from .._lib import MpnError
from .coco_eval import CocoEval, iou_thrs, mean_valid, rec_thrs  # noqa: F401  (the tables are part of this module's surface)

SIGMAS = np.array([.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89]) / 10.0
AREA_RNG = [[0 ** 2, 1e5 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]            # all, medium, large
NAMES = ['AP', 'AP50', 'AP75', 'APm', 'APl', 'AR', 'AR50', 'AR75', 'ARm', 'ARl']


def summarize_stats(precision, recall, thrs):
    """COCOeval._summarizeKps on precision [T, R, A] / recall [T, A]: mean over the entries > -1, or -1."""
    def one(ap, thr, a):
        s = precision if ap else recall
        if thr is not None:
            s = s[np.where(thr == thrs)[0]]
        s = s[:, :, a] if ap else s[:, a]
        return mean_valid(s)
    return np.array([one(ap, thr, a) for ap in (1, 0) for thr, a in ((None, 0), (.5, 0), (.75, 0), (None, 1), (None, 2))], dtype=np.float64)


class KeypointEval(CocoEval):
    GT, CONST = ('gt_kp', 'gt_area', 'gt_bbox', 'gt_flags'), {'var': 'var'}

    def __init__(self, annotations, max_dets=20, sigmas=None):
        if not 1 <= int(max_dets) <= 128:
            raise MpnError("max_dets must be in 1..128")
        self.max_dets = int(max_dets)
        sig = SIGMAS if sigmas is None else np.asarray(sigmas, dtype=np.float64)
        if sig.shape != (17,):
            raise MpnError("sigmas must hold 17 values")
        self.var = (sig * 2) ** 2
        CocoEval.__init__(self, AREA_RNG)
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

    # ------------------------------------------------------------------ host packing
    def pack(self, results, img_ids=None):
        """Host arrays of one evaluation: (image ids, ground-truth row index, det_kp [D, 17, 3], det_score [D], img_tab [I + 1, 4])."""
        ids = self.image_ids(results, img_ids)
        pos = {int(v): i for i, v in enumerate(ids)}
        per = [[] for _ in ids]
        for r in results:
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
        c, (gt_kp, gt_area, gt_bbox, gt_flags), (d_kp, d_score) = self.device_inputs(dev, gsel, det_kp, det_score)
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

    def stat_rows(self):
        return [(ap, thr, area, self.max_dets) for ap in (1, 0)
                for thr, area in ((None, 'all'), (.5, 'all'), (.75, 'all'), (None, 'medium'), (None, 'large'))]
