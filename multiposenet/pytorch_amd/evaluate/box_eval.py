"""BoxEval — COCO box AP / AR (iouType 'bbox') on the device, for the detection head.

    ev = BoxEval(annotations, categories=None, max_dets=(1, 10, 100))      # the json's ``annotations`` list
    out = ev.evaluate(results, img_ids=None)        # dicts {'image_id', 'category_id', 'bbox': [x, y, w, h], 'score'}
    out['stats']                                    # the twelve COCO numbers: AP, AP50, AP75, APs, APm, APl, AR@1, AR@10, AR@100, ARs, ARm, ARl
    out['per_category_ap']                          # AP (IoU .50:.95, all areas, last maxDets) of every category, -1 without ground truth
    ev.summarize()                                  # logs the twelve lines in COCO's wording

Stands in for ``COCOeval(coco, coco.loadRes(file), 'bbox')`` + evaluate / accumulate / summarize.  pycocotools is not used: the
published algorithm is restated.  IoU blocks, matching and the per-category accumulation run in csrc/coco_eval.hip, the last two in
the kernels that score keypoints too (``ops.oks_match`` matches on any similarity blocks), five launches in all, and only the two
result arrays come back to the host, in one read.  The constant tables are built exactly as COCOeval's Params builds them with numpy.

One row of the table is one (category, image) pair with at least one detection or ground truth — COCOeval's evaluateImg returns
None for the others — ordered category-major, then by ascending image id, so that every category's kept detections and ground
truths are contiguous.  ``stats`` follows COCOeval._summarizeDets with the LAST ``max_dets`` entry wherever it names 100 or
``maxDets[2]`` (the same thing for COCO's list), and the first two entries for AR@1 / AR@10.
"""
import numpy as np
import torch

from .. import ops
from .._lib import MpnError
from .coco_eval import CocoEval, iou_thrs, mean_valid, rec_thrs  # noqa: F401  (the tables are part of this module's surface)

AREA_RNG = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]      # all, small, medium, large
AREA_LBL = ['all', 'small', 'medium', 'large']
NAMES = ['AP', 'AP50', 'AP75', 'APs', 'APm', 'APl', 'AR1', 'AR10', 'AR100', 'ARs', 'ARm', 'ARl']


def _stat_rows(M):
    """(ap, IoU threshold or None, area index, maxDets index) of the twelve lines of COCOeval._summarizeDets."""
    last = M - 1
    return [(1, None, 0, last), (1, .5, 0, last), (1, .75, 0, last), (1, None, 1, last), (1, None, 2, last), (1, None, 3, last),
            (0, None, 0, 0), (0, None, 0, min(1, last)), (0, None, 0, last), (0, None, 1, last), (0, None, 2, last), (0, None, 3, last)]


def summarize_stats(precision, recall, thrs):
    """COCOeval._summarizeDets on precision [T, R, K, A, M] / recall [T, K, A, M]: mean over the entries > -1, or -1."""
    def one(ap, thr, a, m):
        s = precision if ap else recall
        if thr is not None:
            s = s[np.where(thr == thrs)[0]]
        s = s[:, :, :, a, m] if ap else s[:, :, a, m]
        return mean_valid(s)
    return np.array([one(*row) for row in _stat_rows(precision.shape[4])], dtype=np.float64)


def per_category_ap(precision):
    """Mean over the entries > -1 of precision[:, :, k, all areas, last maxDets], or -1, for every category k."""
    return np.array([mean_valid(precision[:, :, k, 0, -1]) for k in range(precision.shape[2])], dtype=np.float64)


class BoxEval(CocoEval):
    GT, CONST = ('gt_box', 'gt_area', 'gt_flags'), {}

    def __init__(self, annotations, categories=None, max_dets=(1, 10, 100)):
        md = [int(m) for m in max_dets]
        if not 1 <= len(md) <= 4 or any(not 1 <= m <= 128 for m in md):
            raise MpnError("max_dets must hold 1..4 values in 1..128")
        self.max_dets = md
        if categories is None:
            categories = sorted(set(a['category_id'] for a in annotations))
        self.categories = sorted(set(int(c) for c in categories))            # COCOeval: catIds = np.unique(catIds)
        if not self.categories:
            raise MpnError("no category to evaluate")
        CocoEval.__init__(self, AREA_RNG)
        # ground truths grouped by category (ascending id), then image (ascending id), annotation order inside a pair
        cpos = {c: k for k, c in enumerate(self.categories)}
        anns = [a for a in annotations if a['category_id'] in cpos]
        key = np.asarray([[cpos[a['category_id']], a['image_id']] for a in anns], dtype=np.int64).reshape(-1, 2)
        order = np.lexsort((key[:, 1], key[:, 0]))                           # stable
        n = len(anns)
        self.gt_cat, self.gt_img = key[order, 0], key[order, 1]
        self.gt_box = np.zeros((n, 4), dtype=np.float64)
        self.gt_area = np.zeros((n,), dtype=np.float64)
        self.gt_flags = np.zeros((n,), dtype=np.int32)
        for row, j in enumerate(order):
            a = anns[j]
            self.gt_box[row] = a['bbox']
            self.gt_area[row] = a['area']
            crowd = 1 if a.get('iscrowd', 0) else 0
            self.gt_flags[row] = (1 if (crowd or a.get('ignore', 0)) else 0) | (crowd << 1)
        self.gt_img_ids = np.unique(np.asarray([a['image_id'] for a in annotations], dtype=np.int64))

    # ------------------------------------------------------------------ host packing
    def pack(self, results, img_ids=None):
        """Host arrays of one evaluation: (image ids, rows [n_row, 2] = (category index, image id), ground-truth row index, det_box
        [D, 4], det_score [D], tab [n_row + 1, 4], cat_tab [K + 1, 2])."""
        ids = self.image_ids(results, img_ids)
        chosen = set(ids.tolist())
        cpos = {c: k for k, c in enumerate(self.categories)}
        per = {}
        for r in results:
            k = cpos.get(r['category_id'])
            if k is None or int(r['image_id']) not in chosen:
                continue
            per.setdefault((k, int(r['image_id'])), []).append(r)
        gsel_all = np.nonzero(np.isin(self.gt_img, ids))[0].astype(np.int64)
        gts = {}
        for g in gsel_all:
            gts.setdefault((int(self.gt_cat[g]), int(self.gt_img[g])), []).append(g)
        rows = sorted(set(per) | set(gts))
        D = sum(len(p) for p in per.values())
        det_box = np.zeros((D, 4), dtype=np.float64)
        det_score = np.zeros((D,), dtype=np.float64)
        tab = np.zeros((len(rows) + 1, 4), dtype=np.int64)
        cat_tab = np.zeros((len(self.categories) + 1, 2), dtype=np.int64)
        md = self.max_dets[-1]
        gsel = []
        d = 0
        for i, row in enumerate(rows):
            dts = per.get(row, ())
            for r in dts:
                det_box[d] = r['bbox']
                det_score[d] = r['score']
                d += 1
            g = gts.get(row, ())
            gsel.extend(g)
            nk = min(len(dts), md)
            tab[i + 1] = tab[i] + (len(dts), len(g), nk, nk * len(g))
            cat_tab[row[0] + 1:] = tab[i + 1, [2, 1]]
        if not np.isfinite(det_score).all():
            raise MpnError("detection scores must be finite")
        return ids, np.asarray(rows, dtype=np.int64).reshape(-1, 2), np.asarray(gsel, dtype=np.int64), det_box, det_score, tab, cat_tab

    # ------------------------------------------------------------------ device
    def evaluate(self, results, img_ids=None, keep_intermediates=False):
        """Returns {'stats': float64[12], 'precision' [T, R, K, A, M], 'recall' [T, K, A, M], 'names', 'per_category_ap': float64[K]}.
        With keep_intermediates the device results of the three stages stay in ``self.debug`` (tests read them)."""
        if not torch.cuda.is_available():
            raise MpnError("BoxEval needs the MI355X HIP kernels (no CPU fallback)")
        dev = torch.device('cuda', torch.cuda.current_device())
        ids, rows, gsel, det_box, det_score, tab, cat_tab = self.pack(results, img_ids)
        if len(ids) == 0:
            raise MpnError("no image to evaluate")
        T, R, A, M, C = len(self.iou_thrs), len(self.rec_thrs), len(self.area_rng), len(self.max_dets), len(self.categories)
        c, (gt_box, gt_area, gt_flags), (d_box, d_score) = self.device_inputs(dev, gsel, det_box, det_score)
        tab_d, cat_tab_d = torch.from_numpy(tab).to(dev), torch.from_numpy(cat_tab).to(dev)
        md = np.asarray(self.max_dets, dtype=np.int32)
        out = torch.empty((T * R * C * A * M + T * C * A * M,), dtype=torch.float64, device=dev)
        if len(rows):
            kept_src, kept_score, kept_area, kept_rank, iou = ops.box_iou_matrix(d_box, d_score, gt_box, gt_flags, tab, tab_d, self.max_dets[-1])
            det_match, det_ig, gt_ig, gt_match = ops.oks_match(iou, kept_area, gt_area, gt_flags, tab, tab_d, self.max_dets[-1],
                                                               c['area_rng'], c['iou'])
        else:                                                    # no pair has a detection or a ground truth: every entry is -1
            e32 = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)
            e64 = torch.empty((0,), dtype=torch.float64, device=dev)
            kept_src, kept_score, kept_area, kept_rank, iou = e32(0), e64, e64, e32(0), e64
            det_match, det_ig, gt_ig, gt_match = e32(A, T, 0), e32(A, T, 0), e32(A, 0), e32(A, T, 0)
        order = ops.box_accumulate(kept_score, kept_rank, det_match, det_ig, gt_ig, cat_tab, cat_tab_d, md, c['rec'], out)
        host = out.cpu().numpy()                                 # the one host read
        n_pr = T * R * C * A * M
        precision, recall = host[:n_pr].reshape(T, R, C, A, M), host[n_pr:].reshape(T, C, A, M)
        self.last = {'stats': summarize_stats(precision, recall, self.iou_thrs), 'precision': precision, 'recall': recall,
                     'names': list(NAMES), 'per_category_ap': per_category_ap(precision)}
        self.debug = None
        if keep_intermediates:
            self.debug = {'img_ids': ids, 'rows': rows, 'tab': tab, 'cat_tab': cat_tab, 'kept_src': kept_src, 'kept_score': kept_score,
                          'kept_area': kept_area, 'kept_rank': kept_rank, 'iou': iou, 'det_match': det_match, 'det_ig': det_ig,
                          'gt_ig': gt_ig, 'gt_match': gt_match, 'order': order}
        return self.last

    def stat_rows(self):
        return [(ap, thr, AREA_LBL[a], self.max_dets[m]) for ap, thr, a, m in _stat_rows(len(self.max_dets))]
