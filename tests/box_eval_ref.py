"""COCO box AP / AR — COCOeval(iouType='bbox') computeIoU (maskApi.c:bbIou) / evaluateImg / accumulate / _summarizeDets restated in
plain numpy loops from the published algorithm.  Test-side only: independent of multiposenet/pytorch_amd/evaluate/box_eval.py, of
csrc/box_eval.hip and of tests/oks_eval_ref.py (nothing is imported from any of them).  ``mis`` switches on one modelled misreading
at a time (MISREADINGS); the tests require each to change the result on the shared inputs below, which both tiers use.

Conventions shared with the product so that results can be compared index for index: a row is one (category, image) pair with a
detection or a ground truth, category-major then ascending image id; det_match holds the index of the matched ground truth in that
row order (or -1), gt_match the index of the last matched kept detection (or -1).  ``stats`` is _summarizeDets with the LAST maxDets
entry wherever COCOeval names 100 / maxDets[2], and entries 0 and 1 for AR@1 / AR@10 (identical for COCO's [1, 10, 100]).
"""
import numpy as np

MISREADINGS = ('crowd_union', 'xyxy', 'plus_one', 'gt_box_area', 'neg_overlap', 'pooled', 'no_maxdets_slice', 'slice_after_sort',
               'exclusive_area', 'side_right', 'tie_first')

AREA_LBL = ['all', 'small', 'medium', 'large']


def constants():
    """(IoU thresholds, recall thresholds, area ranges) as COCOeval.Params.setDetParams builds them."""
    iou = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
    rec = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
    rng = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
    return iou, rec, rng


def bb_iou(D, G, crowd, mis=()):
    """maskApi.c:bbIou for one pair of (x, y, w, h) boxes."""
    dx, dy, dw, dh = [float(v) for v in D]
    gx, gy, gw, gh = [float(v) for v in G]
    if 'xyxy' in mis:
        dw, dh, gw, gh = dw - dx, dh - dy, gw - gx, gh - gy
    one = 1.0 if 'plus_one' in mis else 0.0
    ga = (gw + one) * (gh + one)
    da = (dw + one) * (dh + one)
    w = min(dw + dx, gw + gx) - max(dx, gx) + one
    h = min(dh + dy, gh + gy) - max(dy, gy) + one
    if 'neg_overlap' in mis:
        if w * h <= 0:
            return 0.0
    else:
        if w <= 0:
            return 0.0
        if h <= 0:
            return 0.0
    i = w * h
    u = da if (crowd and 'crowd_union' not in mis) else da + ga - i
    return i / u


def evaluate(anns, res, img_ids=None, categories=None, max_dets=(1, 10, 100), mis=()):
    iou_thrs, rec_thrs, area_rng = constants()
    max_dets = [int(m) for m in max_dets]
    T, R, A, M = len(iou_thrs), len(rec_thrs), len(area_rng), len(max_dets)
    if img_ids is None:
        img_ids = [a['image_id'] for a in anns]
    img_ids = sorted(set(int(i) for i in img_ids))
    if categories is None:
        categories = [a['category_id'] for a in anns]
    cats = sorted(set(int(c) for c in categories))
    cat_of = (lambda c: 0) if 'pooled' in mis else (lambda c: cats.index(c))
    n_cat = 1 if 'pooled' in mis else len(cats)
    # ---------------------------------------------------------------- computeIoU per (category, image)
    rows = []
    G = K = 0
    for k in range(n_cat):
        for img in img_ids:
            gts = [a for a in anns if a['image_id'] == img and a['category_id'] in cats and cat_of(a['category_id']) == k]
            dts = [r for r in res if r['image_id'] == img and r['category_id'] in cats and cat_of(r['category_id']) == k]
            if not gts and not dts:
                continue
            order = sorted(range(len(dts)), key=lambda j: -dts[j]['score'])[:max_dets[-1]]          # sorted() is stable
            crowd = [1 if g.get('iscrowd', 0) else 0 for g in gts]
            ig = [1 if (g.get('iscrowd', 0) or g.get('ignore', 0)) else 0 for g in gts]
            iou = np.zeros((len(order), len(gts)))
            for r_, j in enumerate(order):
                for g_, g in enumerate(gts):
                    iou[r_, g_] = bb_iou(dts[j]['bbox'], g['bbox'], crowd[g_], mis)
            g_area = [float(g['bbox'][2]) * float(g['bbox'][3]) if 'gt_box_area' in mis else float(g['area']) for g in gts]
            d_area = [float(dts[j]['bbox'][2]) * float(dts[j]['bbox'][3]) for j in order]
            rows.append(dict(cat=k, img=img, gts=gts, dts=dts, order=order, score=[float(dts[j]['score']) for j in order], iou=iou,
                             ig=ig, crowd=crowd, g_area=g_area, d_area=d_area, g0=G, k0=K))
            G += len(gts)
            K += len(order)
    # ---------------------------------------------------------------- evaluateImg
    gt_ig = np.zeros((A, G), dtype=np.int32)
    det_match = np.full((A, T, K), -1, dtype=np.int32)
    det_ig = np.zeros((A, T, K), dtype=np.int32)
    gt_match = np.full((A, T, G), -1, dtype=np.int32)
    for p in rows:
        ng, nk, g0, k0 = len(p['gts']), len(p['order']), p['g0'], p['k0']
        for a, (lo, hi) in enumerate(area_rng):
            if 'exclusive_area' in mis:
                gig = [1 if (p['ig'][g] or p['g_area'][g] <= lo or p['g_area'][g] >= hi) else 0 for g in range(ng)]
            else:
                gig = [1 if (p['ig'][g] or p['g_area'][g] < lo or p['g_area'][g] > hi) else 0 for g in range(ng)]
            gt_ig[a, g0:g0 + ng] = gig
            gtind = sorted(range(ng), key=lambda g: gig[g])                  # non-ignored first, stable
            for t, thr in enumerate(iou_thrs):
                gtm = [-1] * ng
                for d in range(nk):
                    best = min([thr, 1 - 1e-10])
                    m = -1
                    for g in gtind:
                        if gtm[g] >= 0 and not p['crowd'][g]:
                            continue
                        if m > -1 and gig[m] == 0 and gig[g] == 1:
                            break
                        v = p['iou'][d, g]
                        if 'tie_first' in mis:
                            if v < best or (m > -1 and v == best):
                                continue
                        elif v < best:
                            continue
                        best = v
                        m = g
                    if m == -1:
                        continue
                    det_ig[a, t, k0 + d] = gig[m]
                    det_match[a, t, k0 + d] = g0 + m
                    gtm[m] = k0 + d
                gt_match[a, t, g0:g0 + ng] = gtm
                for d in range(nk):
                    if det_match[a, t, k0 + d] < 0 and (p['d_area'][d] < lo or p['d_area'][d] > hi):
                        det_ig[a, t, k0 + d] = 1
    # ---------------------------------------------------------------- accumulate
    precision = -np.ones((T, R, n_cat, A, M))
    recall = -np.ones((T, n_cat, A, M))
    order_all = np.zeros((K,), dtype=np.int32)
    for k in range(n_cat):
        E = [p for p in rows if p['cat'] == k]
        if not E:
            continue
        for a in range(A):
            for m, max_det in enumerate(max_dets):
                if 'no_maxdets_slice' in mis or 'slice_after_sort' in mis:
                    idx = [p['k0'] + d for p in E for d in range(len(p['order']))]
                else:
                    idx = [p['k0'] + d for p in E for d in range(min(len(p['order']), max_det))]
                sc = np.asarray([s for p in E for s in p['score']] + [0.0])       # indexable by kept position - first k0
                first = E[0]['k0']
                scores = np.asarray([sc[i - first] for i in idx])
                inds = np.argsort(-scores, kind='mergesort')
                if 'slice_after_sort' in mis:
                    inds = inds[:max_det]
                idx = np.asarray(idx, dtype=np.int64)[inds]
                if a == 0 and m == M - 1 and 'no_maxdets_slice' not in mis and 'slice_after_sort' not in mis:
                    order_all[first:first + len(idx)] = idx
                npig = int(sum(int(gt_ig[a, p['g0'] + g] == 0) for p in E for g in range(len(p['gts']))))
                if npig == 0:
                    continue
                for t in range(T):
                    dtm = det_match[a, t, idx] >= 0
                    dig = det_ig[a, t, idx] != 0
                    tp = np.cumsum(np.logical_and(dtm, np.logical_not(dig))).astype(dtype=float)
                    fp = np.cumsum(np.logical_and(np.logical_not(dtm), np.logical_not(dig))).astype(dtype=float)
                    nd = len(tp)
                    rc = tp / npig
                    pr = tp / (fp + tp + np.spacing(1))
                    q = np.zeros((R,)).tolist()
                    recall[t, k, a, m] = rc[-1] if nd else 0
                    pr = pr.tolist()
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    pos = np.searchsorted(rc, rec_thrs, side='right' if 'side_right' in mis else 'left')
                    try:
                        for ri, pi in enumerate(pos):
                            q[ri] = pr[pi]
                    except IndexError:
                        pass
                    precision[t, :, k, a, m] = np.array(q)
    stats = summarize(precision, recall, iou_thrs)
    per_cat = np.full((n_cat,), -1.0)
    for k in range(n_cat):
        s = precision[:, :, k, 0, -1]
        if len(s[s > -1]):
            per_cat[k] = np.mean(s[s > -1])
    return dict(img_ids=img_ids, cats=cats, rows=rows, gt_ig=gt_ig, det_match=det_match, det_ig=det_ig, gt_match=gt_match,
                order=order_all, precision=precision, recall=recall, stats=stats, per_category_ap=per_cat, max_dets=max_dets)


def stat_rows(M):
    last = M - 1
    return [(1, None, 0, last), (1, .5, 0, last), (1, .75, 0, last), (1, None, 1, last), (1, None, 2, last), (1, None, 3, last),
            (0, None, 0, 0), (0, None, 0, min(1, last)), (0, None, 0, last), (0, None, 1, last), (0, None, 2, last), (0, None, 3, last)]


def summarize(precision, recall, iou_thrs):
    """COCOeval._summarizeDets: twelve times _summarize."""
    out = []
    for ap, thr, a, m in stat_rows(precision.shape[4]):
        s = precision if ap == 1 else recall
        if thr is not None:
            s = s[np.where(thr == iou_thrs)[0]]
        s = s[:, :, :, a, m] if ap == 1 else s[:, :, a, m]
        out.append(-1 if len(s[s > -1]) == 0 else np.mean(s[s > -1]))
    return np.asarray(out, dtype=np.float64)


def summary_lines(stats, max_dets=(1, 10, 100)):
    """COCOeval.summarize's lines, from its format string."""
    i_str = ' {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}'
    lines = []
    for (ap, thr, a, m), v in zip(stat_rows(len(max_dets)), stats):
        title_str = 'Average Precision' if ap == 1 else 'Average Recall'
        type_str = '(AP)' if ap == 1 else '(AR)'
        iou_str = '{:0.2f}:{:0.2f}'.format(0.5, 0.95) if thr is None else '{:0.2f}'.format(thr)
        lines.append(i_str.format(title_str, type_str, iou_str, AREA_LBL[a], max_dets[m], v))
    return lines


# ---------------------------------------------------------------------------------------------- shared inputs
def ann(img, cat, box, area=None, crowd=0, **kw):
    box = [float(v) for v in box]
    d = {'image_id': img, 'category_id': cat, 'bbox': box, 'area': float(box[2] * box[3] if area is None else area), 'iscrowd': crowd}
    d.update(kw)
    return d


def det(img, cat, box, score):
    return {'image_id': img, 'category_id': cat, 'bbox': [float(v) for v in box], 'score': float(score)}


def pin_perfect():
    """One ground truth per image in each of the three size ranges, detected exactly: every stat is 1 / (1 + 2^-52)."""
    boxes = [[5, 5, 10, 10], [20, 30, 50, 50], [40, 10, 200, 200]]
    return [ann(i + 1, 1, b) for i, b in enumerate(boxes)], [det(i + 1, 1, b, .9 - .1 * i) for i, b in enumerate(boxes)]


def pin_shift():
    """A 10 x 10 box shifted by 2: intersection 80, union 120."""
    return [ann(1, 1, [0, 0, 10, 10])], [det(1, 1, [2, 0, 10, 10], .9)]


def pin_crowd():
    """A small detection inside a large crowd (IoU = intersection / detection area = 1) beside one ordinary, exactly detected box;
    the crowd detection has the higher score, so as a false positive it would halve the precision."""
    anns = [ann(1, 1, [0, 0, 100, 100], crowd=1), ann(1, 1, [200, 200, 20, 20])]
    return anns, [det(1, 1, [10, 10, 5, 5], .9), det(1, 1, [200, 200, 20, 20], .8)]


def pin_twelve():
    boxes = [[40 * i, 0, 30, 30] for i in range(12)]
    return [ann(1, 1, b) for b in boxes], [det(1, 1, b, .95 - .01 * i) for i, b in enumerate(boxes)]


def pin_no_gt_category():
    """Category 2 has detections and no ground truth: -1 everywhere, left out of the means."""
    return [ann(1, 1, [0, 0, 40, 40])], [det(1, 1, [0, 0, 40, 40], .9), det(1, 2, [0, 0, 40, 40], .95), det(1, 2, [5, 5, 40, 40], .5)], [1], [1, 2]


def pin_tie():
    """Two identical ground truths, one detection: '>=' moves the match to the later one."""
    return [ann(1, 1, [0, 0, 20, 20]), ann(1, 1, [0, 0, 20, 20])], [det(1, 1, [0, 0, 20, 20], .9)]


def edge_set():
    """(annotations, results, image ids, categories).  Categories 1 (the cases below), 3 (ground truths, no detection), 5 (touching
    and diagonal pairs), 7 (detections, no ground truth)."""
    A, D = [], []
    # 10: ground truths only; 11: detections only; 12: known through img_ids alone
    A += [ann(10, 1, [10, 10, 40, 40]), ann(10, 1, [100, 100, 120, 120])]
    D += [det(11, 1, [0, 0, 30, 30], .5), det(11, 1, [50, 50, 30, 30], .5), det(11, 7, [0, 0, 50, 50], .7)]
    # 13: a crowd matched three times beside an ordinary box
    A += [ann(13, 1, [0, 0, 100, 100], crowd=1), ann(13, 1, [200, 200, 30, 30])]
    D += [det(13, 1, [10, 10, 10, 10], .9), det(13, 1, [30, 30, 10, 10], .5), det(13, 1, [60, 60, 20, 20], .5),
          det(13, 1, [201, 200, 30, 30], .85), det(13, 1, [400, 400, 10, 10], .5)]
    # 14, category 5: boxes that touch (w == 0), a diagonal pair whose w and h are both -10 (their product equals the union that
    # remains), and one proper match so that the category has a true positive
    A += [ann(14, 5, [0, 0, 10, 10]), ann(14, 5, [100, 100, 20, 20])]
    D += [det(14, 5, [10, 0, 10, 10], .9), det(14, 5, [20, 20, 10, 10], .8), det(14, 5, [100, 100, 20, 21], .7)]
    # 15: zero-area boxes on both sides; areas exactly 32^2, 96^2 and 0
    A += [ann(15, 1, [5, 5, 0, 10]), ann(15, 1, [100, 0, 32, 32]), ann(15, 1, [200, 0, 96, 96]), ann(15, 1, [0, 200, 40, 40], area=0.0)]
    D += [det(15, 1, [5, 5, 0, 0], .6), det(15, 1, [100, 0, 32, 32], .9), det(15, 1, [200, 0, 96, 96], .9), det(15, 1, [0, 200, 40, 40], .4),
          det(15, 1, [5, 5, 0, 10], .3)]
    # 16: two identical ground truths and one detection; a ground truth whose area field puts it in another range than its box;
    # an 'ignore' field
    A += [ann(16, 1, [0, 0, 20, 20]), ann(16, 1, [0, 0, 20, 20]), ann(16, 1, [100, 100, 40, 40], area=900.0),
          ann(16, 1, [300, 300, 50, 50], ignore=1)]
    D += [det(16, 1, [0, 0, 20, 20], .5), det(16, 1, [100, 100, 40, 38], .5), det(16, 1, [300, 300, 50, 50], .45)]
    # category 3: ground truths, no detection; category 7: detections, no ground truth
    A += [ann(13, 3, [0, 0, 50, 50]), ann(16, 3, [10, 10, 200, 200])]
    D += [det(13, 7, [0, 0, 50, 50], .9), det(16, 7, [0, 0, 10, 10], .5)]
    return A, D, [10, 11, 12, 13, 14, 15, 16], [1, 3, 5, 7]


def random_set(seed, n_img, cats, n_gt, n_det, tie_scores=True, crowd=0.05):
    """Seeded images 1..n_img: per (image, category) n_gt[0]..n_gt[1] ground truths; each is detected with probability 0.75 by a
    jittered copy, plus false positives up to n_det[0]..n_det[1] detections.  Coordinates have two decimals, the area field is a
    fraction of the box (a mask's area), scores have two decimals (many ties) or are left continuous."""
    rs = np.random.RandomState(seed)
    A, D = [], []
    for img in range(1, n_img + 1):
        for c in cats:
            ng = rs.randint(n_gt[0], n_gt[1] + 1)
            nd = rs.randint(n_det[0], n_det[1] + 1)
            dts = []
            for _ in range(ng):
                w, h = np.exp(rs.uniform(np.log(8), np.log(300), 2))
                x, y = rs.uniform(0, 640 - 8), rs.uniform(0, 480 - 8)
                box = [round(float(v), 2) for v in (x, y, w, h)]
                A.append(ann(img, c, box, area=round(box[2] * box[3] * rs.uniform(.4, 1.0), 1), crowd=int(rs.uniform() < crowd)))
                if rs.uniform() < .75 and len(dts) < nd:
                    j = rs.normal(0, .08, 4)
                    dts.append([box[0] + j[0] * box[2], box[1] + j[1] * box[3], box[2] * np.exp(j[2]), box[3] * np.exp(j[3])])
            while len(dts) < nd:
                w, h = np.exp(rs.uniform(np.log(8), np.log(300), 2))
                dts.append([rs.uniform(0, 632), rs.uniform(0, 472), w, h])
            for b in dts:
                s = rs.uniform(.05, 1)
                D.append(det(img, c, [round(float(v), 2) for v in b], round(s, 2) if tie_scores else s))
    return A, D


def big_row():
    """One row: 70 ground truths (more than a wave's 64 lanes) and 120 detections, truncated to 100."""
    anns, res = random_set(5, 1, [1], (70, 70), (120, 120))
    return anns, res, None, None


def three_cats():
    """Three categories over 40 images, 0..4 ground truths and 0..9 detections per pair."""
    anns, res = random_set(7, 40, [2, 4, 9], (0, 4), (0, 9))
    return anns, res, list(range(1, 41)), [2, 4, 9]


def one_cat_200():
    """One category, 200 images, 10..20 detections each: about 3 000 kept detections, so the segmented sort and the scans cross a
    1024-element chunk."""
    anns, res = random_set(9, 200, [1], (0, 8), (10, 20))
    return anns, res, list(range(1, 201)), [1]


SEEDED = {'big_row': big_row, 'edge': edge_set, 'three_cats': three_cats, 'one_cat_200': one_cat_200}
