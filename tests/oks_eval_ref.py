"""COCO keypoint evaluation (COCOeval(iouType='keypoints'): computeOks, evaluateImg, accumulate, summarize) restated in plain
numpy loops from the published algorithm — test-side only, independent of multiposenet/pytorch_amd/evaluate/oks_eval.py and of
csrc/oks_eval.hip.  ``mis`` switches on one modelled misreading at a time (MISREADINGS); the tests require each to change the
result on their inputs."""
import numpy as np

EPS = np.spacing(1)
MISREADINGS = ('sigma_not_doubled', 'no_half', 'gt_bbox_area', 'det_bbox_area', 'tie_first', 'no_stop_ignored',
               'crowd_not_rematchable', 'exclusive_area', 'no_maxdets', 'upper_bound')


def constants():
    iou = np.linspace(.5, 0.95, 10)
    rec = np.linspace(0, 1, 101)
    rng = [[0.0, 1e10], [32.0 ** 2, 96.0 ** 2], [96.0 ** 2, 1e10]]
    sig = np.array([.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89]) / 10.0
    return iou, rec, rng, sig


def oks_one(dk, g, var, mis=()):
    """dk: 51 floats of the detection; g: the annotation dict."""
    gk = np.asarray(g['keypoints'], dtype=np.float64)
    xg, yg, vg = gk[0::3], gk[1::3], gk[2::3]
    dk = np.asarray(dk, dtype=np.float64)
    xd, yd = dk[0::3], dk[1::3]
    k1 = int(np.count_nonzero(vg > 0))
    area = g['bbox'][2] * g['bbox'][3] if 'gt_bbox_area' in mis else g['area']
    terms = []
    bb = g['bbox']
    x0, x1, y0, y1 = bb[0] - bb[2], bb[0] + bb[2] * 2, bb[1] - bb[3], bb[1] + bb[3] * 2
    for k in range(17):
        if k1 > 0:
            if not vg[k] > 0:
                continue
            dx, dy = xd[k] - xg[k], yd[k] - yg[k]
        else:
            dx = max(0.0, x0 - xd[k]) + max(0.0, xd[k] - x1)
            dy = max(0.0, y0 - yd[k]) + max(0.0, yd[k] - y1)
        e = (dx * dx + dy * dy) / var[k] / (area + EPS)
        if 'no_half' not in mis:
            e = e / 2
        terms.append(np.exp(-e))
    s = 0.0
    for v in terms:
        s += v
    return s / len(terms)


def evaluate(annotations, results, img_ids=None, max_dets=20, mis=()):
    iou_thrs, rec_thrs, area_rng, sig = constants()
    var = sig ** 2 if 'sigma_not_doubled' in mis else (sig * 2) ** 2
    T, R, A = len(iou_thrs), len(rec_thrs), len(area_rng)
    if img_ids is None:
        img_ids = [a['image_id'] for a in annotations]
    img_ids = sorted(set(int(i) for i in img_ids))
    per_img = []
    G = K = 0
    for img in img_ids:
        gts = [a for a in annotations if a['image_id'] == img]
        dts = [r for r in results if r['image_id'] == img]
        if 'det_bbox_area' in mis:
            d_area = [r['bbox'][2] * r['bbox'][3] for r in dts]
        else:
            d_area = []
            for r in dts:
                k = np.asarray(r['keypoints'], dtype=np.float64)
                d_area.append((k[0::3].max() - k[0::3].min()) * (k[1::3].max() - k[1::3].min()))
        # stable descending sort by score
        order = sorted(range(len(dts)), key=lambda j: (-dts[j]['score'], j))
        if 'no_maxdets' not in mis:
            order = order[:max_dets]
        oks = np.zeros((len(order), len(gts)))
        for r, j in enumerate(order):
            for g, gt in enumerate(gts):
                oks[r, g] = oks_one(dts[j]['keypoints'], gt, var, mis)
        ig = [bool(g.get('iscrowd', 0)) or g['num_keypoints'] == 0 for g in gts]
        crowd = [bool(g.get('iscrowd', 0)) for g in gts]
        g_area = [(g['bbox'][2] * g['bbox'][3] if 'gt_bbox_area' in mis else g['area']) for g in gts]
        per_img.append(dict(img=img, gts=gts, dts=dts, order=order, d_area=[d_area[j] for j in order], score=[dts[j]['score'] for j in order],
                            oks=oks, ig=ig, crowd=crowd, g_area=g_area, g0=G, k0=K))
        G += len(gts)
        K += len(order)
    det_match = -np.ones((A, T, K), dtype=np.int64)
    det_ig = np.zeros((A, T, K), dtype=np.int64)
    gt_ig = np.zeros((A, G), dtype=np.int64)
    gt_match = -np.ones((A, T, G), dtype=np.int64)

    def outside(v, lo, hi):
        return (v <= lo or v >= hi) if 'exclusive_area' in mis else (v < lo or v > hi)

    for p in per_img:
        ng, nk, g0, k0 = len(p['gts']), len(p['order']), p['g0'], p['k0']
        for a, (lo, hi) in enumerate(area_rng):
            gig = [1 if (p['ig'][g] or outside(p['g_area'][g], lo, hi)) else 0 for g in range(ng)]
            gt_ig[a, g0:g0 + ng] = gig
            gtind = sorted(range(ng), key=lambda g: (gig[g], g))
            for t, thr in enumerate(iou_thrs):
                gtm = [-1] * ng
                for d in range(nk):
                    best = min(thr, 1 - 1e-10)
                    m = -1
                    for g in gtind:
                        if gtm[g] >= 0 and (not p['crowd'][g] or 'crowd_not_rematchable' in mis):
                            continue
                        if m > -1 and gig[m] == 0 and gig[g] == 1 and 'no_stop_ignored' not in mis:
                            break
                        if 'tie_first' in mis:
                            if p['oks'][d, g] < best or (m > -1 and p['oks'][d, g] == best):
                                continue
                        elif p['oks'][d, g] < best:
                            continue
                        best = p['oks'][d, g]
                        m = g
                    if m == -1:
                        det_ig[a, t, k0 + d] = 1 if outside(p['d_area'][d], lo, hi) else 0
                        continue
                    det_ig[a, t, k0 + d] = gig[m]
                    det_match[a, t, k0 + d] = g0 + m
                    gtm[m] = k0 + d
                gt_match[a, t, g0:g0 + ng] = gtm
    scores = [s for p in per_img for s in p['score']]
    order = sorted(range(K), key=lambda k: (-scores[k], k))
    precision = -np.ones((T, R, A))
    recall = -np.ones((T, A))
    for a in range(A):
        npig = int(np.count_nonzero(gt_ig[a] == 0))
        if npig == 0:
            continue
        for t in range(T):
            tp = fp = 0
            tps, pr, rc = [], [], []
            for k in order:
                if not det_ig[a, t, k]:
                    if det_match[a, t, k] >= 0:
                        tp += 1
                    else:
                        fp += 1
                tps.append(tp)
                rc.append(float(tp) / npig)
                pr.append(float(tp) / (float(fp) + float(tp) + EPS))
            recall[t, a] = rc[-1] if K else 0.0
            for i in range(K - 1, 0, -1):
                if pr[i] > pr[i - 1]:
                    pr[i - 1] = pr[i]
            i = 0                                            # rc and rec_thrs both ascend: the first index only moves right
            for r, thr in enumerate(rec_thrs):
                if 'upper_bound' in mis:
                    while i < K and rc[i] <= thr:
                        i += 1
                else:
                    while i < K and rc[i] < thr:
                        i += 1
                precision[t, r, a] = pr[i] if i < K else 0.0
    return dict(img_ids=img_ids, per_img=per_img, det_match=det_match, det_ig=det_ig, gt_ig=gt_ig, gt_match=gt_match,
                order=np.asarray(order, dtype=np.int64), precision=precision, recall=recall,
                stats=summarize(precision, recall), iou_thrs=iou_thrs)


def summarize(precision, recall):
    def mean(v):
        v = v[v > -1]
        return float(v.mean()) if v.size else -1.0
    out = []
    for arr, ap in ((precision, True), (recall, False)):
        for ts, a in ((slice(None), 0), (slice(0, 1), 0), (slice(5, 6), 0), (slice(None), 1), (slice(None), 2)):
            out.append(mean(arr[ts, :, a] if ap else arr[ts, a]))
    return np.asarray(out)


# ---------------------------------------------------------------------------------------------- seeded inputs
def person(rs, cx, cy, size, vis_p=0.8):
    """17 joints scattered in a size x size box around (cx, cy); returns (keypoints[51], bbox, area, num_keypoints)."""
    x = cx + rs.uniform(-0.5, 0.5, 17) * size
    y = cy + rs.uniform(-0.5, 0.5, 17) * size
    v = (rs.uniform(size=17) < vis_p).astype(np.float64) * rs.randint(1, 3, 17)
    k = np.zeros(51)
    k[0::3], k[1::3], k[2::3] = np.round(x), np.round(y), v
    k[0::3] *= v > 0
    k[1::3] *= v > 0
    bbox = [float(cx - size / 2), float(cy - size / 2), float(size), float(size)]
    return k.tolist(), bbox, float(size * size * 0.6), int((v > 0).sum())


def det_from(rs, kp, noise, score):
    k = np.asarray(kp, dtype=np.float64).copy()
    k[0::3] += rs.normal(0, noise, 17)
    k[1::3] += rs.normal(0, noise, 17)
    k[2::3] = 1.0
    xs, ys = k[0::3], k[1::3]
    return {'category_id': 1, 'keypoints': k.tolist(), 'score': float(score),
            'bbox': [float(xs.min()), float(ys.min()), float(xs.max() - xs.min()) * 1.3 + 5.0, float(ys.max() - ys.min()) * 1.3 + 5.0]}


def random_set(seed, n_img, gts_per_img=(0, 5), dets_per_img=(0, 8), crowd_p=0.1, nokp_p=0.1, tie_scores=True, first_id=1):
    """Annotations and results over n_img images: people of 20..260 px, detections = noisy copies of ground truths plus strays;
    some crowds, some annotations without keypoints, scores on a coarse grid so that ties occur within and across images."""
    rs = np.random.RandomState(seed)
    anns, res = [], []
    for i in range(n_img):
        img = first_id + 3 * i
        people = []
        for _ in range(rs.randint(gts_per_img[0], gts_per_img[1] + 1)):
            size = float(rs.choice([20, 31, 50, 70, 97, 140, 260]))
            kp, bbox, area, nk = person(rs, rs.uniform(50, 500), rs.uniform(50, 400), size)
            crowd = int(rs.uniform() < crowd_p)
            if rs.uniform() < nokp_p:
                kp, nk = [0.0] * 51, 0
            anns.append({'id': len(anns) + 1, 'image_id': img, 'category_id': 1, 'keypoints': kp, 'bbox': bbox, 'area': area,
                         'iscrowd': crowd, 'num_keypoints': nk})
            people.append((kp, size, bbox))
        for _ in range(rs.randint(dets_per_img[0], dets_per_img[1] + 1)):
            score = float(rs.randint(1, 40)) / 40.0 if tie_scores else float(rs.uniform())
            if people and rs.uniform() < 0.8:
                kp, size, bbox = people[rs.randint(len(people))]
                if not any(kp):
                    kp = person(rs, bbox[0] + bbox[2] / 2, bbox[1] + bbox[3] / 2, size, 1.0)[0]
                d = det_from(rs, kp, size * rs.choice([0.01, 0.03, 0.08]), score)
            else:
                d = det_from(rs, person(rs, rs.uniform(50, 500), rs.uniform(50, 400), 80.0, 1.0)[0], 1.0, score)
            d['image_id'] = img
            res.append(d)
    return anns, res


def margins(ref):
    """(smallest |oks - effective threshold|, smallest gap between two competing ground truths' OKS for one detection), over values
    that are not exactly 0 or 1.  Two ground truths compete for a detection when both can pass a threshold, i.e. both OKS values
    reach the lowest effective threshold (0.5) less the margin; below it neither is ever a candidate and their order is never read."""
    thr = [min(t, 1 - 1e-10) for t in ref['iou_thrs']]
    m_thr = m_pair = np.inf
    for p in ref['per_img']:
        o = p['oks']
        for r in range(o.shape[0]):
            row = [v for v in o[r] if v != 0.0 and v != 1.0]
            for v in row:
                m_thr = min(m_thr, min(abs(v - t) for t in thr))
            s = sorted(v for v in row if v >= thr[0] - 1e-9)
            for i in range(1, len(s)):
                m_pair = min(m_pair, s[i] - s[i - 1])
    return m_thr, m_pair


# ---------------------------------------------------------------------------------------------- hand-built inputs
def full_person(x0, y0, w, h, area=None, vis=2, crowd=0, img=1, nk=None):
    """All 17 joints on a regular pattern inside [x0, x0 + w] x [y0, y0 + h] (corners included, so the keypoint extent is w x h)."""
    fx = [0, 1, 0, 1, .5, .25, .75, .5, .25, .75, .5, .125, .875, .375, .625, .5, .5]
    fy = [0, 1, 1, 0, .5, .25, .25, .75, .75, .5, .25, .5, .5, .125, .875, .375, .625]
    k = np.zeros(51)
    k[0::3] = [x0 + f * w for f in fx]
    k[1::3] = [y0 + f * h for f in fy]
    k[2::3] = vis
    if vis == 0:
        k[:] = 0
    return {'image_id': img, 'category_id': 1, 'keypoints': k.tolist(), 'bbox': [float(x0), float(y0), float(w), float(h)],
            'area': float(w * h if area is None else area), 'iscrowd': crowd, 'num_keypoints': (17 if vis else 0) if nk is None else nk}


def det_of(ann, score, dx=0.0, dy=0.0, img=None):
    k = np.asarray(ann['keypoints'], dtype=np.float64).copy()
    k[0::3] += dx
    k[1::3] += dy
    k[2::3] = 1
    return {'image_id': ann['image_id'] if img is None else img, 'category_id': 1, 'keypoints': k.tolist(), 'score': float(score),
            'bbox': [0.0, 0.0, 7.0, 9.0]}


def pin_a():
    anns = [full_person(10, 10, 50, 60, img=1), full_person(100, 40, 120, 150, img=1), full_person(30, 30, 200, 220, img=2)]
    return anns, [det_of(a, 0.9 - 0.1 * i) for i, a in enumerate(anns)]


def pin_b(d):
    a = full_person(10, 10, 60, 72, area=4320.0)
    return [a], [det_of(a, 0.7, dx=float(d))]


def pin_c():
    a1, a2 = full_person(10, 10, 50, 60, img=1), full_person(10, 10, 50, 60, img=2)
    return [a1, a2], [det_of(a1, 0.9), det_of(a2, 0.8, dx=1000.0)]


def pin_d():
    a1, a2 = full_person(10, 10, 50, 60), full_person(10, 10, 50, 60)
    return [a1, a2], [det_of(a1, 0.9)]


def edge_set():
    """Images 10..17: ground truths only / detections only / neither (12, present through img_ids alone) / a crowd matched by three
    detections next to an ordinary person / a num_keypoints == 0 annotation with detections inside, just outside and far outside
    its doubled box / areas exactly 32^2, 96^2 and 0 on both sides / equal scores within and across images."""
    anns, res = [], []
    anns += [full_person(20, 20, 40, 80, img=10), full_person(200, 20, 100, 120, img=10)]
    ghost = full_person(50, 60, 70, 90, img=11)
    res += [det_of(ghost, 0.5), det_of(ghost, 0.5, dx=3), det_of(ghost, 0.25, dx=40)]
    crowd = full_person(100, 100, 120, 160, crowd=1, img=13)
    plain = full_person(300, 100, 60, 100, img=13)
    anns += [crowd, plain]
    res += [det_of(crowd, 0.75, dx=2), det_of(crowd, 0.5, dx=-3), det_of(crowd, 0.5, dy=4), det_of(plain, 0.625, dx=2), det_of(plain, 0.5, dx=5)]
    nokp = full_person(100, 100, 50, 50, vis=0, img=14)
    inside = full_person(60, 60, 130, 130, img=14)            # doubled box is [50, 200]^2
    res += [det_of(inside, 0.5), det_of(inside, 0.375, dx=40), det_of(inside, 0.875, dx=700)]
    anns += [nokp]
    e1, e2, e3 = full_person(10, 10, 32, 32, img=15), full_person(100, 10, 96, 96, img=15), full_person(300, 300, 0, 0, img=15)
    anns += [e1, e2, e3]
    res += [det_of(e1, 0.5, dx=1), det_of(e2, 0.5, dx=2), det_of(e3, 0.125), det_of(e3, 0.125, dx=50)]
    far = full_person(10, 10, 80, 90, img=16)
    anns += [far]
    res += [det_of(far, 0.75, dx=300)]
    # a detection right on a crowd that also passes on the ordinary person beside it: the scan stops at the first ignored one
    p17, c17 = full_person(100, 100, 60, 100, img=17), full_person(102, 100, 60, 100, crowd=1, img=17)
    anns += [p17, c17]
    res += [det_of(c17, 0.875)]
    return anns, res, [10, 11, 12, 13, 14, 15, 16, 17]


def small_only_set():
    """Every ground truth is smaller than 32^2: the medium and large ranges have npig == 0."""
    anns = [full_person(10 + 40 * i, 10, 20, 25, img=1 + i // 2) for i in range(4)]
    return anns, [det_of(a, 0.5 + 0.1 * i, dx=i) for i, a in enumerate(anns)]


def _with_ids(anns, res):
    return anns, res, sorted(set(a['image_id'] for a in anns) | set(r['image_id'] for r in res))


# the seeded inputs the CPU and GPU tests share (name -> (annotations, results, img_ids)); seeds chosen so that the margin condition
# holds (test_oks_eval_cpu.py asserts it)
SEEDED = {
    'big70': lambda: random_set(3, 1, (70, 70), (25, 25)) + (None,),
    'r40': lambda: _with_ids(*random_set(2, 40, (0, 5), (0, 8))),
    'r200': lambda: _with_ids(*random_set(3, 200, (0, 5), (11, 20), nokp_p=0.03)),
    'edge': edge_set,
    'small_only': lambda: small_only_set() + (None,),
}
