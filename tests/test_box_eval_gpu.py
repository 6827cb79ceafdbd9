"""Box AP / AR evaluation on the device (csrc/coco_eval.hip through evaluate/box_eval.py)
against the numpy restatement of the published algorithm (tests/box_eval_ref.py) on the same inputs.  Everything is compared bit
for bit, no tolerance and no excluded case: the IoU stage is IEEE + - * / and min / max in the order of maskApi.c:bbIou on both
sides, the matching compares those equal values, precision and recall are IEEE divisions of equal integers, and the twelve stats
are numpy means over equal arrays of equal shape."""
import json
import os

import numpy as np
import pytest
import torch

import box_eval_ref as R
import oks_eval_ref as K
from helpers import report

pytestmark = pytest.mark.gpu

_REF = {}


def _ref(name, args):
    if name not in _REF:
        _REF[name] = R.evaluate(*args)
    return _REF[name]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same_result(out, ref):
    for k in ('precision', 'recall', 'stats', 'per_category_ap'):
        assert out[k].shape == ref[k].shape and np.array_equal(_bits(out[k]), _bits(ref[k])), k


def _compare(name, anns, res, ids, cats, max_dets=(1, 10, 100)):
    from multiposenet.pytorch_amd.evaluate.box_eval import NAMES, BoxEval
    ref = _ref(name, (anns, res, ids, cats, max_dets))
    ev = BoxEval(anns, categories=cats, max_dets=max_dets)
    out = ev.evaluate(res, ids, keep_intermediates=True)
    d = {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in ev.debug.items()}
    tab = d['tab']
    line = "box_eval %-14s images %d rows %d kept %d gts %d maxDets %s: stats %s" % (
        name, len(ref['img_ids']), len(ref['rows']), tab[-1, 2], tab[-1, 1], list(max_dets), np.array2string(out['stats'], precision=4, max_line_width=1000))
    print(line)
    report(line)
    assert list(d['img_ids']) == ref['img_ids'] and ev.categories == ref['cats']
    assert d['rows'].tolist() == [[p['cat'], p['img']] for p in ref['rows']]
    assert d['kept_src'].tolist() == [tab[i, 0] + j for i, p in enumerate(ref['rows']) for j in p['order']]      # in-row order, truncation
    assert d['kept_rank'].tolist() == [r for p in ref['rows'] for r in range(len(p['order']))]
    assert np.array_equal(_bits(d['kept_area']), _bits([a for p in ref['rows'] for a in p['d_area']]))
    assert np.array_equal(_bits(d['kept_score']), _bits([s for p in ref['rows'] for s in p['score']]))
    assert np.array_equal(_bits(d['iou']), _bits(np.concatenate([p['iou'].ravel() for p in ref['rows']] + [np.zeros(0)])))
    for k in ('gt_ig', 'det_match', 'det_ig', 'gt_match'):
        assert d[k].shape == ref[k].shape and np.array_equal(d[k], ref[k]), k
    assert np.array_equal(d['order'], ref['order'])                                      # every category's stable order
    _same_result(out, ref)
    assert out['names'] == NAMES == ['AP', 'AP50', 'AP75', 'APs', 'APm', 'APl', 'AR1', 'AR10', 'AR100', 'ARs', 'ARm', 'ARl']
    return ev, out, ref


@pytest.mark.parametrize("name", ['big_row', 'edge', 'three_cats', 'one_cat_200'])
def test_device_matches_the_restatement(name):
    """big_row: one row of 70 ground truths (the > 64-lane scan of the matching) and 120 detections truncated at 100; edge: rows
    with ground truths only and with detections only, an image present through img_ids alone, a crowd matched three times beside an
    ordinary box, touching boxes (w == 0) and a diagonal pair whose w and h are both negative, zero-area boxes on both sides, areas
    exactly 32^2, 96^2 and 0, equal scores within and across images, a recall threshold never reached, a category without ground
    truth and one without detection; three_cats: three categories over 40 images; one_cat_200: about 3 000 kept detections of one
    category over 200 images, so the segmented sort and the scans cross a workgroup's 1024-element chunk."""
    _compare(name, *R.SEEDED[name]())


def test_other_max_dets_and_a_subset_of_images():
    from multiposenet.pytorch_amd.evaluate.box_eval import BoxEval
    anns, res, ids, cats = R.three_cats()
    _compare('three_cats_135', anns, res, ids, cats, max_dets=(1, 3, 5))
    _compare('three_cats_m1', anns, res, ids, cats, max_dets=(7,))
    _compare('three_cats_m4', anns, res, ids, cats, max_dets=(1, 2, 10, 100))
    # a subset through img_ids: the other images' results and ground truths stay out
    sub = ids[5:25]
    _, out, _ = _compare('three_cats_sub', anns, res, sub, cats)
    keep = set(sub)
    alone = BoxEval([a for a in anns if a['image_id'] in keep], categories=cats).evaluate([r for r in res if r['image_id'] in keep], sub)
    _same_result(alone, out)
    # a non-contiguous category list drops the third category's rows
    _compare('three_cats_29', anns, res, ids, [9, 2])


def test_pins_through_box_eval():
    ev, out, _ = _compare('pin_perfect', *R.pin_perfect(), None, None)
    assert np.abs(out['stats'] - 1).max() <= 1e-12
    lines = ev.summarize()
    assert len(lines) == 12 and lines[0] == ' Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ] = 1.000'
    assert lines[6] == ' Average Recall     (AR) @[ IoU=0.50:0.95 | area=   all | maxDets=  1 ] = 1.000'
    assert lines[11] == ' Average Recall     (AR) @[ IoU=0.50:0.95 | area= large | maxDets=100 ] = 1.000'
    ev, out, _ = _compare('pin_shift', *R.pin_shift(), None, None)
    assert float(ev.debug['iou'][0]) == 80 / 120 and abs(out['stats'][0] - 0.4) <= 1e-12
    ev, out, _ = _compare('pin_crowd', *R.pin_crowd(), None, None)
    assert float(ev.debug['iou'][0]) == 1.0 and np.abs(out['stats'][[0, 1, 2, 3]] - 1).max() <= 1e-12
    _, out, _ = _compare('pin_twelve', *R.pin_twelve(), None, None)
    assert abs(out['stats'][6] - 1 / 12) <= 1e-12 and abs(out['stats'][7] - 10 / 12) <= 1e-12 and out['stats'][8] == 1
    _, out, _ = _compare('pin_no_gt_cat', *R.pin_no_gt_category())
    assert out['per_category_ap'][1] == -1 and (out['precision'][:, :, 1] == -1).all() and abs(out['stats'][0] - 1) <= 1e-12
    ev, out, _ = _compare('pin_tie', *R.pin_tie(), None, None)
    assert (ev.debug['det_match'].cpu().numpy()[0] == 1).all()                           # the later of the two identical ground truths


def test_errors_raise():
    from multiposenet.pytorch_amd._lib import MpnError
    from multiposenet.pytorch_amd.evaluate.box_eval import BoxEval
    anns, res = R.pin_crowd()
    with pytest.raises(MpnError):
        BoxEval(anns).evaluate(res + [dict(res[0], image_id=77)])                        # neither annotated nor in img_ids
    with pytest.raises(MpnError):
        BoxEval(anns).evaluate(res + [dict(res[0], score=float('nan'))])
    with pytest.raises(MpnError):
        BoxEval(anns).evaluate(res, img_ids=[])
    with pytest.raises(MpnError):
        BoxEval(anns, max_dets=(1, 10, 200))
    with pytest.raises(MpnError):
        BoxEval(anns).summarize()
    out = BoxEval(anns).evaluate(res + [dict(res[0], category_id=5)])                    # a category that is not evaluated: skipped
    _same_result(out, R.evaluate(anns, res))
    empty = BoxEval(anns).evaluate([], img_ids=[3])                                      # no pair has anything: every entry is -1
    assert (empty['stats'] == -1).all() and (empty['precision'] == -1).all()


def _kept_1100():
    anns, res = K.random_set(7, 60, (1, 5), (19, 20))                                    # <= 20 per image: every detection is kept
    return anns, res[:1100]


# name -> (annotations, keypoint results): (a) 1 100 kept detections over 60 images with tied scores, one chunk past 1024;
# (b) no detection at all beside ground truths; (c) every ground truth below 32^2, so the medium and large ranges have npig == 0
ONE_CATEGORY = {'kept_1100': _kept_1100, 'no_detection': lambda: (K.random_set(2, 40)[0], []), 'small_only': K.small_only_set}


@pytest.mark.parametrize("name", sorted(ONE_CATEGORY))
def test_keypoint_and_box_accumulate_agree_on_one_category(name):
    """mpn_oks_accumulate is mpn_box_accumulate with one category, one maxDets entry and nothing sliced off: on the same stage-2
    results both give the same order, precision and recall, bit for bit."""
    from multiposenet.pytorch_amd import ops
    from multiposenet.pytorch_amd.evaluate.oks_eval import KeypointEval
    anns, res = ONE_CATEGORY[name]()
    ev = KeypointEval(anns)
    ev.evaluate(res, keep_intermediates=True)
    d = ev.debug
    tab = d['tab']
    n_kept, G = int(tab[-1, 2]), int(tab[-1, 1])
    A, T, R_ = len(ev.area_rng), len(ev.iou_thrs), len(ev.rec_thrs)
    rec = torch.from_numpy(ev.rec_thrs).cuda()
    out_k, out_b = (torch.full((T * R_ * A + T * A,), 7.0, dtype=torch.float64, device="cuda") for _ in range(2))
    order_k = ops.oks_accumulate(d['kept_score'], d['det_match'], d['det_ig'], d['gt_ig'], rec, out_k)
    rank = np.concatenate([np.arange(n) for n in np.diff(tab[:, 2])] + [np.zeros(0)]).astype(np.int32)
    cat_tab = np.array([[0, 0], [n_kept, G]], dtype=np.int64)
    order_b = ops.box_accumulate(d['kept_score'], torch.from_numpy(rank).cuda(), d['det_match'], d['det_ig'], d['gt_ig'], cat_tab,
                                 torch.from_numpy(cat_tab).cuda(), np.array([ev.max_dets], dtype=np.int32), rec, out_b)
    hk, hb = out_k.cpu().numpy(), out_b.cpu().numpy()
    pk, rk = hk[:T * R_ * A].reshape(T, R_, A), hk[T * R_ * A:].reshape(T, A)
    pb, rb = hb[:T * R_ * A].reshape(T, R_, 1, A, 1), hb[T * R_ * A:].reshape(T, 1, A, 1)
    line = "accumulate, one category, %-12s kept %d gts %d: recall[0] %s" % (name, n_kept, G, np.array2string(rk[0], precision=4))
    print(line)
    report(line)
    assert order_k.shape == order_b.shape == (n_kept,) and torch.equal(order_k, order_b)
    assert np.array_equal(_bits(pk), _bits(pb.reshape(T, R_, A))) and np.array_equal(_bits(rk), _bits(rb.reshape(T, A)))
    assert not (hk == 7.0).any()                                                         # every entry was written
    score = d['kept_score'].cpu().numpy()
    if name == 'kept_1100':
        assert n_kept == 1100 and len(ev.gt_img_ids) > 50 and len(set(score.tolist())) < 50 and (rk[:, 0] > 0).all()
        assert sorted(order_k.cpu().tolist()) == list(range(1100))
    elif name == 'no_detection':
        assert n_kept == 0 and G > 0 and (pk[:, :, 0] == 0).all() and (rk[:, 0] == 0).all()
    else:
        assert n_kept > 0 and (pk[:, :, 1:] == -1).all() and (rk[:, 1:] == -1).all() and (rk[:, 0] > 0).all()


def _lift_scores(model, S, per_image=40.0):
    """Random weights score every anchor far below the model's 0.05 threshold: shift the classification bias so that about
    ``per_image`` class scores of a noise image exceed 0.5."""
    with torch.no_grad():
        _, (cls, _, _) = model([torch.zeros(2, 3, S, S, device="cuda").normal_(), "detection_subnet"])
        s_ = cls.float().flatten().clamp(1e-6, 1 - 1e-6)
        q = torch.quantile(s_, 1.0 - per_image * 2 / float(s_.numel()))
        model.classificationModel.output.bias.data += float(-torch.log(q / (1 - q)))


def test_tester_detect_images_and_coco_eval_bbox(tmp_path):
    """Tester.detect_images / coco_eval_bbox end to end on a random-weight R50 fp32 model with a 3-class head at inp_size 96 and two
    images of different shapes.  The annotations are the tester's own detections plus one hand-placed box per image and class, so
    that there is a ground truth whatever the random weights find; last_box_eval equals the restatement on the returned results bit
    for bit."""
    from multiposenet.pytorch_amd._lib import MpnError
    from multiposenet.pytorch_amd.evaluate.tester import Tester, TestParams
    from test_model_gpu import get_model
    from test_multiclass_gpu import model_k
    S = 96
    model, _ = model_k(50, torch.float32, 3, swap=False)
    model.eval()
    model.freeze_bn()
    _lift_scores(model, S)
    params = TestParams()
    params.ckpt, params.inp_size = None, S
    params.coco_result_filename = str(tmp_path / "coco_box_results.json")
    tester = Tester(model, params)
    assert tester.last_box_eval is None
    rs = np.random.RandomState(1)
    images = [(5, "a.jpg", rs.uniform(0, 255, (64, 96, 3)).astype(np.float32)), (9, "b.jpg", rs.uniform(0, 255, (64, 48, 3)).astype(np.float32))]
    with pytest.raises(MpnError):
        tester.detect_images(images)                                                     # category_ids = [1] for a 3-class head
    params.category_ids = [11, 4, 30]
    dets = tester.detect_images(images)
    assert dets and set(d['category_id'] for d in dets) <= {11, 4, 30} and set(d['image_id'] for d in dets) <= {5, 9}
    assert all(sorted(d) == ['bbox', 'category_id', 'file_name', 'image_id', 'score'] and len(d['bbox']) == 4 and d['score'] > 0.05 for d in dets)
    # the rows are those of the padded batched detection path: every kept post-NMS row, boxes * scale in float32, then (x, y, w, h)
    def rows_of(group):
        with torch.no_grad():
            x = torch.stack([_network_input(tester, img) for _, _, img in group])
            _, boxes, scores, kept, classes = model.forward_all_images_padded(x, return_class=True)
        want = []
        for li, (image_id, name, img) in enumerate(group):
            scale = np.float32(float(max(img.shape[0], img.shape[1])) / S)
            for j in range(int(kept[li])):
                b = (boxes[li, j].cpu().numpy() * scale).astype(np.float64)
                want.append({'image_id': image_id, 'file_name': name, 'category_id': params.category_ids[int(classes[li, j])],
                             'bbox': [b[0], b[1], b[2] - b[0], b[3] - b[1]], 'score': float(scores[li, j])})
        return want

    assert dets == rows_of(images)
    assert tester.detect_images(images, batch=1) == rows_of(images[:1]) + rows_of(images[1:])      # one network batch per image
    per = [sum(d['image_id'] == i for d in dets) for i in (5, 9)]
    capped = tester.detect_images(images, max_per_image=2)
    assert [sum(d['image_id'] == i for d in capped) for i in (5, 9)] == [min(2, n) for n in per]
    assert capped == [d for i in (5, 9) for d in [d for d in dets if d['image_id'] == i][:2]]          # the best-scored rows
    anns = [R.ann(d['image_id'], d['category_id'], d['bbox']) for d in dets]
    for image_id, _, _ in images:
        for k, c in enumerate(params.category_ids):
            anns.append(R.ann(image_id, c, [4 + 10 * k, 6, 20, 24 + k]))
    got = tester.coco_eval_bbox(images, anns)
    assert got == dets and not os.path.exists(params.coco_result_filename)               # no file unless testresult_write_json
    want = R.evaluate(anns, got, [5, 9])
    line = "Tester.coco_eval_bbox: %d results (%s per image), %d annotations, stats %s" % (
        len(got), per, len(anns), np.array2string(tester.last_box_eval['stats'], precision=4, max_line_width=1000))
    print(line)
    report(line)
    _same_result(tester.last_box_eval, want)
    assert tester.last_box_eval['precision'].shape == (10, 101, 3, 4, 3) and tester.last_box_eval['stats'][0] > 0
    first = tester.last_box_eval
    params.testresult_write_json = True
    got1 = tester.coco_eval_bbox(images[:1], anns, categories=[4, 11])
    with open(params.coco_result_filename) as f:
        assert json.load(f) == got1 and got1 and all(d['image_id'] == 5 for d in got1)
    _same_result(tester.last_box_eval, R.evaluate(anns, got1, [5], [4, 11]))
    assert tester.last_box_eval is not first and tester.last_eval is None
    # the single-class default: category 1
    one = get_model(50, torch.float32)
    one.eval()
    one.freeze_bn()
    old_bias = one.classificationModel.output.bias.data.clone()
    try:
        _lift_scores(one, S)
        p1 = TestParams()
        p1.ckpt, p1.inp_size = None, S
        d1 = Tester(one, p1).detect_images(images)
        line = "Tester.detect_images, single-class head: %d results" % len(d1)
        print(line)
        report(line)
        assert d1 and all(d['category_id'] == 1 for d in d1)
    finally:
        one.classificationModel.output.bias.data.copy_(old_bias)


def _network_input(tester, img):
    from multiposenet.pytorch_amd.evaluate.tester import resize, resnet_preprocess
    S = tester.params.inp_size
    img = torch.from_numpy(img).cuda().float()
    side = max(img.shape[0], img.shape[1])
    sq = torch.zeros((side, side, 3), dtype=torch.float32, device="cuda")
    sq[:img.shape[0], :img.shape[1]] = img
    return resnet_preprocess(resize(sq, (S, S), cubic=False))
