"""Keypoint AP / AR evaluation on the device (csrc/coco_eval.hip through evaluate/oks_eval.py) against the numpy restatement of the
published algorithm (tests/oks_eval_ref.py) on the same inputs.  OKS blocks to 1e-12 absolute (both sides: a double exp good to
about an ulp, <= 0.37 * 3 eps of propagated argument error per term, a mean of <= 17 terms: below 1e-14); orders, truncation,
areas, every flag and match identical (test_oks_eval_cpu.py asserts the margin condition that makes the comparisons take the same
side); precision, recall and the ten stats bit for bit, being IEEE divisions of equal integers."""
import json
import os

import numpy as np
import pytest
import torch

import oks_eval_ref as R
from helpers import report

pytestmark = pytest.mark.gpu

_REF = {}


def _ref(name, args):
    if name not in _REF:
        _REF[name] = R.evaluate(*args)
    return _REF[name]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _compare(name, anns, res, ids, max_dets=20):
    from multiposenet.pytorch_amd.evaluate.oks_eval import KeypointEval
    ref = _ref(name, (anns, res, ids, max_dets))
    ev = KeypointEval(anns, max_dets=max_dets)
    out = ev.evaluate(res, ids, keep_intermediates=True)
    d = {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in ev.debug.items()}
    assert list(d['img_ids']) == ref['img_ids']
    tab = d['tab']
    want_src = [tab[i, 0] + j for i, p in enumerate(ref['per_img']) for j in p['order']]
    want_oks = np.concatenate([p['oks'].ravel() for p in ref['per_img']] + [np.zeros(0)])
    err = float(np.abs(d['oks'] - want_oks).max()) if want_oks.size else 0.0
    line = "oks_eval %-10s images %d kept %d gts %d: max |oks - ref| = %.3e, stats %s" % (
        name, len(ref['img_ids']), tab[-1, 2], tab[-1, 1], err, np.array2string(out['stats'], precision=4))
    print(line)
    report(line)
    assert d['kept_src'].tolist() == want_src                                           # in-image order and truncation
    assert np.array_equal(_bits(d['kept_area']), _bits([a for p in ref['per_img'] for a in p['d_area']]))
    assert np.array_equal(_bits(d['kept_score']), _bits([s for p in ref['per_img'] for s in p['score']]))
    assert err <= 1e-12
    for k in ('gt_ig', 'det_match', 'det_ig', 'gt_match'):
        assert np.array_equal(d[k], ref[k]), k
    assert np.array_equal(d['order'], ref['order'])
    assert np.array_equal(_bits(out['precision']), _bits(ref['precision']))
    assert np.array_equal(_bits(out['recall']), _bits(ref['recall']))
    assert np.array_equal(_bits(out['stats']), _bits(ref['stats']))
    assert out['names'] == ['AP', 'AP50', 'AP75', 'APm', 'APl', 'AR', 'AR50', 'AR75', 'ARm', 'ARl']
    return ev, out, ref


@pytest.mark.parametrize("name", ['big70', 'edge', 'small_only', 'r40', 'r200'])
def test_device_matches_the_restatement(name):
    """big70: 70 ground truths (the > 64-lane loop) and 25 detections truncated to 20; edge: images with ground truths only,
    detections only and neither, a crowd matched three times, a num_keypoints == 0 annotation, equal scores, areas on 32^2, 96^2
    and 0, a recall threshold never reached; small_only: ranges with npig == 0; r200: about 3 000 kept detections over 200 images, so
    the rank sort and the scan cross a workgroup's 1024-element chunk."""
    _compare(name, *R.SEEDED[name]())


def test_truncation_below_the_default_and_a_subset_of_images():
    anns, res, ids = R.SEEDED['r40']()
    _compare('r40_md3', anns, res, ids, max_dets=3)
    sub = ids[5:25]
    keep = set(sub)
    _compare('r40_sub', [a for a in anns if a['image_id'] in keep], [r for r in res if r['image_id'] in keep], sub)
    # the same subset chosen through img_ids from the full annotation list gives the same numbers
    from multiposenet.pytorch_amd.evaluate.oks_eval import KeypointEval
    annotated = set(a['image_id'] for a in anns)                                        # a result of an image that is neither raises
    out = KeypointEval(anns).evaluate([r for r in res if r['image_id'] in annotated or r['image_id'] in keep], sub)
    assert np.array_equal(_bits(out['stats']), _bits(_REF['r40_sub']['stats']))


def test_pins_through_keypoint_eval():
    ev, out, _ = _compare('pin_a', *R.pin_a(), None)
    assert np.abs(out['stats'] - 1).max() <= 1e-12
    lines = ev.summarize()
    assert len(lines) == 10 and lines[0] == ' Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets= 20 ] = 1.000'
    assert lines[9] == ' Average Recall     (AR) @[ IoU=0.50:0.95 | area= large | maxDets= 20 ] = 1.000'
    _, out, _ = _compare('pin_b0', *R.pin_b(0), None)
    assert out['precision'][:, :, 0].max() == 0.9999999999999998 == out['precision'][:, :, 0].min()
    for dpx, ap in ((3, 0.8), (6, 0.4), (9, 0.1)):
        ev, out, _ = _compare('pin_b%d' % dpx, *R.pin_b(dpx), None)
        sig = R.constants()[3]
        assert abs(float(ev.debug['oks'][0]) - np.mean(np.exp(-dpx * dpx / (2 * 4320.0 * (2 * sig) ** 2)))) <= 1e-12
        assert abs(out['stats'][0] - ap) <= 1e-12
    _, out, _ = _compare('pin_c', *R.pin_c(), None)
    s = out['stats']
    assert np.abs(s[[0, 1, 2, 3]] - 51.0 / 101.0).max() <= 1e-12 and np.abs(s[[5, 6, 7, 8]] - 0.5).max() <= 1e-12 and s[4] == -1 and s[9] == -1
    ev, out, _ = _compare('pin_d', *R.pin_d(), None)
    assert (ev.debug['det_match'].cpu().numpy()[0] == 1).all()                          # the later of the two identical ground truths


def test_unknown_image_raises():
    from multiposenet.pytorch_amd._lib import MpnError
    from multiposenet.pytorch_amd.evaluate.oks_eval import KeypointEval
    anns, res = R.pin_c()
    with pytest.raises(MpnError):
        KeypointEval(anns).evaluate(res + [dict(res[0], image_id=77)])


def test_tester_coco_eval_with_annotations(tmp_path):
    """Tester.coco_eval(..., annotations=...) end to end on a random-weight model: the annotations are the tester's own single-scale
    results (plus one hand-placed person per image, so that there is a ground truth whatever the random weights find);
    last_eval['stats'] equals the restatement's on the same results, the file is removed or kept per testresult_write_json, and a
    call without annotations behaves as before."""
    from multiposenet.pytorch_amd.evaluate.tester import Tester, TestParams
    from multiposenet.pytorch_amd.network import net_utils
    from multiposenet.pytorch_amd.network.posenet import poseNet
    from test_model_gpu import get_model
    model = get_model(50, torch.float32)
    ck = str(tmp_path / "ckpt_1.h5")
    net_utils.save_net(ck, model, epoch=1)
    params = TestParams()
    params.ckpt, params.inp_size = ck, 96
    params.coco_result_filename = str(tmp_path / "coco_results.json")
    tester = Tester(poseNet(50, compute_dtype=torch.float32), params)
    assert tester.last_eval is None
    rs = np.random.RandomState(1)
    images = [(5, "a.jpg", rs.uniform(0, 255, (64, 96, 3)).astype(np.float32)), (9, "b.jpg", rs.uniform(0, 255, (64, 48, 3)).astype(np.float32))]
    anns = []
    for image_id, name, img in images:
        for r in tester.infer_image(img, name, image_id):
            k = np.asarray(r['keypoints']).reshape(17, 3)
            vis = (k[:, 2] > 0) * 2.0
            kp = np.concatenate([k[:, :2] * (vis[:, None] > 0), vis[:, None]], 1)
            anns.append({'image_id': image_id, 'category_id': 1, 'keypoints': kp.reshape(-1).tolist(), 'bbox': r['bbox'],
                         'area': r['bbox'][2] * r['bbox'][3], 'iscrowd': 0, 'num_keypoints': int((vis > 0).sum())})
        anns.append(R.full_person(10, 10, 40, 50, img=image_id))
    got = tester.coco_eval(images, annotations=anns)
    assert not os.path.exists(params.coco_result_filename)                               # removed, as tester.py:188-189
    want = R.evaluate(anns, got, [5, 9])
    line = "Tester.coco_eval(annotations=): %d results, %d annotations, stats %s" % (len(got), len(anns), np.array2string(tester.last_eval['stats'], precision=4))
    print(line)
    report(line)
    assert np.array_equal(_bits(tester.last_eval['stats']), _bits(want['stats']))
    assert np.array_equal(_bits(tester.last_eval['precision']), _bits(want['precision']))
    first = tester.last_eval
    params.testresult_write_json = True
    one = images[:1]
    got1 = tester.coco_eval(one, annotations=anns)
    with open(params.coco_result_filename) as f:
        assert json.load(f) == got1 == [r for r in got if r['image_id'] == 5]            # kept
    assert np.array_equal(_bits(tester.last_eval['stats']), _bits(R.evaluate(anns, got1, [5])['stats']))
    os.remove(params.coco_result_filename)
    params.testresult_write_json = False
    kept = tester.last_eval
    assert tester.coco_eval(one) == got1 and tester.last_eval is kept and first is not kept
    with open(params.coco_result_filename) as f:
        assert json.load(f) == got1                                                      # without annotations the file is the product
