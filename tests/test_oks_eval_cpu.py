"""Keypoint AP / AR evaluation, CPU tier: the numpy restatement of the published COCOeval(iouType='keypoints') algorithm
(tests/oks_eval_ref.py) pinned by hand-derived values, the modelled misreadings it must tell apart, the margin condition the GPU
comparisons rely on, the C-ABI surface of csrc/coco_eval.hip and the host packing of evaluate/oks_eval.py.  pycocotools is not
available here: parity is against the algorithm as published and the hand-derived pins, not against the live library."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import oks_eval_ref as R
from helpers import ROOT

NEW = ("mpn_oks_eval_workspace_bytes", "mpn_oks_matrix", "mpn_oks_match", "mpn_oks_accumulate")


SEEDED = R.SEEDED


def test_pin_a_perfect_detections():
    anns, res = R.pin_a()
    e = R.evaluate(anns, res)
    assert np.abs(e['stats'] - 1).max() <= 1e-12
    anns, res = R.pin_b(0)                         # one ground truth, one detection: tp / (fp + tp + 2^-52) = 1 / (1 + 2^-52)
    e = R.evaluate(anns, res)
    assert e['precision'][:, :, 0].max() == 0.9999999999999998 and e['precision'][:, :, 0].min() == 0.9999999999999998
    assert np.abs(e['stats'][[0, 1, 2, 3, 5, 6, 7, 8]] - 1).max() <= 1e-12
    assert e['stats'][4] == -1 and e['stats'][9] == -1          # area 4320: medium; the large range has no ground truth


@pytest.mark.parametrize("d,ap", [(3, 0.8), (6, 0.4), (9, 0.1)])
def test_pin_b_shifted_detection(d, ap):
    anns, res = R.pin_b(d)
    e = R.evaluate(anns, res)
    sig = R.constants()[3]
    want = np.mean(np.exp(-d * d / (2 * 4320.0 * (2 * sig) ** 2)))
    got = e['per_img'][0]['oks'][0, 0]
    assert abs(got - want) <= 1e-12
    n = int(np.count_nonzero(R.constants()[0] <= got))
    assert n == round(ap * 10)
    assert abs(e['stats'][0] - n / 10.0) <= 1e-12 and abs(e['stats'][0] - ap) <= 1e-12


def test_pin_c_one_hit_one_miss():
    e = R.evaluate(*R.pin_c())
    s = e['stats']
    assert np.abs(s[[0, 1, 2, 3]] - 51.0 / 101.0).max() <= 1e-12
    assert np.abs(s[[5, 6, 7, 8]] - 0.5).max() <= 1e-12
    assert s[4] == -1 and s[9] == -1


def test_pin_d_tie_goes_to_the_later_ground_truth():
    e = R.evaluate(*R.pin_d())
    assert (e['det_match'][0] == 1).all() and (e['gt_match'][0, :, 0] == -1).all() and (e['gt_match'][0, :, 1] == 0).all()


def _differs(e, e2):
    if e2['det_match'].shape != e['det_match'].shape:
        return True
    return not (np.array_equal(e2['stats'], e['stats']) and np.array_equal(e2['det_match'], e['det_match'])
                and np.array_equal(e2['det_ig'], e['det_ig']))


@pytest.fixture(scope="module")
def base():
    sets = {k: SEEDED[k]() for k in ('edge', 'big70', 'r40')}
    sets['pin_d'] = R.pin_d() + (None,)
    return sets, {k: R.evaluate(*v) for k, v in sets.items()}


# where each misreading must show: inputs built for it (edge_set, pin_d) or the seeded sets
EXPOSED_ON = {'sigma_not_doubled': 'edge', 'no_half': 'edge', 'gt_bbox_area': 'r40', 'det_bbox_area': 'edge', 'tie_first': 'pin_d',
              'no_stop_ignored': 'edge', 'crowd_not_rematchable': 'edge', 'exclusive_area': 'edge', 'no_maxdets': 'big70',
              'upper_bound': 'edge'}


@pytest.mark.parametrize("mis", R.MISREADINGS)
def test_modelled_misreading_changes_the_result(base, mis):
    sets, ref = base
    k = EXPOSED_ON[mis]
    assert _differs(ref[k], R.evaluate(*sets[k], mis=(mis,))), "%s is invisible on %s" % (mis, k)


@pytest.mark.parametrize("name", sorted(SEEDED))
def test_margin_condition(name):
    """No OKS within 1e-9 of an effective threshold and no two competing ground truths within 1e-9 of each other (values that are
    exactly 0 or 1 aside): a device OKS within the 1e-12 gate then takes the same side of every comparison."""
    e = R.evaluate(*SEEDED[name]())
    m_thr, m_pair = R.margins(e)
    print(name, "margins", m_thr, m_pair, "kept", e['det_match'].shape[2])
    assert m_thr > 1e-9 and m_pair > 1e-9


def test_seeded_inputs_cover_the_cases():
    e = R.evaluate(*SEEDED['edge']())
    by = {p['img']: p for p in e['per_img']}
    assert len(by[10]['gts']) == 2 and not by[10]['order'] and by[11]['order'] and not by[11]['gts'] and not by[12]['gts'] and not by[12]['order']
    g0 = by[13]['g0']
    assert (e['det_match'][0, 0] == g0).sum() == 3                      # the crowd takes three detections at OKS .5
    o14 = sorted(by[14]['oks'][:, 0])                                  # far outside, just outside, inside the doubled box
    assert o14[0] == 0.0 and 0.5 < o14[1] < 1.0 and o14[2] == 1.0
    assert sorted(by[15]['g_area']) == [0.0, 1024.0, 9216.0] and sorted(by[15]['d_area']) == [0.0, 0.0, 1024.0, 9216.0]
    p17 = by[17]
    assert e['det_match'][0, 0, p17['k0']] == p17['g0'] and p17['oks'][0, 1] == 1.0        # the person, not the better-fitting crowd
    assert (e['recall'][:, 0] < 1).all() and (e['precision'][:, -1, 0] == 0).all()         # recall 1 is never reached
    s = R.evaluate(*SEEDED['small_only']())
    assert (s['precision'][:, :, 1:] == -1).all() and (s['recall'][:, 1:] == -1).all() and s['stats'][0] > 0
    big = R.evaluate(*SEEDED['big70']())
    assert len(big['per_img'][0]['gts']) == 70 and len(big['per_img'][0]['dts']) == 25 and big['det_match'].shape[2] == 20
    r200 = R.evaluate(*SEEDED['r200']())
    assert 2800 <= r200['det_match'].shape[2] <= 3400 and len(r200['img_ids']) <= 200
    sc = [s_ for p in r200['per_img'] for s_ in p['score']]
    assert len(set(sc)) < len(sc) / 10                                   # equal scores within and across images


def test_pycocotools_agrees_when_present():
    pytest.importorskip("pycocotools")
    from pycocotools.coco import COCO
    from pycocotools.cocoeval import COCOeval
    anns, res, _ = SEEDED['r40']()
    coco = COCO()
    imgs = sorted(set(a['image_id'] for a in anns) | set(r['image_id'] for r in res))
    coco.dataset = {'images': [{'id': i} for i in imgs], 'annotations': anns, 'categories': [{'id': 1}]}
    coco.createIndex()
    ev = COCOeval(coco, coco.loadRes([dict(r) for r in res]), 'keypoints')
    ev.evaluate(); ev.accumulate(); ev.summarize()
    assert np.array_equal(ev.stats, R.evaluate(anns, res, imgs)['stats'])


# ---------------------------------------------------------------------------------------------- C ABI
def test_new_entry_points_are_declared_exported_and_bound():
    from multiposenet.pytorch_amd import _lib
    _lib.build()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mpn.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(mpn_[a-z0-9_]+)\s*\(", src))
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    exported = set(l.split()[-1] for l in out.splitlines() if " T mpn_" in l)
    for name in NEW:
        assert name in declared and name in exported and name in _lib.SIGNATURES
        nargs = len([a for a in re.search(r"\b%s\s*\(([^)]*)\)" % name, src).group(1).split(",") if a.strip()])
        assert nargs == len(_lib.SIGNATURES[name][1]), name
    assert "evaluate/tester.py:179-186" in open(os.path.join(ROOT, "include", "mpn.h")).read()
    mk = open(os.path.join(ROOT, "multiposenet", "pytorch_amd", "csrc", "Makefile")).read()
    assert re.search(r"^FP_STRICT = .*\bcoco_eval\b", mk, flags=re.M)
    assert re.search(r"\$\(FP_STRICT:=\.o\):.*\n\t.*-ffp-contract=off", mk) and re.search(r"filter \$\*,\$\(FP_STRICT\)\),-ffp-contract=off", mk)


def test_bad_arguments_return_badarg_without_a_gpu():
    from multiposenet.pytorch_amd import _lib
    L = _lib.lib()
    BAD = int(re.search(r"#define\s+MPN_E_BADARG\s+\(?(-?\d+)\)?", open(os.path.join(ROOT, "include", "mpn.h")).read()).group(1))
    nul, one, odd = ctypes.c_void_p(None), ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1004)       # never dereferenced
    good = np.array([[0, 0, 0, 0], [3, 2, 2, 4]], dtype=np.int64)
    tab = lambda a: ctypes.c_void_p(a.ctypes.data)

    def matrix(**kw):
        a = dict(det_kp=one, det_score=one, gt_kp=one, gt_area=one, gt_bbox=one, th=tab(good), td=one, n=1, md=2, var=one, ks=one, ksc=one,
                 ka=one, oks=one)
        a.update(kw)
        return L.mpn_oks_matrix(a['det_kp'], a['det_score'], a['gt_kp'], a['gt_area'], a['gt_bbox'], a['th'], a['td'], a['n'], a['md'], a['var'],
                                a['ks'], a['ksc'], a['ka'], a['oks'], nul)

    def match(**kw):
        a = dict(oks=one, ka=one, ga=one, gf=one, th=tab(good), td=one, n=1, md=2, rng=one, A=3, thr=one, T=10, dm=one, di=one, gi=one, gm=one)
        a.update(kw)
        return L.mpn_oks_match(a['oks'], a['ka'], a['ga'], a['gf'], a['th'], a['td'], a['n'], a['md'], a['rng'], a['A'], a['thr'], a['T'],
                               a['dm'], a['di'], a['gi'], a['gm'], nul)

    def accum(**kw):
        a = dict(sc=one, dm=one, di=one, gi=one, K=4, G=2, A=3, T=10, rec=one, R=101, order=one, pr=one, rc=one, ws=one)
        a.update(kw)
        return L.mpn_oks_accumulate(a['sc'], a['dm'], a['di'], a['gi'], a['K'], a['G'], a['A'], a['T'], a['rec'], a['R'], a['order'], a['pr'],
                                    a['rc'], a['ws'], nul)

    for k in ('det_kp', 'det_score', 'gt_kp', 'gt_area', 'gt_bbox', 'th', 'td', 'var', 'ks', 'ksc', 'ka', 'oks'):
        assert matrix(**{k: nul}) == BAD, k
    for k in ('det_kp', 'det_score', 'gt_kp', 'gt_area', 'gt_bbox', 'var', 'ksc', 'ka', 'oks'):
        assert matrix(**{k: odd}) == BAD, k                                  # misaligned doubles
    assert matrix(n=0) == BAD and matrix(n=-3) == BAD and matrix(md=0) == BAD and matrix(md=129) == BAD
    for bad in ([[0, 0, 0, 0], [3, 2, 3, 6]],          # kept 3 > max_dets 2
                [[0, 0, 0, 0], [3, 2, 2, 5]],          # OKS block is not kept x ground truths
                [[0, 0, 0, 0], [-1, 2, 0, 0]],         # descending detections
                [[0, 0, 0, 0], [3, -2, 2, 0]],         # descending ground truths
                [[1, 0, 0, 0], [3, 2, 2, 4]]):         # first row not zero
        b = np.array(bad, dtype=np.int64)
        assert matrix(th=tab(b)) == BAD and match(th=tab(b)) == BAD, bad
    for k in ('oks', 'ka', 'ga', 'gf', 'th', 'td', 'rng', 'thr', 'dm', 'di', 'gi', 'gm'):
        assert match(**{k: nul}) == BAD, k
    for k in ('oks', 'ka', 'ga', 'rng', 'thr'):
        assert match(**{k: odd}) == BAD, k
    assert match(n=0) == BAD and match(md=0) == BAD and match(md=200) == BAD and match(A=0) == BAD and match(A=9) == BAD
    assert match(T=0) == BAD and match(T=65) == BAD
    for k in ('sc', 'dm', 'di', 'gi', 'rec', 'order', 'pr', 'rc', 'ws'):
        assert accum(**{k: nul}) == BAD, k
    for k in ('sc', 'rec', 'pr', 'rc', 'ws'):
        assert accum(**{k: odd}) == BAD, k
    assert accum(K=-1) == BAD and accum(G=-1) == BAD and accum(A=0) == BAD and accum(T=0) == BAD and accum(R=0) == BAD and accum(R=5000) == BAD
    assert L.mpn_oks_eval_workspace_bytes(0, 3, 10) == 256 and L.mpn_oks_eval_workspace_bytes(5, 0, 10) == 256
    assert L.mpn_oks_eval_workspace_bytes(1000, 3, 10) == (30 * 1000 * 4 + 255) // 256 * 256 + (30 * 1000 * 8 + 255) // 256 * 256


# ---------------------------------------------------------------------------------------------- host packing
def test_host_packing():
    from multiposenet.pytorch_amd._lib import MpnError
    from multiposenet.pytorch_amd.evaluate.oks_eval import KeypointEval, iou_thrs, rec_thrs, summarize_stats
    assert iou_thrs()[8] == 0.8999999999999999 and np.array_equal(iou_thrs(), np.linspace(.5, .95, 10))
    assert np.array_equal(rec_thrs(), np.linspace(0, 1, 101))
    anns, res, ids = R.edge_set()
    shuffled = anns[::-1]
    ev = KeypointEval(shuffled)
    assert list(ev.gt_img_ids) == [10, 13, 14, 15, 16, 17] and np.array_equal(ev.var, (2 * R.constants()[3]) ** 2)
    # annotation order inside an image is kept; flags: bit 0 ignored (crowd or no keypoints), bit 1 crowd
    want = [a for i in ev.gt_img_ids for a in shuffled if a['image_id'] == i]
    assert [float(a['area']) for a in want] == ev.gt_area.tolist()
    assert ev.gt_flags.tolist() == [(1 if (a['iscrowd'] or a['num_keypoints'] == 0) else 0) | (2 if a['iscrowd'] else 0) for a in want]
    assert sorted(set(ev.gt_flags.tolist())) == [0, 1, 3]
    img, gsel, det_kp, det_score, tab = ev.pack(res, ids)
    assert list(img) == ids and len(gsel) == len(anns) and tab.dtype == np.int64 and tab.flags['C_CONTIGUOUS']
    e = R.evaluate(anns, res, ids)
    assert tab[-1].tolist() == [len(res), len(anns), e['det_match'].shape[2], sum(p['oks'].size for p in e['per_img'])]
    assert np.array_equal(np.diff(tab[:, 0]), [len(p['dts']) for p in e['per_img']])
    # the detection area comes from the keypoints, whatever the result's bbox / area fields say
    d0 = [r for r in res if r['image_id'] == 15]
    k = det_kp[tab[5, 0]:tab[6, 0]]
    assert np.array_equal(k.reshape(len(d0), 51), np.asarray([r['keypoints'] for r in d0]))
    # a subset leaves the other images' results and ground truths out; ids are taken unique and ascending
    annotated = [r for r in res if r['image_id'] != 11]              # image 11 has detections only: outside img_ids it is unknown
    img, gsel, det_kp, det_score, tab = ev.pack(annotated, [15, 13, 15])
    with pytest.raises(MpnError):
        ev.pack(res, [15, 13, 15])
    assert list(img) == [13, 15] and tab[-1, 0] == 9 and tab[-1, 1] == 5
    ev20 = KeypointEval(anns, max_dets=2)
    assert ev20.pack(res, ids)[4][-1, 2] == sum(min(2, len(p['dts'])) for p in e['per_img'])
    with pytest.raises(MpnError):
        ev.pack(res + [dict(res[0], image_id=999)], None)
    with pytest.raises(MpnError):
        ev.pack([dict(res[0], image_id=12)], None)            # 12 is known only through img_ids
    ev.pack([dict(res[0], image_id=12)], ids)
    with pytest.raises(MpnError):
        KeypointEval(anns, max_dets=0)
    # summary on the host equals the restatement's
    assert np.array_equal(summarize_stats(e['precision'], e['recall'], iou_thrs()), e['stats'])
