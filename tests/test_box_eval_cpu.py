"""Box AP / AR evaluation, CPU tier: the numpy restatement of the published COCOeval(iouType='bbox') algorithm
(tests/box_eval_ref.py) pinned by hand-derived values, the modelled misreadings it must tell apart, the C-ABI surface of
csrc/coco_eval.hip, the host packing of evaluate/box_eval.py and the summary lines.  pycocotools is not available where this suite
is built: parity is against the algorithm as published and the hand-derived pins; the live comparison runs where it imports."""
import ctypes
import logging
import os
import re
import subprocess

import numpy as np
import pytest

import box_eval_ref as R
from helpers import ROOT

NEW = ("mpn_box_eval_workspace_bytes", "mpn_box_iou_matrix", "mpn_box_accumulate")


# ---------------------------------------------------------------------------------------------- hand-derived pins
def test_pin_perfect_detections_in_three_size_ranges():
    e = R.evaluate(*R.pin_perfect())
    assert np.abs(e['stats'] - 1).max() <= 1e-12
    assert e['precision'].min() >= 0.9999999999999998 and e['precision'].max() <= 1    # tp / (fp + tp + 2^-52): 1 / (1 + 2^-52), 2 / 2, 3 / 3
    one = R.evaluate(*R.pin_shift())['precision'][0, :, 0, 0, -1]
    assert one.min() == 0.9999999999999998 == one.max()                                  # a single true positive: 1 / (1 + 2^-52)
    assert (e['recall'] == 1).all()


def test_pin_shifted_box():
    e = R.evaluate(*R.pin_shift())
    got = e['rows'][0]['iou'][0, 0]
    assert got == 80 / 120                                                               # exactly: intersection 80, union 120
    assert int(np.count_nonzero(R.constants()[0] <= got)) == 4
    assert (e['det_match'][0, :4, 0] == 0).all() and (e['det_match'][0, 4:, 0] == -1).all()
    assert abs(e['stats'][0] - 0.4) <= 1e-12 and abs(e['stats'][1] - 1) <= 1e-12 and e['stats'][2] == 0
    assert abs(e['stats'][3] - 0.4) <= 1e-12 and e['stats'][4] == -1 and e['stats'][5] == -1          # area 100: small


def test_pin_small_detection_inside_a_crowd():
    e = R.evaluate(*R.pin_crowd())
    assert e['rows'][0]['iou'][0, 0] == 1.0                                              # 25 / 25: the crowd rule
    assert (e['det_match'][0, :, 0] == 0).all() and (e['det_ig'][0, :, 0] == 1).all()    # matched, ignored
    assert np.abs(e['stats'][[0, 1, 2, 3]] - 1).max() <= 1e-12                           # hence no false positive
    wrong = R.evaluate(*R.pin_crowd(), mis=('crowd_union',))
    assert wrong['rows'][0]['iou'][0, 0] == 25 / 10000 and abs(wrong['stats'][0] - 0.5) <= 1e-12


def test_pin_twelve_pairs_in_one_image():
    e = R.evaluate(*R.pin_twelve())
    s = e['stats']
    assert abs(s[6] - 1 / 12) <= 1e-12 and abs(s[7] - 10 / 12) <= 1e-12 and s[8] == 1
    assert abs(s[0] - 1) <= 1e-12


def test_pin_category_without_ground_truth_is_left_out():
    anns, res, ids, cats = R.pin_no_gt_category()
    e = R.evaluate(anns, res, ids, cats)
    assert (e['precision'][:, :, 1] == -1).all() and (e['recall'][:, 1] == -1).all()
    assert e['per_category_ap'][1] == -1 and abs(e['per_category_ap'][0] - 1) <= 1e-12
    assert np.abs(e['stats'][[0, 1, 2, 4, 6, 7, 8, 10]] - 1).max() <= 1e-12              # area 1600: medium
    assert (e['stats'][[3, 5, 9, 11]] == -1).all()


def test_pin_tie_goes_to_the_later_ground_truth():
    e = R.evaluate(*R.pin_tie())
    assert (e['det_match'][0] == 1).all() and (e['gt_match'][0, :, 0] == -1).all() and (e['gt_match'][0, :, 1] == 0).all()


# ---------------------------------------------------------------------------------------------- misreadings
def _differs(e, e2):
    if e2['det_match'].shape != e['det_match'].shape or e2['precision'].shape != e['precision'].shape:
        return True
    return not (np.array_equal(e2['stats'], e['stats']) and np.array_equal(e2['det_match'], e['det_match'])
                and np.array_equal(e2['det_ig'], e['det_ig']))


@pytest.fixture(scope="module")
def base():
    sets = {k: R.SEEDED[k]() for k in ('edge', 'three_cats', 'big_row')}
    return sets, {k: R.evaluate(*v) for k, v in sets.items()}


# the inputs built for each misreading (edge_set) and a seeded set that must show it as well where random data can
EXPOSED_ON = {'crowd_union': ('edge', 'three_cats'), 'xyxy': ('edge', 'three_cats'), 'plus_one': ('edge', 'three_cats'),
              'gt_box_area': ('edge', 'three_cats'), 'neg_overlap': ('edge', 'three_cats'), 'pooled': ('edge', 'three_cats'),
              'no_maxdets_slice': ('edge', 'big_row'), 'slice_after_sort': ('edge', 'three_cats'), 'exclusive_area': ('edge',),
              'side_right': ('edge', 'three_cats'), 'tie_first': ('edge',)}


@pytest.mark.parametrize("mis", R.MISREADINGS)
def test_modelled_misreading_changes_the_result(base, mis):
    sets, ref = base
    for k in EXPOSED_ON[mis]:
        assert _differs(ref[k], R.evaluate(*sets[k], mis=(mis,))), "%s is invisible on %s" % (mis, k)


def test_seeded_inputs_cover_the_cases():
    anns, res, ids, cats = R.edge_set()
    e = R.evaluate(anns, res, ids, cats)
    by = {(cats[p['cat']], p['img']): p for p in e['rows']}
    assert [(cats[p['cat']], p['img']) for p in e['rows']] == sorted(by)                 # category-major, then image
    assert len(by[1, 10]['gts']) == 2 and not by[1, 10]['order'] and by[1, 11]['order'] and not by[1, 11]['gts']
    assert all(img != 12 for _, img in by) and 12 in e['img_ids']
    p = by[1, 13]
    assert (e['det_match'][0, 0] == p['g0']).sum() == 3 and p['crowd'] == [1, 0]          # the crowd takes three detections
    p = by[5, 14]
    assert p['iou'][0, 0] == 0 and p['iou'][1, 0] == 0 and R.bb_iou(p['dts'][1]['bbox'], p['gts'][0]['bbox'], 0, ('neg_overlap',)) == 1.0
    p = by[1, 15]
    assert sorted(p['g_area']) == [0.0, 0.0, 1024.0, 9216.0] and sorted(p['d_area']) == [0.0, 0.0, 1024.0, 1600.0, 9216.0]
    g32 = p['g0'] + 1
    assert e['gt_ig'][:, g32].tolist() == [0, 0, 0, 1] and e['gt_ig'][:, g32 + 1].tolist() == [0, 1, 0, 0]      # bounds are inclusive
    assert (e['recall'][:, 0, 0, -1] < 1).all() and (e['precision'][:, -1, 0, 0, -1] == 0).all()      # recall 1 is never reached
    assert e['per_category_ap'][1] == 0 and e['per_category_ap'][3] == -1                # no detection; no ground truth
    assert (e['recall'][:, 1, 0] == 0).all() and (e['precision'][:, :, 3] == -1).all()
    sc = [s for p in e['rows'] for s in p['score']]
    assert sc.count(.5) >= 6                                                             # equal scores within and across images
    big = R.evaluate(*R.big_row())
    assert len(big['rows']) == 1 and len(big['rows'][0]['gts']) == 70 and len(big['rows'][0]['dts']) == 120 and big['det_match'].shape[2] == 100
    r200 = R.evaluate(*R.one_cat_200())
    assert 2800 <= r200['det_match'].shape[2] <= 3400 and len(r200['img_ids']) == 200
    sc = [s for p in r200['rows'] for s in p['score']]
    assert len(set(sc)) < len(sc) / 10
    c3 = R.evaluate(*R.three_cats())
    assert c3['precision'].shape == (10, 101, 3, 4, 3) and (c3['per_category_ap'] > 0).all()
    small = R.evaluate(*R.three_cats()[:2], img_ids=R.three_cats()[2], categories=[2, 4, 9], max_dets=(1, 3, 5))
    assert small['det_match'].shape[2] == sum(min(5, len(p['dts'])) for p in c3['rows'])
    assert small['stats'][8] < c3['stats'][8]


def test_slice_then_sort_equals_carrying_the_sliced_entries():
    """The subsequence argument of DESIGN.md on data: for every maxDets entry, COCOeval's slice-then-merge-sort order is the full
    per-category order with the detections of in-row position >= maxDets removed."""
    anns, res, ids, cats = R.three_cats()
    e = R.evaluate(anns, res, ids, cats, max_dets=(1, 3, 5))
    rank = np.concatenate([np.arange(len(p['order'])) for p in e['rows']])
    score = np.concatenate([p['score'] for p in e['rows']] + [np.zeros(0)])
    for k in range(3):
        E = [p for p in e['rows'] if p['cat'] == k]
        first, n = E[0]['k0'], sum(len(p['order']) for p in E)
        full = e['order'][first:first + n]
        assert sorted(full.tolist()) == list(range(first, first + n))
        for md in (1, 3, 5):
            idx = np.asarray([p['k0'] + d for p in E for d in range(min(len(p['order']), md))])
            want = idx[np.argsort(-score[idx], kind='mergesort')]
            assert np.array_equal(full[rank[full] < md], want)


def test_pycocotools_agrees_when_present():
    pytest.importorskip("pycocotools")
    from pycocotools.coco import COCO
    from pycocotools.cocoeval import COCOeval
    anns, res, ids, cats = R.three_cats()
    anns = [dict(a, id=i + 1) for i, a in enumerate(anns)]
    coco = COCO()
    coco.dataset = {'images': [{'id': i} for i in ids], 'annotations': anns, 'categories': [{'id': c} for c in cats]}
    coco.createIndex()
    ev = COCOeval(coco, coco.loadRes([dict(r) for r in res]), 'bbox')
    ev.evaluate(); ev.accumulate(); ev.summarize()
    want = R.evaluate(anns, res, ids, cats)
    assert np.array_equal(ev.stats, want['stats']) and np.array_equal(ev.eval['precision'], want['precision'])


# ---------------------------------------------------------------------------------------------- C ABI
def test_new_entry_points_are_declared_exported_and_bound():
    from multiposenet.pytorch_amd import _lib
    _lib.build()
    text = open(os.path.join(ROOT, "include", "mpn.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(mpn_[a-z0-9_]+)\s*\(", src))
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    exported = set(l.split()[-1] for l in out.splitlines() if " T mpn_" in l)
    for name in NEW:
        assert name in declared and name in exported and name in _lib.SIGNATURES
        nargs = len([a for a in re.search(r"\b%s\s*\(([^)]*)\)" % name, src).group(1).split(",") if a.strip()])
        assert nargs == len(_lib.SIGNATURES[name][1]), name
    assert "maskApi.c:bbIou" in text and "COCOeval(coco, res, 'bbox')" in text
    mk = open(os.path.join(ROOT, "multiposenet", "pytorch_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS = .*\bcoco_eval\.hip\b", mk, flags=re.M) and re.search(r"^FP_STRICT = .*\bcoco_eval\b", mk, flags=re.M)
    assert re.search(r"\$\(FP_STRICT:=\.o\):.*\n\t.*-ffp-contract=off", mk) and re.search(r"filter \$\*,\$\(FP_STRICT\)\),-ffp-contract=off", mk)


def test_the_library_holds_one_rank_and_one_accumulate_kernel():
    """Keypoints and boxes share stages 2 and 3: the evaluation kernels of the production library are the two similarity front ends,
    the match, one rank sort and one accumulate."""
    import sys
    from multiposenet.pytorch_amd import _lib
    tools = os.path.join(ROOT, "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import codeobj
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    names = [k["name"] for k in codeobj.kernels(_lib.LIB_PATH)]
    base = [n[m.end():m.end() + int(m.group(1))] for n in names for m in [re.match(r"^_ZN12_GLOBAL__N_1(\d+)", n)] if m]
    found = sorted(b for b in base if re.match(r"^(oks_|coco_|box_(iou|rank|accum))", b))
    assert found == ['box_iou_kernel', 'coco_accum_kernel', 'coco_rank_kernel', 'oks_match_kernel', 'oks_matrix_kernel'], found


def test_bad_arguments_return_badarg_without_a_gpu():
    from multiposenet.pytorch_amd import _lib
    L = _lib.lib()
    BAD = int(re.search(r"#define\s+MPN_E_BADARG\s+\(?(-?\d+)\)?", open(os.path.join(ROOT, "include", "mpn.h")).read()).group(1))
    nul, one, odd = ctypes.c_void_p(None), ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1004)       # never dereferenced
    good = np.array([[0, 0, 0, 0], [3, 2, 2, 4]], dtype=np.int64)
    cgood = np.array([[0, 0], [4, 2]], dtype=np.int64)
    mgood = np.array([1, 10, 100], dtype=np.int32)
    hp = lambda a: ctypes.c_void_p(a.ctypes.data)

    def matrix(**kw):
        a = dict(db=one, ds=one, gb=one, gf=one, th=hp(good), td=one, n=1, md=2, ks=one, ksc=one, ka=one, kr=one, iou=one)
        a.update(kw)
        return L.mpn_box_iou_matrix(a['db'], a['ds'], a['gb'], a['gf'], a['th'], a['td'], a['n'], a['md'], a['ks'], a['ksc'], a['ka'], a['kr'],
                                    a['iou'], nul)

    def accum(**kw):
        a = dict(sc=one, kr=one, dm=one, di=one, gi=one, ch=hp(cgood), cd=one, C=1, K=4, G=2, A=4, T=10, mh=hp(mgood), M=3, rec=one, R=101,
                 order=one, pr=one, rc=one, ws=one)
        a.update(kw)
        return L.mpn_box_accumulate(a['sc'], a['kr'], a['dm'], a['di'], a['gi'], a['ch'], a['cd'], a['C'], a['K'], a['G'], a['A'], a['T'],
                                    a['mh'], a['M'], a['rec'], a['R'], a['order'], a['pr'], a['rc'], a['ws'], nul)

    for k in ('db', 'ds', 'gb', 'gf', 'th', 'td', 'ks', 'ksc', 'ka', 'kr', 'iou'):
        assert matrix(**{k: nul}) == BAD, k
    for k in ('db', 'ds', 'gb', 'td', 'ksc', 'ka', 'iou'):
        assert matrix(**{k: odd}) == BAD, k                                  # misaligned doubles / int64 table
    assert matrix(n=0) == BAD and matrix(n=-3) == BAD and matrix(md=0) == BAD and matrix(md=129) == BAD
    for bad in ([[0, 0, 0, 0], [3, 2, 3, 6]],          # kept 3 > max_dets 2
                [[0, 0, 0, 0], [3, 2, 2, 5]],          # IoU block is not kept x ground truths
                [[0, 0, 0, 0], [-1, 2, 0, 0]],         # descending detections
                [[0, 0, 0, 0], [3, -2, 2, 0]],         # descending ground truths
                [[1, 0, 0, 0], [3, 2, 2, 4]]):         # first row not zero
        assert matrix(th=hp(np.array(bad, dtype=np.int64))) == BAD, bad
    for k in ('sc', 'kr', 'dm', 'di', 'gi', 'ch', 'cd', 'mh', 'rec', 'order', 'pr', 'rc', 'ws'):
        assert accum(**{k: nul}) == BAD, k
    for k in ('sc', 'cd', 'rec', 'pr', 'rc', 'ws'):
        assert accum(**{k: odd}) == BAD, k
    assert accum(K=-1) == BAD and accum(G=-1) == BAD and accum(A=0) == BAD and accum(A=9) == BAD and accum(T=0) == BAD and accum(T=65) == BAD
    assert accum(R=0) == BAD and accum(R=5000) == BAD and accum(M=0) == BAD and accum(M=5) == BAD and accum(C=0) == BAD and accum(C=70000) == BAD
    for bad in ([[1, 0], [4, 2]],                      # first row not zero
                [[0, 0], [3, 2]],                      # does not end at the kept total
                [[0, 0], [4, 1]]):                     # does not end at the ground-truth total
        assert accum(ch=hp(np.array(bad, dtype=np.int64))) == BAD, bad
    two = np.array([[0, 0], [5, 1], [4, 2]], dtype=np.int64)                 # descending kept detections
    assert accum(ch=hp(two), C=2) == BAD
    for bad in ([0, 10, 100], [1, 10, 129]):
        assert accum(mh=hp(np.array(bad, dtype=np.int32))) == BAD, bad
    W = L.mpn_box_eval_workspace_bytes
    assert W(0, 4, 3, 10) == 256 and W(5, 0, 3, 10) == 256 and W(5, 4, 0, 10) == 256 and W(5, 4, 3, 0) == 256
    assert W(1000, 4, 3, 10) == (120 * 1000 * 4 + 255) // 256 * 256 + (120 * 1000 * 8 + 255) // 256 * 256


# ---------------------------------------------------------------------------------------------- host packing
def test_host_packing():
    from multiposenet.pytorch_amd._lib import MpnError
    from multiposenet.pytorch_amd.evaluate.box_eval import AREA_RNG, BoxEval, summarize_stats, per_category_ap
    assert np.array_equal(np.asarray(AREA_RNG, dtype=np.float64), np.asarray([[0, 1e10], [0, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e10]]))
    anns, res, ids, cats = R.edge_set()
    shuffled = anns[::-1]
    ev = BoxEval(shuffled)
    assert ev.categories == [1, 3, 5] and ev.max_dets == [1, 10, 100]                    # the default: the annotations' categories
    ev = BoxEval(shuffled, categories=[7, 1, 5, 3, 1])
    assert ev.categories == cats and list(ev.gt_img_ids) == [10, 13, 14, 15, 16]
    assert np.array_equal(ev.iou_thrs, R.constants()[0]) and np.array_equal(ev.rec_thrs, R.constants()[1])
    # ground truths: category-major, then image, annotation order inside a pair; flags: bit 0 ignored (crowd or ignore), bit 1 crowd
    want = [a for c in cats for i in ev.gt_img_ids for a in shuffled if a['category_id'] == c and a['image_id'] == i]
    assert [a['bbox'] for a in want] == ev.gt_box.tolist() and [a['area'] for a in want] == ev.gt_area.tolist()
    assert ev.gt_flags.tolist() == [(1 if (a['iscrowd'] or a.get('ignore')) else 0) | (2 if a['iscrowd'] else 0) for a in want]
    assert sorted(set(ev.gt_flags.tolist())) == [0, 1, 3]
    assert ev.gt_area[[a['area'] == 900.0 for a in want].index(True)] == 900.0            # the area field, not w * h = 1600
    ev = BoxEval(anns, categories=cats)
    img, rows, gsel, det_box, det_score, tab, cat_tab = ev.pack(res, ids)
    e = R.evaluate(anns, res, ids, cats)
    assert list(img) == ids and tab.dtype == np.int64 and tab.flags['C_CONTIGUOUS'] and cat_tab.dtype == np.int64 and cat_tab.flags['C_CONTIGUOUS']
    # rows: every (category, image) pair with a detection or a ground truth, category-major then ascending image id
    assert rows.tolist() == [[p['cat'], p['img']] for p in e['rows']] and rows.tolist() == sorted(rows.tolist())
    assert gsel.tolist() == list(range(len(anns)))
    # tab invariants: starts at zero, kept = min(detections, last maxDets), IoU block = kept x ground truths, totals last
    assert tab[0].tolist() == [0, 0, 0, 0]
    d = np.diff(tab, axis=0)
    assert d[:, 0].tolist() == [len(p['dts']) for p in e['rows']] and d[:, 1].tolist() == [len(p['gts']) for p in e['rows']]
    assert np.array_equal(d[:, 2], np.minimum(d[:, 0], 100)) and np.array_equal(d[:, 3], d[:, 2] * d[:, 1]) and ((d[:, 0] > 0) | (d[:, 1] > 0)).all()
    assert tab[-1].tolist() == [len(res), len(anns), e['det_match'].shape[2], sum(p['iou'].size for p in e['rows'])]
    # cat_tab invariants: first kept detection and first ground truth of every category, totals last; empty segments allowed
    assert cat_tab.shape == (5, 2) and cat_tab[0].tolist() == [0, 0] and cat_tab[-1].tolist() == [tab[-1, 2], tab[-1, 1]]
    for k in range(4):
        sel = rows[:, 0] == k
        assert cat_tab[k + 1, 0] - cat_tab[k, 0] == d[sel, 2].sum() and cat_tab[k + 1, 1] - cat_tab[k, 1] == d[sel, 1].sum()
    assert cat_tab[2, 0] == cat_tab[1, 0] and cat_tab[4, 1] == cat_tab[3, 1]              # category 3: no detection; 7: no ground truth
    # detections in input order inside a row
    first = [r for r in res if r['category_id'] == 1 and r['image_id'] == 11]
    assert det_box[:2].tolist() == [r['bbox'] for r in first] and det_score[:2].tolist() == [r['score'] for r in first]
    # truncation follows the last maxDets entry
    ev3 = BoxEval(anns, categories=cats, max_dets=(1, 2, 3))
    assert ev3.pack(res, ids)[5][-1, 2] == sum(min(3, len(p['dts'])) for p in e['rows'])
    # a non-contiguous category list: results and ground truths of other categories are skipped, never an error
    ev17 = BoxEval(anns + [R.ann(13, 4, [0, 0, 5, 5])], categories=[1, 3, 7])
    _, rows17, gsel17, box17, _, tab17, cat17 = ev17.pack(res, ids)
    assert sorted(set(rows17[:, 0].tolist())) == [0, 1, 2] and tab17[-1, 0] == sum(r['category_id'] in (1, 7) for r in res)
    assert tab17[-1, 1] == sum(a['category_id'] in (1, 3) for a in anns) and cat17[:, 1].tolist()[-2:] == [tab17[-1, 1]] * 2
    # a subset leaves the other images' results and ground truths out; ids are taken unique and ascending
    annotated = [r for r in res if r['image_id'] != 11]              # image 11 has detections only: outside img_ids it is unknown
    img, rows_s, gsel_s, _, _, tab_s, _ = ev.pack(annotated, [15, 13, 15])
    assert list(img) == [13, 15] and sorted(set(rows_s[:, 1].tolist())) == [13, 15]
    assert tab_s[-1, 0] == sum(r['image_id'] in (13, 15) for r in res) and tab_s[-1, 1] == sum(a['image_id'] in (13, 15) for a in anns)
    assert [ev.gt_img[g] for g in gsel_s] == [13, 13, 15, 15, 15, 15, 13]
    with pytest.raises(MpnError):
        ev.pack(res, [15, 13, 15])                                   # image 11: neither annotated nor in img_ids
    with pytest.raises(MpnError):
        ev.pack(res + [dict(res[0], image_id=999)], ids)
    with pytest.raises(MpnError):
        ev.pack([dict(res[0], image_id=12)], None)                   # 12 is known only through img_ids
    ev.pack([dict(res[0], image_id=12)], ids)
    with pytest.raises(MpnError):
        ev.pack(res + [dict(res[0], score=float('nan'))], ids)
    with pytest.raises(MpnError):
        ev.pack(res + [dict(res[0], score=float('inf'))], ids)
    n = ev.pack(res + [dict(res[0], category_id=99)], ids)[5][-1, 0]
    assert n == len(res)                                             # unknown category: skipped
    for bad in ((), (1, 2, 3, 4, 5), (0, 10), (1, 129)):
        with pytest.raises(MpnError):
            BoxEval(anns, max_dets=bad)
    # summary on the host equals the restatement's, bit for bit
    assert np.array_equal(summarize_stats(e['precision'], e['recall'], ev.iou_thrs), e['stats'])
    assert np.array_equal(per_category_ap(e['precision']), e['per_category_ap'])


def test_summary_lines_follow_cocos_format(caplog):
    from multiposenet.pytorch_amd._lib import MpnError
    from multiposenet.pytorch_amd.evaluate.box_eval import NAMES, BoxEval
    anns, res, ids, cats = R.edge_set()
    e = R.evaluate(anns, res, ids, cats)
    ev = BoxEval(anns, categories=cats)
    with pytest.raises(MpnError):
        ev.summarize()
    ev.last = {'stats': e['stats']}
    with caplog.at_level(logging.INFO, logger="multiposenet"):
        lines = ev.summarize()
    assert lines == R.summary_lines(e['stats']) and len(lines) == 12 == len(NAMES)
    assert [r.getMessage() for r in caplog.records if r.name == "multiposenet"][-12:] == lines
    fmt = ' {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}'
    assert lines[0] == fmt.format('Average Precision', '(AP)', '0.50:0.95', 'all', 100, e['stats'][0])
    assert lines[1].startswith(' Average Precision  (AP) @[ IoU=0.50      | area=   all | maxDets=100 ] = ')
    assert lines[3] == fmt.format('Average Precision', '(AP)', '0.50:0.95', 'small', 100, e['stats'][3])
    assert lines[6] == fmt.format('Average Recall', '(AR)', '0.50:0.95', 'all', 1, e['stats'][6])
    assert lines[7] == fmt.format('Average Recall', '(AR)', '0.50:0.95', 'all', 10, e['stats'][7])
    assert lines[11] == fmt.format('Average Recall', '(AR)', '0.50:0.95', 'large', 100, e['stats'][11])
    ev5 = BoxEval(anns, categories=cats, max_dets=(1, 3, 5))
    assert ev5.summary_lines(e['stats'])[8].endswith('maxDets=  5 ] = %0.3f' % e['stats'][8])
    assert ev5.summary_lines(e['stats']) == R.summary_lines(e['stats'], (1, 3, 5))


def test_no_cpu_fallback():
    import torch
    from multiposenet.pytorch_amd._lib import MpnError
    from multiposenet.pytorch_amd.evaluate.box_eval import BoxEval
    if not torch.cuda.is_available():
        with pytest.raises(MpnError):
            BoxEval(*R.pin_shift()[:1]).evaluate(R.pin_shift()[1])


def test_test_params_carry_the_category_mapping():
    from multiposenet.pytorch_amd.evaluate.tester import Tester, TestParams
    assert TestParams.category_ids == [1] and hasattr(Tester, 'detect_images') and hasattr(Tester, 'coco_eval_bbox')
