"""CPU tier of the detection filter / gather tests (tests/det_filter_ref.py): the generator conditions the GPU tier relies on, and
teeth — numpy models of score_filter_kernel and the gather kernels pass the GPU tier's comparisons, each named mutant fails one."""
import numpy as np
import pytest

import det_filter_ref as D
from helpers import report


def filter_runs():
    for A in D.A_SIZES:
        for name in D.CASES:
            if name == "beyond 1024" and A <= 1024:
                continue
            yield A, name


def test_filter_cases_hold_their_conditions():
    n = 0
    for A, name in filter_runs():
        boxes, s, thr = D.filter_case(A, name)
        with np.errstate(invalid="ignore"):
            passed = s > thr
        cnt = passed.sum(1)
        if name == "all":
            assert passed.all()
        if name == "none":
            assert not passed.any()
        if name == "mixed" and A >= 1023:
            assert len(set(cnt.tolist())) == 3 and cnt.min() > 0                 # different pass counts per image
        if name == "equal to the threshold":
            assert (s == thr).sum() >= D.B and not passed[s == thr].any()
        if name == "nan":
            assert np.isnan(s).sum() >= D.B and not passed[np.isnan(s)].any()
        if name == "last partial wave":
            assert cnt.min() > 0 and not passed[:, :(A - 1) // 64 * 64].any()
        if name == "beyond 1024":
            assert cnt.min() > 0 and not passed[:, :1024].any()
        n += 1
    assert {1, 63, 64, 65, 1023, 1024, 1025, 2500} == set(D.A_SIZES)
    report("det_filter cpu: %d filter cases (A in %s) hold their conditions" % (n, list(D.A_SIZES)))


def test_gather_and_chain_cases_hold_their_conditions():
    for kmax in D.KMAX:
        c = D.gather_case(kmax)
        assert c["num"].tolist() == [0, 1, kmax - 1, kmax] and c["out_stride"] > kmax and c["keep_stride"] > kmax and c["dets_stride"] > c["A"] * 5
        assert not (c["src"] == np.arange(c["A"])).all() and (c["cls_id"] != 0).all()          # a padding 0 cannot be a gathered id
    assert any(k <= 256 for k in D.KMAX) and any(k > 256 for k in D.KMAX)
    boxes, scores, cls_id, thr, iou = D.chain_case()
    cnt = (scores > thr).sum(1)
    assert cnt[2] == 0 and (cnt[[0, 1, 3]] > 64).all() and len(set(cnt.tolist())) == 4
    assert all(len(set(scores[b].tolist())) == scores.shape[1] for b in range(4))
    res, _ = D.ref_chain(boxes, scores, cls_id, thr, iou)
    kept = [len(r[1]) if r is not None else 0 for r in res]
    assert res[2] is None and all(0 < k < c_ for k, c_ in zip([kept[0], kept[1], kept[3]], cnt[[0, 1, 3]]))      # NMS suppresses some, keeps some
    report("det_filter cpu: gather cases kmax %s; chain case: candidates %s, kept by the oracle NMS %s" % (list(D.KMAX), cnt.tolist(), kept))


def _filter_checks(mut):
    failed = []
    for A, name in filter_runs():
        boxes, s, thr = D.filter_case(A, name)
        try:
            D.check_filter(D.ref_filter(boxes, s, thr), *D.model_filter(boxes, s, thr, mut))
        except AssertionError:
            failed.append("A=%d %s" % (A, name))
    return failed


def test_filter_model_is_accepted():
    assert _filter_checks(None) == []
    report("det_filter cpu: teeth: score filter model accepted by %d comparisons" % len(list(filter_runs())))


@pytest.mark.parametrize("mut", [">=", "no carry", "wrong waves", "src chunk base"])
def test_filter_mutant_is_rejected(mut):
    failed = _filter_checks(mut)
    assert failed, "mutant '%s' passes every comparison" % mut
    report("det_filter cpu: teeth: filter mutant %-16s rejected by %d comparisons, first %s" % (mut, len(failed), failed[0]))


def test_gather_model_is_accepted_and_unwritten_class_padding_is_rejected():
    for kmax in D.KMAX:
        c = D.gather_case(kmax)
        D.check_gather(D.ref_gather(c), *D.model_gather(c))
    failed = []
    for kmax in D.KMAX:
        c = D.gather_case(kmax)
        try:
            D.check_gather(D.ref_gather(c), *D.model_gather(c, "class padding unwritten"))
        except AssertionError:
            failed.append(kmax)
    assert failed
    report("det_filter cpu: teeth: gather model accepted (kmax %s); mutant 'class padding unwritten' rejected at kmax %s" % (list(D.KMAX), failed))
