"""CPU tests of the PRN training-pair path (datasets/prn_data.py, mpn_prn_train_maps): the float64 restatement
tests/prn_train_ref.py against the fixture recorded from the real reference with real scikit-image (tests/golden/g18_prn_train.npz,
written by tests/golden/make_golden_prn_train.py), the host side of the product (sample order, raising samples, loader), the
C-ABI argument checks, and the teeth of the comparison.

Bounds.  The restatement and the fixture run the same float64 operations in the same order; the only difference is the tap
vectors, whose ``exp`` differs by an ulp between the two interpreters' numpy builds.  So: float64 difference <= 1e-15 absolute (the
bound of the g12 gaussian test), and the float32 casts equal bit for bit on this fixture (checked when it was generated).
"""
import ctypes

import numpy as np
import pytest
import torch

import prn_train_ref as ref
from helpers import gold

G = gold("g18_prn_train.npz")
THR = float(G["threshold"])
NK = int(G["num_of_keypoints"])
ORDER = [int(i) for i in G["order"]]
COEFFS = (1, 2, 3)


def annotations():
    return [{"bbox": [float(v) for v in G["bbox"][i]], "keypoints": [float(v) for v in G["keypoints"][i]], "image_id": int(G["image_id"][i]),
             "iscrowd": int(G["iscrowd"][i]), "num_keypoints": int(G["num_keypoints"][i])} for i in range(G["bbox"].shape[0])]


def sample_args(s):
    i = ORDER[s]
    rows = ref.image_rows(G["image_id"], i)
    return G["bbox"][i], G["keypoints"][i], G["keypoints"][rows]


def raising(coeff):
    return {s: str(e) for s, e in enumerate(G["exc_%d" % coeff]) if str(e)}


def test_fixture_covers_the_cases_it_was_built_for():
    assert len(set(G["image_id"].tolist())) == 2 and int((G["image_id"] == 202).sum()) == 1
    assert int(G["iscrowd"].sum()) == 1 and int((G["num_keypoints"] <= NK).sum()) >= 1
    assert len(ORDER) == 10 and G["bbox"].shape[0] == 12
    nk = G["num_keypoints"][ORDER]
    assert np.all(np.diff(nk) <= 0) and len(set(nk.tolist())) < len(nk)             # descending, with ties
    for c in COEFFS:
        names = sorted(raising(c).values())
        assert names == ["IndexError", "IndexError", "ZeroDivisionError", "ZeroDivisionError"]
    assert set(np.unique(G["keypoints"].reshape(-1, 17, 3)[..., 2]).tolist()) == {0.0, 1.0, 2.0}
    assert np.any(G["keypoints"] != np.round(G["keypoints"]))
    assert np.any((G["bbox"][:, 2] > 0) & (G["bbox"][:, 2] < 1)) and np.any(G["bbox"][:, 2] == 0)


@pytest.mark.parametrize("coeff", COEFFS)
def test_restatement_equals_the_real_reference(coeff):
    bad = raising(coeff)
    worst, mism, total = 0.0, 0, 0
    for s in range(len(ORDER)):
        if s in bad:
            continue
        w, o = ref.get_data(*sample_args(s), coeff=coeff, threshold=THR)
        gw, go = G["weights_%d" % coeff][s], G["output_%d" % coeff][s]
        assert w.shape == gw.shape == (28 * coeff, 18 * coeff, 17) and w.dtype == np.float64
        worst = max(worst, float(np.abs(w - gw).max()), float(np.abs(o - go).max()))
        mism += int((w.astype(np.float32).view(np.int32) != gw.astype(np.float32).view(np.int32)).sum())
        mism += int((o.astype(np.float32).view(np.int32) != go.astype(np.float32).view(np.int32)).sum())
        total += 2 * w.size
        assert gw.max() > 0.1 and go.max() > 0.01
    print("coeff %d: max float64 difference %.3e, float32 mismatches %d of %d" % (coeff, worst, mism, total))
    assert worst <= 1e-15
    assert mism == 0


@pytest.mark.parametrize("coeff", COEFFS)
def test_raising_samples(coeff):
    from multiposenet.pytorch_amd.datasets import PRNSampleSet
    bad = raising(coeff)
    for s, name in bad.items():
        with pytest.raises(Exception) as ei:
            ref.get_data(*sample_args(s), coeff=coeff, threshold=THR)
        assert type(ei.value).__name__ == name
        assert not G["weights_%d" % coeff][s].any() and not G["output_%d" % coeff][s].any()
    ss = PRNSampleSet(annotations(), NK, coeff=coeff, threshold=THR)
    assert ss.would_raise == sorted(bad) and ss.raise_names == bad
    assert len(ss) == len(ORDER) - len(bad) and ss.valid.tolist() == [s for s in range(len(ORDER)) if s not in bad]
    with pytest.raises(ValueError) as ei:
        PRNSampleSet(annotations(), NK, coeff=coeff, threshold=THR, strict=True)
    for s in bad:
        assert "(%d, %d, '%s')" % (s, ORDER[s], bad[s]) in str(ei.value)


def test_sample_order_is_get_anns_order_ties_included():
    from multiposenet.pytorch_amd.datasets import PRNSampleSet
    ss = PRNSampleSet(annotations(), NK)
    assert ss.order.tolist() == ORDER
    assert ref.get_anns(G["iscrowd"].tolist(), G["num_keypoints"].tolist(), NK) == ORDER
    # image grouping: every sample sees all annotations of its image, in file order
    for s, i in enumerate(ORDER):
        rows = ref.image_rows(G["image_id"], i)
        got = ss.img_kp[ss.img_start[s]: ss.img_start[s] + ss.img_count[s]]
        assert np.array_equal(got.reshape(-1, 51), G["keypoints"][rows])


def test_would_raise_agrees_with_the_restatement_on_random_annotations():
    """The vectorised search of PRNSampleSet against get_data run sample by sample, on boxes with negative and fractional
    corners and keypoints far outside them (so that the input-side IndexError cases occur too)."""
    from multiposenet.pytorch_amd.datasets import PRNSampleSet
    rs = np.random.RandomState(5)
    seen = set()
    for coeff in COEFFS:
        anns = []
        for i in range(60):
            w, h = rs.choice([0.0, 0.4, 1.0, 3.7, 20.0, 55.5]), rs.choice([0.0, 0.9, 1.0, 2.5, 30.0, 80.2])
            x, y = rs.uniform(-3, 40), rs.uniform(-3, 40)
            kp = np.zeros((17, 3))
            kp[:, 0] = x + w * rs.uniform(-2.5, 3.0, 17)
            kp[:, 1] = y + h * rs.uniform(-2.5, 3.0, 17)
            kp[:, 2] = rs.choice([0, 1, 2], 17)
            anns.append({"bbox": [x, y, w, h], "keypoints": kp.reshape(-1).tolist(), "image_id": int(i % 7), "iscrowd": int(i % 11 == 0),
                         "num_keypoints": int(rs.randint(0, 18))})
        ss = PRNSampleSet(anns, NK, coeff=coeff, threshold=0.9)           # a wide margin lets far keypoints through to the chain
        kps = np.array([a["keypoints"] for a in anns])
        img = [a["image_id"] for a in anns]
        want = {}
        for s, i in enumerate(ss.order.tolist()):
            try:
                ref.get_data(anns[i]["bbox"], kps[i], kps[ref.image_rows(img, i)], coeff=coeff, threshold=0.9)
            except (IndexError, ZeroDivisionError) as e:
                want[s] = type(e).__name__
        assert ss.raise_names == want
        seen.update(want.values())
    assert seen == {"IndexError", "ZeroDivisionError"}


def _differs(fault, coeff, s):
    try:
        w, o = ref.get_data(*sample_args(s), coeff=coeff, threshold=THR, fault=fault)
    except Exception:
        return True
    gw, go = G["weights_%d" % coeff][s], G["output_%d" % coeff][s]
    return bool(np.abs(w - gw).max() > 1e-15 or np.abs(o - go).max() > 1e-15 or
                np.any(w.astype(np.float32) != gw.astype(np.float32)) or np.any(o.astype(np.float32) != go.astype(np.float32)))


@pytest.mark.parametrize("fault", ref.FAULTS)
def test_modelled_faults_fail_the_comparison(fault):
    hit = [(c, s) for c in COEFFS for s in range(len(ORDER)) if s not in raising(c) and _differs(fault, c, s)]
    print("%s: caught on (coeff, sample) %s" % (fault, hit))
    assert hit, "fault %r passes the fixture comparison on every sample" % fault


def test_product_taps_are_scipys():
    from multiposenet.pytorch_amd.datasets import prn_data
    assert np.array_equal(prn_data.TAPS9, ref.gaussian_taps(1.0)) and np.array_equal(prn_data.TAPS17, ref.gaussian_taps(2.0))
    assert prn_data.TAPS9.shape == (9,) and prn_data.TAPS17.shape == (17,)
    assert np.abs(prn_data.TAPS9 - G["taps9"]).max() <= 1e-15 and np.abs(prn_data.TAPS17 - G["taps17"]).max() <= 1e-15
    from scipy.ndimage import gaussian_filter
    rs = np.random.RandomState(1)
    m = (rs.uniform(size=(28, 18)) < 0.02).astype(np.float64)
    assert np.array_equal(ref.blur(m, prn_data.TAPS9, "nearest"), gaussian_filter(m, 1.0, mode="nearest", truncate=4.0))
    assert np.array_equal(ref.blur(m, prn_data.TAPS17, "constant"), gaussian_filter(m, 2.0, mode="constant", cval=0, truncate=4.0))


def test_entry_point_rejects_bad_arguments_without_a_device():
    from multiposenet.pytorch_amd import _lib
    L = _lib.lib()
    BAD = -2
    nul, p8, p4, odd = ctypes.c_void_p(None), ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1004), ctypes.c_void_p(0x1002)

    def go(box=p8, own=p8, img=p8, off=p8, B=2, P=3, coeff=2, t9=p8, t17=p8, inp=p8, lab=p8, err=p8):
        return L.mpn_prn_train_maps(box, own, img, off, B, P, coeff, 0.21, t9, t17, inp, lab, err, nul)
    for name in ("box", "own", "img", "off", "t9", "t17", "inp", "lab", "err"):
        assert go(**{name: nul}) == BAD, name
        assert go(**{name: odd}) == BAD, name
    for name in ("box", "own", "img", "t9", "t17"):                     # doubles need 8-byte alignment
        assert go(**{name: p4}) == BAD, name
    assert go(B=0) == BAD and go(B=-1) == BAD and go(P=-1) == BAD
    assert go(coeff=0) == BAD and go(coeff=4) == BAD


def test_batcher_has_no_cpu_path():
    from multiposenet.pytorch_amd._lib import MpnError
    from multiposenet.pytorch_amd.datasets import DevicePRNBatcher
    with pytest.raises(MpnError):
        DevicePRNBatcher(device="cpu")
    if not torch.cuda.is_available():
        with pytest.raises(MpnError):
            DevicePRNBatcher()
    with pytest.raises(MpnError):
        DevicePRNBatcher(coeff=4)


def test_loader_batches_len_and_seeded_permutation():
    from multiposenet.pytorch_amd._lib import MpnError
    from multiposenet.pytorch_amd.datasets import PRNDeviceLoader, PRNSampleSet
    ss = PRNSampleSet(annotations(), NK)
    assert len(ss) == 6

    def echo(sampleset, idx):
        return list(idx)
    ld = PRNDeviceLoader(ss, echo, 4, shuffle=False)
    assert len(ld) == 2 and list(ld) == [[0, 1, 2, 3], [4, 5]]
    ld = PRNDeviceLoader(ss, echo, 4, shuffle=False, drop_last=True)
    assert len(ld) == 1 and list(ld) == [[0, 1, 2, 3]]
    a, b, c = (PRNDeviceLoader(ss, echo, 4, seed=sd) for sd in (3, 3, 4))
    pa, pb, pc = [list(a), list(a)], [list(b), list(b)], [list(c), list(c)]
    assert pa == pb and pa != pc
    assert pa[0] != pa[1]                                                # a new permutation per pass, from the same generator
    for p in pa:
        assert len(p) == 2 and sorted(i for batch in p for i in batch) == list(range(6))
    ld = PRNDeviceLoader(ss, echo, 2, seed=1, indices=[5, 1, 3])
    assert len(ld) == 2 and sorted(i for batch in ld for i in batch) == [1, 3, 5]
    with pytest.raises(MpnError):
        PRNDeviceLoader(ss, echo, 2, indices=[6])
    with pytest.raises(MpnError):
        PRNDeviceLoader(ss, echo, 0)
