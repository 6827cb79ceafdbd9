"""GPU tests of the PRN training pairs rendered on the device (csrc/prn_targets.hip through datasets/prn_data.py).

Expectations, none of them taken from what the kernel returns:
* against tests/prn_train_ref.py evaluated here with the SAME tap vectors the product hands the kernel: bit-for-bit equality of the
  float32 cast.  The float64 operations and their order are the same on both sides and the kernel is built without contraction.
* against tests/golden/g18_prn_train.npz (the real reference with real scikit-image, another numpy build): the taps differ by a
  float64 ulp, so every element is equal or the adjacent float32, and at most 1e-5 of all elements are not bit-equal.
* a sample's maps do not depend on its batch; raising samples have zero maps and a set error word.
"""
import numpy as np
import pytest
import torch

import prn_train_ref as ref
from helpers import report
from test_prn_train_cpu import G, NK, ORDER, THR, annotations, raising, sample_args

pytestmark = pytest.mark.gpu

COEFFS = (1, 2, 3)
S = len(ORDER)


def _render(coeff, batch):
    from multiposenet.pytorch_amd.datasets import DevicePRNBatcher, PRNSampleSet
    ss = PRNSampleSet(annotations(), NK, coeff=coeff, threshold=THR)
    bt = DevicePRNBatcher(coeff=coeff, threshold=THR)
    inp, lab, err = [], [], []
    for s0 in range(0, S, batch):
        i, l, e = bt.render(ss, list(range(s0, min(S, s0 + batch))), raw=True)
        assert i.dtype == l.dtype == torch.float32 and i.is_contiguous() and l.is_contiguous() and e.dtype == torch.int32
        assert tuple(i.shape) == tuple(l.shape) == (min(S, s0 + batch) - s0, 28 * coeff, 18 * coeff, 17)
        inp.append(i); lab.append(l); err.append(e)
    torch.cuda.synchronize()
    return torch.cat(inp), torch.cat(lab), torch.cat(err)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


@pytest.mark.parametrize("coeff", COEFFS)
def test_maps_vs_restatement_fixture_and_batch_independence(coeff):
    from multiposenet.pytorch_amd.datasets import prn_data
    inp, lab, err = _render(coeff, S)
    for batch in (1, 5):
        i2, l2, e2 = _render(coeff, batch)
        assert torch.equal(i2, inp) and torch.equal(l2, lab) and torch.equal(e2, err), "batch size %d changes a sample's maps" % batch
    inp, lab, err = inp.cpu().numpy(), lab.cpu().numpy(), err.cpu().numpy()
    bad = raising(coeff)
    codes = {"IndexError": 1, "ZeroDivisionError": 2}
    assert err.tolist() == [codes[bad[s]] if s in bad else 0 for s in range(S)]
    n_el, n_ne = 0, 0
    for s in range(S):
        gw, go = G["weights_%d" % coeff][s].astype(np.float32), G["output_%d" % coeff][s].astype(np.float32)
        if s in bad:
            assert not inp[s].any() and not lab[s].any() and not gw.any() and not go.any()
            continue
        w, o = ref.get_data(*sample_args(s), coeff=coeff, threshold=THR, taps9=prn_data.TAPS9, taps17=prn_data.TAPS17)
        dw, do = int((_bits(inp[s]) != _bits(w)).sum()), int((_bits(lab[s]) != _bits(o)).sum())
        print("coeff %d sample %d: vs restatement %d + %d elements differ; max |input| %.4f max |label| %.4f" % (
            coeff, s, dw, do, inp[s].max(), lab[s].max()))
        assert dw == 0 and do == 0, "coeff %d sample %d: %d input / %d label elements differ from the float64 restatement" % (coeff, s, dw, do)
        for got, want in ((inp[s], gw), (lab[s], go)):
            ne = _bits(got) != _bits(want)
            n_el += got.size
            n_ne += int(ne.sum())
            nxt = (got == np.nextafter(want, np.float32(np.inf))) | (got == np.nextafter(want, np.float32(-np.inf)))
            assert np.all(~ne | nxt), "an element is neither the fixture's float32 nor its neighbour"
        assert inp[s].max() > 0.1 and lab[s].max() > 0.01
    report("prn_train_maps coeff %d: bit-equal to the float64 restatement; vs real skimage %d of %d elements on the adjacent float32" % (
        coeff, n_ne, n_el))
    print("coeff %d: vs fixture %d of %d elements not bit-equal" % (coeff, n_ne, n_el))
    assert n_ne <= 1e-5 * n_el


def test_one_batcher_call_is_one_library_launch():
    from multiposenet.pytorch_amd import _lib
    from multiposenet.pytorch_amd.datasets import DevicePRNBatcher, PRNSampleSet
    ss = PRNSampleSet(annotations(), NK)
    bt = DevicePRNBatcher()
    bt(ss, [0, 1])                                    # loads the library outside the observed call
    assert _lib.TAPE is None
    _lib.TAPE = tape = []
    try:
        inp, lab = bt(ss, list(range(len(ss))))
    finally:
        _lib.TAPE = None
    assert len(tape) == 1 and tape[0][2] is True and tape[0][0].__name__ == "mpn_prn_train_maps"
    assert bt.err is not None and not bt.err.any() and tuple(inp.shape) == (len(ss), 56, 36, 17)


def _valid_fixture_batch(coeff=2):
    ok = [s for s in range(S) if s not in raising(coeff)]
    x = torch.from_numpy(G["weights_%d" % coeff][ok].astype(np.float32)).cuda()
    y = torch.from_numpy(G["output_%d" % coeff][ok].astype(np.float32)).cuda()
    return ok, x, y


def test_prn_forward_on_device_batch_equals_forward_on_uploaded_fixture():
    from multiposenet.pytorch_amd.datasets import DevicePRNBatcher, PRNSampleSet
    from test_model_gpu import get_model
    ok, x, y = _valid_fixture_batch()
    ss = PRNSampleSet(annotations(), NK, threshold=THR)
    assert ss.valid.tolist() == ok
    inp, lab = DevicePRNBatcher(threshold=THR)(ss, list(range(len(ss))))
    model = get_model(50, torch.float32)
    model.eval()
    with torch.no_grad():
        a, _ = model([inp, "prn_subnet"])
        b, _ = model([x, "prn_subnet"])
    assert tuple(a.shape) == (len(ok), 56, 36, 17) and torch.isfinite(a).all() and torch.equal(a, b)
    assert torch.equal(lab, y)


class _State(object):
    pass


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_loader_batches_train_the_prn(dtype):
    """PRNDeviceLoader -> batch_processor ('prn_subnet': no copy) -> train_step: a finite loss, and the PRN's parameters move."""
    from multiposenet.pytorch_amd.datasets import DevicePRNBatcher, PRNDeviceLoader, PRNSampleSet
    from multiposenet.pytorch_amd.optim import FusedAdam
    from multiposenet.pytorch_amd.training.batch_processor import batch_processor, train_step
    from test_model_gpu import get_model
    ss = PRNSampleSet(annotations(), NK, threshold=THR)
    loader = PRNDeviceLoader(ss, DevicePRNBatcher(threshold=THR), 4, seed=2)
    assert len(loader) == 2
    model = get_model(50, dtype)
    for n, p in model.named_parameters():
        p.requires_grad = n.startswith("prn.")
    model.train()
    st = _State(); st.model = model; st.params = _State(); st.params.subnet_name = "prn_subnet"; st.params.gpus = [0]
    opt = FusedAdam(model, lr=1e-3)
    before = model.prn.dens1.weight.detach().clone()
    sizes = []
    for batch in loader:
        inp, lab = batch
        assert inp.is_cuda and inp.dtype == torch.float32 and tuple(inp.shape[1:]) == (56, 36, 17)
        inputs, gts, _ = batch_processor(st, batch)
        assert inputs[0][0].data_ptr() == inp.data_ptr() and gts[1].data_ptr() == lab.data_ptr()
        loss, log = train_step(model, opt, inputs, gts)
        assert np.isfinite(float(loss.detach())) and float(loss.detach()) > 0
        sizes.append(int(inp.shape[0]))
    torch.cuda.synchronize()
    assert sorted(sizes) == [2, 4]
    after = model.prn.dens1.weight.detach()
    assert torch.isfinite(after).all() and not torch.equal(before, after)
    for p in model.parameters():
        p.requires_grad = True
