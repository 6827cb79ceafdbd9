"""GPU tests of the detection loader's device augmentation (csrc/augment.hip: mpn_augment_boxes through datasets/augment.py:
boxes_from_rects, DeviceBBoxAugmenter, DeviceAugmenter.call_with_boxes).

PARITY.  Every device box against the float64 restatement tests/augment_bbox_ref.py: each pixel of the (S + 1)^2 mask frame has a
float64 value and the element-wise float32 bound of augment_ref (C_SUM_BOX = 9 roundings of the 16-term sum, W_ABS = 374 for the
float32 weights; both from operation counts).  Pixels above 0.5 by more than the bound are surely ON and give the INNER box, those
within the bound of 0.5 are undecided and widen it to the OUTER box; a device coordinate must lie between the two and must be EQUAL
where they agree (the -1 rows included).  Undecided coordinates may not carry the suite: at most 1 % of its coordinates may be
undecided (test_undecided_coordinates_are_rare).  The geometry of the golden cases comes from tests/golden/g19_augment_bbox.npz,
recorded from the reference's real aug_*_bbox functions, never from the product's host code.
"""
import numpy as np
import pytest
import torch

import augment_bbox_ref as br
import augment_ref as ar

pytestmark = pytest.mark.gpu

CASES, INP, STRIDE, G = br.golden()
N_SHAPES = 7
_REF = {}


def _shapes(i):
    c = CASES[i]
    return br.instance_shapes(900 + i, int(c["hw"][0]), int(c["hw"][1]))


def _truth(i):
    """(inner rows, outer rows) [7, 5] of golden case i at S = 480, computed once and shared."""
    if i not in _REF:
        geo = br.case_geo(CASES[i])
        io = [br.inner_outer(m, geo, INP)[:2] for m in _shapes(i)]
        _REF[i] = (np.stack([a for a, _ in io]), np.stack([b for _, b in io]))
    return _REF[i]


def _golden_sample(i):
    c = CASES[i]
    img = br.synth_image(40 + i, int(c["hw"][0]), int(c["hw"][1]))
    return {"img": torch.from_numpy(img), "objpos": c["objpos_in"], "scale_provided": float(c["scale_provided"]),
            "instances": [torch.from_numpy(m) for m in _shapes(i)], "iscrowd": [0] * N_SHAPES}


def _check_rows(got, inner, outer, what):
    und = 0
    for r in range(inner.shape[0]):
        ok, u = br.check_row(got[r], inner[r], outer[r])
        print("%s row %d: device %s inner %s outer %s" % (what, r, got[r].tolist(), inner[r].tolist(), outer[r].tolist()))
        assert ok, "%s row %d: device %s not within inner %s / outer %s" % (what, r, got[r], inner[r], outer[r])
        und += u
    return und


# ---- 1. kernel against the restatement ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("i", range(len(CASES)))
def test_boxes_vs_float64_restatement_on_golden_geometry(i):
    from multiposenet.pytorch_amd.datasets.augment import DeviceBBoxAugmenter
    c = CASES[i]
    da = DeviceBBoxAugmenter(INP, STRIDE, ar.case_params(c))
    img, bbox, metas = da([_golden_sample(i)], dice=c["dice"][None])
    assert bbox.is_cuda and bbox.dtype == torch.float32 and bbox.is_contiguous() and tuple(bbox.shape) == (1, N_SHAPES, 5)
    inner, outer = _truth(i)
    _check_rows(bbox[0].cpu().numpy(), inner, outer, "case %d" % i)


def test_undecided_coordinates_are_rare():
    """A coordinate with inner != outer passes on an interval, not on a value: at most 1 % of the suite's coordinates may do so."""
    total = und = 0
    for i in range(len(CASES)):
        inner, outer = _truth(i)
        total += 4 * inner.shape[0]
        und += int(np.sum(inner[:, :4] != outer[:, :4]))
    print("undecided coordinates: %d of %d; rows warped out entirely: %d" % (und, total, sum(int((_truth(i)[0][:, 4] < 0).sum()) for i in range(len(CASES)))))
    assert total == 4 * N_SHAPES * len(CASES) and und <= 0.01 * total


# ---- 2. small shapes, where tiling goes wrong -----------------------------------------------------------------------------------

def _blob(H, W, y0, y1, x0, x1):
    m = np.zeros((H, W), dtype=np.uint8)
    m[y0:y1, x0:x1] = 1
    return m


def _small_batch(S):
    """B = 3 on 50 x 70 / 53 x 67 / 50 x 70 sources with 5, 1 and 0 non-crowd instances (the last sample: a crowd only)."""
    H, W = 50, 70
    yy, xx = np.mgrid[0:H, 0:W]
    inst0 = [_blob(H, W, 0, 6, 0, 9),                                            # touches the source's corner
             _blob(H, W, 44, 50, 63, 70),                                        # the opposite corner: outside the crop at S = 64
             (((yy - 20) / 9.0) ** 2 + ((xx - 25) / 14.0) ** 2 < 1).astype(np.uint8),
             _blob(H, W, 10, 40, 33, 34),                                        # one-pixel-wide line
             _blob(H, W, 27, 28, 18, 19)]                                        # single pixel
    s0 = {"img": torch.from_numpy(br.synth_image(1, H, W)), "objpos": (20.0, 16.0), "scale_provided": 0.6 if S == 64 else 0.3,
          "instances": inst0, "iscrowd": [0, 0, 0, 0, 0]}
    H1, W1 = 53, 67
    yy, xx = np.mgrid[0:H1, 0:W1]
    s1 = {"img": torch.from_numpy(br.synth_image(2, H1, W1)), "objpos": (30.0, 30.0), "scale_provided": 0.6 if S == 64 else 0.3,
          "instances": [np.zeros((H1, W1), dtype=np.uint8), (((yy - 28) / 15.0) ** 2 + ((xx - 36) / 11.0) ** 2 < 1)], "iscrowd": [0, 0]}
    s2 = {"img": torch.from_numpy(br.synth_image(3, H, W)), "objpos": (35.0, 25.0), "scale_provided": 0.6,
          "instances": [np.ones((H, W), dtype=np.uint8)], "iscrowd": [1]}
    # dice: scale, scale2, rotate, crop x, crop y, flip (flip_prob 0.3: the second sample is flipped)
    dice = np.array([[0.2, 0.9, 0.8, 0.4, 0.6, 0.9], [0.5, 0.3, 0.1, 0.7, 0.2, 0.1], [0.3, 0.5, 0.5, 0.5, 0.5, 0.9]])
    return [s0, s1, s2], dice


@pytest.mark.parametrize("S", [64, 130])
def test_small_shapes_ragged_tiles_crowds_and_padding(S):
    from multiposenet.pytorch_amd.datasets.augment import DeviceBBoxAugmenter
    samples, dice = _small_batch(S)
    da = DeviceBBoxAugmenter(S, 4, dict(center_perterb_max=10))
    img, bbox, metas = da(samples, dice=dice)
    assert tuple(bbox.shape) == (3, 5, 5) and tuple(img.shape) == (3, 3, S, S)
    assert [len(g["rects"]) for g in metas] == [5, 1, 0] and [g["flip"] for g in metas] == [False, True, False]
    got = bbox.cpu().numpy()
    for b in range(2):
        geo = br.product_geo(metas[b])
        masks = [m for m in samples[b]["instances"] if np.any(m)]
        io = [br.inner_outer(m, geo, S)[:2] for m in masks]
        inner, outer = np.stack([a for a, _ in io]), np.stack([o for _, o in io])
        assert _check_rows(got[b], inner, outer, "S %d sample %d" % (S, b)) == 0
        if b == 0:
            assert inner[0][4] == 0 and inner[2][4] == 0
            if S == 64:
                assert np.array_equal(inner[1], br.EMPTY)                      # entirely outside the crop: a -1 row that is NOT padding
    assert np.all(got[1, 1:] == -1) and np.all(got[2] == -1)                      # padding rows; the crowd-only image has none
    assert torch.isfinite(img).all()


# ---- 3. exact cases -------------------------------------------------------------------------------------------------------------

def test_exact_identity_transform_moves_the_mask_extents_by_the_crop_origin():
    """scale 1 (scale_provided = target_dist, scale_prob 0), 0 degrees, no flip: every fraction is 0, the weights are (0, 1, 0, 0),
    the frame shows the source mask itself.  Independent of the restatement.  The same sample flipped mirrors x over S + 1."""
    from multiposenet.pytorch_amd.datasets.augment import DeviceBBoxAugmenter, DEFAULT_PARAMS
    H, W, S = 200, 240, 96
    rects = [(60, 90, 70, 110), (100, 101, 120, 121), (20, 180, 5, 230), (0, 200, 0, 240)]          # y0, y1, x0, x1
    inst = [_blob(H, W, *r) for r in rects]
    s = {"img": torch.from_numpy(br.synth_image(5, H, W)), "objpos": (120.0, 100.0), "scale_provided": 0.6, "instances": inst,
         "iscrowd": [0] * len(inst)}
    da = DeviceBBoxAugmenter(S, 4, dict(DEFAULT_PARAMS, scale_prob=0.0))
    plain = np.array([[0.7, np.nan, 0.5, 0.5, 0.5, 0.9]])
    flipped = np.array([[0.7, np.nan, 0.5, 0.5, 0.5, 0.1]])
    _, bbox, metas = da([s], dice=plain)
    g = metas[0]
    assert g["scale"] == 1.0 and g["degree"] == 0.0 and not g["flip"] and (g["ox"], g["oy"]) == (120 - S // 2, 100 - S // 2)
    want = []
    for y0, y1, x0, x1 in rects:
        xa, xb = max(x0 - g["ox"], 0), min(x1 - g["ox"], S + 1)
        ya, yb = max(y0 - g["oy"], 0), min(y1 - g["oy"], S + 1)
        want.append([xa, ya, xb, yb, 0] if xa < xb and ya < yb else [-1] * 5)
    want = np.array(want, dtype=np.float32)
    got = bbox[0].cpu().numpy()
    assert np.array_equal(got, want), (got, want)
    assert want[3].tolist() == [0, 0, S + 1, S + 1, 0] and want[1].tolist() == [48, 48, 49, 49, 0] and bool((want[:, 4] == 0).all())
    _, fb, fm = da([s], dice=flipped)
    assert fm[0]["flip"]
    f = fb[0].cpu().numpy()
    mirrored = want.copy()
    mirrored[:, 0], mirrored[:, 2] = S + 1 - want[:, 2], S + 1 - want[:, 0]
    assert np.array_equal(f, mirrored), (f, mirrored)


# ---- 4. determinism and batch independence --------------------------------------------------------------------------------------

def test_rows_do_not_depend_on_batch_position_neighbours_or_launch():
    from multiposenet.pytorch_amd.datasets.augment import DeviceBBoxAugmenter
    samples, dice = _small_batch(64)
    da = DeviceBBoxAugmenter(64, 4, dict(center_perterb_max=10))
    s0, s1, s2 = samples
    _, a, _ = da([s0, s1, s2, s1], dice=dice[[0, 1, 2, 1]])
    _, b, _ = da([s1, s2, s0], dice=dice[[1, 2, 0]])
    _, a2, _ = da([s0, s1, s2, s1], dice=dice[[0, 1, 2, 1]])
    torch.cuda.synchronize()
    assert torch.equal(a, a2)
    assert torch.equal(a[0], b[2]) and torch.equal(a[1], b[0]) and torch.equal(a[3], b[0]) and torch.equal(a[1], a[3])
    assert float(a[0, 0, 4]) == 0.0


def _full_batch(B=32, H=480, W=640, n_inst=5):
    samples = []
    rs = np.random.RandomState(9)
    img = torch.from_numpy(br.synth_image(7, H, W))                    # the boxes do not depend on the pixels: one image serves all
    for b in range(B):
        masks = br.instance_shapes(300 + b, H, W)[:n_inst]
        samples.append({"img": img,
                        "objpos": (rs.uniform(100, 540), rs.uniform(100, 380)), "scale_provided": float(rs.uniform(0.3, 1.0)),
                        "instances": masks, "iscrowd": [0] * n_inst})
    return samples


def test_full_size_batch_is_deterministic():
    """B = 32, 480 x 480 from 640 x 480 sources, 5 instances each: two calls are byte-identical, a sub-batch equals its rows."""
    import random
    from multiposenet.pytorch_amd.datasets.augment import DeviceBBoxAugmenter, draw_dice
    samples = _full_batch()
    rng = random.Random(3)
    dice = np.stack([draw_dice(rng) for _ in samples])
    da = DeviceBBoxAugmenter(480, 4, row_multiple=8)
    img, a, _ = da(samples, dice=dice)
    img2, b, _ = da(samples, dice=dice)
    torch.cuda.synchronize()
    assert tuple(a.shape) == (32, 8, 5) and torch.equal(a, b) and torch.equal(img, img2)
    assert torch.isfinite(a).all() and bool((a[:, 5:] == -1).all()) and int((a[:, :5, 4] == 0).sum()) > 32
    sub = [3, 17, 31]
    _, c, _ = da([samples[k] for k in sub], dice=dice[sub])
    assert torch.equal(c, a[sub])


# ---- 5. rectangle upload against the full mask ----------------------------------------------------------------------------------

def test_rectangle_upload_equals_full_mask_upload():
    from multiposenet.pytorch_amd.datasets.augment import DeviceBBoxAugmenter, boxes_from_rects
    dev = torch.device("cuda", torch.cuda.current_device())
    for i in (0, 5):
        c = CASES[i]
        da = DeviceBBoxAugmenter(INP, STRIDE, ar.case_params(c))
        metas = da.geometry([_golden_sample(i)], dice=c["dice"][None])
        H, W = metas[0]["H"], metas[0]["W"]
        assert any((r[3], r[4]) != (W, H) for r in metas[0]["rects"])
        cropped, _ = boxes_from_rects([metas[0]["rects"]], metas, INP, 1, dev)
        full, _ = boxes_from_rects([[(r[0], 0, 0, W, H) for r in metas[0]["rects"]]], metas, INP, 1, dev)
        assert torch.equal(cropped, full) and int((cropped[0, :, 4] == 0).sum()) >= 4


# ---- 6. DeviceBBoxAugmenter end to end ------------------------------------------------------------------------------------------

def test_image_equals_augment_image_under_the_recorded_bbox_geometry():
    from multiposenet.pytorch_amd.datasets import augment as aug
    idx = [i for i, c in enumerate(CASES) if np.array_equal(c["params"], [0.8, 1.2, 1, 0.6, 40, 40, 0.3])]
    assert len(idx) >= 6
    da = aug.DeviceBBoxAugmenter(INP, STRIDE)
    samples = [_golden_sample(i) for i in idx]
    img, bbox, metas = da(samples, dice=np.stack([CASES[i]["dice"] for i in idx]))
    rows, srcs, off = [], [], 0
    for i, s in zip(idx, samples):
        H, W = int(CASES[i]["hw"][0]), int(CASES[i]["hw"][1])
        rows.append(aug.table_row(br.case_geo(CASES[i]), H, W, off, W * 3))
        srcs.append(s["img"].view(-1))
        off += H * W * 3
    want = aug.augment_image(torch.cat(srcs).cuda(), torch.from_numpy(np.stack(rows)).cuda(), INP, INP)
    assert img.dtype == torch.float32 and img.is_contiguous() and torch.equal(img, want)
    for b, i in enumerate(idx):
        inner, outer = _truth(i)
        _check_rows(bbox[b].cpu().numpy(), inner, outer, "batched case %d" % i)


class _State(object):
    pass


def _train_samples(H=120, W=160):
    out = []
    for b in range(2):
        masks = br.instance_shapes(500 + b, H, W)[:5]
        rs = np.random.RandomState(50 + b)
        j = np.zeros((17, 3))
        j[:, 0], j[:, 1], j[:, 2] = rs.uniform(0, W, 17), rs.uniform(0, H, 17), rs.choice([0.0, 1.0, 2.0], 17)
        img, mm = ar.synth_sources(60 + b, H, W)
        out.append({"img": torch.from_numpy(img), "mask_miss": torch.from_numpy(mm), "objpos": (80.0, 60.0), "scale_provided": 0.6,
                    "instances": masks, "iscrowd": [0, 0, 1, 0, 0], "joint_self": j})
    dice = np.array([[0.4, 0.5, 0.55, 0.5, 0.5, 0.9], [0.3, 0.2, 0.4, 0.6, 0.4, 0.1]])
    return out, dice


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_detection_batch_trains_a_detection_subnet_for_two_recorded_steps(dtype):
    """The pair goes through batch_processor without a copy and trains an R50 detection_subnet at 128 x 128: one eager step, then the
    recording and its replay; finite, non-increasing loss on the repeated batch.  With row_multiple = 8 the recorded step's
    annotation bucket has nothing left to pad."""
    from multiposenet.pytorch_amd.datasets.augment import DeviceBBoxAugmenter
    from multiposenet.pytorch_amd.optim import FusedAdam
    from multiposenet.pytorch_amd.replay import ReplayedTrainStep
    from multiposenet.pytorch_amd.training.batch_processor import batch_processor
    from test_model_gpu import get_model
    S = 128
    samples, dice = _train_samples()
    img, bbox, _ = DeviceBBoxAugmenter(S, 4, row_multiple=8)(samples, dice=dice)
    assert tuple(img.shape) == (2, 3, S, S) and tuple(bbox.shape) == (2, 8, 5) and int((bbox[:, :, 4] == 0).sum()) >= 4
    model = get_model(50, dtype)
    for p in model.prn.parameters():
        p.requires_grad = False
    model.train()
    st = _State(); st.model = model; st.params = _State(); st.params.subnet_name = 'detection_subnet'; st.params.gpus = [0]
    inputs, gts, _ = batch_processor(st, (img, bbox))
    assert inputs[0][0].data_ptr() == img.data_ptr() and gts[1].data_ptr() == bbox.data_ptr()          # no copy
    # the first step of a signature runs eagerly (it fills the host-side caches), the second is the recording, the third replays it
    step = ReplayedTrainStep(model, FusedAdam(model, lr=1e-4))
    loss = [float(step(inputs, gts)[0]) for _ in range(3)]
    torch.cuda.synchronize()
    print("detection_subnet %s: losses %s (replays %d)" % (dtype, loss, step.replays))
    assert step.replays == 1 and len(step._entries) == 1 and all(np.isfinite(v) for v in loss)
    assert loss[0] > 0 and loss[1] <= loss[0] and loss[2] <= loss[1]


def test_call_with_boxes_feeds_train_both():
    from multiposenet.pytorch_amd.datasets.augment import DeviceAugmenter
    from multiposenet.pytorch_amd.optim import FusedAdam
    from multiposenet.pytorch_amd.replay import ReplayedTrainStep
    from multiposenet.pytorch_amd.training.batch_processor import batch_processor
    from test_model_gpu import get_model
    S = 128
    samples, dice = _train_samples()
    da = DeviceAugmenter(S, 4)
    img, heat, hm, bbox, metas = da.call_with_boxes(samples, dice=dice)
    img0, heat0, hm0, metas0 = da(samples, dice=dice)                              # __call__ keeps its return value
    assert torch.equal(img, img0) and torch.equal(heat, heat0) and torch.equal(hm, hm0)
    assert tuple(bbox.shape) == (2, 4, 5)                                          # one crowd of five: four rows
    # the KEYPOINT chain's geometry (rotated objpos), through the same kernel
    got = bbox.cpu().numpy()
    for b in range(2):
        geo = br.product_geo(metas[b])
        masks = [m for m, c in zip(samples[b]["instances"], samples[b]["iscrowd"]) if not c]
        io = [br.inner_outer(m, geo, S)[:2] for m in masks]
        _check_rows(got[b], np.stack([a for a, _ in io]), np.stack([o for _, o in io]), "train_both sample %d" % b)
    model = get_model(50, torch.bfloat16)
    for p in model.prn.parameters():
        p.requires_grad = False
    model.train()
    st = _State(); st.model = model; st.params = _State(); st.params.subnet_name = 'train_both'; st.params.gpus = [0]
    inputs, gts, _ = batch_processor(st, (img, heat, hm, bbox))
    assert inputs[0][0].data_ptr() == img.data_ptr() and gts[3].data_ptr() == bbox.data_ptr() and gts[1].data_ptr() == heat.data_ptr()
    step = ReplayedTrainStep(model, FusedAdam(model, lr=1e-4))
    loss = [float(step(inputs, gts)[0]) for _ in range(3)]                          # eager, recording, replay
    torch.cuda.synchronize()
    print("train_both bf16: losses %s" % loss)
    assert step.replays == 1 and all(np.isfinite(v) for v in loss) and loss[0] > 0 and loss[1] <= loss[0] and loss[2] <= loss[1]


def test_no_rows_gives_the_collaters_empty_shape_and_padding_to_a_multiple():
    from multiposenet.pytorch_amd.datasets.augment import DeviceBBoxAugmenter
    samples, dice = _small_batch(64)
    crowd_only = [samples[2], samples[2]]
    _, bbox, _ = DeviceBBoxAugmenter(64, 4)(crowd_only, dice=dice[[2, 2]])
    assert tuple(bbox.shape) == (2, 0, 5) and bbox.is_cuda and bbox.dtype == torch.float32
    _, b8, _ = DeviceBBoxAugmenter(64, 4, dict(center_perterb_max=10), row_multiple=8)(samples, dice=dice)
    _, b1, _ = DeviceBBoxAugmenter(64, 4, dict(center_perterb_max=10))(samples, dice=dice)
    assert tuple(b8.shape) == (3, 8, 5) and torch.equal(b8[:, :5], b1) and bool((b8[:, 5:] == -1).all())


def test_row_whose_rectangle_leaves_the_source_or_the_buffer_is_nan_and_not_read():
    """The guard of the table row (never produced by the host wrapper): such an instance is not dereferenced, its row is NaN, its
    neighbours are untouched; a row map entry past the table is NaN as well."""
    from multiposenet.pytorch_amd.datasets import augment as aug
    samples, dice = _small_batch(64)
    metas = aug.DeviceBBoxAugmenter(64, 4, dict(center_perterb_max=10)).geometry(samples[:1], dice=dice[:1])
    g = metas[0]
    m, rx0, ry0, rw, rh = g["rects"][2]
    packed = torch.from_numpy(np.ascontiguousarray(m[ry0:ry0 + rh, rx0:rx0 + rw])).view(-1).cuda()

    def row(off, pitch, rect):
        r = np.zeros(aug.TB_COLS)
        r[:aug.T_COLS] = aug.table_row(g, g["H"], g["W"], 0, 0, off, pitch)
        r[aug.TB_RX0:] = rect
        return r
    good = row(0, rw, (rx0, ry0, rw, rh))
    table = np.stack([good,
                      row(16, rw, (rx0, ry0, rw, rh)),                 # the last rows would lie behind the buffer
                      row(0, rw - 1, (rx0, ry0, rw, rh)),              # pitch shorter than the rectangle
                      row(0, rw, (g["W"] - rw + 1, ry0, rw, rh)),      # rectangle leaves the source
                      row(-8, rw, (rx0, ry0, rw, rh)),                 # negative offset
                      good])
    rowmap = torch.tensor([0, 1, 2, 3, 4, 5, -1, 6], dtype=torch.int32).cuda()
    out = aug.augment_boxes(packed, torch.from_numpy(table).cuda(), rowmap, 1, 8, 64, 64)[0].cpu().numpy()
    want = br.inner_outer(m, br.product_geo(g), 64)[0]
    assert np.array_equal(out[0], want) and np.array_equal(out[5], want) and want[4] == 0
    assert np.isnan(out[1:5]).all() and np.all(out[6] == -1) and np.isnan(out[7]).all()


# ---- 7. bad inputs --------------------------------------------------------------------------------------------------------------

def test_bad_inputs_raise():
    from multiposenet.pytorch_amd._lib import MpnError
    from multiposenet.pytorch_amd.datasets.augment import DeviceBBoxAugmenter, DeviceAugmenter
    samples, dice = _small_batch(64)
    good, d = samples[0], dice[:1]
    da = DeviceBBoxAugmenter(64, 4, dict(center_perterb_max=10))
    da([good], dice=d)
    m = good["instances"]
    bad = [dict(good, instances=[torch.from_numpy(m[0]).cuda()] + m[1:]),              # a CUDA mask
           dict(good, instances=[m[0].astype(np.float32)] + m[1:]),                    # not uint8 / bool
           dict(good, instances=[torch.from_numpy(m[0]).to(torch.int16)] + m[1:]),
           dict(good, instances=[m[0][:-1]] + m[1:]),                                  # another size
           dict(good, instances=[m[0][None]] + m[1:]),                                 # not 2-dimensional
           dict(good, iscrowd=[0, 0, 0, 0]),                                           # iscrowd of another length
           dict(good, instances=[], iscrowd=[]),                                       # nothing to centre on
           dict(good, img=good["img"].float()),
           dict(good, objpos=(-5000.0, 10.0))]                                         # the reference's slices would wrap
    for s in bad:
        with pytest.raises(MpnError):
            da([s], dice=d)
    with pytest.raises(MpnError):
        da([good], dice=np.zeros((1, 5)))
    with pytest.raises(MpnError):
        DeviceAugmenter(64, 4).call_with_boxes([dict(good, joint_self=np.ones((17, 3)), instances=None)], dice=d)
