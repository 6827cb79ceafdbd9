"""Tester — the reference's inference drivers (``evaluate/tester.py``) over the MI355X path.

    tester = Tester(model, TestParams())                       # loads params.ckpt (HDF5), eval mode, frozen BN (:105-129)
    results = tester.infer_image(img, 'name.jpg')              # body of Tester.test() for one image (:200-239)
    results = tester.infer_image_multiscale(img, 'name.jpg', image_id)    # body of Tester.coco_eval() for one image (:143-175):
                                                                # 5 scales x {original, flipped} test-time augmentation

    results = tester.infer_image_multiscale_fused(img, 'name.jpg', image_id)   # the same dicts from 5 paired forwards and csrc/tta.hip
    results = tester.infer_images_multiscale(images, names, ids)   # ... over many images, post-processing under the next image's network

    results = tester.coco_eval(images)                         # :131-191 from decoded images on: results file in COCO order
    mean, std = tester.val()                                   # :515-543 validation-loss loop

``img`` is the decoded image the reference gets from ``cv2.imread(...).astype(np.float32)``: [H, W, 3] BGR, 0..255.  Decoding
and the COCO annotation tools (cv2.imread, pycocotools: tester.py:133-139,179-186) stay with the caller — neither library
exists in this image; the result files (:176-178, :243-245) are written here.  Everything between the decoded image and the result dicts runs on the device: OpenCV-rule resizes
(csrc/peaks.hip: mpn_resize), the network, heat-map averaging, peak extraction (network/joint_utils.py) and the PRN
assignment (prn_process.py).  ``cv2.resize`` is restated, not linked: parity with OpenCV is unpinned (no cv2 here), see
DESIGN.md.
"""
import ctypes
import json
import logging
import os

import numpy as np
import torch

from .. import ops
from .._lib import TtaScale, call
from ..network import net_utils
from ..network.joint_utils import get_joint_list
from .prn_process import prn_process

logger = logging.getLogger("multiposenet")

# COCO order of the 17 keypoints (tester.py:140) and the left/right swap of the 18 heat-map channels (tester.py:326-327)
COCO_ORDER = [0, 14, 13, 16, 15, 4, 1, 5, 2, 6, 3, 10, 7, 11, 8, 12, 9]
SWAP_HEAT = [0, 1, 5, 6, 7, 2, 3, 4, 11, 12, 13, 8, 9, 10, 15, 14, 17, 16]


class TestParams(object):
    """tester.py:85-103."""
    trunk = 'resnet101'
    coeff = 2
    in_thres = 0.21
    testdata_dir = './demo/test_images/'
    testresult_dir = './demo/output/'
    testresult_write_image = False
    testresult_write_json = False
    gpus = [0]
    ckpt = './demo/models/ckpt_baseline_resnet101.h5'
    coco_root = 'coco_root/'
    coco_result_filename = './extra/multipose_coco2017_results.json'
    inp_size = 480
    exp_name = 'multipose101'
    subnet_name = 'keypoint_subnet'
    batch_size = 32
    print_freq = 20
    gaussian_filt = False             # NMS(..., bool_gaussian_filt=True): smooth every up-sampled peak patch (sigma 3) before its arg-max
    category_ids = [1]                # detect_images / coco_eval_bbox: class index of the detection head -> COCO category id
    tta_fused = False                 # coco_eval: the fused, flip-paired test-time augmentation (infer_images_multiscale; same results)
    mask_thresh = 0.5                 # return_masks / person_masks / seg_eval: mask = 255 where the channel-18 plane > mask_thresh (not in the reference)
    nms_per_class = False             # detect_images / coco_eval_bbox: every (anchor, class) score is a candidate, NMS per class (not in the reference)


def resize(img, out_hw, cubic, inv_scale=None):
    """cv2.resize(img, (out_w, out_h), interpolation=INTER_CUBIC if cubic else INTER_LINEAR) for a CUDA float32 [H, W, C] tensor.
    ``inv_scale=(1/fy, 1/fx)`` selects OpenCV's ``fx/fy`` call form (``cv2.resize(img, None, fx=, fy=)``), which maps destination
    to source coordinates with exactly 1/f instead of src/dst (they differ whenever round(src * f) != src * f)."""
    H, W, C = img.shape
    Hd, Wd = int(out_hw[0]), int(out_hw[1])
    out = torch.empty((Hd, Wd, C), dtype=torch.float32, device=img.device)
    sy, sx = (0.0, 0.0) if inv_scale is None else (float(inv_scale[0]), float(inv_scale[1]))
    call("mpn_resize", ops.ptr(img), img.stride(0), img.stride(1), img.stride(2), H, W, C, ops.ptr(out), Hd, Wd, 1 if cubic else 0, sy, sx, ops.stream_ptr())
    return out


def _round_half_even(v):
    return int(np.rint(v))          # cv::saturate_cast<int> of a double = cvRound


def scale_geometry(h0, w0, dest_size, factor=32, basedon='min'):
    """The host arithmetic of crop_with_factor (tester.py:38-82) for an h0 x w0 image: (im_scale, h, w, padded h, padded w) — the
    scale that brings the chosen side to dest_size, the resized shape and its round-up to a multiple of `factor`."""
    base = {'min': min(h0, w0), 'max': max(h0, w0), 'w': w0, 'h': h0}.get(basedon, min(h0, w0))
    im_scale = float(dest_size) / base
    h, w = _round_half_even(h0 * im_scale), _round_half_even(w0 * im_scale)       # dsize = round(src * f)
    new_h, new_w = int(np.ceil(float(h) / factor)) * factor, int(np.ceil(float(w) / factor)) * factor
    return im_scale, h, w, new_h, new_w


def crop_with_factor(im, dest_size, factor=32, pad_val=0, basedon='min'):
    """tester.py:38-82 for a CUDA [H, W, C] tensor: scale so that the chosen side becomes dest_size (cv2.resize with fx = fy =
    scale, bilinear), pad bottom/right with pad_val to a multiple of `factor`.  Returns (padded, scale, unpadded shape)."""
    im_scale, h, w, new_h, new_w = scale_geometry(im.shape[0], im.shape[1], dest_size, factor, basedon)
    scaled = resize(im, (h, w), cubic=False, inv_scale=(1.0 / im_scale, 1.0 / im_scale))       # cv2.resize(im, None, fx=s, fy=s), tester.py:68
    padded = torch.full((new_h, new_w, im.shape[2]), float(pad_val), dtype=torch.float32, device=im.device)
    padded[:h, :w] = scaled
    return padded, im_scale, (h, w, im.shape[2])


def resnet_preprocess(image):
    """datasets/coco_data/preprocessing.py:14-25 on the device: BGR 0..255 [H,W,3] -> RGB, /255, ImageNet mean/std, [3,H,W]."""
    img = image.float() / 255.
    img = img.flip(2)
    mean = torch.tensor([0.485, 0.456, 0.406], dtype=torch.float32, device=img.device)
    std = torch.tensor([0.229, 0.224, 0.225], dtype=torch.float32, device=img.device)
    return ((img - mean) / std).permute(2, 0, 1).contiguous()


def tta_input(img, h, w, hp, wp, inv_scale):
    """mpn_tta_input: float32 [2, 3, hp, wp], ``resnet_preprocess(crop_with_factor(x, ..., pad_val=128)[0])`` for x = img (image 0) and
    x = img.flip(1) (image 1) in one launch; (h, w, hp, wp) and inv_scale = 1 / im_scale from ``scale_geometry``.  img: CUDA float32
    [H, W, 3] BGR 0..255, any strides."""
    x = torch.empty((2, 3, hp, wp), dtype=torch.float32, device=img.device)
    call("mpn_tta_input", ops.ptr(img), img.stride(0), img.stride(1), img.stride(2), int(img.shape[0]), int(img.shape[1]), ops.ptr(x), h, w, hp, wp,
         float(inv_scale), ops.stream_ptr())
    return x


def tta_upsample(heat, rh, rw):
    """The pair map of one scale: heat [2, 18, hq, wq] read as one 36-channel image, the first rh x rw of its x4 INTER_CUBIC map (scale
    1/4 exactly, which is what the dsize form gives for the whole map) -> float32 [rh, rw, 36].  One mpn_resize."""
    if heat.stride(0) != 18 * heat.stride(1):
        heat = heat.contiguous()
    u = torch.empty((rh, rw, 36), dtype=torch.float32, device=heat.device)
    call("mpn_resize", ops.ptr(heat), heat.stride(2), heat.stride(3), heat.stride(1), int(heat.shape[2]), int(heat.shape[3]), 36, ops.ptr(u), rh, rw, 1,
         0.25, 0.25, ops.stream_ptr())
    return u


def tta_merge(pair_maps, H, W, swap=SWAP_HEAT):
    """mpn_tta_merge: the averaged float32 [H, W, 18] maps from the pair maps ([rh, rw, 36], channel stride 1, pixel stride 36) of every
    scale — both ``_get_outputs`` accumulations, ``_handle_heat`` and the final ``.float()`` in one launch."""
    n = len(pair_maps)
    table = (TtaScale * max(n, 1))()
    for s, u in enumerate(pair_maps):
        if u.dtype != torch.float32 or u.shape[2] != 36 or u.stride(2) != 1 or u.stride(1) != 36:
            raise ValueError("pair map %d: float32 [rh, rw, 36] with dense pixels expected" % s)
        table[s].u, table[s].rh, table[s].rw, table[s].pitch = u.data_ptr(), int(u.shape[0]), int(u.shape[1]), int(u.stride(0))
    out = torch.empty((H, W, 18), dtype=torch.float32, device=pair_maps[0].device)
    call("mpn_tta_merge", table, n, (ctypes.c_int32 * 18)(*swap), ops.ptr(out), H, W, ops.stream_ptr())
    return out


def _thr32(thr):
    return float(np.float32(thr))       # the threshold is a float32: the same value for the tensor library's compare and the kernels


def _mask_views(sizes, dev):
    """One uint8 buffer for the H x W masks of ``sizes``, every plane starting on a 16-byte boundary, pitch W -> (buffer, offsets, views)."""
    from ..datasets.augment import _aligned_offsets
    offsets, total = _aligned_offsets([int(H) * int(W) for H, W in sizes])
    buf = torch.empty(max(total, 16), dtype=torch.uint8, device=dev)
    return buf, offsets, [buf[o:o + int(H) * int(W)].view(int(H), int(W)) for o, (H, W) in zip(offsets, sizes)]


def seg_masks(heat, geometry, thr, planes=False):
    """mpn_seg_masks: the person masks of a single-scale batch in one launch.  heat: float32 CUDA [B, 19, hq, wq] maps of a person_seg
    model (any positive strides; channel 18 is read in place); geometry: the (H, W) of every image — it was zero-padded to D x D,
    D = max(H, W), before the resize to the network input.  -> list of uint8 [H, W] masks (views of one buffer, 16-byte-aligned starts,
    pitch W), 255 where ``resize(q[:, :, None], (D, D), cubic=True)[:H, :W, 0] > thr``; with ``planes`` also the list of those float32
    planes."""
    B = int(heat.shape[0])
    if heat.dtype != torch.float32 or heat.dim() != 4 or heat.shape[1] < 19 or len(geometry) != B or B < 1:
        raise ValueError("seg_masks: float32 [B, 19, hq, wq] maps and one (H, W) per image expected")
    if min(heat.stride(2), heat.stride(3)) <= 0 or (B > 1 and heat.stride(0) <= 0):
        raise ValueError("seg_masks: maps with positive strides expected")
    sizes = [(int(H), int(W)) for H, W in geometry]
    buf, offsets, views = _mask_views(sizes, heat.device)
    q = heat[:, 18]
    table = np.zeros((B, 7), dtype=np.int64)
    poff = 0
    for b, ((H, W), off) in enumerate(zip(sizes, offsets)):
        table[b] = (b * heat.stride(0), max(H, W), H, W, off, W, poff)
        poff += H * W
    pl = torch.empty(poff, dtype=torch.float32, device=heat.device) if planes else None
    hq, wq = int(heat.shape[2]), int(heat.shape[3])
    span = (B - 1) * heat.stride(0) + (hq - 1) * heat.stride(2) + (wq - 1) * heat.stride(3) + 1
    d_table = torch.from_numpy(table).to(heat.device)
    call("mpn_seg_masks", ops.ptr(q), heat.stride(2), heat.stride(3), hq, wq, span, ops.ptr(d_table), B, max(W for _, W in sizes),
         max(H for H, _ in sizes), _thr32(thr), ops.ptr(buf), buf.numel(), ops.ptr(pl) if planes else None, poff if planes else 0,
         ops.stream_ptr())
    if not planes:
        return views
    return views, [pl[o:o + H * W].view(H, W) for o, (H, W) in zip(table[:, 6].tolist(), sizes)]


def tta_seg_upsample(heat, rh, rw):
    """The seg pair map of one scale: channel 18 of heat [2, 19, hq, wq], read in place as one two-channel image (channel stride =
    heat.stride(0)), the first rh x rw of its x4 INTER_CUBIC map -> float32 [rh, rw, 2].  One mpn_resize."""
    u = torch.empty((rh, rw, 2), dtype=torch.float32, device=heat.device)
    call("mpn_resize", ops.ptr(heat[:, 18]), heat.stride(2), heat.stride(3), heat.stride(0), int(heat.shape[2]), int(heat.shape[3]), 2, ops.ptr(u),
         rh, rw, 1, 0.25, 0.25, ops.stream_ptr())
    return u


def tta_merge_mask(seg_pair_maps, H, W, thr, plane=False, out=None):
    """mpn_tta_merge_mask: the uint8 [H, W] person mask from the seg pair maps ([rh, rw, 2], channel 0 the original pass, channel 1 the
    mirrored one) of every scale — ``_get_outputs`` for both passes on channel 18, the mirror, the halving, one rounding to float32 and
    the threshold in one launch.  ``out``: a uint8 [H, W] view with dense columns to write instead of a new tensor; with ``plane`` the
    float32 [H, W] plane is returned as well."""
    n = len(seg_pair_maps)
    table = (TtaScale * max(n, 1))()
    for s, u in enumerate(seg_pair_maps):
        if u.dtype != torch.float32 or u.dim() != 3 or u.shape[2] != 2 or u.stride(2) != 1 or u.stride(1) != 2:
            raise ValueError("seg pair map %d: float32 [rh, rw, 2] with dense pixels expected" % s)
        table[s].u, table[s].rh, table[s].rw, table[s].pitch = u.data_ptr(), int(u.shape[0]), int(u.shape[1]), int(u.stride(0))
    dev = seg_pair_maps[0].device
    if out is None:
        out = torch.empty((H, W), dtype=torch.uint8, device=dev)
    elif out.dtype != torch.uint8 or tuple(out.shape) != (H, W) or (W > 1 and out.stride(1) != 1):
        raise ValueError("tta_merge_mask: out must be a uint8 [%d, %d] tensor with dense columns" % (H, W))
    pl = torch.empty((H, W), dtype=torch.float32, device=dev) if plane else None
    call("mpn_tta_merge_mask", table, n, H, W, _thr32(thr), ops.ptr(pl) if plane else None, ops.ptr(out), int(out.stride(0)) if H > 1 else W,
         ops.stream_ptr())
    return (out, pl) if plane else out


def _to_device_image(img, dev):
    if isinstance(img, np.ndarray):
        img = torch.from_numpy(np.ascontiguousarray(img))
    return img.to(dev).float()


class Tester(object):
    TestParams = TestParams

    def __init__(self, model, train_params, batch_processor=None, val_data=None):
        assert isinstance(train_params, TestParams)
        self.params = train_params
        self.val_data = val_data
        self.batch_processor = batch_processor
        self.model = model
        self.last_eval = None             # coco_eval(..., annotations=...): the KeypointEval result dict
        self.last_box_eval = None         # coco_eval_bbox(...): the BoxEval result dict
        self.last_seg_eval = None         # seg_eval(...): the person-mask IoU result dict
        if self.params.ckpt is not None:
            self._load_ckpt(self.params.ckpt)
            logger.info('Load ckpt from {}'.format(self.params.ckpt))
        self.dev = torch.device('cuda', self.params.gpus[0])
        torch.cuda.set_device(self.dev)
        self.model = self.model.to(self.dev)
        self.model.eval()
        self.model.freeze_bn()

    def _load_ckpt(self, ckpt):
        _, _ = net_utils.load_net(ckpt, self.model, load_state_dict=True)

    # ------------------------------------------------------------------ validation loss (Tester.val, tester.py:515-543)
    def val(self):
        """Loss of ``params.subnet_name`` over ALL of ``val_data`` in eval mode with frozen statistics: every batch goes through
        ``batch_processor`` -> forward -> ``build_loss``; a log block every ``print_freq`` batches.  The reference only logs the
        result; here ``(mean, std)`` of the per-batch losses is returned as well.  Log values are fetched asynchronously
        (losses.LazyFloat) and read when a block is printed, so the loop never waits for the device in between."""
        from ..network import losses
        from ..training.trainer import LogBook, RunningStat, Stopwatch, _scalar_proxy
        if self.val_data is None or self.batch_processor is None:
            raise ValueError('Tester.val() needs the val_data and batch_processor given to the constructor')
        modes = [(m, m.training) for m in self.model.modules()]      # EVERY module's mode (a PRN Dropout set to eval under a training root …)
        self.model.eval()
        was_lazy = losses.set_lazy_log(True)          # build_loss's log values: asynchronous proxies, read when a block is printed
        try:
            return self._val_loop(LogBook, RunningStat, Stopwatch, _scalar_proxy)
        finally:
            losses.set_lazy_log(was_lazy)
            for m, mode in modes:                     # the modes the caller had — a deliberate divergence: the reference
                m.training = mode                     # leaves the model in eval mode; a Trainer calling val() between epochs must get its modes back

    def _val_loop(self, LogBook, RunningStat, Stopwatch, _scalar_proxy):
        book, seen = LogBook(), RunningStat()
        batch_timer, data_timer = Stopwatch(), Stopwatch()
        logger.info('Val on validation set...')
        n = len(self.val_data)
        batch_timer.start()
        data_timer.start()
        with torch.no_grad():
            for step, batch in enumerate(self.val_data):
                data_timer.lap()
                inputs, gts, _ = self.batch_processor(self, batch)
                _, saved_for_loss = self.model(*inputs)
                batch_timer.lap()
                loss, log = self.model.build_loss(saved_for_loss, *gts)
                seen.add(_scalar_proxy(loss, True))
                book.record(log)
                if step % self.params.print_freq == 0:
                    text = '{}\n{}: epoch {}[{}/{}]'.format(self.params.exp_name, 'Validation', 0, step, n) + ''.join(book.lines())
                    text += '\n\t({:.2f}/{:.2f}s, fps:{:.1f})'.format(data_timer.mean + 1e-6, batch_timer.mean + 1e-6,
                                                                     self.params.batch_size / (batch_timer.mean + 1e-6))
                    logger.info(text)
                    batch_timer.clear()
                    data_timer.clear()
                data_timer.start()
                batch_timer.start()
        mean, std = seen.value()
        logger.info('\n\nValidation loss: mean: {}, std: {}'.format(mean, std))
        self.last_val_log = book
        return mean, std

    # ------------------------------------------------------------------ shared pieces
    def _boxes(self, scores, classification, transformed_anchors, scale):
        """tester.py:228-234 / :304-310: person boxes with score > 0.5, coordinates multiplied by `scale`."""
        if scores.numel() == 0:
            return []
        scores = scores.detach().cpu().numpy()
        classification = classification.detach().cpu().numpy()
        boxes = transformed_anchors.detach().cpu().numpy()
        out = []
        for j in np.where(scores > 0.5)[0]:
            if int(classification[j]) == 0:
                out.append((boxes[j, :] * scale).tolist())
        return out

    @staticmethod
    def _body_joints(joint_list):
        """tester.py:158-164 / :217-223: drop the neck (type 1), shift the later types down by one."""
        joints = []
        for joint in joint_list.tolist():
            if int(joint[-1]) != 1:
                joint[-1] = max(0, int(joint[-1]) - 1)
                joints.append(joint)
        return joints

    def _need_person_seg(self):
        from .._lib import MpnError
        if not getattr(self.model, 'person_seg', False):
            raise MpnError("return_masks needs a person_seg model: a plain model has no channel 18")

    def _threshold_plane(self, plane):
        """M = 255 where P > mask_thresh, else 0 (strict; a NaN gives 0) with the tensor library's ops: the unfused yardstick."""
        return (plane > _thr32(self.params.mask_thresh)).to(torch.uint8) * 255

    def prn_process(self, kps, bbox_list, file_name, image_id=0):
        return prn_process(self.model, kps, bbox_list, file_name, image_id, coeff=self.params.coeff, in_thres=self.params.in_thres)

    # ------------------------------------------------------------------ single scale (Tester.test, :194-245)
    def infer_image(self, img, file_name='', image_id=0, return_masks=False):
        """``return_masks`` (person_seg models): -> (results, [mask]) with the uint8 [H, W] person mask composed from existing ops."""
        if return_masks:
            self._need_person_seg()
        img = _to_device_image(img, self.dev)
        shape_dst = max(img.shape[0], img.shape[1])
        scale = float(shape_dst) / self.params.inp_size
        pad = abs(img.shape[1] - img.shape[0])
        sq = torch.zeros((img.shape[0] + pad, img.shape[1] + pad, 3), dtype=torch.float32, device=self.dev)
        sq[:img.shape[0], :img.shape[1]] = img                                    # np.pad(..., 'constant')
        sq = sq[:shape_dst, :shape_dst]
        img_resized = resize(sq, (self.params.inp_size, self.params.inp_size), cubic=False)
        img_input = resnet_preprocess(img_resized)[None]
        with torch.no_grad():
            heatmaps, (scores, classification, transformed_anchors) = self.model([img_input, 'both'])
        param = {'thre1': 0.1, 'thre2': 0.05, 'thre3': 0.5}
        joint_list = get_joint_list(img_resized, param, heatmaps[0, :18].permute(1, 2, 0), scale, bool_gaussian_filt=self.params.gaussian_filt)
        bboxs = self._boxes(scores, classification, transformed_anchors, scale)
        results = self.prn_process(self._body_joints(joint_list), bboxs, file_name, image_id)
        if not return_masks:
            return results
        H, W = int(img.shape[0]), int(img.shape[1])
        plane = resize(heatmaps[0, 18][:, :, None], (shape_dst, shape_dst), cubic=True)[:H, :W, 0]
        _, _, views = _mask_views([(H, W)], self.dev)
        views[0].copy_(self._threshold_plane(plane))
        return results, views

    def infer_images_batched(self, images, file_names=None, image_ids=None, batch=64, pipeline=True, return_masks=False):
        """``infer_image`` for many images with the network, the peak extraction and the PRN assignment running on whole batches:
        every image is padded to a square and resized to inp_size x inp_size (tester.py:203-213), so images of any size share a
        forward; per-image scales are applied to peaks and boxes afterwards.  Same result dicts, image by image, as
        ``infer_image`` (tests/test_round3_gpu.py).

        ``pipeline`` (round 6): the network of batch k + 1 is enqueued BEFORE batch k is post-processed, and the post-processing
        launches (NMS, peaks, PRN forward, candidate compaction) go to a second stream that waits for batch k's network only — the
        host's numpy work and its device reads run under the next batch's network instead of leaving the GPU idle (2 - 5 ms of a 33 ms
        batch at 640 x 640 x 64).  Results are identical (same launches on the same data).

        ``return_masks`` (person_seg models): -> (results, masks), one uint8 [H, W] person mask per image, the masks of a batch views of
        one buffer written by ONE mpn_seg_masks on the network's stream, before the event the post-processing stream waits for."""
        if return_masks:
            self._need_person_seg()
        masks = []
        n = len(images)
        file_names = file_names if file_names is not None else [''] * n
        image_ids = image_ids if image_ids is not None else [0] * n
        S = self.params.inp_size
        out = [None] * n
        post = self._post_stream() if pipeline else None
        pending = None
        for i0 in list(range(0, n, batch)) + [None]:
            nxt = None
            if i0 is not None:
                idx = list(range(i0, min(n, i0 + batch)))
                xs, scales, sizes = [], [], []
                for i in idx:
                    img = _to_device_image(images[i], self.dev)
                    shape_dst = max(img.shape[0], img.shape[1])
                    scales.append(float(shape_dst) / S)
                    sizes.append((int(img.shape[0]), int(img.shape[1])))
                    pad = abs(img.shape[1] - img.shape[0])
                    sq = torch.zeros((img.shape[0] + pad, img.shape[1] + pad, 3), dtype=torch.float32, device=self.dev)
                    sq[:img.shape[0], :img.shape[1]] = img
                    xs.append(resnet_preprocess(resize(sq[:shape_dst, :shape_dst], (S, S), cubic=False)))
                with torch.no_grad():
                    heat, anchors, cls, keep = self.model.forward_padded_begin(torch.stack(xs))
                if return_masks:
                    masks.extend(seg_masks(heat, sizes, self.params.mask_thresh))
                ev = None
                if post is not None:
                    ev = torch.cuda.Event()
                    ev.record()
                nxt = (idx, scales, heat, anchors, cls, keep, ev)
            if not pipeline and nxt is not None:
                self._finish_batch(nxt, out, file_names, image_ids, None)
                nxt = None
            if pending is not None:
                self._finish_batch(pending, out, file_names, image_ids, post)
            pending = nxt
        return (out, masks) if return_masks else out

    def _post_stream(self):
        if getattr(self, '_post', None) is None:
            self._post = torch.cuda.Stream(device=self.dev)
        return self._post

    def _finish_batch(self, item, out, file_names, image_ids, post):
        """Detections, peaks and the PRN assignment of one batch whose network has been enqueued (infer_images_batched)."""
        idx, scales, heat, anchors, cls, keep, ev = item
        heat = heat[:, :18]                                         # a person_seg model's channel 18 is the mask, not a heat-map
        if post is not None:
            post.wait_event(ev)
            with torch.cuda.stream(post):
                self._finish_batch_on_current_stream(idx, scales, heat, anchors, cls, out, file_names, image_ids)
        else:
            self._finish_batch_on_current_stream(idx, scales, heat, anchors, cls, out, file_names, image_ids)

    def _finish_batch_on_current_stream(self, idx, scales, heat, anchors, cls, out, file_names, image_ids):
        from ..network.joint_utils import NMS_batch_arrays, body_peaks_flat
        from .prn_process import prn_assign_arrays
        S = self.params.inp_size
        multi = cls.shape[-1] > 1
        det = self.model.detect_padded(anchors, cls, return_class=multi)
        boxes, scores, kept = det[:3]
        pk, cnt = NMS_batch_arrays({'thre1': 0.1}, heat, float(S) / heat.shape[2], bool_gaussian_filt=self.params.gaussian_filt)
        peaks_xy, joint_off = body_peaks_flat(pk, cnt)
        sc = np.asarray(scales)
        per_img = np.diff(np.concatenate([joint_off[:, 0], joint_off[-1:, 17]]))          # peaks per image
        peaks_xy = peaks_xy * np.repeat(sc, per_img)[:, None]                             # get_joint_list: peaks * scale
        nmax = boxes.shape[1]
        if nmax:
            # score > 0.5 among the kept rows of class 0 = person (the reference's `classification == 0` filter, tester.py:232; a
            # single-class head has no other class); masks built on the host from the arrays that travel anyway
            scores_h, boxes_h = scores.cpu().numpy(), boxes.cpu().numpy()
            ok_h = (scores_h > 0.5) & (np.arange(nmax)[None, :] < np.asarray(kept)[:, None])
            if multi:
                ok_h &= det[3].cpu().numpy() == 0
        else:
            ok_h, boxes_h = np.zeros((len(idx), 0), dtype=bool), np.zeros((len(idx), 0, 4), dtype=np.float32)
        # boxes * scale in float32 like the reference's numpy expression (tester.py:228-234), image-major
        b4 = (boxes_h[ok_h] * np.repeat(sc, ok_h.sum(1))[:, None].astype(np.float32)).astype(np.float64)
        start = np.concatenate([[0], np.cumsum(ok_h.sum(1))]).astype(np.int32)
        b4[:, 2:] -= b4[:, :2]
        kp = prn_assign_arrays(self.model, peaks_xy, joint_off, b4, start, in_thres=self.params.in_thres)
        for li, i in enumerate(idx):
            res = []
            for bi in range(start[li], start[li + 1]):
                k = np.zeros(51)
                k[0::3], k[1::3], k[2::3] = kp[bi, :, 0], kp[bi, :, 1], kp[bi, :, 2]
                pose_score = 0
                for f in range(17):
                    pose_score += kp[bi, f, 2]
                res.append({'image_id': image_ids[i], 'file_name': file_names[i], 'category_id': 1, 'bbox': b4[bi].tolist(),
                            'score': pose_score / 17.0, 'keypoints': k.tolist()})
            out[i] = res

    def test(self, images):
        """tester.py:194-245 over decoded images: ``images`` maps file name -> [H, W, 3] BGR array.  With
        ``params.testresult_write_json`` the result list also goes to <testresult_dir>multipose_results.json (:243-245);
        drawing the canvases (:238-241) needs cv2 and stays with the caller."""
        out = []
        for name, img in images.items():
            out.extend(self.infer_image(img, name))
        if self.params.testresult_write_json:
            with open(self.params.testresult_dir + 'multipose_results.json', "w") as f:
                json.dump(out, f)
        return out

    def coco_eval(self, images, coco=None, annotations=None):
        """tester.py:131-191 from the decoded images on: ``images`` yields (image_id, file_name, [H, W, 3] BGR array) — what the
        reference reads with pycocotools + cv2.imread.  Every image runs the 5-scale, flipped test-time augmentation; the results
        (keypoints in COCO order) are written to ``params.coco_result_filename`` (indent 4, :176-178).  With pycocotools present
        and ``coco`` the loaded annotation object, the keypoint evaluation runs as in :179-186 and the file is removed unless
        ``params.testresult_write_json`` (:188-189); without it (this image has none) the file is the product and is kept.
        With ``annotations`` (the annotation json's ``annotations`` list, what PRNSampleSet takes) the evaluation of :179-186 runs on
        the device instead (oks_eval.KeypointEval over the evaluated image ids): the ten COCO lines are logged, the result dict is
        kept in ``self.last_eval`` and the file is removed unless ``params.testresult_write_json``.  Returns the result list."""
        results, img_ids = [], []
        if getattr(self.params, 'tta_fused', False):
            images = list(images)
            img_ids = [image_id for image_id, _, _ in images]
            for res in self.infer_images_multiscale([img for _, _, img in images], [name for _, name, _ in images], img_ids):
                results.extend(res)
        else:
            for image_id, file_name, img in images:
                img_ids.append(image_id)
                results.extend(self.infer_image_multiscale(img, file_name, image_id))
        ann_filename = self.params.coco_result_filename
        with open(ann_filename, "w") as f:
            json.dump(results, f, indent=4)
        if annotations is not None:
            from .oks_eval import KeypointEval
            ev = KeypointEval(annotations)
            self.last_eval = ev.evaluate(results, img_ids=img_ids)
            ev.summarize()
            if not self.params.testresult_write_json:
                os.remove(ann_filename)
            return results
        if coco is not None:
            try:
                from pycocotools.cocoeval import COCOeval
            except ImportError:
                logger.warning("pycocotools is not installed: results left in %s", ann_filename)
                return results
            ev = COCOeval(coco, coco.loadRes(ann_filename), 'keypoints')
            ev.params.imgIds = img_ids
            ev.evaluate()
            ev.accumulate()
            ev.summarize()
            if not self.params.testresult_write_json:
                os.remove(ann_filename)
        return results

    # ------------------------------------------------------------------ detection head: boxes and box AP / AR (not in the reference)
    def detect_images(self, images, batch=64, max_per_image=None):
        """Box results of the detection head for COCO's bbox evaluation: ``images`` yields (image_id, file_name, [H, W, 3] BGR array).
        Every image takes the square-pad / resize / forward_padded_begin / detect_padded path of ``infer_images_batched``; boxes are
        multiplied by the image's scale in float32 and turned into [x, y, w, h].  One dict {'image_id', 'file_name', 'category_id',
        'bbox', 'score'} per kept post-NMS row — every row above the model's 0.05 score threshold, in descending score, not only the
        persons above 0.5 that feed the PRN — with ``params.category_ids[class index]`` as its category.  ``max_per_image`` keeps the
        best-scored rows of an image.  ``params.nms_per_class`` takes the class-wise post-processing (poseNet.detect_padded(class_wise=True):
        an anchor yields a candidate for every class above 0.05, boxes of different classes never suppress each other); the rows
        stay in descending score across classes, so ``max_per_image`` is the top N across classes."""
        from .._lib import MpnError
        cats = [int(c) for c in self.params.category_ids]
        K = int(self.model.classificationModel.num_classes)
        if len(cats) != K:
            raise MpnError("params.category_ids names %d categories, the detection head has %d classes" % (len(cats), K))
        images = list(images)
        S = self.params.inp_size
        out = []
        for i0 in range(0, len(images), batch):
            chunk = images[i0:i0 + batch]
            xs, scales = [], []
            for _, _, arr in chunk:
                img = _to_device_image(arr, self.dev)
                shape_dst = max(img.shape[0], img.shape[1])
                scales.append(float(shape_dst) / S)
                pad = abs(img.shape[1] - img.shape[0])
                sq = torch.zeros((img.shape[0] + pad, img.shape[1] + pad, 3), dtype=torch.float32, device=self.dev)
                sq[:img.shape[0], :img.shape[1]] = img
                xs.append(resnet_preprocess(resize(sq[:shape_dst, :shape_dst], (S, S), cubic=False)))
            with torch.no_grad():
                _, anchors, cls, keep = self.model.forward_padded_begin(torch.stack(xs))
            boxes, scores, kept, classes = self.model.detect_padded(anchors, cls, return_class=True,
                                                                    class_wise=bool(getattr(self.params, "nms_per_class", False)))
            boxes_h, scores_h, classes_h = boxes.cpu().numpy(), scores.cpu().numpy(), classes.cpu().numpy()
            del keep
            for li, (image_id, file_name, _) in enumerate(chunk):
                n = int(kept[li]) if max_per_image is None else min(int(kept[li]), int(max_per_image))
                b4 = (boxes_h[li, :n] * np.float32(scales[li])).astype(np.float64)       # boxes * scale in float32, as _finish_batch
                b4[:, 2:] -= b4[:, :2]
                for j in range(n):
                    out.append({'image_id': image_id, 'file_name': file_name, 'category_id': cats[int(classes_h[li, j])],
                                'bbox': b4[j].tolist(), 'score': float(scores_h[li, j])})
        return out

    def coco_eval_bbox(self, images, annotations, categories=None):
        """Box AP / AR of the detection head on the device: ``detect_images`` over ``images``, then box_eval.BoxEval(annotations,
        categories) over the evaluated image ids.  The twelve COCO lines are logged, the result dict is kept in
        ``self.last_box_eval``; with ``params.testresult_write_json`` the results also go to ``params.coco_result_filename`` (indent 4,
        as ``coco_eval``), otherwise no file is written.  Returns the result list."""
        from .box_eval import BoxEval
        images = list(images)
        results = self.detect_images(images)
        if self.params.testresult_write_json:
            with open(self.params.coco_result_filename, "w") as f:
                json.dump(results, f, indent=4)
        ev = BoxEval(annotations, categories=categories)
        self.last_box_eval = ev.evaluate(results, img_ids=[image_id for image_id, _, _ in images])
        ev.summarize()
        return results

    # ------------------------------------------------------------------ multi-scale + flip (Tester.coco_eval, :143-175)
    def _get_multiplier(self, img):
        """tester.py:256-262."""
        return [x * self.params.inp_size / float(img.shape[0]) for x in [0.5, 1., 1.5, 2, 2.5]]

    def _get_outputs(self, multiplier, img, seg=False):
        """tester.py:264-313: heat-maps of every scale resized back to the image and averaged; boxes per scale.  ``seg``: the same
        steps on channel 18 as well, into a float64 [H, W, 1] accumulator returned third."""
        H, W = img.shape[0], img.shape[1]
        heatmap_avg = torch.zeros((H, W, 18), dtype=torch.float64, device=self.dev)       # np.zeros(...) accumulator: float64 (tester.py:266)
        seg_avg = torch.zeros((H, W, 1), dtype=torch.float64, device=self.dev) if seg else None
        bbox_all = []
        for scale in multiplier:
            inp_size = scale * H
            im_cropped, im_scale, real_shape = crop_with_factor(img, inp_size, factor=32, pad_val=128)
            im_data = resnet_preprocess(im_cropped)[None]
            with torch.no_grad():
                heatmaps, (scores, classification, transformed_anchors) = self.model([im_data, 'both'])
            hm = heatmaps[0, :18].permute(1, 2, 0)[:int(im_cropped.shape[0] / 4), :int(im_cropped.shape[1] / 4), :]
            hm = resize(hm, (hm.shape[0] * 4, hm.shape[1] * 4), cubic=True)
            hm = hm[0:real_shape[0], 0:real_shape[1], :]
            hm = resize(hm, (H, W), cubic=True)
            heatmap_avg = heatmap_avg + hm / len(multiplier)
            if seg:
                sm = heatmaps[0, 18:19].permute(1, 2, 0)[:int(im_cropped.shape[0] / 4), :int(im_cropped.shape[1] / 4), :]
                sm = resize(sm, (sm.shape[0] * 4, sm.shape[1] * 4), cubic=True)
                sm = sm[0:real_shape[0], 0:real_shape[1], :]
                sm = resize(sm, (H, W), cubic=True)
                seg_avg = seg_avg + sm / len(multiplier)
            bbox_all.append(self._boxes(scores, classification, transformed_anchors, 1.0 / im_scale))
        return (heatmap_avg, bbox_all, seg_avg) if seg else (heatmap_avg, bbox_all)

    @staticmethod
    def _handle_heat(normal_heat, flipped_heat):
        """tester.py:315-331."""
        return (normal_heat + flipped_heat.flip(1)[:, :, SWAP_HEAT]) / 2.

    def infer_image_multiscale(self, img, file_name='', image_id=0, return_masks=False):
        """tester.py:143-175 for one image.  The float64 averaged maps are rounded to float32 once before the peak kernel; with
        ``params.gaussian_filt`` the smoothing then follows the float32 semantics of ``NMS`` (float32 up-sampled patch, float64 sums,
        one float32 rounding per axis), where the reference would filter a float64 patch.

        ``return_masks`` (person_seg models): -> (results, [mask]); the mask comes from ``_get_outputs``' steps on channel 18 of both
        passes, the mirrored one flipped back (no channel swap), halved, rounded to float32 once and thresholded."""
        if return_masks:
            self._need_person_seg()
        img = _to_device_image(img, self.dev)
        multiplier = self._get_multiplier(img)
        if return_masks:
            orig_heat, orig_bbox_all, seg_o = self._get_outputs(multiplier, img, seg=True)
            flipped_heat, _, seg_f = self._get_outputs(multiplier, img.flip(1).contiguous(), seg=True)
        else:
            orig_heat, orig_bbox_all = self._get_outputs(multiplier, img)
            flipped_heat, _ = self._get_outputs(multiplier, img.flip(1).contiguous())
        heatmaps = self._handle_heat(orig_heat, flipped_heat)
        param = {'thre1': 0.1, 'thre2': 0.05, 'thre3': 0.5}
        # the averaged maps are float64 as in the reference (np.zeros accumulator); the peak kernel takes float32, so they are
        # rounded ONCE here (the reference's find_peaks / cv2 refinement run on the float64 maps: a <= 1 ulp(f32) deviation)
        joint_list = get_joint_list(img, param, heatmaps[:, :, :18].float().contiguous(), 1, bool_gaussian_filt=self.params.gaussian_filt)
        results = self.prn_process(self._body_joints(joint_list), orig_bbox_all[1], file_name, image_id)
        for result in results:                                    # tester.py:167-175: COCO keypoint order
            kp = result['keypoints']
            result['keypoints'] = [kp[COCO_ORDER[i] * 3 + j] for i in range(17) for j in range(3)]
        if not return_masks:
            return results
        plane = ((seg_o + seg_f.flip(1)) / 2.).float()[:, :, 0]
        _, _, views = _mask_views([(int(img.shape[0]), int(img.shape[1]))], self.dev)
        views[0].copy_(self._threshold_plane(plane))
        return results, views

    # ------------------------------------------------------------------ the same, fused and flip-paired (params.tta_fused)
    def _tta_enqueue(self, img, pair=True, mask_out=None):
        """Everything of ``infer_image_multiscale`` up to the averaged maps, enqueued on the current stream without a host read: per
        scale ONE mpn_tta_input (the original and the mirrored network input), ONE forward over the pair — keypoint-only except for
        scale index 1, the only scale whose boxes are used (tester.py:169) — and ONE mpn_resize (the x4 up-sampling of both maps,
        only the region that survives the crop); then ONE mpn_tta_merge.  ``pair=False``: the two images of a pair go through the
        network one at a time.  ``mask_out`` (a uint8 [H, W] view): per scale one more mpn_resize (channel 18 of both images of the pair, in
        place) and ONE mpn_tta_merge_mask that writes the person mask into it, on this stream.  Returns the item ``_tta_finish`` takes;
        it owns every tensor another stream may still read."""
        img = _to_device_image(img, self.dev)
        H, W = int(img.shape[0]), int(img.shape[1])
        multiplier = self._get_multiplier(img)
        alive, det, pair_maps, seg_maps = [img], None, [], []
        for si, scale in enumerate(multiplier):
            im_scale, h, w, hp, wp = scale_geometry(H, W, scale * H, 32)
            x = tta_input(img, h, w, hp, wp, 1.0 / im_scale)
            with torch.no_grad():
                if si == 1:
                    heat, anchors, cls, keep = self.model.forward_padded_begin(x if pair else x[:1])
                    det = (anchors[:1], cls[:1], 1.0 / im_scale)
                else:
                    heat, keep = self.model.forward_heat(x if pair else x[:1])
                alive.append(keep)
                if not pair:
                    heat1, keep = self.model.forward_heat(x[1:])
                    alive.append(keep)
                    heat = torch.cat([heat, heat1])
            hq, wq = int(hp / 4), int(wp / 4)
            if mask_out is not None:
                seg_maps.append(tta_seg_upsample(heat[:, :, :hq, :wq], min(h, 4 * hq), min(w, 4 * wq)))
            heat = heat[:, :18, :hq, :wq]
            pair_maps.append(tta_upsample(heat, min(h, 4 * hq), min(w, 4 * wq)))       # only the region that survives the crop
            alive += [x, heat]
        if mask_out is not None:
            tta_merge_mask(seg_maps, H, W, self.params.mask_thresh, out=mask_out)
        return img, tta_merge(pair_maps, H, W), det, alive + pair_maps + seg_maps

    def _tta_finish(self, item, file_name, image_id):
        """Boxes of scale index 1 (image 0 of the pair), peaks of the averaged maps, PRN assignment, COCO order — on the current stream."""
        img, heat, (anchors, cls, box_scale), _alive = item
        multi = cls.shape[-1] > 1
        det = self.model.detect_padded(anchors, cls, return_class=multi)
        boxes, scores, kept = det[:3]
        bboxs = []
        k = int(kept[0]) if boxes.shape[1] else 0
        if k:
            scores_h, boxes_h = scores[0, :k].cpu().numpy(), boxes[0, :k].cpu().numpy()
            classes_h = det[3][0, :k].cpu().numpy() if multi else np.zeros(k, dtype=np.int64)
            for j in np.where(scores_h > 0.5)[0]:                     # _boxes: score > 0.5, class 0, box * scale in float32
                if int(classes_h[j]) == 0:
                    bboxs.append((boxes_h[j, :] * box_scale).tolist())
        param = {'thre1': 0.1, 'thre2': 0.05, 'thre3': 0.5}
        joint_list = get_joint_list(img, param, heat, 1, bool_gaussian_filt=self.params.gaussian_filt)
        results = self.prn_process(self._body_joints(joint_list), bboxs, file_name, image_id)
        for result in results:
            kp = result['keypoints']
            result['keypoints'] = [kp[COCO_ORDER[i] * 3 + j] for i in range(17) for j in range(3)]
        return results

    def infer_image_multiscale_fused(self, img, file_name='', image_id=0, pair=True, return_masks=False):
        """``infer_image_multiscale`` with the same result dicts, value for value, from 5 paired forwards instead of 10 single ones
        (one detection head instead of ten) and two fused element-wise kernels around them (csrc/tta.hip); the only host reads are
        those of the detections, the peaks and the PRN assignment.  ``return_masks`` (person_seg models): -> (results, [mask]), the mask
        of ``infer_image_multiscale`` from five more mpn_resize and one mpn_tta_merge_mask."""
        if not return_masks:
            return self._tta_finish(self._tta_enqueue(img, pair), file_name, image_id)
        self._need_person_seg()
        _, _, views = _mask_views([(int(img.shape[0]), int(img.shape[1]))], self.dev)
        return self._tta_finish(self._tta_enqueue(img, pair, views[0]), file_name, image_id), views

    def infer_images_multiscale(self, images, file_names=None, image_ids=None, pipeline=True, pair=True, return_masks=False):
        """``infer_image_multiscale_fused`` over many images.  ``pipeline``: the launches of image k + 1 up to and including its merge are
        enqueued BEFORE image k's detections, peaks and PRN assignment are read; those go to the post-processing stream behind an event,
        as in ``infer_images_batched``.  Same launches on the same data: results identical to ``pipeline=False``.
        ``return_masks`` (person_seg models): -> (results, masks); the masks are views of one buffer, each written before its image's event."""
        images = list(images)
        n = len(images)
        views = [None] * n
        if return_masks:
            self._need_person_seg()
            _, _, views = _mask_views([(int(im.shape[0]), int(im.shape[1])) for im in images], self.dev)
        file_names = file_names if file_names is not None else [''] * n
        image_ids = image_ids if image_ids is not None else [0] * n
        out = [None] * n
        post = self._post_stream() if pipeline else None
        pending = None
        for i in list(range(n)) + [None]:
            nxt = None
            if i is not None:
                item = self._tta_enqueue(images[i], pair, views[i])
                if post is None:
                    out[i] = self._tta_finish(item, file_names[i], image_ids[i])
                else:
                    ev = torch.cuda.Event()
                    ev.record()
                    nxt = (i, item, ev)
            if pending is not None:
                k, item, ev = pending
                post.wait_event(ev)
                with torch.cuda.stream(post):
                    out[k] = self._tta_finish(item, file_names[k], image_ids[k])
                torch.cuda.current_stream(self.dev).wait_stream(post)      # the item's tensors return to this stream's allocator pool
            pending = nxt
        return (out, views) if return_masks else out

    # ------------------------------------------------------------------ person masks and their score (not in the reference)
    def person_masks(self, images, multiscale=False, batch=64):
        """The uint8 [H, W] person mask (255 where channel 18's image-sized plane > ``params.mask_thresh``) of every decoded image:
        ``infer_images_batched`` (single scale) or ``infer_images_multiscale`` (5 scales x flip) with ``return_masks``."""
        images = list(images)
        if multiscale:
            return self.infer_images_multiscale(images, return_masks=True)[1]
        return self.infer_images_batched(images, batch=batch, return_masks=True)[1]

    def seg_eval(self, images, annotations, multiscale=False, batch=64):
        """IoU of the predicted person masks against ``mask_all`` on the device.  ``images`` yields (image_id, file_name, [H, W, 3] BGR
        array) as for ``coco_eval``; ``annotations`` is the annotation json's ``annotations`` list (person annotations, category 1).
        Per chunk of ``batch`` images: the masks (``person_masks``), ``mask_all`` of the chunk (datasets/segm.py: person_masks_batch on
        each image's annotations in json order) and the counts (mpn_mask_iou) into one device array; ONE host read at the end.  The
        summary lines are logged; the dict (seg_eval.summarize_counts plus ``inter``, ``pred``, ``gt``, ``pixels``, ``image_ids``) is kept
        in ``self.last_seg_eval`` and returned."""
        from ..datasets.segm import person_masks_batch
        from .seg_eval import mask_iou_counts, summarize_counts
        self._need_person_seg()
        images = list(images)
        by_img = {}
        for a in annotations:
            if int(a.get('category_id', 1)) == 1:
                by_img.setdefault(a['image_id'], []).append(a)
        n = len(images)
        counts = torch.zeros((max(n, 1), 3), dtype=torch.int64, device=self.dev)
        sizes = [(int(arr.shape[0]), int(arr.shape[1])) for _, _, arr in images]
        for i0 in range(0, n, batch):
            chunk, csz = images[i0:i0 + batch], sizes[i0:i0 + batch]
            masks = self.person_masks([arr for _, _, arr in chunk], multiscale=multiscale, batch=batch)
            base = masks[0].storage_offset()              # the chunk's masks are views of one buffer, the first at its start
            pred_buf = torch.empty(0, dtype=torch.uint8, device=self.dev).set_(masks[0].untyped_storage())[base:]
            _, gt_buf, gt_off = person_masks_batch([by_img.get(image_id, []) for image_id, _, _ in chunk], csz, dev=self.dev)
            table = np.array([(H, W, m.storage_offset() - base, W, go, W) for (H, W), m, go in zip(csz, masks, gt_off)], dtype=np.int64)
            mask_iou_counts(pred_buf, gt_buf, table, out=counts[i0:i0 + len(chunk)])
        c = counts[:n].cpu().numpy()
        pixels = np.array([H * W for H, W in sizes], dtype=np.int64)
        ev = summarize_counts(c, pixels)
        ev.update({'inter': c[:, 0].copy(), 'pred': c[:, 1].copy(), 'gt': c[:, 2].copy(), 'pixels': pixels,
                   'image_ids': [image_id for image_id, _, _ in images]})
        mode = 'multi-scale' if multiscale else 'single scale'
        for key in ('iou', 'mean_iou', 'precision', 'recall', 'pixel_acc'):
            logger.info(' Person mask %-9s (%s, thr %.3f) = %0.3f' % (key, mode, self.params.mask_thresh, ev[key]))
        logger.info(' Person mask images = %d, without any ON pixel in either mask = %d' % (ev['n_images'], ev['n_empty']))
        self.last_seg_eval = ev
        return ev
