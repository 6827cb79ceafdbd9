"""Plain-numpy restatement of the mask_miss rule for the tests of datasets/segm.py's mask_miss functions and of
csrc/segm.hip's compose launch.  For one image, its person annotations in json order, ``M_p`` = ``segm_ref.ann_to_mask`` of
annotation ``p``::

    all = 0; miss = 0
    for p in order:
        if iscrowd(p):            miss |= M_p & ~all          # "all" as accumulated SO FAR, not the final union
        else:                     all  |= M_p
                                  if num_keypoints(p) <= 0: miss |= M_p
    mask_miss = 255 where miss == 0, else 0                   # uint8

SEQUENTIAL over whole H x W arrays (:func:`compose`); the kernel walks 64 x 512 tiles of 64-bit words and never holds a mask.
:func:`closed_form` is the same rule per pixel without a running state.

``mis`` names ONE modelled misreading (tests/test_mask_miss_cpu.py checks that the committed inputs reject each of them):
"final_union" (crowd minus the FINAL union), "no_reduce" (crowd not reduced at all), "no_crowd" (crowds ignored), "all_N" (every
non-crowd treated as N), "N_as_K", "reversed" (annotation order reversed), "one" (1 instead of 255), "not_inverted".
"""
import numpy as np

import segm_cases as sc
import segm_ref as sr

K, N, C = "K", "N", "C"
MISREADINGS = ["final_union", "no_reduce", "no_crowd", "all_N", "N_as_K", "reversed", "one", "not_inverted"]

# the committed case: the seven instances of segm_cases.segmentations with these kinds, at these sizes
CASE_KINDS = (N, C, C, K, C, C, N)
SIZES = list(sc.SIZES) + [(513, 66), (520, 131)]


def kind_of(ann):
    """'C' if iscrowd is truthy, 'N' if num_keypoints <= 0, else 'K'; num_keypoints absent = the v > 0 entries of keypoints."""
    if ann.get("iscrowd"):
        return C
    n = ann.get("num_keypoints")
    if n is None:
        n = sum(1 for v in list(ann["keypoints"])[2::3] if v > 0)
    return N if n <= 0 else K


def compose(masks, kinds, mis=None):
    """The rule over ready masks (uint8 / bool [h, w] each, at least one: :func:`mask_miss` answers for an image without
    annotations) and their kinds -> uint8 [h, w]."""
    masks = [np.asarray(m).astype(bool) for m in masks]
    kinds = list(kinds)
    if mis == "reversed":
        masks, kinds = masks[::-1], kinds[::-1]
    if mis == "all_N":
        kinds = [k if k == C else N for k in kinds]
    if mis == "N_as_K":
        kinds = [K if k == N else k for k in kinds]
    final = np.zeros_like(masks[0])
    for m, k in zip(masks, kinds):
        if k != C:
            final |= m
    every = np.zeros_like(masks[0])
    miss = np.zeros_like(masks[0])
    for m, k in zip(masks, kinds):
        if k == C:
            if mis == "no_crowd":
                continue
            if mis == "final_union":
                miss |= m & ~final
            elif mis == "no_reduce":
                miss |= m
            else:
                miss |= m & ~every
        else:
            every |= m
            if k == N:
                miss |= m
    on = 1 if mis == "one" else 255
    if mis == "not_inverted":
        return np.where(miss, on, 0).astype(np.uint8)
    return np.where(miss, 0, on).astype(np.uint8)


def closed_form(masks, kinds):
    """Per pixel, no running state: a cell is 0 iff some N covers it, or the first crowd covering it comes before the first
    non-crowd covering it."""
    masks = [np.asarray(m).astype(bool) for m in masks]
    h, w = masks[0].shape
    never = len(masks)
    first_crowd = np.full((h, w), never)
    first_person = np.full((h, w), never)
    some_n = np.zeros((h, w), dtype=bool)
    for i in range(len(masks) - 1, -1, -1):
        if kinds[i] == C:
            first_crowd[masks[i]] = i
        else:
            first_person[masks[i]] = i
            if kinds[i] == N:
                some_n |= masks[i]
    zero = some_n | (first_crowd < first_person)
    return np.where(zero, 0, 255).astype(np.uint8)


def mask_miss(anns, h, w, mis=None):
    """mask_miss of one h x w image from its annotation dicts (``segmentation``, ``iscrowd``, ``num_keypoints`` / ``keypoints``)."""
    if len(anns) == 0:
        return np.full((h, w), 0 if mis == "not_inverted" else (1 if mis == "one" else 255), dtype=np.uint8)
    return compose([sr.ann_to_mask(a["segmentation"], h, w) for a in anns], [kind_of(a) for a in anns], mis)


def annotation(segm, kind, fallback=False):
    """An annotation dict of the given kind; ``fallback`` leaves num_keypoints out and gives ``keypoints`` instead."""
    if kind == C:
        return {"segmentation": segm, "iscrowd": 1, "num_keypoints": 0}
    n = 0 if kind == N else 5
    ann = {"segmentation": segm, "iscrowd": 0}
    if fallback:
        ann["keypoints"] = [10.0, 12.0, 2] * n + [0.0, 0.0, 0] * (17 - n)
    else:
        ann["num_keypoints"] = n
    return ann


def case_annotations(h, w, kinds=CASE_KINDS):
    return [annotation(s, k, fallback=(i % 2 == 1)) for i, (s, k) in enumerate(zip(sc.segmentations(h, w)[0], kinds))]


_CASE = {}


def case(h, w):
    """The committed case at one size, computed once and shared: (annotations, [masks], mask_miss).  Leave it unchanged."""
    if (h, w) not in _CASE:
        anns = case_annotations(h, w)
        masks = [sr.ann_to_mask(a["segmentation"], h, w) for a in anns]
        _CASE[(h, w)] = (anns, masks, compose(masks, CASE_KINDS))
    return _CASE[(h, w)]
