"""The committed inputs of tests/test_segm_cpu.py and tests/test_segm_gpu.py: for an h x w image, seven annotations'
``segmentation`` fields (not a multiple of any workgroup's size) built from fractions of the image size, so that every size gets the
same situations:

0. a 16-vertex star: edges in all eight octants, both ``dx >= dy`` branches, both directions, non-integer coordinates;
1. two OVERLAPPING parts (a union, not an XOR);
2. disjoint parts, a part wholly outside the frame, a zero-area part (an outline that runs back over itself: every toggle comes
   twice) and repeated vertices;
3. a diamond through all four borders with negative, non-integer coordinates, and a part across the bottom border (``yd = h``);
4. an uncompressed RLE whose runs span several columns;
5. a compressed RLE with a zero-length first run (cell (0, 0) is ON);
6. a polygon wholly outside the frame: an instance that rasterises EMPTY.

The RLE encoder (maskApi.c: rleEncode, rleToString) is written here for the tests only; the product has none.
"""
import math

import numpy as np

SIZES = [(5, 6), (37, 53), (64, 65), (130, 70)]
N_INST = 7
EMPTY = 6                       # the instance that has no ON cell


def mask_counts(m):
    """rleEncode: run lengths of the column-major flat mask, the first run OFF (0 long when cell (0, 0) is ON)."""
    flat = np.asarray(m, dtype=np.uint8).T.reshape(-1)
    counts, prev, run = [], 0, 0
    for v in flat:
        if v != prev:
            counts.append(run)
            run, prev = 0, v
        run += 1
    counts.append(run)
    return counts


def counts_string(counts):
    """rleToString: the compressed form of a list of run lengths."""
    s = bytearray()
    for i, x in enumerate(counts):
        x = int(x)
        if i > 2:
            x -= int(counts[i - 2])
        more = True
        while more:
            c = x & 0x1f
            x >>= 5
            more = (x != -1) if (c & 0x10) else (x != 0)
            if more:
                c |= 0x20
            s.append(c + 48)
    return bytes(s).decode("ascii")


def _r(v):
    return round(float(v), 2)               # COCO stores two decimals


def segmentations(h, w):
    m = min(h, w)
    star = []
    for j in range(16):
        a = 2 * math.pi * j / 16 + 0.1
        rad = (0.46 if j % 2 == 0 else 0.21) * m
        star += [_r(0.48 * w + rad * math.cos(a)), _r(0.52 * h + rad * math.sin(a))]
    overlap = [[_r(0.1 * w), _r(0.15 * h), _r(0.62 * w), _r(0.15 * h), _r(0.62 * w), _r(0.55 * h), _r(0.1 * w), _r(0.55 * h)],
               [_r(0.3 * w), _r(0.3 * h), _r(0.93 * w), _r(0.41 * h), _r(0.5 * w), _r(0.96 * h)]]
    a0, b0, a1, b1 = _r(0.55 * w), _r(0.6 * h), _r(0.9 * w), _r(0.93 * h)
    mixed = [[0.4, 0.3, 0.4, 0.3, _r(0.3 * w), 0.3, _r(0.33 * w), _r(0.3 * h), _r(0.33 * w), _r(0.3 * h), 0.4, _r(0.27 * h)],
             [a0, b0, a1, b0, a1, b1, a0, b1],
             [w + 2.0, 1.0, w + 5.5, 1.0, w + 5.5, 4.0, w + 2.0, 4.0],
             [_r(0.1 * w), _r(0.5 * h), _r(0.45 * w), _r(0.85 * h), _r(0.275 * w), _r(0.675 * h)]]
    borders = [[-2.37, _r(0.4 * h), _r(0.5 * w), -3.33, w + 2.61, _r(0.55 * h), _r(0.45 * w), h + 3.2],
               [_r(0.2 * w), h - 1.5, _r(0.7 * w), h - 0.7, _r(0.6 * w), h + 4.0, _r(0.1 * w), h + 2.1]]
    band = np.zeros((h, w), dtype=np.uint8)
    band[:, w // 4: w // 4 + 3] = 1                           # one run over three whole columns
    band[h // 2:, w // 4 + 3] = 1                             # ... that goes on into the next one
    band[h // 3, w - 1] = 1
    band[h - 1, w // 2] = 1
    band[0, w // 2 + 1] = 1                                   # the last cell of a column and the first of the next: one run
    corner = np.zeros((h, w), dtype=np.uint8)
    corner[: h // 2 + 1, :2] = 1
    corner[h // 4:, w - 2] = 1
    corner[h - 1, w - 1] = 1                                  # the last cell of the image: the final run is ON
    outside = [[-5.0, -5.0, -2.0, -5.0, -2.0, -2.0, -5.0, -2.0]]
    return [[star], overlap, mixed, borders, {"size": [h, w], "counts": mask_counts(band)},
            {"size": [h, w], "counts": counts_string(mask_counts(corner))}, outside], (band, corner)
