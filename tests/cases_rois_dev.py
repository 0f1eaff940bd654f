"""The case table of tests/test_gpu_rois_dev.py (vpf_convert_resize_tensor_rois_dev), importable without a GPU: tests/test_rois_dev_bounds_cpu.py asserts
through the kernel's own per-tile policy (roi_tile_need, csrc/vpf_job_bounds.h) that these calls hold staged AND per-tap tiles — the GPU cannot
tell which form wrote a pixel, both give the same bits."""
import numpy as np

F = np.float32
FRAME_SIZES = [(131, 79), (130, 78)]
DST_SIZES = [(64, 128), (64, 48), (300, 40), (24, 16)]  # 300 x 40: a second column chunk and a third row band; 24 x 16: large down-scales, per tap


def inexact_sides(limit, d):
    """sides s <= limit whose scale factor (float)s / (float)d is NOT s times the rounded reciprocal of d: a kernel that multiplied by a reciprocal
    instead of dividing would sample these rectangles with another scale"""
    return [s for s in range(1, limit + 1) if F(s) * (F(1) / F(d)) != F(s) / F(d)]


def geometry_rects(W, H, dw, dh):
    """the rectangles of one call: the whole frame, one pixel, odd and even corners, rectangles that touch the right and bottom edges, up-scales, and
    every width (height) whose quotient by dw (dh) a reciprocal-multiply would miss"""
    rects = [(0, 0, W, H), (0, 0, 1, 1), (W - 1, H - 1, 1, 1), (17, 9, 55, 41), (16, 8, 56, 40), (W - 20, H - 10, 20, 10), (1, 0, 129, 78),
             (5, 7, 13, 9), (40, 31, 10, 6), (W - 7, 3, 7, H - 3), (2, H - 5, W - 2, 5)]
    for i, w in enumerate(inexact_sides(W, dw)):
        h = 1 + (7 * i + 3) % H
        rects.append(((3 * i) % (W - w + 1), (5 * i) % (H - h + 1), w, h))
    for i, h in enumerate(inexact_sides(H, dh)):
        w = 1 + (11 * i + 5) % W
        rects.append(((7 * i) % (W - w + 1), (3 * i) % (H - h + 1), w, h))
    return rects


def frame_of(i):
    """two frames, interleaved"""
    return i % 2
