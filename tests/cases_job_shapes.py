"""The case table of tests/test_gpu_job_shapes.py: wide, short frames and the destination sizes at which the per-job kernels (k_roi_strip,
k_roi_gather, k_warp_strip, k_warp_gather) run more than one 256-column chunk, full 64-lane waves and more than one 32-pixel tile.  A module of
its own so that the CPU test of the table (tests/test_job_bounds_cpu.py: which jobs the policy stages, which gather) imports it without a GPU."""
import math

# wide and short: coordinates are large, the oracle still converts a frame in milliseconds.  4100 x 24: the column range of a 4K decoder.
FRAMES = [(1100, 40), (1101, 41), (4100, 24)]

# chunks 0, 1 and 2 of k_roi_strip / k_roi_gather all run:
#   256 x 20  one chunk, every lane of every wave active; two bands, the second with three idle waves
#   260 x 5   a second chunk holding ONE lane; one band of two waves
#   258 x 17  a second chunk whose last (only) lane has nv = 2: the whole wave leaves the vector path; a second band of one row
#   640 x 4   three chunks, the third half full; one wave per workgroup
#   384 x 33  a second chunk of 32 lanes; three bands, the third of one row
#   224 x 24  the classic network input width: 56 lanes
ROI_DESTS = [(256, 20), (260, 5), (258, 17), (640, 4), (384, 33), (224, 24)]


def roi_rects(W, H, dw, dh):
    """the rectangles of one call on a W x H frame into dw x dh"""
    if (W, H) == (4100, 24):
        return [(3801, 1, 260, 20), (3583, 0, 517, 24), (0, 0, W, H), (W - 9, H - 5, 9, 5), (2999, 1, 1098, 22), (3000 + dw // 7, 3, 33, 17), (W - 1, H - 1, 1, 1)]
    rects = [
        (0, 0, W, H),
        (301, 3, dw, dh),          # an identity crop at an odd offset
        (301, 3, 517, 33),
        (843, 7, 257, 33),         # (1100 wide: touches the right edge)
        (1, 1, 1098, 38),
        (5, 0, 130, 40),
        (W - 9, H - 5, 9, 5),
        (0, 0, 1, 1),
        (100, 2, 999, 7),
        (7, 9, 333, 31),
    ]
    if (W, H) == (1101, 41):       # the odd-sized frame: the last column and row have a chroma sample of their own
        rects += [(W - 517, H - 33, 517, 33), (W - 130, 0, 130, H), (0, H - 7, W, 7), (W - 1, H - 1, 1, 1)]
    return rects


# warp: three tiles in x, the last partial with 8 columns, and two in y / seven tiles in x, one in y with 8 rows
WARP_FRAMES = [(1100, 40), (4100, 24)]
WARP_DESTS = [(72, 40), (224, 8)]
_C30, _S30 = 1.3 * math.cos(math.radians(30)), 1.3 * math.sin(math.radians(30))


def warp_mats(W, H, dw, dh):
    """the matrices of one call on a W x H frame into dw x dh"""
    cx = 3900.0 if W > 3900 else W - 200.0   # the rotation's centre column: around column 3900 on the 4100-wide frame
    return [
        (1, 0, W - dw, 0, 1, 0),                                  # identity at (W - dw, 0): sx hits W - 1 exactly
        (_C30, -_S30, cx - _C30 * dw / 2, _S30, _C30, -_S30 * dw / 2 + H / 2),   # 30 degrees x 1.3 around (cx, H / 2)
        (-1, 0, W - 3, 0, 1, 1),                                  # a flip
        (2.9, 0, W - 2.9 * dw - 7, 0, 2.9, 0.25),                 # a 2.9 x down-scale (rows beyond the short frame: the border / the clamp)
        # a 7 x down-scale.  On a 131 x 79 frame its tiles outgrow the strip limit; these frames are 40 / 24 rows short, so a tile's window
        # (224 columns x every row) still fits and the job is STAGED with one of the largest strips ...
        (7, 0, W - 7 * dw - 11 if W > 7 * dw + 11 else 3, 0, 7, 0.5),
        # ... and 23 x in x is what takes the gather class here (a tile spans 716 columns x every row: 113 KiB / 68 KiB against 64 KiB)
        (23, 0, 5, 0, 7, 0.5),
        (1, 0, W + 500, 0, 1, 0),                                 # wholly outside
        (1, 0, W - dw / 2 + 0.5, 0, 1, H - dh / 2 + 0.5),         # half outside, to the right and below
    ]
