"""The case table of tests/test_gpu_letterbox_dev.py (vpf_convert_letterbox_tensor_dev), importable without a GPU: tests/test_letterbox_dev_cpu.py
asserts through the kernel's own per-tile policy (letterbox_tile_window, csrc/vpf_job_bounds.h) that these calls hold padded, staged AND per-tap tiles —
the GPU cannot tell which form wrote a pixel, all give the same bits — and that the two fit ties are ties."""
import numpy as np

FRAME_SIZES = [(131, 79), (96, 64)]  # odd in both sides | even
SOURCES = ["NV12", "YUV420", "P10"]
# 64 x 48: one column tile, three row tiles; 300 x 40: the picture crosses column 256 and row 16 or 32; 24 x 16: the whole frame lands in it, so per-tap
# tiles; 17 x 33: odd, a partial last lane group
DST_SIZES = [(64, 48), (300, 40), (24, 16), (17, 33)]
PAD = (114, 7, 250)  # three different values: a channel mix-up shows

# per destination: a (w, h) of the destination's exact aspect (w * dh == h * dw: the tie of the fit's branch, and the fit is the whole plane), and a
# (w, h) whose free side lands exactly on a half (2 w dh + h is a multiple of 2 h: the half-up tie).  All fit the smaller frame.
ASPECT = {(64, 48): (80, 60), (300, 40): (90, 12), (24, 16): (90, 60), (17, 33): (17, 33)}
HALF_UP = {(64, 48): (3, 32), (300, 40): (3, 16), (24, 16): (3, 32), (17, 33): (1, 6)}


def fit(w, h, dw, dh):
    """vpf_letterbox_fit restated on Python's unbounded integers (include/vpf_hip.h)"""
    if w * dh >= h * dw:
        iw, ih = dw, min(max((2 * h * dw + w) // (2 * w), 1), dh)
    else:
        iw, ih = min(max((2 * w * dh + h) // (2 * h), 1), dw), dh
    return ((dw - iw) // 2, (dh - ih) // 2, iw, ih)


def geometry_rects(W, H, dw, dh):
    """the rectangles of one call: the whole frame, one pixel, odd and even corners, the right and bottom edges, a tall 3-wide box (3 x 70; 3 x 60 on
    the frame that is 64 high) whose picture is one or two columns wide, a wide 2-high box (120 x 2; 92 x 2 on the frame that is 96 wide), a box of the
    destination's exact aspect and the two fit ties"""
    aw, ah = ASPECT[(dw, dh)]
    tw, th = HALF_UP[(dw, dh)]
    return [(0, 0, W, H), (0, 0, 1, 1), (W - 1, H - 1, 1, 1), (17, 9, 55, 41), (16, 8, 56, 40), (W - 20, H - 10, 20, 10), (W - 7, 3, 7, H - 3),
            (2, H - 5, W - 2, 5), (5, 3, 3, min(70, H - 4)), (3, 5, min(120, W - 4), 2), (5, 3, aw, ah), (W - tw, H - th, tw, th), (7, 2, tw, th)]


def explicit_rects(dw, dh, n):
    """n placements inside dw x dh with odd ix and iy, of many sizes, the whole plane, one element and the far corner among them"""
    out = [(0, 0, dw, dh), (dw - 1, dh - 1, 1, 1), (1, 1, 1, 1)]
    for i in range(n):
        ix, iy = (2 * i + 1) % dw, (2 * (3 * i) + 1) % dh
        iw, ih = 1 + (5 * i + 2) % (dw - ix), 1 + (7 * i + 3) % (dh - iy)
        out.append((ix, iy, iw, ih))
    return out[:n]


def frame_of(i):
    """two frames, interleaved"""
    return i % 2


# ------------------------------------------------------------------------------------------------ the seeded family
FUZZ_DEFAULT = 16


def fuzz_case(seed):
    """one call: frame size, source format, destination (one of DST_SIZES), 3 .. 24 boxes — most valid, some not —, fitted or explicit placements (some
    of them invalid), dtype, B G R, channels-last, padded rows, the table strides and the count"""
    rng = np.random.default_rng(90210 + seed)
    W, H = FRAME_SIZES[int(rng.integers(len(FRAME_SIZES)))]
    sf = SOURCES[int(rng.integers(len(SOURCES)))]
    dw, dh = DST_SIZES[int(rng.integers(len(DST_SIZES)))]
    n = int(rng.integers(3, 25))
    boxes, rects = [], []
    explicit = bool(rng.integers(2))
    for _ in range(n):
        w, h = int(rng.integers(1, W + 1)), int(rng.integers(1, H + 1))
        if rng.random() < 0.3:  # thin boxes: the fit clamps
            w, h = (int(rng.integers(1, 4)), h) if rng.random() < 0.5 else (w, int(rng.integers(1, 4)))
        x, y = int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1))
        f = int(rng.integers(2))
        kind = rng.random()
        if kind < 0.08:
            x = W - w + 1
        elif kind < 0.12:
            f = 2
        elif kind < 0.16:
            h = 0
        boxes.append((f, x, y, w, h))
        iw, ih = int(rng.integers(1, dw + 1)), int(rng.integers(1, dh + 1))
        ix, iy = int(rng.integers(0, dw - iw + 1)), int(rng.integers(0, dh - ih + 1))
        kind = rng.random()
        if kind < 0.06:
            iw = dw - ix + 1
        elif kind < 0.10:
            iy = -1
        rects.append((ix, iy, iw, ih))
    count = [None, n, int(rng.integers(0, n + 1)), n + 3][int(rng.integers(4))]
    return dict(W=W, H=H, sf=sf, dw=dw, dh=dh, boxes=boxes, rects=rects if explicit else None, dtype=int(rng.integers(3)), bgr=bool(rng.integers(2)),
                nhwc=bool(rng.integers(2)), padded=bool(rng.integers(2)), box_width=int(rng.choice([5, 6, 8])), rect_width=int(rng.choice([4, 6])),
                count=count, cs=int(rng.integers(2)), cr=int(rng.integers(2)))


def box_valid(box, W, H, n_frames=2):
    f, x, y, w, h = box
    return 0 <= f < n_frames and w >= 1 and h >= 1 and x >= 0 and y >= 0 and x + w <= W and y + h <= H


def rect_valid(rect, dw, dh):
    ix, iy, iw, ih = rect
    return iw >= 1 and ih >= 1 and ix >= 0 and iy >= 0 and ix + iw <= dw and iy + ih <= dh
