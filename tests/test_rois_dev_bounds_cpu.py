"""What the device-resident ROI kernel (k_convert_roi_dev.hip, vpf_convert_resize_tensor_rois_dev) decides for itself, on the CPU: the header the kernel
includes on host and device (csrc/vpf_job_bounds.h) is compiled with g++ as it stands (tests/c/rois_dev_bounds_capi.cpp).
  roi_dev_box_ok   the ONLY thing between five untrusted ints in device memory and a read outside the frame: against a restatement in Python's
                   unbounded integers, at every corner and for random boxes
  roi_tile_need    the per-tile form of roi_strip_need (what the host entry's launcher walks per job): over all tiles of a job its largest strip and its
                   largest conversion count are the job's
  the GPU cases    tests/cases_rois_dev.py hold tiles of BOTH forms under the kernel's own policy — the GPU test cannot tell, both give the same bits"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cases_rois_dev as cases
from test_job_bounds_cpu import lin_taps, roi_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
N_BOXES, N_JOBS = 6000, 3000


@pytest.fixture(scope="module")
def rd(tmp_path_factory):
    from conftest import native_test_build
    so = str(tmp_path_factory.mktemp("rd") / "libroisdevbounds.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-shared", "-fPIC", "-Wall", "-Werror", "-Wno-unused-function", *native_test_build()[0],
                           "-I" + os.path.join(ROOT, "videoprocessingframework_amd", "csrc"), os.path.join(ROOT, "tests", "c", "rois_dev_bounds_capi.cpp"), "-o", so, "-lm"])
    L = C.CDLL(so)
    u32, i32 = C.c_uint32, C.c_int32
    L.rd_box_ok.argtypes, L.rd_box_ok.restype = [i32] * 5 + [u32] * 3, C.c_int
    L.rd_boxes_ok.argtypes, L.rd_boxes_ok.restype = [C.c_void_p, u32, u32, u32, u32, C.c_void_p], None
    L.rd_lds_bytes.argtypes, L.rd_lds_bytes.restype = [u32, u32], u32
    L.rd_job_need.argtypes, L.rd_job_need.restype = [u32] * 5 + [C.POINTER(C.c_double)], u32
    L.rd_tiles.argtypes, L.rd_tiles.restype = [u32] * 6 + [C.c_void_p] * 3, u32
    L.rd_tile_windows.argtypes, L.rd_tile_windows.restype = [u32] * 5 + [C.c_void_p], u32
    return L


def box_ok(frame, x, y, w, h, n_frames, W, H):
    """the definition (include/vpf_hip.h), in integers that cannot overflow"""
    return 0 <= frame < n_frames and w >= 1 and h >= 1 and x >= 0 and y >= 0 and x + w <= W and y + h <= H


def test_guard_at_the_corners(rd):
    """every combination of the corner values per field: 0, +-1, the size, the size +- 1, INT32_MIN / MAX, values whose 32-bit SUM wraps into range"""
    for W, H, n_frames in ((131, 79, 2), (1, 1, 1), (65536, 65536, 128), (130, 78, 128)):
        xs = sorted({0, 1, -1, W, W - 1, W + 1, W // 2, I32_MIN, I32_MAX, I32_MIN + 1, I32_MAX - 1, I32_MAX - W + 1, -W})
        ys = sorted({0, 1, -1, H, H - 1, H + 1, H // 2, I32_MIN, I32_MAX, I32_MAX - H + 1})
        ws = sorted({0, 1, -1, W, W - 1, W + 1, W // 2, I32_MIN, I32_MAX, I32_MIN + W, 2})
        hs = sorted({0, 1, -3, H, H - 1, H + 1, H + 2, I32_MIN, I32_MAX})
        fs = sorted({0, -1, n_frames, n_frames - 1, n_frames + 1, I32_MIN, I32_MAX, 128, 127})
        boxes = np.array([(f, x, y, w, h) for f in fs for x in xs for y in ys for w in ws for h in hs], dtype=np.int32)
        got = np.empty(len(boxes), np.uint8)
        rd.rd_boxes_ok(boxes.ctypes.data, len(boxes), n_frames, W, H, got.ctypes.data)
        want = np.array([box_ok(*(int(v) for v in b), n_frames, W, H) for b in boxes], dtype=np.uint8)
        bad = np.flatnonzero(got != want)
        assert not len(bad), (W, H, n_frames, boxes[bad[:5]].tolist())
        assert want.any() and not want.all()
    # the sums the unsigned form must not take: x + w wraps to a small number in 32 bits
    assert not rd.rd_box_ok(0, I32_MAX, 0, I32_MAX, 1, 1, 131, 79) and not rd.rd_box_ok(0, 2, 0, -1, 1, 1, 131, 79)
    assert not rd.rd_box_ok(0, -2 ** 31, 0, -2 ** 31, 1, 1, 131, 79) and not rd.rd_box_ok(0, 0, I32_MAX - 3, 1, 8, 1, 131, 79)
    assert rd.rd_box_ok(0, 130, 78, 1, 1, 1, 131, 79) and rd.rd_box_ok(127, 0, 0, 65536, 65536, 128, 65536, 65536)


def test_guard_on_random_boxes(rd):
    rng = np.random.default_rng(20250)
    n_ok = 0
    for W, H, n_frames in ((131, 79, 2), (1920, 1080, 4), (65536, 65536, 128)):
        near = rng.integers(-3, 4, size=(N_BOXES, 5))                       # around the frame's own edges
        base = np.stack([rng.integers(-1, n_frames + 1, N_BOXES), rng.integers(-2, W + 2, N_BOXES), rng.integers(-2, H + 2, N_BOXES),
                         rng.integers(-2, W + 3, N_BOXES), rng.integers(-2, H + 3, N_BOXES)], axis=1)
        fit = base.copy()                                                     # ... and rectangles cut to end exactly at, or just past, the edge
        fit[:, 3] = W - fit[:, 1] + near[:, 3] % 2
        fit[:, 4] = H - fit[:, 2] + near[:, 4] % 2
        wild = rng.integers(I32_MIN, I32_MAX + 1, size=(N_BOXES, 5))          # any five ints
        boxes = np.concatenate([base, fit, wild]).astype(np.int32)
        got = np.empty(len(boxes), np.uint8)
        rd.rd_boxes_ok(boxes.ctypes.data, len(boxes), n_frames, W, H, got.ctypes.data)
        want = np.array([box_ok(*(int(v) for v in b), n_frames, W, H) for b in boxes], dtype=np.uint8)
        assert np.array_equal(got, want), (W, H, boxes[np.flatnonzero(got != want)[:5]].tolist())
        n_ok += int(want.sum())
    assert n_ok > 1000


def tiles(rd, x, w, h, dw, dh, lds=None):
    n = ((dw + 255) // 256) * ((dh + 15) // 16)
    b, c, s = np.empty(n, np.uint32), np.empty(n, np.float64), np.empty(n, np.uint8)
    got = rd.rd_tiles(x, w, h, dw, dh, rd.rd_lds_bytes(dw, dh) if lds is None else lds, b.ctypes.data, c.ctypes.data, s.ctypes.data)
    assert got == n
    return b, c, s.astype(bool)


def test_tile_need_agrees_with_the_job_need(rd):
    """over all tiles of a job: max(bytes) == roi_strip_need.bytes and max(conv) == roi_strip_need.conv, exactly (the same double expression on the
    same integers); and a tile is staged under the dispatch's LDS (roi_dev_lds_bytes) exactly when it is under the host policy's two limits"""
    rng = np.random.default_rng(20251)
    n_staged = n_tap = n_mixed = 0
    for (x, y, w, h, dw, dh) in roi_cases(rng, N_JOBS):
        conv = C.c_double()
        jb = rd.rd_job_need(x, w, h, dw, dh, C.byref(conv))
        b, c, s = tiles(rd, x, w, h, dw, dh)
        what = (x, y, w, h, dw, dh)
        assert int(b.max()) == jb, what
        assert float(c.max()) == conv.value, what
        lds = rd.rd_lds_bytes(dw, dh)
        assert lds <= 53 * 1024 and lds % 16 == 0
        assert np.array_equal(s, (b <= 53 * 1024) & (c <= 3.0)), what    # the LDS of the dispatch never turns a tile away that the policy would stage
        assert np.array_equal(s, tiles(rd, x, w, h, dw, dh, 53 * 1024)[2]), what
        assert not tiles(rd, x, w, h, dw, dh, 0)[2].any()                 # VPF_TUNE_NV12_RGB_VARIANT = 9: no LDS, every tile per tap
        n_staged += int(s.all()); n_tap += int(not s.any()); n_mixed += int(s.any() and not s.all())
    assert n_staged > 300 and n_tap > 300 and n_mixed > 0, (n_staged, n_tap, n_mixed)


def test_tile_window_is_the_staged_kernels_make_tap_arithmetic(rd):
    """roi_tile_window's first, last, lo, hi of every tile against the four make_tap<LINEAR> calls of the staged form, restated in numpy float32
    (test_job_bounds_cpu.lin_taps): first = x + tap(xs).i0, last = x + tap(xe).i1, lo = tap(Y0).i0, hi = tap(Y1).i1 on the rectangle's size.  Both
    staged kernels (k_roi_strip, k_roi_dev) fill and address their strip from these four values."""
    rng = np.random.default_rng(20251)
    edge = [(0, 0, 1, 1, 1, 1), (7, 3, 640, 360, 1, 1),      # a 1 x 1 destination
            (5, 0, 300, 40, 257, 16), (0, 0, 31, 9, 257, 3),  # dw = 257: a second tile one column wide
            (3, 1, 200, 90, 64, 17), (0, 0, 8, 5, 256, 17),   # dh = 17: a second band one row high
            (130, 2, 1, 77, 24, 16), (0, 0, 1, 1, 257, 17),   # a rectangle of width 1
            (4095, 0, 1, 9, 300, 40), (3840, 0, 256, 64, 513, 33)]  # a rectangle that ends at the last column of a 4096-wide frame
    for (x, y, w, h, dw, dh) in edge + list(roi_cases(rng, N_JOBS)):
        nx, ny = (dw + 255) // 256, (dh + 15) // 16
        win = np.empty((ny * nx, 4), np.uint32)
        assert rd.rd_tile_windows(x, w, h, dw, dh, win.ctypes.data) == ny * nx
        xs, Y0 = np.arange(0, dw, 256), np.arange(0, dh, 16)
        xe, Y1 = np.minimum(xs + 255, dw - 1), np.minimum(Y0 + 15, dh - 1)
        first, last = x + lin_taps(xs, w, dw)[0], x + lin_taps(xe, w, dw)[1]
        lo, hi = lin_taps(Y0, h, dh)[0], lin_taps(Y1, h, dh)[1]
        want = np.stack([np.tile(first, ny), np.tile(last, ny), np.repeat(lo, nx), np.repeat(hi, nx)], axis=1)  # band-major
        assert np.array_equal(win.astype(np.int64), want), (x, y, w, h, dw, dh)


def test_gpu_cases_hold_tiles_of_both_forms(rd):
    """the calls of tests/test_gpu_rois_dev.py::test_geometry into 64 x 48 and 24 x 16 hold staged and per-tap tiles in ONE dispatch; the widths a
    reciprocal-multiply would miss are there, at least 40 of them in one call"""
    most = 0
    both = set()
    for (W, H) in cases.FRAME_SIZES:
        for (dw, dh) in cases.DST_SIZES:
            rects = cases.geometry_rects(W, H, dw, dh)
            assert all(0 <= x and 0 <= y and w >= 1 and h >= 1 and x + w <= W and y + h <= H for (x, y, w, h) in rects)
            assert len({cases.frame_of(i) for i in range(len(rects))}) == 2
            st = np.concatenate([tiles(rd, x, w, h, dw, dh)[2] for (x, y, w, h) in rects])
            if st.any() and not st.all():
                both.add((dw, dh))
            most = max(most, len(cases.inexact_sides(W, dw)))
            if (dw, dh) == (24, 16):
                whole = tiles(rd, 0, W, H, dw, dh)[2]
                assert not whole.any()                                     # whole frame -> 24 x 16: per tap
            if (dw, dh) == (300, 40):
                assert len(tiles(rd, 0, W, H, dw, dh)[0]) == 6             # two column chunks x three row bands
    # 131 x 79 into 64 x 128 and 300 x 40 never converts three source pixels per destination pixel: those two calls are all staged (up-scales, the
    # second column chunk, the third row band); the two smaller destinations hold both forms in one dispatch
    assert both == {(64, 48), (24, 16)}, both
    assert most >= 40
    f32 = np.float32
    for w in cases.inexact_sides(131, 24)[:5]:
        assert f32(w) * (f32(1) / f32(24)) != f32(w) / f32(24)
