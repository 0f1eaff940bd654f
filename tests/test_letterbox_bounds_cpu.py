"""The strip sizing of the letterbox kernels (letterbox_strip_need, csrc/vpf_job_bounds.h — the header k_convert_letterbox.hip includes on host and
device) against an independent restatement of the staged kernel's per-workgroup arithmetic, on the CPU.  A short bound is silent on the device:
k_lb_strip returns without writing.  The header is compiled with g++ as it stands (tests/c/letterbox_bounds_capi.cpp); the reference side is
numpy float32 (lin_taps of tests/test_job_bounds_cpu.py: make_tap<LINEAR> restated) and never calls it.

Restated here: the workgroup tiles of k_lb_strip — 256 columns x 16 rows laid on the DESTINATION PLANE —, which of them meet the picture, the clip
of a tile's column and row range to the picture (xs' = max(xs, ix) - ix, xe' = min(xe, ix + iw - 1) - ix, rows likewise) and the strip of the
clipped range (first tap's even pixel, whole units of eight pixels, 32 ng + 16 bytes per row)."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from test_job_bounds_cpu import lin_taps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_CASES = 3000


@pytest.fixture(scope="module")
def lb(tmp_path_factory):
    from conftest import native_test_build
    so = str(tmp_path_factory.mktemp("lb") / "libletterboxbounds.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-shared", "-fPIC", "-Wall", "-Werror", "-Wno-unused-function", *native_test_build()[0],
                           "-I" + os.path.join(ROOT, "videoprocessingframework_amd", "csrc"), os.path.join(ROOT, "tests", "c", "letterbox_bounds_capi.cpp"),
                           "-o", so, "-lm"])
    L = C.CDLL(so)
    u32 = C.c_uint32
    L.lb_strip_need.argtypes, L.lb_strip_need.restype = [u32] * 9 + [C.POINTER(C.c_double), C.POINTER(C.c_int)], u32
    L.lb_roi_strip_need.argtypes, L.lb_roi_strip_need.restype = [u32] * 5 + [C.POINTER(C.c_double)], u32
    return L


def need(lb, x, w, h, ix, iy, iw, ih, dw, dh):
    conv, staged = C.c_double(), C.c_int()
    b = lb.lb_strip_need(x, w, h, ix, iy, iw, ih, dw, dh, C.byref(conv), C.byref(staged))
    return b, conv.value, bool(staged.value)


def tile_strips(x, w, h, ix, iy, iw, ih, dw, dh):
    """per chunk that meets the picture (clipped first / last picture column, first, last, base_px, ng, rowbytes) and per band that meets it the
    strip's row count — what k_lb_strip computes in the workgroups that do not leave before the barrier"""
    xs = np.arange(0, dw, 256)
    xe = np.minimum(xs + 255, dw - 1)
    hit = (xs <= ix + iw - 1) & (xe >= ix)
    xs, xe = xs[hit], xe[hit]
    cs, ce = np.maximum(xs, ix) - ix, np.minimum(xe, ix + iw - 1) - ix
    first, last = x + lin_taps(cs, w, iw)[0], x + lin_taps(ce, w, iw)[1]
    base_px = first & ~1
    ng = ((last - base_px) >> 3) + 1
    y0 = np.arange(0, dh, 16)
    y1 = np.minimum(y0 + 15, dh - 1)
    hit = (y0 <= iy + ih - 1) & (y1 >= iy)
    y0, y1 = y0[hit], y1[hit]
    r0, r1 = np.maximum(y0, iy) - iy, np.minimum(y1, iy + ih - 1) - iy
    rows = lin_taps(r1, h, ih)[1] - lin_taps(r0, h, ih)[0] + 1
    return xs, cs, ce, first, last, base_px, ng, 32 * ng + 16, rows


def cases(rng, n):
    """(x, w, h, ix, iy, iw, ih, dw, dh): pictures placed just below and just above the multiples of 256 columns and of 16 rows, 1 x 1 rectangles and
    pictures, pictures that are the whole destination, scales 0.05 .. 12"""
    out = [(301, 517, 33, 0, 0, 256, 20, 256, 20), (0, 1, 1, 0, 0, 1, 1, 1, 1), (17, 55, 41, 252, 12, 8, 20, 260, 70), (17, 55, 41, 256, 16, 4, 16, 260, 70),
           (17, 55, 41, 259, 0, 1, 70, 260, 70), (4095, 1, 1, 1023, 63, 1, 1, 1024, 64), (0, 4096, 4096, 0, 0, 1024, 64, 1024, 64),
           (3, 1, 1, 255, 15, 2, 2, 600, 40), (3, 1, 1, 100, 3, 300, 30, 600, 40)]
    while len(out) < n:
        k = len(out)
        dw, dh = int(rng.integers(1, 1025)), int(rng.integers(1, 65))
        if k % 5 == 0:   # the picture is the whole destination
            ix, iy, iw, ih = 0, 0, dw, dh
        else:
            if k % 2 and dw > 256:   # ix around a multiple of 256
                ix = min(dw - 1, max(0, 256 * int(rng.integers(1, (dw - 1) // 256 + 1)) + int(rng.integers(-2, 3))))
            else:
                ix = int(rng.integers(0, dw))
            if k % 3 == 0 and dh > 16:   # iy around a multiple of 16
                iy = min(dh - 1, max(0, 16 * int(rng.integers(1, (dh - 1) // 16 + 1)) + int(rng.integers(-2, 3))))
            else:
                iy = int(rng.integers(0, dh))
            iw, ih = int(rng.integers(1, dw - ix + 1)), int(rng.integers(1, dh - iy + 1))
        if k % 11 == 0:
            w, h = 1, 1
        elif k % 7 == 0:   # sides drawn on their own: scales far outside 0.05 .. 12 too
            w, h = int(rng.integers(1, 4097)), int(rng.integers(1, 4097))
        else:
            w = int(np.clip(round(iw * math.exp(rng.uniform(math.log(0.05), math.log(12.0)))), 1, 4096))
            h = int(np.clip(round(ih * math.exp(rng.uniform(math.log(0.05), math.log(12.0)))), 1, 4096))
        out.append((int(rng.integers(0, 4096)), w, h, ix, iy, iw, ih, dw, dh))
    return out


def test_letterbox_strip_need_covers_every_workgroup(lb):
    """never short: every (chunk, band) pair that meets the picture is a workgroup with a strip; the bound is exactly the product of the largest row
    count and the largest row pitch; `conv` as defined; every picture column's two tap dwords lie inside its chunk's strip row; with the picture
    = the whole destination the bound equals roi_strip_need's"""
    rng = np.random.default_rng(20250)
    n_staged = n_gather = n_edge_x = n_edge_y = n_whole = n_1x1 = 0
    for (x, w, h, ix, iy, iw, ih, dw, dh) in cases(rng, N_CASES):
        what = (x, w, h, ix, iy, iw, ih, dw, dh)
        xs, cs, ce, first, last, base_px, ng, rowbytes, rows = tile_strips(x, w, h, ix, iy, iw, ih, dw, dh)
        assert len(xs) and len(rows), what   # the picture lies inside the destination: some tile meets it
        bytes_, conv, staged = need(lb, x, w, h, ix, iy, iw, ih, dw, dh)
        largest = int((rows[:, None] * rowbytes[None, :]).max())
        assert largest <= bytes_, what
        assert bytes_ == int(rows.max()) * int(rowbytes.max()), what
        assert conv == float(rows.max()) * (int(rowbytes.max()) // 4) / (float(min(iw, 256)) * min(ih, 16)), what
        assert staged == (bytes_ <= 53 * 1024 and conv <= 3.0), what
        # the blend stage reads two dwords at 4 (i0 - base_px) of its chunk's strip row, for every picture column of the chunk (columns outside
        # the picture are clamped to the chunk's clipped range first); the fill stage converts pixels [base_px, base_px + 8 ng)
        cols = np.arange(iw)
        chunk = (cols + ix) // 256 - xs[0] // 256
        a = 4 * (x + lin_taps(cols, w, iw)[0] - base_px[chunk])
        assert int(a.min()) >= 0 and int((a + 8 - rowbytes[chunk]).max()) <= 0, what
        assert (cs[chunk] <= cols).all() and (cols <= ce[chunk]).all(), what
        assert (last < base_px + 8 * ng).all() and (base_px % 2 == 0).all() and (first >= x).all() and (last <= x + w - 1).all(), what
        if (ix, iy, iw, ih) == (0, 0, dw, dh):
            rconv = C.c_double()
            assert bytes_ == lb.lb_roi_strip_need(x, w, h, dw, dh, C.byref(rconv)) and conv == rconv.value, what
            n_whole += 1
        n_staged += staged
        n_gather += not staged
        n_edge_x += ix >= 254 and (ix + 2) % 256 <= 4
        n_edge_y += iy >= 14 and (iy + 2) % 16 <= 4
        n_1x1 += (w, h) == (1, 1)
    print(f"letterbox: {N_CASES} cases, {n_staged} staged, {n_gather} gather, {n_edge_x} / {n_edge_y} at chunk / band edges, {n_whole} whole, {n_1x1} 1 x 1")
    assert n_staged > 500 and n_gather > 300 and n_edge_x > 300 and n_edge_y > 300 and n_whole > 500 and n_1x1 > 200


def test_roi_and_warp_bounds_are_untouched():
    """the new function was ADDED to vpf_job_bounds.h: the ROI and warp functions keep their text (tests/test_job_bounds_cpu.py checks what they compute)"""
    src = open(os.path.join(ROOT, "videoprocessingframework_amd", "csrc", "vpf_job_bounds.h")).read()
    for name in ("static inline RoiStripNeed roi_strip_need(", "static inline bool roi_job_staged(", "static inline WarpNeed warp_need(",
                 "static inline RoiStripNeed letterbox_strip_need("):
        assert src.count(name) == 1, name
