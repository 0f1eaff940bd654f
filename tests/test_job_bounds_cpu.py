"""The strip sizing of the two per-job kernel families (csrc/vpf_job_bounds.h — the header k_convert_roi.hip and k_convert_warp.hip include, on
host and device) against an independent restatement of the kernels' fp32 arithmetic, on the CPU.  A short bound is silent on the device:
k_roi_strip returns without writing, k_warp_strip blends a pixel from the wrong texels.  The header is compiled with g++ as it stands
(tests/c/job_bounds_capi.cpp); the reference side is numpy float32 and never calls it.

Restated here: make_tap<LINEAR> (k_bilinear_blend.h; fma in fp32: the product of two floats is exact in float64, the sum with -0.5 as well at
these magnitudes, one rounding to float32), the strip geometry of k_roi_strip (k_convert_roi.hip), the coordinates of the warp definition
(include/vpf_hip.h: sx = (m00 dx + m01 dy) + m02, every operation rounded on its own — numpy float32 arrays round every operation, and the
library is built with -ffp-contract=off), vpf_remap's range test, and the unit index of strip_fill_window (k_fused_common.h)."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import cases_job_shapes as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
N_ROI, N_WARP = 3200, 5200
ABI_MAX = 16777216.0   # |matrix entry| limit of vpf_convert_warp_tensor (include/vpf_hip.h)


@pytest.fixture(scope="module")
def jb(tmp_path_factory):
    from conftest import native_test_build
    so = str(tmp_path_factory.mktemp("jb") / "libjobbounds.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-shared", "-fPIC", "-Wall", "-Werror", *native_test_build()[0],
                           "-I" + os.path.join(ROOT, "videoprocessingframework_amd", "csrc"), os.path.join(ROOT, "tests", "c", "job_bounds_capi.cpp"), "-o", so, "-lm"])
    L = C.CDLL(so)
    u32, fp, up = C.c_uint32, C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    for name in ("jb_roi_strip_max", "jb_warp_strip_max", "jb_warp_tile_w", "jb_warp_tile_h"):
        getattr(L, name).argtypes, getattr(L, name).restype = [], u32
    L.jb_roi_conv_max.argtypes, L.jb_roi_conv_max.restype = [], C.c_double
    L.jb_roi_strip_need.argtypes, L.jb_roi_strip_need.restype = [u32] * 5 + [C.POINTER(C.c_double), C.POINTER(C.c_int)], u32
    L.jb_warp_tile.argtypes, L.jb_warp_tile.restype = [fp] + [u32] * 4 + [C.c_int, u32, u32, up], None
    L.jb_warp_tiles.argtypes, L.jb_warp_tiles.restype = [fp, C.c_int] + [u32] * 4 + [up], None
    L.jb_warp_xy.argtypes, L.jb_warp_xy.restype = [fp, u32, u32, C.c_int, u32, u32, fp], None
    L.jb_warp_need.argtypes, L.jb_warp_need.restype = [fp] + [u32] * 4, u32
    assert (L.jb_roi_strip_max(), L.jb_roi_conv_max(), L.jb_warp_strip_max(), L.jb_warp_tile_w(), L.jb_warp_tile_h()) == (53 * 1024, 3.0, 64 * 1024, 32, 32)
    return L


# ------------------------------------------------------------------------------------------------ ROI
def _s(d, scale):
    """fma((float)d + 0.5f, scale, -0.5f) for an array of destination indices"""
    d = np.asarray(d)
    return ((d.astype(F) + F(0.5)).astype(np.float64) * np.float64(scale) - 0.5).astype(F)


def lin_taps(d, S, D):
    """make_tap<LINEAR> of a rectangle side S -> D with the entry's scale (float)S / (float)D: (i0, i1) of destination indices d"""
    s = np.minimum(np.maximum(_s(d, F(F(S) / F(D))), F(0)), F(S - 1))
    i0 = s.astype(np.int64)
    return i0, np.minimum(i0 + 1, S - 1)


def roi_strips(x, y, w, h, dw, dh):
    """what k_roi_strip computes per 256-column chunk (first, last, base_px, ng, rowbytes) and per 16-row band (R_hi - R_lo + 1)"""
    xs = np.arange(0, dw, 256)
    xe = np.minimum(xs + 255, dw - 1)
    first, last = x + lin_taps(xs, w, dw)[0], x + lin_taps(xe, w, dw)[1]
    base_px = first & ~1
    ng = ((last - base_px) >> 3) + 1
    rowbytes = 32 * ng + 16
    y0 = np.arange(0, dh, 16)
    y1 = np.minimum(y0 + 15, dh - 1)
    r_lo, r_hi = y + lin_taps(y0, h, dh)[0], y + lin_taps(y1, h, dh)[1]
    return first, last, base_px, ng, rowbytes, r_hi - r_lo + 1


def roi_need(jb, x, w, h, dw, dh):
    conv, staged = C.c_double(), C.c_int()
    b = jb.jb_roi_strip_need(x, w, h, dw, dh, C.byref(conv), C.byref(staged))
    return b, conv.value, bool(staged.value)


def roi_cases(rng, n):
    """(x, y, w, h, dw, dh): sides 1..4096 at offsets 0..4095, destinations 1..1024 x 1..64 with the chunk and band edges, scales 0.05..12"""
    out = [(301, 3, 517, 33, 256, 20), (0, 0, 1, 1, 1, 1), (4095, 4095, 1, 1, 1024, 64), (0, 0, 4096, 4096, 1024, 64), (4095, 0, 4096, 1, 513, 17),
           (1, 1, 4096, 4096, 342, 1), (3801, 1, 260, 20, 260, 5), (17, 9, 3072, 768, 256, 64), (5, 7, 13, 4, 257, 15)]
    dws, dhs = (255, 256, 257, 511, 512, 513, 1, 4, 1023, 1024), (15, 16, 17, 1, 31, 32, 33, 63, 64)
    while len(out) < n:
        k = len(out)
        dw = dws[k % len(dws)] if k % 2 else int(rng.integers(1, 1025))
        dh = dhs[k % len(dhs)] if k % 3 == 0 else int(rng.integers(1, 65))
        if k % 7 == 0:   # sides drawn on their own: scales far outside 0.05..12 too
            w, h = int(rng.integers(1, 4097)), int(rng.integers(1, 4097))
        else:
            w = int(np.clip(round(dw * math.exp(rng.uniform(math.log(0.05), math.log(12.0)))), 1, 4096))
            h = int(np.clip(round(dh * math.exp(rng.uniform(math.log(0.05), math.log(12.0)))), 1, 4096))
        out.append((int(rng.integers(0, 4096)), int(rng.integers(0, 4096)), w, h, dw, dh))
    return out


def test_roi_strip_need_covers_every_workgroup(jb):
    """roi_strip_need against the strip of every (256-column chunk, 16-row band) workgroup of the job: never short, exactly the product of the
    largest row count and the largest row pitch (what the launcher passes as dynamic LDS), `conv` as defined; and every destination column's two
    tap dwords lie inside its chunk's strip row"""
    rng = np.random.default_rng(20240)
    n_staged = n_gather = n_multi = 0
    for (x, y, w, h, dw, dh) in roi_cases(rng, N_ROI):
        first, last, base_px, ng, rowbytes, rows = roi_strips(x, y, w, h, dw, dh)
        bytes_, conv, staged = roi_need(jb, x, w, h, dw, dh)
        what = (x, y, w, h, dw, dh)
        largest = int((rows[:, None] * rowbytes[None, :]).max())   # every (band, chunk) pair is a workgroup of the grid
        assert largest <= bytes_, what
        assert bytes_ == int(rows.max()) * int(rowbytes.max()), what
        assert conv == float(rows.max()) * (int(rowbytes.max()) // 4) / (float(min(dw, 256)) * min(dh, 16)), what
        assert staged == (bytes_ <= 53 * 1024 and conv <= 3.0), what
        # the blend stage reads two dwords at 4 (i0 - base_px) of its chunk's strip row; the fill stage converts pixels [base_px, base_px + 8 ng)
        cols = np.arange(dw)
        a = 4 * (x + lin_taps(cols, w, dw)[0] - base_px[cols // 256])
        assert int(a.min()) >= 0 and int((a + 8 - rowbytes[cols // 256]).max()) <= 0, what
        assert (last < base_px + 8 * ng).all() and (base_px % 2 == 0).all(), what
        n_staged += staged
        n_gather += not staged
        n_multi += dw > 256
    print(f"ROI: {N_ROI} cases, {n_staged} staged, {n_gather} gather, {n_multi} with more than one chunk")
    assert n_staged > 500 and n_gather > 500 and n_multi > 800


# ------------------------------------------------------------------------------------------------ warp
def warp_cases(rng, n):
    """(matrix as 6 float32, W, H, dw, dh, replicate): rotations of every angle class, scales 0.05..8, shears, flips, the all-zero linear part,
    translations up to +-2^20, entries at the ABI limit, identities landing on W - 1 and half a pixel past it; frames 1 x 1 .. 4096 x 2160;
    destinations 1..224 with the tile edges"""
    frames = [(1, 1), (1, 7), (7, 1), (2, 2), (3, 5), (131, 79), (130, 78), (401, 299), (1100, 40), (1101, 41), (1920, 1080), (1919, 1079), (3840, 2160), (4096, 2160),
              (4095, 2159), (33, 2160), (4096, 3)]
    dsts = [1, 31, 32, 33, 63, 64, 65, 72, 4, 8, 127, 129, 224, 223]
    angles = [0, 90, 180, 270, 45, 135, 30, 60, 15, 1, 89, 179.5, 0.01, 269.99]
    out = []
    while len(out) < n:
        k = len(out)
        W, H = frames[k % len(frames)] if k % 3 else (int(rng.integers(1, 4097)), int(rng.integers(1, 2161)))
        dw = dsts[k % len(dsts)] if k % 2 else int(rng.integers(1, 225))
        dh = dsts[(k // 2) % len(dsts)] if k % 5 < 2 else int(rng.integers(1, 225))
        cls = k % 11
        cx, cy = rng.uniform(-0.2 * W, 1.2 * W), rng.uniform(-0.2 * H, 1.2 * H)   # where the destination's centre lands
        if cls <= 3:      # rotation x scale about the destination centre
            th = math.radians(angles[(k // 11) % len(angles)] if cls < 3 else rng.uniform(0, 360))
            s = math.exp(rng.uniform(math.log(0.05), math.log(8.0)))
            a, b, c, d = s * math.cos(th), -s * math.sin(th), s * math.sin(th), s * math.cos(th)
        elif cls == 4:    # shear, anisotropic scale, flips
            a, d = (rng.choice([-1, 1]) * math.exp(rng.uniform(math.log(0.05), math.log(8.0))) for _ in range(2))
            b, c = rng.uniform(-2, 2), rng.uniform(-2, 2)
        elif cls == 5:    # the all-zero linear part (every pixel samples one point) and single-axis degenerate ones
            a, b, c, d = [(0, 0, 0, 0), (1, 0, 0, 0), (0, 0, 0, 1), (0, 1, 0, 0)][(k // 11) % 4]
        elif cls == 6:    # a pure translation by whole and half pixels
            a, b, c, d = 1, 0, 0, 1
        else:
            a = b = c = d = None
        if cls == 7:      # identity landing exactly on W - 1 / H - 1, and half a pixel past it
            half = 0.5 * ((k // 11) % 2)
            m = [1, 0, W - dw + half, 0, 1, H - dh + half]
        elif cls == 8:    # translations up to +-2^20: coordinates with an ulp of 1/8
            s = math.exp(rng.uniform(math.log(0.05), math.log(8.0)))
            m = [s, rng.uniform(-1, 1), rng.uniform(-2 ** 20, 2 ** 20), rng.uniform(-1, 1), -s, rng.uniform(-2 ** 20, 2 ** 20)]
        elif cls == 9:    # entries at the ABI limit
            m = [rng.uniform(-2, 2) for _ in range(6)]
            for i in rng.choice(6, size=int(rng.integers(1, 7)), replace=False):
                m[i] = ABI_MAX * rng.choice([-1, 1])
        elif cls == 10:   # a large down-scale whose footprint covers the frame several times: every clamp and the frame cap of warp_need
            s = rng.uniform(8, 200)
            m = [s, 0, -rng.uniform(0, s * dw), rng.uniform(-0.5, 0.5), s * rng.uniform(0.2, 1), -rng.uniform(0, s * dh)]
        else:
            m = [a, b, cx - a * (dw - 1) / 2 - b * (dh - 1) / 2, c, d, cy - c * (dw - 1) / 2 - d * (dh - 1) / 2]
            if cls == 6:
                m[2], m[5] = round(2 * m[2]) / 2, round(2 * m[5]) / 2
        out.append((np.array(m, dtype=F), W, H, dw, dh, bool((k // 7) % 2)))
    return out


def warp_coords(m, dw, dh, rep, W, H):
    """the definition's coordinates of every destination pixel: separately rounded float32 operations, REPLICATE a max then a min"""
    fx, fy = np.arange(dw, dtype=F)[None, :], np.arange(dh, dtype=F)[:, None]
    sx = (m[0] * fx + m[1] * fy) + m[2]
    sy = (m[3] * fx + m[4] * fy) + m[5]
    assert sx.dtype == F and sy.dtype == F
    if rep:
        sx = np.minimum(np.maximum(sx, F(0)), F(W - 1))
        sy = np.minimum(np.maximum(sy, F(0)), F(H - 1))
    return sx, sy


def check_warp_job(jb, m, W, H, dw, dh, rep, rng, tiles_max=12):
    """every visited tile of one job, pixel by pixel -> (largest tile strip bytes of ALL tiles, warp_need bytes, pixels checked)"""
    tx, ty = (dw + 31) // 32, (dh + 31) // 32
    win = np.zeros((ty * tx, 10), dtype=np.uint32)
    mp = m.ctypes.data_as(C.POINTER(C.c_float))
    jb.jb_warp_tiles(mp, int(rep), W, H, dw, dh, win.ctypes.data_as(C.POINTER(C.c_uint32)))
    win = win.astype(np.int64).reshape(ty, tx, 10)
    empty = win[..., 4] == 1
    need = jb.jb_warp_need(mp, W, H, dw, dh)
    what = (m.tolist(), W, H, dw, dh, rep)
    # the strip of the window, restated (warp_strip_tile, k_convert_warp_common.h, fills [base_px, base_px + 8 ng) x [y_lo, y_hi])
    base = win[..., 0] & ~1
    ng = ((win[..., 1] - base) >> 3) + 1
    assert ((win[..., 5] == base) & (win[..., 6] == ng) & (win[..., 7] == 32 * ng + 16) & (win[..., 8] == win[..., 3] - win[..., 2] + 1)
            & (win[..., 9] == win[..., 8] * win[..., 7]))[~empty].all(), what
    assert ((win[..., 1] < W) & (win[..., 3] < H) & (win[..., 0] <= win[..., 1]) & (win[..., 2] <= win[..., 3]))[~empty].all(), what
    actual = int(win[..., 9][~empty].max()) if (~empty).any() else 0
    assert actual <= need, (what, actual, need)            # warp_need: every tile's strip fits the bound
    # the pixels: the whole destination at once, every pixel against the window of ITS tile; of a large destination a sample of tiles
    visit = np.ones((ty, tx), bool)
    if ty * tx > tiles_max:
        visit[:] = False
        visit[[0, 0, -1, -1], [0, -1, 0, -1]] = True
        visit.reshape(-1)[rng.choice(ty * tx, size=tiles_max - 4, replace=False)] = True
    sx, sy = warp_coords(m, dw, dh, rep, W, H)
    inr = (sx >= 0) & (sx <= F(W - 1)) & (sy >= 0) & (sy <= F(H - 1))      # vpf_remap's range test
    if rep:
        assert inr.all(), what
    per_px = lambda a: np.repeat(np.repeat(a, 32, axis=0), 32, axis=1)[:dh, :dw]
    seen = per_px(visit)
    in_empty = inr & per_px(empty) & seen
    assert not in_empty.any(), (what, "an in-range pixel in a tile called empty", np.argwhere(in_empty)[0].tolist())
    sel = inr & seen
    x0, y0 = sx[sel].astype(np.int64), sy[sel].astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    lo_x, hi_x, lo_y, hi_y = (per_px(win[..., i])[sel] for i in range(4))
    bad = (x0 < lo_x) | (x1 > hi_x) | (y0 < lo_y) | (y1 > hi_y)
    assert not bad.any(), (what, "a tap outside the tile's window", np.argwhere(sel)[np.argmax(bad)].tolist())
    return actual, need, int(seen.sum())


def test_warp_window_holds_every_tap_and_need_covers_every_tile(jb):
    """warp_window's claim, per pixel: the four corners of a tile bound every in-range tap of the tile (x0, min(x0 + 1, W - 1), y0,
    min(y0 + 1, H - 1) inside [x_lo, x_hi] x [y_lo, y_hi]); `empty` only where no pixel of the tile is in range; every pixel in range under
    REPLICATE.  warp_need: no tile's strip (warp_strip of its window) exceeds the job's bound.  The largest need : actual ratio is printed,
    not asserted: a loose bound costs occupancy, not pixels."""
    rng = np.random.default_rng(20241)
    ratios, n_px, n_over, n_empty_jobs = [], 0, 0, 0
    for (m, W, H, dw, dh, rep) in warp_cases(rng, N_WARP):
        actual, need, px = check_warp_job(jb, m, W, H, dw, dh, rep, rng)
        n_px += px
        n_over += need > 64 * 1024
        if actual:
            ratios.append((need / actual, m.tolist(), W, H, dw, dh, rep, need))
        else:
            n_empty_jobs += 1
    ratios.sort(key=lambda r: r[0])
    print(f"warp: {N_WARP} jobs, {n_px} pixels checked, {n_over} jobs above the strip limit, {n_empty_jobs} wholly outside")
    print(f"warp_need : largest tile strip — largest {ratios[-1][0]:.3f} at {ratios[-1][1:]}, median {ratios[len(ratios) // 2][0]:.3f}, smallest {ratios[0][0]:.3f}")
    fit = [r for r in ratios if r[7] <= 64 * 1024]
    print(f"... among the {len(fit)} jobs the policy stages (need <= 64 KiB): largest {fit[-1][0]:.3f} at {fit[-1][1:]}, median {fit[len(fit) // 2][0]:.3f}")
    assert ratios[0][0] >= 1.0 and n_over > 300 and n_empty_jobs > 100 and len(ratios) > 3000


def test_warp_named_cases(jb):
    """cases kept by name: the matrices of the GPU tests on their frames, every tile visited"""
    rng = np.random.default_rng(3)
    for W, H in cases.WARP_FRAMES:
        for dw, dh in cases.WARP_DESTS:
            for m in cases.warp_mats(W, H, dw, dh):
                for rep in (False, True):
                    check_warp_job(jb, np.array(m, dtype=F), W, H, dw, dh, rep, rng, tiles_max=64)
    for m, W, H, dw, dh in (((1, 0, 70, 0, 1, 44), 131, 79, 61, 35), ((1, 0, 70.5, 0, 1, 44.5), 131, 79, 61, 35), ((0, 0, 5.5, 0, 0, 7.25), 131, 79, 224, 224),
                            ((ABI_MAX, ABI_MAX, ABI_MAX, -ABI_MAX, ABI_MAX, -ABI_MAX), 4096, 2160, 224, 224), ((1, 0, -0.5, 0, 1, -0.5), 1, 1, 33, 33)):
        for rep in (False, True):
            check_warp_job(jb, np.array(m, dtype=F), W, H, dw, dh, rep, rng, tiles_max=64)


def test_warp_xy_is_the_definition(jb):
    """warp_xy, the function the kernels call per pixel, bit for bit the separately rounded float32 expression (no fused multiply-add)"""
    rng = np.random.default_rng(20242)
    out = (C.c_float * 2)()
    for (m, W, H, dw, dh, rep) in warp_cases(rng, 600):
        sx, sy = warp_coords(m, dw, dh, rep, W, H)
        for (x, y) in ((0, 0), (dw - 1, dh - 1), (int(rng.integers(0, dw)), int(rng.integers(0, dh)))):
            jb.jb_warp_xy(m.ctypes.data_as(C.POINTER(C.c_float)), x, y, int(rep), W, H, out)
            assert F(out[0]).tobytes() == sx[y, x].tobytes() and F(out[1]).tobytes() == sy[y, x].tobytes(), (m.tolist(), W, H, x, y, rep)


def test_fill_stage_unit_index_is_integer_division():
    """strip_fill_window maps unit u to (u / ng, u % ng) through (uint32_t)(((float)u + 0.5f) * (1.0f / ng)): equal to integer division for
    every ng and every u < units of every strip within the larger of the two strip limits (64 KiB: rows x (32 ng + 16) bytes; `rows` rows
    lie under at most rows / 2 + 1 chroma rows, one unit per chroma row and group), enumerated exhaustively"""
    limit = 64 * 1024
    total = 0
    for ng in range(1, (limit - 16) // 32 + 1):
        rows = limit // (32 * ng + 16)
        assert rows >= 1
        u = np.arange((rows // 2 + 1) * ng, dtype=np.int64)
        rng_ = F(1.0) / F(ng)
        ci = ((u.astype(F) + F(0.5)) * rng_).astype(np.int64)
        assert np.array_equal(ci, u // ng), (ng, int(np.argmax(ci != u // ng)))
        total += u.size
    assert (limit - 16) // 32 == 2047 and total > 2_900_000


# ------------------------------------------------------------------------------------------------ the case table of tests/test_gpu_job_shapes.py
def test_gpu_case_table_has_both_job_classes(jb):
    """every destination size of the GPU test's ROI table holds at least two staged and two gather jobs on the 1100 x 40 frame, every call (frame,
    size) at least one of each; every warp call at least three staged jobs and one that gathers under the default policy"""
    for dw, dh in cases.ROI_DESTS:
        for W, H in cases.FRAMES:
            rects = cases.roi_rects(W, H, dw, dh)
            assert all(w >= 1 and h >= 1 and x + w <= W and y + h <= H for x, y, w, h in rects), (W, H, dw, dh)
            staged = [roi_need(jb, x, w, h, dw, dh)[2] for x, y, w, h in rects]
            print(f"ROI {W}x{H} -> {dw}x{dh}: {sum(staged)} staged, {len(staged) - sum(staged)} gather")
            few = 2 if (W, H) == cases.FRAMES[0] else 1
            assert sum(staged) >= few and len(staged) - sum(staged) >= few, (W, H, dw, dh, staged)
    for dw, dh in cases.WARP_DESTS:
        for W, H in cases.WARP_FRAMES:
            fits = [jb.jb_warp_need(np.array(m, dtype=F).ctypes.data_as(C.POINTER(C.c_float)), W, H, dw, dh) <= 64 * 1024 for m in cases.warp_mats(W, H, dw, dh)]
            print(f"warp {W}x{H} -> {dw}x{dh}: staged {fits}")
            assert sum(fits) >= 3 and not all(fits), (W, H, dw, dh, fits)
