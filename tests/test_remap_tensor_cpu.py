"""The fused per-pixel remap into a normalised tensor (vpf_convert_remap_tensor), without a GPU: the symbols and bindings exist, the structs have the
documented layout, every row of the refusal list answers before any device work (fake pointers: nothing here may reach a launch), the window
arithmetic the kernel shares with the host (csrc/vpf_job_bounds.h: remap_tap / remap_win_*; csrc/vpf_remap_plan.h, compiled with g++ through
tests/c/remap_bounds_capi.cpp) is exact, undistort_maps and maps_max_step do what their docstrings say, and the premise of
tests/test_gpu_remap_tensor.py holds — the ground truth of a remap is composed from the oracle's conversion of the whole frame and its remap of
packed RGB on the maps under test (clamped first under REPLICATE, NaN staying NaN) into a destination pre-filled with the border, and on maps
written as an affine matrix's coordinates it IS tests/test_warp_tensor_cpu.py::warp_reference_u8."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from test_warp_tensor_cpu import warp_maps, warp_reference_u8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
STRIP_MAX = 64 * 1024
FC_NV12, FC_YUV420, FC_P16 = 0, 1, 7


def clamp_maps(sx, sy, W, H, mode):
    """the maps the oracle's remap gets: under REPLICATE a max, then a min (np.maximum / np.minimum keep a NaN)"""
    sx, sy = np.ascontiguousarray(sx, dtype=F32), np.ascontiguousarray(sy, dtype=F32)
    if mode == 1:
        with np.errstate(invalid="ignore"):
            sx, sy = np.minimum(np.maximum(sx, F32(0)), F32(W - 1)), np.minimum(np.maximum(sy, F32(0)), F32(H - 1))
    return np.ascontiguousarray(sx), np.ascontiguousarray(sy)


def remap_reference_u8(orc, sf, cs, cr, W, H, sx, sy, border, mode, rgb=None, src=None):
    """the definition (include/vpf_hip.h): oracle.convert(frame -> RGB_PLANAR, FP32), planes interleaved in numpy, oracle.remap(RGB, FP32) on the maps
    under test into a destination pre-filled with `border` -> [3, dh, dw] bytes.  `rgb`: the converted frame when the caller already has it."""
    if rgb is None:
        st, rgb = orc.convert(getattr(orc, sf), orc.RGB_PLANAR, cs, cr, W, H, src, orc.FP32)
        assert st == 0
    dh, dw = sx.shape
    packed = np.ascontiguousarray(np.stack(rgb, axis=-1).reshape(H, 3 * W))
    cx, cy = clamp_maps(sx, sy, W, H, mode)
    dst = np.ascontiguousarray(np.broadcast_to(np.asarray(border, np.uint8), (dh, dw, 3)).reshape(dh, 3 * dw))
    st, out = orc.remap(orc.RGB, W, H, [packed], cx, cy, orc.FP32, dst=[dst])
    assert st == 0
    return np.ascontiguousarray(out[0].reshape(dh, dw, 3).transpose(2, 0, 1))


def special_coordinates(W, H):
    """the coordinate values the definition names, as (sx, sy) pairs around the in-range point (3.25, 2.5)"""
    nan, inf = F32(np.nan), F32(np.inf)
    wm, hm = F32(W - 1), F32(H - 1)
    x, y = F32(3.25), F32(2.5)
    return [(nan, y), (x, nan), (nan, nan), (inf, y), (-inf, y), (x, inf), (x, -inf), (F32(-0.0), y), (x, F32(-0.0)), (F32(0), F32(0)), (wm, y),
            (np.nextafter(wm, inf), y), (x, hm), (x, np.nextafter(hm, inf)), (wm, hm), (F32(1e30), y), (F32(-1e30), y), (x, F32(1e30)), (x, F32(-1e30)),
            (F32(1e-42), y), (x, F32(1e-42)), (F32(-1e-42), y), (np.nextafter(F32(0), -inf), np.nextafter(F32(0), -inf)), (F32(-1), y), (x, F32(-0.5))]


def sprinkle(sx, sy, W, H, seed):
    """special_coordinates planted at seeded places of a copy of the maps"""
    rng = np.random.default_rng(seed)
    sx, sy = sx.copy(), sy.copy()
    sp = special_coordinates(W, H)
    at = rng.choice(sx.size, size=min(len(sp), sx.size), replace=False)
    for (a, b), k in zip(sp, at):
        sx.flat[k], sy.flat[k] = a, b
    return sx, sy


def test_symbols_and_bindings_exist(capi):
    assert "vpf_convert_remap_tensor" in capi.EXPORTS
    assert hasattr(capi.lib(), "vpf_convert_remap_tensor")
    nm = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert " vpf_convert_remap_tensor\n" in nm
    assert callable(capi.make_remap_jobs) and callable(capi.make_remap_opts) and callable(capi.convert_remap_tensor)
    h = open(os.path.join(ROOT, "include", "vpf_hip.h")).read()
    for decl in ("typedef struct vpf_remap_io", "typedef struct vpf_remap_opts", "VPF_API vpf_status vpf_convert_remap_tensor("):
        assert h.index(decl) > h.index("VPF_API vpf_status vpf_convert_warp_tensor("), decl
    stubs = subprocess.run(["nm", "-C", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for src_fc in (FC_NV12, FC_YUV420, FC_P16):
        for dst_fc in (6, 8):  # FC_TENSOR, FC_TENSOR_NHWC
            assert f"k_remap_tile<{src_fc}, {dst_fc}>" in stubs, (src_fc, dst_fc)


def test_struct_layout(capi):
    """vpf_remap_io is 120 bytes with no implicit padding (6 planes of 16 B, two pointers, two pitches); vpf_remap_opts is 16"""
    R, O = capi.RemapIO, capi.RemapOpts
    assert C.sizeof(R) == 120 and C.sizeof(O) == 16
    assert (R.src.offset, R.dst.offset, R.xmap.offset, R.ymap.offset, R.xmap_pitch.offset, R.ymap_pitch.offset) == (0, 48, 96, 104, 112, 116)
    assert sum(C.sizeof(t) for _, t in R._fields_) == 120
    assert (O.border_mode.offset, O.border.offset, O.reserved.offset, O.max_step.offset, O.reserved2.offset) == (0, 4, 7, 8, 12)


def _norm(capi, dtype=0, flags=0, scale=(0.01, 0.01, 0.01), bias=(-1.0, -1.0, -1.0)):
    n = capi.TensorNorm()
    for c in range(3):
        n.scale[c], n.bias[c] = scale[c], bias[c]
    n.dtype, n.flags = dtype, flags
    return n


def test_validation_without_gpu(capi):
    """every row of the refusal list, before any device work: every pointer below is fake"""
    ex = capi.make_exec()
    W, H, dw, dh = 64, 32, 16, 8
    src = [(0x100000, 64), (0x200000, 64)]
    yuv = [(0x100000, 64), (0x200000, 32), (0x300000, 32)]
    p10 = [(0x100000, 128), (0x200000, 128)]
    f32 = [(0x400000, 64), (0x500000, 64), (0x600000, 64)]  # dw * 4 = 64
    f16 = [(0x400000, 32), (0x500000, 32), (0x600000, 32)]
    xm, ym = (0x700000, 64), (0x800000, 64)
    _none = object()

    def call(dst=f32, norm=None, sf=capi.NV12, cs=1, cr=0, s=src, size=(W, H, dw, dh), x=xm, y=ym, jobs=None, opts=_none):
        jobs = capi.make_remap_jobs([(s, dst, x, y)] if jobs is None else jobs)
        return capi.convert_remap_tensor(ex, sf, cs, cr, size[0], size[1], size[2], size[3], jobs, _norm(capi) if norm is None else norm,
                                         capi.make_remap_opts() if opts is _none else opts, check=False)

    # the warp entry's UNSUPPORTED answers: format, matrix, dtype, flag, border mode
    assert call(sf=capi.RGB) == capi.ERR_UNSUPPORTED
    assert call(sf=capi.YUV444) == capi.ERR_UNSUPPORTED
    assert call(cs=2) == capi.ERR_UNSUPPORTED
    assert call(cr=2) == capi.ERR_UNSUPPORTED
    assert call(norm=_norm(capi, dtype=3)) == capi.ERR_UNSUPPORTED
    assert call(norm=_norm(capi, dtype=0xFFFFFFFF)) == capi.ERR_UNSUPPORTED
    assert call(norm=_norm(capi, flags=2)) == capi.ERR_UNSUPPORTED
    assert call(norm=_norm(capi, flags=capi.TENSOR_BGR | 0x80000000)) == capi.ERR_UNSUPPORTED
    assert call(opts=capi.make_remap_opts(2)) == capi.ERR_UNSUPPORTED
    assert call(opts=capi.make_remap_opts(0xFFFFFFFF)) == capi.ERR_UNSUPPORTED
    # non-zero reserved fields: the options' two, a plane's
    for field in ("reserved", "reserved2"):
        o = capi.make_remap_opts(capi.WARP_REPLICATE, (1, 2, 3), 1.5)
        setattr(o, field, 1)
        assert call(opts=o) == capi.ERR_BAD_ARG, field
    j = capi.make_remap_jobs([(src, f32, xm, ym)])
    j[0].dst[1].reserved = 7
    assert capi.convert_remap_tensor(ex, capi.NV12, 1, 0, W, H, dw, dh, j, _norm(capi), check=False) == capi.ERR_BAD_ARG
    j = capi.make_remap_jobs([(src, f32, xm, ym)])
    j[0].src[0].reserved = 1
    assert capi.convert_remap_tensor(ex, capi.NV12, 1, 0, W, H, dw, dh, j, _norm(capi), check=False) == capi.ERR_BAD_ARG
    # a max_step that is negative or not finite; the options come before the finiteness of scale / bias, unsupported before bad
    for bad in (-1.0, -1e-30, math.nan, math.inf, -math.inf):
        assert call(opts=capi.make_remap_opts(max_step=bad)) == capi.ERR_BAD_ARG, bad
    assert call(opts=capi.make_remap_opts(2, max_step=-1.0)) == capi.ERR_UNSUPPORTED
    # null pointers: exec, the job array, the parameters, a plane, a map
    L, Cb = capi.lib(), C.byref
    good = capi.make_remap_jobs([(src, f32, xm, ym)] * 3)
    assert L.vpf_convert_remap_tensor(None, capi.NV12, 1, 0, capi.Size(W, H), capi.Size(dw, dh), 3, good, Cb(_norm(capi)), None) == capi.ERR_BAD_ARG
    assert L.vpf_convert_remap_tensor(Cb(ex), capi.NV12, 1, 0, capi.Size(W, H), capi.Size(dw, dh), 3, None, Cb(_norm(capi)), None) == capi.ERR_BAD_ARG
    assert L.vpf_convert_remap_tensor(Cb(ex), capi.NV12, 1, 0, capi.Size(W, H), capi.Size(dw, dh), 3, good, None, None) == capi.ERR_BAD_ARG
    assert call(s=[(0, 64), (0x200000, 64)]) == capi.ERR_BAD_ARG
    assert call(s=src[:1]) == capi.ERR_BAD_ARG
    assert call(sf=capi.YUV420, s=yuv[:2]) == capi.ERR_BAD_ARG
    assert call(dst=f32[:2]) == capi.ERR_BAD_ARG
    assert call(x=(0, 64)) == capi.ERR_BAD_ARG
    assert call(y=(0, 64)) == capi.ERR_BAD_ARG
    # a map pointer or pitch that is not a multiple of 4, a pitch below 4 * dw
    for off in (1, 2, 3):
        assert call(x=(xm[0] + off, 64)) == capi.ERR_BAD_ARG
        assert call(y=(ym[0] + off, 64)) == capi.ERR_BAD_ARG
        assert call(x=(xm[0], 64 + off)) == capi.ERR_BAD_ARG
        assert call(y=(ym[0], 64 + off)) == capi.ERR_BAD_ARG
    assert call(x=(xm[0], 60)) == capi.ERR_BAD_ARG
    assert call(y=(ym[0], 60)) == capi.ERR_BAD_ARG
    assert call(x=(xm[0], 0)) == capi.ERR_BAD_ARG
    # n == 0, bad sizes
    assert capi.convert_remap_tensor(ex, capi.NV12, 1, 0, W, H, dw, dh, good, _norm(capi), n=0, check=False) == capi.ERR_BAD_ARG
    for size in ((0, H, dw, dh), (W, 0, dw, dh), (W, H, 0, dh), (W, H, dw, 0), (70000, H, dw, dh), (W, H, 70000, dh)):
        assert call(size=size) == capi.ERR_BAD_ARG, size
    # short pitches: source and destination; misaligned P10 planes
    assert call(s=[(0x100000, 63), (0x200000, 64)]) == capi.ERR_BAD_ARG
    assert call(s=[(0x100000, 64), (0x200000, 63)]) == capi.ERR_BAD_ARG
    assert call(sf=capi.YUV420, s=[(0x100000, 64), (0x200000, 31), (0x300000, 32)]) == capi.ERR_BAD_ARG
    assert call(sf=capi.P10, s=[(p10[0][0] + 1, 128), p10[1]]) == capi.ERR_BAD_ARG
    assert call(sf=capi.P12, s=[p10[0], (p10[1][0], 129)]) == capi.ERR_BAD_ARG
    # misaligned or non-finite tensor parameters
    for dt, planes, elem in ((capi.TENSOR_F32, f32, 4), (capi.TENSOR_F16, f16, 2), (capi.TENSOR_BF16, f16, 2)):
        for k in range(3):
            p = list(planes)
            p[k] = (planes[k][0] + 1, planes[k][1])
            assert call(dst=p, norm=_norm(capi, dtype=dt)) == capi.ERR_BAD_ARG, (dt, k, "pointer")
            p[k] = (planes[k][0], planes[k][1] + 1)
            assert call(dst=p, norm=_norm(capi, dtype=dt)) == capi.ERR_BAD_ARG, (dt, k, "pitch")
            p[k] = (planes[k][0], dw * elem - elem)
            assert call(dst=p, norm=_norm(capi, dtype=dt)) == capi.ERR_BAD_ARG, (dt, k, "short pitch")
            p[k] = (0, planes[k][1])
            assert call(dst=p, norm=_norm(capi, dtype=dt)) == capi.ERR_BAD_ARG, (dt, k, "null")
    for bad in (math.nan, math.inf, -math.inf):
        for c in range(3):
            sc, bi = [0.01] * 3, [-1.0] * 3
            sc[c] = bad
            assert call(norm=_norm(capi, scale=sc)) == capi.ERR_BAD_ARG
            sc[c], bi[c] = 0.01, bad
            assert call(norm=_norm(capi, bias=bi)) == capi.ERR_BAD_ARG
    # one bad job among good ones, beyond the first job table (96 jobs per table): everything is validated before the first launch
    assert call(jobs=[(src, f32, xm, ym)] * 100 + [(src, f32, xm, (ym[0], 60))]) == capi.ERR_BAD_ARG
    with pytest.raises(capi.VpfError):
        capi.convert_remap_tensor(ex, capi.NV12, 1, 0, W, H, dw, dh, capi.make_remap_jobs([(src, f32, (0, 64), ym)]), _norm(capi))


# ------------------------------------------------------------------------------------------------ the window
@pytest.fixture(scope="module")
def rm(tmp_path_factory):
    from conftest import native_test_build
    so = str(tmp_path_factory.mktemp("rm") / "libremapbounds.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-shared", "-fPIC", "-Wall", "-Werror", "-Wno-unused-function", *native_test_build()[0],
                           "-I" + os.path.join(ROOT, "videoprocessingframework_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "remap_bounds_capi.cpp"), "-o", so, "-lm"])
    L = C.CDLL(so)
    u32, vp = C.c_uint32, C.c_void_p
    L.rm_taps.argtypes, L.rm_taps.restype = [vp, vp, u32, C.c_int, u32, u32, vp, vp], None
    L.rm_tile_window.argtypes, L.rm_tile_window.restype = [vp, vp, u32, u32, u32, u32, u32, C.c_int, u32, u32, vp], None
    L.rm_strip_fits.argtypes, L.rm_strip_fits.restype = [u32] * 5, C.c_int
    L.rm_plan.argtypes, L.rm_plan.restype = [C.c_int, C.c_int, u32, u32, u32, u32, u32, C.c_float, C.c_int, vp], None
    L.rm_warp_dev_lds_bytes.argtypes, L.rm_warp_dev_lds_bytes.restype = [C.c_float] + [u32] * 4, u32
    return L


def taps_of(rm, sx, sy, rep, W, H):
    sx, sy = np.ascontiguousarray(sx, dtype=F32).reshape(-1), np.ascontiguousarray(sy, dtype=F32).reshape(-1)
    out, cxy = np.empty((sx.size, 5), np.uint32), np.empty((sx.size, 2), F32)
    rm.rm_taps(sx.ctypes.data, sy.ctypes.data, sx.size, rep, W, H, out.ctypes.data, cxy.ctypes.data)
    return out, cxy


def taps_restated(sx, sy, rep, W, H):
    """the definition on numpy float32: NaN -> the border in both modes; REPLICATE a max, then a min; CONSTANT's test; x0 = (int)sx, x1 = min(x0 + 1, W - 1)"""
    sx, sy = np.asarray(sx, F32).reshape(-1), np.asarray(sy, F32).reshape(-1)
    nan = np.isnan(sx) | np.isnan(sy)
    with np.errstate(invalid="ignore"):
        if rep:
            sx, sy = np.minimum(np.maximum(sx, F32(0)), F32(W - 1)), np.minimum(np.maximum(sy, F32(0)), F32(H - 1))
        inr = ~nan & (sx >= 0) & (sx <= F32(W - 1)) & (sy >= 0) & (sy <= F32(H - 1))
    cx, cy = np.where(inr, sx, F32(0)), np.where(inr, sy, F32(0))
    x0, y0 = cx.astype(np.int64), cy.astype(np.int64)
    return inr, x0, np.minimum(x0 + 1, W - 1), y0, np.minimum(y0 + 1, H - 1), cx, cy


@pytest.mark.parametrize("rep", [0, 1])
@pytest.mark.parametrize("W,H", [(131, 79), (2, 1), (1, 1), (65536, 65536), (640, 360)])
def test_taps_of_special_and_random_coordinates(rm, W, H, rep):
    """remap_tap against the restated definition: the named special values, seeded uniform coordinates around the frame and random BIT PATTERNS
    (denormals, NaNs with payloads, huge values); whatever goes in, every tap lies inside the frame and x0 <= x1, y0 <= y1"""
    rng = np.random.default_rng(4100 + W + rep)
    sp = special_coordinates(W, H)
    sx = np.concatenate([np.array([a for a, _ in sp], F32), rng.uniform(-5, W + 5, 4000).astype(F32), rng.integers(0, 2 ** 32, 4000, dtype=np.uint64).astype(np.uint32).view(F32)])
    sy = np.concatenate([np.array([b for _, b in sp], F32), rng.uniform(-5, H + 5, 4000).astype(F32), rng.integers(0, 2 ** 32, 4000, dtype=np.uint64).astype(np.uint32).view(F32)])
    got, cxy = taps_of(rm, sx, sy, rep, W, H)
    inr, x0, x1, y0, y1, cx, cy = taps_restated(sx, sy, rep, W, H)
    assert np.array_equal(got[:, 0].astype(bool), inr)
    assert np.array_equal(got[:, 1], x0) and np.array_equal(got[:, 2], x1) and np.array_equal(got[:, 3], y0) and np.array_equal(got[:, 4], y1)
    assert np.array_equal(cxy[:, 0].view(np.uint32)[inr], cx.view(np.uint32)[inr]) and np.array_equal(cxy[:, 1].view(np.uint32)[inr], cy.view(np.uint32)[inr])  # -0.0 stays -0.0
    assert (got[:, 1] <= got[:, 2]).all() and (got[:, 2] <= W - 1).all() and (got[:, 3] <= got[:, 4]).all() and (got[:, 4] <= H - 1).all()
    assert not got[~inr][:, [1, 3]].any() and not cxy[~inr].any()  # a pixel that takes the border holds the taps of coordinate (0, 0)
    # the special values' classes
    k = {name: i for i, name in enumerate(["nan_x", "nan_y", "nan_xy", "inf_x", "ninf_x", "inf_y", "ninf_y", "nz_x", "nz_y", "zero", "wmax", "above_w", "hmax", "above_h"])}
    for name in ("nan_x", "nan_y", "nan_xy"):
        assert not inr[k[name]], name  # both modes
    big = W > 4 and H > 3  # (the companion coordinate 3.25, 2.5 lies in the frame)
    if big:
        for name in ("inf_x", "ninf_x", "inf_y", "ninf_y", "above_w", "above_h"):
            assert bool(inr[k[name]]) == bool(rep), name
        for name in ("nz_x", "nz_y", "zero", "wmax", "hmax"):
            assert inr[k[name]], name
        assert (x0[k["wmax"]], x1[k["wmax"]]) == (W - 1, W - 1) and (y0[k["hmax"]], y1[k["hmax"]]) == (H - 1, H - 1)
        if rep:
            assert x0[k["inf_x"]] == W - 1 and x0[k["ninf_x"]] == 0 and y0[k["inf_y"]] == H - 1 and y0[k["ninf_y"]] == 0


def _tile_windows(rm, sx, sy, rep, W, H):
    """{(bx, by): (empty, x_lo, x_hi, y_lo, y_hi, strip bytes)} of maps [dh, dw]"""
    dh, dw = sx.shape
    sx, sy = np.ascontiguousarray(sx, dtype=F32), np.ascontiguousarray(sy, dtype=F32)
    out = {}
    for by in range((dh + 31) // 32):
        for bx in range((dw + 31) // 32):
            o = np.zeros(7, np.uint32)
            rm.rm_tile_window(sx.ctypes.data, sy.ctypes.data, dw, dw, dh, bx, by, rep, W, H, o.ctypes.data)
            out[(bx, by)] = (bool(o[0]), int(o[1]), int(o[2]), int(o[3]), int(o[4]), int(o[5]) | int(o[6]) << 32)
    return out


def _maps_for_windows(kind, dw, dh, W, H, seed):
    rng = np.random.default_rng(seed)
    if kind == "random":
        return rng.uniform(-5, W + 5, (dh, dw)).astype(F32), rng.uniform(-5, H + 5, (dh, dw)).astype(F32)
    if kind == "smooth":
        a = float(rng.uniform(0, 2 * math.pi))
        s = float(rng.uniform(0.4, 2.5))
        return warp_maps((s * math.cos(a), -s * math.sin(a), float(rng.uniform(-10, W)), s * math.sin(a), s * math.cos(a), float(rng.uniform(-10, H))), dw, dh, W, H, 0)
    if kind == "outside":
        return np.full((dh, dw), W + 3, F32), rng.uniform(0, H - 1, (dh, dw)).astype(F32)
    if kind == "nan":
        return np.full((dh, dw), np.nan, F32), np.full((dh, dw), np.nan, F32)
    assert kind == "one"
    sx, sy = np.full((dh, dw), -7, F32), np.full((dh, dw), np.nan, F32)
    k = int(rng.integers(0, dw * dh))
    sx.flat[k], sy.flat[k] = F32(W - 1), F32(rng.uniform(0, H - 1))
    return sx, sy


@pytest.mark.parametrize("rep", [0, 1])
@pytest.mark.parametrize("kind", ["random", "smooth", "outside", "nan", "one"])
def test_tile_window_is_the_smallest_that_holds_every_tap(rm, kind, rep):
    """per destination tile, merged in the kernel's order (lane, wave, workgroup): every in-range pixel's four taps lie inside the window, no smaller
    window holds them (each side is touched by a tap), a tile without an in-range pixel is empty; special values sprinkled in"""
    for n, (W, H, dw, dh) in enumerate([(131, 79, 61, 35), (130, 78, 64, 48), (640, 360, 33, 33), (131, 79, 1, 40), (65536, 65536, 3, 2), (131, 79, 1, 1)]):
        sx, sy = _maps_for_windows(kind, dw, dh, W, H, 900 + n)
        if kind in ("random", "smooth"):
            sx, sy = sprinkle(sx, sy, W, H, 77 + n)
        wins = _tile_windows(rm, sx, sy, rep, W, H)
        inr, x0, x1, y0, y1, _, _ = (a.reshape(dh, dw) for a in taps_restated(sx, sy, rep, W, H))
        for (bx, by), (empty, xl, xh, yl, yh, nbytes) in wins.items():
            t = (slice(32 * by, 32 * by + 32), slice(32 * bx, 32 * bx + 32))
            m = inr[t]
            assert empty == (not m.any()), (kind, W, H, bx, by)
            if empty:
                assert nbytes == 0
                continue
            assert (xl, xh, yl, yh) == (x0[t][m].min(), x1[t][m].max(), y0[t][m].min(), y1[t][m].max()), (kind, W, H, bx, by)
            base, rows = xl & ~1, yh - yl + 1
            assert nbytes == rows * (32 * (((xh - base) >> 3) + 1) + 16)  # warp_strip's layout, in 64 bits
        if kind in ("outside", "nan") and not (kind == "outside" and rep):
            assert all(w[0] for w in wins.values())
        if kind == "one":
            assert sum(not w[0] for w in wins.values()) == 1


def test_strip_fits_in_64_bits(rm):
    """windows of a 65536 x 65536 frame whose rows x row bytes do not fit 32 bits must not wrap into `fits`: the whole frame, and the window of
    8159 units x 49348 rows, whose product is 58304 modulo 2^32 — below the 64 KiB it would be compared with"""
    assert rm.rm_strip_fits(0, 65535, 0, 65535, STRIP_MAX) == 0
    assert (49348 * (32 * 8159 + 16)) % 2 ** 32 == 58304 < STRIP_MAX
    assert rm.rm_strip_fits(0, 8 * 8158, 0, 49347, STRIP_MAX) == 0
    assert rm.rm_strip_fits(0, 130, 0, 78, STRIP_MAX) == 1 and rm.rm_strip_fits(0, 130, 0, 78, 79 * 560 - 1) == 0 and rm.rm_strip_fits(0, 130, 0, 78, 79 * 560) == 1
    assert rm.rm_strip_fits(0, 639, 0, 359, STRIP_MAX) == 0


def test_remap_plan(rm):
    """the documented grid (32 x 32 tiles), 96 jobs per dispatch, warp_dev_lds_bytes' answer for the hint (64 KiB without one), nothing under knob 9, the
    alignment mask of the tensor layouts; refusals"""
    def plan(src_fc=FC_NV12, nhwc=0, dtype=0, W=1920, H=1080, dw=640, dh=640, step=0.0, variant=0):
        o = np.zeros(6, np.uint32)
        rm.rm_plan(src_fc, nhwc, dtype, W, H, dw, dh, step, variant, o.ctypes.data)
        return [int(v) for v in o]

    for (W, H, dw, dh) in [(1920, 1080, 640, 640), (3840, 2160, 1920, 1080), (131, 79, 61, 35), (131, 79, 1, 1), (640, 360, 33, 65), (65536, 65536, 65536, 65536)]:
        for step in (0.0, 1e-3, 0.5, 1.0, 1.37, 3.0, 100.0):
            for variant in (0, 9, 40):
                ok, gx, gy, per, lds, dmask = plan(W=W, H=H, dw=dw, dh=dh, step=step, variant=variant)
                assert (ok, gx, gy, per) == (1, (dw + 31) // 32, (dh + 31) // 32, 96)
                assert lds == (0 if variant == 9 else rm.rm_warp_dev_lds_bytes(step, W, H, dw, dh))
                assert lds <= STRIP_MAX and (step or variant == 9 or lds == STRIP_MAX)
    assert [plan(nhwc=n, dtype=d)[5] for n in (0, 1) for d in (0, 1, 2)] == [15, 7, 7, 15, 15, 15]
    assert all(plan(src_fc=fc)[0] == 1 for fc in (FC_NV12, FC_YUV420, FC_P16))
    assert all(plan(src_fc=fc)[0] == 0 for fc in (2, 3, 4, 5, 6, 8, -1))
    assert plan(W=0)[0] == 0 and plan(dh=0)[0] == 0 and plan(W=65537)[0] == 0 and plan(dw=65537)[0] == 0


@pytest.mark.timeout(900)
def test_the_six_instantiations_spill_nothing_and_use_no_scratch():
    """resource metadata of the code object only (tools/isa_stats.spills): both layouts of k_remap_tile for NV12, YUV420 and P10 / P12 hold the
    border, the staged AND the per-tap form in one kernel — no spilled register (vector or scalar), no scratch, at most 128 VGPRs (two workgroups
    of 256 lanes per SIMD: the 64 KiB of LDS allow no more)"""
    import re
    import sys

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_stats

    rows = [r for r in isa_stats.spills(os.path.join(ROOT, "videoprocessingframework_amd", "csrc", "k_convert_remap.hip")) if re.search(r"k_remap_tile<[017], [68]>", r[0])]
    assert len(rows) == 6 and len({r[0] for r in rows}) == 6, [r[0] for r in rows]
    for name, vgpr, vspill, sspill, scratch in rows:
        print(name[:100], "vgpr", vgpr)
        assert vspill == 0 and sspill == 0 and scratch == 0, (name, vgpr, vspill, sspill, scratch)
        assert vgpr <= 128, (name, vgpr)


# ------------------------------------------------------------------------------------------------ the Python helpers
def _undistort_numpy(K, d, size, Kn=None):
    """the formula of the docstring in float64 numpy, rounded once"""
    K = np.asarray(K, np.float64)
    Kn = K if Kn is None else np.asarray(Kn, np.float64)
    d = list(np.asarray(d, np.float64)) + [0.0]
    k1, k2, p1, p2, k3 = d[:5]
    dw, dh = size
    u, v = np.arange(dw, dtype=np.float64)[None, :], np.arange(dh, dtype=np.float64)[:, None]
    x, y = np.broadcast_to((u - Kn[0, 2]) / Kn[0, 0], (dh, dw)), np.broadcast_to((v - Kn[1, 2]) / Kn[1, 1], (dh, dw))
    r2 = x * x + y * y
    rad = 1.0 + k1 * r2 + k2 * (r2 * r2) + k3 * (r2 * r2 * r2)
    xd = x * rad + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * (x * x))
    yd = y * rad + p1 * (r2 + 2.0 * (y * y)) + 2.0 * p2 * x * y
    return (K[0, 0] * xd + K[0, 2]).astype(F32), (K[1, 1] * yd + K[1, 2]).astype(F32)


def test_undistort_maps():
    """against the float64 restatement (four and five coefficients, a new camera matrix); zero distortion gives the affine map of the two camera
    matrices; ValueError for bad shapes and values"""
    import torch
    from videoprocessingframework_amd import PytorchNvCodec as pnc

    K = [[100.5, 0.0, 64.25], [0.0, 98.75, 39.5], [0.0, 0.0, 1.0]]
    Kn = [[80.0, 0.0, 30.0], [0.0, 82.0, 17.0], [0.0, 0.0, 1.0]]
    for d in ((-0.28, 0.07, 0.001, -0.002), (-0.28, 0.07, 0.001, -0.002, 0.011), (0.2, 0.0, 0.0, 0.0)):
        for new in (None, Kn):
            for size in ((61, 35), (1, 1), (33, 2)):
                sx, sy = pnc.undistort_maps(K, d, size, new_camera_matrix=new)
                assert sx.dtype == torch.float32 and tuple(sx.shape) == (size[1], size[0]) and sx.is_contiguous() and sx.device.type == "cpu"
                wx, wy = _undistort_numpy(K, d, size, new)
                assert np.array_equal(sx.numpy().view(np.uint32), wx.view(np.uint32)) and np.array_equal(sy.numpy().view(np.uint32), wy.view(np.uint32))
    # tensors and arrays are accepted like lists
    a = pnc.undistort_maps(torch.tensor(K, dtype=torch.float64), np.array([0.1, 0.0, 0.0, 0.0]), (8, 4), new_camera_matrix=np.array(Kn))
    b = pnc.undistort_maps(K, [0.1, 0.0, 0.0, 0.0], (8, 4), new_camera_matrix=Kn)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # zero distortion: sx = fx (u - cx') / fx' + cx, an affine map
    sx, sy = pnc.undistort_maps(K, (0, 0, 0, 0), (61, 35), new_camera_matrix=Kn)
    u, v = np.arange(61, dtype=np.float64)[None, :], np.arange(35, dtype=np.float64)[:, None]
    assert np.array_equal(sx.numpy(), np.broadcast_to((100.5 * (((u - 30.0) / 80.0) * 1.0) + 64.25).astype(F32), (35, 61)))
    assert np.array_equal(sy.numpy(), np.broadcast_to((98.75 * (((v - 17.0) / 82.0) * 1.0) + 39.5).astype(F32), (35, 61)))
    ident = pnc.undistort_maps(K, (0, 0, 0, 0, 0), (16, 8))
    assert np.allclose(ident[0].numpy(), np.broadcast_to(np.arange(16, dtype=F32), (8, 16)), atol=1e-4, rtol=0)
    for bad in (dict(camera_matrix=[[1, 0], [0, 1]]), dict(dist_coeffs=(0.1, 0.2, 0.3)), dict(dist_coeffs=(0.1,) * 6), dict(size=(0, 4)), dict(size=(4,)),
                dict(size=(4.5, 4)), dict(dist_coeffs=(math.nan, 0, 0, 0)), dict(new_camera_matrix=[[0.0, 0, 1], [0, 1, 1], [0, 0, 1]]),
                dict(camera_matrix=[[math.inf, 0, 1], [0, 1, 1], [0, 0, 1]])):
        kw = dict(camera_matrix=K, dist_coeffs=(0.1, 0, 0, 0), size=(8, 4))
        kw.update(bad)
        with pytest.raises(ValueError):
            pnc.undistort_maps(**kw)


def test_maps_max_step():
    """on maps of a known matrix the hint is at least max(|m00| + |m01|, |m10| + |m11|) and exceeds it by no more than the rounding of the coordinates
    (each of the two differences: two coordinates of half an ulp each); non-finite neighbours do not count; [N, dh, dw] works; the result is a float32"""
    import torch
    from videoprocessingframework_amd import PytorchNvCodec as pnc

    W, H, dw, dh = 1920, 1080, 61, 35
    for m in ((1.37, -0.41, 300.3, 0.41, 1.37, 20.7), (0.37, 0.0, 20.25, 0.0, 0.37, 11.5), (1, 0, 33, 0, 1, 5), (-2.9, 0.3, 900.1, 0.1, 2.7, -10.2), (0, 0, 5.5, 0, 0, 7.25)):
        sx, sy = warp_maps(m, dw, dh, W, H, 0)
        m32 = np.asarray(m, F32).astype(np.float64)
        bound = max(abs(m32[0]) + abs(m32[1]), abs(m32[3]) + abs(m32[4]))
        slack = 4 * float(np.spacing(F32(max(np.abs(sx).max(), np.abs(sy).max(), 1.0))))
        got = pnc.maps_max_step(torch.from_numpy(sx), torch.from_numpy(sy))
        assert float(F32(got)) == got
        assert bound <= got <= bound + slack, (m, got, bound)
    sx, sy = warp_maps((1.5, 0, 10, 0, 0.5, 3), 8, 6, W, H, 0)
    plain = pnc.maps_max_step(sx, sy)
    assert plain == 1.5
    hx = sx.copy()
    hx[2, 3], hx[4, 4], hx[0, 0] = np.nan, np.inf, -np.inf
    assert pnc.maps_max_step(hx, sy) == 1.5  # the differences next to them are not finite and do not count
    assert pnc.maps_max_step(np.stack([sx, 4 * sx]), np.stack([sy, sy])) == 6.0
    assert pnc.maps_max_step(np.full((4, 4), np.nan, F32), np.full((4, 4), np.nan, F32)) == 0.0
    assert pnc.maps_max_step(np.zeros((1, 1), F32), np.zeros((1, 1), F32)) == 0.0
    up = pnc.maps_max_step(np.array([[0.0, 0.7]], np.float64), np.zeros((1, 2), np.float64))  # float32(0.7) < 0.7: rounded UP, not to nearest
    assert float(F32(0.7)) < 0.7 <= up == float(np.nextafter(F32(0.7), F32(1)))
    for bad in (np.zeros((4,), F32), np.zeros((2, 2), np.int32)):
        with pytest.raises(ValueError):
            pnc.maps_max_step(bad, np.zeros((2, 2), F32))


def test_python_layers_exist():
    import sys

    sys.path.insert(0, os.path.join(ROOT, "videoprocessingframework_amd"))
    import PyNvCodec as nvc  # the project's own extension: a build that does not import is a failure, not a skip
    assert hasattr(nvc.PySurfaceConvertResizer, "ExecuteRemapToTensor")
    stub = open(os.path.join(ROOT, "videoprocessingframework_amd", "PyNvCodec", "__init__.pyi")).read()
    assert "def ExecuteRemapToTensor(self, surfaces: List[Surface], xmap_ptr: int, ymap_ptr: int, ptr: int, dtype: int," in stub
    src = open(os.path.join(ROOT, "videoprocessingframework_amd", "PytorchNvCodec", "__init__.py")).read()
    assert "def remap_to_normalized_tensor(resizer, surfaces, xmap, ymap, mean, std, max_step=None, dtype=torch.float32, bgr=False, border=(0, 0, 0)," in src
    assert "def maps_max_step(xmap, ymap) -> float:" in src
    assert "def undistort_maps(camera_matrix, dist_coeffs, size, new_camera_matrix=None, device=None):" in src


def test_binding_validation_without_gpu():
    """PySurfaceConvertResizer.ExecuteRemapToTensor: ValueError for a bad mean / std, False for a wrong surface, null maps, a refused border, mode,
    pitch, stride or hint — all before any device work (host-memory surfaces, fake device addresses)"""
    import sys

    sys.path.insert(0, os.path.join(ROOT, "videoprocessingframework_amd"))
    import PyNvCodec as nvc  # the project's own extension: a build that does not import is a failure, not a skip
    nvc._UseHostAllocator(True)
    try:
        PF = nvc.PixelFormat
        r = nvc.PySurfaceConvertResizer(64, 32, PF.NV12, 16, 8, PF.RGB_PLANAR, 0, 0)
        good = nvc.Surface.Make(PF.NV12, 64, 32, context=0)
        fake, xm, ym, mean, std = 0x400000, 0x700000, 0x800000, [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
        with pytest.raises(ValueError):
            r.ExecuteRemapToTensor([good], xm, ym, fake, 0, [0, 0, 0], [1, 0, 1])
        assert not r.ExecuteRemapToTensor([], xm, ym, fake, 0, mean, std)
        assert not r.ExecuteRemapToTensor([good], 0, ym, fake, 0, mean, std)
        assert not r.ExecuteRemapToTensor([good], xm, 0, fake, 0, mean, std)
        assert not r.ExecuteRemapToTensor([good], xm, ym, 0, 0, mean, std)
        assert not r.ExecuteRemapToTensor([good], xm + 2, ym, fake, 0, mean, std)                  # a map that is not 4-B aligned
        assert not r.ExecuteRemapToTensor([good], xm, ym, fake, 0, mean, std, xmap_pitch=60)       # below 16 x 4 bytes
        assert not r.ExecuteRemapToTensor([good], xm, ym, fake, 0, mean, std, ymap_pitch=66)       # not a multiple of 4
        assert not r.ExecuteRemapToTensor([good, good], xm, ym, fake, 0, mean, std, map_stride=6)  # the second frame's maps are misaligned
        assert not r.ExecuteRemapToTensor([good], xm, ym, fake, 0, mean, std, max_step=-1.0)
        assert not r.ExecuteRemapToTensor([good], xm, ym, fake, 0, mean, std, max_step=math.inf)
        assert not r.ExecuteRemapToTensor([good], xm, ym, fake, 0, mean, std, border=[0, 256, 0])
        assert not r.ExecuteRemapToTensor([good], xm, ym, fake, 0, mean, std, border_mode=2)
        assert not r.ExecuteRemapToTensor([nvc.Surface.Make(PF.NV12, 32, 32, context=0)], xm, ym, fake, 0, mean, std)    # wrong size
        assert not r.ExecuteRemapToTensor([nvc.Surface.Make(PF.YUV420, 64, 32, context=0)], xm, ym, fake, 0, mean, std)  # wrong format
        assert not r.ExecuteRemapToTensor([good], xm, ym, fake, 3, mean, std)                  # unknown dtype
        assert not r.ExecuteRemapToTensor([good], xm, ym, fake, 0, mean, std, row_stride=66)   # not a multiple of 4
        assert not r.ExecuteRemapToTensor([good], xm, ym, fake, 0, mean, std, row_stride=60)   # below 16 x 4 bytes
    finally:
        nvc._UseHostAllocator(False)


class _Surf:
    def Width(self):
        return 64

    def Height(self):
        return 32


class _Resizer:
    """stands in for PySurfaceConvertResizer: a ValueError must come before the resizer is asked to run"""

    def DstSize(self):
        return (16, 8)

    def Stream(self):
        raise AssertionError("validation must come first")

    def ExecuteRemapToTensor(self, *a, **k):
        raise AssertionError("validation must come first")


def test_python_value_errors():
    """remap_to_normalized_tensor: ValueError for maps on the host (another device than the GPU), another dtype or shape, a border value outside
    0..255, an unknown mode, a bad hint or dtype — before the resizer is asked for anything but its size"""
    import torch
    from videoprocessingframework_amd import PytorchNvCodec as pnc

    rs, surfs, mean, std = _Resizer(), [_Surf(), _Surf()], (0, 0, 0), (1, 1, 1)
    host = torch.zeros((8, 16), dtype=torch.float32)
    meta = torch.empty((8, 16), dtype=torch.float32, device="meta")
    for xm, ym in ((host, host), (meta, meta), (host.numpy(), host.numpy()), (None, None), ([[0.0] * 16] * 8, [[0.0] * 16] * 8)):
        with pytest.raises(ValueError):
            pnc.remap_to_normalized_tensor(rs, surfs, xm, ym, mean, std)
    for kw in (dict(border=(0, 0, 256)), dict(border=(-1, 0, 0)), dict(border=(0, 0)), dict(border=(0.5, 0, 0)), dict(border_mode="reflect"),
               dict(dtype=torch.float64), dict(max_step=-1.0), dict(max_step=math.inf), dict(max_step=math.nan)):
        with pytest.raises(ValueError):
            pnc.remap_to_normalized_tensor(rs, surfs, host, host, mean, std, **kw)


# ------------------------------------------------------------------------------------------------ the premise of the GPU test
@pytest.mark.parametrize("sf", ["NV12", "YUV420"])
def test_premise_affine_maps_give_the_warp_reference(oracle, sf):
    """on warp_maps(m, ...) the composed reference equals warp_reference_u8 for the same matrix, in both modes — for every matrix of the warp test's
    geometry_jobs; and a NaN, which no matrix produces, leaves the border in both modes while an infinity takes the edge under REPLICATE"""
    o = oracle
    W, H, dw, dh = 131, 79, 61, 35
    c30, s30 = 1.3 * math.cos(math.radians(30)), 1.3 * math.sin(math.radians(30))
    ms = [(1, 0, 33, 0, 1, 5), (1, 0, W - dw, 0, 1, H - dh), (1, 0, W - dw + 0.5, 0, 1, H - dh + 0.5), (c30, -s30, 40, s30, c30, -10), (0, -1, 70, 1, 0, 3),
          (-1, 0, 100, 0, 1, 2), (1, 0.35, 10, 0.2, 1, 4), (2.9, 0, -20, 0, 2.9, -10), (0.37, 0, 20.25, 0, 0.37, 11.5), (0, 0, 5.5, 0, 0, 7.25), (1, 0, 500, 0, 1, 0)]
    src = o.synth(getattr(o, sf), W, H, 977)
    st, rgb = o.convert(getattr(o, sf), o.RGB_PLANAR, 1, 0, W, H, src, o.FP32)
    assert st == 0
    border = (7, 114, 250)
    for m in ms:
        sx, sy = warp_maps(m, dw, dh, W, H, 0)  # the UNCLAMPED coordinates: the reference clamps them itself under REPLICATE
        for mode in (0, 1):
            assert np.array_equal(remap_reference_u8(o, sf, 1, 0, W, H, sx, sy, border, mode, rgb=rgb),
                                  warp_reference_u8(o, sf, 1, 0, W, H, m, dw, dh, border, mode, rgb=rgb)), (m, mode)
    sx, sy = warp_maps(ms[0], dw, dh, W, H, 0)
    sx[3, 4], sy[5, 6], sx[7, 8] = np.nan, np.nan, np.inf
    plain = warp_reference_u8(o, sf, 1, 0, W, H, ms[0], dw, dh, border, 0, rgb=rgb)
    for mode in (0, 1):
        got = remap_reference_u8(o, sf, 1, 0, W, H, sx, sy, border, mode, rgb=rgb)
        assert [tuple(got[:, y, x]) for (y, x) in ((3, 4), (5, 6))] == [border, border], mode
        want78 = border if mode == 0 else tuple(int(p[5 + 7, W - 1]) for p in rgb)  # (sy = 5 + 7 exactly: the edge pixel itself)
        assert tuple(got[:, 7, 8]) == want78
        mask = np.ones((dh, dw), bool)
        mask[3, 4] = mask[5, 6] = mask[7, 8] = False
        assert np.array_equal(got[:, mask], plain[:, mask])
