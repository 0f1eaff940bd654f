"""The fused letterbox with the boxes in DEVICE memory (vpf_convert_letterbox_tensor_dev, PySurfaceConvertResizer.ExecuteLetterboxDevToTensor,
PytorchNvCodec.device_letterbox_to_normalized_tensor, PytorchNvCodec.letterbox_fit_boxes), without a GPU: the symbol, the header and the bindings exist,
the structure has the declared layout, every host-side refusal answers before any device work (fake pointers: nothing here may reach a launch), the
Python entry raises ValueError where it says it does, the fit is ONE function (vpf_letterbox_fit, the kernel's letterbox_fit_ints, torch's
letterbox_fit_boxes agree with the definition in Python's integers), what the kernel decides per tile (csrc/vpf_job_bounds.h, compiled with g++ as it
stands: tests/c/letterbox_dev_bounds_capi.cpp) agrees with what the host-table launcher decides per job and never outgrows the dispatch's LDS, the
placement's guard never lets a rectangle leave the plane, the GPU cases hold every form, and the six kernel instantiations use no scratch and at most
128 VGPRs."""
import ctypes as C
import itertools
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import cases_letterbox_dev as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
NAME = "vpf_convert_letterbox_tensor_dev"
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
FIT_DSTS = [(64, 48), (17, 33), (1, 1), (300, 40)]
N_DRAWS = 2000


@pytest.fixture(scope="module")
def ld(tmp_path_factory):
    from conftest import native_test_build
    so = str(tmp_path_factory.mktemp("ld") / "libletterboxdevbounds.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-shared", "-fPIC", "-Wall", "-Werror", "-Wno-unused-function", *native_test_build()[0],
                           "-I" + os.path.join(ROOT, "videoprocessingframework_amd", "csrc"), os.path.join(ROOT, "tests", "c", "letterbox_dev_bounds_capi.cpp"), "-o", so,
                           "-lm"])
    L = C.CDLL(so)
    u32 = C.c_uint32
    L.ld_fit.argtypes, L.ld_fit.restype = [u32] * 4 + [C.POINTER(u32 * 4)], None
    L.ld_rects_ok.argtypes, L.ld_rects_ok.restype = [C.c_void_p, u32, u32, u32, C.c_void_p], None
    L.ld_lds_bytes.argtypes, L.ld_lds_bytes.restype = [u32, u32], u32
    L.ld_job_need.argtypes, L.ld_job_need.restype = [u32] * 9 + [C.POINTER(C.c_double)], u32
    L.ld_tiles.argtypes, L.ld_tiles.restype = [u32] * 10 + [C.c_void_p] * 4, u32
    L.ld_tile_windows.argtypes, L.ld_tile_windows.restype = [u32] * 9 + [C.c_void_p], u32
    return L


def test_symbol_header_and_bindings_exist(capi):
    assert NAME in capi.EXPORTS and hasattr(capi.lib(), NAME)
    nm = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert f" {NAME}\n" in nm
    assert callable(capi.make_letterbox_dev) and callable(capi.convert_letterbox_tensor_dev)
    h = open(os.path.join(ROOT, "include", "vpf_hip.h")).read()
    for decl in ("typedef struct vpf_letterbox_dev", f"VPF_API vpf_status {NAME}("):
        assert h.index(decl) > h.index("VPF_API vpf_rect vpf_letterbox_fit("), decl
    assert h.index("typedef struct vpf_roi_dev") < h.index("typedef struct vpf_letterbox_dev")
    sys.path.insert(0, os.path.join(ROOT, "videoprocessingframework_amd"))
    nvc = pytest.importorskip("PyNvCodec")
    assert hasattr(nvc.PySurfaceConvertResizer, "ExecuteLetterboxDevToTensor")
    stub = open(os.path.join(ROOT, "videoprocessingframework_amd", "PyNvCodec", "__init__.pyi")).read()
    assert "def ExecuteLetterboxDevToTensor(self, surfaces: List[Surface], boxes_ptr: int, max_n: int, count_ptr: int, rects_ptr: int, ptr: int, dtype: int" in stub
    src = open(os.path.join(ROOT, "videoprocessingframework_amd", "PytorchNvCodec", "__init__.py")).read()
    assert ("def device_letterbox_to_normalized_tensor(resizer, surfaces, boxes, mean, std, count=None, dst_rects=None, pad=(114, 114, 114), "
            "dtype=torch.float32,\n") in src
    assert "def letterbox_fit_boxes(boxes, dw, dh)" in src


def test_struct_layout(capi):
    """vpf_letterbox_dev: 96 bytes with no implicit padding, the fields in the header's order"""
    T = capi.LetterboxDev
    assert C.sizeof(T) == 96 and sum(C.sizeof(t) for _, t in T._fields_) == 96
    assert (T.boxes.offset, T.dst_rects.offset, T.count.offset, T.box_stride.offset, T.rect_stride.offset, T.max_n.offset, T.reserved.offset, T.dst.offset,
            T.dst_job_stride.offset) == (0, 8, 16, 24, 28, 32, 36, 40, 88)
    h = open(os.path.join(ROOT, "include", "vpf_hip.h")).read()
    body = h[h.index("typedef struct vpf_letterbox_dev"):h.index("} vpf_letterbox_dev;")]
    order = [body.index(f) for f in ("boxes;", "dst_rects;", "count;", "box_stride;", "rect_stride;", "max_n;", "reserved;", "dst[3];", "dst_job_stride;")]
    assert order == sorted(order)
    abi = open(os.path.join(ROOT, "videoprocessingframework_amd", "csrc", "vpf_abi.hip")).read()
    assert "static_assert(sizeof(vpf_letterbox_dev) == 96" in abi


def _norm(capi, dtype=0, flags=0, scale=(0.01, 0.01, 0.01), bias=(-1.0, -1.0, -1.0)):
    n = capi.TensorNorm()
    for c in range(3):
        n.scale[c], n.bias[c] = scale[c], bias[c]
    n.dtype, n.flags = dtype, flags
    return n


def test_validation_without_gpu(capi):
    """every host-side refusal, before any device work: every pointer below is fake (boxes, placements and count included: the host never
    dereferences them).  The device-ROI entry's list as it stands, then the new fields."""
    ex = capi.make_exec()
    W, H, dw, dh = 64, 32, 16, 8
    src = [(0x100000, 64), (0x200000, 64)]
    yuv = [(0x100000, 64), (0x200000, 32), (0x300000, 32)]
    f32 = [(0x400000, 64), (0x500000, 64), (0x600000, 64)]  # dw * 4 = 64
    f16 = [(0x400000, 32), (0x500000, 32), (0x600000, 32)]
    BOX, CNT, RCT = 0x700000, 0x800000, 0x900000

    def call(dst=f32, norm=None, sf=capi.NV12, cs=1, cr=0, frames=None, size=(W, H, dw, dh), boxes=BOX, count=CNT, rects=RCT, max_n=7, stride=20, rstride=16,
             job=3 * 8 * 64, n_frames=None, reserved=0, opts=None):
        fr = capi.make_frame_srcs([src] if frames is None else frames)
        t = capi.make_letterbox_dev(boxes, max_n, dst, job, count, rects, stride, rstride, reserved)
        return capi.convert_letterbox_tensor_dev(ex, sf, cs, cr, size[0], size[1], size[2], size[3], fr, t, _norm(capi) if norm is None else norm, opts,
                                                 n_frames=n_frames, check=False)

    # unsupported format, matrix, dtype or flag: the rules of the ROI entry
    assert call(sf=capi.RGB) == capi.ERR_UNSUPPORTED
    assert call(sf=capi.YUV444) == capi.ERR_UNSUPPORTED
    assert call(cs=2) == capi.ERR_UNSUPPORTED
    assert call(cr=2) == capi.ERR_UNSUPPORTED
    assert call(norm=_norm(capi, dtype=3)) == capi.ERR_UNSUPPORTED
    assert call(norm=_norm(capi, dtype=0xFFFFFFFF)) == capi.ERR_UNSUPPORTED
    assert call(norm=_norm(capi, flags=2)) == capi.ERR_UNSUPPORTED
    assert call(norm=_norm(capi, flags=capi.TENSOR_BGR | 0x80000000)) == capi.ERR_UNSUPPORTED
    # the order the header states: the format before everything, dtype and flags before the options' reserved byte, that before a non-finite parameter
    bad_opts = capi.make_letterbox_opts((1, 2, 3))
    bad_opts.reserved = 1
    assert call(opts=bad_opts) == capi.ERR_BAD_ARG
    assert call(opts=bad_opts, norm=_norm(capi, dtype=3)) == capi.ERR_UNSUPPORTED
    assert call(opts=bad_opts, sf=capi.RGB) == capi.ERR_UNSUPPORTED
    assert call(sf=capi.RGB, boxes=0, max_n=0, reserved=1) == capi.ERR_UNSUPPORTED
    assert call(norm=_norm(capi, dtype=3), boxes=0, reserved=1) == capi.ERR_UNSUPPORTED
    # null pointers: exec, the frames, the table, the parameters, the boxes, a plane
    L, Cb = capi.lib(), C.byref
    fr, tb = capi.make_frame_srcs([src]), capi.make_letterbox_dev(BOX, 7, f32, 1536, CNT, RCT)
    args = (capi.NV12, 1, 0, capi.Size(W, H), capi.Size(dw, dh), 1)
    assert getattr(L, NAME)(None, *args, fr, Cb(tb), Cb(_norm(capi)), None) == capi.ERR_BAD_ARG
    assert getattr(L, NAME)(Cb(ex), *args, None, Cb(tb), Cb(_norm(capi)), None) == capi.ERR_BAD_ARG
    assert getattr(L, NAME)(Cb(ex), *args, fr, None, Cb(_norm(capi)), None) == capi.ERR_BAD_ARG
    assert getattr(L, NAME)(Cb(ex), *args, fr, Cb(tb), None, None) == capi.ERR_BAD_ARG
    assert call(boxes=0) == capi.ERR_BAD_ARG
    assert call(frames=[[(0, 64), (0x200000, 64)]]) == capi.ERR_BAD_ARG
    assert call(frames=[src[:1]]) == capi.ERR_BAD_ARG
    assert call(sf=capi.YUV420, frames=[yuv[:2]]) == capi.ERR_BAD_ARG
    assert call(frames=[src, src, src[:1]]) == capi.ERR_BAD_ARG      # every frame is looked at
    assert call(dst=f32[:2]) == capi.ERR_BAD_ARG
    # bad sizes
    for size in ((0, H, dw, dh), (W, 0, dw, dh), (W, H, 0, dh), (W, H, dw, 0), (70000, H, dw, dh), (W, H, 70000, dh)):
        assert call(size=size) == capi.ERR_BAD_ARG, size
    # short pitches; misaligned 16-bit sources
    assert call(frames=[[(0x100000, 63), (0x200000, 64)]]) == capi.ERR_BAD_ARG
    assert call(frames=[[(0x100000, 64), (0x200000, 63)]]) == capi.ERR_BAD_ARG
    assert call(sf=capi.YUV420, frames=[[(0x100000, 64), (0x200000, 31), (0x300000, 32)]]) == capi.ERR_BAD_ARG
    assert call(sf=capi.P10, frames=[[(0x100001, 128), (0x200000, 128)]]) == capi.ERR_BAD_ARG
    assert call(sf=capi.P10, frames=[[(0x100000, 128), (0x200000, 129)]]) == capi.ERR_BAD_ARG
    assert call(sf=capi.P10, frames=[[(0x100000, 126), (0x200000, 128)]]) == capi.ERR_BAD_ARG
    # misaligned or short destination planes, non-finite parameters
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
    nhwc = _norm(capi, flags=capi.TENSOR_NHWC)
    assert call(dst=[(0x400000, 3 * dw * 4 - 4), (0, 0), (0, 0)], norm=nhwc) == capi.ERR_BAD_ARG
    assert call(dst=[(0x400002, 3 * dw * 4), (0, 0), (0, 0)], norm=nhwc) == capi.ERR_BAD_ARG
    for bad in (math.nan, math.inf, -math.inf):
        for c in range(3):
            sc, bi = [0.01] * 3, [-1.0] * 3
            sc[c] = bad
            assert call(norm=_norm(capi, scale=sc)) == capi.ERR_BAD_ARG
            sc[c], bi[c] = 0.01, bad
            assert call(norm=_norm(capi, bias=bi)) == capi.ERR_BAD_ARG
    # the device-ROI entry's fields
    assert call(n_frames=0) == capi.ERR_BAD_ARG
    assert call(frames=[src] * 129) == capi.ERR_BAD_ARG
    for max_n in (0, 65536, 0xFFFFFFFF):
        assert call(max_n=max_n) == capi.ERR_BAD_ARG, max_n
    for boxes in (BOX + 1, BOX + 2, BOX + 3):
        assert call(boxes=boxes) == capi.ERR_BAD_ARG, boxes
    for count in (CNT + 1, CNT + 2, CNT + 3):
        assert call(count=count) == capi.ERR_BAD_ARG, count
    for stride in (0, 4, 16, 19, 21, 22, 23, 30):
        assert call(stride=stride) == capi.ERR_BAD_ARG, stride
    for job in (1, 2, 3, 1537, 1538):
        assert call(job=job) == capi.ERR_BAD_ARG, job
    assert call(dst=f16, norm=_norm(capi, dtype=1), job=769) == capi.ERR_BAD_ARG
    # the new fields: a misaligned dst_rects, a rect_stride below 16 or not a multiple of 4 — with dst_rects only —, a non-zero reserved
    for rects in (RCT + 1, RCT + 2, RCT + 3):
        assert call(rects=rects) == capi.ERR_BAD_ARG, rects
    for rstride in (0, 4, 12, 15, 17, 18, 19, 22):
        assert call(rstride=rstride) == capi.ERR_BAD_ARG, rstride
    for reserved in (1, 0x80000000):
        assert call(reserved=reserved) == capi.ERR_BAD_ARG
        assert call(rects=None, reserved=reserved) == capi.ERR_BAD_ARG
    with pytest.raises(capi.VpfError):
        capi.convert_letterbox_tensor_dev(ex, capi.NV12, 1, 0, W, H, dw, dh, capi.make_frame_srcs([src]), capi.make_letterbox_dev(BOX, 0, f32, 1536), _norm(capi))


class _Resizer:
    """stands in for PySurfaceConvertResizer: a ValueError must come before the resizer is asked to run"""

    def DstSize(self):
        return (16, 8)

    def Stream(self):
        raise AssertionError("validation must come first")

    def ExecuteLetterboxDevToTensor(self, *a, **k):
        raise AssertionError("validation must come first")


def test_python_value_errors():
    """device_letterbox_to_normalized_tensor: device_rois_to_normalized_tensor's ValueErrors — host boxes, another dtype or shape, a host count, too many
    surfaces —, a bad pad, and the same for dst_rects: before the resizer runs"""
    torch = pytest.importorskip("torch")
    from videoprocessingframework_amd import PytorchNvCodec as pnc

    rs, surfs, mean, std = _Resizer(), [object(), object()], (0, 0, 0), (1, 1, 1)
    meta = torch.zeros((3, 5), dtype=torch.int32, device="meta")
    for boxes in (torch.zeros((3, 5), dtype=torch.int32), [(0, 0, 0, 8, 8)], np.zeros((3, 5), np.int32), None, meta):
        with pytest.raises(ValueError):
            pnc.device_letterbox_to_normalized_tensor(rs, surfs, boxes, mean, std)
    with pytest.raises(ValueError):
        pnc.device_letterbox_to_normalized_tensor(rs, surfs, torch.zeros((3, 5), dtype=torch.int32), mean, std, dtype=torch.float64)
    with pytest.raises(ValueError):
        pnc.device_letterbox_to_normalized_tensor(rs, [], torch.zeros((3, 5), dtype=torch.int32), mean, std)
    with pytest.raises(ValueError):
        pnc.device_letterbox_to_normalized_tensor(rs, [object()] * 129, torch.zeros((3, 5), dtype=torch.int32), mean, std)
    for pad in ((1, 2), (1, 2, 256), (-1, 2, 3), (1.5, 2, 3), "abc", None):
        with pytest.raises(ValueError):
            pnc.device_letterbox_to_normalized_tensor(rs, surfs, meta, mean, std, pad=pad)
    for rects in (torch.zeros((3, 4), dtype=torch.int32), [(0, 0, 8, 8)] * 3, np.zeros((3, 4), np.int32)):
        with pytest.raises(ValueError):
            pnc.device_letterbox_to_normalized_tensor(rs, surfs, torch.zeros((3, 5), dtype=torch.int32), mean, std, dst_rects=rects)


def _fit_cases():
    """(w, h, dw, dh): all (w, h) in 1 .. 40 squared into four destinations, the corners where the fit clamps to 1, the tie of the branch
    (w dh == h dw) and the half-up tie (2 h dw + w an exact multiple of 2 w, or its mirror) per destination of the GPU cases"""
    out = [(w, h, dw, dh) for (dw, dh) in FIT_DSTS for w in range(1, 41) for h in range(1, 41)]
    out += [(65536, 1, 640, 640), (1, 65536, 640, 640), (65536, 65536, 640, 640), (65536, 1, 65536, 65536), (1, 65536, 65536, 65536), (1920, 1080, 640, 640)]
    for (dw, dh) in cases.DST_SIZES:
        out += [(*cases.ASPECT[(dw, dh)], dw, dh), (*cases.HALF_UP[(dw, dh)], dw, dh)]
    out += [(128, 3, 64, 48), (2 * 64, 5, 64, 48)]  # the width-limited half-up tie: 2 h dw + w = 2 w (n + 1/2) exactly
    return out


def test_the_ties_are_ties():
    for (dw, dh) in cases.DST_SIZES:
        w, h = cases.ASPECT[(dw, dh)]
        assert w * dh == h * dw and cases.fit(w, h, dw, dh) == (0, 0, dw, dh)
        w, h = cases.HALF_UP[(dw, dh)]
        assert w * dh < h * dw and (2 * w * dh + h) % (2 * h) == 0 and (2 * w * dh) % (2 * h) != 0   # height-limited, iw lands on n + 1/2: rounds up
        assert cases.fit(w, h, dw, dh)[2] == (2 * w * dh + h) // (2 * h) == (w * dh) // h + 1
    for (w, h) in ((128, 3), (128, 5)):
        assert w * 48 >= h * 64 and (2 * h * 64 + w) % (2 * w) == 0 and (h * 64) % w != 0
    assert cases.fit(1920, 1080, 640, 640) == (0, 140, 640, 360)
    assert cases.fit(65536, 1, 640, 640) == (0, 319, 640, 1) and cases.fit(1, 65536, 640, 640) == (319, 0, 1, 640)


def test_the_fit_is_one_function(capi, ld):
    """vpf_letterbox_fit (its results did not change: the definition in Python's integers), the function it now calls and the kernel runs
    (letterbox_fit_ints), and torch's letterbox_fit_boxes: the same four ints everywhere"""
    torch = pytest.importorskip("torch")
    from videoprocessingframework_amd import PytorchNvCodec as pnc

    fits = _fit_cases()
    want = [cases.fit(*c) for c in fits]
    assert [capi.letterbox_fit(*c) for c in fits] == want
    out = (C.c_uint32 * 4)()
    for c, w in zip(fits, want):
        ld.ld_fit(*c, C.byref(out))
        assert tuple(out) == w, c
    by_dst = {}
    for c, w in zip(fits, want):
        by_dst.setdefault(c[2:], []).append((c[:2], w))
    for (dw, dh), rows in by_dst.items():
        boxes = torch.tensor([(1, 7, 9, w, h) for ((w, h), _) in rows], dtype=torch.int64)
        for b in (boxes, boxes.to(torch.int32)):
            got = pnc.letterbox_fit_boxes(b, dw, dh)
            assert got.dtype == torch.int32 and tuple(got.shape) == (len(rows), 4) and got.device.type == "cpu"
            assert got.tolist() == [list(w) for (_, w) in rows], (dw, dh)
    # rows with w < 1 or h < 1 give zeros; the others are untouched by them
    mixed = torch.tensor([(0, 0, 0, 0, 5), (0, 0, 0, 5, 0), (0, 0, 0, -3, 5), (0, 0, 0, 5, I32_MIN), (0, 0, 0, 55, 41), (0, 0, 0, I32_MAX, I32_MAX)], dtype=torch.int32)
    assert pnc.letterbox_fit_boxes(mixed, 64, 48).tolist() == [[0] * 4] * 4 + [list(cases.fit(55, 41, 64, 48)), list(cases.fit(I32_MAX, I32_MAX, 64, 48))]
    assert tuple(pnc.letterbox_fit_boxes(torch.zeros((0, 5), dtype=torch.int32), 64, 48).shape) == (0, 4)
    for bad in (torch.zeros((3, 4), dtype=torch.int32), torch.zeros((3, 5)), torch.zeros(5, dtype=torch.int32)):
        with pytest.raises(ValueError):
            pnc.letterbox_fit_boxes(bad, 64, 48)
    for size in ((0, 48), (64, 0), (65537, 48)):
        with pytest.raises(ValueError):
            pnc.letterbox_fit_boxes(mixed, *size)


def test_placement_guard_never_lets_a_rectangle_leave_the_plane(ld):
    """letterbox_dev_rect_ok against the definition in integers that cannot overflow, for every four ints drawn from {INT32_MIN, -1, 0, 1, dw - 1, dw,
    dw + 1, INT32_MAX} (and dh's), and for random ones"""
    rng = np.random.default_rng(20260)
    for (dw, dh) in ((64, 48), (300, 40), (17, 33), (1, 1), (65536, 65536)):
        xs, ys = sorted({I32_MIN, -1, 0, 1, dw - 1, dw, dw + 1, I32_MAX}), sorted({I32_MIN, -1, 0, 1, dh - 1, dh, dh + 1, I32_MAX})
        corner = np.array(list(itertools.product(xs, ys, xs, ys)), dtype=np.int64)
        near = np.stack([rng.integers(-2, dw + 2, 4000), rng.integers(-2, dh + 2, 4000), rng.integers(-2, dw + 3, 4000), rng.integers(-2, dh + 3, 4000)], axis=1)
        wild = rng.integers(I32_MIN, I32_MAX + 1, size=(4000, 4))
        rects = np.concatenate([corner, near, wild]).astype(np.int32)
        got = np.empty(len(rects), np.uint8)
        ld.ld_rects_ok(rects.ctypes.data, len(rects), dw, dh, got.ctypes.data)
        want = np.array([cases.rect_valid(tuple(int(v) for v in r), dw, dh) for r in rects], dtype=np.uint8)
        bad = np.flatnonzero(got != want)
        assert not len(bad), (dw, dh, rects[bad[:5]].tolist())
        assert want.any() and not want.all()
        ok = rects[got.astype(bool)].astype(np.int64)
        assert (ok[:, 0] >= 0).all() and (ok[:, 1] >= 0).all() and (ok[:, 2] >= 1).all() and (ok[:, 3] >= 1).all()
        assert (ok[:, 0] + ok[:, 2] <= dw).all() and (ok[:, 1] + ok[:, 3] <= dh).all()


def tiles(ld, x, w, h, ix, iy, iw, ih, dw, dh, lds=None):
    n = ((dw + 255) // 256) * ((dh + 15) // 16)
    b, c, s, m = np.empty(n, np.uint32), np.empty(n, np.float64), np.empty(n, np.uint8), np.empty(n, np.uint8)
    got = ld.ld_tiles(x, w, h, ix, iy, iw, ih, dw, dh, ld.ld_lds_bytes(dw, dh) if lds is None else lds, b.ctypes.data, c.ctypes.data, s.ctypes.data, m.ctypes.data)
    assert got == n
    return b, c, s.astype(bool), m.astype(bool)


def _draws(rng, n):
    """(x, w, h, ix, iy, iw, ih, dw, dh): rectangles of frames up to 4096 wide into planes up to 700 x 200, placed by the fit or anywhere"""
    for i in range(n):
        W, H = int(rng.integers(1, 4097)), int(rng.integers(1, 2161))
        w, h = int(rng.integers(1, W + 1)), int(rng.integers(1, H + 1))
        if i % 5 == 0:
            w, h = min(w, int(rng.integers(1, 80))), min(h, int(rng.integers(1, 80)))   # small rectangles: up-scales, staged tiles
        x = int(rng.integers(0, W - w + 1))
        dw, dh = int(rng.integers(1, 701)), int(rng.integers(1, 201))
        if i % 2:
            ix, iy, iw, ih = cases.fit(w, h, dw, dh)
        else:
            iw, ih = int(rng.integers(1, dw + 1)), int(rng.integers(1, dh + 1))
            ix, iy = int(rng.integers(0, dw - iw + 1)), int(rng.integers(0, dh - ih + 1))
        yield (x, w, h, ix, iy, iw, ih, dw, dh)


def test_tile_need_agrees_with_the_job_need_and_fits_the_lds(ld):
    """over the tiles of a job that meet the picture: max(bytes) == letterbox_strip_need.bytes and max(conv) == its conv, exactly; every tile with
    conv <= kRoiConvMax has bytes <= roi_dev_lds_bytes(dw, dh), so the dispatch's LDS never turns a tile away that the policy would stage; without
    LDS (VPF_TUNE_NV12_RGB_VARIANT = 9) no tile is staged; and the tiles that meet the picture are exactly those that overlap it"""
    rng = np.random.default_rng(20261)
    n_staged = n_tap = n_mixed = n_missed = 0
    for (x, w, h, ix, iy, iw, ih, dw, dh) in _draws(rng, N_DRAWS):
        what = (x, w, h, ix, iy, iw, ih, dw, dh)
        conv = C.c_double()
        jb = ld.ld_job_need(x, w, h, ix, iy, iw, ih, dw, dh, C.byref(conv))
        b, c, s, m = tiles(ld, x, w, h, ix, iy, iw, ih, dw, dh)
        assert m.any(), what
        nx = (dw + 255) // 256
        for t in range(len(m)):
            X0, Y0 = 256 * (t % nx), 16 * (t // nx)
            overlap = X0 < ix + iw and min(X0 + 256, dw) > ix and Y0 < iy + ih and min(Y0 + 16, dh) > iy
            assert bool(m[t]) == overlap, (what, t)
        assert int(b[m].max()) == jb, what
        assert float(c[m].max()) == conv.value, what
        lds = ld.ld_lds_bytes(dw, dh)
        assert lds <= 53 * 1024 and lds % 16 == 0
        assert (b[m & (c <= 3.0)] <= lds).all(), what
        assert np.array_equal(s, m & (b <= 53 * 1024) & (c <= 3.0)), what
        assert not s[~m].any() and not b[~m].any()
        assert not tiles(ld, x, w, h, ix, iy, iw, ih, dw, dh, 0)[2].any()
        sm = s[m]
        n_staged += int(sm.all()); n_tap += int(not sm.any()); n_mixed += int(sm.any() and not sm.all()); n_missed += int((~m).any())
    assert n_staged > 200 and n_tap > 200 and n_mixed > 0 and n_missed > 200, (n_staged, n_tap, n_mixed, n_missed)


def test_tile_window_is_the_staged_kernels_make_tap_arithmetic(ld):
    """letterbox_tile_window's first, last, lo, hi of every tile that meets the picture against the clip and the four make_tap<LINEAR> calls of the
    staged form, restated in numpy float32 (test_job_bounds_cpu.lin_taps): the tile's columns and rows clipped to the picture, in picture pixels,
    then first = x + tap(cxs).i0, last = x + tap(cxe).i1, lo = tap(cys).i0, hi = tap(cye).i1 on the rectangle with the scale (float)w / (float)iw.
    Both staged kernels (k_lb_strip, k_lb_dev) fill and address their strip from these four values."""
    from test_job_bounds_cpu import lin_taps
    rng = np.random.default_rng(20261)
    edge = [(0, 1, 1, 0, 0, 1, 1, 1, 1), (7, 640, 360, 0, 0, 1, 1, 1, 1),                  # a 1 x 1 destination
            (5, 300, 40, 0, 0, 257, 16, 257, 16), (0, 31, 9, 200, 1, 57, 2, 257, 3),       # dw = 257: a second tile one column wide
            (3, 200, 90, 0, 0, 64, 17, 64, 17), (0, 8, 5, 10, 15, 100, 2, 256, 17),        # dh = 17: a second band one row high
            (130, 1, 77, 11, 0, 1, 16, 24, 16), (0, 1, 1, 0, 0, 257, 17, 257, 17),         # a rectangle of width 1
            (9, 50, 70, 256, 3, 1, 11, 257, 17), (9, 50, 70, 299, 0, 1, 40, 300, 40), (0, 640, 360, 63, 47, 1, 1, 64, 48)]  # a picture at the plane's last column
    for (x, w, h, ix, iy, iw, ih, dw, dh) in edge + list(_draws(rng, N_DRAWS)):
        what = (x, w, h, ix, iy, iw, ih, dw, dh)
        nx, ny = (dw + 255) // 256, (dh + 15) // 16
        win = np.empty((ny * nx, 4), np.uint32)
        assert ld.ld_tile_windows(x, w, h, ix, iy, iw, ih, dw, dh, win.ctypes.data) == ny * nx
        xs, Y0 = np.arange(0, dw, 256), np.arange(0, dh, 16)
        xe, Y1 = np.minimum(xs + 255, dw - 1), np.minimum(Y0 + 15, dh - 1)
        ixe, iye = ix + iw - 1, iy + ih - 1
        mx, my = ~((xs > ixe) | (xe < ix)), ~((Y0 > iye) | (Y1 < iy))
        assert mx.any() and my.any(), what
        cxs, cxe = np.maximum(xs, ix)[mx] - ix, np.minimum(xe, ixe)[mx] - ix
        cys, cye = np.maximum(Y0, iy)[my] - iy, np.minimum(Y1, iye)[my] - iy
        want = np.zeros((ny, nx, 4), np.int64)
        sub = want[np.ix_(my, mx)]
        sub[..., 0], sub[..., 1] = (x + lin_taps(cxs, w, iw)[0])[None, :], (x + lin_taps(cxe, w, iw)[1])[None, :]
        sub[..., 2], sub[..., 3] = lin_taps(cys, h, ih)[0][:, None], lin_taps(cye, h, ih)[1][:, None]
        want[np.ix_(my, mx)] = sub
        assert np.array_equal(win.astype(np.int64).reshape(ny, nx, 4), want), what


def test_gpu_cases_hold_every_form(ld):
    """the calls of tests/test_gpu_letterbox_dev.py::test_geometry hold padded tiles, staged tiles and per-tap tiles; the whole frame into 24 x 16 is per
    tap; into 300 x 40 some picture crosses column 256 and a row-tile edge; the tall box's picture does not start and end on lane boundaries"""
    forms = {}
    for (W, H) in cases.FRAME_SIZES:
        for (dw, dh) in cases.DST_SIZES:
            rects = cases.geometry_rects(W, H, dw, dh)
            assert all(0 <= x and 0 <= y and w >= 1 and h >= 1 and x + w <= W and y + h <= H for (x, y, w, h) in rects), (W, H, dw, dh)
            got = forms.setdefault((dw, dh), set())
            for (x, y, w, h) in rects:
                f = cases.fit(w, h, dw, dh)
                b, c, s, m = tiles(ld, x, w, h, *f, dw, dh)
                got |= ({"pad"} if (~m).any() else set()) | ({"staged"} if s.any() else set()) | ({"tap"} if (m & ~s).any() else set())
                if (dw, dh) == (300, 40) and f[0] < 256 < f[0] + f[2] and f[1] + f[3] > 16 and f[1] < 16:
                    got.add("crosses")
            whole = cases.fit(W, H, dw, dh)
            if (dw, dh) == (24, 16):
                b, c, s, m = tiles(ld, 0, W, H, *whole, dw, dh)
                assert m.all() and not s.any()
            tall = cases.fit(3, min(70, H - 4), dw, dh)
            assert tall[2] <= 2 and (tall[0] % 4 != 0 or (tall[0] + tall[2]) % 4 != 0)
    assert forms[(64, 48)] >= {"pad", "staged", "tap"} and forms[(300, 40)] >= {"pad", "staged", "crosses"}, forms
    assert "tap" in forms[(24, 16)] and "staged" in forms[(17, 33)] and "pad" in forms[(17, 33)], forms
    for seed in range(cases.FUZZ_DEFAULT):
        c = cases.fuzz_case(seed)
        assert len(c["boxes"]) <= 64 and (c["dw"], c["dh"]) in cases.DST_SIZES
    assert {cases.fuzz_case(s)["rects"] is None for s in range(cases.FUZZ_DEFAULT)} == {True, False}


_DEV_KERNEL = re.compile(r"k_lb_dev<[017], [68]>")  # FC_NV12 = 0, FC_YUV420 = 1, FC_P16 = 7; FC_TENSOR = 6, FC_TENSOR_NHWC = 8


@pytest.mark.timeout(900)
def test_the_six_instantiations_use_no_scratch():
    """resource metadata of the code object only (tools/isa_stats.spills): both layouts of k_lb_dev for NV12, YUV420 and P10 / P12 hold the pad, the
    staged AND the per-tap form in one kernel — no scratch, no spills, at most 128 VGPRs (two workgroups of 256 lanes per SIMD)"""
    import isa_stats

    rows = [r for r in isa_stats.spills(os.path.join(ROOT, "videoprocessingframework_amd", "csrc", "k_convert_letterbox_dev.hip")) if _DEV_KERNEL.search(r[0])]
    assert len(rows) == 6, [r[0] for r in rows]
    assert len({r[0] for r in rows}) == 6
    for name, vgpr, vspill, sspill, scratch in rows:
        print(name[:100], "vgpr", vgpr)
        assert vspill == 0 and sspill == 0 and scratch == 0, (name, vgpr, vspill, sspill, scratch)
        assert vgpr <= 128, (name, vgpr)
