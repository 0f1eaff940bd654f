"""The fused multi-ROI crop + resize into a normalised tensor (vpf_convert_resize_tensor_rois, PySurfaceConvertResizer.ExecuteRoisToTensor,
PytorchNvCodec.rois_to_normalized_tensor), without a GPU: the symbols and bindings exist, every validation rule answers before any device
work (fake pointers: nothing here may reach a launch), the Python entry raises ValueError where it says it does, and the premise of
tests/test_gpu_roi_tensor.py holds — the oracle's fused convert + resize equals its conversion of the whole frame, a numpy crop, and its
plain RGB_PLANAR resize (so the ground truth of a rectangle at ANY offset can be composed from the three)."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def roi_reference_u8(orc, sf, cs, cr, W, H, src, rect, dw, dh, rgb=None):
    """the definition (include/vpf_hip.h): oracle.convert(frame -> RGB_PLANAR), crop in numpy, oracle.resize(RGB_PLANAR, LINEAR) -> [3, dh, dw] bytes.
    `rgb`: the converted frame when the caller already has it."""
    if rgb is None:
        st, rgb = orc.convert(getattr(orc, sf), orc.RGB_PLANAR, cs, cr, W, H, src, orc.FP32)
        assert st == 0
    x, y, w, h = rect
    crop = [p[y:y + h, x:x + w] for p in rgb]  # views: pitch = the frame's, like plane pointers advanced by y * pitch + x
    st, out = orc.resize(orc.RGB_PLANAR, orc.LINEAR, w, h, crop, dw, dh, orc.FP32)
    assert st == 0
    return np.stack(out)


def test_symbols_and_bindings_exist(capi):
    assert "vpf_convert_resize_tensor_rois" in capi.EXPORTS
    assert hasattr(capi.lib(), "vpf_convert_resize_tensor_rois")
    nm = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert " vpf_convert_resize_tensor_rois\n" in nm
    assert callable(capi.make_rois) and callable(capi.convert_resize_tensor_rois)
    sys.path.insert(0, os.path.join(ROOT, "videoprocessingframework_amd"))
    nvc = pytest.importorskip("PyNvCodec")
    assert hasattr(nvc.PySurfaceConvertResizer, "ExecuteRoisToTensor")
    stub = open(os.path.join(ROOT, "videoprocessingframework_amd", "PyNvCodec", "__init__.pyi")).read()
    assert "def ExecuteRoisToTensor(" in stub
    src = open(os.path.join(ROOT, "videoprocessingframework_amd", "PytorchNvCodec", "__init__.py")).read()
    assert "def rois_to_normalized_tensor(resizer, surfaces, rois, mean, std, dtype=torch.float32, bgr=False, out=None, cc_ctx=None)" in src
    h = open(os.path.join(ROOT, "include", "vpf_hip.h")).read()
    for decl in ("typedef struct vpf_rect", "typedef struct vpf_roi_io", "VPF_API vpf_status vpf_convert_resize_tensor_rois("):
        assert h.index(decl) > h.index("VPF_API vpf_status vpf_convert_resize_tensor_batch("), decl


def test_struct_layout(capi):
    """vpf_roi_io is 112 bytes with no implicit padding: 6 planes of 16 B, then the rectangle"""
    C = capi.C
    assert C.sizeof(capi.Rect) == 16 and C.sizeof(capi.Plane) == 16
    assert C.sizeof(capi.RoiIO) == 112
    assert (capi.RoiIO.src.offset, capi.RoiIO.dst.offset, capi.RoiIO.rect.offset) == (0, 48, 96)
    assert sum(C.sizeof(t) for _, t in capi.RoiIO._fields_) == 112
    assert [n for n, _ in capi.Rect._fields_] == ["x", "y", "width", "height"]


def _norm(capi, dtype=0, flags=0, scale=(0.01, 0.01, 0.01), bias=(-1.0, -1.0, -1.0)):
    n = capi.TensorNorm()
    for c in range(3):
        n.scale[c], n.bias[c] = scale[c], bias[c]
    n.dtype, n.flags = dtype, flags
    return n


def test_validation_without_gpu(capi):
    """every row of the validation table, before any device work: the plane pointers below are fake"""
    ex = capi.make_exec()
    W, H, dw, dh = 64, 32, 16, 8
    src = [(0x100000, 64), (0x200000, 64)]
    yuv = [(0x100000, 64), (0x200000, 32), (0x300000, 32)]
    f32 = [(0x400000, 64), (0x500000, 64), (0x600000, 64)]  # dw * 4 = 64
    f16 = [(0x400000, 32), (0x500000, 32), (0x600000, 32)]
    rect = (3, 5, 20, 10)

    def call(dst=f32, norm=None, sf=capi.NV12, cs=1, cr=0, s=src, size=(W, H, dw, dh), r=rect, jobs=None):
        jobs = capi.make_rois([(s, dst, r)] if jobs is None else jobs)
        return capi.convert_resize_tensor_rois(ex, sf, cs, cr, size[0], size[1], size[2], size[3], jobs, _norm(capi) if norm is None else norm, check=False)

    # unsupported format, matrix, dtype or flag: the rules of vpf_convert_resize_tensor
    assert call(sf=capi.RGB) == capi.ERR_UNSUPPORTED
    assert call(sf=capi.YUV444) == capi.ERR_UNSUPPORTED
    assert call(cs=2) == capi.ERR_UNSUPPORTED
    assert call(cr=2) == capi.ERR_UNSUPPORTED
    assert call(norm=_norm(capi, dtype=3)) == capi.ERR_UNSUPPORTED
    assert call(norm=_norm(capi, dtype=0xFFFFFFFF)) == capi.ERR_UNSUPPORTED
    assert call(norm=_norm(capi, flags=2)) == capi.ERR_UNSUPPORTED
    assert call(norm=_norm(capi, flags=capi.TENSOR_BGR | 0x80000000)) == capi.ERR_UNSUPPORTED
    # null pointers: exec, the job array, the parameters, a plane
    L, Cb = capi.lib(), capi.C.byref
    good = capi.make_rois([(src, f32, rect)] * 3)
    assert L.vpf_convert_resize_tensor_rois(None, capi.NV12, 1, 0, capi.Size(W, H), capi.Size(dw, dh), 3, good, Cb(_norm(capi))) == capi.ERR_BAD_ARG
    assert L.vpf_convert_resize_tensor_rois(Cb(ex), capi.NV12, 1, 0, capi.Size(W, H), capi.Size(dw, dh), 3, None, Cb(_norm(capi))) == capi.ERR_BAD_ARG
    assert L.vpf_convert_resize_tensor_rois(Cb(ex), capi.NV12, 1, 0, capi.Size(W, H), capi.Size(dw, dh), 3, good, None) == capi.ERR_BAD_ARG
    assert call(s=[(0, 64), (0x200000, 64)]) == capi.ERR_BAD_ARG
    assert call(s=src[:1]) == capi.ERR_BAD_ARG
    assert call(sf=capi.YUV420, s=yuv[:2]) == capi.ERR_BAD_ARG
    assert call(dst=f32[:2]) == capi.ERR_BAD_ARG
    # n == 0
    assert capi.convert_resize_tensor_rois(ex, capi.NV12, 1, 0, W, H, dw, dh, good, _norm(capi), n=0, check=False) == capi.ERR_BAD_ARG
    # bad sizes
    for size in ((0, H, dw, dh), (W, 0, dw, dh), (W, H, 0, dh), (W, H, dw, 0), (70000, H, dw, dh), (W, H, 70000, dh)):
        assert call(size=size) == capi.ERR_BAD_ARG, size
    # an empty rect; a rect outside the frame (no silent clipping), 32-bit wrap-around included
    for r in ((3, 5, 0, 10), (3, 5, 20, 0), (0, 0, 0, 0)):
        assert call(r=r) == capi.ERR_BAD_ARG, r
    for r in ((45, 5, 20, 10), (3, 23, 20, 10), (64, 0, 1, 1), (0, 32, 1, 1), (0, 0, 65, 32), (0, 0, 64, 33), (0xFFFFFFFF, 0, 2, 2),
              (0, 0xFFFFFFF0, 2, 0x20), (2, 0, 0xFFFFFFFF, 1)):
        assert call(r=r) == capi.ERR_BAD_ARG, r
    # short pitches: source and destination
    assert call(s=[(0x100000, 63), (0x200000, 64)]) == capi.ERR_BAD_ARG
    assert call(s=[(0x100000, 64), (0x200000, 63)]) == capi.ERR_BAD_ARG
    assert call(sf=capi.YUV420, s=[(0x100000, 64), (0x200000, 31), (0x300000, 32)]) == capi.ERR_BAD_ARG
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
    jobs = [(src, f32, rect)] * 100 + [(src, f32, (60, 5, 20, 10))]
    assert call(jobs=jobs) == capi.ERR_BAD_ARG
    with pytest.raises(capi.VpfError):
        capi.convert_resize_tensor_rois(ex, capi.NV12, 1, 0, W, H, dw, dh, capi.make_rois([(src, f32, (60, 5, 20, 10))]), _norm(capi))


def test_binding_validation_without_gpu():
    """PySurfaceConvertResizer.ExecuteRoisToTensor: ValueError for a bad mean / std, False for a wrong surface, a bad index or a bad rectangle — all
    before any device work (host-memory surfaces, a fake destination address)"""
    sys.path.insert(0, os.path.join(ROOT, "videoprocessingframework_amd"))
    nvc = pytest.importorskip("PyNvCodec")
    nvc._UseHostAllocator(True)
    try:
        PF = nvc.PixelFormat
        r = nvc.PySurfaceConvertResizer(64, 32, PF.NV12, 16, 8, PF.RGB_PLANAR, 0, 0)
        good = nvc.Surface.Make(PF.NV12, 64, 32, context=0)
        fake, mean, std = 0x400000, [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
        with pytest.raises(ValueError):
            r.ExecuteRoisToTensor([good], [(0, 0, 0, 8, 8)], fake, 0, [0, 0, 0], [1, 0, 1])
        with pytest.raises(ValueError):
            r.ExecuteRoisToTensor([good], [(0, 0, 0, 8, 8)], fake, 0, [math.nan, 0, 0], [1, 1, 1])
        assert not r.ExecuteRoisToTensor([good], [], fake, 0, mean, std)
        assert not r.ExecuteRoisToTensor([], [(0, 0, 0, 8, 8)], fake, 0, mean, std)
        assert not r.ExecuteRoisToTensor([good], [(1, 0, 0, 8, 8)], fake, 0, mean, std)      # no such surface
        assert not r.ExecuteRoisToTensor([good], [(0, -1, 0, 8, 8)], fake, 0, mean, std)     # negative
        assert not r.ExecuteRoisToTensor([good], [(0, 60, 0, 8, 8)], fake, 0, mean, std)     # leaves the surface
        assert not r.ExecuteRoisToTensor([good], [(0, 0, 0, 8, 0)], fake, 0, mean, std)      # empty
        assert not r.ExecuteRoisToTensor([nvc.Surface.Make(PF.NV12, 32, 32, context=0)], [(0, 0, 0, 8, 8)], fake, 0, mean, std)   # wrong size
        assert not r.ExecuteRoisToTensor([nvc.Surface.Make(PF.YUV420, 64, 32, context=0)], [(0, 0, 0, 8, 8)], fake, 0, mean, std)  # wrong format
        assert not r.ExecuteRoisToTensor([good], [(0, 1, 1, 8, 8)], fake, 3, mean, std)                  # unknown dtype
        assert not r.ExecuteRoisToTensor([good], [(0, 1, 1, 8, 8)], fake, 0, mean, std, row_stride=66)   # not a multiple of 4
        assert not r.ExecuteRoisToTensor([good], [(0, 1, 1, 8, 8)], fake, 0, mean, std, row_stride=60)   # below 16 x 4 bytes
        with pytest.raises(TypeError):
            r.ExecuteRoisToTensor([good], [(0, 1.5, 1, 8, 8)], fake, 0, mean, std)
    finally:
        nvc._UseHostAllocator(False)


class _Surf:
    def __init__(self, w, h):
        self.w, self.h = w, h

    def Width(self):
        return self.w

    def Height(self):
        return self.h


class _Resizer:
    """stands in for PySurfaceConvertResizer: a ValueError must come before the resizer is asked to run"""

    def DstSize(self):
        return (16, 8)

    def Stream(self):
        raise AssertionError("validation must come first")

    def ExecuteRoisToTensor(self, *a, **k):
        raise AssertionError("validation must come first")


def test_python_value_errors():
    """rois_to_normalized_tensor: ValueError for rois on a device (the message says .cpu()), a float dtype, a bad index, a rect outside the surface"""
    torch = pytest.importorskip("torch")
    from videoprocessingframework_amd import PytorchNvCodec as pnc

    rs, surfs, mean, std = _Resizer(), [_Surf(64, 32), _Surf(64, 32)], (0, 0, 0), (1, 1, 1)
    bad = [
        [(2, 0, 0, 8, 8)], [(-1, 0, 0, 8, 8)],                       # surface index
        [(0, 60, 0, 8, 8)], [(0, 0, 30, 8, 8)], [(1, -1, 0, 8, 8)],   # outside the surface
        [(0, 0, 0, 0, 8)], [(0, 0, 0, 8, 0)],                         # empty
        [(0, 0, 0, 8)], [(0, 0.5, 0, 8, 8)],                          # not five integers
        torch.tensor([[0, 0, 0, 8, 8]], dtype=torch.float32), torch.tensor([0, 0, 0, 8, 8]), torch.zeros((2, 4), dtype=torch.int64),
        np.array([[0, 0, 0, 8, 8]], dtype=np.float64), np.zeros((1, 6), dtype=np.int32),
        torch.tensor([[0, 0, 0, 8, 8], [0, 57, 0, 8, 8]]),
    ]
    for rois in bad:
        with pytest.raises(ValueError):
            pnc.rois_to_normalized_tensor(rs, surfs, rois, mean, std)
    with pytest.raises(ValueError):
        pnc.rois_to_normalized_tensor(rs, surfs, [(0, 0, 0, 8, 8)], mean, std, dtype=torch.float64)
    with pytest.raises(ValueError, match=r"\.cpu\(\)"):
        pnc.rois_to_normalized_tensor(rs, surfs, torch.empty((1, 5), dtype=torch.int64, device="meta"), mean, std)
    # accepted spellings: lists of tuples, numpy integers, integer tensors / arrays of shape [K, 5]
    want = [(0, 1, 3, 8, 8), (1, 56, 24, 8, 8)]
    for rois in (want, [list(r) for r in want], [tuple(np.int64(v) for v in r) for r in want], torch.tensor(want, dtype=torch.int32), np.array(want, dtype=np.uint16)):
        assert pnc._rois_list(rois, surfs, "t") == want


@pytest.mark.parametrize("sf", ["NV12", "YUV420"])
@pytest.mark.parametrize("W,H,dw,dh", [(64, 48, 32, 24), (37, 91, 64, 128)])
def test_premise_fused_equals_convert_crop_resize(oracle, sf, W, H, dw, dh):
    """oracle.convert_resize == oracle.convert, then oracle.resize, on the whole frame; and a crop at an ODD offset composed the same way equals
    the definition evaluated by hand for a few pixels (taps on the rectangle, chroma at absolute ((x + i) >> 1, (y + j) >> 1))"""
    o = oracle
    src = o.synth(getattr(o, sf), W, H, 4242)
    for cs, cr in ((1, 0), (0, 1)):
        st, fused = o.convert_resize(getattr(o, sf), o.RGB_PLANAR, cs, cr, W, H, src, dw, dh, mode=o.FP32)
        assert st == 0
        assert np.array_equal(np.stack(fused), roi_reference_u8(o, sf, cs, cr, W, H, src, (0, 0, W, H), dw, dh))
        # an odd-offset crop: the composition against a direct evaluation of the definition in numpy fp32
        x, y, w, h = 5, 3, W - 11, H - 8
        got = roi_reference_u8(o, sf, cs, cr, W, H, src, (x, y, w, h), dw, dh)
        st, rgb = o.convert(getattr(o, sf), o.RGB_PLANAR, cs, cr, W, H, src, o.FP32)
        f32 = np.float32

        def tap(d, S, D):
            # fmaf(d + 0.5, scale, -0.5) rounds once: the double evaluation is exact for these small values, so its fp32 rounding is that fma
            s = f32(np.float64(np.float32(d) + f32(0.5)) * np.float64(f32(S) / f32(D)) - 0.5)
            s = min(max(s, f32(0)), f32(S - 1))
            i0 = int(s)
            return i0, min(i0 + 1, S - 1), f32(s - f32(i0))

        for dx, dy in ((0, 0), (dw - 1, dh - 1), (dw // 2, dh // 3), (1, dh - 2), (dw - 2, 1)):
            x0, x1, fx = tap(dx, w, dw)
            y0, y1, fy = tap(dy, h, dh)
            for c in range(3):
                p = rgb[c].astype(np.float64)
                p00, p01, p10, p11 = p[y + y0, x + x0], p[y + y0, x + x1], p[y + y1, x + x0], p[y + y1, x + x1]
                top = f32(np.float64(fx) * (p01 - p00) + p00)
                bot = f32(np.float64(fx) * (p11 - p10) + p10)
                v = f32(f32(np.float64(fy) * np.float64(f32(bot - top)) + np.float64(top)) + f32(0.5))
                assert int(v) == got[c, dy, dx], (sf, cs, cr, dx, dy, c)
