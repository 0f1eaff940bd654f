"""Letterbox into the tensor (vpf_convert_letterbox_tensor, vpf_letterbox_fit, PySurfaceConvertResizer.ExecuteLetterboxToTensor,
PyNvCodec.LetterboxFit, PytorchNvCodec.letterbox_to_normalized_tensor), without a GPU: the symbols and bindings exist, the job structure has the
declared layout, vpf_letterbox_fit equals its definition in exact integers, every validation rule answers before any device work (fake pointers:
nothing here may reach a launch), the Python entries raise ValueError where they say they do, and the premise of
tests/test_gpu_letterbox_tensor.py holds on the oracle — fill, crop and oracle.resize into a sub-window give roi_reference_u8(rect -> (iw, ih))
inside and the pad outside."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from test_roi_tensor_cpu import _Surf, _norm, roi_reference_u8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def letterbox_reference_u8(orc, sf, cs, cr, W, H, src, rect, dst_rect, dw, dh, pad, rgb=None):
    """the definition (include/vpf_hip.h) as a composition: three planes of dw x dh filled with pad[c], then oracle.resize of the cropped converted
    frame INTO the sub-window (views advanced by iy * pitch + ix) -> [3, dh, dw] bytes"""
    if rgb is None:
        st, rgb = orc.convert(getattr(orc, sf), orc.RGB_PLANAR, cs, cr, W, H, src, orc.FP32)
        assert st == 0
    x, y, w, h = rect
    ix, iy, iw, ih = dst_rect
    out = np.empty((3, dh, dw), np.uint8)
    for c in range(3):
        out[c] = pad[c]
    # views: the destination planes advanced by iy * pitch + ix, pitch = the whole plane's
    st, _ = orc.resize(orc.RGB_PLANAR, orc.LINEAR, w, h, [p[y:y + h, x:x + w] for p in rgb], iw, ih, orc.FP32, dst=[out[c, iy:iy + ih, ix:ix + iw] for c in range(3)])
    assert st == 0
    return out


def fit_reference(w, h, dw, dh):
    """vpf_letterbox_fit restated with Python's exact integers"""
    if w * dh >= h * dw:
        iw, ih = dw, min(max((2 * h * dw + w) // (2 * w), 1), dh)
    else:
        ih, iw = dh, min(max((2 * w * dh + h) // (2 * h), 1), dw)
    return ((dw - iw) // 2, (dh - ih) // 2, iw, ih)


def test_symbols_and_bindings_exist(capi):
    for name in ("vpf_convert_letterbox_tensor", "vpf_letterbox_fit"):
        assert name in capi.EXPORTS and hasattr(capi.lib(), name)
    nm = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert " vpf_convert_letterbox_tensor\n" in nm and " vpf_letterbox_fit\n" in nm
    assert callable(capi.make_letterbox_jobs) and callable(capi.convert_letterbox_tensor) and callable(capi.letterbox_fit)
    sys.path.insert(0, os.path.join(ROOT, "videoprocessingframework_amd"))
    nvc = pytest.importorskip("PyNvCodec")
    assert hasattr(nvc.PySurfaceConvertResizer, "ExecuteLetterboxToTensor") and callable(nvc.LetterboxFit)
    assert tuple(nvc.LetterboxFit(1920, 1080, 640, 640)) == (0, 140, 640, 360)
    stub = open(os.path.join(ROOT, "videoprocessingframework_amd", "PyNvCodec", "__init__.pyi")).read()
    assert "def ExecuteLetterboxToTensor(" in stub and "def LetterboxFit(" in stub
    src = open(os.path.join(ROOT, "videoprocessingframework_amd", "PytorchNvCodec", "__init__.py")).read()
    assert "def letterbox_to_normalized_tensor(resizer, surfaces, mean, std, rois=None, dst_rects=None, pad=(114, 114, 114), dtype=torch.float32, bgr=False, out=None," in src
    h = open(os.path.join(ROOT, "include", "vpf_hip.h")).read()
    for decl in ("typedef struct vpf_letterbox_io", "typedef struct vpf_letterbox_opts", "VPF_API vpf_status vpf_convert_letterbox_tensor(",
                 "VPF_API vpf_rect vpf_letterbox_fit("):
        assert h.index(decl) > h.index("VPF_API vpf_status vpf_convert_resize_tensor_rois("), decl


def test_struct_layout(capi):
    """vpf_letterbox_io is 128 bytes with no implicit padding: 6 planes of 16 B, then the two rectangles; vpf_letterbox_opts is 4 bytes"""
    C = capi.C
    assert C.sizeof(capi.LetterboxIO) == 128
    io = capi.LetterboxIO
    assert (io.src.offset, io.dst.offset, io.rect.offset, io.dst_rect.offset) == (0, 48, 96, 112)
    assert sum(C.sizeof(t) for _, t in io._fields_) == 128
    assert C.sizeof(capi.LetterboxOpts) == 4 and (capi.LetterboxOpts.pad.offset, capi.LetterboxOpts.reserved.offset) == (0, 3)


def test_letterbox_fit(capi):
    assert capi.letterbox_fit(1920, 1080, 640, 640) == (0, 140, 640, 360)
    assert capi.letterbox_fit(1080, 1920, 640, 640) == (140, 0, 360, 640)
    assert capi.letterbox_fit(1920, 1080, 640, 360) == (0, 0, 640, 360)      # equal aspect: the whole destination
    assert capi.letterbox_fit(55, 41, 110, 82) == (0, 0, 110, 82)
    assert capi.letterbox_fit(65536, 1, 2, 2) == (0, 0, 2, 1)                # ih = round(2 / 65536) = 0, clamped to 1
    assert capi.letterbox_fit(1, 65536, 2, 2) == (0, 0, 1, 2)
    assert capi.letterbox_fit(65536, 65536, 65536, 65535) == fit_reference(65536, 65536, 65536, 65535) == (0, 0, 65535, 65535)  # 2^33 products
    assert capi.letterbox_fit(65536, 65535, 65535, 65536) == fit_reference(65536, 65535, 65535, 65536)
    rng = np.random.default_rng(77)
    for k in range(2000):
        hi = 65537 if k % 4 == 0 else 2049
        w, h, dw, dh = (int(v) for v in rng.integers(1, hi, 4))
        got = capi.letterbox_fit(w, h, dw, dh)
        assert got == fit_reference(w, h, dw, dh), (w, h, dw, dh)
        ix, iy, iw, ih = got
        assert iw >= 1 and ih >= 1 and ix + iw <= dw and iy + ih <= dh and (iw == dw or ih == dh), (w, h, dw, dh, got)
        assert ix == (dw - iw) // 2 and iy == (dh - ih) // 2


def test_validation_without_gpu(capi):
    """every row of the validation table, before any device work: the plane pointers below are fake"""
    ex = capi.make_exec()
    W, H, dw, dh = 64, 32, 16, 8
    src = [(0x100000, 64), (0x200000, 64)]
    f32 = [(0x400000, 64), (0x500000, 64), (0x600000, 64)]  # dw * 4 = 64
    f16 = [(0x400000, 32), (0x500000, 32), (0x600000, 32)]
    rect, drect = (3, 5, 20, 10), (2, 1, 9, 5)

    def call(dst=f32, norm=None, sf=capi.NV12, cs=1, cr=0, s=src, size=(W, H, dw, dh), r=rect, d=drect, jobs=None, opts=None):
        jobs = capi.make_letterbox_jobs([(s, dst, r, d)] if jobs is None else jobs)
        return capi.convert_letterbox_tensor(ex, sf, cs, cr, size[0], size[1], size[2], size[3], jobs, _norm(capi) if norm is None else norm, opts, check=False)

    # the new refusals: an empty dst_rect, a dst_rect that leaves dst_size (32-bit wrap-around included), a non-zero reserved
    for d in ((2, 1, 0, 5), (2, 1, 9, 0), (0, 0, 0, 0)):
        assert call(d=d) == capi.ERR_BAD_ARG, d
    for d in ((8, 1, 9, 5), (2, 4, 9, 5), (16, 0, 1, 1), (0, 8, 1, 1), (0, 0, 17, 8), (0, 0, 16, 9), (0xFFFFFFFF, 0, 2, 2), (0, 0xFFFFFFF0, 2, 0x20),
              (2, 0, 0xFFFFFFFF, 1)):
        assert call(d=d) == capi.ERR_BAD_ARG, d
    bad_opts = capi.make_letterbox_opts((1, 2, 3))
    bad_opts.reserved = 1
    assert call(opts=bad_opts) == capi.ERR_BAD_ARG
    # unsupported format, matrix, dtype or flag: the rules of vpf_convert_resize_tensor_rois
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
    good = capi.make_letterbox_jobs([(src, f32, rect, drect)] * 3)
    args = (capi.NV12, 1, 0, capi.Size(W, H), capi.Size(dw, dh), 3)
    assert L.vpf_convert_letterbox_tensor(None, *args, good, Cb(_norm(capi)), None) == capi.ERR_BAD_ARG
    assert L.vpf_convert_letterbox_tensor(Cb(ex), *args, None, Cb(_norm(capi)), None) == capi.ERR_BAD_ARG
    assert L.vpf_convert_letterbox_tensor(Cb(ex), *args, good, None, None) == capi.ERR_BAD_ARG
    assert call(s=[(0, 64), (0x200000, 64)]) == capi.ERR_BAD_ARG
    assert call(s=src[:1]) == capi.ERR_BAD_ARG
    assert call(dst=f32[:2]) == capi.ERR_BAD_ARG
    # n == 0
    assert capi.convert_letterbox_tensor(ex, capi.NV12, 1, 0, W, H, dw, dh, good, _norm(capi), n=0, check=False) == capi.ERR_BAD_ARG
    # bad sizes; an empty rect; a rect outside the frame
    for size in ((0, H, dw, dh), (W, 0, dw, dh), (W, H, 0, dh), (W, H, dw, 0), (70000, H, dw, dh), (W, H, 70000, dh)):
        assert call(size=size) == capi.ERR_BAD_ARG, size
    for r in ((3, 5, 0, 10), (3, 5, 20, 0), (45, 5, 20, 10), (3, 23, 20, 10), (0xFFFFFFFF, 0, 2, 2)):
        assert call(r=r) == capi.ERR_BAD_ARG, r
    # short pitches, misaligned planes (the pitch covers the WHOLE dst_size row, whatever dst_rect is), non-finite parameters
    assert call(s=[(0x100000, 63), (0x200000, 64)]) == capi.ERR_BAD_ARG
    for dt, planes, elem in ((capi.TENSOR_F32, f32, 4), (capi.TENSOR_F16, f16, 2)):
        for k in range(3):
            p = list(planes)
            p[k] = (planes[k][0] + 1, planes[k][1])
            assert call(dst=p, norm=_norm(capi, dtype=dt)) == capi.ERR_BAD_ARG, (dt, k, "pointer")
            p[k] = (planes[k][0], dw * elem - elem)
            assert call(dst=p, norm=_norm(capi, dtype=dt)) == capi.ERR_BAD_ARG, (dt, k, "short pitch")
    nhwc = _norm(capi, flags=capi.TENSOR_NHWC)
    assert call(dst=[(0x400000, 3 * dw * 4 - 4), (0, 0), (0, 0)], norm=nhwc) == capi.ERR_BAD_ARG
    for bad in (math.nan, math.inf):
        sc = [0.01, bad, 0.01]
        assert call(norm=_norm(capi, scale=sc)) == capi.ERR_BAD_ARG
        assert call(norm=_norm(capi, bias=sc)) == capi.ERR_BAD_ARG
    # one bad job among good ones, beyond the first two job tables: everything is validated before the first launch
    jobs = [(src, f32, rect, drect)] * 200 + [(src, f32, rect, (8, 1, 9, 5))]
    assert call(jobs=jobs) == capi.ERR_BAD_ARG
    with pytest.raises(capi.VpfError):
        capi.convert_letterbox_tensor(ex, capi.NV12, 1, 0, W, H, dw, dh, capi.make_letterbox_jobs([(src, f32, rect, (8, 1, 9, 5))]), _norm(capi))


def test_binding_validation_without_gpu():
    """PySurfaceConvertResizer.ExecuteLetterboxToTensor: ValueError for a bad mean / std, a bad pad and rois / dst_rects of different lengths; False
    for a wrong surface or a bad rectangle on either side — all before any device work (host-memory surfaces, a fake destination address)"""
    sys.path.insert(0, os.path.join(ROOT, "videoprocessingframework_amd"))
    nvc = pytest.importorskip("PyNvCodec")
    nvc._UseHostAllocator(True)
    try:
        PF = nvc.PixelFormat
        r = nvc.PySurfaceConvertResizer(64, 32, PF.NV12, 16, 8, PF.RGB_PLANAR, 0, 0)
        good = nvc.Surface.Make(PF.NV12, 64, 32, context=0)
        fake, mean, std = 0x400000, [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
        roi, drect = [(0, 0, 0, 8, 8)], [(2, 1, 9, 5)]
        with pytest.raises(ValueError):
            r.ExecuteLetterboxToTensor([good], roi, drect, fake, 0, [0, 0, 0], [1, 0, 1])
        for pad in ([0, 0, 256], [-1, 0, 0], [1, 2], [1, 2, 3, 4]):
            with pytest.raises(ValueError):
                r.ExecuteLetterboxToTensor([good], roi, drect, fake, 0, mean, std, pad=pad)
        with pytest.raises(ValueError):
            r.ExecuteLetterboxToTensor([good], roi * 2, drect, fake, 0, mean, std)
        with pytest.raises(ValueError):
            r.ExecuteLetterboxToTensor([good], roi, [], fake, 0, mean, std)
        assert not r.ExecuteLetterboxToTensor([good], [], [], fake, 0, mean, std)
        assert not r.ExecuteLetterboxToTensor([], roi, drect, fake, 0, mean, std)
        assert not r.ExecuteLetterboxToTensor([good], [(1, 0, 0, 8, 8)], drect, fake, 0, mean, std)      # no such surface
        assert not r.ExecuteLetterboxToTensor([good], [(0, 60, 0, 8, 8)], drect, fake, 0, mean, std)     # leaves the surface
        assert not r.ExecuteLetterboxToTensor([good], roi, [(8, 1, 9, 5)], fake, 0, mean, std)           # leaves the destination
        assert not r.ExecuteLetterboxToTensor([good], roi, [(2, 1, 0, 5)], fake, 0, mean, std)           # empty
        assert not r.ExecuteLetterboxToTensor([good], roi, [(-1, 1, 4, 5)], fake, 0, mean, std)          # negative
        assert not r.ExecuteLetterboxToTensor([nvc.Surface.Make(PF.NV12, 32, 32, context=0)], roi, drect, fake, 0, mean, std)   # wrong size
        assert not r.ExecuteLetterboxToTensor([good], roi, drect, fake, 3, mean, std)                    # unknown dtype
        assert not r.ExecuteLetterboxToTensor([good], roi, drect, fake, 0, mean, std, row_stride=60)     # below 16 x 4 bytes
    finally:
        nvc._UseHostAllocator(False)


class _Resizer:
    """stands in for PySurfaceConvertResizer: a ValueError must come before the resizer is asked to run"""

    def DstSize(self):
        return (16, 8)

    def Stream(self):
        raise AssertionError("validation must come first")

    def ExecuteLetterboxToTensor(self, *a, **k):
        raise AssertionError("validation must come first")


def test_python_value_errors():
    """letterbox_to_normalized_tensor: ValueError for a bad pad, rois / dst_rects of different lengths, a dst_rect that is empty or leaves the
    destination, and what rois_to_normalized_tensor refuses"""
    torch = pytest.importorskip("torch")
    sys.path.insert(0, os.path.join(ROOT, "videoprocessingframework_amd"))
    pytest.importorskip("PyNvCodec")
    from videoprocessingframework_amd import PytorchNvCodec as pnc

    rs, surfs, mean, std = _Resizer(), [_Surf(64, 32), _Surf(64, 32)], (0, 0, 0), (1, 1, 1)
    rois = [(0, 0, 0, 8, 8), (1, 3, 5, 20, 10)]
    for pad in ((0, 0, 256), (-1, 0, 0), (1, 2), (1, 2, 3, 4), (1.5, 0, 0), None):
        with pytest.raises(ValueError):
            pnc.letterbox_to_normalized_tensor(rs, surfs, mean, std, rois=rois, pad=pad) if pad is not None else \
                pnc.letterbox_to_normalized_tensor(rs, surfs, mean, std, rois=rois, pad="abc")
    for dst_rects in ([(0, 0, 16, 8)], [(0, 0, 16, 8)] * 3,                                        # another length than rois
                      [(0, 0, 16, 8), (8, 0, 9, 8)], [(0, 0, 16, 8), (0, 4, 4, 5)],                  # leaves the destination
                      [(0, 0, 0, 8), (0, 0, 16, 8)], [(0, 0, 16, 8), (-1, 0, 4, 4)],                 # empty, negative
                      [(0, 0, 16), (0, 0, 16, 8)], [(0, 0.5, 16, 8), (0, 0, 16, 8)],                 # not four integers
                      torch.tensor([[0, 0, 16, 8], [0, 0, 16, 8]], dtype=torch.float32), np.array([[0, 0, 16, 8], [0, 0, 16, 8]], dtype=np.float64),
                      torch.empty((2, 4), dtype=torch.int64, device="meta")):
        with pytest.raises(ValueError):
            pnc.letterbox_to_normalized_tensor(rs, surfs, mean, std, rois=rois, dst_rects=dst_rects)
    with pytest.raises(ValueError):
        pnc.letterbox_to_normalized_tensor(rs, surfs, mean, std, rois=[(2, 0, 0, 8, 8)])
    with pytest.raises(ValueError):
        pnc.letterbox_to_normalized_tensor(rs, surfs, mean, std, rois=[(0, 60, 0, 8, 8)])
    with pytest.raises(ValueError):
        pnc.letterbox_to_normalized_tensor(rs, surfs, mean, std, dtype=torch.float64)
    want = [(0, 0, 16, 8), (3, 1, 9, 5)]
    for spelling in (want, [list(r) for r in want], torch.tensor(want, dtype=torch.int32), np.array(want, dtype=np.uint16)):
        assert pnc._dst_rects_list(spelling, 2, 16, 8, "t") == want


@pytest.mark.parametrize("sf", ["NV12", "YUV420"])
@pytest.mark.parametrize("W,H,dw,dh,rect,drect", [(64, 48, 40, 40, (0, 0, 64, 48), (0, 5, 40, 30)), (37, 91, 64, 70, (5, 3, 26, 83), (21, 1, 22, 69))])
def test_premise_composition_on_the_oracle(oracle, sf, W, H, dw, dh, rect, drect):
    """fill + crop + oracle.resize INTO a sub-window (the composition the header states) == roi_reference_u8(rect -> (iw, ih)) inside and the pad
    outside: a resize that writes through plane views advanced by iy * pitch + ix touches the sub-window and nothing else"""
    o = oracle
    src = o.synth(getattr(o, sf), W, H, 4243)
    pad = (114, 7, 250)
    ix, iy, iw, ih = drect
    got = letterbox_reference_u8(o, sf, 1, 0, W, H, src, rect, drect, dw, dh, pad)
    inner = roi_reference_u8(o, sf, 1, 0, W, H, src, rect, iw, ih)
    assert np.array_equal(got[:, iy:iy + ih, ix:ix + iw], inner)
    outside = np.ones((dh, dw), bool)
    outside[iy:iy + ih, ix:ix + iw] = False
    for c in range(3):
        assert (got[c][outside] == pad[c]).all()
