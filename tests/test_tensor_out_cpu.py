"""The normalised planar-tensor output of the fused path (vpf_convert_resize_tensor, PySurfaceConvertResizer.ExecuteToTensor,
PytorchNvCodec.to_normalized_tensor), without a GPU: the symbols and bindings exist, every validation rule answers before any device work
(fake pointers: nothing here may reach a launch), mean / std map to scale / bias as torchvision's convention says, and the exactness premise
of tests/test_gpu_tensor_out.py holds for every parameter set it uses.

Output definition (include/vpf_hip.h): out[c] = round_to_dtype(fmaf(u8[c], scale[c], bias[c])), u8 = the RGB_PLANAR byte of
vpf_convert_resize, scale = 1 / (255 std), bias = -mean / std computed in double and rounded to fp32."""
import math
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (name, mean, std): every parameter set the GPU test uses
PARAM_SETS = [
    ("imagenet", (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)),
    ("unit", (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)),            # [0, 1]
    ("symmetric", (0.5, 0.5, 0.5), (0.5, 0.5, 0.5)),       # [-1, 1]
]


def scale_bias_f32(mean, std):
    """the definition: both in double, then rounded to fp32"""
    return (np.array([1.0 / (255.0 * s) for s in std], dtype=np.float32), np.array([-m / s for m, s in zip(mean, std)], dtype=np.float32))


def test_symbols_and_bindings_exist(capi):
    for name in ("vpf_convert_resize_tensor", "vpf_convert_resize_tensor_batch"):
        assert name in capi.EXPORTS
        assert hasattr(capi.lib(), name)
    nm = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert " vpf_convert_resize_tensor\n" in nm and " vpf_convert_resize_tensor_batch\n" in nm
    assert (capi.TENSOR_F32, capi.TENSOR_F16, capi.TENSOR_BF16, capi.TENSOR_BGR) == (0, 1, 2, 1)
    assert capi.C.sizeof(capi.TensorNorm) == 32
    sys.path.insert(0, os.path.join(ROOT, "videoprocessingframework_amd"))
    nvc = pytest.importorskip("PyNvCodec")
    for m in ("ExecuteToTensor", "Stream", "DstSize"):
        assert hasattr(nvc.PySurfaceConvertResizer, m), m
    stub = open(os.path.join(ROOT, "videoprocessingframework_amd", "PyNvCodec", "__init__.pyi")).read()
    assert "def ExecuteToTensor(" in stub and "def Stream(" in stub and "def DstSize(" in stub
    src = open(os.path.join(ROOT, "videoprocessingframework_amd", "PytorchNvCodec", "__init__.py")).read()
    assert "def to_normalized_tensor(resizer, surfaces, mean, std, dtype=torch.float32, bgr=False, out=None, cc_ctx=None)" in src


def test_header_declarations_follow_the_u8_batch_entry():
    h = open(os.path.join(ROOT, "include", "vpf_hip.h")).read()
    i = h.index("VPF_API vpf_status vpf_convert_resize_batch(")
    for decl in ("typedef enum vpf_tensor_dtype", "typedef struct vpf_tensor_norm", "VPF_API vpf_status vpf_convert_resize_tensor(",
                 "VPF_API vpf_status vpf_convert_resize_tensor_batch("):
        assert h.index(decl) > i, decl


def _norm(capi, dtype=0, flags=0, scale=(0.01, 0.01, 0.01), bias=(-1.0, -1.0, -1.0)):
    n = capi.TensorNorm()
    for c in range(3):
        n.scale[c], n.bias[c] = scale[c], bias[c]
    n.dtype, n.flags = dtype, flags
    return n


def test_validation_without_gpu(capi):
    """every refusal happens before any device work: the plane pointers below are fake"""
    ex = capi.make_exec()
    sw, sh, dw, dh = 64, 32, 16, 8
    src = [(0x100000, 64), (0x200000, 64)]
    yuv = [(0x100000, 64), (0x200000, 32), (0x300000, 32)]

    def call(dst, norm, sf=capi.NV12, cs=1, cr=0, s=src, size=(sw, sh, dw, dh)):
        return capi.convert_resize_tensor(ex, sf, cs, cr, size[0], size[1], s, size[2], size[3], dst, norm, check=False)

    f32 = [(0x400000, 64), (0x500000, 64), (0x600000, 64)]  # dw * 4 = 64
    f16 = [(0x400000, 32), (0x500000, 32), (0x600000, 32)]
    # sources, colour models: what vpf_convert_resize refuses as unsupported
    assert call(f32, _norm(capi), sf=capi.RGB) == capi.ERR_UNSUPPORTED
    assert call(f32, _norm(capi), sf=capi.YUV444) == capi.ERR_UNSUPPORTED
    assert call(f32, _norm(capi), cs=2) == capi.ERR_UNSUPPORTED
    assert call(f32, _norm(capi), cr=2) == capi.ERR_UNSUPPORTED
    # an unknown dtype or flag bit
    assert call(f32, _norm(capi, dtype=3)) == capi.ERR_UNSUPPORTED
    assert call(f32, _norm(capi, dtype=0xFFFFFFFF)) == capi.ERR_UNSUPPORTED
    assert call(f32, _norm(capi, flags=2)) == capi.ERR_UNSUPPORTED
    assert call(f32, _norm(capi, flags=capi.TENSOR_BGR | 0x80000000)) == capi.ERR_UNSUPPORTED
    # a non-finite scale or bias
    for bad in (math.nan, math.inf, -math.inf):
        for c in range(3):
            sc, bi = [0.01] * 3, [-1.0] * 3
            sc[c] = bad
            assert call(f32, _norm(capi, scale=sc)) == capi.ERR_BAD_ARG
            sc[c], bi[c] = 0.01, bad
            assert call(f32, _norm(capi, bias=bi)) == capi.ERR_BAD_ARG
    # no parameters at all
    assert capi.lib().vpf_convert_resize_tensor(capi.C.byref(ex), capi.NV12, 1, 0, capi.Size(sw, sh), capi.planes(src), capi.Size(dw, dh),
                                                capi.planes(f32), None) == capi.ERR_BAD_ARG
    # plane pointers / pitches that are not multiples of the element size, pitches below dw * elem, missing planes
    for dt, planes, elem in ((capi.TENSOR_F32, f32, 4), (capi.TENSOR_F16, f16, 2), (capi.TENSOR_BF16, f16, 2)):
        for k in range(3):
            p = list(planes)
            p[k] = (planes[k][0] + 1, planes[k][1])
            assert call(p, _norm(capi, dtype=dt)) == capi.ERR_BAD_ARG, (dt, k, "pointer")
            p[k] = (planes[k][0], planes[k][1] + 1)
            assert call(p, _norm(capi, dtype=dt)) == capi.ERR_BAD_ARG, (dt, k, "pitch")
            p[k] = (planes[k][0], dw * elem - elem)
            assert call(p, _norm(capi, dtype=dt)) == capi.ERR_BAD_ARG, (dt, k, "short pitch")
            p[k] = (0, planes[k][1])
            assert call(p, _norm(capi, dtype=dt)) == capi.ERR_BAD_ARG, (dt, k, "null")
        if elem == 4:
            odd = [(a + 2, b) for a, b in planes]
            assert call(odd, _norm(capi, dtype=dt)) == capi.ERR_BAD_ARG
    assert call(f32[:2], _norm(capi)) == capi.ERR_BAD_ARG  # the third plane is missing
    # what vpf_convert_resize already refuses: sizes, source planes
    assert call(f32, _norm(capi), size=(0, sh, dw, dh)) == capi.ERR_BAD_ARG
    assert call(f32, _norm(capi), size=(sw, sh, 0, dh)) == capi.ERR_BAD_ARG
    assert call(f32, _norm(capi), size=(sw, sh, 70000, dh)) == capi.ERR_BAD_ARG
    assert call(f32, _norm(capi), s=[(0x100000, 63), (0x200000, 64)]) == capi.ERR_BAD_ARG
    assert call(f32, _norm(capi), s=[(0, 64), (0x200000, 64)]) == capi.ERR_BAD_ARG
    assert call(f32, _norm(capi), sf=capi.YUV420, s=[(0x100000, 64), (0x200000, 31), (0x300000, 32)]) == capi.ERR_BAD_ARG
    assert call(f32, _norm(capi), sf=capi.YUV420, s=yuv[:2]) == capi.ERR_BAD_ARG
    # the batch entry: n = 0, no frames, and one bad frame among good ones
    good = capi.make_batch([(src, f32)] * 3)
    assert capi.convert_resize_tensor_batch(ex, capi.NV12, 1, 0, sw, sh, dw, dh, good, _norm(capi), n=0, check=False) == capi.ERR_BAD_ARG
    assert capi.lib().vpf_convert_resize_tensor_batch(capi.C.byref(ex), capi.NV12, 1, 0, capi.Size(sw, sh), capi.Size(dw, dh), 3, None,
                                                      capi.C.byref(_norm(capi))) == capi.ERR_BAD_ARG
    mixed = capi.make_batch([(src, f32), (src, f32), (src, [(0x400000, 64), (0x500002, 64), (0x600000, 64)])])
    assert capi.convert_resize_tensor_batch(ex, capi.NV12, 1, 0, sw, sh, dw, dh, mixed, _norm(capi), check=False) == capi.ERR_BAD_ARG
    assert capi.convert_resize_tensor_batch(ex, capi.NV12, 1, 0, sw, sh, dw, dh, good, _norm(capi, dtype=7), check=False) == capi.ERR_UNSUPPORTED
    with pytest.raises(capi.VpfError):
        capi.convert_resize_tensor(ex, capi.NV12, 1, 0, sw, sh, src, dw, dh, f32, _norm(capi, dtype=3))


def test_mean_std_to_scale_bias(capi):
    """scale = 1 / (255 std), bias = -mean / std, in double, then fp32: [0, 1] for mean 0 / std 1, [-1, 1] for mean 0.5 / std 0.5"""
    for name, mean, std in PARAM_SETS:
        scale, bias = scale_bias_f32(mean, std)
        n = capi.make_tensor_norm(mean, std, dtype=capi.TENSOR_BF16, bgr=True)
        assert (n.dtype, n.flags) == (capi.TENSOR_BF16, capi.TENSOR_BGR)
        for c in range(3):
            assert np.float32(n.scale[c]) == scale[c] and np.float32(n.bias[c]) == bias[c], (name, c)
            # the fp32 values are the double values rounded once: within half an fp32 ulp of the exact quotient of the (double) inputs
            exact = Fraction(1) / (255 * Fraction(std[c]))
            assert abs(Fraction(float(scale[c])) - exact) <= Fraction(float(np.spacing(scale[c]))) / 2, (name, c)
    s, b = scale_bias_f32((0.0,) * 3, (1.0,) * 3)
    assert (s == np.float32(1 / 255)).all() and (b == 0).all()
    s, b = scale_bias_f32((0.5,) * 3, (0.5,) * 3)
    assert (s == np.float32(2 / 255)).all() and (b == -1).all()
    assert float(np.float32(0) * s[0] + b[0]) == -1.0 and abs(float(np.float32(255) * s[0] + b[0]) - 1.0) < 1e-6
    for bad_mean, bad_std in (((0, 0, 0), (1, 0, 1)), ((0, 0, 0), (1, -1, 1)), ((0, math.nan, 0), (1, 1, 1)), ((0, 0, 0), (1, math.inf, 1)),
                              ((0, 0), (1, 1))):
        with pytest.raises(ValueError):
            capi.norm_params(bad_mean, bad_std)


@pytest.mark.parametrize("name,mean,std", PARAM_SETS)
def test_exactness_premise(name, mean, std):
    """tests/test_gpu_tensor_out.py computes ref32 = float32(float64(u8) * float64(scale_f32) + float64(bias_f32)).  That is fmaf(u8, scale,
    bias) only if both float64 operations are exact: checked with fractions over all 256 codes and the three channels."""
    scale, bias = scale_bias_f32(mean, std)
    for c in range(3):
        s64, b64 = np.float64(scale[c]), np.float64(bias[c])
        fs, fb = Fraction(float(s64)), Fraction(float(b64))
        for u in range(256):
            prod = np.float64(u) * s64
            assert Fraction(float(prod)) == u * fs, (name, c, u, "product")
            r64 = prod + b64
            assert Fraction(float(r64)) == u * fs + fb, (name, c, u, "sum")


def test_binding_validation_without_gpu():
    """PySurfaceConvertResizer.ExecuteToTensor: ValueError for std <= 0 or a non-finite mean / std, False for a wrong size or format —
    all before any device work (host-memory surfaces, a fake destination address)"""
    sys.path.insert(0, os.path.join(ROOT, "videoprocessingframework_amd"))
    nvc = pytest.importorskip("PyNvCodec")
    nvc._UseHostAllocator(True)
    try:
        PF = nvc.PixelFormat
        r = nvc.PySurfaceConvertResizer(64, 32, PF.NV12, 16, 8, PF.RGB_PLANAR, 0, 0)
        assert tuple(r.DstSize()) == (16, 8)
        assert isinstance(r.Stream(), int)
        good = nvc.Surface.Make(PF.NV12, 64, 32, context=0)
        fake = 0x400000
        im_mean, im_std = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
        for m, s in (([0, 0, 0], [1, 0, 1]), ([0, 0, 0], [1, -0.5, 1]), ([math.nan, 0, 0], [1, 1, 1]), ([0, 0, 0], [1, 1, math.inf]),
                     ([0, math.inf, 0], [1, 1, 1]), ([0, 0], [1, 1, 1]), ([0, 0, 0], [1e-45, 1, 1])):
            with pytest.raises(ValueError):
                r.ExecuteToTensor([good], fake, 0, m, s)
        assert not r.ExecuteToTensor([nvc.Surface.Make(PF.NV12, 32, 32, context=0)], fake, 0, im_mean, im_std)   # wrong size
        assert not r.ExecuteToTensor([nvc.Surface.Make(PF.YUV420, 64, 32, context=0)], fake, 0, im_mean, im_std)  # wrong format
        assert not r.ExecuteToTensor([good, nvc.Surface.Make(PF.NV12, 64, 16, context=0)], fake, 1, im_mean, im_std)
        assert not r.ExecuteToTensor([], fake, 0, im_mean, im_std)
        assert not r.ExecuteToTensor([good], fake, 3, im_mean, im_std)                   # unknown dtype: the library refuses it
        assert not r.ExecuteToTensor([good], fake, 0, im_mean, im_std, row_pitch=66)     # not a multiple of 4
        assert not r.ExecuteToTensor([good], fake + 2, 1, im_mean, im_std, row_pitch=34)  # f16 planes at an odd address
        assert not r.ExecuteToTensor([good], fake, 0, im_mean, im_std, row_pitch=60)     # below 16 x 4 bytes
        # the colour-context rules of the u8 path: NV12 BT.601 + MPEG needs the extended colour spaces
        nvc.SetExtendedColorspaces(False)
        cc = nvc.ColorspaceConversionContext(nvc.ColorSpace.BT_601, nvc.ColorRange.MPEG)
        assert not r.ExecuteToTensor([good], fake, 0, im_mean, im_std, cc_ctx=cc, row_pitch=66)
    finally:
        nvc._UseHostAllocator(False)
