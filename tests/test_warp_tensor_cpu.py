"""The fused multi-ROI affine warp into a normalised tensor (vpf_convert_warp_tensor), without a GPU: the symbols and bindings exist, the structs
have the documented sizes, every validation rule answers before any device work (fake pointers: nothing here may reach a launch), and the
premise of tests/test_gpu_warp_tensor.py holds — the ground truth of a warp is composed from the oracle's conversion of the whole frame and its
remap of packed RGB on float32 maps written exactly as the definition, into a destination pre-filled with the border."""
import math
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def warp_maps(m, dw, dh, W, H, mode):
    """the definition's sx, sy as float32 arrays [dh, dw]: every operation separately rounded, in the definition's order"""
    m = np.asarray(m, dtype=F32).reshape(6)
    dx, dy = np.arange(dw, dtype=F32)[None, :], np.arange(dh, dtype=F32)[:, None]
    sx = ((m[0] * dx + m[1] * dy) + m[2]).astype(F32)
    sy = ((m[3] * dx + m[4] * dy) + m[5]).astype(F32)
    assert sx.dtype == F32 and sy.dtype == F32
    if mode == 1:  # REPLICATE: a max, then a min
        sx, sy = np.minimum(np.maximum(sx, F32(0)), F32(W - 1)), np.minimum(np.maximum(sy, F32(0)), F32(H - 1))
    return np.ascontiguousarray(sx), np.ascontiguousarray(sy)


def warp_reference_u8(orc, sf, cs, cr, W, H, m, dw, dh, border, mode, rgb=None, src=None):
    """the definition (include/vpf_hip.h): oracle.convert(frame -> RGB_PLANAR, FP32), planes interleaved in numpy, float32 maps, oracle.remap(RGB,
    FP32) into a destination pre-filled with `border` -> [3, dh, dw] bytes.  `rgb`: the converted frame when the caller already has it."""
    if rgb is None:
        st, rgb = orc.convert(getattr(orc, sf), orc.RGB_PLANAR, cs, cr, W, H, src, orc.FP32)
        assert st == 0
    packed = np.ascontiguousarray(np.stack(rgb, axis=-1).reshape(H, 3 * W))
    sx, sy = warp_maps(m, dw, dh, W, H, mode)
    dst = np.ascontiguousarray(np.broadcast_to(np.asarray(border, np.uint8), (dh, dw, 3)).reshape(dh, 3 * dw))
    st, out = orc.remap(orc.RGB, W, H, [packed], sx, sy, orc.FP32, dst=[dst])
    assert st == 0
    return np.ascontiguousarray(out[0].reshape(dh, dw, 3).transpose(2, 0, 1))


def test_symbols_and_bindings_exist(capi):
    assert "vpf_convert_warp_tensor" in capi.EXPORTS
    assert hasattr(capi.lib(), "vpf_convert_warp_tensor")
    nm = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert " vpf_convert_warp_tensor\n" in nm
    assert callable(capi.make_warps) and callable(capi.convert_warp_tensor)
    assert (capi.WARP_CONSTANT, capi.WARP_REPLICATE) == (0, 1)
    h = open(os.path.join(ROOT, "include", "vpf_hip.h")).read()
    for decl in ("#define VPF_WARP_CONSTANT 0u", "#define VPF_WARP_REPLICATE 1u", "typedef struct vpf_warp_io", "typedef struct vpf_warp_opts",
                 "VPF_API vpf_status vpf_convert_warp_tensor("):
        assert h.index(decl) > h.index("VPF_API vpf_status vpf_convert_resize_tensor_rois("), decl


def test_struct_layout(capi):
    """vpf_warp_io is 120 bytes with no implicit padding (6 planes of 16 B, six floats); vpf_warp_opts is 8"""
    C = capi.C
    assert C.sizeof(capi.WarpIO) == 120 and C.sizeof(capi.WarpOpts) == 8
    assert (capi.WarpIO.src.offset, capi.WarpIO.dst.offset, capi.WarpIO.m.offset) == (0, 48, 96)
    assert sum(C.sizeof(t) for _, t in capi.WarpIO._fields_) == 120
    assert (capi.WarpOpts.border_mode.offset, capi.WarpOpts.border.offset, capi.WarpOpts.reserved.offset) == (0, 4, 7)


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
    ident = (1.0, 0.0, 3.0, 0.0, 1.0, 5.0)
    _none = object()

    def call(dst=f32, norm=None, sf=capi.NV12, cs=1, cr=0, s=src, size=(W, H, dw, dh), m=ident, jobs=None, opts=_none):
        jobs = capi.make_warps([(s, dst, m)] if jobs is None else jobs)
        return capi.convert_warp_tensor(ex, sf, cs, cr, size[0], size[1], size[2], size[3], jobs, _norm(capi) if norm is None else norm,
                                        capi.make_warp_opts() if opts is _none else opts, check=False)

    # unsupported format, matrix, dtype or flag: the rules of vpf_convert_resize_tensor; an unknown border mode
    assert call(sf=capi.RGB) == capi.ERR_UNSUPPORTED
    assert call(sf=capi.YUV444) == capi.ERR_UNSUPPORTED
    assert call(cs=2) == capi.ERR_UNSUPPORTED
    assert call(cr=2) == capi.ERR_UNSUPPORTED
    assert call(norm=_norm(capi, dtype=3)) == capi.ERR_UNSUPPORTED
    assert call(norm=_norm(capi, dtype=0xFFFFFFFF)) == capi.ERR_UNSUPPORTED
    assert call(norm=_norm(capi, flags=2)) == capi.ERR_UNSUPPORTED
    assert call(norm=_norm(capi, flags=capi.TENSOR_BGR | 0x80000000)) == capi.ERR_UNSUPPORTED
    assert call(opts=capi.make_warp_opts(2)) == capi.ERR_UNSUPPORTED
    assert call(opts=capi.make_warp_opts(0xFFFFFFFF)) == capi.ERR_UNSUPPORTED
    # a non-zero reserved field
    o = capi.make_warp_opts(capi.WARP_REPLICATE, (1, 2, 3))
    o.reserved = 1
    assert call(opts=o) == capi.ERR_BAD_ARG
    j = capi.make_warps([(src, f32, ident)])
    j[0].dst[1].reserved = 7
    assert capi.convert_warp_tensor(ex, capi.NV12, 1, 0, W, H, dw, dh, j, _norm(capi), check=False) == capi.ERR_BAD_ARG
    # null pointers: exec, the job array, the parameters, a plane
    L, Cb = capi.lib(), capi.C.byref
    good = capi.make_warps([(src, f32, ident)] * 3)
    assert L.vpf_convert_warp_tensor(None, capi.NV12, 1, 0, capi.Size(W, H), capi.Size(dw, dh), 3, good, Cb(_norm(capi)), None) == capi.ERR_BAD_ARG
    assert L.vpf_convert_warp_tensor(Cb(ex), capi.NV12, 1, 0, capi.Size(W, H), capi.Size(dw, dh), 3, None, Cb(_norm(capi)), None) == capi.ERR_BAD_ARG
    assert L.vpf_convert_warp_tensor(Cb(ex), capi.NV12, 1, 0, capi.Size(W, H), capi.Size(dw, dh), 3, good, None, None) == capi.ERR_BAD_ARG
    assert call(s=[(0, 64), (0x200000, 64)]) == capi.ERR_BAD_ARG
    assert call(s=src[:1]) == capi.ERR_BAD_ARG
    assert call(sf=capi.YUV420, s=yuv[:2]) == capi.ERR_BAD_ARG
    assert call(dst=f32[:2]) == capi.ERR_BAD_ARG
    # n == 0
    assert capi.convert_warp_tensor(ex, capi.NV12, 1, 0, W, H, dw, dh, good, _norm(capi), n=0, check=False) == capi.ERR_BAD_ARG
    # bad sizes
    for size in ((0, H, dw, dh), (W, 0, dw, dh), (W, H, 0, dh), (W, H, dw, 0), (70000, H, dw, dh), (W, H, 70000, dh)):
        assert call(size=size) == capi.ERR_BAD_ARG, size
    # a matrix coefficient that is not finite or exceeds 2^24 in magnitude (2^24 itself is accepted up to the device guard: not called here)
    for k in range(6):
        for bad in (math.nan, math.inf, -math.inf, 16777218.0, -3.0e7):
            m = list(ident)
            m[k] = bad
            assert call(m=m) == capi.ERR_BAD_ARG, (k, bad)
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
    jobs = [(src, f32, ident)] * 100 + [(src, f32, (1.0, math.nan, 0.0, 0.0, 1.0, 0.0))]
    assert call(jobs=jobs) == capi.ERR_BAD_ARG
    with pytest.raises(capi.VpfError):
        capi.convert_warp_tensor(ex, capi.NV12, 1, 0, W, H, dw, dh, capi.make_warps([(src, f32, (math.inf, 0, 0, 0, 1, 0))]), _norm(capi))


@pytest.mark.parametrize("sf", ["NV12", "YUV420"])
def test_premise_identity_translation_is_the_crop(oracle, sf):
    """identity + integer translation == the crop of the plain conversion, at odd and even offsets and touching the right and bottom edges
    (sx reaches W - 1 exactly); REPLICATE == CONSTANT wherever every pixel is in range; a wholly-outside job is all border"""
    o = oracle
    W, H, dw, dh = 131, 79, 61, 35
    src = o.synth(getattr(o, sf), W, H, 977)
    st, rgb = o.convert(getattr(o, sf), o.RGB_PLANAR, 1, 0, W, H, src, o.FP32)
    assert st == 0
    border = (7, 114, 250)
    for tx, ty in ((33, 5), (16, 8), (W - dw, H - dh), (0, 0)):
        m = (1, 0, tx, 0, 1, ty)
        got = warp_reference_u8(o, sf, 1, 0, W, H, m, dw, dh, border, 0, rgb=rgb)
        assert np.array_equal(got, np.stack([p[ty:ty + dh, tx:tx + dw] for p in rgb])), (tx, ty)
        assert np.array_equal(got, warp_reference_u8(o, sf, 1, 0, W, H, m, dw, dh, border, 1, src=src))
    rot = (0.9, -0.3, 30.0, 0.3, 0.9, 2.0)  # in range everywhere: x in [19.8, 84], y in [2, 50.6]
    sx, sy = warp_maps(rot, dw, dh, W, H, 0)
    assert sx.min() >= 0 and sx.max() <= W - 1 and sy.min() >= 0 and sy.max() <= H - 1
    assert np.array_equal(warp_reference_u8(o, sf, 1, 0, W, H, rot, dw, dh, border, 0, rgb=rgb), warp_reference_u8(o, sf, 1, 0, W, H, rot, dw, dh, border, 1, rgb=rgb))
    out = warp_reference_u8(o, sf, 1, 0, W, H, (1, 0, 500, 0, 1, 0), dw, dh, border, 0, rgb=rgb)
    assert all((out[c] == border[c]).all() for c in range(3))
    edge = warp_reference_u8(o, sf, 1, 0, W, H, (1, 0, 500, 0, 1, 0), dw, dh, border, 1, rgb=rgb)  # REPLICATE: the right edge column, rows 0 ..
    assert np.array_equal(edge, np.stack([np.repeat(p[0:dh, W - 1:W], dw, axis=1) for p in rgb]))


def test_python_layers_exist():
    import sys

    sys.path.insert(0, os.path.join(ROOT, "videoprocessingframework_amd"))
    import PyNvCodec as nvc  # the project's own extension: a build that does not import is a failure, not a skip
    assert hasattr(nvc.PySurfaceConvertResizer, "ExecuteWarpsToTensor")
    stub = open(os.path.join(ROOT, "videoprocessingframework_amd", "PyNvCodec", "__init__.pyi")).read()
    assert "def ExecuteWarpsToTensor(" in stub
    src = open(os.path.join(ROOT, "videoprocessingframework_amd", "PytorchNvCodec", "__init__.py")).read()
    assert ("def warps_to_normalized_tensor(resizer, surfaces, surface_index, matrices, mean, std, dtype=torch.float32, bgr=False, border=(0, 0, 0), "
            "border_mode=\"constant\", out=None, cc_ctx=None)") in src


def test_binding_validation_without_gpu():
    """PySurfaceConvertResizer.ExecuteWarpsToTensor: ValueError for a bad mean / std, False for a wrong surface, a bad index, a refused matrix, border
    or mode — all before any device work (host-memory surfaces, a fake destination address)"""
    import sys

    sys.path.insert(0, os.path.join(ROOT, "videoprocessingframework_amd"))
    import PyNvCodec as nvc  # the project's own extension: a build that does not import is a failure, not a skip
    nvc._UseHostAllocator(True)
    try:
        PF = nvc.PixelFormat
        r = nvc.PySurfaceConvertResizer(64, 32, PF.NV12, 16, 8, PF.RGB_PLANAR, 0, 0)
        good = nvc.Surface.Make(PF.NV12, 64, 32, context=0)
        fake, mean, std, m = 0x400000, [0.485, 0.456, 0.406], [0.229, 0.224, 0.225], [[1, 0, 3, 0, 1, 5]]
        with pytest.raises(ValueError):
            r.ExecuteWarpsToTensor([good], [0], m, fake, 0, [0, 0, 0], [1, 0, 1])
        assert not r.ExecuteWarpsToTensor([good], [], [], fake, 0, mean, std)
        assert not r.ExecuteWarpsToTensor([], [0], m, fake, 0, mean, std)
        assert not r.ExecuteWarpsToTensor([good], [1], m, fake, 0, mean, std)          # no such surface
        assert not r.ExecuteWarpsToTensor([good], [-1], m, fake, 0, mean, std)         # negative
        assert not r.ExecuteWarpsToTensor([good], [0, 0], m, fake, 0, mean, std)       # two indices, one matrix
        assert not r.ExecuteWarpsToTensor([good], [0], [[math.nan, 0, 3, 0, 1, 5]], fake, 0, mean, std)
        assert not r.ExecuteWarpsToTensor([good], [0], [[1, 0, 3.0e7, 0, 1, 5]], fake, 0, mean, std)
        assert not r.ExecuteWarpsToTensor([good], [0], m, fake, 0, mean, std, border=[0, 256, 0])
        assert not r.ExecuteWarpsToTensor([good], [0], m, fake, 0, mean, std, border_mode=2)
        assert not r.ExecuteWarpsToTensor([nvc.Surface.Make(PF.NV12, 32, 32, context=0)], [0], m, fake, 0, mean, std)   # wrong size
        assert not r.ExecuteWarpsToTensor([nvc.Surface.Make(PF.YUV420, 64, 32, context=0)], [0], m, fake, 0, mean, std)  # wrong format
        assert not r.ExecuteWarpsToTensor([good], [0], m, fake, 3, mean, std)                  # unknown dtype
        assert not r.ExecuteWarpsToTensor([good], [0], m, fake, 0, mean, std, row_stride=66)   # not a multiple of 4
        assert not r.ExecuteWarpsToTensor([good], [0], m, fake, 0, mean, std, row_stride=60)   # below 16 x 4 bytes
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

    def ExecuteWarpsToTensor(self, *a, **k):
        raise AssertionError("validation must come first")


def test_python_value_errors():
    """warps_to_normalized_tensor: ValueError for matrices on a device (the message says .cpu()), a wrong shape, a non-float dtype, a non-finite or
    oversized coefficient, a bad surface index, a border value outside 0..255, an unknown mode"""
    import torch
    from videoprocessingframework_amd import PytorchNvCodec as pnc

    rs, surfs, mean, std = _Resizer(), [_Surf(), _Surf()], (0, 0, 0), (1, 1, 1)
    ident = [[1.0, 0.0, 3.0], [0.0, 1.0, 5.0]]

    def call(matrices=None, index=(0,), **kw):
        return pnc.warps_to_normalized_tensor(rs, surfs, list(index), [ident] if matrices is None else matrices, mean, std, **kw)

    bad_matrices = [
        torch.zeros((1, 3, 2)), torch.zeros((2, 3)), torch.zeros((1, 2, 3), dtype=torch.int64), np.zeros((1, 2, 3), dtype=np.int32),
        np.zeros((1, 6), dtype=np.float32), [[[1.0, 0.0], [0.0, 1.0]]],
        [[[math.nan, 0.0, 3.0], [0.0, 1.0, 5.0]]], [[[1.0, math.inf, 3.0], [0.0, 1.0, 5.0]]], [[[1.0, 0.0, 3.0e7], [0.0, 1.0, 5.0]]],
        np.array([[[1.0, 0.0, 1e300], [0.0, 1.0, 5.0]]]),  # float64 that overflows float32
    ]
    for mtx in bad_matrices:
        with pytest.raises(ValueError):
            call(mtx)
    with pytest.raises(ValueError, match=r"\.cpu\(\)"):
        call(torch.empty((1, 2, 3), device="meta"))
    for index in ((2,), (-1,), (0, 1), (0.5,)):
        with pytest.raises(ValueError):
            call(index=index)
    for border in ((0, 0, 256), (-1, 0, 0), (0, 0), (0.5, 0, 0)):
        with pytest.raises(ValueError):
            call(border=border)
    with pytest.raises(ValueError):
        call(border_mode="reflect")
    with pytest.raises(ValueError):
        call(dtype=torch.float64)
    # accepted spellings: nested lists, float32 / float64 tensors and arrays of shape [K, 2, 3]; float64 rounds to float32 once
    want = [[float(np.float32(v)) for v in (1.1, 0.0, 3.0, 0.0, 1.0, 5.0)]]
    m = [[[1.1, 0.0, 3.0], [0.0, 1.0, 5.0]]]
    for spelled in (m, torch.tensor(m, dtype=torch.float64), torch.tensor(m, dtype=torch.float32), np.array(m), np.array(m, dtype=np.float32)):
        assert pnc._matrices_list(spelled, "t") == want
