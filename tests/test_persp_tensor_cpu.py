"""The fused multi-ROI perspective warp into a normalised tensor (vpf_convert_persp_tensor), without a GPU: the symbol, the struct and the Python layers
exist, every validation rule answers before any device work (fake pointers: nothing here may reach a launch), quads_to_homographies solves what it
says, and the premise of tests/test_gpu_persp_tensor.py holds — the ground truth of a perspective warp is composed from the oracle's conversion of
the whole frame and its remap of packed RGB on float32 maps written exactly as the definition (pixels with !(w > 0) out of range under CONSTANT,
overwritten with the border afterwards under REPLICATE), into a destination pre-filled with the border; with the last row (0, 0, 1) it is the affine
reference (tests/test_warp_tensor_cpu.py::warp_reference_u8)."""
import math
import os
import subprocess

import numpy as np
import pytest

from test_warp_tensor_cpu import warp_reference_u8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def persp_coords(m, dx, dy):
    """the definition's (sx, sy, front) of float32 arrays dx, dy before any border mode: every operation separately rounded, in the definition's
    order, the division IEEE; where !(w > 0) sx = sy = 0 and front is False"""
    m = np.asarray(m, dtype=F32).reshape(9)
    dx, dy = np.asarray(dx, dtype=F32), np.asarray(dy, dtype=F32)
    nx = ((m[0] * dx + m[1] * dy) + m[2]).astype(F32)
    ny = ((m[3] * dx + m[4] * dy) + m[5]).astype(F32)
    w = ((m[6] * dx + m[7] * dy) + m[8]).astype(F32)
    assert nx.dtype == F32 and ny.dtype == F32 and w.dtype == F32
    front = w > 0
    ws = np.where(front, w, F32(1))
    with np.errstate(over="ignore", divide="ignore", under="ignore"):
        sx, sy = (nx / ws).astype(F32), (ny / ws).astype(F32)
    assert sx.dtype == F32 and not np.isnan(sx[front]).any() and not np.isnan(sy[front]).any()
    return np.where(front, sx, F32(0)), np.where(front, sy, F32(0)), front


def persp_maps(m, dw, dh, W, H, mode):
    """(sx, sy, front) as float32 arrays [dh, dw]; REPLICATE: a max, then a min on the pixels in front of the plane"""
    dx, dy = np.broadcast_arrays(np.arange(dw, dtype=F32)[None, :], np.arange(dh, dtype=F32)[:, None])
    sx, sy, front = persp_coords(m, dx, dy)
    if mode == 1:
        sx, sy = np.minimum(np.maximum(sx, F32(0)), F32(W - 1)), np.minimum(np.maximum(sy, F32(0)), F32(H - 1))
    return np.ascontiguousarray(sx), np.ascontiguousarray(sy), front


def persp_reference_u8(orc, sf, cs, cr, W, H, m, dw, dh, border, mode, rgb=None, src=None):
    """the definition (include/vpf_hip.h) composed from the oracle -> [3, dh, dw] bytes.  `rgb`: the converted frame when the caller already has it."""
    if rgb is None:
        st, rgb = orc.convert(getattr(orc, sf), orc.RGB_PLANAR, cs, cr, W, H, src, orc.FP32)
        assert st == 0
    packed = np.ascontiguousarray(np.stack(rgb, axis=-1).reshape(H, 3 * W))
    sx, sy, front = persp_maps(m, dw, dh, W, H, mode)
    fill = F32(-1) if mode == 0 else F32(0)  # CONSTANT: out of range, the pre-filled border stays; REPLICATE: any pixel, overwritten below
    sx, sy = np.where(front, sx, fill), np.where(front, sy, fill)
    dst = np.ascontiguousarray(np.broadcast_to(np.asarray(border, np.uint8), (dh, dw, 3)).reshape(dh, 3 * dw))
    st, out = orc.remap(orc.RGB, W, H, [packed], np.ascontiguousarray(sx), np.ascontiguousarray(sy), orc.FP32, dst=[dst])
    assert st == 0
    out = np.array(out[0].reshape(dh, dw, 3).transpose(2, 0, 1), order="C")  # (a copy of its own: the border is written into it)
    for c in range(3):
        out[c][~front] = border[c]
    return out


def in_range_share(m, dw, dh, W, H):
    sx, sy, front = persp_maps(m, dw, dh, W, H, 0)
    return float((front & (sx >= 0) & (sx <= W - 1) & (sy >= 0) & (sy <= H - 1)).mean()), float(front.mean())


KEYSTONE = (1.1, .12, 8, .05, 1.2, 4, .0015, .0021, 1)
NAMED = {  # the matrices of the GPU test on 131 x 79 -> 61 x 35, with the share of in-range pixels of the reference itself (and of w > 0)
    "keystone": (KEYSTONE, 1.00, 1.0),
    "keystone x 3.7": (tuple(3.7 * v for v in KEYSTONE), 1.00, 1.0),
    "strong": ((.9, -.4, 30, .3, 1.4, -5, .004, .012, .8), 0.98, 1.0),
    "down-scale": ((2.9, .1, -20, .05, 2.9, -10, .002, .004, 1), 0.79, 1.0),
    "horizon": ((1, 0, 20, 0, 1, 10, -.03, 0, 1), 0.34, 0.56),
    "horizon on a pixel": ((1, 0, 20, 0, 1, 10, -.03125, 0, 1), 0.33, None),
    "huge": ((1, 0, 3, 0, 1, 2, 0, 0, 1e-30), 0.0, 1.0),
    "denormal w": ((1, 0, 3, 0, 1, 2, 0, 0, 1e-40), 0.0, 1.0),
    "behind": ((1, 0, 33, 0, 1, 5, 0, 0, -1), 0.0, 0.0),
    "cancelling": ((3e5, 0, -3e5 * 20 + 40.25, 0, 1, 7, 0, 0, 1), None, 1.0),
    # cancellation in nx on the ONE row a last tile row of a 33-row destination holds (dy = 32): nx moves in steps of one (the ulp of 1.27e7) while w
    # grows 2 % per pixel, so sx is a sawtooth along dx and pixels next to a tile corner lie outside the corners' box, the extra pixel included —
    # found by search for 131 x 79 -> 33 x 33 (tests/test_persp_bounds_cpu.py::test_named_cases counts the pixels that take the per-pixel fallback)
    "sawtooth": ((0.09039774537086487, -396405.5, 12684981.0, 0.0, 0.0, 2.313730239868164, 0.0011883797124028206, 0.0, 0.060716427862644196), None, 1.0),
}


def test_named_matrices_are_what_the_gpu_test_takes_them_for():
    W, H, dw, dh = 131, 79, 61, 35
    for name, (m, share, front_share) in NAMED.items():
        got, gf = in_range_share(m, dw, dh, W, H)
        if share is not None:
            assert abs(got - share) < 0.006, (name, got)
        if front_share is not None:
            assert abs(gf - front_share) < 0.006, (name, gf)
    sx, sy, front = persp_maps(NAMED["horizon on a pixel"][0], dw, dh, W, H, 0)
    assert front[:, :32].all() and not front[:, 32:].any()  # w is exactly 0 at dx = 32
    sx, sy, front = persp_maps(NAMED["denormal w"][0], dw, dh, W, H, 0)
    assert front.all() and np.isposinf(sx).all() and np.isposinf(sy).all()
    sx, sy, front = persp_maps(NAMED["denormal w"][0], dw, dh, W, H, 1)
    assert (sx == W - 1).all() and (sy == H - 1).all()
    sx, sy, front = persp_maps(NAMED["huge"][0], dw, dh, W, H, 0)
    assert np.isfinite(sx).all() and sx.min() > 1e29


def test_symbols_and_bindings_exist(capi):
    assert "vpf_convert_persp_tensor" in capi.EXPORTS
    assert hasattr(capi.lib(), "vpf_convert_persp_tensor")
    nm = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert " vpf_convert_persp_tensor\n" in nm
    assert callable(capi.make_persps) and callable(capi.convert_persp_tensor)
    h = open(os.path.join(ROOT, "include", "vpf_hip.h")).read()
    for decl in ("typedef struct vpf_persp_io", "VPF_API vpf_status vpf_convert_persp_tensor("):
        assert h.index(decl) > h.index("VPF_API vpf_status vpf_convert_warp_tensor("), decl


def test_struct_layout(capi, tmp_path):
    """vpf_persp_io is 136 bytes with no implicit padding (6 planes of 16 B, nine floats, one reserved word), in ctypes and in C"""
    C = capi.C
    assert C.sizeof(capi.PerspIO) == 136
    assert (capi.PerspIO.src.offset, capi.PerspIO.dst.offset, capi.PerspIO.m.offset, capi.PerspIO.reserved.offset) == (0, 48, 96, 132)
    assert sum(C.sizeof(t) for _, t in capi.PerspIO._fields_) == 136
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "vpf_hip.h"\nint main(void){ printf("%zu %zu %zu %zu %zu\\n", sizeof(vpf_persp_io), '
                   'offsetof(vpf_persp_io, src), offsetof(vpf_persp_io, dst), offsetof(vpf_persp_io, m), offsetof(vpf_persp_io, reserved)); return 0; }\n')
    exe = tmp_path / "t"
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert subprocess.run([str(exe)], capture_output=True, text=True).stdout.split() == ["136", "0", "48", "96", "132"]


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
    p16 = [(0x100000, 128), (0x200000, 128)]
    f32 = [(0x400000, 64), (0x500000, 64), (0x600000, 64)]  # dw * 4 = 64
    f16 = [(0x400000, 32), (0x500000, 32), (0x600000, 32)]
    ident = (1.0, 0.0, 3.0, 0.0, 1.0, 5.0, 0.0, 0.0, 1.0)
    _none = object()

    def call(dst=f32, norm=None, sf=capi.NV12, cs=1, cr=0, s=src, size=(W, H, dw, dh), m=ident, jobs=None, opts=_none):
        jobs = capi.make_persps([(s, dst, m)] if jobs is None else jobs)
        return capi.convert_persp_tensor(ex, sf, cs, cr, size[0], size[1], size[2], size[3], jobs, _norm(capi) if norm is None else norm,
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
    # unsupported comes before bad: an unknown mode with a NaN coefficient
    assert call(opts=capi.make_warp_opts(2), m=(math.nan,) * 9) == capi.ERR_UNSUPPORTED
    # non-zero reserved fields: the options', a plane's, the job's
    o = capi.make_warp_opts(capi.WARP_REPLICATE, (1, 2, 3))
    o.reserved = 1
    assert call(opts=o) == capi.ERR_BAD_ARG
    j = capi.make_persps([(src, f32, ident)])
    j[0].dst[1].reserved = 7
    assert capi.convert_persp_tensor(ex, capi.NV12, 1, 0, W, H, dw, dh, j, _norm(capi), check=False) == capi.ERR_BAD_ARG
    j = capi.make_persps([(src, f32, ident)])
    j[0].src[0].reserved = 1
    assert capi.convert_persp_tensor(ex, capi.NV12, 1, 0, W, H, dw, dh, j, _norm(capi), check=False) == capi.ERR_BAD_ARG
    j = capi.make_persps([(src, f32, ident)])
    j[0].reserved = 1
    assert capi.convert_persp_tensor(ex, capi.NV12, 1, 0, W, H, dw, dh, j, _norm(capi), check=False) == capi.ERR_BAD_ARG
    # null pointers: exec, the job array, the parameters, a plane
    L, Cb = capi.lib(), capi.C.byref
    good = capi.make_persps([(src, f32, ident)] * 3)
    assert L.vpf_convert_persp_tensor(None, capi.NV12, 1, 0, capi.Size(W, H), capi.Size(dw, dh), 3, good, Cb(_norm(capi)), None) == capi.ERR_BAD_ARG
    assert L.vpf_convert_persp_tensor(Cb(ex), capi.NV12, 1, 0, capi.Size(W, H), capi.Size(dw, dh), 3, None, Cb(_norm(capi)), None) == capi.ERR_BAD_ARG
    assert L.vpf_convert_persp_tensor(Cb(ex), capi.NV12, 1, 0, capi.Size(W, H), capi.Size(dw, dh), 3, good, None, None) == capi.ERR_BAD_ARG
    assert call(s=[(0, 64), (0x200000, 64)]) == capi.ERR_BAD_ARG
    assert call(s=src[:1]) == capi.ERR_BAD_ARG
    assert call(sf=capi.YUV420, s=yuv[:2]) == capi.ERR_BAD_ARG
    assert call(dst=f32[:2]) == capi.ERR_BAD_ARG
    # n == 0
    assert capi.convert_persp_tensor(ex, capi.NV12, 1, 0, W, H, dw, dh, good, _norm(capi), n=0, check=False) == capi.ERR_BAD_ARG
    # bad sizes
    for size in ((0, H, dw, dh), (W, 0, dw, dh), (W, H, 0, dh), (W, H, dw, 0), (70000, H, dw, dh), (W, H, 70000, dh)):
        assert call(size=size) == capi.ERR_BAD_ARG, size
    # one of the NINE coefficients not finite or above 2^24 in magnitude
    for k in range(9):
        for bad in (math.nan, math.inf, -math.inf, 16777218.0, -3.0e7):
            m = list(ident)
            m[k] = bad
            assert call(m=m) == capi.ERR_BAD_ARG, (k, bad)
    # short pitches: source and destination; P10 planes at odd addresses
    assert call(s=[(0x100000, 63), (0x200000, 64)]) == capi.ERR_BAD_ARG
    assert call(s=[(0x100000, 64), (0x200000, 63)]) == capi.ERR_BAD_ARG
    assert call(sf=capi.YUV420, s=[(0x100000, 64), (0x200000, 31), (0x300000, 32)]) == capi.ERR_BAD_ARG
    assert call(sf=capi.P10, s=[(0x100001, 128), (0x200000, 128)]) == capi.ERR_BAD_ARG
    assert call(sf=capi.P10, s=[(0x100000, 127), (0x200000, 128)]) == capi.ERR_BAD_ARG
    assert p16  # (a well-formed P10 job would reach the device: not called here)
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
    # NHWC: one plane of 3 x dw elements
    assert call(dst=[(0x400000, 3 * 64 - 4)], norm=_norm(capi, flags=capi.TENSOR_NHWC)) == capi.ERR_BAD_ARG
    for bad in (math.nan, math.inf, -math.inf):
        for c in range(3):
            sc, bi = [0.01] * 3, [-1.0] * 3
            sc[c] = bad
            assert call(norm=_norm(capi, scale=sc)) == capi.ERR_BAD_ARG
            sc[c], bi[c] = 0.01, bad
            assert call(norm=_norm(capi, bias=bi)) == capi.ERR_BAD_ARG
    # one bad job among good ones, beyond the first job table (82 jobs per table): everything is validated before the first launch
    jobs = [(src, f32, ident)] * 90 + [(src, f32, (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, math.nan, 1.0))]
    assert call(jobs=jobs) == capi.ERR_BAD_ARG
    with pytest.raises(capi.VpfError):
        capi.convert_persp_tensor(ex, capi.NV12, 1, 0, W, H, dw, dh, capi.make_persps([(src, f32, (1, 0, 0, 0, 1, 0, math.inf, 0, 1))]), _norm(capi))


@pytest.mark.parametrize("sf", ["NV12", "YUV420"])
def test_premise_last_row_001_is_the_affine_reference(oracle, sf):
    """with the last row (0, 0, 1) w is exactly 1 and nx / 1 == nx: the composed perspective reference equals warp_reference_u8 in both modes; a
    matrix behind the plane is all border in both modes; the horizon matrix keeps the border right of dx = 32 under REPLICATE too"""
    o = oracle
    W, H, dw, dh = 131, 79, 61, 35
    src = o.synth(getattr(o, sf), W, H, 977)
    st, rgb = o.convert(getattr(o, sf), o.RGB_PLANAR, 1, 0, W, H, src, o.FP32)
    assert st == 0
    border = (7, 114, 250)
    c30, s30 = 1.3 * math.cos(math.radians(30)), 1.3 * math.sin(math.radians(30))
    for m6 in ((1, 0, 33, 0, 1, 5), (1, 0, W - dw + 0.5, 0, 1, H - dh + 0.5), (c30, -s30, 40, s30, c30, -10), (2.9, 0, -20, 0, 2.9, -10), (1, 0, 500, 0, 1, 0)):
        for mode in (0, 1):
            want = warp_reference_u8(o, sf, 1, 0, W, H, m6, dw, dh, border, mode, rgb=rgb)
            assert np.array_equal(persp_reference_u8(o, sf, 1, 0, W, H, tuple(m6) + (0, 0, 1), dw, dh, border, mode, rgb=rgb), want), (m6, mode)
    for mode in (0, 1):
        out = persp_reference_u8(o, sf, 1, 0, W, H, NAMED["behind"][0], dw, dh, border, mode, rgb=rgb)
        assert all((out[c] == border[c]).all() for c in range(3))
        out = persp_reference_u8(o, sf, 1, 0, W, H, NAMED["horizon on a pixel"][0], dw, dh, border, mode, rgb=rgb)
        assert all((out[c][:, 32:] == border[c]).all() for c in range(3))
        assert not all((out[c][:, :32] == border[c]).all() for c in range(3))
    edge = persp_reference_u8(o, sf, 1, 0, W, H, NAMED["denormal w"][0], dw, dh, border, 1, rgb=rgb)  # REPLICATE: pixel (W - 1, H - 1) everywhere
    assert all((edge[c] == rgb[c][H - 1, W - 1]).all() for c in range(3))
    out = persp_reference_u8(o, sf, 1, 0, W, H, NAMED["denormal w"][0], dw, dh, border, 0, rgb=rgb)  # CONSTANT: +inf is out of range
    assert all((out[c] == border[c]).all() for c in range(3))


def test_python_layers_exist():
    import inspect
    import sys

    sys.path.insert(0, os.path.join(ROOT, "videoprocessingframework_amd"))
    import PyNvCodec as nvc  # the project's own extension: a build that does not import is a failure, not a skip
    from videoprocessingframework_amd import PytorchNvCodec as pnc

    assert hasattr(nvc.PySurfaceConvertResizer, "ExecutePerspsToTensor")
    assert "channels_last: bool = False" in nvc.PySurfaceConvertResizer.ExecutePerspsToTensor.__doc__
    stub = open(os.path.join(ROOT, "videoprocessingframework_amd", "PyNvCodec", "__init__.pyi")).read()
    assert "def ExecutePerspsToTensor(" in stub
    hpp = open(os.path.join(ROOT, "videoprocessingframework_amd", "csrc", "tc", "Tasks.hpp")).read()
    assert "TaskExecStatus RunTensorPersps(" in hpp
    want = list(inspect.signature(pnc.warps_to_normalized_tensor).parameters.items())
    got = list(inspect.signature(pnc.persps_to_normalized_tensor).parameters.items())
    assert [(k, v.default) for k, v in got] == [(k, v.default) for k, v in want] and got[-1][0] == "channels_last"
    assert list(inspect.signature(pnc.quads_to_homographies).parameters) == ["quads", "size"]


def test_binding_validation_without_gpu():
    """PySurfaceConvertResizer.ExecutePerspsToTensor: ValueError for a bad mean / std, False for a wrong surface, a bad index, a refused matrix, border
    or mode — all before any device work (host-memory surfaces, a fake destination address)"""
    import sys

    sys.path.insert(0, os.path.join(ROOT, "videoprocessingframework_amd"))
    import PyNvCodec as nvc  # the project's own extension: a build that does not import is a failure, not a skip
    nvc._UseHostAllocator(True)
    try:
        PF = nvc.PixelFormat
        r = nvc.PySurfaceConvertResizer(64, 32, PF.NV12, 16, 8, PF.RGB_PLANAR, 0, 0)
        good = nvc.Surface.Make(PF.NV12, 64, 32, context=0)
        fake, mean, std, m = 0x400000, [0.485, 0.456, 0.406], [0.229, 0.224, 0.225], [[1, 0, 3, 0, 1, 5, 0, 0, 1]]
        with pytest.raises(ValueError):
            r.ExecutePerspsToTensor([good], [0], m, fake, 0, [0, 0, 0], [1, 0, 1])
        with pytest.raises(TypeError):
            r.ExecutePerspsToTensor([good], [0], [[1, 0, 3, 0, 1, 5]], fake, 0, mean, std)  # six floats: the affine method's matrix
        assert not r.ExecutePerspsToTensor([good], [], [], fake, 0, mean, std)
        assert not r.ExecutePerspsToTensor([], [0], m, fake, 0, mean, std)
        assert not r.ExecutePerspsToTensor([good], [1], m, fake, 0, mean, std)          # no such surface
        assert not r.ExecutePerspsToTensor([good], [-1], m, fake, 0, mean, std)         # negative
        assert not r.ExecutePerspsToTensor([good], [0, 0], m, fake, 0, mean, std)       # two indices, one matrix
        for k in range(9):
            for bad in (math.nan, 3.0e7):
                mm = list(m[0])
                mm[k] = bad
                assert not r.ExecutePerspsToTensor([good], [0], [mm], fake, 0, mean, std), (k, bad)
        assert not r.ExecutePerspsToTensor([good], [0], m, fake, 0, mean, std, border=[0, 256, 0])
        assert not r.ExecutePerspsToTensor([good], [0], m, fake, 0, mean, std, border_mode=2)
        assert not r.ExecutePerspsToTensor([nvc.Surface.Make(PF.NV12, 32, 32, context=0)], [0], m, fake, 0, mean, std)   # wrong size
        assert not r.ExecutePerspsToTensor([nvc.Surface.Make(PF.YUV420, 64, 32, context=0)], [0], m, fake, 0, mean, std)  # wrong format
        assert not r.ExecutePerspsToTensor([good], [0], m, fake, 3, mean, std)                  # unknown dtype
        assert not r.ExecutePerspsToTensor([good], [0], m, fake, 0, mean, std, row_stride=66)   # not a multiple of 4
        assert not r.ExecutePerspsToTensor([good], [0], m, fake, 0, mean, std, row_stride=60)   # below 16 x 4 bytes
        assert not r.ExecutePerspsToTensor([good], [0], m, fake, 0, mean, std, row_stride=16 * 12 - 4, channels_last=True)  # below 16 x 3 x 4 bytes
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

    def ExecutePerspsToTensor(self, *a, **k):
        raise AssertionError("validation must come first")


def test_python_value_errors():
    """persps_to_normalized_tensor: the ValueErrors of warps_to_normalized_tensor, on [K, 3, 3] / [K, 9] matrices"""
    import torch
    from videoprocessingframework_amd import PytorchNvCodec as pnc

    rs, surfs, mean, std = _Resizer(), [_Surf(), _Surf()], (0, 0, 0), (1, 1, 1)
    ident = [[1.0, 0.0, 3.0], [0.0, 1.0, 5.0], [0.0, 0.0, 1.0]]

    def call(matrices=None, index=(0,), **kw):
        return pnc.persps_to_normalized_tensor(rs, surfs, list(index), [ident] if matrices is None else matrices, mean, std, **kw)

    def with_coef(k, v):
        flat = [c for row in ident for c in row]
        flat[k] = v
        return [[flat[0:3], flat[3:6], flat[6:9]]]

    bad_matrices = [
        torch.zeros((1, 2, 3)), torch.zeros((3, 3)), torch.zeros((1, 3, 3), dtype=torch.int64), np.zeros((1, 3, 3), dtype=np.int32),
        np.zeros((1, 6), dtype=np.float32), np.zeros((1, 8), dtype=np.float32), [[[1.0, 0.0], [0.0, 1.0], [0.0, 1.0]]],
        np.array(with_coef(2, 1e300)),  # float64 that overflows float32
    ]
    bad_matrices += [with_coef(k, v) for k in range(9) for v in (math.nan, math.inf, 3.0e7)]
    for mtx in bad_matrices:
        with pytest.raises(ValueError):
            call(mtx)
    with pytest.raises(ValueError, match=r"\.cpu\(\)"):
        call(torch.empty((1, 3, 3), device="meta"))
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
    # accepted spellings: nested lists, float32 / float64 tensors and arrays of shape [K, 3, 3] and [K, 9]; float64 rounds to float32 once
    want = [[float(np.float32(v)) for v in (1.1, 0.0, 3.0, 0.0, 1.0, 5.0, 0.001, 0.0, 1.0)]]
    m = [[[1.1, 0.0, 3.0], [0.0, 1.0, 5.0], [0.001, 0.0, 1.0]]]
    for spelled in (m, torch.tensor(m, dtype=torch.float64), torch.tensor(m, dtype=torch.float32), np.array(m), np.array(m, dtype=np.float32),
                    np.array(m).reshape(1, 9), torch.tensor(m).reshape(1, 9)):
        assert pnc._matrices_list(spelled, "t", rows=3) == want
    # the affine function's shapes are what they were
    with pytest.raises(ValueError):
        pnc._matrices_list(np.zeros((1, 3, 3), dtype=np.float32), "t")
    assert pnc._matrices_list(np.zeros((0,)), "t") == [] and pnc._matrices_list([], "t", rows=3) == []


def _apply(h, pts):
    """float64 homography [3, 3] on points [N, 2]"""
    p = np.concatenate([pts, np.ones((len(pts), 1))], axis=1) @ np.asarray(h, dtype=np.float64).T
    return p[:, :2] / p[:, 2:3]


def test_quads_to_homographies():
    """the four destination corners map to the quad within 1e-3 px; a unit-scale axis-aligned quad gives identity + translation; a batch of K solves
    equals K single solves; m22 = 1; float32 [K, 3, 3]; ValueError for other shapes and sizes below 2"""
    import torch
    from videoprocessingframework_amd import PytorchNvCodec as pnc

    rng = np.random.default_rng(5)
    dw, dh = 61, 35
    corners = np.array([[0, 0], [dw - 1, 0], [dw - 1, dh - 1], [0, dh - 1]], dtype=np.float64)
    quads = []
    for _ in range(40):
        c, s, a = rng.uniform(100, 1500, size=2), rng.uniform(0.3, 6.0), rng.uniform(0, 2 * math.pi)
        r = np.array([[math.cos(a), -math.sin(a)], [math.sin(a), math.cos(a)]])
        base = (corners - corners.mean(0)) * s @ r.T + c
        quads.append(base + rng.uniform(-0.15, 0.15, size=(4, 2)) * s * min(dw, dh))
    quads = np.array(quads)
    hs = pnc.quads_to_homographies(quads, (dw, dh))
    assert isinstance(hs, torch.Tensor) and hs.dtype == torch.float32 and tuple(hs.shape) == (40, 3, 3) and hs.device.type == "cpu"
    assert bool((hs[:, 2, 2] == 1).all())
    for k in range(40):
        assert np.abs(_apply(hs[k].numpy(), corners) - quads[k]).max() < 1e-3, k
        one = pnc.quads_to_homographies(quads[k:k + 1], (dw, dh))
        assert torch.equal(one[0], hs[k]), k
    # torch input, float32, a list
    assert torch.equal(pnc.quads_to_homographies(torch.tensor(quads), (dw, dh)), hs)
    assert tuple(pnc.quads_to_homographies(quads[:1].tolist(), [dw, dh]).shape) == (1, 3, 3)
    # a unit-scale axis-aligned quad: identity + translation
    tx, ty = 33.0, 5.0
    h = pnc.quads_to_homographies([[[tx, ty], [tx + dw - 1, ty], [tx + dw - 1, ty + dh - 1], [tx, ty + dh - 1]]], (dw, dh))[0].numpy()
    assert np.abs(h - np.array([[1, 0, tx], [0, 1, ty], [0, 0, 1]])).max() < 1e-6
    assert tuple(pnc.quads_to_homographies(np.zeros((0, 4, 2)), (dw, dh)).shape) == (0, 3, 3)
    for bad in (np.zeros((4, 2)), np.zeros((1, 4, 3)), np.zeros((1, 3, 2))):
        with pytest.raises(ValueError):
            pnc.quads_to_homographies(bad, (dw, dh))
    for size in ((1, 35), (61, 1), (61,), 61):
        with pytest.raises(ValueError):
            pnc.quads_to_homographies(quads, size)
