"""The fused multi-ROI affine warp with the matrices in DEVICE memory (vpf_convert_warp_tensor_dev, PySurfaceConvertResizer.ExecuteWarpsDevToTensor,
PytorchNvCodec.device_warps_to_normalized_tensor, PytorchNvCodec.rotated_boxes_to_warps), without a GPU: the symbol, the header and the bindings exist,
the structure has the declared layout, every host-side refusal answers before any device work (fake pointers: nothing here may reach a launch), the
Python entry raises ValueError where it says it does, rotated_boxes_to_warps is its definition to within the rounding of its few operations, and
the six new kernel instantiations use no scratch and at most 128 VGPRs."""
import inspect
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
NAME = "vpf_convert_warp_tensor_dev"


def test_symbol_header_and_bindings_exist(capi):
    assert NAME in capi.EXPORTS and hasattr(capi.lib(), NAME)
    nm = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert f" {NAME}\n" in nm
    assert callable(capi.make_warps_dev) and callable(capi.convert_warp_tensor_dev) and callable(capi.make_frame_srcs)
    h = open(os.path.join(ROOT, "include", "vpf_hip.h")).read()
    for decl in ("typedef struct vpf_warps_dev", f"VPF_API vpf_status {NAME}("):
        assert h.index(decl) > h.index("VPF_API vpf_status vpf_convert_warp_tensor("), decl
        assert h.index(decl) > h.index("typedef struct vpf_frame_src"), decl
    sys.path.insert(0, os.path.join(ROOT, "videoprocessingframework_amd"))
    nvc = pytest.importorskip("PyNvCodec")
    assert hasattr(nvc.PySurfaceConvertResizer, "ExecuteWarpsDevToTensor")
    stub = open(os.path.join(ROOT, "videoprocessingframework_amd", "PyNvCodec", "__init__.pyi")).read()
    assert "def ExecuteWarpsDevToTensor(self, surfaces: List[Surface], matrices_ptr: int, max_n: int, index_ptr: int, count_ptr: int, ptr: int, dtype: int" in stub
    src = open(os.path.join(ROOT, "videoprocessingframework_amd", "PytorchNvCodec", "__init__.py")).read()
    assert "def rotated_boxes_to_warps(boxes_cxcywha, dw, dh)" in src
    # the host-table entry still refuses device tensors, in its own words
    assert "pass matrices.cpu()" in src and "pass surface_index.cpu()" in src


def test_python_signature():
    torch = pytest.importorskip("torch")
    from videoprocessingframework_amd import PytorchNvCodec as pnc

    sig = inspect.signature(pnc.device_warps_to_normalized_tensor)
    assert list(sig.parameters) == ["resizer", "surfaces", "matrices", "mean", "std", "surface_index", "count", "max_step", "dtype", "bgr", "border",
                                    "border_mode", "out", "cc_ctx", "channels_last"]
    d = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert d == dict(surface_index=None, count=None, max_step=None, dtype=torch.float32, bgr=False, border=(0, 0, 0), border_mode="constant", out=None,
                     cc_ctx=None, channels_last=False)
    assert list(inspect.signature(pnc.rotated_boxes_to_warps).parameters) == ["boxes_cxcywha", "dw", "dh"]


def test_struct_layout(capi):
    """vpf_warps_dev: 96 bytes with no implicit padding, offsets 0 8 16 24 28 32 36 40 88; the header's field order is the ctypes order"""
    C = capi.C
    T = capi.WarpsDev
    assert C.sizeof(T) == 96 and sum(C.sizeof(t) for _, t in T._fields_) == 96
    names = ["matrices", "frame_index", "count", "matrix_stride", "frame_stride", "max_n", "max_step", "dst", "dst_job_stride"]
    assert [n for n, _ in T._fields_] == names
    assert [getattr(T, n).offset for n in names] == [0, 8, 16, 24, 28, 32, 36, 40, 88]
    assert dict(T._fields_)["max_step"] is C.c_float and dict(T._fields_)["dst_job_stride"] is C.c_uint64
    h = open(os.path.join(ROOT, "include", "vpf_hip.h")).read()
    body = h[h.index("typedef struct vpf_warps_dev"):h.index("} vpf_warps_dev;")]
    declared = re.findall(r"^\s+(?:const )?\w+\*? (\w+)(?:\[3\])?;", body, re.M)   # the declarations, not the words of their comments
    assert declared == names


def _norm(capi, dtype=0, flags=0, scale=(0.01, 0.01, 0.01), bias=(-1.0, -1.0, -1.0)):
    n = capi.TensorNorm()
    for c in range(3):
        n.scale[c], n.bias[c] = scale[c], bias[c]
    n.dtype, n.flags = dtype, flags
    return n


def test_validation_without_gpu(capi):
    """every host-side refusal, before any device work: every pointer below is fake (matrices, frame indices and count included: the host never
    dereferences them)"""
    ex = capi.make_exec()
    W, H, dw, dh = 64, 32, 16, 8
    src = [(0x100000, 64), (0x200000, 64)]
    yuv = [(0x100000, 64), (0x200000, 32), (0x300000, 32)]
    f32 = [(0x400000, 64), (0x500000, 64), (0x600000, 64)]  # dw * 4 = 64
    f16 = [(0x400000, 32), (0x500000, 32), (0x600000, 32)]
    MAT, IDX, CNT = 0x700000, 0x780000, 0x800000

    def call(dst=f32, norm=None, sf=capi.NV12, cs=1, cr=0, frames=None, size=(W, H, dw, dh), mats=MAT, index=IDX, count=CNT, max_n=7, mstride=24, fstride=4,
             job=3 * 8 * 64, n_frames=None, max_step=0.0, opts=None):
        fr = capi.make_frame_srcs([src] if frames is None else frames)
        t = capi.make_warps_dev(mats, max_n, dst, job, index, count, mstride, fstride, max_step)
        return capi.convert_warp_tensor_dev(ex, sf, cs, cr, size[0], size[1], size[2], size[3], fr, t, _norm(capi) if norm is None else norm, opts,
                                            n_frames=n_frames, check=False)

    # unsupported format, matrix, dtype, flag or border mode: the rules of the warp entry
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
    # non-zero reserved fields
    o = capi.make_warp_opts(capi.WARP_REPLICATE, (1, 2, 3))
    o.reserved = 1
    assert call(opts=o) == capi.ERR_BAD_ARG
    fr = capi.make_frame_srcs([src])
    fr[0].src[1].reserved = 5
    t = capi.make_warps_dev(MAT, 7, f32, 1536, IDX, CNT)
    assert capi.convert_warp_tensor_dev(ex, capi.NV12, 1, 0, W, H, dw, dh, fr, t, _norm(capi), check=False) == capi.ERR_BAD_ARG
    t.dst[2].reserved = 9
    assert capi.convert_warp_tensor_dev(ex, capi.NV12, 1, 0, W, H, dw, dh, capi.make_frame_srcs([src]), t, _norm(capi), check=False) == capi.ERR_BAD_ARG
    # null pointers: exec, the frames, the table, the parameters, the matrices, a plane
    L, Cb = capi.lib(), capi.C.byref
    fr, tb = capi.make_frame_srcs([src]), capi.make_warps_dev(MAT, 7, f32, 1536, IDX, CNT)
    args = (capi.NV12, 1, 0, capi.Size(W, H), capi.Size(dw, dh), 1)
    assert getattr(L, NAME)(None, *args, fr, Cb(tb), Cb(_norm(capi)), None) == capi.ERR_BAD_ARG
    assert getattr(L, NAME)(Cb(ex), *args, None, Cb(tb), Cb(_norm(capi)), None) == capi.ERR_BAD_ARG
    assert getattr(L, NAME)(Cb(ex), *args, fr, None, Cb(_norm(capi)), None) == capi.ERR_BAD_ARG
    assert getattr(L, NAME)(Cb(ex), *args, fr, Cb(tb), None, None) == capi.ERR_BAD_ARG
    assert call(mats=0) == capi.ERR_BAD_ARG
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
    # the new fields
    assert call(n_frames=0) == capi.ERR_BAD_ARG
    assert call(frames=[src] * 129) == capi.ERR_BAD_ARG
    for max_n in (0, 65536, 0xFFFFFFFF):
        assert call(max_n=max_n) == capi.ERR_BAD_ARG, max_n
    for off in (1, 2, 3):
        assert call(mats=MAT + off) == capi.ERR_BAD_ARG, off
        assert call(index=IDX + off) == capi.ERR_BAD_ARG, off
        assert call(count=CNT + off) == capi.ERR_BAD_ARG, off
    for stride in (0, 4, 20, 23, 25, 26, 27, 30):
        assert call(mstride=stride) == capi.ERR_BAD_ARG, stride
    for stride in (0, 1, 2, 3, 5, 6, 7, 10):
        assert call(fstride=stride) == capi.ERR_BAD_ARG, stride
    for job in (1, 2, 3, 1537, 1538):
        assert call(job=job) == capi.ERR_BAD_ARG, job
    assert call(dst=f16, norm=_norm(capi, dtype=1), job=769) == capi.ERR_BAD_ARG
    for step in (-1.0, -1e-30, math.nan, math.inf, -math.inf):
        assert call(max_step=step) == capi.ERR_BAD_ARG, step
    with pytest.raises(capi.VpfError):
        capi.convert_warp_tensor_dev(ex, capi.NV12, 1, 0, W, H, dw, dh, capi.make_frame_srcs([src]), capi.make_warps_dev(MAT, 0, f32, 1536), _norm(capi))


class _Resizer:
    """stands in for PySurfaceConvertResizer: a ValueError must come before the resizer is asked to run"""

    def DstSize(self):
        return (16, 8)

    def Stream(self):
        raise AssertionError("validation must come first")

    def ExecuteWarpsDevToTensor(self, *a, **k):
        raise AssertionError("validation must come first")


def test_python_value_errors():
    """device_warps_to_normalized_tensor: ValueError for host matrices, another dtype or shape, too many surfaces, a bad border or mode — before the
    resizer runs; warps_to_normalized_tensor still refuses device tensors"""
    torch = pytest.importorskip("torch")
    from videoprocessingframework_amd import PytorchNvCodec as pnc

    rs, surfs, mean, std = _Resizer(), [object(), object()], (0, 0, 0), (1, 1, 1)
    host = torch.zeros((3, 2, 3), dtype=torch.float32)
    for m in (host, torch.zeros((3, 6)), [[[1, 0, 0], [0, 1, 0]]], np.zeros((3, 2, 3), np.float32), None, torch.zeros((3, 2, 3), device="meta"),
              torch.zeros((3, 2, 3), dtype=torch.float64, device="meta"), torch.zeros((3, 3, 2), device="meta"), torch.zeros((3, 5), device="meta"),
              torch.zeros((6,), device="meta")):
        with pytest.raises(ValueError):
            pnc.device_warps_to_normalized_tensor(rs, surfs, m, mean, std)
    with pytest.raises(ValueError):
        pnc.device_warps_to_normalized_tensor(rs, surfs, host, mean, std, dtype=torch.float64)
    with pytest.raises(ValueError):
        pnc.device_warps_to_normalized_tensor(rs, [], host, mean, std)
    with pytest.raises(ValueError):
        pnc.device_warps_to_normalized_tensor(rs, [object()] * 129, host, mean, std)
    with pytest.raises(ValueError):
        pnc.device_warps_to_normalized_tensor(rs, surfs, host, mean, std, border_mode="reflect")
    with pytest.raises(ValueError):
        pnc.device_warps_to_normalized_tensor(rs, surfs, host, mean, std, border=(0, 0, 256))
    with pytest.raises(ValueError, match=r"\.cpu\(\)"):
        pnc.warps_to_normalized_tensor(rs, surfs, [0, 0, 0], torch.zeros((3, 2, 3), device="meta"), mean, std)


def _warps_exact(boxes, dw, dh):
    """rotated_boxes_to_warps restated in float64 on the float32 inputs: per coefficient (value, the largest magnitude among the terms summed into it)"""
    out = []
    for cx, cy, w, h, a in boxes:
        ax, ay, c, s = w / dw, h / dh, math.cos(a), math.sin(a)
        u0, v0 = 0.5 * ax - 0.5 * w, 0.5 * ay - 0.5 * h
        tx = [cx, 0.5 * ax * c, 0.5 * w * c, 0.5 * ay * s, 0.5 * h * s, 0.5]
        ty = [cy, 0.5 * ax * s, 0.5 * w * s, 0.5 * ay * c, 0.5 * h * c, 0.5]
        vals = [ax * c, -ay * s, cx + u0 * c - v0 * s - 0.5, ax * s, ay * c, cy + u0 * s + v0 * c - 0.5]
        mags = [abs(ax * c), abs(ay * s), max(abs(t) for t in tx), abs(ax * s), abs(ay * c), max(abs(t) for t in ty)]
        out.append((vals, mags))
    return out


def test_rotated_boxes_to_warps_is_its_definition():
    """every coefficient within 16 float32 ulps of the largest-magnitude term summed into it (at most about seven rounded operations and two trig
    evaluations of a few ulps each enter a coefficient): angles 0, +-pi/2, pi, 0.3 and random ones, boxes on a 1920 x 1080 frame; the destination
    pixel centre maps to the box centre; non-finite rows give non-finite matrices"""
    torch = pytest.importorskip("torch")
    from videoprocessingframework_amd import PytorchNvCodec as pnc

    rng = np.random.default_rng(9)
    boxes = [(960.0, 540.0, 200.0, 100.0, a) for a in (0.0, math.pi / 2, -math.pi / 2, math.pi, 0.3)]
    boxes += [(100.5, 900.25, 64.0, 48.0, 0.3), (1919.5, 0.5, 1.0, 1.0, 0.0), (12.0, 1070.0, 333.3, 7.7, -2.5), (1000.0, 500.0, 1920.0, 1080.0, 0.0)]
    boxes += [(float(rng.uniform(0, 1920)), float(rng.uniform(0, 1080)), float(rng.uniform(1, 600)), float(rng.uniform(1, 600)), float(rng.uniform(-7, 7)))
              for _ in range(400)]
    b32 = torch.tensor(boxes, dtype=torch.float32)
    rounded = [[float(v) for v in row] for row in b32.tolist()]      # the float32 inputs, exactly
    for (dw, dh) in ((112, 112), (64, 48), (1, 1), (224, 96)):
        got = pnc.rotated_boxes_to_warps(b32, dw, dh)
        assert got.dtype == torch.float32 and tuple(got.shape) == (len(boxes), 2, 3) and got.device.type == "cpu"
        g = got.reshape(-1, 6).to(torch.float64).numpy()
        for i, (vals, mags) in enumerate(_warps_exact(rounded, dw, dh)):
            for k in range(6):
                tol = 16 * float(np.spacing(np.float32(mags[k])))
                assert abs(g[i, k] - vals[k]) <= tol, (dw, dh, boxes[i], k, g[i, k], vals[k], tol)
        # the centre of the destination maps to the box centre minus half a pixel (the index of the pixel whose centre that is)
        cx = g[:, 0] * ((dw - 1) / 2) + g[:, 1] * ((dh - 1) / 2) + g[:, 2]
        cy = g[:, 3] * ((dw - 1) / 2) + g[:, 4] * ((dh - 1) / 2) + g[:, 5]
        assert np.allclose(cx, np.array(rounded)[:, 0] - 0.5, atol=2e-3) and np.allclose(cy, np.array(rounded)[:, 1] - 0.5, atol=2e-3)
    # angle 0 is the resize convention of an axis-aligned rectangle: m00 = w / dw, m02 = x + 0.5 w / dw - 0.5 with x = cx - w / 2
    m = pnc.rotated_boxes_to_warps(torch.tensor([[110.0, 60.0, 100.0, 50.0, 0.0]]), 50, 25)[0].tolist()
    assert m == [[2.0, -0.0, 60.5], [0.0, 2.0, 35.5]] or m == [[2.0, 0.0, 60.5], [0.0, 2.0, 35.5]]
    # float64 input gives float32 output; non-finite rows give non-finite matrices, the other rows are untouched
    bad = torch.tensor([[960.0, 540.0, 200.0, 100.0, 0.3], [math.nan, 540.0, 200.0, 100.0, 0.3], [960.0, 540.0, math.inf, 100.0, 0.3],
                        [960.0, 540.0, 200.0, 100.0, math.nan], [960.0, -math.inf, 200.0, 100.0, 0.0]], dtype=torch.float64)
    out = pnc.rotated_boxes_to_warps(bad, 112, 112)
    assert out.dtype == torch.float32
    finite = torch.isfinite(out).reshape(5, 6).all(dim=1).tolist()
    assert finite == [True, False, False, False, False]
    assert torch.equal(out[0], pnc.rotated_boxes_to_warps(bad[:1], 112, 112)[0])
    assert tuple(pnc.rotated_boxes_to_warps(torch.zeros((0, 5)), 8, 8).shape) == (0, 2, 3)
    for wrong in (torch.zeros((3, 4)), torch.zeros((3, 5), dtype=torch.int32), torch.zeros(5)):
        with pytest.raises(ValueError):
            pnc.rotated_boxes_to_warps(wrong, 8, 8)
    with pytest.raises(ValueError):
        pnc.rotated_boxes_to_warps(torch.zeros((3, 5)), 0, 8)


_DEV_KERNEL = re.compile(r"k_warp_dev<[017], [68]>")  # FC_NV12 = 0, FC_YUV420 = 1, FC_P16 = 7; FC_TENSOR = 6, FC_TENSOR_NHWC = 8


@pytest.mark.timeout(900)
def test_the_six_instantiations_use_no_scratch():
    """resource metadata of the code object only (tools/isa_stats.spills): both layouts of k_warp_dev for NV12, YUV420 and P10 / P12 hold the staged
    AND the per-tap form in one kernel — no scratch, no spills, at most 128 VGPRs (two workgroups of 256 lanes per SIMD)"""
    import isa_stats

    rows = [r for r in isa_stats.spills(os.path.join(ROOT, "videoprocessingframework_amd", "csrc", "k_convert_warp_dev.hip")) if _DEV_KERNEL.search(r[0])]
    assert len(rows) == 6, [r[0] for r in rows]
    assert len({r[0] for r in rows}) == 6
    for name, vgpr, vspill, sspill, scratch in rows:
        print(name[:100], "vgpr", vgpr)
        assert vspill == 0 and sspill == 0 and scratch == 0, (name, vgpr, vspill, sspill, scratch)
        assert vgpr <= 128, (name, vgpr)
