"""The fused multi-ROI crop + resize with the rectangles in DEVICE memory (vpf_convert_resize_tensor_rois_dev, PySurfaceConvertResizer.ExecuteRoisDevToTensor,
PytorchNvCodec.device_rois_to_normalized_tensor, PytorchNvCodec.boxes_to_rois), without a GPU: the symbol, the header and the bindings exist, the
structures have the declared layout, every host-side refusal answers before any device work (fake pointers: nothing here may reach a launch), the
Python entry raises ValueError where it says it does, boxes_to_rois is its exact-integer definition, and the six new kernel instantiations use no
scratch and at most 128 VGPRs."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
NAME = "vpf_convert_resize_tensor_rois_dev"


def test_symbol_header_and_bindings_exist(capi):
    assert NAME in capi.EXPORTS and hasattr(capi.lib(), NAME)
    nm = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert f" {NAME}\n" in nm
    assert callable(capi.make_rois_dev) and callable(capi.convert_resize_tensor_rois_dev) and callable(capi.make_frame_srcs)
    h = open(os.path.join(ROOT, "include", "vpf_hip.h")).read()
    for decl in ("typedef struct vpf_roi_dev", "typedef struct vpf_frame_src", "typedef struct vpf_rois_dev", f"VPF_API vpf_status {NAME}("):
        assert h.index(decl) > h.index("VPF_API vpf_status vpf_convert_resize_tensor_rois("), decl
    sys.path.insert(0, os.path.join(ROOT, "videoprocessingframework_amd"))
    nvc = pytest.importorskip("PyNvCodec")
    assert hasattr(nvc.PySurfaceConvertResizer, "ExecuteRoisDevToTensor")
    stub = open(os.path.join(ROOT, "videoprocessingframework_amd", "PyNvCodec", "__init__.pyi")).read()
    assert "def ExecuteRoisDevToTensor(self, surfaces: List[Surface], boxes_ptr: int, max_n: int, count_ptr: int, ptr: int, dtype: int" in stub
    src = open(os.path.join(ROOT, "videoprocessingframework_amd", "PytorchNvCodec", "__init__.py")).read()
    assert "def device_rois_to_normalized_tensor(resizer, surfaces, boxes, mean, std, count=None, dtype=torch.float32, bgr=False, out=None, cc_ctx=None,\n" in src
    assert "def boxes_to_rois(boxes_xyxy, frame_index, width, height)" in src
    # the host-table entry still refuses device tensors, in its own words
    assert "pass rois.cpu()" in src


def test_struct_layout(capi):
    """vpf_roi_dev: 20 bytes, a row of an int32 [K, 5] tensor; vpf_frame_src: 48; vpf_rois_dev: 80 with no implicit padding"""
    C = capi.C
    assert C.sizeof(capi.RoiDev) == 20 and [n for n, _ in capi.RoiDev._fields_] == ["frame", "x", "y", "width", "height"]
    assert all(t is C.c_int32 for _, t in capi.RoiDev._fields_)
    assert C.sizeof(capi.FrameSrc) == 48 and capi.FrameSrc.src.offset == 0
    T = capi.RoisDev
    assert C.sizeof(T) == 80 and sum(C.sizeof(t) for _, t in T._fields_) == 80
    assert (T.boxes.offset, T.count.offset, T.box_stride.offset, T.max_n.offset, T.dst.offset, T.dst_job_stride.offset) == (0, 8, 16, 20, 24, 72)
    h = open(os.path.join(ROOT, "include", "vpf_hip.h")).read()
    body = h[h.index("typedef struct vpf_rois_dev"):h.index("} vpf_rois_dev;")]
    order = [body.index(f) for f in ("boxes;", "count;", "box_stride;", "max_n;", "dst[3];", "dst_job_stride;")]
    assert order == sorted(order)


def _norm(capi, dtype=0, flags=0, scale=(0.01, 0.01, 0.01), bias=(-1.0, -1.0, -1.0)):
    n = capi.TensorNorm()
    for c in range(3):
        n.scale[c], n.bias[c] = scale[c], bias[c]
    n.dtype, n.flags = dtype, flags
    return n


def test_validation_without_gpu(capi):
    """every host-side refusal, before any device work: every pointer below is fake (boxes and count included: the host never dereferences them)"""
    ex = capi.make_exec()
    W, H, dw, dh = 64, 32, 16, 8
    src = [(0x100000, 64), (0x200000, 64)]
    yuv = [(0x100000, 64), (0x200000, 32), (0x300000, 32)]
    f32 = [(0x400000, 64), (0x500000, 64), (0x600000, 64)]  # dw * 4 = 64
    f16 = [(0x400000, 32), (0x500000, 32), (0x600000, 32)]
    BOX, CNT = 0x700000, 0x800000

    def call(dst=f32, norm=None, sf=capi.NV12, cs=1, cr=0, frames=None, size=(W, H, dw, dh), boxes=BOX, count=CNT, max_n=7, stride=20, job=3 * 8 * 64,
             n_frames=None):
        fr = capi.make_frame_srcs([src] if frames is None else frames)
        t = capi.make_rois_dev(boxes, max_n, dst, job, count, stride)
        return capi.convert_resize_tensor_rois_dev(ex, sf, cs, cr, size[0], size[1], size[2], size[3], fr, t, _norm(capi) if norm is None else norm,
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
    # null pointers: exec, the frames, the table, the parameters, the boxes, a plane
    L, Cb = capi.lib(), capi.C.byref
    fr, tb = capi.make_frame_srcs([src]), capi.make_rois_dev(BOX, 7, f32, 1536, CNT)
    args = (capi.NV12, 1, 0, capi.Size(W, H), capi.Size(dw, dh), 1)
    assert getattr(L, NAME)(None, *args, fr, Cb(tb), Cb(_norm(capi))) == capi.ERR_BAD_ARG
    assert getattr(L, NAME)(Cb(ex), *args, None, Cb(tb), Cb(_norm(capi))) == capi.ERR_BAD_ARG
    assert getattr(L, NAME)(Cb(ex), *args, fr, None, Cb(_norm(capi))) == capi.ERR_BAD_ARG
    assert getattr(L, NAME)(Cb(ex), *args, fr, Cb(tb), None) == capi.ERR_BAD_ARG
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
    # the new fields
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
    with pytest.raises(capi.VpfError):
        capi.convert_resize_tensor_rois_dev(ex, capi.NV12, 1, 0, W, H, dw, dh, capi.make_frame_srcs([src]), capi.make_rois_dev(BOX, 0, f32, 1536), _norm(capi))


class _Resizer:
    """stands in for PySurfaceConvertResizer: a ValueError must come before the resizer is asked to run"""

    def DstSize(self):
        return (16, 8)

    def Stream(self):
        raise AssertionError("validation must come first")

    def ExecuteRoisDevToTensor(self, *a, **k):
        raise AssertionError("validation must come first")


def test_python_value_errors():
    """device_rois_to_normalized_tensor: ValueError for host boxes, another dtype or shape, a host count, too many surfaces — before the resizer runs;
    rois_to_normalized_tensor still refuses device boxes"""
    torch = pytest.importorskip("torch")
    from videoprocessingframework_amd import PytorchNvCodec as pnc

    rs, surfs, mean, std = _Resizer(), [object(), object()], (0, 0, 0), (1, 1, 1)
    for boxes in (torch.zeros((3, 5), dtype=torch.int32), [(0, 0, 0, 8, 8)], np.zeros((3, 5), np.int32), None,
                  torch.zeros((3, 5), dtype=torch.int32, device="meta")):
        with pytest.raises(ValueError):
            pnc.device_rois_to_normalized_tensor(rs, surfs, boxes, mean, std)
    with pytest.raises(ValueError):
        pnc.device_rois_to_normalized_tensor(rs, surfs, torch.zeros((3, 5), dtype=torch.int32), mean, std, dtype=torch.float64)
    with pytest.raises(ValueError):
        pnc.device_rois_to_normalized_tensor(rs, [], torch.zeros((3, 5), dtype=torch.int32), mean, std)
    with pytest.raises(ValueError):
        pnc.device_rois_to_normalized_tensor(rs, [object()] * 129, torch.zeros((3, 5), dtype=torch.int32), mean, std)


def _rois_exact(boxes, frames, W, H):
    """boxes_to_rois restated on Python numbers: math.floor / math.ceil of a float are exact integers"""
    out = []
    for (x1, y1, x2, y2), f in zip(boxes, frames):
        if any(math.isnan(v) for v in (x1, y1, x2, y2)):
            fl = lambda v, hi: 0 if math.isnan(v) else (min(max(math.floor(v), 0), hi) if math.isfinite(v) else (hi if v > 0 else 0))
            out.append((f, fl(x1, W - 1), fl(y1, H - 1), 0, 0))
            continue

        def lo(v, hi):
            return (hi if v > 0 else 0) if math.isinf(v) else min(max(math.floor(v), 0), hi)

        def up(v, a, b):
            c = (b if v > 0 else a) if math.isinf(v) else math.ceil(v)
            return min(max(c, a), b)

        x, y = lo(x1, W - 1), lo(y1, H - 1)
        out.append((f, x, y, up(x2, x + 1, W) - x, up(y2, y + 1, H) - y))
    return out


def test_boxes_to_rois_is_its_integer_definition():
    torch = pytest.importorskip("torch")
    from videoprocessingframework_amd import PytorchNvCodec as pnc

    W, H = 131, 79
    nan, inf = math.nan, math.inf
    boxes = [(0.0, 0.0, 131.0, 79.0), (17.0, 9.0, 72.0, 50.0),            # already integral
             (17.3, 9.9, 71.2, 49.01), (0.5, 0.5, 0.6, 0.6),              # rounded outwards; inside one pixel
             (-5.5, -0.1, 10.2, 3.0), (-50.0, -60.0, -3.0, -2.0),         # negative: clipped; wholly left / above: one pixel at the edge
             (120.0, 70.0, 140.7, 90.0), (200.0, 100.0, 300.0, 120.0),    # past the edge; wholly outside
             (130.0, 78.0, 131.0, 79.0), (130.9, 78.9, 131.0, 79.0), (131.0, 79.0, 135.0, 85.0),
             (50.0, 40.0, 50.0, 40.0), (60.0, 30.0, 20.0, 10.0),          # empty and inverted boxes: one pixel
             (nan, 0.0, 10.0, 10.0), (0.0, nan, 10.0, 10.0), (0.0, 0.0, nan, 10.0), (0.0, 0.0, 10.0, nan), (nan, nan, nan, nan),
             (-inf, -inf, inf, inf), (inf, 3.0, inf, 7.0), (1e30, -1e30, 3e38, 5.0)]
    rng = np.random.default_rng(7)
    boxes += [(float(rng.uniform(-20, 160)), float(rng.uniform(-20, 100)), float(rng.uniform(-20, 160)), float(rng.uniform(-20, 100))) for _ in range(300)]
    frames = [i % 3 for i in range(len(boxes))]
    want = _rois_exact(boxes, frames, W, H)
    for dt in (torch.float32, torch.float64):
        b = torch.tensor(boxes, dtype=dt)
        exact = _rois_exact(b.tolist(), frames, W, H) if dt == torch.float32 else want   # (float32 rounds the inputs first)
        for fi in (torch.tensor(frames, dtype=torch.int64), torch.tensor(frames, dtype=torch.int32), frames):
            got = pnc.boxes_to_rois(b, fi, W, H)
            assert got.dtype == torch.int32 and tuple(got.shape) == (len(boxes), 5) and got.device.type == "cpu"
            assert got.tolist() == [list(r) for r in exact]
    got = np.array(want)
    valid = got[:, 3] > 0
    assert (got[~valid][:, 3:] == 0).all() and int((~valid).sum()) == 5                   # NaN: w = h = 0, an invalid box
    v = got[valid]
    assert (v[:, 1] >= 0).all() and (v[:, 2] >= 0).all() and (v[:, 3] >= 1).all() and (v[:, 4] >= 1).all()
    assert (v[:, 1] + v[:, 3] <= W).all() and (v[:, 2] + v[:, 4] <= H).all()
    assert want[0] == (0, 0, 0, 131, 79) and want[2] == (2, 17, 9, 55, 41) and want[3] == (0, 0, 0, 1, 1) and want[5] == (2, 0, 0, 1, 1)
    assert want[7] == (1, 130, 78, 1, 1) and want[12] == (0, 60, 30, 1, 1)
    assert tuple(pnc.boxes_to_rois(torch.zeros((0, 4)), torch.zeros((0,), dtype=torch.int64), W, H).shape) == (0, 5)
    for bad in (torch.zeros((3, 5)), torch.zeros((3, 4), dtype=torch.int32), torch.zeros(4)):
        with pytest.raises(ValueError):
            pnc.boxes_to_rois(bad, [0, 0, 0], W, H)
    with pytest.raises(ValueError):
        pnc.boxes_to_rois(torch.zeros((3, 4)), torch.zeros(3), W, H)          # float frame indices
    with pytest.raises(ValueError):
        pnc.boxes_to_rois(torch.zeros((3, 4)), [0, 0], W, H)


_DEV_KERNEL = re.compile(r"k_roi_dev<[017], [68]>")  # FC_NV12 = 0, FC_YUV420 = 1, FC_P16 = 7; FC_TENSOR = 6, FC_TENSOR_NHWC = 8


@pytest.mark.timeout(900)
def test_the_six_instantiations_use_no_scratch():
    """resource metadata of the code object only (tools/isa_stats.spills): both layouts of k_roi_dev for NV12, YUV420 and P10 / P12 hold the staged
    AND the per-tap form in one kernel — no scratch, no spills, at most 128 VGPRs (two workgroups of 256 lanes per SIMD)"""
    import isa_stats

    rows = [r for r in isa_stats.spills(os.path.join(ROOT, "videoprocessingframework_amd", "csrc", "k_convert_roi_dev.hip")) if _DEV_KERNEL.search(r[0])]
    assert len(rows) == 6, [r[0] for r in rows]
    assert len({r[0] for r in rows}) == 6
    for name, vgpr, vspill, sspill, scratch in rows:
        print(name[:100], "vgpr", vgpr)
        assert vspill == 0 and sspill == 0 and scratch == 0, (name, vgpr, vspill, sspill, scratch)
        assert vgpr <= 128, (name, vgpr)
