"""The fused multi-ROI perspective warp with the homographies in DEVICE memory (vpf_convert_persp_tensor_dev, vpf_persp_max_step,
PySurfaceConvertResizer.ExecutePerspsDevToTensor, PytorchNvCodec.device_persps_to_normalized_tensor, homographies_max_step,
quads_to_homographies_unchecked), without a GPU: the symbols, the header and the bindings exist, the structure has the declared layout, every
host-side refusal answers before any device work (fake pointers: nothing here may reach a launch), the Python entry raises ValueError where it says it
does, the Python hint is the C function, the unchecked solve equals the checked one on proper quads, and the six new kernel instantiations spill no
VGPR and use no scratch."""
import inspect
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from test_persp_tensor_cpu import NAMED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
NAME = "vpf_convert_persp_tensor_dev"


def test_symbols_header_and_bindings_exist(capi):
    for name in (NAME, "vpf_persp_max_step"):
        assert name in capi.EXPORTS and hasattr(capi.lib(), name)
    nm = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert f" {NAME}\n" in nm and " vpf_persp_max_step\n" in nm
    assert callable(capi.make_persps_dev) and callable(capi.convert_persp_tensor_dev) and callable(capi.persp_max_step)
    h = open(os.path.join(ROOT, "include", "vpf_hip.h")).read()
    for decl in ("typedef struct vpf_persps_dev", f"VPF_API vpf_status {NAME}(", "VPF_API float vpf_persp_max_step(const float m[9], vpf_size dst);"):
        assert h.index(decl) > h.index("VPF_API vpf_status vpf_convert_persp_tensor("), decl
        assert h.index(decl) > h.index("typedef struct vpf_frame_src"), decl
    sys.path.insert(0, os.path.join(ROOT, "videoprocessingframework_amd"))
    nvc = pytest.importorskip("PyNvCodec")
    assert hasattr(nvc.PySurfaceConvertResizer, "ExecutePerspsDevToTensor") and callable(nvc.PerspMaxStep)
    stub = open(os.path.join(ROOT, "videoprocessingframework_amd", "PyNvCodec", "__init__.pyi")).read()
    assert "def ExecutePerspsDevToTensor(self, surfaces: List[Surface], matrices_ptr: int, max_n: int, index_ptr: int, count_ptr: int, ptr: int, dtype: int" in stub
    assert "def PerspMaxStep(matrix: Sequence[float], dw: int, dh: int) -> float" in stub
    # the binding takes ExecuteWarpsDevToTensor's argument list
    doc_w, doc_p = nvc.PySurfaceConvertResizer.ExecuteWarpsDevToTensor.__doc__, nvc.PySurfaceConvertResizer.ExecutePerspsDevToTensor.__doc__
    sig = lambda d: re.sub(r"matrix_stride: [\w. |]+ = \d+", "matrix_stride", d.split("\n")[0].split("(", 1)[1])  # noqa: E731
    assert sig(doc_w) == sig(doc_p) and re.search(r"matrix_stride: [\w. |]+ = 36\b", doc_p)
    # the host-table entry still refuses device tensors, in its own words
    src = open(os.path.join(ROOT, "videoprocessingframework_amd", "PytorchNvCodec", "__init__.py")).read()
    assert "pass matrices.cpu()" in src


def test_python_signatures():
    torch = pytest.importorskip("torch")
    from videoprocessingframework_amd import PytorchNvCodec as pnc

    sig = inspect.signature(pnc.device_persps_to_normalized_tensor)
    assert sig == inspect.signature(pnc.device_warps_to_normalized_tensor)
    assert list(sig.parameters) == ["resizer", "surfaces", "matrices", "mean", "std", "surface_index", "count", "max_step", "dtype", "bgr", "border",
                                    "border_mode", "out", "cc_ctx", "channels_last"]
    d = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert d == dict(surface_index=None, count=None, max_step=None, dtype=torch.float32, bgr=False, border=(0, 0, 0), border_mode="constant", out=None,
                     cc_ctx=None, channels_last=False)
    assert list(inspect.signature(pnc.homographies_max_step).parameters) == ["matrices", "dw", "dh"]
    assert list(inspect.signature(pnc.quads_to_homographies_unchecked).parameters) == list(inspect.signature(pnc.quads_to_homographies).parameters) == ["quads", "size"]


def test_struct_layout(capi):
    """vpf_persps_dev: 96 bytes with no implicit padding, offsets 0 8 16 24 28 32 36 40 88 — vpf_warps_dev's; the header's field order is the ctypes
    order"""
    C = capi.C
    T = capi.PerspsDev
    assert C.sizeof(T) == 96 and sum(C.sizeof(t) for _, t in T._fields_) == 96
    names = ["matrices", "frame_index", "count", "matrix_stride", "frame_stride", "max_n", "max_step", "dst", "dst_job_stride"]
    assert [n for n, _ in T._fields_] == names
    assert [getattr(T, n).offset for n in names] == [0, 8, 16, 24, 28, 32, 36, 40, 88] == [getattr(capi.WarpsDev, n).offset for n in names]
    assert dict(T._fields_)["max_step"] is C.c_float and dict(T._fields_)["dst_job_stride"] is C.c_uint64
    h = open(os.path.join(ROOT, "include", "vpf_hip.h")).read()
    body = h[h.index("typedef struct vpf_persps_dev"):h.index("} vpf_persps_dev;")]
    declared = re.findall(r"^\s+(?:const )?\w+\*? (\w+)(?:\[3\])?;", body, re.M)   # the declarations, not the words of their comments
    assert declared == names
    t = capi.make_persps_dev(0x1000, 5, [(0x2000, 64), (0x3000, 64), (0x4000, 64)], 1536)
    assert (t.matrix_stride, t.frame_stride, t.max_n, t.max_step) == (36, 4, 5, 0.0)


def _norm(capi, dtype=0, flags=0, scale=(0.01, 0.01, 0.01), bias=(-1.0, -1.0, -1.0)):
    n = capi.TensorNorm()
    for c in range(3):
        n.scale[c], n.bias[c] = scale[c], bias[c]
    n.dtype, n.flags = dtype, flags
    return n


def test_validation_without_gpu(capi):
    """every host-side refusal of the warp-dev entry, with its status, before any device work: every pointer below is fake (matrices, frame indices and
    count included: the host never dereferences them)"""
    ex = capi.make_exec()
    W, H, dw, dh = 64, 32, 16, 8
    src = [(0x100000, 64), (0x200000, 64)]
    yuv = [(0x100000, 64), (0x200000, 32), (0x300000, 32)]
    f32 = [(0x400000, 64), (0x500000, 64), (0x600000, 64)]  # dw * 4 = 64
    f16 = [(0x400000, 32), (0x500000, 32), (0x600000, 32)]
    MAT, IDX, CNT = 0x700000, 0x780000, 0x800000

    def call(dst=f32, norm=None, sf=capi.NV12, cs=1, cr=0, frames=None, size=(W, H, dw, dh), mats=MAT, index=IDX, count=CNT, max_n=7, mstride=36, fstride=4,
             job=3 * 8 * 64, n_frames=None, max_step=0.0, opts=None):
        fr = capi.make_frame_srcs([src] if frames is None else frames)
        t = capi.make_persps_dev(mats, max_n, dst, job, index, count, mstride, fstride, max_step)
        return capi.convert_persp_tensor_dev(ex, sf, cs, cr, size[0], size[1], size[2], size[3], fr, t, _norm(capi) if norm is None else norm, opts,
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
    t = capi.make_persps_dev(MAT, 7, f32, 1536, IDX, CNT)
    assert capi.convert_persp_tensor_dev(ex, capi.NV12, 1, 0, W, H, dw, dh, fr, t, _norm(capi), check=False) == capi.ERR_BAD_ARG
    t.dst[2].reserved = 9
    assert capi.convert_persp_tensor_dev(ex, capi.NV12, 1, 0, W, H, dw, dh, capi.make_frame_srcs([src]), t, _norm(capi), check=False) == capi.ERR_BAD_ARG
    # null pointers: exec, the frames, the table, the parameters, the matrices, a plane
    L, Cb = capi.lib(), capi.C.byref
    fr, tb = capi.make_frame_srcs([src]), capi.make_persps_dev(MAT, 7, f32, 1536, IDX, CNT)
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
    # the table's fields
    assert call(n_frames=0) == capi.ERR_BAD_ARG
    assert call(frames=[src] * 129) == capi.ERR_BAD_ARG
    for max_n in (0, 65536, 0xFFFFFFFF):
        assert call(max_n=max_n) == capi.ERR_BAD_ARG, max_n
    for off in (1, 2, 3):
        assert call(mats=MAT + off) == capi.ERR_BAD_ARG, off
        assert call(index=IDX + off) == capi.ERR_BAD_ARG, off
        assert call(count=CNT + off) == capi.ERR_BAD_ARG, off
    for stride in (0, 4, 24, 32, 35, 37, 38, 39, 42):   # 24: the affine entry's stride is too short for nine floats
        assert call(mstride=stride) == capi.ERR_BAD_ARG, stride
    for stride in (0, 1, 2, 3, 5, 6, 7, 10):
        assert call(fstride=stride) == capi.ERR_BAD_ARG, stride
    for job in (1, 2, 3, 1537, 1538):
        assert call(job=job) == capi.ERR_BAD_ARG, job
    assert call(dst=f16, norm=_norm(capi, dtype=1), job=769) == capi.ERR_BAD_ARG
    for step in (-1.0, -1e-30, math.nan, math.inf, -math.inf):
        assert call(max_step=step) == capi.ERR_BAD_ARG, step
    with pytest.raises(capi.VpfError):
        capi.convert_persp_tensor_dev(ex, capi.NV12, 1, 0, W, H, dw, dh, capi.make_frame_srcs([src]), capi.make_persps_dev(MAT, 0, f32, 1536), _norm(capi))


class _Resizer:
    """stands in for PySurfaceConvertResizer: a ValueError must come before the resizer is asked to run"""

    def DstSize(self):
        return (16, 8)

    def Stream(self):
        raise AssertionError("validation must come first")

    def ExecutePerspsDevToTensor(self, *a, **k):
        raise AssertionError("validation must come first")


def test_python_value_errors():
    """device_persps_to_normalized_tensor: ValueError for host matrices, another dtype or shape (the affine entry's [K, 2, 3] and [K, 6] included), too
    many surfaces, a bad border, mode or hint — before the resizer runs; persps_to_normalized_tensor still refuses device tensors"""
    torch = pytest.importorskip("torch")
    from videoprocessingframework_amd import PytorchNvCodec as pnc

    rs, surfs, mean, std = _Resizer(), [object(), object()], (0, 0, 0), (1, 1, 1)
    host = torch.zeros((3, 3, 3), dtype=torch.float32)
    for m in (host, torch.zeros((3, 9)), [[[1, 0, 0], [0, 1, 0], [0, 0, 1]]], np.zeros((3, 3, 3), np.float32), None, torch.zeros((3, 3, 3), device="meta"),
              torch.zeros((3, 3, 3), dtype=torch.float64, device="meta"), torch.zeros((3, 2, 3), device="meta"), torch.zeros((3, 6), device="meta"),
              torch.zeros((3, 10), device="meta"), torch.zeros((9,), device="meta")):
        with pytest.raises(ValueError):
            pnc.device_persps_to_normalized_tensor(rs, surfs, m, mean, std)
    with pytest.raises(ValueError):
        pnc.device_persps_to_normalized_tensor(rs, surfs, host, mean, std, dtype=torch.float64)
    with pytest.raises(ValueError):
        pnc.device_persps_to_normalized_tensor(rs, [], host, mean, std)
    with pytest.raises(ValueError):
        pnc.device_persps_to_normalized_tensor(rs, [object()] * 129, host, mean, std)
    with pytest.raises(ValueError):
        pnc.device_persps_to_normalized_tensor(rs, surfs, host, mean, std, border_mode="reflect")
    with pytest.raises(ValueError):
        pnc.device_persps_to_normalized_tensor(rs, surfs, host, mean, std, border=(0, 0, 256))
    with pytest.raises(ValueError, match="device_persps_to_normalized_tensor: matrices must be a device tensor"):
        pnc.device_persps_to_normalized_tensor(rs, surfs, host, mean, std)
    with pytest.raises(ValueError, match=r"\.cpu\(\)"):
        pnc.persps_to_normalized_tensor(rs, surfs, [0, 0, 0], torch.zeros((3, 3, 3), device="meta"), mean, std)
    for bad in ([[1, 0, 0, 0, 1, 0]], torch.zeros((2, 3, 3), device="meta"), [[math.nan] * 9], [[2.0 ** 25] + [0] * 8]):
        with pytest.raises(ValueError):
            pnc.homographies_max_step(bad, 16, 8)
    for size in ((0, 8), (16, 0), (70000, 8), (1.5, 8)):
        with pytest.raises(ValueError):
            pnc.homographies_max_step(host, *size)


def test_homographies_max_step_is_the_c_function(capi):
    """per matrix vpf_persp_max_step (capi.persp_max_step), the maximum over the table, 0.0 as soon as one matrix has no bound; a last row (0, 0, 1)
    gives the affine hint; the C function answers 0 for what the entry would refuse"""
    torch = pytest.importorskip("torch")
    from videoprocessingframework_amd import PytorchNvCodec as pnc

    mats = [[float(np.float32(v)) for v in NAMED[k][0]] for k in ("keystone", "strong", "down-scale")]
    mats += [[1.5, -0.25, 10, 0.5, 2.0, -3, 0, 0, 1], [0.9, 0.1, 5, -0.1, 1.1, 7, 0.002, -0.001, 1.0], [2, 0, 0, 0, 2, 0, 0.001, 0.001, 0.5]]
    for dw, dh in ((61, 35), (64, 48), (112, 112)):
        each = [capi.persp_max_step(m, dw, dh) for m in mats]
        assert all(s > 0 for s in each), each
        assert pnc.homographies_max_step(mats, dw, dh) == max(each)
        assert pnc.homographies_max_step(torch.tensor(mats, dtype=torch.float64), dw, dh) == max(each)
        assert pnc.homographies_max_step(np.array(mats, np.float32).reshape(-1, 3, 3), dw, dh) == max(each)
        for k, m in enumerate(mats):
            assert pnc.homographies_max_step([m], dw, dh) == each[k]
        for unbounded in ("horizon", "behind"):
            bad = [float(np.float32(v)) for v in NAMED[unbounded][0]]
            assert capi.persp_max_step(bad, dw, dh) == 0.0
            assert pnc.homographies_max_step(mats + [bad], dw, dh) == 0.0 and pnc.homographies_max_step([bad] + mats, dw, dh) == 0.0
    assert pnc.homographies_max_step(np.zeros((0, 9), np.float32), 64, 48) == 0.0
    got = capi.persp_max_step([1.5, -0.25, 10, 0.5, 2.0, -3, 0, 0, 1], 64, 48)
    assert 2.5 <= got <= 2.5 * (1 + 2.0 ** -19)
    L = capi.lib()
    assert L.vpf_persp_max_step(None, capi.Size(64, 48)) == 0.0
    one = (capi.C.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    assert L.vpf_persp_max_step(one, capi.Size(0, 48)) == 0.0 and L.vpf_persp_max_step(one, capi.Size(64, 70000)) == 0.0
    for bad in (math.nan, math.inf, 2.0 ** 25):
        assert capi.persp_max_step([1, 0, 0, 0, 1, 0, 0, bad, 1], 64, 48) == 0.0


def test_quads_to_homographies_unchecked_equals_checked_on_proper_quads():
    """quads_to_homographies_unchecked goes through torch.linalg.solve_ex(..., check_errors=False): the same LU factorisation, so the same tensor for
    proper quads; a degenerate quad raises nothing (its matrix is whatever the factorisation gives); quads_to_homographies itself is unchanged"""
    torch = pytest.importorskip("torch")
    from videoprocessingframework_amd import PytorchNvCodec as pnc

    rng = np.random.default_rng(2330)
    quads = []
    for _ in range(200):
        cx, cy, r = rng.uniform(100, 1800), rng.uniform(100, 1000), rng.uniform(20, 300)
        a0 = rng.uniform(0, 2 * math.pi)
        ang = [a0 + k * math.pi / 2 + rng.uniform(-0.4, 0.4) for k in range(4)]
        quads.append([[cx + r * rng.uniform(0.7, 1.3) * math.cos(a), cy + r * rng.uniform(0.7, 1.3) * math.sin(a)] for a in ang])
    q = torch.tensor(quads, dtype=torch.float64)
    for size in ((61, 35), (112, 112), (2, 2)):
        a, b = pnc.quads_to_homographies(q, size), pnc.quads_to_homographies_unchecked(q, size)
        assert a.dtype == b.dtype == torch.float32 and tuple(a.shape) == tuple(b.shape) == (200, 3, 3)
        assert torch.equal(a, b)
        assert bool(torch.isfinite(a).all())
    line = torch.tensor([[[0.0, 0.0], [10.0, 0.0], [20.0, 0.0], [30.0, 0.0]]], dtype=torch.float64)   # four corners on a line
    out = pnc.quads_to_homographies_unchecked(line, (16, 8))
    assert tuple(out.shape) == (1, 3, 3) and out.dtype == torch.float32
    assert tuple(pnc.quads_to_homographies_unchecked(torch.zeros((0, 4, 2)), (16, 8)).shape) == (0, 3, 3)
    for wrong in (torch.zeros((3, 4, 3)), torch.zeros((4, 2))):
        with pytest.raises(ValueError, match="quads_to_homographies_unchecked"):
            pnc.quads_to_homographies_unchecked(wrong, (16, 8))
    with pytest.raises(ValueError):
        pnc.quads_to_homographies_unchecked(torch.zeros((1, 4, 2)), (1, 8))
    assert "solve_ex(a, b, check_errors=False)" in inspect.getsource(pnc._quads_to_homographies)


_DEV_KERNEL = re.compile(r"k_persp_dev<[017], [68]>")  # FC_NV12 = 0, FC_YUV420 = 1, FC_P16 = 7; FC_TENSOR = 6, FC_TENSOR_NHWC = 8


@pytest.mark.timeout(900)
def test_the_six_instantiations_spill_no_vgpr_and_use_no_scratch():
    """resource metadata of the code object only (tools/isa_stats.spills): both layouts of k_persp_dev for NV12, YUV420 and P10 / P12 hold the staged
    AND the per-tap form in one kernel — no VGPR spill, no scratch, at most 128 VGPRs (two workgroups of 256 lanes per SIMD).  Scalar spills (nine
    wave-uniform floats beside the frame's planes) go to VGPR lanes and are printed, not bounded"""
    import isa_stats

    rows = [r for r in isa_stats.spills(os.path.join(ROOT, "videoprocessingframework_amd", "csrc", "k_convert_persp_dev.hip")) if _DEV_KERNEL.search(r[0])]
    assert len(rows) == 6, [r[0] for r in rows]
    assert len({r[0] for r in rows}) == 6
    for name, vgpr, vspill, sspill, scratch in rows:
        print(name[:100], "vgpr", vgpr, "spilled sgprs", sspill)
        assert vspill == 0 and scratch == 0, (name, vgpr, vspill, sspill, scratch)
        assert vgpr <= 128, (name, vgpr)
