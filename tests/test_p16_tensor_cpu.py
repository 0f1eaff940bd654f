"""P10 / P12 sources of the fused tensor entries (vpf_convert_resize_tensor(_batch), vpf_convert_resize_tensor_rois, vpf_convert_warp_tensor and
PySurfaceConvertResizer on top of them), without a GPU: the premise of tests/test_gpu_p16_tensor.py (the oracle's P10 -> NV12 is
min(255, (v + 128) >> 8) on the samples that sit on its rounding and saturation edges), every validation rule of the 16-bit sources before any
device work (fake pointers: nothing here may reach a launch), the answers that must NOT change (vpf_convert_supported, the 8-bit fused entries,
vpf_resize, vpf_tensor_convert), the Task layer's construction and refusal rules, and the register metadata of the new kernel instantiations."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

PLANTED = [0x007F, 0x0080, 0x017F, 0x0180, 0xFF7F, 0xFF80, 0xFFFF]
PLANTED_8 = [0, 1, 1, 2, 255, 255, 255]


def plant(planes):
    """the samples on the edges of (v + 128) >> 8 and of its saturation, in luma and in both chroma components: at the start of the first row and
    the end of the last one (running over into the neighbouring rows of pictures narrower than seven samples).  In place; -> planes"""
    y, uv = (p.reshape(-1) for p in planes)  # views: the planes are C-contiguous
    n = len(PLANTED)
    y[:n] = PLANTED
    y[-n:] = PLANTED
    uv[0:2 * n:2] = PLANTED          # U
    uv[1:2 * n:2] = PLANTED          # V
    uv[-2 * n::2] = PLANTED
    uv[-2 * n + 1::2] = PLANTED[::-1]
    return planes


@pytest.mark.parametrize("fmt", ["P10", "P12"])
def test_oracle_premise_on_the_planted_samples(oracle, fmt):
    W, H = 34, 6
    src = plant(oracle.synth(getattr(oracle, fmt), W, H, 4100))
    st, nv = oracle.convert(getattr(oracle, fmt), oracle.NV12, 0, 0, W, H, src, oracle.FP32)
    assert st == 0
    n = len(PLANTED)
    assert nv[0][0, :n].tolist() == PLANTED_8 and nv[0][-1, -n:].tolist() == PLANTED_8
    assert nv[1][0, 0:2 * n:2].tolist() == PLANTED_8 and nv[1][0, 1:2 * n:2].tolist() == PLANTED_8
    assert nv[1][-1, -2 * n::2].tolist() == PLANTED_8 and nv[1][-1, -2 * n + 1::2].tolist() == PLANTED_8[::-1]
    for p16, p8 in zip(src, nv):  # and the whole frame: the definition, sample by sample
        want = np.minimum(255, (p16.astype(np.uint32) + 128) >> 8).astype(np.uint8)
        assert np.array_equal(p8, want)


def _norm(capi, dtype=0):
    n = capi.TensorNorm()
    for c in range(3):
        n.scale[c], n.bias[c] = 0.01, -1.0
    n.dtype, n.flags = dtype, 0
    return n


W, H, DW, DH = 64, 32, 16, 8
DST = [(0x400000, 64), (0x500000, 64), (0x600000, 64)]  # f32: dw * 4 = 64
ENTRIES = ["tensor", "tensor_batch", "rois", "warps"]


def _call(capi, entry, sf, src, cs=1, cr=0):
    ex = capi.make_exec()
    if entry == "tensor":
        return capi.convert_resize_tensor(ex, sf, cs, cr, W, H, src, DW, DH, DST, _norm(capi), check=False)
    if entry == "tensor_batch":
        return capi.convert_resize_tensor_batch(ex, sf, cs, cr, W, H, DW, DH, capi.make_batch([(src, DST)] * 2), _norm(capi), check=False)
    if entry == "rois":
        return capi.convert_resize_tensor_rois(ex, sf, cs, cr, W, H, DW, DH, capi.make_rois([(src, DST, (3, 5, 20, 10))]), _norm(capi), check=False)
    return capi.convert_warp_tensor(ex, sf, cs, cr, W, H, DW, DH, capi.make_warps([(src, DST, (1, 0, 3, 0, 1, 5))]), _norm(capi), check=False)


@pytest.mark.parametrize("fmt", ["P10", "P12"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_validation_of_16_bit_sources_without_gpu(capi, entry, fmt):
    """every rule of the 16-bit sources answers before any device access (the pointers are fake).  At the parent every one of these calls answered
    UNSUPPORTED."""
    sf = getattr(capi, fmt)
    good = [(0x100000, 2 * W), (0x200000, 2 * W)]  # luma: 2 W bytes per row; chroma: 4 ceil(W / 2) = 2 W
    for k in range(2):
        p = list(good)
        p[k] = (good[k][0] + 1, good[k][1])
        assert _call(capi, entry, sf, p) == capi.ERR_BAD_ARG, (k, "odd pointer")
        p[k] = (good[k][0], good[k][1] + 1)
        assert _call(capi, entry, sf, p) == capi.ERR_BAD_ARG, (k, "odd pitch")
        p[k] = (good[k][0], 2 * W - 2)
        assert _call(capi, entry, sf, p) == capi.ERR_BAD_ARG, (k, "short pitch")
        p[k] = (good[k][0], W)  # an 8-bit row's bytes
        assert _call(capi, entry, sf, p) == capi.ERR_BAD_ARG, (k, "the pitch of an 8-bit row")
        p[k] = (0, good[k][1])
        assert _call(capi, entry, sf, p) == capi.ERR_BAD_ARG, (k, "null")
    assert _call(capi, entry, sf, good, cs=2) == capi.ERR_UNSUPPORTED
    assert _call(capi, entry, sf, good, cr=2) == capi.ERR_UNSUPPORTED
    # an otherwise valid call gets as far as the identical NV12 call (same planes, read as 8-bit rows of the same pitch)
    assert _call(capi, entry, sf, good) == _call(capi, entry, capi.NV12, good)
    if capi.device_count() == 0:
        assert _call(capi, entry, sf, good) not in (capi.OK, capi.ERR_UNSUPPORTED, capi.ERR_BAD_ARG)
    # a 2-B aligned pitch that is no multiple of 4 or 16 is legal (the gather and the per-job kernels take any 2-B alignment)
    odd2 = [(0x100002, 2 * W + 2), (0x200006, 2 * W + 6)]
    assert _call(capi, entry, sf, odd2) == _call(capi, entry, capi.NV12, good)


def test_odd_width_chroma_pitch(capi):
    """W = 63: luma rows hold 126 bytes, chroma rows 4 ceil(63 / 2) = 128"""
    ex = capi.make_exec()
    for luma, chroma, bad in ((126, 128, False), (124, 128, True), (126, 126, True)):
        st = capi.convert_resize_tensor(ex, capi.P10, 1, 0, 63, 32, [(0x100000, luma), (0x200000, chroma)], DW, DH, DST, _norm(capi), check=False)
        assert (st == capi.ERR_BAD_ARG) == bad, (luma, chroma, st)


def test_unchanged_answers(capi):
    """what does NOT accept P10 / P12, exactly as before"""
    for df in (capi.RGB, capi.BGR, capi.RGB_PLANAR):
        for cs in (0, 1):
            for cr in (0, 1):
                assert capi.convert_supported(capi.P10, df, cs, cr) == 0
                assert capi.convert_supported(capi.P12, df, cs, cr) == 0
    assert capi.convert_supported(capi.P10, capi.NV12, 0, 0) and capi.convert_supported(capi.P12, capi.NV12, 0, 0)
    ex = capi.make_exec()
    src = [(0x100000, 2 * W), (0x200000, 2 * W)]
    rgb = [(0x400000, 3 * DW)]
    for sf in (capi.P10, capi.P12):
        assert capi.convert_resize(ex, sf, capi.RGB, 1, 0, W, H, src, DW, DH, rgb, check=False) == capi.ERR_UNSUPPORTED
        assert capi.convert_resize_batch(ex, sf, capi.RGB_PLANAR, 1, 0, W, H, DW, DH, capi.make_batch([(src, DST)]), check=False) == capi.ERR_UNSUPPORTED
        assert capi.convert(ex, sf, capi.RGB, 1, 0, W, H, src, rgb, check=False) == capi.ERR_UNSUPPORTED
        assert capi.resize(ex, sf, 1, W, H, src, DW, DH, src, check=False) == capi.ERR_UNSUPPORTED
        assert not capi.tensor_convert_supported(sf, 0, 1)
        assert capi.tensor_convert(ex, sf, 0, 1, W, H, DST, src, _norm(capi), check=False) == capi.ERR_UNSUPPORTED
    # and the sources the tensor entries never took still answer UNSUPPORTED there
    for sf in (capi.RGB, capi.YUV444, capi.Y, capi.YUV422):
        for entry in ENTRIES:
            assert _call(capi, entry, sf, src) == capi.ERR_UNSUPPORTED, (sf, entry)


def test_task_layer_construction_and_refusals(capfd):
    sys.path.insert(0, os.path.join(ROOT, "videoprocessingframework_amd"))
    nvc = pytest.importorskip("PyNvCodec")
    PF = nvc.PixelFormat
    nvc._UseHostAllocator(True)
    try:
        for s in ("P10", "P12"):
            for d in ("RGB", "BGR", "RGB_PLANAR"):
                f = nvc.PySurfaceConvertResizer(64, 32, getattr(PF, s), 32, 16, getattr(PF, d), 0, 0)
                assert f.Format() == getattr(PF, d) and f.DstSize() == (32, 16)
        for s, d in (("P10", "NV12"), ("P10", "Y"), ("P12", "NV12"), ("P10", "YUV420"), ("P10", "P10")):
            with pytest.raises(ValueError, match="Unsupported fused conversion"):
                nvc.PySurfaceConvertResizer(64, 32, getattr(PF, s), 32, 16, getattr(PF, d), 0, 0)
        f = nvc.PySurfaceConvertResizer(64, 32, PF.P10, 32, 16, PF.RGB_PLANAR, 0, 0)
        surf = nvc.Surface.Make(PF.P10, 64, 32, context=0)
        capfd.readouterr()
        assert f.Execute(surf, None).Empty()
        assert "8-bit outputs take 8-bit sources" in capfd.readouterr().err
        dst = nvc.Surface.Make(PF.RGB_PLANAR, 32, 16, context=0)
        assert not f.ExecuteBatch([surf], [dst], None)
        assert "8-bit outputs take 8-bit sources" in capfd.readouterr().err
        # the tensor entry of a P10 task takes P10 surfaces only, of the task's size
        mean, std = [0.5] * 3, [0.5] * 3
        assert not f.ExecuteToTensor([nvc.Surface.Make(PF.NV12, 64, 32, context=0)], 0x400000, 0, mean, std)
        assert not f.ExecuteToTensor([nvc.Surface.Make(PF.P12, 64, 32, context=0)], 0x400000, 0, mean, std)
        assert not f.ExecuteToTensor([nvc.Surface.Make(PF.P10, 32, 32, context=0)], 0x400000, 0, mean, std)
        assert not f.ExecuteRoisToTensor([nvc.Surface.Make(PF.NV12, 64, 32, context=0)], [(0, 0, 0, 8, 8)], 0x400000, 0, mean, std)
        assert not f.ExecuteWarpsToTensor([nvc.Surface.Make(PF.NV12, 64, 32, context=0)], [0], [(1, 0, 0, 0, 1, 0)], 0x400000, 0, mean, std)
        # the colour-context rule is the NV12 pair's: BT.601 MPEG is refused unless the extended colour spaces are on
        nvc.SetExtendedColorspaces(False)
        capfd.readouterr()
        assert not f.ExecuteToTensor([surf], 0x400000, 0, mean, std, nvc.ColorspaceConversionContext(nvc.ColorSpace.BT_601, nvc.ColorRange.MPEG))
        assert "Rec. 601 NV12 -> RGB MPEG range conversion isn't supported yet." in capfd.readouterr().err
        stub = open(os.path.join(ROOT, "videoprocessingframework_amd", "PyNvCodec", "__init__.pyi")).read()
        assert "P10 / P12" in stub[stub.index("class PySurfaceConvertResizer"):stub.index("class PyTensorToSurface")]
    finally:
        nvc._UseHostAllocator(False)


_P16_KERNEL = re.compile(r"k_convert_half<7, 6,|k_convert_strip_wg<7, 6,|k_convert_resize<7, 6,|k_roi_(strip|gather)<7, 6>|k_warp_(strip|gather)<7, 6>")  # FC_P16 = 7, FC_TENSOR = 6


@pytest.mark.timeout(900)
@pytest.mark.parametrize("tu,count", [("k_convert_resize.hip", 12), ("k_convert_roi.hip", 2), ("k_convert_warp.hip", 2)])
def test_no_16_bit_instantiation_spills(tu, count):
    """resource metadata of the code object only (tools/isa_stats.spills): the instantiations with the 16-bit source class — the half kernel, the
    four band heights of the workgroup strip and the gather form, each with both frame tables; the staged and gather forms of the ROI and warp
    kernels — use no scratch and spill nothing"""
    import isa_stats

    rows = [r for r in isa_stats.spills(os.path.join(ROOT, "videoprocessingframework_amd", "csrc", tu)) if _P16_KERNEL.search(r[0])]
    assert len(rows) == count, [r[0] for r in rows]
    for name, vgpr, vspill, sspill, scratch in rows:
        print(name[:100], "vgpr", vgpr)
        assert vspill == 0 and sspill == 0 and scratch == 0, (name, vgpr, vspill, sspill, scratch)
        assert vgpr <= 128, (name, vgpr)  # two workgroups of 256 lanes per SIMD at least, like the 8-bit instantiations
