"""Channels-last (NHWC) tensors in the fused tensor entries (VPF_TENSOR_NHWC, include/vpf_hip.h), without a GPU: the flag's validation rules in
the six entries answer before any device work (fake pointers: nothing here may reach a launch; the one call per entry that passes validation names
a device that does not exist, so it ends at VPF_ERR_NO_DEVICE), the Python layer refuses strides that are not torch.channels_last, and the
channels-last kernel instantiations use no scratch, spill nothing and stay within 128 VGPRs.

Definition: with the flag, dst[0] (src[0] on the way back) is the ONE interleaved plane of a frame or job, element (y, x, c) at
ptr + y * pitch + (3 x + c) * elem; dst[1..2] are ignored; ptr and pitch are multiples of elem and pitch >= 3 * width * elem."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

SW, SH, DW, DH = 64, 32, 16, 8
SRC = [(0x100000, 64), (0x200000, 64)]       # NV12 planes of the 64 x 32 source (fake)
NV12_OUT = [(0x100000, 16), (0x200000, 16)]  # NV12 planes of a 16 x 8 destination (fake)
NO_GPU = 1 << 20                              # a device index no machine has: a call that passes validation stops at the device switch


def _norm(capi, dtype, flags):
    n = capi.TensorNorm()
    for c in range(3):
        n.scale[c], n.bias[c] = 0.01, -1.0
    n.dtype, n.flags = dtype, flags
    return n


def _entries(capi):
    """name -> call(plane_list, norm, device) for the six entries; plane_list = the tensor planes of the one frame / job (dst, or src on the way back)"""
    def ex(dev):
        return capi.make_exec(device=dev)

    def single(p, n, dev=-1):
        return capi.convert_resize_tensor(ex(dev), capi.NV12, 1, 0, SW, SH, SRC, DW, DH, p, n, check=False)

    def batch(p, n, dev=-1):
        return capi.convert_resize_tensor_batch(ex(dev), capi.NV12, 1, 0, SW, SH, DW, DH, capi.make_batch([(SRC, p)] * 2), n, check=False)

    def rois(p, n, dev=-1):
        return capi.convert_resize_tensor_rois(ex(dev), capi.NV12, 1, 0, SW, SH, DW, DH, capi.make_rois([(SRC, p, (3, 1, 20, 10))]), n, check=False)

    def warps(p, n, dev=-1):
        return capi.convert_warp_tensor(ex(dev), capi.NV12, 1, 0, SW, SH, DW, DH, capi.make_warps([(SRC, p, (1, 0, 0, 0, 1, 0))]), n,
                                        capi.make_warp_opts(capi.WARP_CONSTANT, (1, 2, 3)), check=False)

    def back(p, n, dev=-1):
        return capi.tensor_convert(ex(dev), capi.NV12, 0, 1, DW, DH, p, NV12_OUT, n, check=False)

    def back_batch(p, n, dev=-1):
        return capi.tensor_convert_batch(ex(dev), capi.NV12, 0, 1, DW, DH, capi.make_batch([(p, NV12_OUT)] * 2), n, check=False)

    return {"vpf_convert_resize_tensor": single, "vpf_convert_resize_tensor_batch": batch, "vpf_convert_resize_tensor_rois": rois,
            "vpf_convert_warp_tensor": warps, "vpf_tensor_convert": back, "vpf_tensor_convert_batch": back_batch}


ENTRY_NAMES = ["vpf_convert_resize_tensor", "vpf_convert_resize_tensor_batch", "vpf_convert_resize_tensor_rois", "vpf_convert_warp_tensor",
               "vpf_tensor_convert", "vpf_tensor_convert_batch"]


def test_flag_value(capi):
    assert capi.TENSOR_NHWC == 4 and capi.TENSOR_BGR == 1
    h = open(os.path.join(ROOT, "include", "vpf_hip.h")).read()
    assert re.search(r"#define\s+VPF_TENSOR_NHWC\s+4u", h)
    assert capi.make_tensor_norm((0, 0, 0), (1, 1, 1), nhwc=True).flags == 4
    assert capi.make_tensor_norm((0, 0, 0), (1, 1, 1), bgr=True, nhwc=True).flags == 5
    assert capi.make_tensor_denorm((0, 0, 0), (1, 1, 1), dtype=capi.TENSOR_F16, nhwc=True).flags == 4
    assert capi.make_tensor_norm((0, 0, 0), (1, 1, 1)).flags == 0
    assert "vpf_convert_resize_tensor_nhwc" not in capi.EXPORTS  # a flag, no new symbol


@pytest.mark.parametrize("entry", ENTRY_NAMES)
def test_validation_without_gpu(capi, entry):
    """every refusal comes before any device access"""
    call = _entries(capi)[entry]
    NHWC, BGR = capi.TENSOR_NHWC, capi.TENSOR_BGR
    for dt, elem in ((capi.TENSOR_F32, 4), (capi.TENSOR_F16, 2), (capi.TENSOR_BF16, 2)):
        pitch = 3 * DW * elem
        ok = [(0x400000, pitch), (0, 0), (0, 0)]  # planes 1 and 2 are zero: ignored
        for flags in (NHWC, NHWC | BGR):
            n = _norm(capi, dt, flags)
            # the one plane: pitch below 3 * w * elem (enough for a planar row), a pointer or a pitch that is no multiple of elem, a null pointer
            assert call([(0x400000, pitch - elem), (0, 0), (0, 0)], n) == capi.ERR_BAD_ARG, (dt, flags, "short pitch")
            assert call([(0x400000 + 1, pitch), (0, 0), (0, 0)], n) == capi.ERR_BAD_ARG, (dt, flags, "pointer")
            assert call([(0x400000, pitch + 1), (0, 0), (0, 0)], n) == capi.ERR_BAD_ARG, (dt, flags, "pitch")
            if elem == 4:
                assert call([(0x400000 + 2, pitch), (0, 0), (0, 0)], n) == capi.ERR_BAD_ARG, (dt, flags, "pointer + 2")
                assert call([(0x400000, pitch + 2), (0, 0), (0, 0)], n) == capi.ERR_BAD_ARG, (dt, flags, "pitch + 2")
            assert call([(0, pitch), (0x500000, pitch), (0x600000, pitch)], n) == capi.ERR_BAD_ARG, (dt, flags, "null")
            # null planes 1 and 2 with everything else valid: past validation (the device named does not exist, so nothing is launched)
            st = call(ok, n, NO_GPU)
            assert st not in (capi.OK, capi.ERR_BAD_ARG, capi.ERR_UNSUPPORTED), (dt, flags, st)
            # ... and the same three planes WITHOUT the flag are refused: two of them are null
            assert call(ok, _norm(capi, dt, flags & BGR)) == capi.ERR_BAD_ARG
        # padded rows and garbage in the ignored planes are fine
        st = call([(0x400000, pitch + 64), (0x1, 3), (0x3, 1)], _norm(capi, dt, NHWC), NO_GPU)
        assert st not in (capi.OK, capi.ERR_BAD_ARG, capi.ERR_UNSUPPORTED), (dt, st)
        # unknown flag bits stay unsupported: 2 on its own and next to the known ones, and the top bit
        for flags in (2, NHWC | 2, NHWC | BGR | 2, NHWC | 0x80000000, NHWC | 8):
            assert call(ok, _norm(capi, dt, flags)) == capi.ERR_UNSUPPORTED, (dt, hex(flags))
    assert call([(0x400000, 3 * DW * 4), (0, 0), (0, 0)], _norm(capi, 3, NHWC)) == capi.ERR_UNSUPPORTED  # unknown dtype


class _Resizer:
    """stands in for PySurfaceConvertResizer: a ValueError must come before the resizer is asked to run"""

    def DstSize(self):
        return (16, 8)

    def Stream(self):
        raise AssertionError("validation must come first")

    def ExecuteToTensor(self, *a, **k):
        raise AssertionError("validation must come first")


class _Converter:
    def Size(self):
        return (16, 8)

    def Device(self):
        return 0

    def Stream(self):
        raise AssertionError("validation must come first")

    def ExecuteBatch(self, *a, **k):
        raise AssertionError("validation must come first")


def test_python_stride_rules():
    """the layout is explicit: channels_last=True takes strides (s0, 1, s2, 3) with s2 >= 3 W and s0 >= H s2 and nothing else; the ValueError names
    the strides.  (CPU tensors: the stride rule is checked before anything touches a device.)"""
    torch = pytest.importorskip("torch")
    sys.path.insert(0, os.path.join(ROOT, "videoprocessingframework_amd"))
    import PyNvCodec  # noqa: F401  (under the name every test imports it by, before from_normalized_tensor looks for it)
    from videoprocessingframework_amd import PytorchNvCodec as pnc

    n, h, w = 4, 8, 16
    cl = torch.zeros((n, 3, h, w)).contiguous(memory_format=torch.channels_last)
    assert pnc._channels_last_strides("t", cl, "out") == (h * w * 3, w * 3)
    big = torch.zeros((7, 3, h, w)).contiguous(memory_format=torch.channels_last)
    assert pnc._channels_last_strides("t", big[2:5], "out") == (h * w * 3, w * 3)                # a batch slice
    padded = torch.zeros((n, h, w + 5, 3)).permute(0, 3, 1, 2)[:, :, :, :w]                        # padded rows
    assert pnc._channels_last_strides("t", padded, "out") == (h * (w + 5) * 3, (w + 5) * 3)
    gaps = torch.zeros((n, h + 2, w, 3)).permute(0, 3, 1, 2)[:, :, :h, :]                          # gaps between frames
    assert pnc._channels_last_strides("t", gaps, "out") == ((h + 2) * w * 3, w * 3)
    one = torch.zeros((1, 3, h, w)).contiguous(memory_format=torch.channels_last)
    assert pnc._channels_last_strides("t", one, "out") == (0, w * 3)                               # one frame: the frame stride is never walked
    refused = [torch.zeros((n, 3, h, w)),                                                          # planar
               torch.zeros((n, h, w, 4)).permute(0, 3, 1, 2)[:, :3],                               # a padded fourth channel
               torch.zeros((n, w, h, 3)).permute(0, 3, 2, 1),                                      # transposed rows
               torch.zeros((1, 3, h, w)).contiguous(memory_format=torch.channels_last).expand(n, 3, h, w)]  # an expanded batch: frames overlap
    for t in refused:
        with pytest.raises(ValueError, match=re.escape(str(tuple(t.stride())))):
            pnc._channels_last_strides("t", t, "out")
    # the public functions: from_normalized_tensor checks the layout first ...
    with pytest.raises(ValueError, match="channels_last"):
        pnc.from_normalized_tensor(_Converter(), torch.zeros((2, 3, 8, 16)), (0, 0, 0), (1, 1, 1), channels_last=True)
    with pytest.raises(ValueError, match=re.escape(str((384, 128, 16, 1)))):
        pnc.from_normalized_tensor(_Converter(), torch.zeros((2, 3, 8, 16)), (0, 0, 0), (1, 1, 1), channels_last=True)
    # ... and without the keyword a channels-last tensor is refused exactly as before (nothing is inferred from strides)
    with pytest.raises(ValueError, match="unit stride along W"):
        pnc.from_normalized_tensor(_Converter(), torch.zeros((2, 3, 8, 16)).contiguous(memory_format=torch.channels_last), (0, 0, 0), (1, 1, 1))
    # to_normalized_tensor: `out` must be a device tensor whatever the layout (no GPU here: the stride rule itself is the helper's, above)
    with pytest.raises(ValueError):
        pnc.to_normalized_tensor(_Resizer(), [object()] * 2, (0, 0, 0), (1, 1, 1), out=torch.zeros((2, 3, 8, 16)), channels_last=True)


def test_binding_arguments_without_gpu():
    """the five binding entries take a trailing channels_last (positional calls of before keep their meaning); with it one plane per frame goes
    down and plane_stride is ignored — host-memory surfaces, fake addresses, every call refused before device work"""
    sys.path.insert(0, os.path.join(ROOT, "videoprocessingframework_amd"))
    import PyNvCodec as nvc

    nvc._UseHostAllocator(True)
    try:
        PF = nvc.PixelFormat
        r = nvc.PySurfaceConvertResizer(64, 32, PF.NV12, 16, 8, PF.RGB_PLANAR, 0, 0)
        good = nvc.Surface.Make(PF.NV12, 64, 32, context=0)
        fake, mean, std = 0x400000, [0.5] * 3, [0.5] * 3
        # f32 rows of 16 px: 192 B channels-last.  188 is a fine PLANAR pitch (>= 64) but short for one interleaved row
        assert not r.ExecuteToTensor([good], fake, 0, mean, std, None, False, 188, 0, 0, True)
        assert not r.ExecuteToTensor([good], fake, 0, mean, std, row_pitch=190, channels_last=True)       # not a multiple of 4
        assert not r.ExecuteToTensor([good], fake + 2, 0, mean, std, channels_last=True)                   # f32 at an address that is 2 mod 4
        assert not r.ExecuteRoisToTensor([good], [(0, 0, 0, 8, 8)], fake, 1, mean, std, row_stride=94, channels_last=True)   # f16: below 96
        assert not r.ExecuteWarpsToTensor([good], [0], [(1, 0, 0, 0, 1, 0)], fake, 2, mean, std, row_stride=95, channels_last=True)
        assert not r.ExecuteToTensor([nvc.Surface.Make(PF.NV12, 32, 32, context=0)], fake, 0, mean, std, channels_last=True)  # wrong size
        t = nvc.PyTensorToSurface(16, 8, PF.NV12, 0, 0)
        assert t.Execute(fake, 0, mean, std, None, False, 188, 0, True).Empty()
        assert t.Execute(fake + 1, 1, mean, std, channels_last=True).Empty()
        dst = [nvc.Surface.Make(PF.NV12, 16, 8, context=0)]
        assert not t.ExecuteBatch(fake, dst, 0, mean, std, None, False, 188, 0, 0, True)
        assert not t.ExecuteBatch(fake, dst, 2, mean, std, row_pitch=94, channels_last=True)
        stub = open(os.path.join(ROOT, "videoprocessingframework_amd", "PyNvCodec", "__init__.pyi")).read()
        assert stub.count("channels_last: bool = ...") == 5
    finally:
        nvc._UseHostAllocator(False)


# FC_TENSOR_NHWC = 8 (FC_TENSOR = 6, FC_P16 = 7): the channels-last instantiations of the fused families, of the ROI / warp kernels and of the way back
_NHWC_KERNEL = re.compile(r"k_convert_(half|strip_wg|resize_band|resize_lds|resize)<\d, 8, |k_(roi|warp)_(strip|gather)<\d, 8>|k_tensor_yuv_r<\d, (true|false), true>|k_tensor_yuv_quad<(true|false), true>")


@pytest.mark.timeout(900)
@pytest.mark.parametrize("tu,count", [
    # both frame tables each: half x 3 sources; strip R = 2 4 8 16 x 3 sources; band and lds x 2 strip sizes x NV12 / YUV420; gather x 3 sources
    ("k_convert_resize.hip", 2 * (3 + 4 * 3 + 2 * 2 + 2 * 2 + 3)),
    ("k_convert_roi.hip", 6), ("k_convert_warp.hip", 6),   # staged and gather forms x NV12 / YUV420 / P16
    ("k_rgb2yuv.hip", 3 * 2 + 2),                          # the fast kernel x three dtypes x NV12 / YUV420, the quad kernel x NV12 / YUV420
])
def test_no_nhwc_instantiation_spills(tu, count):
    """resource metadata of the code object only (tools/isa_stats.spills): every channels-last instantiation uses no scratch, spills nothing and
    stays within 128 VGPRs (two workgroups of 256 lanes per SIMD at least: the bound of the 16-bit source class)"""
    import isa_stats

    rows = [r for r in isa_stats.spills(os.path.join(ROOT, "videoprocessingframework_amd", "csrc", tu)) if _NHWC_KERNEL.search(r[0])]
    assert len(rows) == count, [r[0] for r in rows]
    for name, vgpr, vspill, sspill, scratch in rows:
        print(name[:100], "vgpr", vgpr)
        assert vspill == 0 and sspill == 0 and scratch == 0, (name, vgpr, vspill, sspill, scratch)
        assert vgpr <= 128, (name, vgpr)
