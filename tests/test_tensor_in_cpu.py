"""The planar float tensor -> NV12 / YUV420 path (vpf_tensor_convert, PyTensorToSurface, PytorchNvCodec.from_normalized_tensor) without a GPU:
the symbols and bindings exist, every validation rule answers before any device work (fake pointers: nothing here may reach a launch),
mean / std map to scale / bias, and the quantiser restated in numpy and in torch-CPU agree bit for bit.

Definition (include/vpf_hip.h), for input plane c and element x widened exactly to fp32:
    v = fl32(fl32(x * scale[c]) + bias[c]);  q = fminf(fmaxf(v, 0), 255) with NaN -> 0;  u8 = rint(q), ties to even
then the bytes of vpf_convert(RGB_PLANAR -> YUV420, BT_601, range) [+ vpf_convert(YUV420 -> NV12)] on the three u8 planes."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (name, mean, std): every parameter set the GPU test uses
PARAM_SETS = [
    ("imagenet", (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)),
    ("unit", (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)),  # the identity normalisation of [0, 1] pixels: scale 255, bias 0
]
RAW_IDENTITY = ("raw_identity", None, None)  # scale 1, bias 0 handed to the C ABI directly: v = x, so ties k + 0.5 can be written down


def denorm_scale_bias_f32(mean, std):
    """the definition: scale = 255 std, bias = 255 mean, both in double, then rounded to fp32"""
    return (np.array([255.0 * s for s in std], dtype=np.float32), np.array([255.0 * m for m in mean], dtype=np.float32))


def quantise_numpy(x, scale, bias):
    """x: [3, H, W] float32 / float16 (bf16 arrives widened to float32), scale / bias: float32[3] -> uint8 [3, H, W].  The three lines of the
    definition: numpy's float32 multiply and add round once each (no fma), np.rint rounds ties to even."""
    x32 = np.asarray(x).astype(np.float32)  # exact widening
    s = np.asarray(scale, dtype=np.float32)[:, None, None]
    b = np.asarray(bias, dtype=np.float32)[:, None, None]
    with np.errstate(all="ignore"):
        p = (x32 * s).astype(np.float32)
        v = (p + b).astype(np.float32)
        v = np.where(np.isnan(v), np.float32(0), v)  # fmaxf(NaN, 0) = 0
        q = np.minimum(np.maximum(v, np.float32(0)), np.float32(255))
        return np.rint(q).astype(np.uint8)


def quantise_torch(x, scale, bias):
    """the same in torch on the CPU: [3, H, W] tensor of float32 / float16 / bfloat16 -> uint8 numpy"""
    import torch

    x32 = x.to(torch.float32)
    s = torch.from_numpy(np.asarray(scale, dtype=np.float32)).view(3, 1, 1)
    b = torch.from_numpy(np.asarray(bias, dtype=np.float32)).view(3, 1, 1)
    v = torch.mul(x32, s)
    v = torch.add(v, b)
    v = torch.nan_to_num(v, nan=0.0, posinf=math.inf, neginf=-math.inf)
    return torch.round(torch.clamp(v, 0.0, 255.0)).to(torch.uint8).numpy()


def special_values_f32():
    """+-0, +-inf, NaN, +-3e38, exact ties k + 0.5 for even and odd k (identity parameters), values around both clamps, fp32 / f16 subnormals"""
    ties = [k + 0.5 for k in range(-2, 258)]
    f16_sub = [float(np.float16(2.0 ** -24) * k) for k in (1, 2, 3, 511, 1023)]
    vals = [0.0, -0.0, math.inf, -math.inf, math.nan, 3e38, -3e38, 1e-45, -1e-45, 1.1754942e-38, 254.5, 255.5, 254.49998, 255.0, 256.0, -0.5, 0.49999997,
            0.5, 0.50000006, 1.5, 2.5, 1e10, -1e10] + ties + f16_sub + [-v for v in f16_sub]
    return np.array(vals, dtype=np.float32)


def test_symbols_and_bindings_exist(capi):
    names = ("vpf_tensor_convert_supported", "vpf_tensor_convert", "vpf_tensor_convert_batch")
    nm = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    h = open(os.path.join(ROOT, "include", "vpf_hip.h")).read()
    for name in names:
        assert name in capi.EXPORTS
        assert hasattr(capi.lib(), name)
        assert f" {name}\n" in nm
        assert f" {name}(" in h
    for decl in ("VPF_API int vpf_tensor_convert_supported(int dst_fmt, int color_space, int color_range)", "VPF_API vpf_status vpf_tensor_convert(",
                 "VPF_API vpf_status vpf_tensor_convert_batch("):
        assert h.index(decl) > h.index("typedef struct vpf_tensor_norm"), decl
    for fn in ("tensor_convert_supported", "tensor_convert", "tensor_convert_batch", "denorm_params", "make_tensor_denorm"):
        assert callable(getattr(capi, fn)), fn


def test_python_classes_exist():
    sys.path.insert(0, os.path.join(ROOT, "videoprocessingframework_amd"))
    import PyNvCodec as nvc
    for m in ("Execute", "ExecuteBatch", "Stream", "Format", "Size", "Device"):
        assert hasattr(nvc.PyTensorToSurface, m), m
    stub = open(os.path.join(ROOT, "videoprocessingframework_amd", "PyNvCodec", "__init__.pyi")).read()
    i = stub.index("class PyTensorToSurface")
    body = stub[i:stub.index("\nclass ", i + 1)]
    for m in ("def Execute(", "def ExecuteBatch(", "def Stream(", "def Format(", "def Size(", "gpu_id: int", "context: int, stream: int"):
        assert m in body, m
    src = open(os.path.join(ROOT, "videoprocessingframework_amd", "PytorchNvCodec", "__init__.py")).read()
    assert "def from_normalized_tensor(converter, tensor, mean, std, bgr=False, cc_ctx=None, out=None)" in src


def test_supported_agrees_with_the_rgb_planar_yuv420_pair(capi):
    for cs in range(-1, 5):
        for cr in range(-1, 5):
            want = capi.convert_supported(capi.RGB_PLANAR, capi.YUV420, cs, cr)
            assert want == (cs == capi.BT_601 and cr in (capi.MPEG, capi.JPEG))
            for df in range(-1, 20):
                assert capi.tensor_convert_supported(df, cs, cr) == (want and df in (capi.NV12, capi.YUV420)), (df, cs, cr)


def _norm(capi, dtype=0, flags=0, scale=(58.0, 57.0, 56.0), bias=(120.0, 110.0, 100.0)):
    n = capi.TensorNorm()
    for c in range(3):
        n.scale[c], n.bias[c] = scale[c], bias[c]
    n.dtype, n.flags = dtype, flags
    return n


def test_validation_without_gpu(capi):
    """every refusal happens before any device work: the plane pointers below are fake"""
    ex = capi.make_exec()
    w, h = 16, 8
    nv12 = [(0x100000, 16), (0x200000, 16)]
    yuv = [(0x100000, 16), (0x200000, 8), (0x300000, 8)]
    f32 = [(0x400000, 64), (0x500000, 64), (0x600000, 64)]  # w * 4 = 64
    f16 = [(0x400000, 32), (0x500000, 32), (0x600000, 32)]

    def call(src, norm, df=capi.NV12, cs=0, cr=1, dst=nv12, size=(w, h)):
        return capi.tensor_convert(ex, df, cs, cr, size[0], size[1], src, dst, norm, check=False)

    # destinations and colour models: only NV12 / YUV420, only what vpf_convert(RGB_PLANAR, YUV420) takes (BT.601, MPEG / JPEG)
    for df in (capi.RGB, capi.YUV444, capi.RGB_PLANAR, capi.Y, capi.YCBCR, capi.P10, 99):
        assert call(f32, _norm(capi), df=df, dst=yuv) == capi.ERR_UNSUPPORTED, df
    assert call(f32, _norm(capi), cs=capi.BT_709) == capi.ERR_UNSUPPORTED
    assert call(f32, _norm(capi), cs=2) == capi.ERR_UNSUPPORTED
    assert call(f32, _norm(capi), cr=2) == capi.ERR_UNSUPPORTED
    assert call(f32, _norm(capi), df=capi.YUV420, dst=yuv, cs=capi.BT_709, cr=0) == capi.ERR_UNSUPPORTED
    # an unknown dtype or flag bit
    assert call(f32, _norm(capi, dtype=3)) == capi.ERR_UNSUPPORTED
    assert call(f32, _norm(capi, dtype=0xFFFFFFFF)) == capi.ERR_UNSUPPORTED
    assert call(f32, _norm(capi, flags=2)) == capi.ERR_UNSUPPORTED
    assert call(f32, _norm(capi, flags=capi.TENSOR_BGR | 0x80000000)) == capi.ERR_UNSUPPORTED
    # a non-finite scale or bias
    for bad in (math.nan, math.inf, -math.inf):
        for c in range(3):
            sc, bi = [58.0] * 3, [100.0] * 3
            sc[c] = bad
            assert call(f32, _norm(capi, scale=sc)) == capi.ERR_BAD_ARG
            sc[c], bi[c] = 58.0, bad
            assert call(f32, _norm(capi, bias=bi)) == capi.ERR_BAD_ARG
    # no parameters, no exec, no planes
    L = capi.lib()
    assert L.vpf_tensor_convert(capi.C.byref(ex), capi.NV12, 0, 1, capi.Size(w, h), capi.planes(f32), capi.planes(nv12), None) == capi.ERR_BAD_ARG
    assert L.vpf_tensor_convert(None, capi.NV12, 0, 1, capi.Size(w, h), capi.planes(f32), capi.planes(nv12), capi.C.byref(_norm(capi))) == capi.ERR_BAD_ARG
    assert L.vpf_tensor_convert(capi.C.byref(ex), capi.NV12, 0, 1, capi.Size(w, h), None, capi.planes(nv12), capi.C.byref(_norm(capi))) == capi.ERR_BAD_ARG
    assert L.vpf_tensor_convert(capi.C.byref(ex), capi.NV12, 0, 1, capi.Size(w, h), capi.planes(f32), None, capi.C.byref(_norm(capi))) == capi.ERR_BAD_ARG
    # source pointers / pitches that are not multiples of the element size, pitches below w * elem, missing planes
    for dt, planes, elem in ((capi.TENSOR_F32, f32, 4), (capi.TENSOR_F16, f16, 2), (capi.TENSOR_BF16, f16, 2)):
        for k in range(3):
            p = list(planes)
            p[k] = (planes[k][0] + 1, planes[k][1])
            assert call(p, _norm(capi, dtype=dt)) == capi.ERR_BAD_ARG, (dt, k, "pointer")
            p[k] = (planes[k][0], planes[k][1] + 1)
            assert call(p, _norm(capi, dtype=dt)) == capi.ERR_BAD_ARG, (dt, k, "pitch")
            p[k] = (planes[k][0], w * elem - elem)
            assert call(p, _norm(capi, dtype=dt)) == capi.ERR_BAD_ARG, (dt, k, "short pitch")
            p[k] = (0, planes[k][1])
            assert call(p, _norm(capi, dtype=dt)) == capi.ERR_BAD_ARG, (dt, k, "null")
        if elem == 4:
            assert call([(a + 2, b) for a, b in planes], _norm(capi, dtype=dt)) == capi.ERR_BAD_ARG
    assert call(f32[:2], _norm(capi)) == capi.ERR_BAD_ARG  # the third plane is missing
    # destinations: what vpf_convert refuses (null planes, short pitches), for both formats
    assert call(f32, _norm(capi), dst=[(0x100000, 16)]) == capi.ERR_BAD_ARG
    assert call(f32, _norm(capi), dst=[(0x100000, 15), (0x200000, 16)]) == capi.ERR_BAD_ARG
    assert call(f32, _norm(capi), dst=[(0x100000, 16), (0x200000, 15)]) == capi.ERR_BAD_ARG
    assert call(f32, _norm(capi), df=capi.YUV420, dst=yuv[:2]) == capi.ERR_BAD_ARG
    assert call(f32, _norm(capi), df=capi.YUV420, dst=[(0x100000, 16), (0x200000, 8), (0x300000, 7)]) == capi.ERR_BAD_ARG
    # odd widths: NV12 chroma rows hold 2 * ceil(w / 2) bytes
    assert call([(a, 60) for a, _ in f32], _norm(capi), dst=[(0x100000, 15), (0x200000, 15)], size=(15, 8)) == capi.ERR_BAD_ARG
    # sizes
    assert call(f32, _norm(capi), size=(0, h)) == capi.ERR_BAD_ARG
    assert call(f32, _norm(capi), size=(w, 0)) == capi.ERR_BAD_ARG
    assert call(f32, _norm(capi), size=(w, 65537)) == capi.ERR_BAD_ARG
    assert call(f32, _norm(capi), size=(65537, h)) == capi.ERR_BAD_ARG
    # the batch entry: n = 0, no frames, one bad frame among good ones
    good = capi.make_batch([(f32, nv12)] * 3)
    assert capi.tensor_convert_batch(ex, capi.NV12, 0, 1, w, h, good, _norm(capi), n=0, check=False) == capi.ERR_BAD_ARG
    assert L.vpf_tensor_convert_batch(capi.C.byref(ex), capi.NV12, 0, 1, capi.Size(w, h), 3, None, capi.C.byref(_norm(capi))) == capi.ERR_BAD_ARG
    mixed = capi.make_batch([(f32, nv12), (f32, nv12), ([(0x400000, 64), (0x500002, 64), (0x600000, 64)], nv12)])
    assert capi.tensor_convert_batch(ex, capi.NV12, 0, 1, w, h, mixed, _norm(capi), check=False) == capi.ERR_BAD_ARG
    assert capi.tensor_convert_batch(ex, capi.NV12, 0, 1, w, h, good, _norm(capi, dtype=7), check=False) == capi.ERR_UNSUPPORTED
    assert capi.tensor_convert_batch(ex, capi.RGB, 0, 1, w, h, good, _norm(capi), check=False) == capi.ERR_UNSUPPORTED
    with pytest.raises(capi.VpfError):
        capi.tensor_convert(ex, capi.NV12, 0, 1, w, h, f32, nv12, _norm(capi, dtype=3))


def test_mean_std_to_scale_bias(capi):
    """scale = 255 std, bias = 255 mean, in double, then fp32; identity parameters are raw scale 1 / bias 0"""
    for name, mean, std in PARAM_SETS:
        scale, bias = denorm_scale_bias_f32(mean, std)
        n = capi.make_tensor_denorm(mean, std, dtype=capi.TENSOR_BF16, bgr=True)
        assert (n.dtype, n.flags) == (capi.TENSOR_BF16, capi.TENSOR_BGR)
        for c in range(3):
            assert np.float32(n.scale[c]) == scale[c] and np.float32(n.bias[c]) == bias[c], (name, c)
            assert scale[c] == np.float32(255.0 * std[c]) and bias[c] == np.float32(255.0 * mean[c])
    s, b = denorm_scale_bias_f32((0.5,) * 3, (0.5,) * 3)
    assert (s == np.float32(127.5)).all() and (b == np.float32(127.5)).all()  # [-1, 1] -> [0, 255]
    n = capi.make_tensor_denorm(scale=(1.0, 1.0, 1.0), bias=(0.0, 0.0, 0.0))
    assert [n.scale[c] for c in range(3)] == [1.0] * 3 and [n.bias[c] for c in range(3)] == [0.0] * 3
    for bad_mean, bad_std in (((0, 0, 0), (1, 0, 1)), ((0, 0, 0), (1, -1, 1)), ((0, math.nan, 0), (1, 1, 1)), ((0, 0, 0), (1, math.inf, 1)),
                              ((0, 0), (1, 1))):
        with pytest.raises(ValueError):
            capi.denorm_params(bad_mean, bad_std)
    # the round trip of the parameters: normalise then denormalise a code lands on the code (ImageNet, all 256 codes, fp32 arithmetic)
    for name, mean, std in PARAM_SETS:
        scale, bias = denorm_scale_bias_f32(mean, std)
        codes = np.arange(256, dtype=np.float64)
        for c in range(3):
            x = ((codes / 255.0 - mean[c]) / std[c]).astype(np.float32)
            back = quantise_numpy(np.broadcast_to(x[None, None, :], (3, 1, 256)), scale[[c] * 3], bias[[c] * 3])[0, 0]
            assert (back == np.arange(256)).all(), (name, c)


@pytest.mark.parametrize("name,mean,std", PARAM_SETS + [RAW_IDENTITY])
def test_quantiser_restatements_agree(name, mean, std):
    """numpy and torch-CPU compute x * scale + bias in fp32 with two roundings, clamp with NaN -> 0 and round ties to even: bit-identical on
    random inputs and on the special values, for every dtype"""
    import torch
    if name == "raw_identity":
        scale, bias = np.ones(3, np.float32), np.zeros(3, np.float32)
    else:
        scale, bias = denorm_scale_bias_f32(mean, std)
    rng = np.random.default_rng(20240917)
    sp = special_values_f32()
    spread, centre = {"imagenet": (1.0, 0.0), "unit": (0.35, 0.5), "raw_identity": (140.0, 120.0)}[name]
    rand = (rng.standard_normal((3, 64, 257)) * spread + centre).astype(np.float32)
    special = np.broadcast_to(sp[None, None, :], (3, 1, sp.size)).copy()
    for x in (rand, special):
        for tdt in (torch.float32, torch.float16, torch.bfloat16):
            with np.errstate(all="ignore"):
                t = torch.from_numpy(x).to(tdt)
            widened = t.to(torch.float32).numpy()
            a = quantise_numpy(widened if tdt != torch.float16 else t.numpy(), scale, bias)
            b = quantise_torch(t, scale, bias)
            assert np.array_equal(a, b), (name, tdt, int((a != b).sum()))
            if x is rand:
                assert (a == 0).any() and (a == 255).any() and ((a > 0) & (a < 255)).any()
    # the special values under identity parameters, spelled out: ties go to the even neighbour, NaN and -inf to 0, +inf and 3e38 to 255
    if name == "raw_identity":
        q = quantise_numpy(special, scale, bias)[0, 0]
        look = {float(v): int(r) for v, r in zip(sp, q) if not math.isnan(v)}
        assert look[0.5] == 0 and look[1.5] == 2 and look[2.5] == 2 and look[253.5] == 254 and look[254.5] == 254 and look[255.5] == 255
        assert look[-0.5] == 0 and look[math.inf] == 255 and look[-math.inf] == 0 and look[float(np.float32(3e38))] == 255
        assert look[float(np.float32(-3e38))] == 0 and look[256.0] == 255 and look[float(np.float32(0.50000006))] == 1
        assert q[[i for i, v in enumerate(sp) if math.isnan(v)]].tolist() == [0]


def test_binding_validation_without_gpu():
    """PyTensorToSurface: ValueError for std <= 0 or a non-finite mean / std, False / an empty Surface for a wrong surface size or format, a
    refused layout or a refused colour context: all before any device work (host-memory surfaces, a fake source address)"""
    sys.path.insert(0, os.path.join(ROOT, "videoprocessingframework_amd"))
    import PyNvCodec as nvc
    nvc._UseHostAllocator(True)
    try:
        PF = nvc.PixelFormat
        for bad in (PF.RGB, PF.RGB_PLANAR, PF.YUV444, PF.Y):
            with pytest.raises(ValueError):
                nvc.PyTensorToSurface(16, 8, bad, 0, 0)
        with pytest.raises(ValueError):
            nvc.PyTensorToSurface(0, 8, PF.NV12, 0, 0)
        t = nvc.PyTensorToSurface(16, 8, PF.NV12, 0, 0)
        assert tuple(t.Size()) == (16, 8) and t.Format() == PF.NV12 and isinstance(t.Stream(), int)
        ty = nvc.PyTensorToSurface(16, 8, PF.YUV420, 0, 0)
        assert ty.Format() == PF.YUV420
        good = nvc.Surface.Make(PF.NV12, 16, 8, context=0)
        fake = 0x400000
        im_mean, im_std = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
        for m, s in (([0, 0, 0], [1, 0, 1]), ([0, 0, 0], [1, -0.5, 1]), ([math.nan, 0, 0], [1, 1, 1]), ([0, 0, 0], [1, 1, math.inf]),
                     ([0, math.inf, 0], [1, 1, 1]), ([0, 0], [1, 1, 1]), ([0, 0, 0], [1e38, 1, 1]), ([1e38, 0, 0], [1, 1, 1])):
            with pytest.raises(ValueError):
                t.ExecuteBatch(fake, [good], 0, m, s)
            with pytest.raises(ValueError):
                t.Execute(fake, 0, m, s)
        assert not t.ExecuteBatch(fake, [nvc.Surface.Make(PF.NV12, 32, 8, context=0)], 0, im_mean, im_std)   # wrong size
        assert not t.ExecuteBatch(fake, [nvc.Surface.Make(PF.YUV420, 16, 8, context=0)], 0, im_mean, im_std)  # wrong format
        assert not t.ExecuteBatch(fake, [good, nvc.Surface.Make(PF.NV12, 16, 4, context=0)], 1, im_mean, im_std)
        assert not t.ExecuteBatch(fake, [], 0, im_mean, im_std)
        assert not t.ExecuteBatch(0, [good], 0, im_mean, im_std)                         # no tensor
        assert not t.ExecuteBatch(fake, [good], 3, im_mean, im_std)                      # unknown dtype: the library refuses it
        assert not t.ExecuteBatch(fake, [good], 0, im_mean, im_std, row_pitch=66)        # not a multiple of 4
        assert not t.ExecuteBatch(fake + 2, [good], 0, im_mean, im_std)                  # f32 planes at a 2-byte address
        assert not t.ExecuteBatch(fake + 1, [good], 1, im_mean, im_std)                  # f16 planes at an odd address
        assert not t.ExecuteBatch(fake, [good], 0, im_mean, im_std, row_pitch=60)        # below 16 x 4 bytes
        assert t.Execute(fake, 3, im_mean, im_std).Empty()
        assert t.Execute(fake, 0, im_mean, im_std, row_pitch=60).Empty()
        assert t.Execute(0, 0, im_mean, im_std).Empty()
        # the colour-context rule of rgb_planar_yuv420: BT.601 only, whatever the extended colour spaces say
        for ext in (False, True):
            nvc.SetExtendedColorspaces(ext)
            cc709 = nvc.ColorspaceConversionContext(nvc.ColorSpace.BT_709, nvc.ColorRange.JPEG)
            assert not t.ExecuteBatch(fake, [good], 0, im_mean, im_std, cc_ctx=cc709)
            assert t.Execute(fake, 0, im_mean, im_std, cc_ctx=cc709).Empty()
            assert not ty.ExecuteBatch(fake, [nvc.Surface.Make(PF.YUV420, 16, 8, context=0)], 0, im_mean, im_std, cc_ctx=cc709)
    finally:
        nvc.SetExtendedColorspaces(False)
        nvc._UseHostAllocator(False)


def test_from_normalized_tensor_refuses_bad_arguments_without_gpu():
    import torch
    sys.path.insert(0, os.path.join(ROOT, "videoprocessingframework_amd"))
    import PyNvCodec as nvc
    from videoprocessingframework_amd import PytorchNvCodec as pnc

    nvc._UseHostAllocator(True)
    try:
        t = nvc.PyTensorToSurface(16, 8, nvc.PixelFormat.NV12, 0, 0)
        mean, std = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
        for bad in (torch.zeros((1, 3, 8, 16), dtype=torch.float64), torch.zeros((1, 3, 8, 16), dtype=torch.uint8), np.zeros((1, 3, 8, 16), np.float32),
                    torch.zeros((1, 3, 8, 16)),            # a host tensor
                    torch.zeros((1, 3, 16, 8)), torch.zeros((1, 4, 8, 16)), torch.zeros((8, 16))):
            with pytest.raises(ValueError):
                pnc.from_normalized_tensor(t, bad, mean, std)
        # zero strides: the binding reads a stride of 0 as "contiguous", so an expanded channel / frame / row must never reach it (it would be
        # read at the contiguous offsets, past the end of the storage); negative, short and non-unit strides likewise.  The layout is
        # checked before the device, so host tensors show it.
        gray, frame, row = torch.zeros((2, 1, 8, 16)), torch.zeros((1, 3, 8, 16)), torch.zeros((2, 3, 1, 16))
        col = torch.zeros((2, 3, 8, 1))
        for bad in (gray.expand(-1, 3, -1, -1), gray[0].expand(3, -1, -1), frame.expand(2, -1, -1, -1), row.expand(-1, -1, 8, -1), col.expand(-1, -1, -1, 16),
                    torch.zeros((2, 3, 8, 32))[..., ::2], torch.zeros((2, 3, 16, 8)).transpose(2, 3), torch.zeros((2, 3, 8, 24)).as_strided((2, 3, 8, 16), (384, 128, 8, 1))):
            assert tuple(bad.shape[-3:]) == (3, 8, 16)
            with pytest.raises(ValueError, match="contiguous"):
                pnc.from_normalized_tensor(t, bad, mean, std)
        with pytest.raises(ValueError, match="device tensor"):  # a good layout on the host gets as far as the device check
            pnc.from_normalized_tensor(t, torch.zeros((2, 3, 8, 16)), mean, std)
        assert t.Device() in (-1, 0)
    finally:
        nvc._UseHostAllocator(False)
