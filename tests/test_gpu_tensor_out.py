"""The normalised planar-tensor output of the fused path on the MI355X: vpf_convert_resize_tensor(_batch), PySurfaceConvertResizer.ExecuteToTensor
and PytorchNvCodec.to_normalized_tensor.

Ground truth is the oracle's 8-bit RGB_PLANAR picture (oracle.convert_resize(..., RGB_PLANAR, ..., mode=FP32)), computed once per (shape, source,
matrix) and reused for every dtype and layout.  From it:
  ref32 = float32(float64(u8) * float64(scale_f32) + float64(bias_f32))    exact in float64 (tests/test_tensor_out_cpu.py::test_exactness_premise),
                                                                           so ref32 IS fmaf(u8, scale, bias)
  ref16 = ref32.astype(float16), refbf = torch.from_numpy(ref32).to(torch.bfloat16)   (round to nearest even)
Every element of every output must be bit-identical to its reference: an off-by-one in the 8-bit stage moves an fp32 output by at least
1 / (255 x 0.229) = 0.017.  Bytes around the written elements hold canaries that must come back untouched."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from cases_fused_families import FAMILIES, TENSOR_OUT_CASES
from gpu_util import DevPlanes, stream_handle
from test_tensor_out_cpu import PARAM_SETS, scale_bias_f32

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = 0xCD
ELEM = {0: 4, 1: 2, 2: 2}
MATRICES = [(0, 0), (0, 1), (1, 0), (1, 1)]  # (colour space, range): BT.601 / BT.709 x MPEG / JPEG
PARAMS = {name: (mean, std) for name, mean, std in PARAM_SETS}

# the fused families: (name, sw, sh, dw, dh, frames, VPF_TUNE_NV12_RGB_VARIANT, source offset, the label the selection log must carry)
FAMILY_CASES = TENSOR_OUT_CASES


@pytest.fixture(scope="module")
def orc(oracle):
    oracle.set_threads(16)
    return oracle


_PICS = {}


def picture(orc, sf, cs, cr, sw, sh, dw, dh, seed):
    """(source planes, oracle RGB_PLANAR planes), once per (shape, source, matrix, seed)"""
    key = (sf, cs, cr, sw, sh, dw, dh, seed)
    if key not in _PICS:
        src = orc.synth(getattr(orc, sf), sw, sh, seed)
        st, want = orc.convert_resize(getattr(orc, sf), orc.RGB_PLANAR, cs, cr, sw, sh, src, dw, dh, mode=orc.FP32)
        assert st == 0
        _PICS[key] = (src, np.stack(want))
    return _PICS[key]


def reference_bits(u8, mean, std, dtype, bgr):
    """u8: [3, dh, dw] R G B bytes -> the output planes' bit patterns [3, dh, dw] in output channel order"""
    scale, bias = scale_bias_f32(mean, std)
    planes = u8[::-1] if bgr else u8
    ref32 = (planes.astype(np.float64) * scale.astype(np.float64)[:, None, None] + bias.astype(np.float64)[:, None, None]).astype(np.float32)
    if dtype == 0:
        return ref32.view(np.uint32)
    if dtype == 1:
        return ref32.astype(np.float16).view(np.uint16)
    return torch.from_numpy(np.ascontiguousarray(ref32)).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


class TensorBuf:
    """n frames of three planes in one canary-filled byte buffer: plane (i, c) at lead + i frame + c plane, rows `row` bytes apart"""

    def __init__(self, n, dw, dh, elem, row=0, plane=0, frame=0, lead=256, tail=256):
        self.n, self.dw, self.dh, self.elem = n, dw, dh, elem
        self.row = row or dw * elem
        self.plane = plane or dh * self.row
        self.frame = frame or 3 * self.plane
        self.lead = lead
        size = lead + (n - 1) * self.frame + 2 * self.plane + (dh - 1) * self.row + dw * elem + tail
        self.buf = torch.full((size,), CANARY, dtype=torch.uint8, device="cuda")

    def planes(self, i):
        base = self.buf.data_ptr() + self.lead + i * self.frame
        return [(base + c * self.plane, self.row) for c in range(3)]

    def frames(self):
        """-> ([n, 3, dh, dw] bit patterns, canaries intact)"""
        h = self.buf.cpu().numpy()
        mask = np.zeros(h.shape, bool)
        out = np.empty((self.n, 3, self.dh, self.dw), np.uint32 if self.elem == 4 else np.uint16)
        for i in range(self.n):
            for c in range(3):
                off = self.lead + i * self.frame + c * self.plane
                view = np.lib.stride_tricks.as_strided(h[off:], shape=(self.dh, self.dw * self.elem), strides=(self.row, 1))
                out[i, c] = np.ascontiguousarray(view).view(out.dtype)
                np.lib.stride_tricks.as_strided(mask[off:], shape=(self.dh, self.dw * self.elem), strides=(self.row, 1))[:] = True
        return out, bool((h[~mask] == CANARY).all())


def assert_bits(got, want, what):
    if not np.array_equal(got, want):
        d = np.argwhere(got != want)
        first = tuple(d[0])
        raise AssertionError(f"{what}: {len(d)} of {got.size} elements differ; first at {first}: got {got[first]:#x} want {want[first]:#x}")


def run_capi(capi, sf, cs, cr, sw, sh, dw, dh, srcs, dtype, bgr, params, buf, batch=True):
    mean, std = PARAMS[params]
    norm = capi.make_tensor_norm(mean, std, dtype=dtype, bgr=bgr)
    ex = capi.make_exec(stream_handle())
    if batch:
        capi.convert_resize_tensor_batch(ex, getattr(capi, sf), cs, cr, sw, sh, dw, dh,
                                         capi.make_batch([(s.desc(), buf.planes(i)) for i, s in enumerate(srcs)]), norm)
    else:
        assert len(srcs) == 1
        capi.convert_resize_tensor(ex, getattr(capi, sf), cs, cr, sw, sh, srcs[0].desc(), dw, dh, buf.planes(0), norm)
    torch.cuda.synchronize()


def test_every_family_is_selected():
    """the kernel-selection log (VPF_HIP_LOG=2, child process) carries, for every case of FAMILY_CASES, exactly the label of its instantiation: family,
    NV12 -> planar tensor, band height, frame table with the epilogue (tests/cases_fused_families.py)"""
    code = f"""
import sys
sys.path.insert(0, {ROOT!r})
import torch
from videoprocessingframework_amd import capi
ex = capi.make_exec(torch.cuda.current_stream().cuda_stream)
for name, sw, sh, dw, dh, n, variant, off in {[c[:8] for c in FAMILY_CASES]!r}:
    y = torch.zeros(sh * ((sw + 255) // 256 * 256) * 2 + 4096, dtype=torch.uint8, device="cuda")
    p = (sw + 255) // 256 * 256
    src = [(y.data_ptr() + off, p), (y.data_ptr() + off + p * sh, p)]
    out = torch.empty(n * 3 * dh * dw, dtype=torch.float32, device="cuda")
    dst = [[(out.data_ptr() + 4 * dw * dh * (3 * i + c), 4 * dw) for c in range(3)] for i in range(n)]
    prev = capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, variant)
    print("CASE", name, file=sys.stderr, flush=True)
    capi.convert_resize_tensor_batch(ex, capi.NV12, 1, 0, sw, sh, dw, dh, capi.make_batch([(src, d) for d in dst]), capi.make_tensor_norm((0, 0, 0), (1, 1, 1)))
    torch.cuda.synchronize()
    capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, prev)
print("done")
"""
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, VPF_HIP_LOG="2"), timeout=300)
    assert r.returncode == 0 and "done" in r.stdout, r.stdout + r.stderr
    logs = {}
    for chunk in r.stderr.split("CASE ")[1:]:
        name, rest = chunk.split("\n", 1)
        logs[name.strip()] = [l for l in rest.split("\n") if "libvpfhip: launch" in l]
    seen = set()
    for name, *_, label in FAMILY_CASES:
        lines = logs[name]
        print(name, lines)
        assert lines and all(l.split("launch ", 1)[1].strip() == label for l in lines), (name, label, lines)
        seen.add(label[1:label.index("<")])
    assert seen == set(FAMILIES), seen


@pytest.mark.parametrize("case", FAMILY_CASES, ids=[c[0] for c in FAMILY_CASES])
def test_families_sources_matrices_dtypes(capi, orc, case):
    """each family x NV12 / YUV420 x the four (colour space, range) pairs x f32 / f16 / bf16 x RGB / BGR: bit-identical, canaries intact"""
    name, sw, sh, dw, dh, n, variant, off, _ = case
    prev = capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, variant)
    try:
        for sf in ("NV12", "YUV420"):
            for k, (cs, cr) in enumerate(MATRICES):
                seeds = [9100 + k, 9200 + k] if n > 1 else [9100 + k]
                pics = [picture(orc, sf, cs, cr, sw, sh, dw, dh, s) for s in seeds]
                S = [DevPlanes(p[0], offset=off) for p in pics]
                srcs = [S[i % len(S)] for i in range(n)]
                for dtype in (0, 1, 2):
                    bgr = (k + dtype) % 2 == 1
                    params = ("imagenet", "unit", "symmetric")[(k + dtype) % 3]
                    buf = TensorBuf(n, dw, dh, ELEM[dtype])
                    run_capi(capi, sf, cs, cr, sw, sh, dw, dh, srcs, dtype, bgr, params, buf, batch=n > 1 or k % 2 == 0)
                    got, intact = buf.frames()
                    what = f"{name} {sf} cs{cs} cr{cr} dtype{dtype} bgr{bgr} {params}"
                    assert intact, what
                    refs = [reference_bits(p[1], *PARAMS[params], dtype, bgr) for p in pics]
                    for i in range(n):
                        assert_bits(got[i], refs[i % len(refs)], f"{what} frame {i}")
    finally:
        capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, prev)


@pytest.mark.parametrize("n", [1, 7, 33, 129])
def test_batch_sizes_and_layouts(capi, orc, n):
    """n across the 32- and 128-frame tables, 1080p -> 224 x 224 (the ResNet input), every dtype in both channel orders, into a contiguous
    [n, 3, H, W] tensor and into padded planes: rows padded by 16 B + 1 element (so the vector stores are off: scalar stores) or by 64 B,
    gaps between planes and frames, canaries before, between and after every plane"""
    sw, sh, dw, dh = 1920, 1080, 224, 224
    pics = [picture(orc, "NV12", 1, 1, sw, sh, dw, dh, 9300 + j) for j in range(3)]
    S = [DevPlanes(p[0]) for p in pics]
    srcs = [S[i % 3] for i in range(n)]
    for dtype in (0, 1, 2):
        e = ELEM[dtype]
        layouts = {"contiguous": dict(lead=0, tail=256),
                   "padded": dict(row=dw * e + 16 + e, plane=dh * (dw * e + 16 + e) + 40 * e, frame=3 * (dh * (dw * e + 16 + e) + 40 * e) + 8 * e, lead=24 * e),
                   "padded64": dict(row=dw * e + 64, plane=dh * (dw * e + 64) + 64, frame=3 * (dh * (dw * e + 64) + 64) + 256, lead=512)}
        for lname, geo in layouts.items():
            for bgr in (False, True):
                buf = TensorBuf(n, dw, dh, e, **geo)
                run_capi(capi, "NV12", 1, 1, sw, sh, dw, dh, srcs, dtype, bgr, "imagenet", buf, batch=n > 1)
                got, intact = buf.frames()
                what = f"n{n} dtype{dtype} {lname} bgr{bgr}"
                assert intact, what
                refs = [reference_bits(p[1], *PARAMS["imagenet"], dtype, bgr) for p in pics]
                for i in range(n):
                    assert_bits(got[i], refs[i % 3], f"{what} frame {i}")


def _nvc():
    sys.path.insert(0, os.path.join(ROOT, "videoprocessingframework_amd"))
    import PyNvCodec as nvc
    from videoprocessingframework_amd import PytorchNvCodec as pnc

    return nvc, pnc


def _upload(nvc, orc_planes, w, h):
    up = nvc.PyFrameUploader(w, h, nvc.PixelFormat.NV12, 0)
    return up.UploadSingleFrame(np.concatenate([p.reshape(-1) for p in orc_planes])).Clone(0)


def test_python_path_matches_the_torch_chain(orc):
    """to_normalized_tensor on 1080p NV12 -> 224 x 224 (BT.709 JPEG, ImageNet mean / std) == the chain users run today (ExecuteBatch into
    surface_from_tensor, then .float().div(255).sub(mean).div(std)) within 4x the largest |restatement - torch chain| over the 256 codes, and
    bit-identical to the restatement.  The result is consumed by a torch op right away (no synchronize in between); also a slice out[k:k+n]
    of a larger tensor, in every dtype, with the rest of that tensor untouched."""
    nvc, pnc = _nvc()
    PF = nvc.PixelFormat
    sw, sh, dw, dh, n = 1920, 1080, 224, 224, 5
    mean, std = PARAMS["imagenet"]
    cc = nvc.ColorspaceConversionContext(nvc.ColorSpace.BT_709, nvc.ColorRange.JPEG)
    pics = [picture(orc, "NV12", 1, 1, sw, sh, dw, dh, 9400 + i) for i in range(n)]
    surfs = [_upload(nvc, p[0], sw, sh) for p in pics]
    torch.cuda.synchronize()
    # tolerance: 4x the largest difference between the restatement fmaf(u8, scale, bias) and the torch chain over the 256 codes (CPU, fp32)
    codes = torch.arange(256, dtype=torch.float32)
    scale, bias = scale_bias_f32(mean, std)
    worst = 0.0
    for c in range(3):
        chain = codes.div(255).sub(mean[c]).div(std[c])
        rest = torch.from_numpy((np.arange(256, dtype=np.float64) * np.float64(scale[c]) + np.float64(bias[c])).astype(np.float32))
        worst = max(worst, float((chain - rest).abs().max()))
    tol = 4 * worst
    print("largest |restatement - chain| over the 256 codes", worst, "tolerance", tol)
    assert 0 < tol < 1e-5
    # the chain of today, on the resizer's own stream and then synchronised, as the samples do
    rs8 = nvc.PySurfaceConvertResizer(sw, sh, PF.NV12, dw, dh, PF.RGB_PLANAR, 0)
    u8 = torch.empty((n, 3, dh, dw), dtype=torch.uint8, device="cuda")
    assert rs8.ExecuteBatch(surfs, [pnc.surface_from_tensor(u8[i]) for i in range(n)], cc)
    torch.cuda.synchronize()
    m_t, s_t = torch.tensor(mean, device="cuda").view(1, 3, 1, 1), torch.tensor(std, device="cuda").view(1, 3, 1, 1)
    chain = u8.float().div(255).sub(m_t).div(s_t)
    # the new path: its own resizer on its own (non-blocking) stream; the result is consumed on torch's stream without a synchronize
    rs = nvc.PySurfaceConvertResizer(sw, sh, PF.NV12, dw, dh, PF.RGB_PLANAR, 0)
    out = pnc.to_normalized_tensor(rs, surfs, mean, std, cc_ctx=cc)
    consumed = out * 1.0
    assert tuple(out.shape) == (n, 3, dh, dw) and out.dtype == torch.float32
    diff = float((consumed - chain).abs().max())
    print("largest |to_normalized_tensor - chain|", diff)
    assert diff <= tol
    got = consumed.cpu().numpy().view(np.uint32)
    for i in range(n):
        assert_bits(got[i], reference_bits(pics[i][1], mean, std, 0, False), f"to_normalized_tensor frame {i}")
    # out = a slice of a larger tensor, every dtype, both channel orders: the rest of the larger tensor keeps its canary bits
    for dtype, tdt, bits in ((0, torch.float32, torch.int32), (1, torch.float16, torch.int16), (2, torch.bfloat16, torch.int16)):
        for bgr in (False, True):
            big = torch.full((n + 4, 3, dh, dw), 0x3C3C3C3C if bits == torch.int32 else 0x3C3C, dtype=bits, device="cuda")
            res = pnc.to_normalized_tensor(rs, surfs, mean, std, dtype=tdt, bgr=bgr, out=big.view(tdt)[2:2 + n], cc_ctx=cc)
            assert res.data_ptr() == big.view(tdt)[2:2 + n].data_ptr()
            h = big.cpu().numpy()
            h = h.view(np.uint32 if bits == torch.int32 else np.uint16)
            canary = 0x3C3C3C3C if bits == torch.int32 else 0x3C3C
            assert (h[:2] == canary).all() and (h[2 + n:] == canary).all(), (dtype, bgr)
            for i in range(n):
                assert_bits(h[2 + i], reference_bits(pics[i][1], mean, std, dtype, bgr), f"slice dtype{dtype} bgr{bgr} frame {i}")
    # the Task layer's colour rules hold: NV12 BT.601 MPEG is refused unless the extended colour spaces are on
    nvc.SetExtendedColorspaces(False)
    with pytest.raises(RuntimeError):
        pnc.to_normalized_tensor(rs, surfs, mean, std, cc_ctx=nvc.ColorspaceConversionContext(nvc.ColorSpace.BT_601, nvc.ColorRange.MPEG))
    with pytest.raises(ValueError):
        pnc.to_normalized_tensor(rs, surfs, mean, std, out=torch.empty((n, 3, dh, dw), dtype=torch.float16, device="cuda"))
    with pytest.raises(ValueError):
        pnc.to_normalized_tensor(rs, surfs, mean, std, out=torch.empty((n, 3, dh, dw + 1), dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError):
        pnc.to_normalized_tensor(rs, surfs, mean, std, out=torch.empty((n, 3, dw, dh), dtype=torch.float32, device="cuda").transpose(2, 3))


def test_graph_capture(orc):
    """the batched call captured in a torch.cuda.graph on one stream (the resizer's), replayed twice into a cleared output"""
    nvc, pnc = _nvc()
    PF = nvc.PixelFormat
    sw, sh, dw, dh, n = 1280, 720, 224, 224, 9
    mean, std = PARAMS["symmetric"]
    cc = nvc.ColorspaceConversionContext(nvc.ColorSpace.BT_709, nvc.ColorRange.MPEG)
    st = torch.cuda.Stream()
    rs = nvc.PySurfaceConvertResizer(sw, sh, PF.NV12, dw, dh, PF.RGB_PLANAR, 0, st.cuda_stream)
    pics = [picture(orc, "NV12", 1, 0, sw, sh, dw, dh, 9500 + i) for i in range(n)]
    surfs = [_upload(nvc, p[0], sw, sh) for p in pics]
    out = torch.zeros((n, 3, dh, dw), dtype=torch.float16, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        pnc.to_normalized_tensor(rs, surfs, mean, std, dtype=torch.float16, out=out, cc_ctx=cc)
    for rep in range(2):
        out.fill_(0)
        torch.cuda.synchronize()
        g.replay()
        st.synchronize()
        got = out.cpu().numpy().view(np.uint16)
        for i in range(n):
            assert_bits(got[i], reference_bits(pics[i][1], mean, std, 1, False), f"graph replay {rep} frame {i}")
