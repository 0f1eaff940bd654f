"""The fused multi-ROI crop + resize into a normalised tensor on the MI355X: vpf_convert_resize_tensor_rois, PySurfaceConvertResizer.ExecuteRoisToTensor
and PytorchNvCodec.rois_to_normalized_tensor.

Ground truth is the CPU oracle, composed as the definition says (tests/test_roi_tensor_cpu.py::roi_reference_u8, whose premise is checked there):
oracle.convert(frame -> RGB_PLANAR, FP32) of the WHOLE frame once per (frame, matrix), a numpy crop, oracle.resize(RGB_PLANAR, LINEAR, FP32), then
reference_bits of tests/test_gpu_tensor_out.py (fp64 evaluation of the fma, round to nearest even to the dtype).  Every element of every
output must be bit-identical; there is no tolerance.  Destinations hold canaries around every plane, which must survive."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from gpu_util import DevPlanes, stream_handle
from test_gpu_tensor_out import ELEM, MATRICES, PARAMS, TensorBuf, assert_bits, reference_bits
from test_roi_tensor_cpu import roi_reference_u8

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAME_SIZES = [(131, 79), (130, 78)]
ROI_CAP = 96  # jobs per job table (kRoiBatch, vpf_internal.h)


@pytest.fixture(scope="module")
def orc(oracle):
    oracle.set_threads(16)
    return oracle


_FRAMES, _RGB, _REFS = {}, {}, {}


def frame(orc, sf, W, H, seed=0):
    """(host planes, device planes) of one synthetic frame, once per (format, size, seed)"""
    key = (sf, W, H, seed)
    if key not in _FRAMES:
        src = orc.synth(getattr(orc, sf), W, H, 7700 + 13 * seed + W)
        _FRAMES[key] = (src, DevPlanes(src, align=64, extra=3))  # odd pitches: rows start at every alignment
    return _FRAMES[key]


def ref_u8(orc, sf, cs, cr, W, H, rect, dw, dh, seed=0):
    """[3, dh, dw] reference bytes of one job, computed once and shared (never modified)"""
    key = (sf, cs, cr, W, H, seed, rect, dw, dh)
    if key not in _REFS:
        fk = (sf, cs, cr, W, H, seed)
        if fk not in _RGB:
            st, rgb = orc.convert(getattr(orc, sf), orc.RGB_PLANAR, cs, cr, W, H, frame(orc, sf, W, H, seed)[0], orc.FP32)
            assert st == 0
            _RGB[fk] = rgb
        _REFS[key] = roi_reference_u8(orc, sf, cs, cr, W, H, None, rect, dw, dh, rgb=_RGB[fk])
        _REFS[key].setflags(write=False)
    return _REFS[key]


def run_rois(capi, sf, cs, cr, W, H, dw, dh, jobs, dtype, bgr, params, buf, plane_of=None):
    """jobs: [(DevPlanes of the frame, rect)]; job i writes buf.planes(i) (or plane_of(i))"""
    mean, std = PARAMS[params]
    norm = capi.make_tensor_norm(mean, std, dtype=dtype, bgr=bgr)
    rois = capi.make_rois([(dev.desc(), (plane_of or buf.planes)(i), rect) for i, (dev, rect) in enumerate(jobs)])
    capi.convert_resize_tensor_rois(capi.make_exec(stream_handle()), getattr(capi, sf), cs, cr, W, H, dw, dh, rois, norm)
    torch.cuda.synchronize()


@pytest.mark.parametrize("sf", ["NV12", "YUV420"])
@pytest.mark.parametrize("W,H", FRAME_SIZES)
def test_rect_geometry(capi, orc, sf, W, H):
    """one call to 64 x 128 f32: the whole frame, one pixel, odd offsets up-scaled, even offsets, a rect touching the right and bottom edges of the
    frame ((111, 69, 20, 10) on the odd-sized one), a rect one column in"""
    dw, dh, cs, cr = 64, 128, 1, 0
    dev = frame(orc, sf, W, H)[1]
    rects = [(0, 0, W, H), (0, 0, 1, 1), (17, 9, 55, 41), (16, 8, 56, 40), (W - 20, H - 10, 20, 10), (1, 0, 129, 78)]
    buf = TensorBuf(len(rects), dw, dh, 4)
    run_rois(capi, sf, cs, cr, W, H, dw, dh, [(dev, r) for r in rects], 0, False, "imagenet", buf)
    got, intact = buf.frames()
    assert intact
    for i, r in enumerate(rects):
        assert_bits(got[i], reference_bits(ref_u8(orc, sf, cs, cr, W, H, r, dw, dh), *PARAMS["imagenet"], 0, False), f"{sf} {W}x{H} rect {r}")


@pytest.mark.parametrize("sf", ["NV12", "YUV420"])
@pytest.mark.parametrize("W,H", FRAME_SIZES)
def test_identity_rect_is_the_plain_conversion(capi, orc, sf, W, H):
    """a rect equal to the destination size (identity scale) at odd and even offsets: the bytes must equal the plain conversion's.  (A call of its
    own: 64 x 128 does not fit these frames, so the destination here is 64 x 48, next to an up-scaled rect in the same call.)"""
    dw, dh, cs, cr = 64, 48, 1, 0
    dev = frame(orc, sf, W, H)[1]
    rects = [(33, 5, dw, dh), (17, 9, 55, 41), (W - dw, H - dh, dw, dh), (0, 0, dw, dh)]
    buf = TensorBuf(len(rects), dw, dh, 4)
    run_rois(capi, sf, cs, cr, W, H, dw, dh, [(dev, r) for r in rects], 0, False, "unit", buf)
    got, intact = buf.frames()
    assert intact
    st, rgb = orc.convert(getattr(orc, sf), orc.RGB_PLANAR, cs, cr, W, H, frame(orc, sf, W, H)[0], orc.FP32)
    assert st == 0
    for i, (x, y, w, h) in enumerate(rects):
        assert_bits(got[i], reference_bits(ref_u8(orc, sf, cs, cr, W, H, rects[i], dw, dh), *PARAMS["unit"], 0, False), f"{sf} {W}x{H} rect {rects[i]}")
        if (w, h) == (dw, dh):
            plain = np.stack([p[y:y + h, x:x + w] for p in rgb])
            assert_bits(got[i], reference_bits(plain, *PARAMS["unit"], 0, False), f"identity rect {rects[i]} == plain conversion")


@pytest.mark.parametrize("sf", ["NV12", "YUV420"])
@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_whole_frame_rect_equals_convert_resize_tensor(capi, orc, sf, dtype):
    """rect = the whole frame: bit-identical to vpf_convert_resize_tensor on the same frame, compared on the GPU, 130 x 78 -> 61 x 35"""
    W, H, dw, dh = 130, 78, 61, 35
    dev = frame(orc, sf, W, H)[1]
    a, b = TensorBuf(1, dw, dh, ELEM[dtype]), TensorBuf(1, dw, dh, ELEM[dtype])
    run_rois(capi, sf, 1, 1, W, H, dw, dh, [(dev, (0, 0, W, H))], dtype, True, "symmetric", a)
    norm = capi.make_tensor_norm(*PARAMS["symmetric"], dtype=dtype, bgr=True)
    capi.convert_resize_tensor(capi.make_exec(stream_handle()), getattr(capi, sf), 1, 1, W, H, dev.desc(), dw, dh, b.planes(0), norm)
    torch.cuda.synchronize()
    assert bool((a.buf == b.buf).all())
    got, intact = a.frames()
    assert intact
    assert_bits(got[0], reference_bits(ref_u8(orc, sf, 1, 1, W, H, (0, 0, W, H), dw, dh), *PARAMS["symmetric"], dtype, True), "whole frame")


@pytest.mark.parametrize("dw", [61, 64, 1])
@pytest.mark.parametrize("dtype", [0, 1])
def test_destination_widths_alignment_and_strides(capi, orc, dw, dtype):
    """destination widths with and without scalar tails; plane pointers one element off the vector alignment; padded row, plane and frame strides"""
    W, H, dh, sf = 131, 79, 37, "NV12"
    e = ELEM[dtype]
    dev = frame(orc, sf, W, H)[1]
    rects = [(17, 9, 55, 41), (0, 0, W, H), (111, 69, 20, 10)]
    layouts = {"contiguous": dict(lead=256),
               "off_by_one_element": dict(lead=256 + e),
               "padded": dict(row=dw * e + 16 + e, plane=dh * (dw * e + 16 + e) + 40 * e, frame=3 * (dh * (dw * e + 16 + e) + 40 * e) + 8 * e, lead=24 * e),
               "padded64": dict(row=dw * e + 64, plane=dh * (dw * e + 64) + 64, frame=3 * (dh * (dw * e + 64) + 64) + 256, lead=512)}
    for lname, geo in layouts.items():
        buf = TensorBuf(len(rects), dw, dh, e, **geo)
        run_rois(capi, sf, 1, 0, W, H, dw, dh, [(dev, r) for r in rects], dtype, False, "imagenet", buf)
        got, intact = buf.frames()
        assert intact, (lname, dw, dtype)
        for i, r in enumerate(rects):
            assert_bits(got[i], reference_bits(ref_u8(orc, sf, 1, 0, W, H, r, dw, dh), *PARAMS["imagenet"], dtype, False), f"{lname} dw{dw} dtype{dtype} rect {r}")


@pytest.mark.parametrize("sf", ["NV12", "YUV420"])
def test_dtypes_and_channel_orders(capi, orc, sf):
    W, H, dw, dh = 131, 79, 64, 48
    dev = frame(orc, sf, W, H)[1]
    rects = [(17, 9, 55, 41), (2, 3, 120, 70)]
    for dtype in (0, 1, 2):
        for bgr in (False, True):
            params = ("imagenet", "unit", "symmetric")[(dtype + bgr) % 3]
            buf = TensorBuf(len(rects), dw, dh, ELEM[dtype])
            run_rois(capi, sf, 1, 1, W, H, dw, dh, [(dev, r) for r in rects], dtype, bgr, params, buf)
            got, intact = buf.frames()
            assert intact
            for i, r in enumerate(rects):
                assert_bits(got[i], reference_bits(ref_u8(orc, sf, 1, 1, W, H, r, dw, dh), *PARAMS[params], dtype, bgr), f"{sf} dtype{dtype} bgr{bgr} rect {r}")


@pytest.mark.parametrize("cs,cr", MATRICES)
def test_matrices_f16(capi, orc, cs, cr):
    W, H, dw, dh = 130, 78, 64, 48
    for sf in ("NV12", "YUV420"):
        dev = frame(orc, sf, W, H)[1]
        rects = [(17, 9, 55, 41), (1, 0, 129, 78)]
        buf = TensorBuf(len(rects), dw, dh, 2)
        run_rois(capi, sf, cs, cr, W, H, dw, dh, [(dev, r) for r in rects], 1, False, "imagenet", buf)
        got, intact = buf.frames()
        assert intact
        for i, r in enumerate(rects):
            assert_bits(got[i], reference_bits(ref_u8(orc, sf, cs, cr, W, H, r, dw, dh), *PARAMS["imagenet"], 1, False), f"{sf} cs{cs} cr{cr} rect {r}")


def test_mixed_jobs_over_the_table_cap(capi, orc):
    """cap + 1 jobs over three frames in one call, sizes from 1 x 1 to the whole frame: a second job table, and staged and gather jobs (the
    large down-scale factors of a 12 x 10 destination) in the same call"""
    W, H, dw, dh, sf = 131, 79, 12, 10, "NV12"
    devs = [frame(orc, sf, W, H, seed)[1] for seed in range(3)]
    rng = np.random.default_rng(5)
    rects = [(0, 0, W, H), (0, 0, 1, 1), (130, 78, 1, 1), (17, 9, 55, 41), (5, 7, 13, 9), (1, 1, 20, 70), (3, 2, 100, 12)]
    while len(rects) < ROI_CAP + 1:
        w, h = int(rng.integers(1, W + 1)), int(rng.integers(1, H + 1))
        rects.append((int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1)), w, h))
    jobs = [(devs[i % 3], r) for i, r in enumerate(rects)]
    buf = TensorBuf(len(jobs), dw, dh, 4)
    run_rois(capi, sf, 1, 0, W, H, dw, dh, jobs, 0, False, "imagenet", buf)
    got, intact = buf.frames()
    assert intact
    for i, r in enumerate(rects):
        assert_bits(got[i], reference_bits(ref_u8(orc, sf, 1, 0, W, H, r, dw, dh, seed=i % 3), *PARAMS["imagenet"], 0, False), f"job {i} rect {r}")


def test_gather_form_and_kernel_selection(orc):
    """a child process with VPF_HIP_LOG=2: 1080p, rect (101, 53, 1500, 900) -> 224 x 224 takes the gather kernel, (17, 9, 55, 41) -> 64 x 128 the staged
    one; with VPF_TUNE_NV12_RGB_VARIANT = 9 the small case takes the gather kernel with identical bits.  The large case is checked against the oracle."""
    W, H = 1920, 1080
    src = orc.synth(orc.NV12, W, H, 7801)
    st, rgb = orc.convert(orc.NV12, orc.RGB_PLANAR, 1, 0, W, H, src, orc.FP32)
    assert st == 0
    big = (101, 53, 1500, 900)
    want_big = reference_bits(roi_reference_u8(orc, "NV12", 1, 0, W, H, None, big, 224, 224, rgb=rgb), *PARAMS["imagenet"], 0, False)
    want_small = reference_bits(roi_reference_u8(orc, "NV12", 1, 0, W, H, None, (17, 9, 55, 41), 64, 128, rgb=rgb), *PARAMS["imagenet"], 0, False)
    tmp = os.path.join(ROOT, "tests", "_build")
    os.makedirs(tmp, exist_ok=True)
    path = os.path.join(tmp, f"roi_child_{os.getpid()}.npz")
    np.savez(path, y=src[0], uv=src[1])
    code = f"""
import sys
sys.path.insert(0, {ROOT!r})
import numpy as np, torch
from videoprocessingframework_amd import capi
d = np.load({path!r})
y, uv = torch.from_numpy(d["y"]).cuda(), torch.from_numpy(d["uv"]).cuda()
src = [(y.data_ptr(), {W}), (uv.data_ptr(), {W})]
ex = capi.make_exec(torch.cuda.current_stream().cuda_stream)
norm = capi.make_tensor_norm({PARAMS["imagenet"][0]!r}, {PARAMS["imagenet"][1]!r})
outs = {{}}
for name, rects, dw, dh, variant in (("big", [{big!r}], 224, 224, 0), ("small", [(17, 9, 55, 41)], 64, 128, 0), ("small9", [(17, 9, 55, 41)], 64, 128, 9),
                                      ("mixed", [(17, 9, 55, 41), {big!r}, (16, 8, 56, 40)], 64, 128, 0)):
    out = torch.zeros((len(rects), 3, dh, dw), dtype=torch.float32, device="cuda")
    prev = capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, variant)
    print("CASE", name, file=sys.stderr, flush=True)
    capi.convert_resize_tensor_rois(ex, capi.NV12, 1, 0, {W}, {H}, dw, dh,
                                    capi.make_rois([(src, [(out[i, c].data_ptr(), 4 * dw) for c in range(3)], r) for i, r in enumerate(rects)]), norm)
    torch.cuda.synchronize()
    capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, prev)
    outs[name] = out.cpu().numpy().view(np.uint32)
np.savez({path!r}, **outs)
print("done")
"""
    try:
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, VPF_HIP_LOG="2"), timeout=120)
        assert r.returncode == 0 and "done" in r.stdout, r.stdout + r.stderr
        outs = dict(np.load(path))
    finally:
        if os.path.exists(path):
            os.remove(path)
    logs = {}
    for chunk in r.stderr.split("CASE ")[1:]:
        name, rest = chunk.split("\n", 1)
        logs[name.strip()] = [l for l in rest.split("\n") if "libvpfhip: launch" in l]
    print(logs)
    assert len(logs["big"]) == 1 and "k_roi_gather<" in logs["big"][0]
    assert len(logs["small"]) == 1 and "k_roi_strip<" in logs["small"][0]
    assert len(logs["small9"]) == 1 and "k_roi_gather<" in logs["small9"][0]
    assert len(logs["mixed"]) == 2 and "k_roi_strip<" in logs["mixed"][0] and "k_roi_gather<" in logs["mixed"][1]  # one call, both forms
    assert_bits(outs["big"][0], want_big, "gather form, 1500 x 900 -> 224 x 224")
    assert_bits(outs["small"][0], want_small, "staged form")
    assert_bits(outs["small9"][0], want_small, "gather form forced (variant 9)")
    assert_bits(outs["mixed"][0], want_small, "staged job of the mixed call")
    assert_bits(outs["mixed"][1], reference_bits(roi_reference_u8(orc, "NV12", 1, 0, W, H, None, big, 64, 128, rgb=rgb), *PARAMS["imagenet"], 0, False),
                "gather job of the mixed call")


def _nvc():
    sys.path.insert(0, os.path.join(ROOT, "videoprocessingframework_amd"))
    import PyNvCodec as nvc
    from videoprocessingframework_amd import PytorchNvCodec as pnc

    return nvc, pnc


def _upload(nvc, planes, w, h):
    up = nvc.PyFrameUploader(w, h, nvc.PixelFormat.NV12, 0)
    return up.UploadSingleFrame(np.concatenate([p.reshape(-1) for p in planes])).Clone(0)


def test_python_path(orc):
    """rois_to_normalized_tensor: a new tensor from a resizer on its own stream, consumed on torch's current stream without a host
    synchronisation; `out` as a slice of a larger batch; a CPU tensor [K, 5]; K = 0"""
    nvc, pnc = _nvc()
    PF = nvc.PixelFormat
    W, H, dw, dh = 130, 78, 64, 48
    mean, std = PARAMS["imagenet"]
    cc = nvc.ColorspaceConversionContext(nvc.ColorSpace.BT_709, nvc.ColorRange.JPEG)
    surfs = [_upload(nvc, frame(orc, "NV12", W, H, seed)[0], W, H) for seed in range(2)]
    torch.cuda.synchronize()
    rois = [(0, 17, 9, 55, 41), (1, 0, 0, W, H), (1, 1, 0, 129, 78), (0, 110, 68, 20, 10)]
    refs = [ref_u8(orc, "NV12", 1, 1, W, H, tuple(r[1:]), dw, dh, seed=r[0]) for r in rois]
    rs = nvc.PySurfaceConvertResizer(W, H, PF.NV12, dw, dh, PF.RGB_PLANAR, 0)  # its own non-blocking stream
    out = pnc.rois_to_normalized_tensor(rs, surfs, rois, mean, std, cc_ctx=cc)
    consumed = out * 1.0  # on torch's current stream, no synchronize in between
    assert tuple(out.shape) == (len(rois), 3, dh, dw) and out.dtype == torch.float32
    got = consumed.cpu().numpy().view(np.uint32)
    for i in range(len(rois)):
        assert_bits(got[i], reference_bits(refs[i], mean, std, 0, False), f"new tensor, job {i}")
    # a CPU tensor [K, 5], f16, B G R, into a slice of a larger batch whose other frames keep their canary bits
    big = torch.full((len(rois) + 3, 3, dh, dw), 0x3C3C, dtype=torch.int16, device="cuda")
    view = big.view(torch.float16)[2:2 + len(rois)]
    res = pnc.rois_to_normalized_tensor(rs, surfs, torch.tensor(rois, dtype=torch.int64), mean, std, dtype=torch.float16, bgr=True, out=view, cc_ctx=cc)
    assert res.data_ptr() == view.data_ptr()
    h = big.cpu().numpy().view(np.uint16)
    assert (h[:2] == 0x3C3C).all() and (h[2 + len(rois):] == 0x3C3C).all()
    for i in range(len(rois)):
        assert_bits(h[2 + i], reference_bits(refs[i], mean, std, 1, True), f"slice, job {i}")
    # K = 0: an empty tensor, nothing launched
    empty = pnc.rois_to_normalized_tensor(rs, surfs, [], mean, std, dtype=torch.bfloat16)
    assert tuple(empty.shape) == (0, 3, dh, dw) and empty.dtype == torch.bfloat16
    assert tuple(pnc.rois_to_normalized_tensor(rs, surfs, torch.empty((0, 5), dtype=torch.int32), mean, std).shape) == (0, 3, dh, dw)
    with pytest.raises(ValueError, match=r"\.cpu\(\)"):
        pnc.rois_to_normalized_tensor(rs, surfs, torch.tensor(rois, device="cuda"), mean, std)
    with pytest.raises(ValueError):
        pnc.rois_to_normalized_tensor(rs, surfs, [(0, 100, 9, 55, 41)], mean, std)
    with pytest.raises(ValueError):
        pnc.rois_to_normalized_tensor(rs, surfs, rois, mean, std, out=torch.empty((len(rois), 3, dh, dw), dtype=torch.float16, device="cuda"))


def test_graph_capture(orc):
    """one capture of the call on a single stream (the resizer's), one replay into a cleared output: the bits of the eager call"""
    nvc, pnc = _nvc()
    PF = nvc.PixelFormat
    W, H, dw, dh = 130, 78, 64, 48  # (even: an NV12 Surface of the Task layer is one plane of `width` bytes per row, chroma rows included)
    mean, std = PARAMS["symmetric"]
    cc = nvc.ColorspaceConversionContext(nvc.ColorSpace.BT_709, nvc.ColorRange.MPEG)
    st = torch.cuda.Stream()
    rs = nvc.PySurfaceConvertResizer(W, H, PF.NV12, dw, dh, PF.RGB_PLANAR, 0, st.cuda_stream)
    surfs = [_upload(nvc, frame(orc, "NV12", W, H, seed)[0], W, H) for seed in range(2)]
    rois = [(0, 17, 9, 55, 41), (1, 0, 0, W, H), (0, 110, 68, 20, 10), (1, 3, 3, 6, 70)]
    out = torch.zeros((len(rois), 3, dh, dw), dtype=torch.float16, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        eager = pnc.rois_to_normalized_tensor(rs, surfs, rois, mean, std, dtype=torch.float16, cc_ctx=cc)
    st.synchronize()
    eager_bits = eager.cpu().numpy().view(np.uint16)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        pnc.rois_to_normalized_tensor(rs, surfs, rois, mean, std, dtype=torch.float16, out=out, cc_ctx=cc)
    out.fill_(0)
    torch.cuda.synchronize()
    g.replay()
    st.synchronize()
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint16)
    assert_bits(got, eager_bits, "graph replay == eager call")
    for i, r in enumerate(rois):
        assert_bits(got[i], reference_bits(ref_u8(orc, "NV12", 1, 0, W, H, tuple(r[1:]), dw, dh, seed=r[0]), mean, std, 1, False), f"graph replay, job {i}")
