"""P10 / P12 sources of the fused tensor entries on the MI355X: vpf_convert_resize_tensor(_batch), vpf_convert_resize_tensor_rois,
vpf_convert_warp_tensor and the three PytorchNvCodec.*_to_normalized_tensor functions on P10 surfaces.

Ground truth is the CPU oracle, composed as the definition says (include/vpf_hip.h, "10 / 12-bit sources"): oracle.convert(P10 | P12 -> NV12) of the
frame, then the reference the 8-bit GPU tests use on that NV12 frame — oracle.convert_resize(NV12 -> RGB_PLANAR, FP32) for whole frames,
roi_reference_u8 for rectangles, warp_reference_u8 for warps —, then reference_bits (tests/test_gpu_tensor_out.py).  Every element of every output must
be bit-identical; there is no tolerance.  Sources are oracle.synth(P10): full-range random 16-bit samples, with the samples that sit on the edges of
(v + 128) >> 8 and of its saturation planted in luma and both chroma components (tests/test_p16_tensor_cpu.py::plant, whose premise is checked
there).  Destinations hold canaries around every plane (TensorBuf), which must survive.  Shapes are the smallest that reach each kernel form; the
kernel-selection log (VPF_HIP_LOG=2, a child process) names the form each of them takes."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from cases_fused_families import P16_WHOLE_CASES
from gpu_util import DevPlanes, stream_handle
from test_gpu_tensor_out import ELEM, MATRICES, PARAMS, TensorBuf, assert_bits, reference_bits
from test_gpu_warp_tensor import BORDER, geometry_jobs
from test_p16_tensor_cpu import plant
from test_roi_tensor_cpu import roi_reference_u8
from test_warp_tensor_cpu import warp_reference_u8

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAME_SIZES = [(131, 79), (130, 78)]

# whole frames: (name, sw, sh, dw, dh, frames, VPF_TUNE_NV12_RGB_VARIANT, (row alignment, extra pitch bytes), the label the selection log must carry)
WHOLE_CASES = P16_WHOLE_CASES
CASE = {c[0]: c for c in WHOLE_CASES}


@pytest.fixture(scope="module")
def orc(oracle):
    oracle.set_threads(16)
    return oracle


_SRC, _NV12, _WHOLE, _RGB = {}, {}, {}, {}


def p16_frame(orc, fmt, W, H, seed):
    """host planes of one planted synthetic P10 / P12 frame, once per key (never modified afterwards)"""
    key = (fmt, W, H, seed)
    if key not in _SRC:
        _SRC[key] = plant(orc.synth(getattr(orc, fmt), W, H, 5100 + 17 * seed + W))
    return _SRC[key]


def nv12_of(orc, fmt, W, H, seed):
    """step 1 of the definition: the NV12 planes oracle.convert(P10 | P12 -> NV12) writes for that frame"""
    key = (fmt, W, H, seed)
    if key not in _NV12:
        st, nv = orc.convert(getattr(orc, fmt), orc.NV12, 0, 0, W, H, p16_frame(orc, fmt, W, H, seed), orc.FP32)
        assert st == 0
        _NV12[key] = nv
    return _NV12[key]


def whole_u8(orc, fmt, cs, cr, sw, sh, dw, dh, seed):
    key = (fmt, cs, cr, sw, sh, dw, dh, seed)
    if key not in _WHOLE:
        st, want = orc.convert_resize(orc.NV12, orc.RGB_PLANAR, cs, cr, sw, sh, nv12_of(orc, fmt, sw, sh, seed), dw, dh, mode=orc.FP32)
        assert st == 0
        _WHOLE[key] = np.stack(want)
        _WHOLE[key].setflags(write=False)
    return _WHOLE[key]


def rgb_of(orc, fmt, cs, cr, W, H, seed):
    """the converted whole frame the ROI and warp references crop / sample"""
    key = (fmt, cs, cr, W, H, seed)
    if key not in _RGB:
        st, rgb = orc.convert(orc.NV12, orc.RGB_PLANAR, cs, cr, W, H, nv12_of(orc, fmt, W, H, seed), orc.FP32)
        assert st == 0
        _RGB[key] = rgb
    return _RGB[key]


def run_whole(capi, fmt, cs, cr, sw, sh, dw, dh, devs, dtype, bgr, params, buf, batch=True):
    norm = capi.make_tensor_norm(*PARAMS[params], dtype=dtype, bgr=bgr)
    ex = capi.make_exec(stream_handle())
    if batch:
        capi.convert_resize_tensor_batch(ex, getattr(capi, fmt), cs, cr, sw, sh, dw, dh, capi.make_batch([(d.desc(), buf.planes(i)) for i, d in enumerate(devs)]), norm)
    else:
        capi.convert_resize_tensor(ex, getattr(capi, fmt), cs, cr, sw, sh, devs[0].desc(), dw, dh, buf.planes(0), norm)
    torch.cuda.synchronize()


def whole_case(capi, orc, name, fmt="P10", cs=1, cr=0, dtype=0, bgr=False, params="imagenet"):
    """run one case of WHOLE_CASES -> its canary-checked output bits [n, 3, dh, dw], compared with the oracle"""
    _, sw, sh, dw, dh, n, variant, (align, extra), _ = CASE[name]
    seeds = list(range(min(n, 3)))
    devs = [DevPlanes(p16_frame(orc, fmt, sw, sh, s), align=align, extra=extra) for s in seeds]
    buf = TensorBuf(n, dw, dh, ELEM[dtype])
    prev = capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, variant)
    try:
        run_whole(capi, fmt, cs, cr, sw, sh, dw, dh, [devs[i % len(devs)] for i in range(n)], dtype, bgr, params, buf, batch=n > 1)
    finally:
        capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, prev)
    got, intact = buf.frames()
    what = f"{name} {fmt} cs{cs} cr{cr} dtype{dtype} bgr{bgr} {params}"
    assert intact, what
    refs = [reference_bits(whole_u8(orc, fmt, cs, cr, sw, sh, dw, dh, s), *PARAMS[params], dtype, bgr) for s in seeds]
    for i in range(n):
        assert_bits(got[i], refs[i % len(refs)], f"{what} frame {i}")
    return got


def test_every_form_is_selected():
    """the kernel-selection log (VPF_HIP_LOG=2, child process) carries exactly the label of the instantiation each whole-frame case takes
    (tests/cases_fused_families.py: family, FC_P16 -> FC_TENSOR, band height, the table of 32 or of 128 frames with the epilogue) and names the
    form the ROI call and the warp call take, in the default policy and with VPF_TUNE_NV12_RGB_VARIANT = 9, every one of them an FC_P16 instantiation"""
    code = f"""
import sys
sys.path.insert(0, {ROOT!r})
import torch
from videoprocessingframework_amd import capi
ex = capi.make_exec(torch.cuda.current_stream().cuda_stream)
norm = capi.make_tensor_norm((0, 0, 0), (1, 1, 1), dtype=1)
def planes(w, h, align, extra):
    p = (2 * w + align - 1) // align * align + extra
    y = torch.zeros(p * (h + (h + 1) // 2) + 64, dtype=torch.uint8, device="cuda")
    return y, [(y.data_ptr(), p), (y.data_ptr() + p * h, p)]
for name, sw, sh, dw, dh, n, variant, (align, extra) in {[c[:8] for c in WHOLE_CASES]!r}:
    keep, src = planes(sw, sh, align, extra)
    out = torch.empty((n, 3, dh, dw), dtype=torch.float16, device="cuda")
    prev = capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, variant)
    print("CASE", name, file=sys.stderr, flush=True)
    capi.convert_resize_tensor_batch(ex, capi.P10, 1, 0, sw, sh, dw, dh,
                                     capi.make_batch([(src, [(out[i, c].data_ptr(), 2 * dw) for c in range(3)]) for i in range(n)]), norm)
    torch.cuda.synchronize()
    capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, prev)
keep, src = planes(131, 79, 64, 2)
for variant in (0, 9):
    prev = capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, variant)
    out = torch.empty((1, 3, 128, 64), dtype=torch.float16, device="cuda")
    print("CASE", "roi%d" % variant, file=sys.stderr, flush=True)
    capi.convert_resize_tensor_rois(ex, capi.P10, 1, 0, 131, 79, 64, 128, capi.make_rois([(src, [(out[0, c].data_ptr(), 128) for c in range(3)], (17, 9, 55, 41))]), norm)
    torch.cuda.synchronize()
    out = torch.empty((1, 3, 35, 61), dtype=torch.float16, device="cuda")
    print("CASE", "warp%d" % variant, file=sys.stderr, flush=True)
    capi.convert_warp_tensor(ex, capi.P10, 1, 0, 131, 79, 61, 35, capi.make_warps([(src, [(out[0, c].data_ptr(), 122) for c in range(3)], (1, 0, 33, 0, 1, 5))]), norm)
    torch.cuda.synchronize()
    capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, prev)
print("done")
"""
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, VPF_HIP_LOG="2"), timeout=120)
    assert r.returncode == 0 and "done" in r.stdout, r.stdout + r.stderr
    logs = {}
    for chunk in r.stderr.split("CASE ")[1:]:
        name, rest = chunk.split("\n", 1)
        logs[name.strip()] = [l for l in rest.split("\n") if "libvpfhip: launch" in l]
    print(logs)
    for name, *_, label in WHOLE_CASES:
        assert len(logs[name]) == 1 and logs[name][0].split("launch ", 1)[1].strip() == label, (name, label, logs[name])
    assert "BatchArgsTE<128>" in logs["batch_33_large_table"][0] and "BatchArgsTE<128>" in logs["strip_r16_large_table"][0]
    for name, kernel in (("roi0", "k_roi_strip<7, 6>"), ("roi9", "k_roi_gather<7, 6>"), ("warp0", "k_warp_strip<7, 6>"), ("warp9", "k_warp_gather<7, 6>")):  # FC_P16 = 7, FC_TENSOR = 6
        assert len(logs[name]) == 1 and kernel in logs[name][0], (name, logs[name])


@pytest.mark.parametrize("name", [c[0] for c in WHOLE_CASES if c[0] != "gather_forced"])
def test_whole_frame_forms(capi, orc, name):
    """each form on P10, f32, R G B: bit-identical to the oracle, canaries intact"""
    whole_case(capi, orc, name)


def test_forced_gather_gives_the_strip_bits(capi, orc):
    """VPF_TUNE_NV12_RGB_VARIANT = 9 on the 160 x 96 case: the gather form, the oracle's bits, and so the strip form's"""
    assert np.array_equal(whole_case(capi, orc, "gather_forced"), whole_case(capi, orc, "strip_down_1_25"))


def test_dtypes_and_channel_orders(capi, orc):
    for name in ("strip_down_1_25", "half_across_chunks", "odd_sizes_pitch_plus_2"):
        for dtype in (0, 1, 2):
            for bgr in (False, True):
                whole_case(capi, orc, name, dtype=dtype, bgr=bgr, params=("imagenet", "unit", "symmetric")[(dtype + bgr) % 3])


@pytest.mark.parametrize("cs,cr", MATRICES)
def test_matrices(capi, orc, cs, cr):
    for name in ("half_across_chunks", "strip_up_2", "odd_3x"):
        whole_case(capi, orc, name, cs=cs, cr=cr, dtype=1)


def test_p12(capi, orc):
    """P12 is the same code: MSB-aligned samples whose low bits take part in the rounding"""
    for name in ("strip_down_1_25", "half_across_chunks", "odd_sizes_pitch_plus_2"):
        whole_case(capi, orc, name, fmt="P12")


def _chain_nv12(capi, dev, W, H, orc):
    """vpf_convert(P10 -> NV12) of device planes `dev` into fresh NV12 device planes"""
    nv = DevPlanes(orc.alloc(orc.NV12, W, H), align=64, extra=3)
    capi.convert(capi.make_exec(stream_handle()), capi.P10, capi.NV12, 0, 0, W, H, dev.desc(), nv.desc())
    return nv


def test_equals_the_chain_on_the_gpu(capi, orc):
    """one whole-frame case, one ROI call and one warp call: the P10 entry's destination buffer == the NV12 entry's on the planes
    vpf_convert(P10 -> NV12) wrote, compared on the GPU"""
    W, H = 131, 79
    dev = DevPlanes(p16_frame(orc, "P10", W, H, 0), align=64, extra=2)
    nv = _chain_nv12(capi, dev, W, H, orc)
    ex = capi.make_exec(stream_handle())
    norm = capi.make_tensor_norm(*PARAMS["imagenet"], dtype=1, bgr=True)
    for sw, sh, dw, dh in ((160, 96, 128, 80), (W, H, 61, 35)):
        d16 = DevPlanes(p16_frame(orc, "P10", sw, sh, 0), align=256 if sw == 160 else 64, extra=0 if sw == 160 else 2)
        d8 = _chain_nv12(capi, d16, sw, sh, orc)
        a, b = TensorBuf(1, dw, dh, 2), TensorBuf(1, dw, dh, 2)
        capi.convert_resize_tensor(ex, capi.P10, 1, 1, sw, sh, d16.desc(), dw, dh, a.planes(0), norm)
        capi.convert_resize_tensor(ex, capi.NV12, 1, 1, sw, sh, d8.desc(), dw, dh, b.planes(0), norm)
        torch.cuda.synchronize()
        assert torch.equal(a.buf, b.buf), (sw, sh)
    rects = [(0, 0, W, H), (17, 9, 55, 41), (W - 20, H - 10, 20, 10)]
    a, b = TensorBuf(len(rects), 64, 128, 2), TensorBuf(len(rects), 64, 128, 2)
    capi.convert_resize_tensor_rois(ex, capi.P10, 1, 1, W, H, 64, 128, capi.make_rois([(dev.desc(), a.planes(i), r) for i, r in enumerate(rects)]), norm)
    capi.convert_resize_tensor_rois(ex, capi.NV12, 1, 1, W, H, 64, 128, capi.make_rois([(nv.desc(), b.planes(i), r) for i, r in enumerate(rects)]), norm)
    torch.cuda.synchronize()
    assert torch.equal(a.buf, b.buf)
    ms = geometry_jobs(W, H, 61, 35)
    a, b = TensorBuf(len(ms), 61, 35, 2), TensorBuf(len(ms), 61, 35, 2)
    opts = capi.make_warp_opts(0, BORDER)
    capi.convert_warp_tensor(ex, capi.P10, 1, 1, W, H, 61, 35, capi.make_warps([(dev.desc(), a.planes(i), m) for i, m in enumerate(ms)]), norm, opts)
    capi.convert_warp_tensor(ex, capi.NV12, 1, 1, W, H, 61, 35, capi.make_warps([(nv.desc(), b.planes(i), m) for i, m in enumerate(ms)]), norm, opts)
    torch.cuda.synchronize()
    assert torch.equal(a.buf, b.buf)


# ------------------------------------------------------------------------------------------------ ROIs
def run_rois(capi, fmt, cs, cr, W, H, dw, dh, jobs, dtype, params, buf, variant=0):
    norm = capi.make_tensor_norm(*PARAMS[params], dtype=dtype)
    rois = capi.make_rois([(dev.desc(), buf.planes(i), rect) for i, (dev, rect) in enumerate(jobs)])
    prev = capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, variant)
    try:
        capi.convert_resize_tensor_rois(capi.make_exec(stream_handle()), getattr(capi, fmt), cs, cr, W, H, dw, dh, rois, norm)
        torch.cuda.synchronize()
    finally:
        capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, prev)


@pytest.mark.parametrize("W,H", FRAME_SIZES)
def test_roi_geometry_both_forms(capi, orc, W, H):
    """the rect list of tests/test_gpu_roi_tensor.py::test_rect_geometry -> 64 x 128 on frames whose rows are only 2-B aligned (pitch = round_up + 2):
    the whole frame, one pixel, odd and even corners, the rect touching the right and bottom edges; the staged form (default) and the gather form
    (VPF_TUNE_NV12_RGB_VARIANT = 9) give the oracle's bits"""
    dw, dh, cs, cr = 64, 128, 1, 0
    dev = DevPlanes(p16_frame(orc, "P10", W, H, 0), align=64, extra=2)
    rects = [(0, 0, W, H), (0, 0, 1, 1), (17, 9, 55, 41), (16, 8, 56, 40), (W - 20, H - 10, 20, 10), (1, 0, 129, 78)]
    rgb = rgb_of(orc, "P10", cs, cr, W, H, 0)
    want = [reference_bits(roi_reference_u8(orc, "NV12", cs, cr, W, H, None, r, dw, dh, rgb=rgb), *PARAMS["imagenet"], 0, False) for r in rects]
    outs = []
    for variant in (0, 9):
        buf = TensorBuf(len(rects), dw, dh, 4)
        run_rois(capi, "P10", cs, cr, W, H, dw, dh, [(dev, r) for r in rects], 0, "imagenet", buf, variant)
        got, intact = buf.frames()
        assert intact, variant
        for i, r in enumerate(rects):
            assert_bits(got[i], want[i], f"{W}x{H} variant {variant} rect {r}")
        outs.append(got)
    assert np.array_equal(outs[0], outs[1])


def test_roi_jobs_over_the_table_cap(capi, orc):
    """97 jobs over two frames in one call, 12 x 10 f16: a second job table, staged and gather jobs in one call, P12"""
    W, H, dw, dh = 131, 79, 12, 10
    devs = [DevPlanes(p16_frame(orc, "P12", W, H, s), align=64, extra=2) for s in range(2)]
    rng = np.random.default_rng(6)
    rects = [(0, 0, W, H), (0, 0, 1, 1), (130, 78, 1, 1), (17, 9, 55, 41), (5, 7, 13, 9), (1, 1, 20, 70), (3, 2, 100, 12)]
    while len(rects) < 97:
        w, h = int(rng.integers(1, W + 1)), int(rng.integers(1, H + 1))
        rects.append((int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1)), w, h))
    buf = TensorBuf(len(rects), dw, dh, 2)
    run_rois(capi, "P12", 1, 1, W, H, dw, dh, [(devs[i % 2], r) for i, r in enumerate(rects)], 1, "symmetric", buf)
    got, intact = buf.frames()
    assert intact
    for i, r in enumerate(rects):
        want = roi_reference_u8(orc, "NV12", 1, 1, W, H, None, r, dw, dh, rgb=rgb_of(orc, "P12", 1, 1, W, H, i % 2))
        assert_bits(got[i], reference_bits(want, *PARAMS["symmetric"], 1, False), f"job {i} rect {r}")


# ------------------------------------------------------------------------------------------------ warps
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("W,H", FRAME_SIZES)
def test_warp_geometry_both_forms(capi, orc, W, H, mode):
    """geometry_jobs of tests/test_gpu_warp_tensor.py (rotation, flips, shear, scales, the footprint wholly outside the frame) -> 61 x 35 f32, per
    border mode, staged and gather forms"""
    dw, dh, cs, cr = 61, 35, 1, 0
    dev = DevPlanes(p16_frame(orc, "P10", W, H, 1), align=64, extra=2)
    ms = geometry_jobs(W, H, dw, dh)
    rgb = rgb_of(orc, "P10", cs, cr, W, H, 1)
    want = [reference_bits(warp_reference_u8(orc, "NV12", cs, cr, W, H, m, dw, dh, BORDER, mode, rgb=rgb), *PARAMS["imagenet"], 0, False) for m in ms]
    norm = capi.make_tensor_norm(*PARAMS["imagenet"])
    outs = []
    for variant in (0, 9):
        buf = TensorBuf(len(ms), dw, dh, 4)
        prev = capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, variant)
        try:
            capi.convert_warp_tensor(capi.make_exec(stream_handle()), capi.P10, cs, cr, W, H, dw, dh,
                                     capi.make_warps([(dev.desc(), buf.planes(i), m) for i, m in enumerate(ms)]), norm, capi.make_warp_opts(mode, BORDER))
            torch.cuda.synchronize()
        finally:
            capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, prev)
        got, intact = buf.frames()
        assert intact, variant
        for i, m in enumerate(ms):
            assert_bits(got[i], want[i], f"{W}x{H} mode {mode} variant {variant} job {i} {m}")
        outs.append(got)
    assert np.array_equal(outs[0], outs[1])


# ------------------------------------------------------------------------------------------------ the Python path
def test_python_path_on_p10_surfaces(orc):
    """P10 Surfaces uploaded with PyFrameUploader through to_normalized_tensor, rois_to_normalized_tensor and warps_to_normalized_tensor of one
    P10 resizer; Execute of that resizer refuses"""
    sys.path.insert(0, os.path.join(ROOT, "videoprocessingframework_amd"))
    import PyNvCodec as nvc
    from videoprocessingframework_amd import PytorchNvCodec as pnc

    PF = nvc.PixelFormat
    W, H, dw, dh = 130, 78, 64, 48  # (even: a semi-planar Surface of the Task layer is one plane, chroma rows included)
    mean, std = PARAMS["imagenet"]
    cc = nvc.ColorspaceConversionContext(nvc.ColorSpace.BT_709, nvc.ColorRange.JPEG)
    up = nvc.PyFrameUploader(W, H, PF.P10, 0)
    surfs = [up.UploadSingleFrame(np.concatenate([p.reshape(-1) for p in p16_frame(orc, "P10", W, H, s)])).Clone(0) for s in range(2)]
    torch.cuda.synchronize()
    assert surfs[0].Format() == PF.P10
    rs = nvc.PySurfaceConvertResizer(W, H, PF.P10, dw, dh, PF.RGB_PLANAR, 0)
    out = pnc.to_normalized_tensor(rs, surfs, mean, std, cc_ctx=cc)
    got = (out * 1.0).cpu().numpy().view(np.uint32)
    for i in range(2):
        assert_bits(got[i], reference_bits(whole_u8(orc, "P10", 1, 1, W, H, dw, dh, i), mean, std, 0, False), f"to_normalized_tensor frame {i}")
    rois = [(0, 17, 9, 55, 41), (1, 0, 0, W, H), (1, 1, 0, 129, 78), (0, 110, 68, 20, 10)]
    out = pnc.rois_to_normalized_tensor(rs, surfs, rois, mean, std, dtype=torch.float16, bgr=True, cc_ctx=cc)
    got = (out * 1.0).cpu().numpy().view(np.uint16)
    for i, r in enumerate(rois):
        want = roi_reference_u8(orc, "NV12", 1, 1, W, H, None, tuple(r[1:]), dw, dh, rgb=rgb_of(orc, "P10", 1, 1, W, H, r[0]))
        assert_bits(got[i], reference_bits(want, mean, std, 1, True), f"rois_to_normalized_tensor job {i}")
    ms = geometry_jobs(W, H, dw, dh)[:5]
    index = [i % 2 for i in range(len(ms))]
    out = pnc.warps_to_normalized_tensor(rs, surfs, index, np.array(ms, dtype=np.float64).reshape(-1, 2, 3), mean, std, cc_ctx=cc, border=BORDER)
    got = (out * 1.0).cpu().numpy().view(np.uint32)
    for i, m in enumerate(ms):
        want = warp_reference_u8(orc, "NV12", 1, 1, W, H, m, dw, dh, BORDER, 0, rgb=rgb_of(orc, "P10", 1, 1, W, H, index[i]))
        assert_bits(got[i], reference_bits(want, mean, std, 0, False), f"warps_to_normalized_tensor job {i}")
    assert rs.Execute(surfs[0], cc).Empty()  # the 8-bit outputs take 8-bit sources
