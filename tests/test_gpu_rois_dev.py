"""The fused multi-ROI crop + resize with the rectangles in DEVICE memory on the MI355X: vpf_convert_resize_tensor_rois_dev,
PySurfaceConvertResizer.ExecuteRoisDevToTensor, PytorchNvCodec.device_rois_to_normalized_tensor and boxes_to_rois.

Ground truth is the HOST-TABLE entry (vpf_convert_resize_tensor_rois, itself held to the CPU oracle by tests/test_gpu_roi_tensor.py) on the same
rectangles into a buffer of the same layout: the two canary-filled buffers are compared on the device, byte for byte — every element, every
canary, no tolerance.  One case goes against the oracle chain directly (ref_u8 / reference_bits), so the two entries cannot drift together.
Which tiles of these calls are staged and which sample per tap is asserted on the CPU (tests/test_rois_dev_bounds_cpu.py, through the kernel's
own policy function): the GPU cannot tell, both forms give the same bits."""
import os
import sys

import numpy as np
import pytest
import torch

import cases_rois_dev as cases
import test_gpu_p16_tensor as p16
import test_gpu_roi_tensor as roi
from gpu_util import DevPlanes, stream_handle
from test_gpu_tensor_nhwc import NhwcBuf, hwc
from test_gpu_tensor_out import CANARY, ELEM, PARAMS, TensorBuf, assert_bits, reference_bits

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def orc(oracle):
    oracle.set_threads(16)
    return oracle


_P10 = {}


def frames_of(orc, sf, W, H):
    """the two device frames of a call (seeds 0 and 1), once per (format, size)"""
    if sf != "P10":
        return [roi.frame(orc, sf, W, H, seed)[1] for seed in range(2)]
    key = (W, H)
    if key not in _P10:
        _P10[key] = [DevPlanes(p16.p16_frame(orc, "P10", W, H, seed), align=64, extra=2) for seed in range(2)]  # rows only 2-B aligned
    return _P10[key]


def make_buf(n, dw, dh, dtype, nhwc, padded):
    e = ELEM[dtype]
    if nhwc:
        return NhwcBuf(n, dw, dh, e, **(dict(row=3 * dw * e + 16 + e, frame=dh * (3 * dw * e + 16 + e) + 24 * e, lead=24 * e) if padded else {}))
    return TensorBuf(n, dw, dh, e, **(dict(row=dw * e + 16 + e, plane=dh * (dw * e + 16 + e) + 40 * e, frame=3 * (dh * (dw * e + 16 + e) + 40 * e) + 8 * e,
                                           lead=24 * e) if padded else {}))


def run_host(capi, sf, cs, cr, W, H, dw, dh, devs, jobs, buf, dtype, bgr, params, nhwc, stream=None):
    """the host-table entry: jobs = [(job index, frame index, rect)], job k writes buf.planes(k)"""
    norm = capi.make_tensor_norm(*PARAMS[params], dtype=dtype, bgr=bgr, nhwc=nhwc)
    if jobs:
        rois = capi.make_rois([(devs[f].desc(), buf.planes(k), rect) for (k, f, rect) in jobs])
        capi.convert_resize_tensor_rois(capi.make_exec(stream or stream_handle()), getattr(capi, sf), cs, cr, W, H, dw, dh, rois, norm)


def run_dev(capi, sf, cs, cr, W, H, dw, dh, devs, boxes, buf, dtype, bgr, params, nhwc, count=None, max_n=None, stream=None):
    """the device entry: boxes = a device int32 tensor [K, >= 5] (its row stride is the box stride), count = a device int32 tensor or None"""
    norm = capi.make_tensor_norm(*PARAMS[params], dtype=dtype, bgr=bgr, nhwc=nhwc)
    table = capi.make_rois_dev(boxes.data_ptr(), boxes.shape[0] if max_n is None else max_n, buf.planes(0), buf.frame,
                               count.data_ptr() if count is not None else None, 4 * boxes.stride(0))
    capi.convert_resize_tensor_rois_dev(capi.make_exec(stream or stream_handle()), getattr(capi, sf), cs, cr, W, H, dw, dh,
                                        capi.make_frame_srcs([d.desc() for d in devs]), table, norm)


def boxes_tensor(jobs, width=5):
    """[(frame, rect)] -> device int32 [K, width], columns 5.. filled with a pattern the kernel must not read as geometry"""
    t = torch.full((len(jobs), width), 0x5A5A5A5A, dtype=torch.int32)
    t[:, :5] = torch.tensor([(f, *r) for (f, r) in jobs], dtype=torch.int32).reshape(-1, 5)
    return t.cuda()


def both(capi, orc, sf, W, H, dw, dh, rects, dtype, bgr, params, nhwc, padded, cs=1, cr=0):
    """one call of each entry on the same rectangles -> (device entry's buffer, host entry's buffer)"""
    devs = frames_of(orc, sf, W, H)
    jobs = [(cases.frame_of(i), r) for i, r in enumerate(rects)]
    a, b = make_buf(len(jobs), dw, dh, dtype, nhwc, padded), make_buf(len(jobs), dw, dh, dtype, nhwc, padded)
    run_dev(capi, sf, cs, cr, W, H, dw, dh, devs, boxes_tensor(jobs), a, dtype, bgr, params, nhwc)
    run_host(capi, sf, cs, cr, W, H, dw, dh, devs, [(k, f, r) for k, (f, r) in enumerate(jobs)], b, dtype, bgr, params, nhwc)
    torch.cuda.synchronize()
    return a, b


# (dtype, B G R, channels-last, padded rows) per destination size of cases.DST_SIZES
VARIANTS = {(64, 128): (0, False, False, False), (64, 48): (1, True, False, True), (300, 40): (2, False, True, False), (24, 16): (0, True, True, False)}


@pytest.mark.parametrize("sf", ["NV12", "YUV420", "P10"])
@pytest.mark.parametrize("W,H", cases.FRAME_SIZES)
def test_geometry(capi, orc, sf, W, H):
    """cases.geometry_rects per destination size, two frames interleaved, one dispatch each: the whole frame, one pixel, odd and even corners, the
    right and bottom edges, up-scales (staged tiles), the whole frame into 24 x 16 (per-tap tiles), and every side whose quotient a
    reciprocal-multiply would miss — byte for byte the host-table entry's buffer"""
    for (dw, dh) in cases.DST_SIZES:
        dtype, bgr, nhwc, padded = VARIANTS[(dw, dh)]
        rects = cases.geometry_rects(W, H, dw, dh)
        a, b = both(capi, orc, sf, W, H, dw, dh, rects, dtype, bgr, ("imagenet", "unit", "symmetric")[dtype], nhwc, padded)
        if not torch.equal(a.buf, b.buf):
            got, want = a.frames()[0], b.frames()[0]
            for i, r in enumerate(rects):
                assert_bits(got[i], want[i], f"{sf} {W}x{H} -> {dw}x{dh} job {i} rect {r}")
            raise AssertionError(f"{sf} {W}x{H} -> {dw}x{dh}: bytes outside the jobs' elements differ")
        assert a.frames()[1]


@pytest.mark.parametrize("dtype,bgr,nhwc,padded", [(0, False, False, True), (2, True, False, False), (1, False, True, True), (2, True, True, False),
                                                   (1, False, False, False), (0, False, True, True)])
def test_dtypes_orders_and_layouts(capi, orc, dtype, bgr, nhwc, padded):
    """the combinations test_geometry's rotation leaves out, NV12 131 x 79 into 64 x 48 and 24 x 16 (staged and per-tap tiles in both)"""
    W, H = 131, 79
    for (dw, dh) in ((64, 48), (24, 16)):
        rects = cases.geometry_rects(W, H, dw, dh)[:24]
        a, b = both(capi, orc, "NV12", W, H, dw, dh, rects, dtype, bgr, "imagenet", nhwc, padded, cs=0, cr=1)
        assert torch.equal(a.buf, b.buf), (dw, dh)
        assert a.frames()[1]


def test_against_the_oracle_chain(capi, orc):
    """the device entry against the CPU oracle directly (convert the whole frame, crop, resize, the fp64 evaluation of the epilogue): NV12 and P10,
    f32 planar and f16 channels-last, 64 x 48 and 24 x 16"""
    W, H = 131, 79
    for sf, dtype, nhwc, (dw, dh) in (("NV12", 0, False, (64, 48)), ("NV12", 1, True, (24, 16)), ("P10", 0, False, (24, 16))):
        rects = cases.geometry_rects(W, H, dw, dh)[:14]
        devs = frames_of(orc, sf, W, H)
        buf = make_buf(len(rects), dw, dh, dtype, nhwc, False)
        run_dev(capi, sf, 1, 0, W, H, dw, dh, devs, boxes_tensor([(cases.frame_of(i), r) for i, r in enumerate(rects)]), buf, dtype, False, "imagenet", nhwc)
        torch.cuda.synchronize()
        got, intact = buf.frames()
        assert intact
        for i, r in enumerate(rects):
            if sf == "P10":
                u8 = roi.roi_reference_u8(orc, "NV12", 1, 0, W, H, None, r, dw, dh, rgb=p16.rgb_of(orc, "P10", 1, 0, W, H, cases.frame_of(i)))
            else:
                u8 = roi.ref_u8(orc, sf, 1, 0, W, H, r, dw, dh, seed=cases.frame_of(i))
            want = reference_bits(u8, *PARAMS["imagenet"], dtype, False)
            assert_bits(got[i], hwc(want) if nhwc else want, f"{sf} dtype {dtype} nhwc {nhwc} job {i} rect {r}")


@pytest.mark.parametrize("sf,nhwc", [("NV12", False), ("YUV420", True), ("P10", False)])
def test_forced_per_tap_gives_the_same_bits(capi, orc, sf, nhwc):
    """VPF_TUNE_NV12_RGB_VARIANT = 9: no strip fits a dispatch without LDS, every tile samples per tap — the bits of the default call and of the host entry"""
    W, H, dw, dh = 131, 79, 64, 48
    rects = cases.geometry_rects(W, H, dw, dh)[:30]
    devs = frames_of(orc, sf, W, H)
    jobs = [(cases.frame_of(i), r) for i, r in enumerate(rects)]
    a, b = both(capi, orc, sf, W, H, dw, dh, rects, 0, False, "imagenet", nhwc, False)
    c = make_buf(len(jobs), dw, dh, 0, nhwc, False)
    prev = capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, 9)
    try:
        run_dev(capi, sf, 1, 0, W, H, dw, dh, devs, boxes_tensor(jobs), c, 0, False, "imagenet", nhwc)
        torch.cuda.synchronize()
    finally:
        capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, prev)
    assert capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, prev) == prev  # the knob is back
    assert torch.equal(a.buf, b.buf) and torch.equal(c.buf, a.buf)


@pytest.mark.parametrize("nhwc", [False, True])
def test_count(capi, orc, nhwc):
    """count = 0: nothing is written; 3 of 7: jobs 3 .. 6 keep their canaries; 9 > max_n: all 7; NULL: all 7; a padded table (box_stride = 32)"""
    W, H, dw, dh, sf, dtype = 130, 78, 64, 48, "NV12", 1
    devs = frames_of(orc, sf, W, H)
    rects = [(0, 0, W, H), (17, 9, 55, 41), (0, 0, 1, 1), (W - 20, H - 10, 20, 10), (5, 7, 13, 9), (1, 0, 129, 78), (16, 8, 56, 40)]
    jobs = [(cases.frame_of(i), r) for i, r in enumerate(rects)]
    want = {}
    for c in (3, 7):
        want[c] = make_buf(7, dw, dh, dtype, nhwc, True)
        run_host(capi, sf, 1, 1, W, H, dw, dh, devs, [(k, f, r) for k, (f, r) in enumerate(jobs[:c])], want[c], dtype, True, "symmetric", nhwc)
    for name, count, width, expect in (("zero", 0, 5, None), ("three", 3, 5, 3), ("nine", 9, 5, 7), ("null", None, 5, 7), ("stride32", 3, 8, 3),
                                        ("negative", -4, 5, None), ("stride32_null", None, 8, 7)):
        buf = make_buf(7, dw, dh, dtype, nhwc, True)
        boxes = boxes_tensor(jobs, width)
        assert boxes.stride(0) == width
        cnt = torch.tensor([count], dtype=torch.int32).cuda() if count is not None else None
        run_dev(capi, sf, 1, 1, W, H, dw, dh, devs, boxes, buf, dtype, True, "symmetric", nhwc, count=cnt)
        torch.cuda.synchronize()
        if expect is None:
            assert bool((buf.buf == CANARY).all()), name
        else:
            assert torch.equal(buf.buf, want[expect].buf), name


def test_spare_jobs_beyond_the_table(capi, orc):
    """max_n = 40 over a table of 5 boxes with count = 5: the 35 spare jobs read no box and write nothing (the buffer holds 5 jobs: a write of job 5
    would land in the canaries or behind the buffer)"""
    W, H, dw, dh, sf = 131, 79, 24, 16, "YUV420"
    devs = frames_of(orc, sf, W, H)
    rects = cases.geometry_rects(W, H, dw, dh)[:5]
    jobs = [(cases.frame_of(i), r) for i, r in enumerate(rects)]
    a, b = make_buf(5, dw, dh, 0, False, False), make_buf(5, dw, dh, 0, False, False)
    table = torch.full((40, 5), -7, dtype=torch.int32)
    table[:5] = torch.tensor([(f, *r) for (f, r) in jobs], dtype=torch.int32)
    run_dev(capi, sf, 1, 0, W, H, dw, dh, devs, table.cuda(), a, 0, False, "unit", False, count=torch.tensor([5], dtype=torch.int32).cuda())
    run_host(capi, sf, 1, 0, W, H, dw, dh, devs, [(k, f, r) for k, (f, r) in enumerate(jobs)], b, 0, False, "unit", False)
    torch.cuda.synchronize()
    assert torch.equal(a.buf, b.buf)


def test_graph_replays_with_live_boxes(capi, orc):
    """one call captured on a side stream (one stream, no parallel branches), replayed twice; boxes and count are overwritten on that stream between
    the replays: each replay equals the host entry on THAT replay's rectangles and count"""
    W, H, dw, dh, sf, dtype = 131, 79, 64, 48, "NV12", 0
    devs = frames_of(orc, sf, W, H)
    all_rects = cases.geometry_rects(W, H, dw, dh)
    sets = [([(cases.frame_of(i), r) for i, r in enumerate(all_rects[:6])], 6), ([(cases.frame_of(i + 1), r) for i, r in enumerate(all_rects[6:12])], 4)]
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        live = boxes_tensor(sets[0][0])
        count = torch.tensor([sets[0][1]], dtype=torch.int32).cuda()
        staged = [(boxes_tensor(j), torch.tensor([c], dtype=torch.int32).cuda()) for (j, c) in sets]
        buf = make_buf(6, dw, dh, dtype, False, False)
        run_dev(capi, sf, 1, 0, W, H, dw, dh, devs, live, buf, dtype, False, "imagenet", False, count=count, stream=st.cuda_stream)  # (eager once: the code object is loaded)
        st.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st):
            run_dev(capi, sf, 1, 0, W, H, dw, dh, devs, live, buf, dtype, False, "imagenet", False, count=count, stream=st.cuda_stream)
        for rep in (1, 0, 1):
            jobs, c = sets[rep]
            live.copy_(staged[rep][0])
            count.copy_(staged[rep][1])
            buf.buf.fill_(CANARY)
            g.replay()
            want = make_buf(6, dw, dh, dtype, False, False)
            run_host(capi, sf, 1, 0, W, H, dw, dh, devs, [(k, f, r) for k, (f, r) in enumerate(jobs[:c])], want, dtype, False, "imagenet", False, stream=st.cuda_stream)
            st.synchronize()
            assert torch.equal(buf.buf, want.buf), rep


def _nvc():
    sys.path.insert(0, os.path.join(ROOT, "videoprocessingframework_amd"))
    import PyNvCodec as nvc
    from videoprocessingframework_amd import PytorchNvCodec as pnc

    return nvc, pnc


def test_python_path(orc):
    """device_rois_to_normalized_tensor == rois_to_normalized_tensor (torch.equal) on the same rectangles: planar and channels_last, bf16, `out` as a slice
    of a larger tensor whose other frames keep their bits, a count, a slice of a wider box table, a P10 surface; boxes_to_rois on the device feeds it"""
    nvc, pnc = _nvc()
    PF = nvc.PixelFormat
    W, H, dw, dh = 130, 78, 64, 48  # (even: a semi-planar Surface of the Task layer is one plane, chroma rows included)
    mean, std = PARAMS["imagenet"]
    cc = nvc.ColorspaceConversionContext(nvc.ColorSpace.BT_709, nvc.ColorRange.JPEG)
    surfs = [roi._upload(nvc, roi.frame(orc, "NV12", W, H, seed)[0], W, H) for seed in range(2)]
    torch.cuda.synchronize()
    rois = [(0, 17, 9, 55, 41), (1, 0, 0, W, H), (1, 1, 0, 129, 78), (0, 110, 68, 20, 10), (1, 5, 7, 13, 9)]
    boxes = torch.tensor(rois, dtype=torch.int32).cuda()
    rs = nvc.PySurfaceConvertResizer(W, H, PF.NV12, dw, dh, PF.RGB_PLANAR, 0)  # its own non-blocking stream
    for kw in (dict(), dict(channels_last=True), dict(dtype=torch.bfloat16, bgr=True), dict(dtype=torch.float16, channels_last=True, bgr=True)):
        want = pnc.rois_to_normalized_tensor(rs, surfs, rois, mean, std, cc_ctx=cc, **kw)
        got = pnc.device_rois_to_normalized_tensor(rs, surfs, boxes, mean, std, cc_ctx=cc, **kw)
        assert got.shape == want.shape and got.dtype == want.dtype and got.stride() == want.stride(), kw
        assert torch.equal(got, want), kw
    # a count and a slice of a wider table, into a slice of a larger batch
    wide = torch.full((len(rois), 7), -1, dtype=torch.int32, device="cuda")
    wide[:, 1:6] = boxes
    big = torch.full((len(rois) + 3, 3, dh, dw), 0x3C3C, dtype=torch.int16, device="cuda")
    view = big.view(torch.float16)[2:2 + len(rois)]
    res = pnc.device_rois_to_normalized_tensor(rs, surfs, wide[:, 1:6], mean, std, count=torch.tensor([3], dtype=torch.int32, device="cuda"), dtype=torch.float16,
                                               out=view, cc_ctx=cc)
    assert res.data_ptr() == view.data_ptr()
    want = pnc.rois_to_normalized_tensor(rs, surfs, rois[:3], mean, std, dtype=torch.float16, cc_ctx=cc)
    assert torch.equal(view[:3], want)
    assert bool((big[:2] == 0x3C3C).all()) and bool((big[5:] == 0x3C3C).all())   # rows at or behind the count are not written
    # a detector's float boxes, turned into the table on the device
    xyxy = torch.tensor([[17.0, 9.0, 72.0, 50.0], [16.6, 8.2, 71.3, 49.9], [-4.0, -4.0, 200.0, 100.0], [110.5, 68.5, 129.2, 77.1], [float("nan"), 0.0, 9.0, 9.0]],
                        device="cuda")
    idx = torch.tensor([0, 1, 1, 0, 1], device="cuda")
    table = pnc.boxes_to_rois(xyxy, idx, W, H)
    assert table.is_cuda and table.dtype == torch.int32
    host = table.cpu().tolist()
    assert host[:4] == [[0, 17, 9, 55, 41], [1, 16, 8, 56, 42], [1, 0, 0, W, H], [0, 110, 68, 20, 10]] and host[4][3:] == [0, 0]
    got = pnc.device_rois_to_normalized_tensor(rs, surfs, table, mean, std, cc_ctx=cc)
    want = pnc.rois_to_normalized_tensor(rs, surfs, host[:4], mean, std, cc_ctx=cc)
    assert torch.equal(got[:4], want)
    zero = torch.from_numpy(reference_bits(np.zeros((3, dh, dw), np.uint8), mean, std, 0, False).view(np.float32)).cuda()
    assert torch.equal(got[4], zero)                                             # the NaN box: an invalid job, normalised zeros
    # a P10 surface
    up = nvc.PyFrameUploader(W, H, PF.P10, 0)
    p10 = [up.UploadSingleFrame(np.concatenate([p.reshape(-1) for p in p16.p16_frame(orc, "P10", W, H, s)])).Clone(0) for s in range(2)]
    torch.cuda.synchronize()
    rs10 = nvc.PySurfaceConvertResizer(W, H, PF.P10, dw, dh, PF.RGB_PLANAR, 0)
    want = pnc.rois_to_normalized_tensor(rs10, p10, rois, mean, std, dtype=torch.float16, cc_ctx=cc)
    got = pnc.device_rois_to_normalized_tensor(rs10, p10, boxes, mean, std, dtype=torch.float16, cc_ctx=cc)
    assert torch.equal(got, want)
    with pytest.raises(ValueError):
        pnc.device_rois_to_normalized_tensor(rs, surfs, boxes.cpu(), mean, std)
    with pytest.raises(ValueError):
        pnc.device_rois_to_normalized_tensor(rs, surfs, boxes.to(torch.int64), mean, std)
    with pytest.raises(ValueError):
        pnc.device_rois_to_normalized_tensor(rs, surfs, boxes, mean, std, count=torch.tensor([3], dtype=torch.int32))
    with pytest.raises(ValueError, match=r"\.cpu\(\)"):
        pnc.rois_to_normalized_tensor(rs, surfs, boxes, mean, std)               # the host-table entry refuses device boxes as before


def test_invalid_boxes_are_zero_filled(capi, orc):
    """w = 0, h = -3, x = -1, x + w = W + 1, y + h = H + 2, frame -1 and frame n_frames, INT32 extremes, among valid boxes: an invalid job is the
    epilogue of byte 0 in every element, the valid jobs are the host entry's, the canaries are intact.  (The guard itself is proven on the CPU,
    tests/test_rois_dev_bounds_cpu.py: this checks the fill.)"""
    W, H, dw, dh, sf = 131, 79, 64, 48, "NV12"
    devs = frames_of(orc, sf, W, H)
    table = [(0, (17, 9, 55, 41)), (1, (3, 5, 0, 10)), (0, (3, 5, 20, -3)), (1, (0, 0, W, H)), (0, (-1, 5, 20, 10)), (1, (W - 19, 5, 20, 10)),
             (0, (W - 20, H - 10, 20, 10)), (1, (3, H - 8, 20, 10)), (-1, (3, 5, 20, 10)), (2, (3, 5, 20, 10)), (1, (5, 7, 13, 9)),
             (0, (2 ** 31 - 1, 0, 2 ** 31 - 1, 1)), (0, (0, -2 ** 31, 1, 1)), (0, (1, 1, -2 ** 31, 2)), (1, (W - 1, H - 1, 1, 1)), (0, (0, 0, W + 1, H))]
    valid = [0 <= f < 2 and w >= 1 and h >= 1 and x >= 0 and y >= 0 and x + w <= W and y + h <= H for (f, (x, y, w, h)) in table]
    assert sum(valid) == 5 and len(table) - sum(valid) == 11
    for dtype, bgr, nhwc, padded in ((0, False, False, False), (2, True, True, True), (1, True, False, True)):
        a, b = make_buf(len(table), dw, dh, dtype, nhwc, padded), make_buf(len(table), dw, dh, dtype, nhwc, padded)
        run_dev(capi, sf, 1, 0, W, H, dw, dh, devs, boxes_tensor(table), a, dtype, bgr, "imagenet", nhwc)
        run_host(capi, sf, 1, 0, W, H, dw, dh, devs, [(k, f, r) for k, (f, r) in enumerate(table) if valid[k]], b, dtype, bgr, "imagenet", nhwc)
        torch.cuda.synchronize()
        got, intact = a.frames()
        want = b.frames()[0]
        assert intact
        zero = reference_bits(np.zeros((3, dh, dw), np.uint8), *PARAMS["imagenet"], dtype, bgr)
        zero = hwc(zero) if nhwc else zero
        for k in range(len(table)):
            assert_bits(got[k], want[k] if valid[k] else zero, f"dtype {dtype} bgr {bgr} nhwc {nhwc} job {k} {table[k]} valid {valid[k]}")
