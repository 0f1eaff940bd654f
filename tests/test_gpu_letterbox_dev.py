"""The fused letterbox with the boxes in DEVICE memory on the MI355X: vpf_convert_letterbox_tensor_dev, PySurfaceConvertResizer.ExecuteLetterboxDevToTensor,
PytorchNvCodec.device_letterbox_to_normalized_tensor and letterbox_fit_boxes.

Ground truth is the HOST-TABLE entry (vpf_convert_letterbox_tensor, itself held to the CPU oracle by tests/test_gpu_letterbox_tensor.py) on the same
rectangles and placements into a buffer of the same layout: the two canary-filled buffers are compared on the device, byte for byte — every element,
every canary, no tolerance.  One case goes against the oracle chain directly (ref_u8 / reference_bits and test_gpu_letterbox_tensor's composition), so
the two entries cannot drift together.  Which tiles of these calls are padded, staged or sampled per tap is asserted on the CPU
(tests/test_letterbox_dev_cpu.py, through the kernel's own policy function): the GPU cannot tell, every form gives the same bits."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cases_letterbox_dev as cases
import test_gpu_p16_tensor as p16
import test_gpu_roi_tensor as roi
from gpu_util import stream_handle
from test_gpu_letterbox_tensor import lb_ref, place
from test_gpu_rois_dev import boxes_tensor, frames_of, make_buf
from test_gpu_rois_dev import run_dev as run_rois_dev
from test_gpu_tensor_nhwc import hwc
from test_gpu_tensor_out import CANARY, PARAMS, assert_bits, reference_bits

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = cases.PAD
_FIRST = int(os.environ.get("VPF_FUZZ_FIRST", "0"))
_FUZZ_SEEDS = range(_FIRST, _FIRST + int(os.environ.get("VPF_FUZZ_SEEDS", str(cases.FUZZ_DEFAULT))))


@pytest.fixture(scope="module")
def orc(oracle):
    oracle.set_threads(16)
    return oracle


def run_host(capi, sf, cs, cr, W, H, dw, dh, devs, jobs, buf, dtype, bgr, params, nhwc, pad=PAD, stream=None):
    """the host-table entry: jobs = [(job index, frame index, rect, dst_rect)], job k writes buf.planes(k)"""
    norm = capi.make_tensor_norm(*PARAMS[params], dtype=dtype, bgr=bgr, nhwc=nhwc)
    if jobs:
        arr = capi.make_letterbox_jobs([(devs[f].desc(), buf.planes(k), rect, drect) for (k, f, rect, drect) in jobs])
        capi.convert_letterbox_tensor(capi.make_exec(stream or stream_handle()), getattr(capi, sf), cs, cr, W, H, dw, dh, arr, norm,
                                      capi.make_letterbox_opts(pad) if pad is not None else None)


def run_dev(capi, sf, cs, cr, W, H, dw, dh, devs, boxes, buf, dtype, bgr, params, nhwc, rects=None, count=None, max_n=None, pad=PAD, stream=None):
    """the device entry: boxes = a device int32 tensor [K, >= 5], rects = a device int32 tensor [K, >= 4] or None (their row strides are the table
    strides), count = a device int32 tensor or None"""
    norm = capi.make_tensor_norm(*PARAMS[params], dtype=dtype, bgr=bgr, nhwc=nhwc)
    table = capi.make_letterbox_dev(boxes.data_ptr(), boxes.shape[0] if max_n is None else max_n, buf.planes(0), buf.frame,
                                    count.data_ptr() if count is not None else None, rects.data_ptr() if rects is not None else None,
                                    4 * boxes.stride(0), 4 * rects.stride(0) if rects is not None else 16)
    capi.convert_letterbox_tensor_dev(capi.make_exec(stream or stream_handle()), getattr(capi, sf), cs, cr, W, H, dw, dh,
                                      capi.make_frame_srcs([d.desc() for d in devs]), table, norm, capi.make_letterbox_opts(pad) if pad is not None else None)


def rects_tensor(rects, width=4):
    """[(ix, iy, iw, ih)] -> device int32 [K, width], columns 4.. filled with a pattern the kernel must not read as geometry"""
    t = torch.full((len(rects), width), 0x5A5A5A5A, dtype=torch.int32)
    t[:, :4] = torch.tensor(rects, dtype=torch.int32).reshape(-1, 4)
    return t.cuda()


def pad_frame(dw, dh, dtype, bgr, nhwc, params, pad=PAD):
    """the bits of a job that shows no picture: the epilogue of pad[c] in every element of OUTPUT channel c"""
    u8 = np.empty((3, dh, dw), np.uint8)
    for k in range(3):
        u8[k] = pad[2 - k] if bgr else pad[k]
    bits = reference_bits(u8, *PARAMS[params], dtype, bgr)
    return hwc(bits) if nhwc else bits


def both(capi, orc, sf, W, H, dw, dh, rects, dtype, bgr, params, nhwc, padded, drects=None, cs=1, cr=0, rect_width=4):
    """one call of each entry on the same rectangles -> (device entry's buffer, host entry's buffer); drects None: the kernel fits, the host entry gets
    vpf_letterbox_fit's placements"""
    devs = frames_of(orc, sf, W, H)
    jobs = [(cases.frame_of(i), r) for i, r in enumerate(rects)]
    a, b = make_buf(len(jobs), dw, dh, dtype, nhwc, padded), make_buf(len(jobs), dw, dh, dtype, nhwc, padded)
    run_dev(capi, sf, cs, cr, W, H, dw, dh, devs, boxes_tensor(jobs), a, dtype, bgr, params, nhwc,
            rects=rects_tensor(drects, rect_width) if drects is not None else None)
    placed = drects if drects is not None else [capi.letterbox_fit(r[2], r[3], dw, dh) for r in rects]
    run_host(capi, sf, cs, cr, W, H, dw, dh, devs, [(k, f, r, placed[k]) for k, (f, r) in enumerate(jobs)], b, dtype, bgr, params, nhwc)
    torch.cuda.synchronize()
    return a, b


# (dtype, B G R, channels-last, padded rows) per destination size of cases.DST_SIZES
VARIANTS = {(64, 48): (1, True, False, True), (300, 40): (2, False, True, False), (24, 16): (0, True, True, False), (17, 33): (0, False, False, True)}


@pytest.mark.parametrize("sf", cases.SOURCES)
@pytest.mark.parametrize("W,H", cases.FRAME_SIZES)
def test_geometry(capi, orc, sf, W, H):
    """cases.geometry_rects per destination size, two frames interleaved, one dispatch each, the kernel's own fit: byte for byte the host-table entry's
    buffer with vpf_letterbox_fit's placements"""
    for (dw, dh) in cases.DST_SIZES:
        dtype, bgr, nhwc, padded = VARIANTS[(dw, dh)]
        rects = cases.geometry_rects(W, H, dw, dh)
        a, b = both(capi, orc, sf, W, H, dw, dh, rects, dtype, bgr, ("imagenet", "unit", "symmetric")[dtype], nhwc, padded)
        if not torch.equal(a.buf, b.buf):
            got, want = a.frames()[0], b.frames()[0]
            for i, r in enumerate(rects):
                assert_bits(got[i], want[i], f"{sf} {W}x{H} -> {dw}x{dh} job {i} rect {r} fit {capi.letterbox_fit(r[2], r[3], dw, dh)}")
            raise AssertionError(f"{sf} {W}x{H} -> {dw}x{dh}: bytes outside the jobs' elements differ")
        assert a.frames()[1]


@pytest.mark.parametrize("dtype,bgr,nhwc,padded", [(0, False, False, False), (2, True, False, True), (1, False, True, True), (2, True, True, False),
                                                   (1, False, False, False), (0, False, True, True)])
def test_dtypes_orders_and_layouts(capi, orc, dtype, bgr, nhwc, padded):
    """the combinations test_geometry's rotation leaves out, NV12 131 x 79 into 64 x 48 and 24 x 16"""
    W, H = 131, 79
    for (dw, dh) in ((64, 48), (24, 16)):
        a, b = both(capi, orc, "NV12", W, H, dw, dh, cases.geometry_rects(W, H, dw, dh), dtype, bgr, "imagenet", nhwc, padded, cs=0, cr=1)
        assert torch.equal(a.buf, b.buf), (dw, dh)
        assert a.frames()[1]


def test_exact_aspect_equals_the_device_roi_entry(capi, orc):
    """boxes of the destination's exact aspect: the fit is the whole plane, nothing is padded, and the buffer is vpf_convert_resize_tensor_rois_dev's"""
    W, H = 131, 79
    for sf, (dw, dh) in (("NV12", (64, 48)), ("YUV420", (300, 40)), ("P10", (24, 16)), ("NV12", (17, 33))):
        dtype, bgr, nhwc, padded = VARIANTS[(dw, dh)]
        aw, ah = cases.ASPECT[(dw, dh)]
        assert capi.letterbox_fit(aw, ah, dw, dh) == (0, 0, dw, dh)
        jobs = [(cases.frame_of(i), (x, y, aw, ah)) for i, (x, y) in enumerate(((0, 0), (5, 3), (96 - aw, 64 - ah)))]
        devs = frames_of(orc, sf, W, H)
        a, b = make_buf(len(jobs), dw, dh, dtype, nhwc, padded), make_buf(len(jobs), dw, dh, dtype, nhwc, padded)
        run_dev(capi, sf, 1, 0, W, H, dw, dh, devs, boxes_tensor(jobs), a, dtype, bgr, "imagenet", nhwc)
        run_rois_dev(capi, sf, 1, 0, W, H, dw, dh, devs, boxes_tensor(jobs), b, dtype, bgr, "imagenet", nhwc)
        torch.cuda.synchronize()
        assert torch.equal(a.buf, b.buf), (sf, dw, dh)


def test_against_the_oracle_chain(capi, orc):
    """the device entry against the CPU oracle directly (convert the whole frame, crop, resize to the fit, place, the fp64 evaluation of the epilogue):
    NV12 and P10, f32 planar and f16 channels-last, fitted and explicit placements"""
    W, H = 131, 79
    for sf, dtype, nhwc, (dw, dh), explicit in (("NV12", 0, False, (64, 48), False), ("NV12", 1, True, (24, 16), True), ("P10", 0, False, (17, 33), False)):
        rects = cases.geometry_rects(W, H, dw, dh)
        drects = cases.explicit_rects(dw, dh, len(rects)) if explicit else [capi.letterbox_fit(r[2], r[3], dw, dh) for r in rects]
        devs = frames_of(orc, sf, W, H)
        buf = make_buf(len(rects), dw, dh, dtype, nhwc, False)
        run_dev(capi, sf, 1, 0, W, H, dw, dh, devs, boxes_tensor([(cases.frame_of(i), r) for i, r in enumerate(rects)]), buf, dtype, False, "imagenet", nhwc,
                rects=rects_tensor(drects) if explicit else None)
        torch.cuda.synchronize()
        got, intact = buf.frames()
        assert intact
        for i, (r, d) in enumerate(zip(rects, drects)):
            if sf == "P10":
                inner = roi.roi_reference_u8(orc, "NV12", 1, 0, W, H, None, r, d[2], d[3], rgb=p16.rgb_of(orc, "P10", 1, 0, W, H, cases.frame_of(i)))
                u8 = place(inner, d, dw, dh, PAD)
            else:
                u8 = lb_ref(orc, sf, 1, 0, W, H, r, d, dw, dh, PAD, seed=cases.frame_of(i))
            want = reference_bits(u8, *PARAMS["imagenet"], dtype, False)
            assert_bits(got[i], hwc(want) if nhwc else want, f"{sf} dtype {dtype} nhwc {nhwc} job {i} rect {r} dst_rect {d}")


@pytest.mark.parametrize("sf,dw,dh,dtype,bgr,nhwc", [("NV12", 64, 48, 0, False, False), ("YUV420", 300, 40, 1, True, True), ("P10", 17, 33, 2, False, False)])
def test_explicit_placements(capi, orc, sf, dw, dh, dtype, bgr, nhwc):
    """dst_rects in device memory, rows 24 bytes apart, odd ix and iy: bit-equal to the host-table entry with those placements"""
    W, H = 131, 79
    rects = cases.geometry_rects(W, H, dw, dh)
    drects = cases.explicit_rects(dw, dh, len(rects))
    assert any(d[0] % 2 and d[1] % 2 for d in drects)
    a, b = both(capi, orc, sf, W, H, dw, dh, rects, dtype, bgr, "imagenet", nhwc, True, drects=drects, rect_width=6)
    assert torch.equal(a.buf, b.buf)
    assert a.frames()[1]


def test_fit_boxes_as_explicit_placements(capi, orc):
    """dst_rects = letterbox_fit_boxes(boxes) is bit-equal to the dst_rects = NULL path: the torch table is the kernel's fit"""
    from videoprocessingframework_amd import PytorchNvCodec as pnc

    W, H, sf = 131, 79, "NV12"
    devs = frames_of(orc, sf, W, H)
    for (dw, dh) in cases.DST_SIZES:
        dtype, bgr, nhwc, padded = VARIANTS[(dw, dh)]
        jobs = [(cases.frame_of(i), r) for i, r in enumerate(cases.geometry_rects(W, H, dw, dh))]
        boxes = boxes_tensor(jobs)
        table = pnc.letterbox_fit_boxes(boxes, dw, dh)
        assert table.is_cuda and table.dtype == torch.int32 and tuple(table.shape) == (len(jobs), 4)
        a, b = make_buf(len(jobs), dw, dh, dtype, nhwc, padded), make_buf(len(jobs), dw, dh, dtype, nhwc, padded)
        run_dev(capi, sf, 1, 0, W, H, dw, dh, devs, boxes, a, dtype, bgr, "imagenet", nhwc)
        run_dev(capi, sf, 1, 0, W, H, dw, dh, devs, boxes, b, dtype, bgr, "imagenet", nhwc, rects=table)
        torch.cuda.synchronize()
        assert torch.equal(a.buf, b.buf), (dw, dh)
        assert table.cpu().tolist() == [list(capi.letterbox_fit(r[2], r[3], dw, dh)) for (_, r) in jobs]


@pytest.mark.parametrize("sf,nhwc,dw,dh", [("NV12", False, 64, 48), ("YUV420", True, 300, 40), ("P10", False, 64, 48)])
def test_forced_per_tap_gives_the_same_bits(capi, orc, sf, nhwc, dw, dh):
    """VPF_TUNE_NV12_RGB_VARIANT = 9: no strip fits a dispatch without LDS, every tile that shows picture samples per tap — the bits of the default call
    and of the host entry"""
    W, H = 131, 79
    rects = cases.geometry_rects(W, H, dw, dh)
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
    """count = 0 and negative: nothing is written; 3 of 7: jobs 3 .. 6 keep their canaries; 9 > max_n: all 7; NULL: all 7; padded tables"""
    W, H, dw, dh, sf, dtype = 96, 64, 64, 48, "NV12", 1
    devs = frames_of(orc, sf, W, H)
    rects = [(0, 0, W, H), (17, 9, 55, 41), (0, 0, 1, 1), (W - 20, H - 10, 20, 10), (5, 7, 13, 9), (5, 3, 3, 60), (16, 8, 56, 40)]
    jobs = [(cases.frame_of(i), r) for i, r in enumerate(rects)]
    placed = [capi.letterbox_fit(r[2], r[3], dw, dh) for r in rects]
    want = {}
    for c in (3, 7):
        want[c] = make_buf(7, dw, dh, dtype, nhwc, True)
        run_host(capi, sf, 1, 1, W, H, dw, dh, devs, [(k, f, r, placed[k]) for k, (f, r) in enumerate(jobs[:c])], want[c], dtype, True, "symmetric", nhwc)
    for name, count, width, explicit, expect in (("zero", 0, 5, False, None), ("three", 3, 5, False, 3), ("nine", 9, 5, True, 7), ("null", None, 5, False, 7),
                                                  ("stride32", 3, 8, True, 3), ("negative", -4, 5, True, None), ("stride32_null", None, 8, False, 7)):
        buf = make_buf(7, dw, dh, dtype, nhwc, True)
        boxes = boxes_tensor(jobs, width)
        cnt = torch.tensor([count], dtype=torch.int32).cuda() if count is not None else None
        run_dev(capi, sf, 1, 1, W, H, dw, dh, devs, boxes, buf, dtype, True, "symmetric", nhwc, rects=rects_tensor(placed, 6) if explicit else None, count=cnt)
        torch.cuda.synchronize()
        if expect is None:
            assert bool((buf.buf == CANARY).all()), name
        else:
            assert torch.equal(buf.buf, want[expect].buf), name


@pytest.mark.parametrize("explicit", [False, True])
def test_spare_jobs_beyond_the_tables(capi, orc, explicit):
    """max_n = 40 over tables of 5 rows with count = 5, the tables lying at the very END of their tensors: the 35 spare jobs read neither box nor
    placement and write nothing (the buffer holds 5 jobs: a write of job 5 would land in the canaries or behind the buffer)"""
    W, H, dw, dh, sf = 131, 79, 24, 16, "YUV420"
    devs = frames_of(orc, sf, W, H)
    rects = cases.geometry_rects(W, H, dw, dh)[:5]
    jobs = [(cases.frame_of(i), r) for i, r in enumerate(rects)]
    placed = cases.explicit_rects(dw, dh, 5) if explicit else [capi.letterbox_fit(r[2], r[3], dw, dh) for r in rects]
    a, b = make_buf(5, dw, dh, 0, False, False), make_buf(5, dw, dh, 0, False, False)
    store = torch.full((64, 5), -7, dtype=torch.int32).cuda()
    store[-5:] = torch.tensor([(f, *r) for (f, r) in jobs], dtype=torch.int32).cuda()
    rstore = torch.full((64, 4), -7, dtype=torch.int32).cuda()
    rstore[-5:] = torch.tensor(placed, dtype=torch.int32).cuda()
    run_dev(capi, sf, 1, 0, W, H, dw, dh, devs, store[-5:], a, 0, False, "unit", False, rects=rstore[-5:] if explicit else None,
            count=torch.tensor([5], dtype=torch.int32).cuda(), max_n=40)
    run_host(capi, sf, 1, 0, W, H, dw, dh, devs, [(k, f, r, placed[k]) for k, (f, r) in enumerate(jobs)], b, 0, False, "unit", False)
    torch.cuda.synchronize()
    assert torch.equal(a.buf, b.buf)


def test_invalid_boxes_and_placements_are_pad_filled(capi, orc):
    """one box and one placement of every kind the guards refuse, among valid jobs: an invalid job is the pad's epilogue in every element, the valid
    jobs are the host entry's, the canaries are intact.  (The guards themselves are proven on the CPU: this checks the fill.)"""
    W, H, dw, dh, sf = 131, 79, 64, 48, "NV12"
    devs = frames_of(orc, sf, W, H)
    good_box, good_rect = (0, (17, 9, 55, 41)), (3, 5, 41, 31)
    table = [(good_box, good_rect), ((1, (3, 5, 0, 10)), good_rect), ((0, (3, 5, 20, -3)), good_rect), ((1, (0, 0, W, H)), (0, 0, dw, dh)),
             ((0, (-1, 5, 20, 10)), good_rect), ((1, (3, -2, 20, 10)), good_rect), ((1, (W - 19, 5, 20, 10)), good_rect), ((0, (W - 20, H - 10, 20, 10)), (1, 1, 62, 46)),
             ((1, (3, H - 8, 20, 10)), good_rect), ((-1, (3, 5, 20, 10)), good_rect), ((2, (3, 5, 20, 10)), good_rect), ((0, (0, 0, W + 1, 5)), good_rect),
             ((0, (0, 0, 5, H + 1)), good_rect), ((0, (2 ** 31 - 1, 0, 2 ** 31 - 1, 1)), good_rect), ((1, (5, 7, 13, 9)), (63, 47, 1, 1)),
             (good_box, (3, 5, 0, 31)), (good_box, (3, 5, 41, -1)), (good_box, (-1, 5, 41, 31)), (good_box, (3, -5, 41, 31)), (good_box, (0, 0, dw + 1, 31)),
             (good_box, (0, 0, 41, dh + 1)), (good_box, (dw - 40, 5, 41, 31)), (good_box, (3, dh - 30, 41, 31)), (good_box, (2 ** 31 - 1, 0, 2 ** 31 - 1, 1)),
             (good_box, (0, -2 ** 31, 1, 1)), ((1, (W - 1, H - 1, 1, 1)), (0, 0, 1, dh))]
    valid = [cases.box_valid((f, *r), W, H) and cases.rect_valid(d, dw, dh) for ((f, r), d) in table]
    assert sum(valid) == 5 and len(table) - sum(valid) == 21
    boxes, drects = [b for (b, _) in table], [d for (_, d) in table]
    for dtype, bgr, nhwc, padded in ((0, False, False, False), (2, True, True, True), (1, True, False, True)):
        a, b = make_buf(len(table), dw, dh, dtype, nhwc, padded), make_buf(len(table), dw, dh, dtype, nhwc, padded)
        run_dev(capi, sf, 1, 0, W, H, dw, dh, devs, boxes_tensor(boxes), a, dtype, bgr, "imagenet", nhwc, rects=rects_tensor(drects))
        run_host(capi, sf, 1, 0, W, H, dw, dh, devs, [(k, f, r, drects[k]) for k, (f, r) in enumerate(boxes) if valid[k]], b, dtype, bgr, "imagenet", nhwc)
        torch.cuda.synchronize()
        got, intact = a.frames()
        want = b.frames()[0]
        assert intact
        fill = pad_frame(dw, dh, dtype, bgr, nhwc, "imagenet")
        for k in range(len(table)):
            assert_bits(got[k], want[k] if valid[k] else fill, f"dtype {dtype} bgr {bgr} nhwc {nhwc} job {k} {table[k]} valid {valid[k]}")
    # without placements the box alone decides; opts == NULL pads with zeros
    a, b = make_buf(len(table), dw, dh, 0, False, False), make_buf(len(table), dw, dh, 0, False, False)
    run_dev(capi, sf, 1, 0, W, H, dw, dh, devs, boxes_tensor(boxes), a, 0, False, "imagenet", False, pad=None)
    ok = [cases.box_valid((f, *r), W, H) for (f, r) in boxes]
    run_host(capi, sf, 1, 0, W, H, dw, dh, devs, [(k, f, r, capi.letterbox_fit(r[2], r[3], dw, dh)) for k, (f, r) in enumerate(boxes) if ok[k]], b, 0, False,
             "imagenet", False, pad=None)
    torch.cuda.synchronize()
    got, intact = a.frames()
    want = b.frames()[0]
    assert intact
    zero = pad_frame(dw, dh, 0, False, False, "imagenet", pad=(0, 0, 0))
    for k in range(len(table)):
        assert_bits(got[k], want[k] if ok[k] else zero, f"fitted, job {k} {boxes[k]} valid {ok[k]}")


def test_graph_replays_with_live_tables(capi, orc):
    """one call captured on a side stream (one stream, no parallel branches), replayed three times; boxes, placements and count are overwritten on that
    stream between the replays: each replay equals the host entry on THAT replay's rectangles, placements and count"""
    W, H, dw, dh, sf, dtype = 131, 79, 64, 48, "NV12", 0
    devs = frames_of(orc, sf, W, H)
    all_rects = cases.geometry_rects(W, H, dw, dh)
    all_placed = cases.explicit_rects(dw, dh, 12)
    sets = [([(cases.frame_of(i), r) for i, r in enumerate(all_rects[:6])], all_placed[:6], 6),
            ([(cases.frame_of(i + 1), r) for i, r in enumerate(all_rects[6:12])], all_placed[6:12], 4)]
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        live = boxes_tensor(sets[0][0])
        live_rects = rects_tensor(sets[0][1])
        count = torch.tensor([sets[0][2]], dtype=torch.int32).cuda()
        staged = [(boxes_tensor(j), rects_tensor(p), torch.tensor([c], dtype=torch.int32).cuda()) for (j, p, c) in sets]
        buf = make_buf(6, dw, dh, dtype, False, False)
        run_dev(capi, sf, 1, 0, W, H, dw, dh, devs, live, buf, dtype, False, "imagenet", False, rects=live_rects, count=count,
                stream=st.cuda_stream)  # (eager once: the code object is loaded)
        st.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st):
            run_dev(capi, sf, 1, 0, W, H, dw, dh, devs, live, buf, dtype, False, "imagenet", False, rects=live_rects, count=count, stream=st.cuda_stream)
        for rep in (1, 0, 1):
            jobs, placed, c = sets[rep]
            live.copy_(staged[rep][0])
            live_rects.copy_(staged[rep][1])
            count.copy_(staged[rep][2])
            buf.buf.fill_(CANARY)
            g.replay()
            want = make_buf(6, dw, dh, dtype, False, False)
            run_host(capi, sf, 1, 0, W, H, dw, dh, devs, [(k, f, r, placed[k]) for k, (f, r) in enumerate(jobs[:c])], want, dtype, False, "imagenet", False,
                     stream=st.cuda_stream)
            st.synchronize()
            assert torch.equal(buf.buf, want.buf), rep


def _nvc():
    sys.path.insert(0, os.path.join(ROOT, "videoprocessingframework_amd"))
    import PyNvCodec as nvc
    from videoprocessingframework_amd import PytorchNvCodec as pnc

    return nvc, pnc


def test_python_path(orc):
    """device_letterbox_to_normalized_tensor == letterbox_to_normalized_tensor (torch.equal) on the same rois: fitted and explicit placements, planar and
    channels_last, bf16, B G R, a count into a slice of a larger tensor whose other frames keep their bits, an invalid box, a P10 surface"""
    nvc, pnc = _nvc()
    PF = nvc.PixelFormat
    W, H, dw, dh = 130, 78, 64, 48  # (even: a semi-planar Surface of the Task layer is one plane, chroma rows included)
    mean, std = PARAMS["imagenet"]
    cc = nvc.ColorspaceConversionContext(nvc.ColorSpace.BT_709, nvc.ColorRange.JPEG)
    surfs = [roi._upload(nvc, roi.frame(orc, "NV12", W, H, seed)[0], W, H) for seed in range(2)]
    torch.cuda.synchronize()
    rois = [(0, 17, 9, 55, 41), (1, 0, 0, W, H), (1, 1, 0, 3, 70), (0, 110, 68, 20, 10), (1, 5, 7, 120, 2)]
    boxes = torch.tensor(rois, dtype=torch.int32).cuda()
    rs = nvc.PySurfaceConvertResizer(W, H, PF.NV12, dw, dh, PF.RGB_PLANAR, 0)  # its own non-blocking stream
    placed = cases.explicit_rects(dw, dh, len(rois))
    drects = torch.tensor(placed, dtype=torch.int32).cuda()
    for kw in (dict(), dict(channels_last=True), dict(dtype=torch.bfloat16, bgr=True, pad=PAD), dict(dtype=torch.float16, channels_last=True, bgr=True, pad=PAD)):
        want, where = pnc.letterbox_to_normalized_tensor(rs, surfs, mean, std, rois=rois, cc_ctx=cc, **kw)
        got = pnc.device_letterbox_to_normalized_tensor(rs, surfs, boxes, mean, std, cc_ctx=cc, **kw)
        assert got.shape == want.shape and got.dtype == want.dtype and got.stride() == want.stride(), kw
        assert torch.equal(got, want), kw
        assert pnc.letterbox_fit_boxes(boxes, dw, dh).cpu().tolist() == where.tolist()
        want, _ = pnc.letterbox_to_normalized_tensor(rs, surfs, mean, std, rois=rois, dst_rects=placed, cc_ctx=cc, **kw)
        got = pnc.device_letterbox_to_normalized_tensor(rs, surfs, boxes, mean, std, dst_rects=drects, cc_ctx=cc, **kw)
        assert torch.equal(got, want), kw
    # a count and slices of wider tables, into a slice of a larger batch
    wide = torch.full((len(rois), 7), -1, dtype=torch.int32, device="cuda")
    wide[:, 1:6] = boxes
    rwide = torch.full((len(rois), 6), -1, dtype=torch.int32, device="cuda")
    rwide[:, 2:6] = drects
    big = torch.full((len(rois) + 3, 3, dh, dw), 0x3C3C, dtype=torch.int16, device="cuda")
    view = big.view(torch.float16)[2:2 + len(rois)]
    res = pnc.device_letterbox_to_normalized_tensor(rs, surfs, wide[:, 1:6], mean, std, count=torch.tensor([3], dtype=torch.int32, device="cuda"),
                                                    dst_rects=rwide[:, 2:6], pad=PAD, dtype=torch.float16, out=view, cc_ctx=cc)
    assert res.data_ptr() == view.data_ptr()
    want, _ = pnc.letterbox_to_normalized_tensor(rs, surfs, mean, std, rois=rois[:3], dst_rects=placed[:3], pad=PAD, dtype=torch.float16, cc_ctx=cc)
    assert torch.equal(view[:3], want)
    assert bool((big[:2] == 0x3C3C).all()) and bool((big[5:] == 0x3C3C).all())   # rows at or behind the count are not written
    # an invalid box: the normalised pad
    bad = boxes.clone()
    bad[1, 3] = 0
    got = pnc.device_letterbox_to_normalized_tensor(rs, surfs, bad, mean, std, pad=PAD, cc_ctx=cc)
    fill = torch.from_numpy(pad_frame(dw, dh, 0, False, False, "imagenet").view(np.float32)).cuda()
    assert torch.equal(got[1], fill)
    assert pnc.letterbox_fit_boxes(bad, dw, dh)[1].tolist() == [0, 0, 0, 0]
    # a P10 surface
    up = nvc.PyFrameUploader(W, H, PF.P10, 0)
    p10 = [up.UploadSingleFrame(np.concatenate([p.reshape(-1) for p in p16.p16_frame(orc, "P10", W, H, s)])).Clone(0) for s in range(2)]
    torch.cuda.synchronize()
    rs10 = nvc.PySurfaceConvertResizer(W, H, PF.P10, dw, dh, PF.RGB_PLANAR, 0)
    want, _ = pnc.letterbox_to_normalized_tensor(rs10, p10, mean, std, rois=rois, dtype=torch.float16, cc_ctx=cc)
    got = pnc.device_letterbox_to_normalized_tensor(rs10, p10, boxes, mean, std, dtype=torch.float16, cc_ctx=cc)
    assert torch.equal(got, want)
    with pytest.raises(ValueError):
        pnc.device_letterbox_to_normalized_tensor(rs, surfs, boxes.cpu(), mean, std)
    with pytest.raises(ValueError):
        pnc.device_letterbox_to_normalized_tensor(rs, surfs, boxes, mean, std, dst_rects=drects.cpu())
    with pytest.raises(ValueError):
        pnc.device_letterbox_to_normalized_tensor(rs, surfs, boxes, mean, std, dst_rects=drects[:3])


def test_one_launch_per_call():
    """a child process with VPF_HIP_LOG=2: every call is ONE launch of k_lb_dev, whatever mix of padded, staged and per-tap tiles it holds"""
    code = f"""
import sys
sys.path.insert(0, {ROOT!r})
import torch
from videoprocessingframework_amd import capi
W, H = 131, 79
y, uv = torch.zeros((H, W), dtype=torch.uint8, device="cuda"), torch.zeros(((H + 1) // 2, 2 * ((W + 1) // 2)), dtype=torch.uint8, device="cuda")
fr = capi.make_frame_srcs([[(y.data_ptr(), W), (uv.data_ptr(), 2 * ((W + 1) // 2))]])
ex = capi.make_exec(torch.cuda.current_stream().cuda_stream)
boxes = torch.tensor([(0, 0, 0, W, H), (0, 5, 3, 3, 70), (0, 17, 9, 55, 41), (0, 0, 0, 0, 0)], dtype=torch.int32).cuda()
for (dw, dh), nhwc, variant in (((64, 48), False, 0), ((300, 40), True, 0), ((24, 16), False, 0), ((64, 48), True, 9)):
    out = torch.zeros((4, 3 * dh * dw), dtype=torch.float32, device="cuda")
    dst = [(out.data_ptr(), 12 * dw)] if nhwc else [(out.data_ptr() + 4 * c * dh * dw, 4 * dw) for c in range(3)]
    prev = capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, variant)
    print("CASE", file=sys.stderr, flush=True)
    capi.convert_letterbox_tensor_dev(ex, capi.NV12, 1, 0, W, H, dw, dh, fr, capi.make_letterbox_dev(boxes.data_ptr(), 4, dst, 12 * dh * dw),
                                      capi.make_tensor_norm((0, 0, 0), (1, 1, 1), nhwc=nhwc), capi.make_letterbox_opts((114, 114, 114)))
    torch.cuda.synchronize()
    capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, prev)
print("done")
"""
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, VPF_HIP_LOG="2"), timeout=120)
    assert r.returncode == 0 and "done" in r.stdout, r.stdout + r.stderr
    chunks = r.stderr.split("CASE")[1:]
    assert len(chunks) == 4
    for chunk, label in zip(chunks, ("k_lb_dev<0, 6>", "k_lb_dev<0, 8>", "k_lb_dev<0, 6>", "k_lb_dev<0, 8>")):
        launches = [ln for ln in chunk.splitlines() if "libvpfhip: launch" in ln]
        assert len(launches) == 1 and "k_lb_dev<" in launches[0] and label in launches[0], chunk


@pytest.mark.parametrize("seed", _FUZZ_SEEDS)  # soak: VPF_FUZZ_SEEDS=500 (VPF_FUZZ_FIRST=n: seeds n .. n + VPF_FUZZ_SEEDS - 1, fresh cases)
def test_seeded_calls_equal_the_host_table_entry(capi, orc, seed):
    """cases.fuzz_case(seed): frame, format, destination, boxes, fitted or explicit placements, layout and count, against the host-table entry on the
    jobs below the count that are valid; the others below the count are the pad, the rest canary"""
    c = cases.fuzz_case(seed)
    W, H, dw, dh, sf, dtype, bgr, nhwc = c["W"], c["H"], c["dw"], c["dh"], c["sf"], c["dtype"], c["bgr"], c["nhwc"]
    devs = frames_of(orc, sf, W, H)
    n = len(c["boxes"])
    live = n if c["count"] is None else max(0, min(c["count"], n))
    placed = c["rects"] if c["rects"] is not None else [cases.fit(b[3], b[4], dw, dh) if b[3] >= 1 and b[4] >= 1 else (0, 0, 0, 0) for b in c["boxes"]]
    valid = [cases.box_valid(b, W, H) and cases.rect_valid(d, dw, dh) for b, d in zip(c["boxes"], placed)]
    a, b = make_buf(n, dw, dh, dtype, nhwc, c["padded"]), make_buf(n, dw, dh, dtype, nhwc, c["padded"])
    boxes = boxes_tensor([(bx[0], bx[1:]) for bx in c["boxes"]], c["box_width"])
    cnt = torch.tensor([c["count"]], dtype=torch.int32).cuda() if c["count"] is not None else None
    run_dev(capi, sf, c["cs"], c["cr"], W, H, dw, dh, devs, boxes, a, dtype, bgr, "imagenet", nhwc,
            rects=rects_tensor(c["rects"], c["rect_width"]) if c["rects"] is not None else None, count=cnt)
    run_host(capi, sf, c["cs"], c["cr"], W, H, dw, dh, devs, [(k, bx[0], tuple(bx[1:]), tuple(placed[k])) for k, bx in enumerate(c["boxes"][:live]) if valid[k]],
             b, dtype, bgr, "imagenet", nhwc)
    torch.cuda.synchronize()
    got, intact = a.frames()
    want = b.frames()[0]
    assert intact, c
    fill = pad_frame(dw, dh, dtype, bgr, nhwc, "imagenet")
    for k in range(live):
        assert_bits(got[k], want[k] if valid[k] else fill, f"seed {seed} job {k} box {c['boxes'][k]} dst_rect {placed[k]} valid {valid[k]}")
    for k in range(live, n):  # jobs at or behind the count: their elements still hold the canary, like the host buffer's (never written there either)
        assert_bits(got[k], want[k], f"seed {seed} job {k} lies at or behind the count {c['count']}")
    if all(valid[:live]):
        assert torch.equal(a.buf, b.buf), f"seed {seed}: bytes outside the jobs' elements differ"
