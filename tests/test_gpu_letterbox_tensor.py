"""Letterbox into the tensor on the MI355X: vpf_convert_letterbox_tensor, PySurfaceConvertResizer.ExecuteLetterboxToTensor and
PytorchNvCodec.letterbox_to_normalized_tensor.

Ground truth is the definition composed from the ROI entry's reference: inside dst_rect = (ix, iy, iw, ih) the bytes ref_u8(rect -> (iw, ih)) of
tests/test_gpu_roi_tensor.py (the CPU oracle: conversion of the whole frame, a numpy crop, oracle.resize), outside pad[c]
(tests/test_letterbox_tensor_cpu.py checks that this is the fill + resize-into-a-sub-window composition), then reference_bits of
tests/test_gpu_tensor_out.py.  Every element of every output must be bit-identical; there is no tolerance.  Destinations hold canaries around
every plane, which must survive.  Two cases compare on the GPU instead: with the ROI entry for a dst_rect that is the whole destination, and with
a fill followed by the ROI entry on sliced planes (the route this entry replaces)."""
import os
import sys

import numpy as np
import pytest
import torch

import test_gpu_p16_tensor as p16
from gpu_util import DevPlanes, stream_handle
from test_gpu_roi_tensor import frame, ref_u8
from test_gpu_tensor_nhwc import NhwcBuf, hwc
from test_gpu_tensor_out import ELEM, PARAMS, TensorBuf, assert_bits, reference_bits
from test_roi_tensor_cpu import roi_reference_u8

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAME_SIZES = [(131, 79), (130, 78)]
RECT = (17, 9, 55, 41)
PAD = (114, 7, 250)   # three different values: a channel mix-up shows
TDT = {0: torch.float32, 1: torch.float16, 2: torch.bfloat16}


@pytest.fixture(scope="module")
def orc(oracle):
    oracle.set_threads(16)
    return oracle


def place(inner, drect, dw, dh, pad, bgr=False):
    """[3, ih, iw] R G B bytes of the picture -> the [3, dh, dw] R G B bytes of the letterboxed frame; pad[c] belongs to OUTPUT channel c"""
    ix, iy, iw, ih = drect
    assert inner.shape == (3, ih, iw)
    out = np.empty((3, dh, dw), np.uint8)
    for k in range(3):
        out[k] = pad[2 - k] if bgr else pad[k]
    out[:, iy:iy + ih, ix:ix + iw] = inner
    return out


def lb_ref(orc, sf, cs, cr, W, H, rect, drect, dw, dh, pad, bgr=False, seed=0):
    return place(ref_u8(orc, sf, cs, cr, W, H, rect, drect[2], drect[3], seed=seed), drect, dw, dh, pad, bgr)


def run_lb(capi, sf, cs, cr, W, H, dw, dh, jobs, dtype, bgr, params, buf, pad=PAD, nhwc=False, variant=None):
    """jobs: [(DevPlanes of the frame, rect, dst_rect)]; job i writes buf.planes(i)"""
    norm = capi.make_tensor_norm(*PARAMS[params], dtype=dtype, bgr=bgr, nhwc=nhwc)
    arr = capi.make_letterbox_jobs([(dev.desc(), buf.planes(i), rect, drect) for i, (dev, rect, drect) in enumerate(jobs)])
    prev = capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, variant) if variant is not None else None
    try:
        capi.convert_letterbox_tensor(capi.make_exec(stream_handle()), getattr(capi, sf), cs, cr, W, H, dw, dh, arr, norm,
                                      capi.make_letterbox_opts(pad) if pad is not None else None)
        torch.cuda.synchronize()
    finally:
        if variant is not None:
            capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, prev)


# ------------------------------------------------------------------------------------------------ 1. geometry
@pytest.mark.parametrize("sf", ["NV12", "YUV420"])
@pytest.mark.parametrize("W,H", FRAME_SIZES)
def test_geometry(capi, orc, sf, W, H):
    """one call into 260 x 70 f32 — two 256-column chunks, the second 4 wide; five 16-row bands, the last partial: the whole destination, one
    element, an odd corner, a picture astride the chunk edge, one that starts exactly on the chunk and band edges, one row, one column at the right
    edge, the fit of the rectangle"""
    dw, dh, cs, cr = 260, 70, 1, 0
    dev = frame(orc, sf, W, H)[1]
    drects = [(0, 0, 260, 70), (1, 1, 1, 1), (3, 5, 61, 35), (252, 12, 8, 20), (256, 16, 4, 16), (0, 0, 260, 1), (259, 0, 1, 70),
              capi.letterbox_fit(RECT[2], RECT[3], dw, dh)]
    assert drects[-1] == (83, 0, 94, 70)
    buf = TensorBuf(len(drects), dw, dh, 4)
    run_lb(capi, sf, cs, cr, W, H, dw, dh, [(dev, RECT, d) for d in drects], 0, False, "imagenet", buf)
    got, intact = buf.frames()
    assert intact
    for i, d in enumerate(drects):
        assert_bits(got[i], reference_bits(lb_ref(orc, sf, cs, cr, W, H, RECT, d, dw, dh, PAD), *PARAMS["imagenet"], 0, False), f"{sf} {W}x{H} dst_rect {d}")


# ------------------------------------------------------------------------------------------------ 2. the whole destination
@pytest.mark.parametrize("sf", ["NV12", "YUV420"])
@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_whole_destination_equals_the_roi_entry(capi, orc, sf, dtype):
    """dst_rect = (0, 0, dw, dh): bit-identical, compared on the GPU, to vpf_convert_resize_tensor_rois; with rect = the whole frame also to
    vpf_convert_resize_tensor.  130 x 78 -> 61 x 35, B G R, opts == NULL (nothing to pad)"""
    W, H, dw, dh = 130, 78, 61, 35
    dev = frame(orc, sf, W, H)[1]
    rects = [RECT, (0, 0, W, H)]
    a, b, c = (TensorBuf(len(rects), dw, dh, ELEM[dtype]) for _ in range(3))
    run_lb(capi, sf, 1, 1, W, H, dw, dh, [(dev, r, (0, 0, dw, dh)) for r in rects], dtype, True, "symmetric", a, pad=None)
    norm = capi.make_tensor_norm(*PARAMS["symmetric"], dtype=dtype, bgr=True)
    ex = capi.make_exec(stream_handle())
    capi.convert_resize_tensor_rois(ex, getattr(capi, sf), 1, 1, W, H, dw, dh, capi.make_rois([(dev.desc(), b.planes(i), r) for i, r in enumerate(rects)]), norm)
    c.buf.copy_(b.buf)
    capi.convert_resize_tensor(ex, getattr(capi, sf), 1, 1, W, H, dev.desc(), dw, dh, c.planes(1), norm)
    torch.cuda.synchronize()
    assert bool((a.buf == b.buf).all()) and bool((a.buf == c.buf).all())
    got, intact = a.frames()
    assert intact
    for i, r in enumerate(rects):
        assert_bits(got[i], reference_bits(ref_u8(orc, sf, 1, 1, W, H, r, dw, dh), *PARAMS["symmetric"], dtype, True), f"whole destination, rect {r}")


# ------------------------------------------------------------------------------------------------ 3. the composition, on the GPU
def _pad_bits(pad, params, dtype, bgr=False):
    """the epilogue of the pad per OUTPUT channel, as signed integers of the element's width (what a torch integer view takes)"""
    bits = reference_bits(np.array(pad[::-1] if bgr else pad, np.uint8).reshape(3, 1, 1), *PARAMS[params], dtype, bgr).reshape(3)
    return [int(v) for v in bits.view(np.int32 if dtype == 0 else np.int16)]


def _filled(n, dw, dh, dtype, pad, params):
    """[n, 3, dh, dw] on the device, every plane filled with the epilogue of its pad"""
    t = torch.empty((n, 3, dh, dw), dtype=TDT[dtype], device="cuda")
    iv = t.view(torch.int32 if dtype == 0 else torch.int16)
    for c, v in enumerate(_pad_bits(pad, params, dtype)):
        iv[:, c] = v
    return t


@pytest.mark.parametrize("sf", ["NV12", "YUV420"])
@pytest.mark.parametrize("dtype", [0, 1])
def test_fill_then_roi_entry_on_sliced_planes(capi, orc, sf, dtype):
    """a fill followed by vpf_convert_resize_tensor_rois(dst_size = (iw, ih)) on the job's planes advanced by iy * pitch + ix * element size — one call
    per distinct inner size, misaligned slices — against ONE call of the new entry, byte for byte on the GPU; even and odd ix"""
    W, H, dw, dh, e = 131, 79, 70, 48, ELEM[dtype]
    dev = frame(orc, sf, W, H)[1]
    jobs = [(RECT, (4, 6, 61, 35)), (RECT, (3, 5, 61, 35)), ((0, 0, W, H), (9, 0, 52, 48)), ((2, 3, 120, 70), (0, 13, 70, 22)), (RECT, (69, 47, 1, 1))]
    norm = capi.make_tensor_norm(*PARAMS["imagenet"], dtype=dtype)
    ex = capi.make_exec(stream_handle())
    want = _filled(len(jobs), dw, dh, dtype, PAD, "imagenet")
    for i, (rect, (ix, iy, iw, ih)) in enumerate(jobs):
        sliced = [(want[i, c].data_ptr() + (iy * dw + ix) * e, dw * e) for c in range(3)]
        capi.convert_resize_tensor_rois(ex, getattr(capi, sf), 1, 0, W, H, iw, ih, capi.make_rois([(dev.desc(), sliced, rect)]), norm)
    got = torch.full((len(jobs), 3, dh, dw), -1, dtype=torch.int32 if dtype == 0 else torch.int16, device="cuda").view(TDT[dtype])
    arr = capi.make_letterbox_jobs([(dev.desc(), [(got[i, c].data_ptr(), dw * e) for c in range(3)], rect, d) for i, (rect, d) in enumerate(jobs)])
    capi.convert_letterbox_tensor(ex, getattr(capi, sf), 1, 0, W, H, dw, dh, arr, norm, capi.make_letterbox_opts(PAD))
    torch.cuda.synchronize()
    iv = torch.int32 if dtype == 0 else torch.int16
    assert torch.equal(got.view(iv), want.view(iv))
    h = got.view(iv).cpu().numpy().view(np.uint32 if dtype == 0 else np.uint16)
    for i, (rect, d) in enumerate(jobs):
        assert_bits(h[i], reference_bits(lb_ref(orc, sf, 1, 0, W, H, rect, d, dw, dh, PAD), *PARAMS["imagenet"], dtype, False), f"{sf} job {i}")


# ------------------------------------------------------------------------------------------------ 4. both forms in one call
def test_both_forms_in_one_call(capi, orc):
    """a staged job and a per-tap job (131 x 79 -> 20 x 12 inside: about 6.5 x) in one call; the same call with every job forced to the per-tap form
    (VPF_TUNE_NV12_RGB_VARIANT = 9) gives identical bits"""
    W, H, dw, dh, sf = 131, 79, 70, 48, "NV12"
    dev = frame(orc, sf, W, H)[1]
    jobs = [(dev, RECT, (3, 5, 61, 35)), (dev, (0, 0, W, H), (25, 18, 20, 12)), (dev, (0, 0, W, H), (0, 0, 70, 48)), (dev, (1, 0, 129, 78), (49, 35, 21, 13))]
    outs = []
    for variant in (0, 9):
        buf = TensorBuf(len(jobs), dw, dh, 4)
        run_lb(capi, sf, 1, 0, W, H, dw, dh, jobs, 0, False, "imagenet", buf, variant=variant)
        got, intact = buf.frames()
        assert intact, variant
        for i, (_, rect, d) in enumerate(jobs):
            assert_bits(got[i], reference_bits(lb_ref(orc, sf, 1, 0, W, H, rect, d, dw, dh, PAD), *PARAMS["imagenet"], 0, False), f"variant {variant} job {i}")
        outs.append(got)
    assert np.array_equal(outs[0], outs[1])


# ------------------------------------------------------------------------------------------------ 5. layouts
LAYOUT_RECTS = {61: [(3, 5, 50, 20), (0, 0, 61, 37), (58, 36, 3, 1)], 64: [(3, 5, 58, 30), (0, 0, 64, 37), (61, 0, 3, 37)], 1: [(0, 3, 1, 20), (0, 0, 1, 37), (0, 36, 1, 1)]}


@pytest.mark.parametrize("dw", [61, 64, 1])
@pytest.mark.parametrize("dtype", [0, 1])
def test_destination_widths_alignment_and_strides(capi, orc, dw, dtype):
    """destination widths with and without scalar tails, pictures that start and end inside a lane's four columns (pad and picture share a vector);
    plane pointers one element off the vector alignment; padded row, plane and frame strides"""
    W, H, dh, sf = 131, 79, 37, "NV12"
    e = ELEM[dtype]
    dev = frame(orc, sf, W, H)[1]
    drects = LAYOUT_RECTS[dw]
    layouts = {"contiguous": dict(lead=256),
               "off_by_one_element": dict(lead=256 + e),
               "padded": dict(row=dw * e + 16 + e, plane=dh * (dw * e + 16 + e) + 40 * e, frame=3 * (dh * (dw * e + 16 + e) + 40 * e) + 8 * e, lead=24 * e),
               "padded64": dict(row=dw * e + 64, plane=dh * (dw * e + 64) + 64, frame=3 * (dh * (dw * e + 64) + 64) + 256, lead=512)}
    for lname, geo in layouts.items():
        buf = TensorBuf(len(drects), dw, dh, e, **geo)
        run_lb(capi, sf, 1, 0, W, H, dw, dh, [(dev, RECT, d) for d in drects], dtype, False, "imagenet", buf)
        got, intact = buf.frames()
        assert intact, (lname, dw, dtype)
        for i, d in enumerate(drects):
            assert_bits(got[i], reference_bits(lb_ref(orc, sf, 1, 0, W, H, RECT, d, dw, dh, PAD), *PARAMS["imagenet"], dtype, False), f"{lname} dw{dw} dtype{dtype} dst_rect {d}")


# ------------------------------------------------------------------------------------------------ 6. flags and sources
FLAG_DRECT, FLAG_DST = (3, 5, 61, 35), (70, 48)


@pytest.mark.parametrize("dtype", [0, 2])
@pytest.mark.parametrize("bgr", [False, True])
def test_channels_last(capi, orc, dtype, bgr):
    """VPF_TENSOR_NHWC: element (y, x, c) is the planar call's element (c, y, x), pad included; staged and per-tap forms"""
    W, H, sf = 131, 79, "NV12"
    dw, dh = FLAG_DST
    dev = frame(orc, sf, W, H)[1]
    jobs = [(dev, RECT, FLAG_DRECT), (dev, (0, 0, W, H), (25, 18, 20, 12)), (dev, RECT, (0, 0, dw, dh))]
    buf = NhwcBuf(len(jobs), dw, dh, ELEM[dtype])
    run_lb(capi, sf, 1, 0, W, H, dw, dh, jobs, dtype, bgr, "imagenet", buf, nhwc=True)
    got, intact = buf.frames()
    assert intact
    for i, (_, rect, d) in enumerate(jobs):
        assert_bits(got[i], hwc(reference_bits(lb_ref(orc, sf, 1, 0, W, H, rect, d, dw, dh, PAD, bgr), *PARAMS["imagenet"], dtype, bgr)), f"nhwc dtype{dtype} bgr{bgr} job {i}")


def test_bgr_pad_follows_the_output_channel(capi, orc):
    """VPF_TENSOR_BGR, planar: plane c holds output channel c (B G R) and pad[c] fills ITS outside"""
    W, H, sf = 130, 78, "YUV420"
    dw, dh = FLAG_DST
    dev = frame(orc, sf, W, H)[1]
    buf = TensorBuf(1, dw, dh, 2)
    run_lb(capi, sf, 0, 1, W, H, dw, dh, [(dev, RECT, FLAG_DRECT)], 1, True, "imagenet", buf)
    got, intact = buf.frames()
    assert intact
    assert_bits(got[0], reference_bits(lb_ref(orc, sf, 0, 1, W, H, RECT, FLAG_DRECT, dw, dh, PAD, True), *PARAMS["imagenet"], 1, True), "bgr")
    pad_bits = reference_bits(np.array(PAD[::-1], np.uint8).reshape(3, 1, 1), *PARAMS["imagenet"], 1, True).reshape(3)  # output channel order
    for c in range(3):
        assert got[0][c, 0, 0] == pad_bits[c] and got[0][c, dh - 1, dw - 1] == pad_bits[c]


@pytest.mark.parametrize("variant", [0, 9])
def test_p10_source(capi, orc, variant):
    """a P10 frame whose rows are only 2-B aligned: the NV12 definition on the narrowed planes, both forms"""
    W, H = 131, 79
    dw, dh = FLAG_DST
    dev = DevPlanes(p16.p16_frame(orc, "P10", W, H, 0), align=64, extra=2)
    rgb = p16.rgb_of(orc, "P10", 1, 0, W, H, 0)
    buf = TensorBuf(1, dw, dh, 4)
    run_lb(capi, "P10", 1, 0, W, H, dw, dh, [(dev, RECT, FLAG_DRECT)], 0, False, "imagenet", buf, variant=variant)
    got, intact = buf.frames()
    assert intact
    inner = roi_reference_u8(orc, "NV12", 1, 0, W, H, None, RECT, FLAG_DRECT[2], FLAG_DRECT[3], rgb=rgb)
    assert_bits(got[0], reference_bits(place(inner, FLAG_DRECT, dw, dh, PAD), *PARAMS["imagenet"], 0, False), f"P10 variant {variant}")


# ------------------------------------------------------------------------------------------------ 7. job tables
def test_jobs_over_the_table_boundaries(capi, orc):
    """200 jobs into 16 x 16 f16 over three frames (many jobs name the same frame), dst_rects of every size and place: the third job table whatever
    a table holds (82 here, 96 in the ROI entry)"""
    W, H, dw, dh, sf = 131, 79, 16, 16, "NV12"
    devs = [frame(orc, sf, W, H, seed)[1] for seed in range(3)]
    rng = np.random.default_rng(11)
    rects = [RECT, (0, 0, W, H), (5, 7, 13, 9), (130, 78, 1, 1), (3, 2, 100, 12)]
    sizes = [(16, 16), (1, 1), (16, 9), (9, 16), (5, 3), (12, 12), (4, 15)]
    jobs = []
    for i in range(200):
        iw, ih = sizes[i % len(sizes)]
        jobs.append((i % 3, rects[i % len(rects)], (int(rng.integers(0, dw - iw + 1)), int(rng.integers(0, dh - ih + 1)), iw, ih)))
    buf = TensorBuf(len(jobs), dw, dh, 2)
    run_lb(capi, sf, 1, 0, W, H, dw, dh, [(devs[k], r, d) for k, r, d in jobs], 1, False, "imagenet", buf)
    got, intact = buf.frames()
    assert intact
    for i, (k, r, d) in enumerate(jobs):
        assert_bits(got[i], reference_bits(lb_ref(orc, sf, 1, 0, W, H, r, d, dw, dh, PAD, seed=k), *PARAMS["imagenet"], 1, False), f"job {i} rect {r} dst_rect {d}")


# ------------------------------------------------------------------------------------------------ 8. Python
def _nvc():
    sys.path.insert(0, os.path.join(ROOT, "videoprocessingframework_amd"))
    import PyNvCodec as nvc
    from videoprocessingframework_amd import PytorchNvCodec as pnc

    return nvc, pnc


def _upload(nvc, planes, w, h):
    up = nvc.PyFrameUploader(w, h, nvc.PixelFormat.NV12, 0)
    return up.UploadSingleFrame(np.concatenate([p.reshape(-1) for p in planes])).Clone(0)


def test_python_path(orc, capi):
    """letterbox_to_normalized_tensor with rois=None on two surfaces: the placement vpf_letterbox_fit gives and the bits of the composition (a fill, then
    rois_to_normalized_tensor of a resizer of the inner size into the sliced view); from a resizer on its own stream, called under a non-default
    torch stream and consumed there without a host synchronisation; `out` reused; explicit rois and dst_rects; K = 0"""
    nvc, pnc = _nvc()
    PF = nvc.PixelFormat
    W, H, dw, dh = 130, 78, 64, 64
    mean, std = PARAMS["imagenet"]
    cc = nvc.ColorspaceConversionContext(nvc.ColorSpace.BT_709, nvc.ColorRange.JPEG)
    surfs = [_upload(nvc, frame(orc, "NV12", W, H, seed)[0], W, H) for seed in range(2)]
    torch.cuda.synchronize()
    fit = capi.letterbox_fit(W, H, dw, dh)
    assert fit == (0, 13, 64, 38) and tuple(nvc.LetterboxFit(W, H, dw, dh)) == fit
    ix, iy, iw, ih = fit
    rs = nvc.PySurfaceConvertResizer(W, H, PF.NV12, dw, dh, PF.RGB_PLANAR, 0)      # its own non-blocking stream
    inner = nvc.PySurfaceConvertResizer(W, H, PF.NV12, iw, ih, PF.RGB_PLANAR, 0)
    want = _filled(2, dw, dh, 0, (114, 114, 114), "imagenet")
    pnc.rois_to_normalized_tensor(inner, surfs, [(0, 0, 0, W, H), (1, 0, 0, W, H)], mean, std, out=want[:, :, iy:iy + ih, ix:ix + iw], cc_ctx=cc)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        out, placement = pnc.letterbox_to_normalized_tensor(rs, surfs, mean, std, cc_ctx=cc)
        consumed = out * 1.0  # on the stream the call was made under, no synchronize in between
    side.synchronize()
    torch.cuda.synchronize()
    assert tuple(out.shape) == (2, 3, dh, dw) and out.dtype == torch.float32
    assert placement.dtype == torch.int64 and placement.device.type == "cpu" and placement.tolist() == [list(fit)] * 2
    assert torch.equal(consumed.view(torch.int32), want.view(torch.int32))
    got = consumed.cpu().numpy().view(np.uint32)
    for i in range(2):
        ref = lb_ref(orc, "NV12", 1, 1, W, H, (0, 0, W, H), fit, dw, dh, (114, 114, 114), seed=i)
        assert_bits(got[i], reference_bits(ref, mean, std, 0, False), f"new tensor, surface {i}")
    # `out` reused: the same storage, written again (f16, B G R, explicit rois and dst_rects, a pad of its own)
    rois, drects = [(1, 17, 9, 55, 41), (0, 0, 0, W, H), (0, 17, 9, 55, 41)], [(3, 5, 50, 30), (20, 40, 30, 20), (0, 0, 64, 64)]
    big = torch.full((len(rois) + 2, 3, dh, dw), 0x3C3C, dtype=torch.int16, device="cuda")
    view = big.view(torch.float16)[1:1 + len(rois)]
    for _ in range(2):
        res, placement = pnc.letterbox_to_normalized_tensor(rs, surfs, mean, std, rois=rois, dst_rects=torch.tensor(drects), pad=PAD, dtype=torch.float16,
                                                            bgr=True, out=view, cc_ctx=cc)
        assert res.data_ptr() == view.data_ptr() and placement.tolist() == [list(d) for d in drects]
        h = big.cpu().numpy().view(np.uint16)
        assert (h[:1] == 0x3C3C).all() and (h[1 + len(rois):] == 0x3C3C).all()
        for i, (r, d) in enumerate(zip(rois, drects)):
            ref = lb_ref(orc, "NV12", 1, 1, W, H, tuple(r[1:]), d, dw, dh, PAD, True, seed=r[0])
            assert_bits(h[1 + i], reference_bits(ref, mean, std, 1, True), f"slice, job {i}")
    # channels_last: the same values in NHWC memory
    cl, _ = pnc.letterbox_to_normalized_tensor(rs, surfs, mean, std, rois=rois, dst_rects=drects, pad=PAD, cc_ctx=cc, channels_last=True)
    pl, _ = pnc.letterbox_to_normalized_tensor(rs, surfs, mean, std, rois=rois, dst_rects=drects, pad=PAD, cc_ctx=cc)
    assert cl.is_contiguous(memory_format=torch.channels_last) and torch.equal(cl.contiguous().view(torch.int32), pl.view(torch.int32))
    # K = 0: an empty tensor and an empty placement, nothing launched
    empty, placement = pnc.letterbox_to_normalized_tensor(rs, surfs, mean, std, rois=[], dtype=torch.bfloat16)
    assert tuple(empty.shape) == (0, 3, dh, dw) and empty.dtype == torch.bfloat16 and tuple(placement.shape) == (0, 4)
    with pytest.raises(ValueError):
        pnc.letterbox_to_normalized_tensor(rs, surfs, mean, std, rois=rois, dst_rects=drects[:2])
    with pytest.raises(ValueError):
        pnc.letterbox_to_normalized_tensor(rs, surfs, mean, std, pad=(0, 0, 300))
