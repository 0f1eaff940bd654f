"""The fused multi-ROI perspective warp with the homographies in DEVICE memory on the MI355X: vpf_convert_persp_tensor_dev,
PySurfaceConvertResizer.ExecutePerspsDevToTensor, PytorchNvCodec.device_persps_to_normalized_tensor and quads_to_homographies_unchecked.

Ground truth is the HOST-TABLE entry (vpf_convert_persp_tensor, itself held to the CPU oracle by tests/test_gpu_persp_tensor.py) on the same matrices
into a buffer of the same layout: the two canary-filled buffers are compared on the device, byte for byte — every element, every canary, no
tolerance.  Two cases go against the oracle chain directly (want_bits), so the two entries cannot drift together, and the seeded fuzz
(tests/cases_persps_dev.py) holds every case to the composed oracle reference.  Which tiles stage, outgrow the hinted LDS or need the per-pixel
fallback is asserted on the CPU (tests/test_persps_dev_bounds_cpu.py, tests/test_persps_dev_cases_cpu.py::test_reach): the GPU cannot tell, every form
gives the same bits."""
import math
import os
import sys

import numpy as np
import pytest
import torch

import cases_persps_dev as pcases
import test_gpu_p16_tensor as p16
import test_gpu_persp_tensor as persp
from gpu_util import stream_handle
from test_gpu_rois_dev import make_buf
from test_gpu_tensor_fuzz import dev_buf, tuned, upload_frames, want_of
from test_gpu_tensor_nhwc import hwc
from test_gpu_tensor_out import CANARY, ELEM, PARAMS, assert_bits, reference_bits
from test_gpu_warp_tensor import BORDER, _upload, frame, geometry_jobs
from test_gpu_warps_dev import POISON, explain, frames_of, index_tensor
from test_gpu_warps_dev import run_dev as run_affine_dev
from test_persp_tensor_cpu import NAMED
from test_tensor_fuzz_cases_cpu import forget_p16, host_jobs, job_u8, rgb_frames, rgb_order

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = 16777216.0


@pytest.fixture(scope="module")
def orc(oracle):
    oracle.set_threads(16)
    return oracle


def run_host(capi, sf, cs, cr, W, H, dw, dh, devs, jobs, buf, dtype, bgr, params, nhwc, border=BORDER, mode=0, stream=None):
    """the host-table entry: jobs = [(job index, frame index, matrix)], job k writes buf.planes(k)"""
    norm = capi.make_tensor_norm(*PARAMS[params], dtype=dtype, bgr=bgr, nhwc=nhwc)
    if jobs:
        table = capi.make_persps([(devs[f].desc(), buf.planes(k), m) for (k, f, m) in jobs])
        capi.convert_persp_tensor(capi.make_exec(stream or stream_handle()), getattr(capi, sf), cs, cr, W, H, dw, dh, table, norm, capi.make_warp_opts(mode, border))


def run_dev(capi, sf, cs, cr, W, H, dw, dh, devs, mats, index, buf, dtype, bgr, params, nhwc, count=None, max_n=None, max_step=0.0, border=BORDER, mode=0,
            stream=None):
    """the device entry: mats = a device float32 tensor [K, >= 9] (its row stride is the matrix stride), index = a device int32 tensor (its stride is
    the frame stride) or None, count = a device int32 tensor or None"""
    norm = capi.make_tensor_norm(*PARAMS[params], dtype=dtype, bgr=bgr, nhwc=nhwc)
    table = capi.make_persps_dev(mats.data_ptr(), mats.shape[0] if max_n is None else max_n, buf.planes(0), buf.frame,
                                 index.data_ptr() if index is not None else None, count.data_ptr() if count is not None else None,
                                 4 * mats.stride(0), 4 * index.stride(0) if index is not None else 4, max_step)
    capi.convert_persp_tensor_dev(capi.make_exec(stream or stream_handle()), getattr(capi, sf), cs, cr, W, H, dw, dh,
                                  capi.make_frame_srcs([d.desc() for d in devs]), table, norm, capi.make_warp_opts(mode, border))


def mats_tensor(ms, width=9):
    """[matrix] -> device float32 [K, width], columns 9.. filled with a NaN the kernel must not read (tests/test_gpu_warps_dev.py's table, nine wide)"""
    assert width >= 9
    t = torch.full((len(ms), width), POISON, dtype=torch.float32)
    t[:, :9] = torch.tensor([[float(v) for v in m] for m in ms], dtype=torch.float64).to(torch.float32).reshape(-1, 9)
    return t.cuda()


def both(capi, orc, sf, W, H, dw, dh, ms, dtype, bgr, params, nhwc, padded, mode, cs=1, cr=0, max_step=0.0):
    """one call of each entry on the same matrices, two frames interleaved -> (device entry's buffer, host entry's buffer)"""
    devs = frames_of(orc, sf, W, H)
    fs = [i % 2 for i in range(len(ms))]
    a, b = make_buf(len(ms), dw, dh, dtype, nhwc, padded), make_buf(len(ms), dw, dh, dtype, nhwc, padded)
    run_dev(capi, sf, cs, cr, W, H, dw, dh, devs, mats_tensor(ms), index_tensor(fs), a, dtype, bgr, params, nhwc, max_step=max_step, mode=mode)
    run_host(capi, sf, cs, cr, W, H, dw, dh, devs, [(k, fs[k], m) for k, m in enumerate(ms)], b, dtype, bgr, params, nhwc, mode=mode)
    torch.cuda.synchronize()
    return a, b


# destination size -> (dtype, B G R, channels-last, padded rows)
VARIANTS = {(61, 35): (0, False, False, False), (64, 48): (1, False, False, True), (33, 33): (2, False, True, False), (24, 16): (0, True, True, False),
            (1, 40): (0, False, False, False)}


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("sf", ["NV12", "YUV420", "P10"])
def test_geometry(capi, orc, sf, mode):
    """every named matrix (the sawtooth on its 131 x 79 -> 33 x 33 shape among them) and every affine one with the last row (0, 0, 1), two frames
    interleaved, per border mode and destination size (partial tiles, whole tiles, one pixel past a tile, smaller than a tile, one column), on both
    frame sizes: byte for byte the host-table entry's buffer"""
    for (W, H) in ((131, 79), (130, 78)):
        for (dw, dh), (dtype, bgr, nhwc, padded) in VARIANTS.items():
            ms = persp.matrices(W, H, dw, dh)
            assert NAMED["sawtooth"][0] in ms
            a, b = both(capi, orc, sf, W, H, dw, dh, ms, dtype, bgr, ("imagenet", "unit", "symmetric")[dtype], nhwc, padded, mode)
            explain(a, b, ms, f"{sf} {W}x{H} -> {dw}x{dh} mode {mode}")


def test_against_the_oracle_chain(capi, orc):
    """the device entry against the CPU oracle directly (convert the whole frame, the definition's maps, remap, the fp64 evaluation of the epilogue):
    NV12 f32 planar replicate and YUV420 f16 channels-last B G R constant"""
    W, H, dw, dh = 131, 79, 61, 35
    for sf, dtype, bgr, nhwc, mode in (("NV12", 0, False, False, 1), ("YUV420", 1, True, True, 0)):
        ms = persp.matrices(W, H, dw, dh)
        fs = [i % 2 for i in range(len(ms))]
        buf = make_buf(len(ms), dw, dh, dtype, nhwc, False)
        run_dev(capi, sf, 1, 0, W, H, dw, dh, frames_of(orc, sf, W, H), mats_tensor(ms), index_tensor(fs), buf, dtype, bgr, "imagenet", nhwc, mode=mode)
        torch.cuda.synchronize()
        got, intact = buf.frames()
        assert intact
        for i, m in enumerate(ms):
            want = persp.want_bits(orc, sf, 1, 0, W, H, m, dw, dh, BORDER, mode, "imagenet", dtype, bgr, seed=fs[i])
            assert_bits(got[i], hwc(want) if nhwc else want, f"{sf} dtype {dtype} nhwc {nhwc} mode {mode} job {i} {m}")


@pytest.mark.parametrize("sf,nhwc", [("NV12", False), ("YUV420", True), ("P10", False)])
def test_the_hint_never_changes_a_pixel(capi, orc, sf, nhwc):
    """max_step = 1.0 with the 2.9 x down-scale (steep) and the keystone matrices in the call (the steep one's tiles outgrow the hinted LDS and take the
    in-kernel per-tap branch), max_step = 0 (the 64 KiB default), the jobs' true step (vpf_persp_max_step), and VPF_TUNE_NV12_RGB_VARIANT = 9 (no LDS
    at all): the host entry's bits, and the knob is back afterwards"""
    W, H, dw, dh = 131, 79, 64, 48
    ms = [NAMED[k][0] for k in ("down-scale", "keystone", "strong", "keystone x 3.7")] + persp.lifted(W, H, dw, dh)[:6]
    true = max(capi.persp_max_step(m, dw, dh) for m in ms)
    assert 2.9 < true < 1e3 and capi.persp_max_step(NAMED["down-scale"][0], dw, dh) > 2.9 > 1.0
    devs = frames_of(orc, sf, W, H)
    fs = [i % 2 for i in range(len(ms))]
    for mode in (0, 1):
        bufs = {}
        for step in (1.0, 0.0, true):
            bufs[step], host = both(capi, orc, sf, W, H, dw, dh, ms, 0, False, "imagenet", nhwc, False, mode, max_step=step)
            explain(bufs[step], host, ms, f"{sf} nhwc {nhwc} mode {mode} max_step {step}")
        c = make_buf(len(ms), dw, dh, 0, nhwc, False)
        prev = capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, 9)
        try:
            run_dev(capi, sf, 1, 0, W, H, dw, dh, devs, mats_tensor(ms), index_tensor(fs), c, 0, False, "imagenet", nhwc, mode=mode)
            torch.cuda.synchronize()
        finally:
            capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, prev)
        assert capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, prev) == prev  # the knob is back
        assert torch.equal(c.buf, bufs[0.0].buf) and torch.equal(c.buf, bufs[1.0].buf) and torch.equal(c.buf, bufs[true].buf), (sf, mode)


@pytest.mark.parametrize("nhwc", [False, True])
def test_count_strides_and_frame_index(capi, orc, nhwc):
    """count = 0: nothing is written; 3 of 7: jobs 3 .. 6 keep their canaries; 9 > max_n: all 7; negative: nothing; NULL: all 7; matrix_stride 36, 40
    and 48 (NaNs in the padding); a strided frame index; frame_index NULL against an explicit all-zero index"""
    W, H, dw, dh, sf, dtype = 130, 78, 64, 48, "NV12", 1
    devs = frames_of(orc, sf, W, H)
    ms = persp.matrices(W, H, dw, dh)[:7]
    fs = [i % 2 for i in range(7)]
    want = {}
    for c in (3, 7):
        want[c] = make_buf(7, dw, dh, dtype, nhwc, True)
        run_host(capi, sf, 1, 1, W, H, dw, dh, devs, [(k, fs[k], ms[k]) for k in range(c)], want[c], dtype, True, "symmetric", nhwc, mode=1)
    for name, count, width, istride, expect in (("zero", 0, 9, 1, None), ("three", 3, 9, 1, 3), ("nine", 9, 9, 1, 7), ("null", None, 9, 1, 7),
                                                 ("stride40", 3, 10, 1, 3), ("negative", -4, 9, 1, None), ("stride48_null", None, 12, 3, 7),
                                                 ("stride40_null", None, 10, 1, 7), ("index_stride", 3, 9, 5, 3)):
        buf = make_buf(7, dw, dh, dtype, nhwc, True)
        mats, index = mats_tensor(ms, width), index_tensor(fs, istride)
        assert mats.stride(0) == width and index.stride(0) == istride
        cnt = torch.tensor([count], dtype=torch.int32).cuda() if count is not None else None
        run_dev(capi, sf, 1, 1, W, H, dw, dh, devs, mats, index, buf, dtype, True, "symmetric", nhwc, count=cnt, mode=1)
        torch.cuda.synchronize()
        if expect is None:
            assert bool((buf.buf == CANARY).all()), name
        else:
            assert torch.equal(buf.buf, want[expect].buf), name
    # no frame index: every job samples frames[0] — what an explicit all-zero index gives, and what the host entry gives on frame 0
    a, b, h = (make_buf(7, dw, dh, dtype, nhwc, False) for _ in range(3))
    run_dev(capi, sf, 1, 1, W, H, dw, dh, devs, mats_tensor(ms), None, a, dtype, False, "imagenet", nhwc)
    run_dev(capi, sf, 1, 1, W, H, dw, dh, devs, mats_tensor(ms), index_tensor([0] * 7), b, dtype, False, "imagenet", nhwc)
    run_host(capi, sf, 1, 1, W, H, dw, dh, devs, [(k, 0, m) for k, m in enumerate(ms)], h, dtype, False, "imagenet", nhwc)
    torch.cuda.synchronize()
    assert torch.equal(a.buf, b.buf) and torch.equal(a.buf, h.buf)


def test_spare_jobs_beyond_the_tables(capi, orc):
    """max_n = 40 over tables of 5 matrices and 5 frame indices with count = 5: the 35 spare jobs read neither and write nothing (the buffer holds 5
    jobs: a write of job 5 would land in the canaries or behind the buffer)"""
    W, H, dw, dh, sf = 131, 79, 24, 16, "YUV420"
    devs = frames_of(orc, sf, W, H)
    ms = persp.matrices(W, H, dw, dh)[:5]
    fs = [i % 2 for i in range(5)]
    a, b = make_buf(5, dw, dh, 0, False, False), make_buf(5, dw, dh, 0, False, False)
    run_dev(capi, sf, 1, 0, W, H, dw, dh, devs, mats_tensor(ms), index_tensor(fs), a, 0, False, "unit", False, count=torch.tensor([5], dtype=torch.int32).cuda(),
            max_n=40)
    run_host(capi, sf, 1, 0, W, H, dw, dh, devs, [(k, fs[k], m) for k, m in enumerate(ms)], b, 0, False, "unit", False)
    torch.cuda.synchronize()
    assert torch.equal(a.buf, b.buf)


def test_invalid_entries_take_the_border(capi, orc):
    """NaN, +-inf and nextafter(2^24) in each third of the matrix (the last row included), frames -1, n_frames, INT32_MIN and INT32_MAX, among valid
    jobs: an invalid job is the epilogue of border[c] in every element in BOTH modes (B G R: the border per OUTPUT channel), coefficients of exactly
    +-2^24 are valid and equal the host entry, the valid jobs are the host entry's bits, the canaries are intact.  (The guard itself is proven on the
    CPU, tests/test_persps_dev_bounds_cpu.py: this checks the fill.)"""
    W, H, dw, dh, sf = 131, 79, 61, 35, "NV12"
    devs = frames_of(orc, sf, W, H)
    nan, inf, above = math.nan, math.inf, float(np.nextafter(np.float32(LIMIT), np.float32(np.inf)))
    g = persp.matrices(W, H, dw, dh)
    key, ident = NAMED["keystone"][0], (1, 0, 33, 0, 1, 5, 0, 0, 1)
    table = [(0, key), (1, (nan, 0, 33, 0, 1, 5, 0, 0, 1)), (0, (1, inf, 33, 0, 1, 5, 0, 0, 1)), (1, g[2]), (0, (1, 0, -inf, 0, 1, 5, 0, 0, 1)),
             (1, (1, 0, 33, above, 1, 5, 0, 0, 1)), (0, (1, 0, LIMIT, 0, 1, 5, 0, 0, 1)), (1, (1, 0, 33, 0, -above, 5, 0, 0, 1)), (-1, key), (2, key),
             (1, (1, 0, 33, 0, 1, nan, 0, 0, 1)), (-2 ** 31, key), (1, (-LIMIT, 0, 100, 0, 1, 2, 0, 0, 1)), (0, (0, 0, 5.5, 0, 0, -LIMIT, 0, 0, 1)), (1, g[4]),
             (2 ** 31 - 1, key), (0, (nan,) * 9), (0, (1, 0, 33, 0, 1, 5, nan, 0, 1)), (1, (1, 0, 33, 0, 1, 5, 0, -inf, 1)), (0, (1, 0, 33, 0, 1, 5, 0, 0, above)),
             (1, (1, 0, 33, 0, 1, 5, 0, 0, inf)), (0, (1, 0, 33, 0, 1, 5, -above, 0, 1)), (1, (1, 0, 33, 0, 1, 5, 0, 0, LIMIT)), (0, (1, 0, 33, 0, 1, 5, -LIMIT, 0, 1)),
             (1, (1, 0, 33, 0, 1, 5, 0, LIMIT, -LIMIT)), (0, ident)]
    valid = [0 <= f < 2 and all(abs(v) <= LIMIT for v in m) for (f, m) in table]
    assert sum(valid) == 10 and len(table) - sum(valid) == 16
    for dtype, bgr, nhwc, padded, mode in ((0, False, False, False, 0), (2, True, True, True, 1), (1, True, False, True, 0), (0, False, True, False, 1)):
        a, b = make_buf(len(table), dw, dh, dtype, nhwc, padded), make_buf(len(table), dw, dh, dtype, nhwc, padded)
        run_dev(capi, sf, 1, 0, W, H, dw, dh, devs, mats_tensor([m for _, m in table]), index_tensor([f for f, _ in table]), a, dtype, bgr, "imagenet", nhwc,
                mode=mode)
        run_host(capi, sf, 1, 0, W, H, dw, dh, devs, [(k, f, m) for k, (f, m) in enumerate(table) if valid[k]], b, dtype, bgr, "imagenet", nhwc, mode=mode)
        torch.cuda.synchronize()
        got, intact = a.frames()
        want = b.frames()[0]
        assert intact
        rgb_border = BORDER[::-1] if bgr else BORDER   # reference_bits takes R G B planes: output channel c of B G R is R G B channel 2 - c
        fill = reference_bits(np.stack([np.full((dh, dw), v, np.uint8) for v in rgb_border]), *PARAMS["imagenet"], dtype, bgr)
        fill = hwc(fill) if nhwc else fill
        for k in range(len(table)):
            assert_bits(got[k], want[k] if valid[k] else fill, f"dtype {dtype} bgr {bgr} nhwc {nhwc} mode {mode} job {k} {table[k]} valid {valid[k]}")


@pytest.mark.parametrize("sf,nhwc,mode", [("NV12", False, 0), ("YUV420", True, 1), ("P10", False, 1)])
def test_affine_matrices_equal_the_affine_device_entry(capi, orc, sf, nhwc, mode):
    """last row (0, 0, 1): the buffer of vpf_convert_warp_tensor_dev on the first six coefficients, byte for byte"""
    W, H, dw, dh = 131, 79, 64, 48
    devs = frames_of(orc, sf, W, H)
    six = geometry_jobs(W, H, dw, dh)
    fs = [i % 2 for i in range(len(six))]
    a, b = make_buf(len(six), dw, dh, 1, nhwc, True), make_buf(len(six), dw, dh, 1, nhwc, True)
    run_dev(capi, sf, 1, 0, W, H, dw, dh, devs, mats_tensor([tuple(m) + (0, 0, 1) for m in six], 12), index_tensor(fs, 2), a, 1, True, "imagenet", nhwc, mode=mode)
    wide = torch.full((len(six), 8), POISON, dtype=torch.float32)
    wide[:, :6] = torch.tensor([[float(v) for v in m] for m in six], dtype=torch.float64).to(torch.float32)
    run_affine_dev(capi, sf, 1, 0, W, H, dw, dh, devs, wide.cuda(), index_tensor(fs), b, 1, True, "imagenet", nhwc, mode=mode)
    torch.cuda.synchronize()
    explain(a, b, six, f"{sf} nhwc {nhwc} mode {mode}: vpf_convert_warp_tensor_dev on the first six coefficients")


def test_graph_replays_with_live_tables(capi, orc):
    """one call captured on a side stream (one stream, no parallel branches; called once eagerly first), replayed three times; matrices, frame indices
    and count are overwritten on that stream between the replays: each replay equals the host entry on THAT replay's tables"""
    W, H, dw, dh, sf, dtype = 131, 79, 64, 48, "NV12", 0
    devs = frames_of(orc, sf, W, H)
    g = persp.matrices(W, H, dw, dh)
    sets = [(g[:6], [i % 2 for i in range(6)], 6), (g[5:11], [(i + 1) % 2 for i in range(6)], 4)]
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        live_m, live_i = mats_tensor(sets[0][0]), index_tensor(sets[0][1])
        count = torch.tensor([sets[0][2]], dtype=torch.int32).cuda()
        staged = [(mats_tensor(m), index_tensor(f), torch.tensor([c], dtype=torch.int32).cuda()) for (m, f, c) in sets]
        buf = make_buf(6, dw, dh, dtype, False, False)
        run_dev(capi, sf, 1, 0, W, H, dw, dh, devs, live_m, live_i, buf, dtype, False, "imagenet", False, count=count, stream=st.cuda_stream)  # (eager once: the code object is loaded)
        st.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st):
            run_dev(capi, sf, 1, 0, W, H, dw, dh, devs, live_m, live_i, buf, dtype, False, "imagenet", False, count=count, stream=st.cuda_stream)
        for rep in (1, 0, 1):
            ms, fs, c = sets[rep]
            live_m.copy_(staged[rep][0])
            live_i.copy_(staged[rep][1])
            count.copy_(staged[rep][2])
            buf.buf.fill_(CANARY)
            graph.replay()
            want = make_buf(6, dw, dh, dtype, False, False)
            run_host(capi, sf, 1, 0, W, H, dw, dh, devs, [(k, fs[k], ms[k]) for k in range(c)], want, dtype, False, "imagenet", False, stream=st.cuda_stream)
            st.synchronize()
            assert torch.equal(buf.buf, want.buf), rep


def _nvc():
    sys.path.insert(0, os.path.join(ROOT, "videoprocessingframework_amd"))
    import PyNvCodec as nvc
    from videoprocessingframework_amd import PytorchNvCodec as pnc

    return nvc, pnc


def test_python_path(orc):
    """device_persps_to_normalized_tensor == persps_to_normalized_tensor (torch.equal) on the same matrices: planar and channels_last, bf16 + bgr,
    replicate, `out` as a slice of a larger tensor whose other frames keep their bits, a count, a [K, 9] slice of a wider table, a P10 surface;
    quads_to_homographies_unchecked on the device feeds it, and a row of NaN corners gives the normalised border"""
    nvc, pnc = _nvc()
    PF = nvc.PixelFormat
    W, H, dw, dh = 130, 78, 61, 35  # (even: a semi-planar Surface of the Task layer is one plane, chroma rows included)
    mean, std = PARAMS["imagenet"]
    cc = nvc.ColorspaceConversionContext(nvc.ColorSpace.BT_709, nvc.ColorRange.JPEG)
    surfs = [_upload(nvc, frame(orc, "NV12", W, H, seed)[0], W, H) for seed in range(2)]
    torch.cuda.synchronize()
    ms = persp.matrices(W, H, dw, dh)[:9]
    index = [i % 2 for i in range(len(ms))]
    host = torch.tensor(ms, dtype=torch.float64).to(torch.float32).reshape(-1, 3, 3)
    mats, idx = host.cuda(), torch.tensor(index, dtype=torch.int32).cuda()
    rs = nvc.PySurfaceConvertResizer(W, H, PF.NV12, dw, dh, PF.RGB_PLANAR, 0)  # its own non-blocking stream
    step = pnc.homographies_max_step(host[:4], dw, dh)
    assert step > 0
    for kw in (dict(), dict(channels_last=True, border=BORDER), dict(dtype=torch.bfloat16, bgr=True, border=BORDER, border_mode="replicate"),
               dict(dtype=torch.float16, channels_last=True, bgr=True, border=BORDER)):
        want = pnc.persps_to_normalized_tensor(rs, surfs, index, host, mean, std, cc_ctx=cc, **kw)
        for hint in (None, step):
            got = pnc.device_persps_to_normalized_tensor(rs, surfs, mats, mean, std, surface_index=idx, max_step=hint, cc_ctx=cc, **kw)
            assert got.shape == want.shape and got.dtype == want.dtype and got.stride() == want.stride(), kw
            assert torch.equal(got, want), (kw, hint)
    # no surface index: surface 0
    want = pnc.persps_to_normalized_tensor(rs, surfs, [0] * len(ms), host, mean, std, cc_ctx=cc)
    assert torch.equal(pnc.device_persps_to_normalized_tensor(rs, surfs, mats, mean, std, cc_ctx=cc), want)
    # a count and a [K, 9] slice of a wider table, into a slice of a larger batch
    wide = torch.full((len(ms), 13), POISON, dtype=torch.float32, device="cuda")
    wide[:, 2:11] = mats.reshape(-1, 9)
    big = torch.full((len(ms) + 3, 3, dh, dw), 0x3C3C, dtype=torch.int16, device="cuda")
    view = big.view(torch.float16)[2:2 + len(ms)]
    res = pnc.device_persps_to_normalized_tensor(rs, surfs, wide[:, 2:11], mean, std, surface_index=idx, count=torch.tensor([3], dtype=torch.int32, device="cuda"),
                                                 dtype=torch.float16, border=BORDER, out=view, cc_ctx=cc)
    assert res.data_ptr() == view.data_ptr()
    want = pnc.persps_to_normalized_tensor(rs, surfs, index[:3], host[:3], mean, std, dtype=torch.float16, border=BORDER, cc_ctx=cc)
    assert torch.equal(view[:3], want)
    assert bool((big[:2] == 0x3C3C).all()) and bool((big[5:] == 0x3C3C).all())   # rows at or behind the count are not written
    # a corner-regression network's quads, solved on the device without a sync
    quads = torch.tensor([[[10, 5], [100, 12], [110, 70], [4, 60]], [[30, 2], [90, 2], [90, 50], [30, 50]], [[120, 70], [20, 75], [5, 3], [125, 8]],
                          [[math.nan, 10], [60, -5], [150, 90], [10, 60]], [[-20, 10], [60, -5], [150, 90], [10, 60]]], dtype=torch.float64, device="cuda")
    qidx = torch.tensor([0, 1, 1, 0, 1], dtype=torch.int32, device="cuda")
    hs = pnc.quads_to_homographies_unchecked(quads, (dw, dh))
    assert hs.is_cuda and hs.dtype == torch.float32 and tuple(hs.shape) == (5, 3, 3)
    got = pnc.device_persps_to_normalized_tensor(rs, surfs, hs, mean, std, surface_index=qidx, border=BORDER, cc_ctx=cc)
    keep = [0, 1, 2, 4]
    want = pnc.persps_to_normalized_tensor(rs, surfs, [0, 1, 1, 1], hs.cpu()[keep], mean, std, border=BORDER, cc_ctx=cc)
    assert torch.equal(got[keep], want)
    assert torch.equal(hs[keep], pnc.quads_to_homographies(quads[keep], (dw, dh)))   # proper quads: the checked solve's tensor
    fill = reference_bits(np.stack([np.full((dh, dw), v, np.uint8) for v in BORDER]), mean, std, 0, False)
    assert not bool(torch.isfinite(hs[3]).all())
    assert torch.equal(got[3], torch.from_numpy(fill.view(np.float32)).cuda())    # the NaN row: an invalid job, the normalised border
    # a P10 surface
    up = nvc.PyFrameUploader(W, H, PF.P10, 0)
    p10 = [up.UploadSingleFrame(np.concatenate([p.reshape(-1) for p in p16.p16_frame(orc, "P10", W, H, s)])).Clone(0) for s in range(2)]
    torch.cuda.synchronize()
    rs10 = nvc.PySurfaceConvertResizer(W, H, PF.P10, dw, dh, PF.RGB_PLANAR, 0)
    want = pnc.persps_to_normalized_tensor(rs10, p10, index, host, mean, std, dtype=torch.float16, cc_ctx=cc)
    got = pnc.device_persps_to_normalized_tensor(rs10, p10, mats.reshape(-1, 9), mean, std, surface_index=idx, dtype=torch.float16, cc_ctx=cc)
    assert torch.equal(got, want)
    for bad in (dict(matrices=host), dict(matrices=mats.to(torch.float64)), dict(matrices=mats.reshape(-1, 9)[:, :6]), dict(surface_index=idx.cpu()),
                dict(surface_index=idx.to(torch.int64)), dict(surface_index=idx[:3]), dict(count=torch.tensor([3], dtype=torch.int32)),
                dict(count=torch.tensor([3, 3], dtype=torch.int32, device="cuda")), dict(max_step=-1.0), dict(max_step=math.nan),
                dict(matrices=mats.reshape(-1, 9).t().contiguous().t())):
        kw = dict(matrices=mats, surface_index=idx)
        kw.update(bad)
        m = kw.pop("matrices")
        with pytest.raises(ValueError):
            pnc.device_persps_to_normalized_tensor(rs, surfs, m, mean, std, **kw)
    with pytest.raises(ValueError, match=r"\.cpu\(\)"):
        pnc.persps_to_normalized_tensor(rs, surfs, index, mats, mean, std)        # the host-table entry refuses device matrices as before


@pytest.mark.parametrize("seed", pcases.seeds())  # soak: VPF_FUZZ_SEEDS=500 (VPF_FUZZ_FIRST=n: seeds n .. n + VPF_FUZZ_SEEDS - 1, fresh cases)
def test_fuzz_persps_dev(capi, orc, seed):
    """vpf_convert_persp_tensor_dev on tests/cases_persps_dev.py: the nine classes of homographies, padded matrix tables with NaNs in the padding, a
    strided frame index, a count, invalid entries (the border in both modes), no hint or a true bound.  Every written job is bit-identical to the
    composed oracle reference of the persp family and to the host-table entry, jobs behind the count keep the canary, so does every other byte"""
    for k, call in enumerate(pcases.cases(seed)):
        what = f"persp_dev seed {seed} case {k}"
        srcs, devs = upload_frames(orc, call)
        descs = [d.desc() for d in devs]
        n, i32 = call["max_n"], torch.int32
        count = torch.tensor([call["count"]], dtype=i32).cuda() if call["count"] is not None else None
        mats = torch.full((n, call["mat_floats"]), POISON, dtype=torch.float32)
        mats[:, :9] = torch.tensor(call["mats"], dtype=torch.float64).to(torch.float32)
        index = torch.full((n, call["index_ints"]), 0x5A5A5A5A, dtype=i32)
        index[:, 0] = torch.tensor(call["index"], dtype=torch.int64).to(i32)
        keep = [mats.cuda(), index.cuda()]
        tables = dict(mats=keep[0].data_ptr(), index=keep[1].data_ptr(), count=count.data_ptr() if count is not None else None)
        a, b = dev_buf(call), dev_buf(call)
        ex = capi.make_exec(stream_handle())
        tuned(capi, call, lambda: (pcases.invoke(capi, call, ex, descs, a.buf.data_ptr(), tables), pcases.invoke_host(capi, call, ex, descs, b.buf.data_ptr())))
        (got, intact), (host, host_intact) = a.frames(), b.frames()
        jobs, c = host_jobs(call)
        jobs = dict(jobs)
        rgb = rgb_frames(orc, call, srcs)
        fill = want_of(call, np.broadcast_to(np.array(rgb_order(call, call["border"]), np.uint8).reshape(3, 1, 1), (3, call["dh"], call["dw"])))
        blank = np.full(got[0].shape, 0xCDCDCDCD if ELEM[call["dtype"]] == 4 else 0xCDCD, got.dtype)
        for i in range(n):
            tag = f"{what} job {i}: {call!r}"
            if i >= c:
                assert_bits(got[i], blank, "a job behind the count was written: " + tag)
                assert_bits(host[i], blank, "host-table entry, a job that was not passed: " + tag)
            elif i in jobs:
                assert_bits(got[i], want_of(call, job_u8(orc, call, jobs[i], rgb[jobs[i]["frame"]])), tag)
                assert_bits(got[i], host[i], "device entry != host-table entry: " + tag)
            else:
                assert_bits(got[i], fill, "the fill of an invalid entry: " + tag)
        assert intact and host_intact, f"{what}: bytes outside the jobs' elements were written: {call!r}"
    forget_p16()
