"""The per-job kernels (k_roi_strip, k_roi_gather, k_warp_strip, k_warp_gather and their channels-last forms) at the shapes the sibling files
do not reach: destinations wider than one 256-column chunk, full 64-lane waves, second and third chunks and bands, frame columns up to 4100,
tiles beyond the first in x and y, and the FC_P16 instantiations of the channels-last forms.  The case table is tests/cases_job_shapes.py;
tests/test_job_bounds_cpu.py checks on the CPU which of its jobs the policy stages and which gather, the child process here reads it off
the kernel-selection log.

Ground truth is the CPU oracle, composed exactly as the sibling files compose it (roi.ref_u8 / warp.want_bits; P10: the 16-bit tests' planted
frames through oracle.convert(P10 -> NV12) first; channels-last: the planar reference transposed).  Every comparison is on bit patterns, every
destination keeps its canaries, nothing takes a tolerance.  Frames are wide and short: large coordinates, a few milliseconds of oracle."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cases_job_shapes as cases
import test_gpu_p16_tensor as p16
import test_gpu_roi_tensor as roi
import test_gpu_warp_tensor as warp
from gpu_util import DevPlanes, stream_handle
from test_gpu_tensor_nhwc import NhwcBuf, hwc
from test_gpu_tensor_out import ELEM, MATRICES, PARAMS, TensorBuf, assert_bits, reference_bits
from test_roi_tensor_cpu import roi_reference_u8
from test_warp_tensor_cpu import warp_reference_u8

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = ["NV12", "YUV420", "P10"]
PARAM_NAMES = ("imagenet", "unit", "symmetric")
BORDER = (10, 128, 250)
DEST_IDS = [f"{dw}x{dh}" for dw, dh in cases.ROI_DESTS]


@pytest.fixture(scope="module")
def orc(oracle):
    oracle.set_threads(16)
    return oracle


_DEV, _ROI_REFS, _WARP_REFS = {}, {}, {}


def dev_frame(orc, sf, W, H, kind):
    """device planes of the frame the references of `kind` ('roi' / 'warp') are computed from"""
    if sf == "P10":
        if (W, H) not in _DEV:
            _DEV[(W, H)] = DevPlanes(p16.p16_frame(orc, "P10", W, H, 0), align=64, extra=2)   # rows start at addresses that are only 2-B aligned
        return _DEV[(W, H)]
    return (roi if kind == "roi" else warp).frame(orc, sf, W, H)[1]


def roi_u8(orc, sf, cs, cr, W, H, rect, dw, dh):
    """[3, dh, dw] reference bytes of one ROI job, computed once per key and never modified"""
    if sf != "P10":
        return roi.ref_u8(orc, sf, cs, cr, W, H, rect, dw, dh)
    key = (cs, cr, W, H, rect, dw, dh)
    if key not in _ROI_REFS:
        _ROI_REFS[key] = roi_reference_u8(orc, "NV12", cs, cr, W, H, None, rect, dw, dh, rgb=p16.rgb_of(orc, "P10", cs, cr, W, H, 0))
        _ROI_REFS[key].setflags(write=False)
    return _ROI_REFS[key]


def warp_bits(orc, sf, cs, cr, W, H, m, dw, dh, mode, params, dtype, bgr):
    """planar reference bits [3, dh, dw] of one warp job; BORDER is per output channel (warp.want_bits)"""
    if sf != "P10":
        return warp.want_bits(orc, sf, cs, cr, W, H, m, dw, dh, BORDER, mode, params, dtype, bgr)
    rgb_border = tuple(BORDER[::-1]) if bgr else BORDER
    key = (cs, cr, W, H, tuple(float(np.float32(v)) for v in m), dw, dh, rgb_border, mode)
    if key not in _WARP_REFS:
        _WARP_REFS[key] = warp_reference_u8(orc, "NV12", cs, cr, W, H, m, dw, dh, rgb_border, mode, rgb=p16.rgb_of(orc, "P10", cs, cr, W, H, 0))
        _WARP_REFS[key].setflags(write=False)
    return reference_bits(_WARP_REFS[key], *PARAMS[params], dtype, bgr)


class tuned:
    """VPF_TUNE_NV12_RGB_VARIANT = variant inside the block (9: every job takes the per-tap kernel)"""

    def __init__(self, capi, variant):
        self.capi, self.variant = capi, variant

    def __enter__(self):
        self.prev = self.capi.set_tuning(self.capi.TUNE_NV12_RGB_VARIANT, self.variant)

    def __exit__(self, *exc):
        self.capi.set_tuning(self.capi.TUNE_NV12_RGB_VARIANT, self.prev)


def run_rois(capi, sf, cs, cr, W, H, dw, dh, dev, rects, dtype, bgr, params, buf, nhwc=False, variant=0):
    norm = capi.make_tensor_norm(*PARAMS[params], dtype=dtype, bgr=bgr, nhwc=nhwc)
    rois = capi.make_rois([(dev.desc(), buf.planes(i), r) for i, r in enumerate(rects)])
    with tuned(capi, variant):
        capi.convert_resize_tensor_rois(capi.make_exec(stream_handle()), getattr(capi, sf), cs, cr, W, H, dw, dh, rois, norm)
        torch.cuda.synchronize()


def run_warps(capi, sf, cs, cr, W, H, dw, dh, dev, mats, dtype, bgr, params, buf, mode, nhwc=False, variant=0):
    norm = capi.make_tensor_norm(*PARAMS[params], dtype=dtype, bgr=bgr, nhwc=nhwc)
    table = capi.make_warps([(dev.desc(), buf.planes(i), m) for i, m in enumerate(mats)])
    with tuned(capi, variant):
        capi.convert_warp_tensor(capi.make_exec(stream_handle()), getattr(capi, sf), cs, cr, W, H, dw, dh, table, norm, capi.make_warp_opts(mode, BORDER))
        torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ ROIs
@pytest.mark.parametrize("dest", cases.ROI_DESTS, ids=DEST_IDS)
@pytest.mark.parametrize("sf", SOURCES)
def test_roi_wide_destinations(capi, orc, sf, dest):
    """one call per (source format, destination size, frame) with every rectangle of the table: f32 planar on the three frames, the (colour space,
    range) pairs rotating; on the 1100 x 40 frame once more in f16 / bf16, R G B / B G R and another parameter set, rotating through the
    cases, and once under tuning 9 (every job gathers), whose whole buffer must equal the default policy's"""
    dw, dh = dest
    k = SOURCES.index(sf) * len(cases.ROI_DESTS) + cases.ROI_DESTS.index(dest)
    for fi, (W, H) in enumerate(cases.FRAMES):
        dev = dev_frame(orc, sf, W, H, "roi")
        rects = cases.roi_rects(W, H, dw, dh)
        runs = [(0, False, "imagenet", MATRICES[(k + fi) % 4], 0)]
        if fi == 0:
            runs += [(0, False, "imagenet", MATRICES[(k + fi) % 4], 9), (1 + k % 2, k % 3 != 0, PARAM_NAMES[k % 3], MATRICES[(k + 1) % 4], 0)]
        first = None
        for dtype, bgr, params, (cs, cr), variant in runs:
            buf = TensorBuf(len(rects), dw, dh, ELEM[dtype])
            run_rois(capi, sf, cs, cr, W, H, dw, dh, dev, rects, dtype, bgr, params, buf, variant=variant)
            got, intact = buf.frames()
            what = f"{sf} {W}x{H} -> {dw}x{dh} cs{cs} cr{cr} dtype{dtype} bgr{bgr} {params} variant {variant}"
            assert intact, what
            for i, r in enumerate(rects):
                assert_bits(got[i], reference_bits(roi_u8(orc, sf, cs, cr, W, H, r, dw, dh), *PARAMS[params], dtype, bgr), f"{what} rect {r}")
            if variant == 9:
                assert torch.equal(buf.buf, first.buf), what + ": the gather form's buffer differs from the default policy's"
            elif first is None:
                first = buf


@pytest.mark.parametrize("dest", cases.ROI_DESTS, ids=DEST_IDS)
def test_roi_wide_destinations_nhwc(capi, orc, dest):
    """the same table into ONE interleaved plane per job: f32 for every size and source format (P10 included), f16 and bf16 at 256 x 20 and
    258 x 17; rows contiguous (f32: the dense hand-off through LDS with 64 active lanes; 16-bit: per-lane vectors) and padded by 16 B + 1 element
    (element stores); bit-identical to the transposed planar reference and to the planar call of the same library"""
    dw, dh = dest
    di = cases.ROI_DESTS.index(dest)
    dtypes = (0, 1, 2) if dest in ((256, 20), (258, 17)) else (0,)
    for si, sf in enumerate(SOURCES):
        W, H = cases.FRAMES[0] if (si + di) % 3 else cases.FRAMES[2]   # the 4100-wide frame takes each source format at two of the sizes
        dev = dev_frame(orc, sf, W, H, "roi")
        rects = cases.roi_rects(W, H, dw, dh)
        cs, cr = MATRICES[(si + di) % 4]
        for dtype in dtypes:
            e = ELEM[dtype]
            bgr, params = (si + di + dtype) % 2 == 1, PARAM_NAMES[(di + dtype) % 3]
            planar = TensorBuf(len(rects), dw, dh, e)
            run_rois(capi, sf, cs, cr, W, H, dw, dh, dev, rects, dtype, bgr, params, planar)
            pgot, pintact = planar.frames()
            assert pintact
            for lname, row in (("contiguous", 0), ("padded_16B_plus_1", 3 * dw * e + 16 + e)):
                buf = NhwcBuf(len(rects), dw, dh, e, row=row)
                run_rois(capi, sf, cs, cr, W, H, dw, dh, dev, rects, dtype, bgr, params, buf, nhwc=True)
                got, intact = buf.frames()
                what = f"nhwc {lname} {sf} {W}x{H} -> {dw}x{dh} cs{cs} cr{cr} dtype{dtype} bgr{bgr} {params}"
                assert intact, what
                for i, r in enumerate(rects):
                    assert_bits(got[i], hwc(reference_bits(roi_u8(orc, sf, cs, cr, W, H, r, dw, dh), *PARAMS[params], dtype, bgr)), f"{what} rect {r}")
                    assert np.array_equal(got[i], hwc(pgot[i])), f"{what} rect {r}: differs from the planar call"


# ------------------------------------------------------------------------------------------------ warps
@pytest.mark.parametrize("dest", cases.WARP_DESTS, ids=[f"{dw}x{dh}" for dw, dh in cases.WARP_DESTS])
@pytest.mark.parametrize("frame", cases.WARP_FRAMES, ids=[f"{W}x{H}" for W, H in cases.WARP_FRAMES])
@pytest.mark.parametrize("sf", SOURCES)
def test_warp_wide_frames_and_nhwc_tiles(capi, orc, sf, frame, dest):
    """72 x 40 (three tiles in x, the last 8 columns wide, two in y) and 224 x 8 (seven tiles of 8 rows) from frame columns up to 1100 / 4100:
    identity on the right edge, 30 degrees x 1.3, a flip, 2.9 x and 7 x down-scales, 23 x (the gather class), wholly and half outside.  Both
    border modes; planar f32 and channels-last in three dtypes and both channel orders with a per-channel border; the default policy and
    tuning 9 (every job per tap)"""
    (W, H), (dw, dh) = frame, dest
    k = SOURCES.index(sf) + cases.WARP_FRAMES.index(frame) + cases.WARP_DESTS.index(dest)
    cs, cr = MATRICES[k % 4]
    dev = dev_frame(orc, sf, W, H, "warp")
    mats = cases.warp_mats(W, H, dw, dh)
    for mode in (0, 1):
        runs = [(False, 0, False, 0), (False, 0, False, 9), (True, 0, True, 9)]
        runs += [(True, dtype, bgr, 0) for dtype in (0, 1, 2) for bgr in (False, True)]
        for nhwc, dtype, bgr, variant in runs:
            params = PARAM_NAMES[(dtype + bgr) % 3]
            buf = NhwcBuf(len(mats), dw, dh, ELEM[dtype]) if nhwc else TensorBuf(len(mats), dw, dh, ELEM[dtype])
            run_warps(capi, sf, cs, cr, W, H, dw, dh, dev, mats, dtype, bgr, params, buf, mode, nhwc=nhwc, variant=variant)
            got, intact = buf.frames()
            what = f"{sf} {W}x{H} -> {dw}x{dh} mode{mode} nhwc{nhwc} dtype{dtype} bgr{bgr} variant {variant}"
            assert intact, what
            for i, m in enumerate(mats):
                want = warp_bits(orc, sf, cs, cr, W, H, m, dw, dh, mode, params, dtype, bgr)
                assert_bits(got[i], hwc(want) if nhwc else want, f"{what} job {i} {m}")


# ------------------------------------------------------------------------------------------------ the kernel-selection log
@pytest.fixture(scope="module")
def logs():
    """one child process under VPF_HIP_LOG=2: every (frame, destination size) ROI call of the table on NV12 planar; the ROI and warp calls on P10
    into channels-last planes under the default policy and under tuning 9 -> {case name: launch lines}"""
    roi_calls = [(f"roi_{W}x{H}_{dw}x{dh}", W, H, dw, dh, cases.roi_rects(W, H, dw, dh)) for W, H in cases.FRAMES for dw, dh in cases.ROI_DESTS]
    (W, H), (dw, dh) = cases.WARP_FRAMES[0], cases.WARP_DESTS[0]
    code = f"""
import sys
sys.path.insert(0, {ROOT!r})
import torch
from videoprocessingframework_amd import capi
ex = capi.make_exec(torch.cuda.current_stream().cuda_stream)
def frame(W, H, e):
    p = (W * e + 255) // 256 * 256
    y = torch.zeros(p * (H + (H + 1) // 2) + 4096, dtype=torch.uint8, device="cuda")
    return y, [(y.data_ptr(), p), (y.data_ptr() + p * H, p)]
norm = capi.make_tensor_norm((0, 0, 0), (1, 1, 1))
cl = capi.make_tensor_norm((0, 0, 0), (1, 1, 1), nhwc=True)
for name, W, H, dw, dh, rects in {roi_calls!r}:
    keep, src = frame(W, H, 1)
    out = torch.empty((len(rects), 3, dh, dw), dtype=torch.float32, device="cuda")
    print("CASE", name, file=sys.stderr, flush=True)
    capi.convert_resize_tensor_rois(ex, capi.NV12, 1, 0, W, H, dw, dh,
                                    capi.make_rois([(src, [(out[i, c].data_ptr(), 4 * dw) for c in range(3)], r) for i, r in enumerate(rects)]), norm)
    torch.cuda.synchronize()
W, H, dw, dh = {(W, H, dw, dh)!r}
keep, src = frame(W, H, 2)
rects, mats = {cases.roi_rects(W, H, 256, 20)!r}, {cases.warp_mats(W, H, dw, dh)!r}
for variant in (0, 9):
    prev = capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, variant)
    out = torch.empty((len(rects), 20, 256, 3), dtype=torch.float32, device="cuda")
    print("CASE", "p10_roi%d" % variant, file=sys.stderr, flush=True)
    capi.convert_resize_tensor_rois(ex, capi.P10, 1, 0, W, H, 256, 20,
                                    capi.make_rois([(src, [(out[i].data_ptr(), 12 * 256), (0, 0), (0, 0)], r) for i, r in enumerate(rects)]), cl)
    torch.cuda.synchronize()
    out = torch.empty((len(mats), dh, dw, 3), dtype=torch.float32, device="cuda")
    print("CASE", "p10_warp%d" % variant, file=sys.stderr, flush=True)
    capi.convert_warp_tensor(ex, capi.P10, 1, 0, W, H, dw, dh,
                             capi.make_warps([(src, [(out[i].data_ptr(), 12 * dw), (0, 0), (0, 0)], m) for i, m in enumerate(mats)]), cl, capi.make_warp_opts(0, (1, 2, 3)))
    torch.cuda.synchronize()
    capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, prev)
print("done")
"""
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, VPF_HIP_LOG="2"), timeout=300)
    assert r.returncode == 0 and "done" in r.stdout, r.stdout + r.stderr
    out = {}
    for chunk in r.stderr.split("CASE ")[1:]:
        name, rest = chunk.split("\n", 1)
        out[name.strip()] = [l for l in rest.split("\n") if "libvpfhip: launch" in l]
    return out


def test_every_roi_call_launches_both_forms(logs):
    """each (frame, destination size) call of the ROI table is two dispatches: its staged jobs, then its gather jobs"""
    names = [f"roi_{W}x{H}_{dw}x{dh}" for W, H in cases.FRAMES for dw, dh in cases.ROI_DESTS]
    for name in names:
        lines = logs[name]
        print(name, lines)
        assert len(lines) == 2 and "k_roi_strip<" in lines[0] and "k_roi_gather<" in lines[1], (name, lines)


def test_log_names_p16_nhwc_job_kernels(logs):
    """the FC_P16 instantiations of the four channels-last per-job kernels are what the P10 calls of this file run (the log carries the template-ids
    of the code object: FC_P16 = 7, FC_TENSOR_NHWC = 8)"""
    for name in ("p10_roi0", "p10_roi9", "p10_warp0", "p10_warp9"):
        print(name, logs[name])
    assert len(logs["p10_roi0"]) == 2 and "k_roi_strip<7, 8>" in logs["p10_roi0"][0] and "k_roi_gather<7, 8>" in logs["p10_roi0"][1], logs["p10_roi0"]
    assert len(logs["p10_roi9"]) == 1 and "k_roi_gather<7, 8>" in logs["p10_roi9"][0], logs["p10_roi9"]
    assert len(logs["p10_warp0"]) == 2 and "k_warp_strip<7, 8>" in logs["p10_warp0"][0] and "k_warp_gather<7, 8>" in logs["p10_warp0"][1], logs["p10_warp0"]
    assert len(logs["p10_warp9"]) == 1 and "k_warp_gather<7, 8>" in logs["p10_warp9"][0], logs["p10_warp9"]
