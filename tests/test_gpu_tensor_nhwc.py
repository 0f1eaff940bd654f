"""Channels-last (NHWC) tensors in the fused tensor entries on the MI355X (VPF_TENSOR_NHWC): vpf_convert_resize_tensor(_batch),
vpf_convert_resize_tensor_rois, vpf_convert_warp_tensor write ONE interleaved plane per frame / job, vpf_tensor_convert(_batch) reads one, and the
Python layers pass torch.channels_last tensors through.

There is nothing new to pin: element (y, x, c) of the interleaved plane is bit for bit element (c, y, x) of the planar call.  So the expected bits
are the existing planar references (tests/test_gpu_tensor_out.py::reference_bits on the oracle's RGB_PLANAR bytes; the ROI, warp and 16-bit
tests' references; the way back: tests/test_gpu_tensor_in.py::reference) transposed to (H, W, 3).  All comparisons are on bit patterns.  Every
destination carries canary bytes before the first row, in every row's padding and behind the last row, which must come back untouched, and the
two planes the flag makes the library ignore are passed as zero.

The shapes are the smallest at which the store path can still go wrong (rows shorter than, equal to and longer than a wave's 256 / 512 pixels,
widths that are no multiple of 4, tall narrow pictures that reach the 4-, 8- and 16-row bands of the workgroup strip with few bytes)."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import test_gpu_p16_tensor as p16
import test_gpu_roi_tensor as roi
import test_gpu_tensor_in as tin
import test_gpu_warp_tensor as warp
from cases_fused_families import FAMILIES, NV12, P16, TENSOR_NHWC, TENSOR_NHWC_CASES, label
from gpu_util import DevPlanes, stream_handle
from test_gpu_tensor_out import ELEM, MATRICES, PARAMS, TensorBuf, assert_bits, picture, reference_bits
from test_tensor_in_cpu import denorm_scale_bias_f32, special_values_f32
from test_tensor_out_cpu import scale_bias_f32

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = 0xCD
TDT = {0: torch.float32, 1: torch.float16, 2: torch.bfloat16}

# (name, sw, sh, dw, dh, frames, VPF_TUNE_NV12_RGB_VARIANT, source offset in samples, (family, band height or strip passes), 16-bit instantiation too)
FAMILY_CASES = TENSOR_NHWC_CASES
CASE = {c[0]: c for c in FAMILY_CASES}

ROI_W, ROI_H, ROI_D = 192, 64, 16
# odd offsets, one pixel, the whole frame (a 12x down-scale: the per-tap job class), an identity crop, edges
ROI_RECTS = [(17, 9, 55, 41), (0, 0, 1, 1), (0, 0, ROI_W, ROI_H), (33, 5, 16, 16), (ROI_W - 21, ROI_H - 11, 21, 11), (1, 3, 100, 50), (2, 2, 30, 30),
             (191, 63, 1, 1), (5, 0, 187, 64)]
WARP_W, WARP_H, WARP_D = 96, 64, 16
_C, _S = math.cos(math.radians(30)), math.sin(math.radians(30))
# identity, 30 degrees, a flip, a 6x down-scale (the whole frame: per-tap class when its strip does not fit), one footprint wholly outside
WARP_MATS = [(1, 0, 20, 0, 1, 7), (_C, -_S, 30, _S, _C, 5), (-1, 0, 60, 0, 1, 2), (6, 0, 0, 0, 4, 0), (1, 0, 500, 0, 1, 0), (1, 0, 88.5, 0, 1, 56.5)]
WARP_BORDER = (10, 128, 250)


@pytest.fixture(scope="module")
def orc(oracle):
    oracle.set_threads(16)
    return oracle


class NhwcBuf:
    """n frames of ONE interleaved plane [dh, dw, 3] each in a canary-filled byte buffer: frame i at lead + i frame, rows `row` bytes apart"""

    def __init__(self, n, dw, dh, elem, row=0, frame=0, lead=256, tail=256):
        self.n, self.dw, self.dh, self.elem = n, dw, dh, elem
        self.row = row or 3 * dw * elem
        self.frame = frame or dh * self.row
        self.lead = lead
        size = lead + (n - 1) * self.frame + (dh - 1) * self.row + 3 * dw * elem + tail
        self.buf = torch.full((size,), CANARY, dtype=torch.uint8, device="cuda")

    def planes(self, i):
        return [(self.buf.data_ptr() + self.lead + i * self.frame, self.row), (0, 0), (0, 0)]

    def frames(self):
        """-> ([n, dh, dw, 3] bit patterns, canaries intact)"""
        h = self.buf.cpu().numpy()
        mask = np.zeros(h.shape, bool)
        out = np.empty((self.n, self.dh, self.dw, 3), np.uint32 if self.elem == 4 else np.uint16)
        rb = 3 * self.dw * self.elem
        for i in range(self.n):
            off = self.lead + i * self.frame
            view = np.lib.stride_tricks.as_strided(h[off:], shape=(self.dh, rb), strides=(self.row, 1))
            out[i] = np.ascontiguousarray(view).view(out.dtype).reshape(self.dh, self.dw, 3)
            np.lib.stride_tricks.as_strided(mask[off:], shape=(self.dh, rb), strides=(self.row, 1))[:] = True
        return out, bool((h[~mask] == CANARY).all())


def hwc(bits):
    """planar reference bits [3, H, W] -> [H, W, 3]"""
    return np.ascontiguousarray(np.transpose(bits, (1, 2, 0)))


def source(orc, sf, cs, cr, sw, sh, dw, dh, seed, off):
    """(device planes, [3, dh, dw] reference bytes) of one frame; P10: the 16-bit tests' planted frames and their definition"""
    if sf == "P10":
        return DevPlanes(p16.p16_frame(orc, sf, sw, sh, seed), offset=2 * off), p16.whole_u8(orc, sf, cs, cr, sw, sh, dw, dh, seed)
    src, want = picture(orc, sf, cs, cr, sw, sh, dw, dh, seed)
    return DevPlanes(src, offset=off), want


def run_whole(capi, sf, cs, cr, sw, sh, dw, dh, devs, dtype, bgr, params, buf, batch=True, nhwc=True):
    norm = capi.make_tensor_norm(*PARAMS[params], dtype=dtype, bgr=bgr, nhwc=nhwc)
    ex = capi.make_exec(stream_handle())
    if batch:
        capi.convert_resize_tensor_batch(ex, getattr(capi, sf), cs, cr, sw, sh, dw, dh, capi.make_batch([(d.desc(), buf.planes(i)) for i, d in enumerate(devs)]), norm)
    else:
        assert len(devs) == 1
        capi.convert_resize_tensor(ex, getattr(capi, sf), cs, cr, sw, sh, devs[0].desc(), dw, dh, buf.planes(0), norm)
    torch.cuda.synchronize()


def _child(code):
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, VPF_HIP_LOG="2"), timeout=300)
    assert r.returncode == 0 and "done" in r.stdout, r.stdout + r.stderr
    logs = {}
    for chunk in r.stderr.split("CASE ")[1:]:
        name, rest = chunk.split("\n", 1)
        logs[name.strip()] = [l for l in rest.split("\n") if "libvpfhip: launch" in l]
    return logs


def test_every_family_is_selected():
    """the kernel-selection log (VPF_HIP_LOG=2, child process) carries, for a channels-last destination, exactly the label of the instantiation each
    case of FAMILY_CASES takes — the family and band height of the planar planes, with the FC_TENSOR_NHWC class, from NV12 and from P10
    (tests/cases_fused_families.py); the ROI and warp calls of this file run their staged AND their gather
    kernels; the way back takes the fast kernel at the aligned shapes and the quad kernel otherwise"""
    code = f"""
import sys
sys.path.insert(0, {ROOT!r})
import torch
from videoprocessingframework_amd import capi
ex = capi.make_exec(torch.cuda.current_stream().cuda_stream)
norm = capi.make_tensor_norm((0, 0, 0), (1, 1, 1), nhwc=True)
def frame(sw, sh, off, e):
    p = (sw * e + 255) // 256 * 256
    y = torch.zeros(sh * p * 2 + 4096, dtype=torch.uint8, device="cuda")
    return y, [(y.data_ptr() + off * e, p), (y.data_ptr() + off * e + p * sh, p)]
keep = []
for name, sw, sh, dw, dh, n, variant, off, p10 in {[c[:8] + (c[9],) for c in FAMILY_CASES]!r}:
    for fmt, e in ((capi.NV12, 1),) + (((capi.P10, 2),) if p10 else ()):
        y, src = frame(sw, sh, off, e)
        out = torch.empty(n * 3 * dh * dw, dtype=torch.float32, device="cuda")
        dst = [[(out.data_ptr() + 12 * dw * dh * i, 12 * dw), (0, 0), (0, 0)] for i in range(n)]
        prev = capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, variant)
        print("CASE", name + ("_p10" if e == 2 else ""), file=sys.stderr, flush=True)
        capi.convert_resize_tensor_batch(ex, fmt, 1, 0, sw, sh, dw, dh, capi.make_batch([(src, d) for d in dst]), norm)
        torch.cuda.synchronize()
        capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, prev)
W, H, D = {(ROI_W, ROI_H, ROI_D)!r}
y, src = frame(W, H, 0, 1)
rects = {ROI_RECTS!r}
out = torch.empty(97 * 3 * D * D, dtype=torch.float32, device="cuda")
print("CASE rois", file=sys.stderr, flush=True)
capi.convert_resize_tensor_rois(ex, capi.NV12, 1, 0, W, H, D, D, capi.make_rois([(src, [(out.data_ptr() + 12 * D * D * i, 12 * D), (0, 0), (0, 0)], rects[i % len(rects)]) for i in range(97)]), norm)
torch.cuda.synchronize()
W, H, D = {(WARP_W, WARP_H, WARP_D)!r}
y, src = frame(W, H, 0, 1)
mats = {WARP_MATS!r}
for name, variant in (("warps", 0), ("warps9", 9)):
    prev = capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, variant)
    print("CASE", name, file=sys.stderr, flush=True)
    capi.convert_warp_tensor(ex, capi.NV12, 1, 0, W, H, D, D, capi.make_warps([(src, [(out.data_ptr() + 12 * D * D * i, 12 * D), (0, 0), (0, 0)], mats[i % len(mats)]) for i in range(97)]), norm, capi.make_warp_opts(0, (1, 2, 3)))
    torch.cuda.synchronize()
    capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, prev)
for name, w, h, dtype, nv12, soff in {ENCODE_LOG_CASES!r}:
    e = 4 if dtype == 0 else 2
    s = torch.zeros(3 * h * w * e + 64, dtype=torch.uint8, device="cuda")
    d = torch.zeros(2 * (h + 1) * (w + 1) + 64, dtype=torch.uint8, device="cuda")
    cw, ch = (w + 1) // 2, (h + 1) // 2
    dp = [(d.data_ptr(), w), (d.data_ptr() + w * h, 2 * cw)] if nv12 else [(d.data_ptr(), w), (d.data_ptr() + w * h, cw), (d.data_ptr() + w * h + cw * ch, cw)]
    print("CASE", name, file=sys.stderr, flush=True)
    capi.tensor_convert(ex, capi.NV12 if nv12 else capi.YUV420, 0, 1, w, h, [(s.data_ptr() + soff * e, 3 * w * e), (0, 0), (0, 0)], dp,
                        capi.make_tensor_denorm((0, 0, 0), (1, 1, 1), dtype=dtype, nhwc=True))
    torch.cuda.synchronize()
print("done")
"""
    logs = _child(code)
    seen = set()
    for name, _, _, _, _, n, _, _, (family, r), p10 in FAMILY_CASES:
        for key, src in ((name, NV12),) + (((name + "_p10", P16),) if p10 else ()):
            lines, want = logs[key], label(family, r, src, TENSOR_NHWC, n)
            print(key, lines)
            assert lines and all(l.split("launch ", 1)[1].strip() == want for l in lines), (key, want, lines)
        seen.add(family)
    assert seen == set(FAMILIES), seen
    # 97 jobs = two job tables; each table of the ROI call holds staged and per-tap jobs (the whole frame is a 12 x 4 down-scale)
    print(logs["rois"], logs["warps"], logs["warps9"])
    # the log carries the kernels' template-ids as the code object has them: <source class, destination class>, FC_NV12 = 0, FC_TENSOR_NHWC = 8
    assert any("k_roi_strip<0, 8>" in l for l in logs["rois"]) and any("k_roi_gather<0, 8>" in l for l in logs["rois"]), logs["rois"]
    assert all(", 8>)" in l for l in logs["rois"] + logs["warps"] + logs["warps9"])
    assert any("k_warp_strip<0, 8>" in l for l in logs["warps"]), logs["warps"]
    assert logs["warps9"] and all("k_warp_gather<0, 8>" in l for l in logs["warps9"]), logs["warps9"]
    for name, w, h, dtype, nv12, soff in ENCODE_LOG_CASES:
        fast = soff == 0 and w % 16 == 0 and h % 2 == 0
        exact = (f"k_tensor_yuv_r<{dtype}, {'true' if nv12 else 'false'}, true>" if fast  # <dtype (VPF_TENSOR_F32 = 0, F16 = 1, BF16 = 2), NV12, NHWC>
                 else f"k_tensor_yuv_quad<{'true' if nv12 else 'false'}, true>")
        assert len(logs[name]) == 1 and exact in logs[name][0], (name, exact, logs[name])


# the way back: (name, w, h, dtype, NV12, source offset in elements).  528 x 4 f32 and 1040 x 4 f16 / bf16: one full chunk of the fast kernel
# (64 lanes x 8 / 16 pixels) plus a partial one; 13 x 7 and a source one element off: the quad kernel
ENCODE_CASES = [("fast_f32", 528, 4, 0, 0), ("fast_f16", 1040, 4, 1, 0), ("fast_bf16", 1040, 4, 2, 0), ("quad_13x7", 13, 7, 0, 0), ("quad_13x7_f16", 13, 7, 1, 0),
                ("quad_off", 528, 4, 2, 1)]
ENCODE_LOG_CASES = [(f"enc_{name}_{int(nv12)}", w, h, dtype, nv12, soff) for name, w, h, dtype, soff in ENCODE_CASES for nv12 in (True, False)]


@pytest.mark.parametrize("case", FAMILY_CASES, ids=[c[0] for c in FAMILY_CASES])
def test_families_sources_matrices_dtypes(capi, orc, case):
    """each family x NV12 / YUV420 (and P10 where the family has a 16-bit instantiation) x the four (colour space, range) pairs x f32 / f16 / bf16;
    RGB / BGR and the three parameter sets rotate through: bit-identical to the transposed planar reference, canaries intact"""
    name, sw, sh, dw, dh, n, variant, off, _, p10 = case
    prev = capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, variant)
    try:
        for sf in ("NV12", "YUV420") + (("P10",) if p10 else ()):
            for k, (cs, cr) in enumerate(MATRICES):
                seeds = [9600 + k, 9700 + k] if n > 1 else [9600 + k]
                made = [source(orc, sf, cs, cr, sw, sh, dw, dh, s, off) for s in seeds]
                devs = [made[i % len(made)][0] for i in range(n)]
                for dtype in (0, 1, 2):
                    bgr = (k + dtype) % 2 == 1
                    params = ("imagenet", "unit", "symmetric")[(k + dtype) % 3]
                    buf = NhwcBuf(n, dw, dh, ELEM[dtype])
                    run_whole(capi, sf, cs, cr, sw, sh, dw, dh, devs, dtype, bgr, params, buf, batch=n > 1 or k % 2 == 0)
                    got, intact = buf.frames()
                    what = f"{name} {sf} cs{cs} cr{cr} dtype{dtype} bgr{bgr} {params}"
                    assert intact, what
                    refs = [hwc(reference_bits(m[1], *PARAMS[params], dtype, bgr)) for m in made]
                    for i in range(n):
                        assert_bits(got[i], refs[i % len(refs)], f"{what} frame {i}")
    finally:
        capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, prev)


@pytest.mark.parametrize("name", ["strip_r2_down", "gather"])
def test_alignment_layouts(capi, orc, name):
    """two frames into: a contiguous [2, H, W, 3] tensor; rows padded by 16 B + 1 element (the vector path is off: element stores); rows padded
    by 64 B; the base pointer one element off; gaps between the frames — every dtype, both channel orders"""
    _, sw, sh, dw, dh, _, variant, off, _, _ = CASE[name]
    n, cs, cr = 2, 1, 0
    made = [source(orc, "NV12", cs, cr, sw, sh, dw, dh, 9800 + j, off) for j in range(n)]
    for dtype in (0, 1, 2):
        e = ELEM[dtype]
        rb = 3 * dw * e
        layouts = {"contiguous": dict(lead=0, tail=256),
                   "padded_16B_plus_1": dict(row=rb + 16 + e, lead=256),
                   "padded_64B": dict(row=rb + 64, lead=512),
                   "base_plus_1_element": dict(lead=256 + e),
                   "frame_gaps": dict(frame=dh * rb + 16 * 7, lead=256)}
        for lname, geo in layouts.items():
            for bgr in (False, True):
                buf = NhwcBuf(n, dw, dh, e, **geo)
                run_whole(capi, "NV12", cs, cr, sw, sh, dw, dh, [m[0] for m in made], dtype, bgr, "imagenet", buf)
                got, intact = buf.frames()
                what = f"{name} dtype{dtype} {lname} bgr{bgr}"
                assert intact, what
                for i in range(n):
                    assert_bits(got[i], hwc(reference_bits(made[i][1], *PARAMS["imagenet"], dtype, bgr)), f"{what} frame {i}")


@pytest.mark.parametrize("n", [1, 33, 129])
def test_batch_sizes(capi, orc, n):
    """n across the 32- and 128-frame tables (129: a second dispatch) at 64 x 32 -> 16 x 8, every frame with a source of its own"""
    sw, sh, dw, dh, cs, cr = 64, 32, 16, 8, 1, 1
    made = [source(orc, "NV12", cs, cr, sw, sh, dw, dh, 9900 + j, 0) for j in range(n)]
    for dtype, bgr in ((0, False), (1, True), (2, False)):
        buf = NhwcBuf(n, dw, dh, ELEM[dtype])
        run_whole(capi, "NV12", cs, cr, sw, sh, dw, dh, [m[0] for m in made], dtype, bgr, "imagenet", buf, batch=n > 1)
        got, intact = buf.frames()
        assert intact, (n, dtype)
        for i in range(n):
            assert_bits(got[i], hwc(reference_bits(made[i][1], *PARAMS["imagenet"], dtype, bgr)), f"n{n} dtype{dtype} frame {i}")


@pytest.mark.parametrize("sf", ["NV12", "YUV420"])
def test_rois(capi, orc, sf):
    """97 jobs (two job tables) on two 192 x 64 frames into 16 x 16: odd offsets, one pixel, the whole frame (12x down: the per-tap class), an
    identity crop; staged and gather dispatches both run (test_every_family_is_selected reads the log of the same call)"""
    W, H, D = ROI_W, ROI_H, ROI_D
    devs = [roi.frame(orc, sf, W, H, seed)[1] for seed in range(2)]
    jobs = [(i % 2, ROI_RECTS[i % len(ROI_RECTS)]) for i in range(97)]
    for k, (cs, cr) in enumerate(MATRICES[:2]):
        for dtype in (0, 1, 2):
            bgr = (k + dtype) % 2 == 1
            params = ("imagenet", "unit", "symmetric")[(k + dtype) % 3]
            buf = NhwcBuf(len(jobs), D, D, ELEM[dtype], row=3 * D * ELEM[dtype] + (16 if dtype == 1 else 0))
            norm = capi.make_tensor_norm(*PARAMS[params], dtype=dtype, bgr=bgr, nhwc=True)
            rois = capi.make_rois([(devs[s].desc(), buf.planes(i), r) for i, (s, r) in enumerate(jobs)])
            capi.convert_resize_tensor_rois(capi.make_exec(stream_handle()), getattr(capi, sf), cs, cr, W, H, D, D, rois, norm)
            torch.cuda.synchronize()
            got, intact = buf.frames()
            assert intact, (sf, cs, cr, dtype)
            for i, (s, r) in enumerate(jobs):
                assert_bits(got[i], hwc(reference_bits(roi.ref_u8(orc, sf, cs, cr, W, H, r, D, D, seed=s), *PARAMS[params], dtype, bgr)),
                            f"{sf} cs{cs} cr{cr} dtype{dtype} bgr{bgr} job {i} rect {r}")


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("sf", ["NV12", "YUV420"])
def test_warps(capi, orc, sf, mode):
    """97 jobs on 96 x 64 frames into 16 x 16: identity, 30 degrees, a flip, a 6x down-scale, a footprint wholly outside, one half outside.
    CONSTANT with border (10, 128, 250) under R G B and B G R — the border lands in the slot of its output channel — and REPLICATE; the default
    policy (staged) and the forced per-tap form"""
    W, H, D, cs, cr = WARP_W, WARP_H, WARP_D, 1, 0
    devs = [warp.frame(orc, sf, W, H, seed)[1] for seed in range(2)]
    jobs = [(i % 2, WARP_MATS[i % len(WARP_MATS)]) for i in range(97)]
    for variant in (0, 9):
        prev = capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, variant)
        try:
            for dtype in ((0, 1, 2) if variant == 0 else (0,)):
                for bgr in (False, True):
                    buf = NhwcBuf(len(jobs), D, D, ELEM[dtype])
                    norm = capi.make_tensor_norm(*PARAMS["imagenet"], dtype=dtype, bgr=bgr, nhwc=True)
                    table = capi.make_warps([(devs[s].desc(), buf.planes(i), m) for i, (s, m) in enumerate(jobs)])
                    capi.convert_warp_tensor(capi.make_exec(stream_handle()), getattr(capi, sf), cs, cr, W, H, D, D, table, norm, capi.make_warp_opts(mode, WARP_BORDER))
                    torch.cuda.synchronize()
                    got, intact = buf.frames()
                    assert intact, (sf, mode, variant, dtype, bgr)
                    for i, (s, m) in enumerate(jobs):
                        want = warp.want_bits(orc, sf, cs, cr, W, H, m, D, D, WARP_BORDER, mode, "imagenet", dtype, bgr, seed=s)
                        assert_bits(got[i], hwc(want), f"{sf} mode{mode} variant{variant} dtype{dtype} bgr{bgr} job {i}")
                    if mode == 0 and dtype == 0:  # the job wholly outside is the border, per output channel slot, through the epilogue
                        scale, bias = scale_bias_f32(*PARAMS["imagenet"])
                        b = (np.array(WARP_BORDER, np.float64) * scale.astype(np.float64) + bias.astype(np.float64)).astype(np.float32)
                        assert (got[4] == b.view(np.uint32)[None, None, :]).all(), (sf, variant, bgr)
        finally:
            capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, prev)


def test_same_build_two_layouts(capi, orc):
    """an additional check: for one case per entry, the channels-last output viewed as [N, H, W, 3] and permuted equals the planar output of the
    same library (torch.equal on integer views)"""
    for name in ("half", "strip_r2_up"):
        _, sw, sh, dw, dh, _, variant, off, _, _ = CASE[name]
        dev = source(orc, "NV12", 1, 0, sw, sh, dw, dh, 9600, off)[0]
        for dtype, bgr in ((0, True), (1, False)):
            a, b = NhwcBuf(1, dw, dh, ELEM[dtype]), TensorBuf(1, dw, dh, ELEM[dtype])
            run_whole(capi, "NV12", 1, 0, sw, sh, dw, dh, [dev], dtype, bgr, "imagenet", a, batch=False)
            run_whole(capi, "NV12", 1, 0, sw, sh, dw, dh, [dev], dtype, bgr, "imagenet", b, batch=True, nhwc=False)
            ga, gb = torch.from_numpy(a.frames()[0].astype(np.int64)), torch.from_numpy(b.frames()[0].astype(np.int64))
            assert torch.equal(ga.permute(0, 3, 1, 2), gb), (name, dtype)
    W, H, D = ROI_W, ROI_H, ROI_D
    dev = roi.frame(orc, "NV12", W, H, 0)[1]
    a, b = NhwcBuf(len(ROI_RECTS), D, D, 2), TensorBuf(len(ROI_RECTS), D, D, 2)
    for buf, flag in ((a, True), (b, False)):
        norm = capi.make_tensor_norm(*PARAMS["unit"], dtype=2, bgr=True, nhwc=flag)
        capi.convert_resize_tensor_rois(capi.make_exec(stream_handle()), capi.NV12, 1, 0, W, H, D, D,
                                        capi.make_rois([(dev.desc(), buf.planes(i), r) for i, r in enumerate(ROI_RECTS)]), norm)
    torch.cuda.synchronize()
    assert torch.equal(torch.from_numpy(a.frames()[0].astype(np.int64)).permute(0, 3, 1, 2), torch.from_numpy(b.frames()[0].astype(np.int64)))
    W, H, D = WARP_W, WARP_H, WARP_D
    dev = warp.frame(orc, "NV12", W, H, 0)[1]
    a, b = NhwcBuf(len(WARP_MATS), D, D, 4), TensorBuf(len(WARP_MATS), D, D, 4)
    for buf, flag in ((a, True), (b, False)):
        norm = capi.make_tensor_norm(*PARAMS["imagenet"], dtype=0, bgr=True, nhwc=flag)
        capi.convert_warp_tensor(capi.make_exec(stream_handle()), capi.NV12, 1, 0, W, H, D, D,
                                 capi.make_warps([(dev.desc(), buf.planes(i), m) for i, m in enumerate(WARP_MATS)]), norm, capi.make_warp_opts(0, WARP_BORDER))
    torch.cuda.synchronize()
    assert torch.equal(torch.from_numpy(a.frames()[0].astype(np.int64)).permute(0, 3, 1, 2), torch.from_numpy(b.frames()[0].astype(np.int64)))


class NhwcSrc:
    """n frames [3, h, w] of float elements, each as ONE interleaved plane [h, w, 3] in a device byte buffer: frame i at lead + i frame"""

    def __init__(self, frames, row=0, frame=0, lead=0):
        n, (_, h, w), e = len(frames), frames[0].shape, frames[0].element_size()
        self.row = row or 3 * w * e
        self.frame = frame or h * self.row
        self.lead = lead
        host = np.full((lead + n * self.frame + 64,), 0xA5, dtype=np.uint8)
        for i, f in enumerate(frames):
            raw = f.permute(1, 2, 0).contiguous().view(torch.uint8).numpy().reshape(h, 3 * w * e)
            np.lib.stride_tricks.as_strided(host[lead + i * self.frame:], shape=(h, 3 * w * e), strides=(self.row, 1))[:] = raw
        self.buf = torch.from_numpy(host).cuda()

    def planes(self, i):
        return [(self.buf.data_ptr() + self.lead + i * self.frame, self.row), (0, 0), (0, 0)]


def planted_input(w, h, seed, params, dtype):
    """tests/test_gpu_tensor_in.py's input with NaN, +-inf, values below 0 and above 255 (after de-normalisation) and ties planted over the
    first elements of every channel -> (torch CPU tensor [3, h, w] of the dtype, widened exactly to float32 numpy)"""
    t, _ = tin.tensor_input(w, h, seed, params, dtype)
    t = t.clone()
    sp = torch.from_numpy(special_values_f32())
    k = min(sp.numel(), h * w)
    for c in range(3):
        t[c].view(-1)[:k] = sp.roll(7 * c)[:k].to(TDT[dtype])
    return t, t.to(torch.float32).numpy()


@pytest.mark.parametrize("case", ENCODE_CASES, ids=[c[0] for c in ENCODE_CASES])
def test_encode(capi, orc, case):
    """vpf_tensor_convert(_batch) from one interleaved plane: the fast kernel (one full chunk plus a partial one) and the quad kernel (odd sizes;
    the source base one element off), NV12 and YUV420, MPEG and JPEG range, R G B and B G R, special values planted: the oracle's planes, and
    byte for byte what the planar call writes for the de-interleaved copy"""
    name, w, h, dtype, soff = case
    e = ELEM[dtype]
    n = 2
    for k, (dst_fmt, cr, bgr) in enumerate([("NV12", 1, False), ("YUV420", 0, True), ("NV12", 0, True), ("YUV420", 1, False)]):
        params = ("imagenet", "unit")[k % 2]
        scale, bias = denorm_scale_bias_f32(*tin.PARAMS[params])
        ins = [planted_input(w, h, 4200 + i, params, dtype) for i in range(n)]
        src = NhwcSrc([t for t, _ in ins], lead=soff * e)
        dn = capi.make_tensor_denorm(dtype=dtype, bgr=bgr, scale=[float(s) for s in scale], bias=[float(b) for b in bias], nhwc=True)
        ex = capi.make_exec(stream_handle())
        dsts = [tin.dst_planes(orc, dst_fmt, w, h) for _ in range(n)]
        if k % 2 == 0:
            capi.tensor_convert_batch(ex, getattr(capi, dst_fmt), 0, cr, w, h, capi.make_batch([(src.planes(i), d.desc()) for i, d in enumerate(dsts)]), dn)
        else:
            for i, d in enumerate(dsts):
                capi.tensor_convert(ex, getattr(capi, dst_fmt), 0, cr, w, h, src.planes(i), d.desc(), dn)
        planar = tin.TensorSrc([t for t, _ in ins])
        pd = [tin.dst_planes(orc, dst_fmt, w, h) for _ in range(n)]
        tin.run_capi(capi, dst_fmt, cr, w, h, planar, pd, dtype, bgr, scale, bias)
        torch.cuda.synchronize()
        for i in range(n):
            what = f"{name} {dst_fmt} cr{cr} bgr{bgr} {params} frame {i}"
            got = tin.check(dsts[i], tin.reference(orc, ins[i][1], scale, bias, bgr, cr, dst_fmt), what)
            for a, b in zip(got, pd[i].download()[0]):
                assert np.array_equal(a, b), what + ": differs from the planar call"


def _nvc():
    sys.path.insert(0, os.path.join(ROOT, "videoprocessingframework_amd"))
    import PyNvCodec as nvc
    from videoprocessingframework_amd import PytorchNvCodec as pnc

    return nvc, pnc


def _upload(nvc, planes, w, h):
    up = nvc.PyFrameUploader(w, h, nvc.PixelFormat.NV12, 0)
    return up.UploadSingleFrame(np.concatenate([p.reshape(-1) for p in planes])).Clone(0)


def test_python_decode(orc):
    """to_normalized_tensor / rois_to_normalized_tensor / warps_to_normalized_tensor with channels_last=True: a tensor of logical shape
    [N, 3, H, W] in torch.channels_last memory, torch.equal to the planar call's; out= as a slice of a channels-last batch with its neighbours
    untouched; a planar `out` is refused"""
    nvc, pnc = _nvc()
    PF = nvc.PixelFormat
    sw, sh, dw, dh, n = 192, 48, 128, 32, 3
    mean, std = PARAMS["imagenet"]
    cc = nvc.ColorspaceConversionContext(nvc.ColorSpace.BT_709, nvc.ColorRange.MPEG)
    pics = [picture(orc, "NV12", 1, 0, sw, sh, dw, dh, 9600 + i) for i in range(n)]
    surfs = [_upload(nvc, p[0], sw, sh) for p in pics]
    torch.cuda.synchronize()
    rs = nvc.PySurfaceConvertResizer(sw, sh, PF.NV12, dw, dh, PF.RGB_PLANAR, 0)
    for tdt, bits in ((torch.float32, torch.int32), (torch.float16, torch.int16), (torch.bfloat16, torch.int16)):
        for bgr in (False, True):
            planar = pnc.to_normalized_tensor(rs, surfs, mean, std, dtype=tdt, bgr=bgr, cc_ctx=cc)
            cl = pnc.to_normalized_tensor(rs, surfs, mean, std, dtype=tdt, bgr=bgr, cc_ctx=cc, channels_last=True)
            assert tuple(cl.shape) == (n, 3, dh, dw) and cl.is_contiguous(memory_format=torch.channels_last) and not cl.is_contiguous()
            assert torch.equal(cl.view(bits), planar.view(bits)), (tdt, bgr)
            canary = 0x3C3C3C3C if bits == torch.int32 else 0x3C3C
            big = torch.full((n + 4, dh, dw, 3), canary, dtype=bits, device="cuda").permute(0, 3, 1, 2)  # a channels-last batch
            res = pnc.to_normalized_tensor(rs, surfs, mean, std, dtype=tdt, bgr=bgr, out=big.view(tdt)[2:2 + n], cc_ctx=cc, channels_last=True)
            assert res.data_ptr() == big[2:2 + n].data_ptr()
            assert bool((big[:2] == canary).all()) and bool((big[2 + n:] == canary).all()), (tdt, bgr)
            assert torch.equal(big[2:2 + n], planar.view(bits)), (tdt, bgr)
    got = pnc.to_normalized_tensor(rs, surfs, mean, std, cc_ctx=cc, channels_last=True).cpu().numpy().view(np.uint32)
    for i in range(n):
        assert_bits(got[i], reference_bits(pics[i][1], mean, std, 0, False), f"to_normalized_tensor(channels_last) frame {i}")
    with pytest.raises(ValueError, match="channels_last"):
        pnc.to_normalized_tensor(rs, surfs, mean, std, out=torch.empty((n, 3, dh, dw), device="cuda"), cc_ctx=cc, channels_last=True)
    with pytest.raises(ValueError):  # and a channels-last `out` without the keyword is refused as before: nothing is inferred
        pnc.to_normalized_tensor(rs, surfs, mean, std, out=torch.empty((n, 3, dh, dw), device="cuda", memory_format=torch.channels_last), cc_ctx=cc)
    # regions and warps of the same surfaces
    rois = [(i % n, x, y, w, h) for i, (x, y, w, h) in enumerate([(17, 9, 55, 31), (0, 0, 1, 1), (0, 0, sw, sh), (33, 5, 128, 32), (1, 3, 100, 40)])]
    mats = torch.tensor([[[1, 0, 20, 0, 1, 7]], [[_C, -_S, 30, _S, _C, 5]], [[-1, 0, 60, 0, 1, 2]], [[1, 0, 500, 0, 1, 0]]], dtype=torch.float32).view(-1, 2, 3)
    idx = [i % n for i in range(len(mats))]
    for tdt, bits in ((torch.float32, torch.int32), (torch.bfloat16, torch.int16)):
        planar = pnc.rois_to_normalized_tensor(rs, surfs, rois, mean, std, dtype=tdt, bgr=True, cc_ctx=cc)
        cl = pnc.rois_to_normalized_tensor(rs, surfs, rois, mean, std, dtype=tdt, bgr=True, cc_ctx=cc, channels_last=True)
        assert cl.is_contiguous(memory_format=torch.channels_last) and torch.equal(cl.view(bits), planar.view(bits)), tdt
        canary = 0x3C3C3C3C if bits == torch.int32 else 0x3C3C
        big = torch.full((len(rois) + 4, dh, dw, 3), canary, dtype=bits, device="cuda").permute(0, 3, 1, 2)
        pnc.rois_to_normalized_tensor(rs, surfs, rois, mean, std, dtype=tdt, bgr=True, out=big.view(tdt)[2:2 + len(rois)], cc_ctx=cc, channels_last=True)
        assert bool((big[:2] == canary).all()) and bool((big[2 + len(rois):] == canary).all()) and torch.equal(big[2:2 + len(rois)], planar.view(bits)), tdt
        planar = pnc.warps_to_normalized_tensor(rs, surfs, idx, mats, mean, std, dtype=tdt, border=WARP_BORDER, cc_ctx=cc)
        cl = pnc.warps_to_normalized_tensor(rs, surfs, idx, mats, mean, std, dtype=tdt, border=WARP_BORDER, cc_ctx=cc, channels_last=True)
        assert cl.is_contiguous(memory_format=torch.channels_last) and torch.equal(cl.view(bits), planar.view(bits)), tdt
        big = torch.full((len(mats) + 4, dh, dw, 3), canary, dtype=bits, device="cuda").permute(0, 3, 1, 2)
        pnc.warps_to_normalized_tensor(rs, surfs, idx, mats, mean, std, dtype=tdt, border=WARP_BORDER, out=big.view(tdt)[2:2 + len(mats)], cc_ctx=cc, channels_last=True)
        assert bool((big[:2] == canary).all()) and bool((big[2 + len(mats):] == canary).all()) and torch.equal(big[2:2 + len(mats)], planar.view(bits)), tdt
    with pytest.raises(ValueError, match="channels_last"):
        pnc.rois_to_normalized_tensor(rs, surfs, rois, mean, std, out=torch.empty((len(rois), 3, dh, dw), device="cuda"), cc_ctx=cc, channels_last=True)
    with pytest.raises(ValueError, match="channels_last"):
        pnc.warps_to_normalized_tensor(rs, surfs, idx, mats, mean, std, out=torch.empty((len(mats), 3, dh, dw), device="cuda"), cc_ctx=cc, channels_last=True)


def test_python_encode(orc):
    """from_normalized_tensor(channels_last=True) on a channels-last model output gives surfaces byte-equal to those of its .contiguous() planar
    copy; a planar tensor passed with channels_last=True raises, and so does a channels-last one without it (as before)"""
    nvc, pnc = _nvc()
    PF = nvc.PixelFormat
    w, h, n = 528, 4, 3
    mean, std = tin.PARAMS["imagenet"]
    for fmt, name in ((PF.NV12, "NV12"), (PF.YUV420, "YUV420")):
        conv = nvc.PyTensorToSurface(w, h, fmt, 0)
        for dtype in (0, 1):
            x = torch.stack([planted_input(w, h, 4300 + i, "imagenet", dtype)[0] for i in range(n)]).cuda()
            cl = x.contiguous(memory_format=torch.channels_last)
            assert not cl.is_contiguous()
            for bgr in (False, True):
                a = pnc.from_normalized_tensor(conv, cl, mean, std, bgr=bgr, channels_last=True)
                b = pnc.from_normalized_tensor(conv, cl.contiguous(), mean, std, bgr=bgr)
                torch.cuda.synchronize()
                for i in range(n):
                    for pa, pb in zip(tin.surface_planes(pnc, orc, a[i], name, w, h), tin.surface_planes(pnc, orc, b[i], name, w, h)):
                        assert torch.equal(pa, pb), (name, dtype, bgr, i)
            big = torch.zeros((n + 2, h, w, 3), dtype=TDT[dtype], device="cuda").permute(0, 3, 1, 2)
            big[1:1 + n] = x
            a = pnc.from_normalized_tensor(conv, big[1:1 + n], mean, std, channels_last=True)   # a slice of a channels-last batch
            b = pnc.from_normalized_tensor(conv, x, mean, std)
            torch.cuda.synchronize()
            for i in range(n):
                for pa, pb in zip(tin.surface_planes(pnc, orc, a[i], name, w, h), tin.surface_planes(pnc, orc, b[i], name, w, h)):
                    assert torch.equal(pa, pb), (name, dtype, i)
            with pytest.raises(ValueError, match="channels_last"):
                pnc.from_normalized_tensor(conv, x, mean, std, channels_last=True)
            with pytest.raises(ValueError):
                pnc.from_normalized_tensor(conv, cl, mean, std)
