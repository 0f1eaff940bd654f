"""Seeded differential fuzz of the fused tensor entries on the MI355X: vpf_convert_resize_tensor(_batch), vpf_convert_resize_tensor_rois(_dev),
vpf_convert_letterbox_tensor(_aa), vpf_convert_warp_tensor(_dev), vpf_convert_persp_tensor, vpf_convert_remap_tensor and
vpf_tensor_convert(_batch).

The calls come from tests/cases_tensor_fuzz.py (one description per call, reproducible from the seed and the case index; tests/
test_tensor_fuzz_cases_cpu.py checks the generator, that the library accepts every call, that both kernel forms of every entry are reached and
that the ground truth is tied to the oracle's EXACT mode).  What the hand-picked tests of these entries pin and this one draws PER JOB: the frame,
the geometry, and the layout of the destination planes — the jobs of a call sit in ONE canary-filled buffer at differing row pitches and base
alignments (JobsBuf: TensorBuf / NhwcBuf parts laid over one allocation), so that one dispatch holds jobs of both store paths, a job table
holds both kernel forms, and the staged dispatch's LDS is the largest of unlike needs.

Ground truth, as in the entries' own tests: the CPU oracle composed as the definition says (roi_reference_u8, letterbox_reference_u8,
warp_reference_u8, persp_reference_u8, remap_reference_u8, aa_ref of tests/c/aa_ref_capi.cpp with the pad around it, oracle.convert_resize; 16-bit sources narrowed by oracle.convert(P10 | P12 -> NV12) first), then reference_bits; the way back:
quantise_numpy, then oracle.convert(RGB_PLANAR -> YUV420 -> NV12).  Every written element must be bit-identical (assert_bits: no tolerance), every
other byte of the buffer must still be the canary, jobs behind a device count must not be written, invalid device entries take the zero / border
fill, and a device-table call must equal the host-table call on the same jobs.  The perspective entry runs every call twice more on the same
uploads: in its other kernel form (the tuning knob at the other of 0 and 9: the two buffers byte-identical) and, for the jobs whose last row is
(0, 0, 1), through vpf_convert_warp_tensor at the same planes (the header promises the affine entry's bits).  The antialiased letterbox runs
every call in its other form too; the remap does both: the other form, and its jobs on unsprinkled affine maps through vpf_convert_warp_tensor.
The remap's maps live in allocations of their own whose every byte that is no coordinate is 0xFF (NaNs: a read outside a map shows in the output).

Seeds: VPF_FUZZ_FIRST / VPF_FUZZ_SEEDS as in tests/test_gpu_parity.py (64 by default; VPF_FUZZ_SEEDS=500 is the soak, profiles/).
Wall time of the default 64 seeds per function on one MI355X (the sum of pytest --durations over its 64 tests, references on 16 CPU threads
included; the whole module: 448 passed in 8.6 s; the 500-seed soak: 3500 passed in 47.6 s, profiles/r15_tensor_fuzz_soak.txt):
  whole_frame_tensor 0.9 s   rois 1.1 s   rois_dev 0.7 s   letterbox 1.1 s   warp 1.5 s   warp_dev 0.7 s   encode 0.6 s
With the perspective family (its three calls per case included): persp 1.8 s, the whole module: 512 passed in 10.1 s; the 500-seed soak of
test_fuzz_persp alone: 500 passed in 19.6 s (profiles/r19_persp_fuzz_soak.txt).
With the antialiased letterbox and the remap (two and two or three calls per case), one run of the whole module: persp 1.7 s, letterbox_aa 2.7 s
(1.6 x persp: the reference's cost per picture pixel grows with the square of the factor), remap 2.3 s (1.3 x), 640 passed in 15.0 s; the
500-seed soaks: letterbox_aa 500 passed in 23.7 s, remap 500 passed in 22.0 s (profiles/letterbox_aa_fuzz_soak.txt, profiles/remap_fuzz_soak.txt).
Neither new function has failed on any seed."""
import os

import numpy as np
import pytest
import torch

import cases_tensor_fuzz as cases
import test_gpu_tensor_in as tin
import test_gpu_tensor_nhwc as nhwc_tests
from gpu_util import DevPlanes, stream_handle
from test_gpu_remap_tensor import DevMaps
from test_gpu_tensor_nhwc import NhwcBuf, hwc
from test_gpu_tensor_out import CANARY, ELEM, PARAMS, TensorBuf, assert_bits, reference_bits
from test_gpu_warps_dev import POISON
from test_tensor_fuzz_cases_cpu import (dev_dst, dst_planes, eight_bit, encode_src_planes, forget_p16, host_frames, host_jobs, invoke, invoke_encode,
                                        invoke_host, job_u8, rgb_frames, rgb_order, source_pitches)
from test_tensor_in_cpu import denorm_scale_bias_f32, special_values_f32

pytestmark = pytest.mark.gpu
_FUZZ_SEEDS = range(int(os.environ.get("VPF_FUZZ_FIRST", "0")), int(os.environ.get("VPF_FUZZ_FIRST", "0")) + int(os.environ.get("VPF_FUZZ_SEEDS", "64")))
P16 = ("P10", "P12")


@pytest.fixture(scope="module")
def orc(oracle):
    oracle.set_threads(16)
    return oracle


class JobsBuf:
    """the jobs of one host-table call in ONE canary-filled buffer, each at the layout the description gives it: a TensorBuf / NhwcBuf of one frame
    per job, whose bytes are a window of the one allocation (their geometry, plane pointers, decoding and canary check are used as they are)"""

    def __init__(self, call):
        self.call = call
        self.buf = torch.full((call["size"],), CANARY, dtype=torch.uint8, device="cuda")
        self.parts = []
        for job in call["jobs"]:
            g = job["layout"]
            geo = dict(row=g["row"], lead=g["lead"], tail=g["tail"], **({} if call["nhwc"] else dict(plane=g["plane"])))
            part = (NhwcBuf if call["nhwc"] else TensorBuf)(1, call["dw"], call["dh"], ELEM[call["dtype"]], **geo)
            assert part.buf.numel() == g["size"]
            part.buf = self.buf[g["off"]:g["off"] + g["size"]]
            assert part.planes(0) == dst_planes(call, job, self.buf.data_ptr())   # the description's offsets ARE the part's planes
            self.parts.append(part)

    def frames(self):
        """-> ([bit patterns of job i: [3, dh, dw], or [dh, dw, 3] channels-last], canaries intact)"""
        host = self.buf.cpu()
        got, intact = [], True
        for part, job in zip(self.parts, self.call["jobs"]):
            g, dev = job["layout"], part.buf
            part.buf = host[g["off"]:g["off"] + g["size"]]
            bits, ok = part.frames()
            part.buf = dev
            got.append(bits[0])
            intact &= ok
        return got, intact


def dev_buf(call):
    """the one destination of a device-table call: max_n jobs a job stride apart"""
    geo = {k: v for k, v in call["geo"].items() if k != "kind"}
    buf = (NhwcBuf if call["nhwc"] else TensorBuf)(call["max_n"], call["dw"], call["dh"], ELEM[call["dtype"]], **geo)
    assert (buf.planes(0), buf.frame) == dev_dst(call, buf.buf.data_ptr())
    return buf


def upload_frames(orc, call):
    srcs = host_frames(orc, call)
    devs = [DevPlanes(s, align=f["align"], extra=f["extra"]) for s, f in zip(srcs, call["frames"])]
    for k, d in enumerate(devs):
        assert d.pitches == source_pitches(call, k)
    return srcs, devs


def tuned(capi, call, fn):
    prev = capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, call["tune"])
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, prev)


def want_of(call, u8):
    bits = reference_bits(u8, *PARAMS[call["params"]], call["dtype"], call["bgr"])
    return hwc(bits) if call["nhwc"] else bits


def host_table_family(capi, orc, family, seed, also=None, prepare=None):
    """whole, rois, letterbox, warp, persp, letterbox_aa, remap: one call per case into a JobsBuf, every job against its reference;
    also(call, descs, buf, got, what): further checks of a family on the same uploads; prepare(call): the device addresses invoke() takes as `tables`"""
    for k, call in enumerate(cases.cases(family, seed)):
        what = f"{family} seed {seed} case {k}"
        srcs, devs = upload_frames(orc, call)
        buf = JobsBuf(call)
        descs = [d.desc() for d in devs]
        tables = prepare(call) if prepare is not None else None
        tuned(capi, call, lambda: invoke(capi, call, capi.make_exec(stream_handle()), descs, buf.buf.data_ptr(), tables))
        got, intact = buf.frames()
        if family == "whole":
            refs = []
            for fmt, planes in eight_bit(orc, call, srcs, orc.FP32):
                st, pic = orc.convert_resize(fmt, orc.RGB_PLANAR, call["cs"], call["cr"], call["W"], call["H"], planes, call["dw"], call["dh"], mode=orc.FP32)
                assert st == 0
                refs.append(want_of(call, np.stack(pic)))
        else:
            rgb = rgb_frames(orc, call, srcs)
        for i, job in enumerate(call["jobs"]):
            want = refs[job["frame"]] if family == "whole" else want_of(call, job_u8(orc, call, job, rgb[job["frame"]]))
            assert_bits(got[i], want, f"{what} job {i} {job}: {cases.describe(call)}")
        assert intact, f"{what}: bytes outside the jobs' elements were written: {cases.describe(call)}"
        if also is not None:
            also(call, descs, buf, got, what)
    forget_p16()


def device_table_family(capi, orc, family, seed):
    """rois_dev, warp_dev: the device entry against the references (written, invalid and unwritten jobs) and against the host-table entry"""
    for k, call in enumerate(cases.cases(family, seed)):
        what = f"{family} seed {seed} case {k}"
        srcs, devs = upload_frames(orc, call)
        descs = [d.desc() for d in devs]
        n, i32 = call["max_n"], torch.int32
        count = torch.tensor([call["count"]], dtype=i32).cuda() if call["count"] is not None else None
        if family == "rois_dev":
            boxes = torch.full((n, call["box_ints"]), 0x5A5A5A5A, dtype=i32)
            boxes[:, :5] = torch.tensor(call["boxes"], dtype=torch.int64).to(i32)
            keep = [boxes.cuda()]
            tables = dict(boxes=keep[0].data_ptr())
        else:
            mats = torch.full((n, call["mat_floats"]), POISON, dtype=torch.float32)
            mats[:, :6] = torch.tensor(call["mats"], dtype=torch.float64).to(torch.float32)
            index = torch.full((n, call["index_ints"]), 0x5A5A5A5A, dtype=i32)
            index[:, 0] = torch.tensor(call["index"], dtype=torch.int64).to(i32)
            keep = [mats.cuda(), index.cuda()]
            tables = dict(mats=keep[0].data_ptr(), index=keep[1].data_ptr())
        tables["count"] = count.data_ptr() if count is not None else None
        a, b = dev_buf(call), dev_buf(call)
        ex = capi.make_exec(stream_handle())
        tuned(capi, call, lambda: (invoke(capi, call, ex, descs, a.buf.data_ptr(), tables), invoke_host(capi, call, ex, descs, b.buf.data_ptr())))
        (got, intact), (host, host_intact) = a.frames(), b.frames()
        jobs, c = host_jobs(call)
        jobs = dict(jobs)
        rgb = rgb_frames(orc, call, srcs)
        fill = np.zeros((3, 1, 1), np.uint8) if family == "rois_dev" else np.array(rgb_order(call, call["border"]), np.uint8).reshape(3, 1, 1)
        fill = want_of(call, np.broadcast_to(fill, (3, call["dh"], call["dw"])))
        blank = np.full(got[0].shape, 0xCDCDCDCD if ELEM[call["dtype"]] == 4 else 0xCDCD, got.dtype)
        for i in range(n):
            tag = f"{what} job {i}: {cases.describe(call)}"
            if i >= c:
                assert_bits(got[i], blank, "a job behind the count was written: " + tag)
                assert_bits(host[i], blank, "host-table entry, a job that was not passed: " + tag)
            elif i in jobs:
                assert_bits(got[i], want_of(call, job_u8(orc, call, jobs[i], rgb[jobs[i]["frame"]])), tag)
                assert_bits(got[i], host[i], "device entry != host-table entry: " + tag)
            else:
                assert_bits(got[i], fill, "the fill of an invalid entry: " + tag)
        assert intact and host_intact, f"{what}: bytes outside the jobs' elements were written: {cases.describe(call)}"
    forget_p16()


@pytest.mark.parametrize("seed", _FUZZ_SEEDS)  # soak: VPF_FUZZ_SEEDS=500 (VPF_FUZZ_FIRST=n: seeds n .. n + VPF_FUZZ_SEEDS - 1, fresh cases)
def test_fuzz_whole_frame_tensor(capi, orc, seed):
    """vpf_convert_resize_tensor(_batch): source format x matrix x size pair (exact 2 x and 3 x among them) x dtype x channel order x layout x 1 .. 40
    frames, every frame's planes at a layout of its own"""
    host_table_family(capi, orc, "whole", seed)


@pytest.mark.parametrize("seed", _FUZZ_SEEDS)
def test_fuzz_rois(capi, orc, seed):
    """vpf_convert_resize_tensor_rois: staged and per-tap jobs, one or two job tables, per-job frame, rectangle and layout"""
    host_table_family(capi, orc, "rois", seed)


@pytest.mark.parametrize("seed", _FUZZ_SEEDS)
def test_fuzz_rois_dev(capi, orc, seed):
    """vpf_convert_resize_tensor_rois_dev: padded box tables, a count below / at / above max_n, invalid boxes (zero fill), a drawn job stride"""
    device_table_family(capi, orc, "rois_dev", seed)


@pytest.mark.parametrize("seed", _FUZZ_SEEDS)
def test_fuzz_letterbox(capi, orc, seed):
    """vpf_convert_letterbox_tensor: per-job rectangle, placement (vpf_letterbox_fit's answer, one pixel, odd ix) and layout; the padded area holds the
    pad's bits (it is part of every job's reference)"""
    host_table_family(capi, orc, "letterbox", seed)


@pytest.mark.parametrize("seed", _FUZZ_SEEDS)
def test_fuzz_warp(capi, orc, seed):
    """vpf_convert_warp_tensor: translations, right angles, rotations at scales 0.3 .. 9, shear, zero rows, footprints wholly outside, both border modes"""
    host_table_family(capi, orc, "warp", seed)


@pytest.mark.parametrize("seed", _FUZZ_SEEDS)
def test_fuzz_warp_dev(capi, orc, seed):
    """vpf_convert_warp_tensor_dev: padded matrix tables with NaNs in the padding, a strided frame index, a count, invalid entries (the border in both
    modes), max_step 0 or a true bound"""
    device_table_family(capi, orc, "warp_dev", seed)


def persp_other_form_and_affine_entry(capi):
    def also(call, descs, buf, got, what):
        other = JobsBuf(call)
        tuned(capi, dict(call, tune=9 - call["tune"]), lambda: invoke(capi, call, capi.make_exec(stream_handle()), descs, other.buf.data_ptr()))
        assert torch.equal(buf.buf, other.buf), f"{what}: the two kernel forms (tuning knob 0 and 9) differ: {cases.describe(call)}"
        lifted = [i for i, j in enumerate(call["jobs"]) if tuple(j["m"][6:]) == (0.0, 0.0, 1.0)]
        if not lifted:
            return
        affine = dict(call, entry="warp", jobs=[dict(call["jobs"][i], m=call["jobs"][i]["m"][:6]) for i in lifted])
        third = JobsBuf(affine)   # the same layout: every job at its own planes, the other jobs' parts stay canary
        tuned(capi, affine, lambda: invoke(capi, affine, capi.make_exec(stream_handle()), descs, third.buf.data_ptr()))
        frames, intact = third.frames()
        for i, f in zip(lifted, frames):
            assert_bits(got[i], f, f"{what} job {i}: last row (0, 0, 1), vpf_convert_warp_tensor gives other bits: {cases.describe(call)}")
        assert intact, f"{what}: vpf_convert_warp_tensor on the lifted jobs wrote outside their elements: {cases.describe(call)}"
    return also


@pytest.mark.parametrize("seed", _FUZZ_SEEDS)
def test_fuzz_persp(capi, orc, seed):
    """vpf_convert_persp_tensor: lifted affine, moderate and steep homographies, the horizon inside the destination (w exactly 0 on pixels), behind the
    plane, denormal and tiny w (coordinates of +-inf and above 1e29), footprints wholly outside, cancelling coefficients up to 2^24 and the sawtooth
    that takes the per-pixel fallback; both border modes; both kernel forms byte-identical; lifted jobs equal to the affine entry"""
    host_table_family(capi, orc, "persp", seed, persp_other_form_and_affine_entry(capi))


def other_form(capi):
    """the same call on the same uploads with the tuning knob at the other of 0 and 9: the two buffers byte-identical, canaries included"""
    def also(call, descs, buf, got, what):
        other = JobsBuf(call)
        tuned(capi, dict(call, tune=9 - call["tune"]), lambda: invoke(capi, call, capi.make_exec(stream_handle()), descs, other.buf.data_ptr()))
        assert torch.equal(buf.buf, other.buf), f"{what}: the two kernel forms (tuning knob 0 and 9) differ: {cases.describe(call)}"
    return also


@pytest.mark.parametrize("seed", _FUZZ_SEEDS)
def test_fuzz_letterbox_aa(capi, orc, seed):
    """vpf_convert_letterbox_tensor_aa: calls of mild jobs (0.4 .. 3 x, the 64 x 16 tile), calls with a 3.6 .. 6.5 x job (the 32 x 8 tile) and
    unrestricted calls (thumbnails of large rectangles per tap next to staged jobs), one or two job tables, per-job frame, rectangle, placement and
    layout, the pad around every picture; both kernel forms byte-identical"""
    host_table_family(capi, orc, "letterbox_aa", seed, other_form(capi))


def remap_checks(capi):
    """-> (prepare, also) of the remap family.  prepare uploads every map pair of the call once (DevMaps of tests/test_gpu_remap_tensor.py: each map
    in an allocation of its own at the pair's pitch and lead, everything that is no coordinate holding NaN bytes, so that a read outside a map shows
    in the output).  also runs the call in its other kernel form (the tuning knob at the other of 0 and 9, no LDS against the hint's: byte-identical
    buffers) and the jobs whose maps are an affine matrix's coordinates, unsprinkled, through vpf_convert_warp_tensor at the same planes (the header
    promises its bits; it promises nothing of the kind for the perspective entry, so homography jobs are not held against it)"""
    live = {}

    def prepare(call):
        live["maps"] = [DevMaps(*cases.pair_maps(call, p), xpitch=p["xpitch"], ypitch=p["ypitch"], xlead=p["xlead"], ylead=p["ylead"]) for p in call["maps"]]
        for m, p in zip(live["maps"], call["maps"]):
            assert (m.x()[0] % 16, m.y()[0] % 16) == (p["xlead"] % 16, p["ylead"] % 16)
        live["tables"] = dict(maps=[(m.x()[0], m.y()[0]) for m in live["maps"]])
        return live["tables"]

    def also(call, descs, buf, got, what):
        other = JobsBuf(call)
        tuned(capi, dict(call, tune=9 - call["tune"]), lambda: invoke(capi, call, capi.make_exec(stream_handle()), descs, other.buf.data_ptr(), live["tables"]))
        assert torch.equal(buf.buf, other.buf), f"{what}: the two kernel forms (tuning knob 0 and 9) differ: {cases.describe(call)}"
        plain = [i for i, j in enumerate(call["jobs"]) if call["maps"][j["maps"]]["kind"] == "affine" and call["maps"][j["maps"]]["sprinkle"] is None]
        if not plain:
            return
        affine = dict(call, entry="warp", jobs=[dict(call["jobs"][i], m=call["maps"][call["jobs"][i]["maps"]]["m"]) for i in plain])
        third = JobsBuf(affine)   # the same layout: every job at its own planes, the other jobs' parts stay canary
        tuned(capi, affine, lambda: invoke(capi, affine, capi.make_exec(stream_handle()), descs, third.buf.data_ptr()))
        frames, intact = third.frames()
        for i, f in zip(plain, frames):
            assert_bits(got[i], f, f"{what} job {i}: maps of an affine matrix, vpf_convert_warp_tensor gives other bits: {cases.describe(call)}")
        assert intact, f"{what}: vpf_convert_warp_tensor on the affine jobs wrote outside their elements: {cases.describe(call)}"
    return prepare, also


@pytest.mark.parametrize("seed", _FUZZ_SEEDS)
def test_fuzz_remap(capi, orc, seed):
    """vpf_convert_remap_tensor: affine, homography (NaN behind the plane), barrel, jittered, random, outside, all-NaN and one-pixel maps, any of them
    sprinkled with the special coordinates; shared pairs, map pitches and bases at 0 / 4 / 8 / 12 mod 16; both border modes; every hint; frames wider
    than 2048; the two named strips at the edge of what a launch gives; both kernel forms byte-identical; affine maps equal to the affine entry"""
    prepare, also = remap_checks(capi)
    host_table_family(capi, orc, "remap", seed, also, prepare)


def encode_inputs(call):
    """n x (torch CPU tensor [3, h, w] of the dtype, the same widened exactly to float32 numpy)"""
    w, h, dtype = call["w"], call["h"], call["dtype"]
    if call["input"] == "planted":
        return [nhwc_tests.planted_input(w, h, call["seed"] % (1 << 20) + i, call["params"], dtype) for i in range(call["n"])]
    sp = special_values_f32()
    out = []
    for i in range(call["n"]):
        t = torch.from_numpy(np.resize(np.roll(sp, call["seed"] % sp.size + 11 * i), 3 * h * w).reshape(3, h, w)).to(tin.TDT[dtype])
        out.append((t, t.to(torch.float32).numpy()))
    return out


@pytest.mark.parametrize("seed", _FUZZ_SEEDS)
def test_fuzz_encode(capi, orc, seed):
    """vpf_tensor_convert(_batch): w x h (odd sizes, the fast kernel's shapes), NV12 / YUV420, dtype, channel order, planar and channels-last sources at
    drawn pitches and bases, destinations at every alignment; NaN, infinities, ties and both clamps in the input"""
    for k, call in enumerate(cases.cases("encode", seed)):
        what = f"encode seed {seed} case {k}"
        ins = encode_inputs(call)
        s = call["src"]
        if call["nhwc"]:
            src = nhwc_tests.NhwcSrc([t for t, _ in ins], row=s["row"], frame=s["frame"], lead=s["lead"])
        else:
            src = tin.TensorSrc([t for t, _ in ins], row=s["row"], plane=s["plane"], frame=s["frame"], lead=s["lead"])
        for i in range(call["n"]):
            assert src.planes(i) == encode_src_planes(call, i, src.buf.data_ptr())
        dsts = [tin.dst_planes(orc, call["dst_fmt"], call["w"], call["h"], **call["dst"]) for _ in range(call["n"])]
        tuned(capi, call, lambda: invoke_encode(capi, call, capi.make_exec(stream_handle()), src.buf.data_ptr(), [d.desc() for d in dsts]))
        scale, bias = denorm_scale_bias_f32(*tin.PARAMS[call["params"]])
        for i in range(call["n"]):
            tin.check(dsts[i], tin.reference(orc, ins[i][1], scale, bias, call["bgr"], call["cr"], call["dst_fmt"]), f"{what} frame {i}: {cases.describe(call)}")
