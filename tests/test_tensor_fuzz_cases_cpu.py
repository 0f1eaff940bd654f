"""The generator of the fused-tensor fuzz (tests/cases_tensor_fuzz.py) and its ground truth, without a GPU.

  - the same seed gives the same description; every rectangle lies inside its frame or destination, every matrix coefficient of a valid job is
    at most 2^24 in magnitude, every destination layout satisfies the alignment rules of include/vpf_hip.h;
  - every generated call passes the library's validation: the real entry is called with fake plane pointers on a device no machine has and
    must answer VPF_ERR_NO_DEVICE (invoke() below is the one place that turns a description into the C call: the GPU test runs the same code);
  - reach: over the default seeds each kernel form holds at least 10 % of the jobs of every entry that has two forms, decided by the kernels' own
    policy functions behind tests/c/*_capi.cpp (csrc/vpf_job_bounds.h compiled with g++), counted over calls with the tuning knob at 0 only — the
    knob's 9 forces the per-tap form and would make the condition empty; and every source format, dtype, channel order, layout, border mode, a
    two-table call, a call whose jobs differ in alignment and a unit clamped at the right edge occur per entry; the perspective entry's tile
    classes, its per-pixel fallback and its dispatches without LDS or without staged jobs besides (persp_reach);
  - the antialiased letterbox (test_reach_letterbox_aa, decided by aa_plan of csrc/vpf_aa_plan.h per job table): staged under the 64 x 16 tile,
    staged under the 32 x 8 tile and per tap each hold at least 10 % of the jobs; a table with a staged and a per-tap dispatch; a call whose two
    tables take unlike tile shapes or forms; a rectangle at the right edge of a frame with W % 8 != 0, an odd ix, s < 1 on one axis with s > 3 on
    the other, a tile window that is the whole rectangle.  Measured over the default seeds: 4 329 jobs, 2 622 / 1 157 / 550;
  - the remap (test_reach_remap, test_remap_named_strips, decided by the kernel's window functions behind tests/c/remap_bounds_capi.cpp and
    remap_plan, with launch_convert_remap's 32 bytes behind the strip restated): border, staged and per-tap tiles each hold at least 10 % of the
    tiles; shared map pairs, map bases at 0 / 4 / 8 / 12 mod 16, a tile with one in-range pixel, windows beyond columns 255 and 2 047, every hint,
    and the two named strips of 65 504 bytes (stages) and 65 520 bytes (per tap).  Measured: 9 924 tiles, 1 678 / 4 100 / 4 146;
  - the independent link: the composed FP32 ground truth of the GPU test (roi_reference_u8, letterbox_reference_u8, warp_reference_u8,
    persp_reference_u8, remap_reference_u8) against the same composition with every oracle call in EXACT mode, at most 2 codes apart
    (test_composed_fp32_reference_is_near_the_exact_chain)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cases_tensor_fuzz as cases
from test_letterbox_tensor_cpu import letterbox_reference_u8
from test_persp_tensor_cpu import persp_maps, persp_reference_u8
from test_remap_tensor_cpu import clamp_maps, remap_reference_u8
from test_roi_tensor_cpu import roi_reference_u8
from test_tensor_in_cpu import PARAM_SETS as DENORM_SETS
from test_tensor_in_cpu import denorm_scale_bias_f32
from test_tensor_out_cpu import PARAM_SETS
from test_warp_tensor_cpu import warp_maps, warp_reference_u8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "videoprocessingframework_amd", "libvpfhip.so")
PARAMS = {name: (mean, std) for name, mean, std in PARAM_SETS}
DENORM = {name: (mean, std) for name, mean, std in DENORM_SETS}
SEEDS = range(64)        # the default seed set of the GPU test
SOAK = range(500)        # the soak's seeds (VPF_FUZZ_SEEDS=500): validity and acceptance are checked for these too
NO_GPU = 1 << 20         # a device index no machine has: a call that passes validation stops at the device switch
FAKE_DST, FAKE_SRC, FAKE_TABLE = 0x40000000, 0x10000000, 0x70000000
HOST_TABLE = ("rois", "letterbox", "warp", "persp", "letterbox_aa", "remap")
EXACT_CHAIN = ("rois", "letterbox", "warp", "persp", "remap")   # the families whose ground truth the oracle has an EXACT mode for
P16 = ("P10", "P12")


def round_up(v, a):
    return (v + a - 1) // a * a


# ------------------------------------------------------------------------------------------------ description -> C call (shared with the GPU test)
def source_pitches(call, k):
    """the pitches DevPlanes gives frame k's planes"""
    f = call["frames"][k]
    e = 2 if call["sf"] in P16 else 1
    W, cw = call["W"], (call["W"] + 1) // 2
    rows = [W * e, 2 * cw * e] if call["sf"] != "YUV420" else [W, cw, cw]
    return [round_up(rb, f["align"]) + f["extra"] for rb in rows]


def dst_planes(call, job, base):
    p = [(base + off, pitch) for off, pitch in cases.plane_offsets(call, job)]
    return p + [(0, 0), (0, 0)] if call["nhwc"] else p


def dev_dst(call, base):
    """(planes of job 0, job stride) of a device-table call"""
    g = call["geo"]
    if call["nhwc"]:
        return [(base + g["lead"], g["row"]), (0, 0), (0, 0)], g["frame"]
    return [(base + g["lead"] + c * g["plane"], g["row"]) for c in range(3)], g["frame"]


def invoke(capi, call, ex, srcs, base, tables=None, check=True):
    """run the decode-side call a description names: srcs = the plane descriptors of its frames, base = the address of its destination buffer,
    tables = the device addresses of a device-table call (boxes / mats, index, count), or of a remap call's map pairs (maps: [(xmap, ymap)])"""
    entry, jobs = call["entry"], call.get("jobs")
    norm = capi.make_tensor_norm(*PARAMS[call["params"]], dtype=call["dtype"], bgr=call["bgr"], nhwc=call["nhwc"])
    head = (ex, getattr(capi, call["sf"]), call["cs"], call["cr"], call["W"], call["H"])
    dw, dh = call["dw"], call["dh"]
    if entry == "whole":
        if call["batch"]:
            return capi.convert_resize_tensor_batch(*head, dw, dh, capi.make_batch([(srcs[j["frame"]], dst_planes(call, j, base)) for j in jobs]), norm, check=check)
        return capi.convert_resize_tensor(*head, srcs[jobs[0]["frame"]], dw, dh, dst_planes(call, jobs[0], base), norm, check=check)
    if entry == "rois":
        return capi.convert_resize_tensor_rois(*head, dw, dh, capi.make_rois([(srcs[j["frame"]], dst_planes(call, j, base), j["rect"]) for j in jobs]), norm, check=check)
    if entry == "letterbox":
        arr = capi.make_letterbox_jobs([(srcs[j["frame"]], dst_planes(call, j, base), j["rect"], j["dst_rect"]) for j in jobs])
        return capi.convert_letterbox_tensor(*head, dw, dh, arr, norm, capi.make_letterbox_opts(call["pad"]), check=check)
    if entry == "letterbox_aa":
        arr = capi.make_letterbox_jobs([(srcs[j["frame"]], dst_planes(call, j, base), j["rect"], j["dst_rect"]) for j in jobs])
        return capi.convert_letterbox_tensor_aa(*head, dw, dh, arr, norm, capi.make_letterbox_opts(call["pad"]), check=check)
    if entry == "warp":
        arr = capi.make_warps([(srcs[j["frame"]], dst_planes(call, j, base), j["m"]) for j in jobs])
        return capi.convert_warp_tensor(*head, dw, dh, arr, norm, capi.make_warp_opts(call["mode"], call["border"]), check=check)
    if entry == "remap":
        def maps(j):
            p, (xa, ya) = call["maps"][j["maps"]], tables["maps"][j["maps"]]
            return (xa, p["xpitch"]), (ya, p["ypitch"])
        arr = capi.make_remap_jobs([(srcs[j["frame"]], dst_planes(call, j, base), *maps(j)) for j in jobs])
        return capi.convert_remap_tensor(*head, dw, dh, arr, norm, capi.make_remap_opts(call["mode"], call["border"], call["max_step"]), check=check)
    if entry == "persp":
        arr = capi.make_persps([(srcs[j["frame"]], dst_planes(call, j, base), j["m"]) for j in jobs])
        return capi.convert_persp_tensor(*head, dw, dh, arr, norm, capi.make_warp_opts(call["mode"], call["border"]), check=check)
    planes0, stride = dev_dst(call, base)
    if entry == "rois_dev":
        table = capi.make_rois_dev(tables["boxes"], call["max_n"], planes0, stride, tables["count"], 4 * call["box_ints"])
        return capi.convert_resize_tensor_rois_dev(*head, dw, dh, capi.make_frame_srcs(srcs), table, norm, check=check)
    assert entry == "warp_dev"
    table = capi.make_warps_dev(tables["mats"], call["max_n"], planes0, stride, tables["index"], tables["count"], 4 * call["mat_floats"], 4 * call["index_ints"],
                                call["max_step"])
    return capi.convert_warp_tensor_dev(*head, dw, dh, capi.make_frame_srcs(srcs), table, norm, capi.make_warp_opts(call["mode"], call["border"]), check=check)


def host_jobs(call):
    """the host-table call on the jobs a device-table call defines as written and valid, into a buffer of the same layout: [(job index k, job)]"""
    c = call["max_n"] if call["count"] is None else min(max(call["count"], 0), call["max_n"])
    if call["entry"] == "rois_dev":
        return [(k, dict(frame=b[0], rect=tuple(b[1:]))) for k, b in enumerate(call["boxes"][:c]) if call["valid"][k]], c
    return [(k, dict(frame=f, m=m)) for k, (f, m) in enumerate(zip(call["index"][:c], call["mats"][:c])) if call["valid"][k]], c


def invoke_host(capi, call, ex, srcs, base):
    """the host-table entry on host_jobs(call), job k at the device-table call's planes of job k"""
    planes0, stride = dev_dst(call, base)
    norm = capi.make_tensor_norm(*PARAMS[call["params"]], dtype=call["dtype"], bgr=call["bgr"], nhwc=call["nhwc"])
    head = (ex, getattr(capi, call["sf"]), call["cs"], call["cr"], call["W"], call["H"], call["dw"], call["dh"])
    jobs, _ = host_jobs(call)
    if not jobs:
        return

    def dst(k):
        return [(p + k * stride if p else 0, pitch) for p, pitch in planes0]

    if call["entry"] == "rois_dev":
        capi.convert_resize_tensor_rois(*head, capi.make_rois([(srcs[j["frame"]], dst(k), j["rect"]) for k, j in jobs]), norm)
    else:
        capi.convert_warp_tensor(*head, capi.make_warps([(srcs[j["frame"]], dst(k), j["m"]) for k, j in jobs]), norm, capi.make_warp_opts(call["mode"], call["border"]))


def encode_src_planes(call, i, base):
    s = call["src"]
    if call["nhwc"]:
        return [(base + s["lead"] + i * s["frame"], s["row"]), (0, 0), (0, 0)]
    return [(base + s["lead"] + i * s["frame"] + c * s["plane"], s["row"]) for c in range(3)]


def invoke_encode(capi, call, ex, base, dsts, check=True):
    """vpf_tensor_convert(_batch): base = the address of the source tensor buffer, dsts = the plane descriptors of the n destination pictures"""
    scale, bias = denorm_scale_bias_f32(*DENORM[call["params"]])
    dn = capi.make_tensor_denorm(dtype=call["dtype"], bgr=call["bgr"], scale=[float(s) for s in scale], bias=[float(b) for b in bias], nhwc=call["nhwc"])
    head = (ex, getattr(capi, call["dst_fmt"]), 0, call["cr"], call["w"], call["h"])
    if call["batch"]:
        return [capi.tensor_convert_batch(*head, capi.make_batch([(encode_src_planes(call, i, base), d) for i, d in enumerate(dsts)]), dn, check=check)]
    return [capi.tensor_convert(*head, encode_src_planes(call, i, base), d, dn, check=check) for i, d in enumerate(dsts)]


# ------------------------------------------------------------------------------------------------ the ground truth of a call (shared with the GPU test)
def host_frames(orc, call):
    """the host planes of the call's frames; 16-bit ones are the planted frames of tests/test_gpu_p16_tensor.py"""
    if call["sf"] in P16:
        import test_gpu_p16_tensor as p16
        return [p16.p16_frame(orc, call["sf"], call["W"], call["H"], f["seed"]) for f in call["frames"]]
    return [orc.synth(getattr(orc, call["sf"]), call["W"], call["H"], f["seed"]) for f in call["frames"]]


def forget_p16():
    """tests/test_gpu_p16_tensor.py keeps every frame it made; a fuzz never asks for the same one twice"""
    import test_gpu_p16_tensor as p16
    p16._SRC.clear()
    p16._NV12.clear()


def eight_bit(orc, call, srcs, mode):
    """(format, planes) per frame as the definition sees them: 16-bit sources narrowed by oracle.convert(P10 | P12 -> NV12) first"""
    if call["sf"] not in P16:
        return [(getattr(orc, call["sf"]), s) for s in srcs]
    if mode == orc.FP32:
        import test_gpu_p16_tensor as p16
        return [(orc.NV12, p16.nv12_of(orc, call["sf"], call["W"], call["H"], f["seed"])) for f in call["frames"]]
    out = []
    for s in srcs:
        st, nv = orc.convert(getattr(orc, call["sf"]), orc.NV12, 0, 0, call["W"], call["H"], s, mode)
        assert st == 0
        out.append((orc.NV12, nv))
    return out


def rgb_frames(orc, call, srcs, mode=None):
    """the converted WHOLE frames the ROI, letterbox and warp references crop and sample"""
    mode = orc.FP32 if mode is None else mode
    out = []
    for fmt, planes in eight_bit(orc, call, srcs, mode):
        st, rgb = orc.convert(fmt, orc.RGB_PLANAR, call["cs"], call["cr"], call["W"], call["H"], planes, mode)
        assert st == 0
        out.append(rgb)
    return out


def rgb_order(call, triple):
    """pad[c] / border[c] belong to OUTPUT channel c: in R G B order for the references"""
    return tuple(triple[::-1]) if call["bgr"] else tuple(triple)


_AA = []


def aa_lib():
    """tests/c/aa_ref_capi.cpp, compiled once per process (tests/test_letterbox_aa_cpu.py::build_aa)"""
    if not _AA:
        import tempfile

        from test_letterbox_aa_cpu import build_aa
        _AA.append(tempfile.TemporaryDirectory(prefix="fuzz_aa"))
        _AA.append(build_aa(_AA[0].name))
    return _AA[1]


def job_u8(orc, call, job, rgb):
    """[3, dh, dw] R G B bytes of one job: the composed FP32 reference the GPU tests of the entry use"""
    W, H, dw, dh = call["W"], call["H"], call["dw"], call["dh"]
    if call["entry"] == "letterbox_aa":   # as tests/test_gpu_letterbox_aa.py::ref_u8: the definition on the converted frame, the pad around it
        from test_gpu_letterbox_tensor import place
        from test_letterbox_aa_cpu import aa_ref
        return place(aa_ref(aa_lib(), rgb, job["rect"], job["dst_rect"][2], job["dst_rect"][3]), job["dst_rect"], dw, dh, rgb_order(call, call["pad"]))
    if "maps" in job:
        return remap_reference_u8(orc, None, call["cs"], call["cr"], W, H, *cases.maps_of(call, job), rgb_order(call, call["border"]), call["mode"], rgb=rgb)
    if "m" in job and len(job["m"]) == 9:
        return persp_reference_u8(orc, None, call["cs"], call["cr"], W, H, job["m"], dw, dh, rgb_order(call, call["border"]), call["mode"], rgb=rgb)
    if "m" in job:
        return warp_reference_u8(orc, None, call["cs"], call["cr"], W, H, job["m"], dw, dh, rgb_order(call, call["border"]), call["mode"], rgb=rgb)
    if "dst_rect" in job:
        return letterbox_reference_u8(orc, None, call["cs"], call["cr"], W, H, None, job["rect"], job["dst_rect"], dw, dh, rgb_order(call, call["pad"]), rgb=rgb)
    return roi_reference_u8(orc, None, call["cs"], call["cr"], W, H, None, job["rect"], dw, dh, rgb=rgb)


def job_u8_exact(orc, call, job, rgb):
    """the same composition with every oracle call in EXACT mode (rgb: the EXACT conversion), on the same float32 maps"""
    W, H, dw, dh = call["W"], call["H"], call["dw"], call["dh"]
    if "m" in job or "maps" in job:
        packed = np.ascontiguousarray(np.stack(rgb, axis=-1).reshape(H, 3 * W))
        border = rgb_order(call, call["border"])
        if "maps" in job:        # as remap_reference_u8: clamped first under REPLICATE, a NaN stays a NaN and leaves the pre-filled border
            sx, sy = clamp_maps(*cases.maps_of(call, job), W, H, call["mode"])
            front = np.ones((dh, dw), bool)
        elif len(job["m"]) == 9:   # as persp_reference_u8: pixels with !front are out of range (CONSTANT) or any pixel (REPLICATE), the border afterwards
            sx, sy, front = persp_maps(job["m"], dw, dh, W, H, call["mode"])
            fill = np.float32(-1 if call["mode"] == 0 else 0)
            sx, sy = np.ascontiguousarray(np.where(front, sx, fill)), np.ascontiguousarray(np.where(front, sy, fill))
        else:
            sx, sy = warp_maps(job["m"], dw, dh, W, H, call["mode"])
            front = np.ones((dh, dw), bool)
        dst = np.ascontiguousarray(np.broadcast_to(np.asarray(border, np.uint8), (dh, dw, 3)).reshape(dh, 3 * dw))
        st, out = orc.remap(orc.RGB, W, H, [packed], sx, sy, orc.EXACT, dst=[dst])
        assert st == 0
        out = np.array(out[0].reshape(dh, dw, 3).transpose(2, 0, 1), order="C")
        for c in range(3):
            out[c][~front] = border[c]
        return out
    x, y, w, h = job["rect"]
    ix, iy, iw, ih = job.get("dst_rect", (0, 0, dw, dh))
    out = np.empty((3, dh, dw), np.uint8)
    for c, v in enumerate(rgb_order(call, call.get("pad", (0, 0, 0)))):
        out[c] = v
    st, _ = orc.resize(orc.RGB_PLANAR, orc.LINEAR, w, h, [p[y:y + h, x:x + w] for p in rgb], iw, ih, orc.EXACT, dst=[out[c, iy:iy + ih, ix:ix + iw] for c in range(3)])
    assert st == 0
    return out


# ------------------------------------------------------------------------------------------------ determinism and validity
@pytest.mark.parametrize("family", cases.FAMILIES)
def test_same_seed_same_description(family):
    for seed in (0, 7, 63, 499):
        a, b = cases.cases(family, seed), cases.cases(family, seed)
        assert [cases.describe(c) for c in a] == [cases.describe(c) for c in b]  # (repr: a NaN coefficient is not equal to itself)
        assert len(a) == cases.CASES_PER_SEED[family]
    assert cases.describe(cases.cases(family, 0)[0]) != cases.describe(cases.cases(family, 1)[0])


def all_cases(family, seeds=SEEDS):
    return [(seed, k, c) for seed in seeds for k, c in enumerate(cases.cases(family, seed))]


def every_job(call):
    """(frame, job) of every job that names a frame and a geometry, device tables included (valid entries only)"""
    if call["entry"] == "rois_dev":
        return [dict(frame=b[0], rect=tuple(b[1:])) for b, ok in zip(call["boxes"], call["valid"]) if ok]
    if call["entry"] == "warp_dev":
        return [dict(frame=f, m=m) for f, m, ok in zip(call["index"], call["mats"], call["valid"]) if ok]
    return call["jobs"]


@pytest.mark.parametrize("family", [f for f in cases.FAMILIES if f != "encode"])
def test_geometry_and_layouts_are_valid(family):
    for seed, k, call in all_cases(family, SOAK):
        what = f"seed {seed} case {k} {cases.describe(call)}"
        W, H, dw, dh, e = call["W"], call["H"], call["dw"], call["dh"], cases.ELEM[call["dtype"]]
        assert call["sf"] not in P16 or ((W + 1) // 2) * ((H + 1) // 2) >= 7, what   # what the planted 16-bit frames need
        assert all(f["extra"] % 2 == 0 for f in call["frames"]) or call["sf"] not in P16, what
        assert 2 <= W <= 2100 and 2 <= H <= 500 and W * H * (2 if call["sf"] in P16 else 1) * 3 // 2 < (1 << 20), what
        assert 1 <= dw <= 600 and 1 <= dh <= 300, what
        assert 2 <= len(call["frames"]) <= 3, what
        for job in every_job(call):
            assert 0 <= job["frame"] < len(call["frames"]), what
            if "rect" in job:
                x, y, w, h = job["rect"]
                assert w >= 1 and h >= 1 and x >= 0 and y >= 0 and x + w <= W and y + h <= H, what
            if "dst_rect" in job:
                ix, iy, iw, ih = job["dst_rect"]
                assert iw >= 1 and ih >= 1 and ix >= 0 and iy >= 0 and ix + iw <= dw and iy + ih <= dh, what
            if family == "letterbox_aa":   # the class a call was drawn under holds for every job of it
                fx, fy = job["rect"][2] / job["dst_rect"][2], job["rect"][3] / job["dst_rect"][3]
                top = {"mild": cases.AA_MILD, "steep": cases.AA_STEEP_HI, "any": 65536.0}[call["cls"]]
                assert fx <= top and fy <= top, what
            if "m" in job:
                assert len(job["m"]) == (9 if family == "persp" else 6) and all(abs(v) <= cases.LIMIT and float(np.float32(v)) == v for v in job["m"]), what
        if family == "remap":
            assert call["max_step"] >= 0 and np.isfinite(call["max_step"]) and float(np.float32(call["max_step"])) == call["max_step"], what
            assert {j["maps"] for j in call["jobs"]} == set(range(len(call["maps"]))), what
            for p in call["maps"]:   # include/vpf_hip.h: a map pointer and pitch are multiples of 4, the pitch at least 4 x dw
                assert p["xpitch"] % 4 == 0 and p["ypitch"] % 4 == 0 and min(p["xpitch"], p["ypitch"]) >= 4 * dw and p["xlead"] % 4 == 0 and p["ylead"] % 4 == 0, what
        if family == "letterbox_aa" and call["cls"] == "steep":
            assert any(cases.AA_STEEP_LO <= j["rect"][2] / j["dst_rect"][2] and cases.AA_STEEP_LO <= j["rect"][3] / j["dst_rect"][3] and j["dst_rect"][2] >= 32
                       and j["dst_rect"][3] >= 8 for j in call["jobs"]), what
        # include/vpf_hip.h: plane pointers and pitches are multiples of the element size, pitch >= width x element size (3 x: one interleaved plane)
        rb = (3 if call["nhwc"] else 1) * dw * e
        if "jobs" in call:
            spans = []
            for job in call["jobs"]:
                g = job["layout"]
                assert g["off"] % 256 == 0 and g["off"] + g["size"] <= call["size"], what
                for off, pitch in cases.plane_offsets(call, job):
                    assert off % e == 0 and pitch % e == 0 and pitch >= rb, what
                    assert g["off"] + 16 <= off and off + (dh - 1) * pitch + rb + 16 <= g["off"] + g["size"], what   # canaries on both sides
                    spans.append((off, off + (dh - 1) * pitch + rb))
            spans.sort()
            assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), what   # no two planes overlap
        else:
            g = call["geo"]
            assert g["lead"] % e == 0 and g["row"] % e == 0 and g["row"] >= rb and g["frame"] % e == 0, what
            assert g["frame"] >= (dh * g["row"] if call["nhwc"] else 3 * g["plane"]) and (call["nhwc"] or g["plane"] >= dh * g["row"]), what
            assert call["max_n"] == len(call["valid"]) and 1 <= call["max_n"] <= 65535, what
        if family == "warp_dev":
            assert call["max_step"] >= 0 and np.isfinite(call["max_step"]), what
            steps = [max(abs(m[0]) + abs(m[1]), abs(m[3]) + abs(m[4])) for m, ok in zip(call["mats"], call["valid"]) if ok]
            assert call["max_step"] == 0 or call["max_step"] >= max(steps), what   # 0 or a TRUE bound


def test_encode_cases_are_valid():
    for seed, k, call in all_cases("encode", SOAK):
        what = f"seed {seed} case {k} {cases.describe(call)}"
        e, s = cases.ELEM[call["dtype"]], call["src"]
        rb = (3 if call["nhwc"] else 1) * call["w"] * e
        assert 1 <= call["w"] <= 1200 and 1 <= call["h"] <= 100 and 1 <= call["n"] <= 4, what
        assert s["lead"] % e == 0 and s["row"] % e == 0 and s["row"] >= rb and s["frame"] % e == 0, what
        assert s["frame"] >= (call["h"] * s["row"] if call["nhwc"] else 3 * s["plane"]) and (call["nhwc"] or s["plane"] >= call["h"] * s["row"]), what


# ------------------------------------------------------------------------------------------------ acceptance
def _lib_or_skip():
    if not os.path.exists(LIB):
        pytest.skip("libvpfhip.so not built")
    from videoprocessingframework_amd import capi
    capi.lib()
    return capi


def fake_sources(call):
    """plane descriptors of the call's frames at fake addresses, with the pitches the GPU test's DevPlanes have"""
    return [[(FAKE_SRC + 0x1000000 * k + 0x400000 * i, p) for i, p in enumerate(source_pitches(call, k))] for k in range(len(call["frames"]))]


@pytest.mark.parametrize("family", cases.FAMILIES)
def test_every_call_passes_validation(family):
    """the real entry, fake pointers, a device that does not exist: VPF_ERR_NO_DEVICE — validation is over by then and nothing was launched"""
    capi = _lib_or_skip()
    ex = capi.make_exec(device=NO_GPU)
    for seed, k, call in all_cases(family, SOAK):
        what = f"seed {seed} case {k} {cases.describe(call)}"
        if family == "encode":
            cw, ch = (call["w"] + 1) // 2, (call["h"] + 1) // 2
            rows = [call["w"], 2 * cw] if call["dst_fmt"] == "NV12" else [call["w"], cw, cw]
            d = call["dst"]
            dsts = [[(FAKE_DST + 0x1000000 * i + 0x400000 * p + d["offset"], round_up(rb, d["align"]) + d["extra"]) for p, rb in enumerate(rows)] for i in range(call["n"])]
            sts = invoke_encode(capi, call, ex, FAKE_SRC, dsts, check=False)
        else:
            tables = dict(boxes=FAKE_TABLE, mats=FAKE_TABLE, index=FAKE_TABLE + 0x100000, count=None if call.get("count") is None else FAKE_TABLE + 0x200000)
            if family == "remap":   # fake map addresses at the alignment the description gives them (4, 8, 12 mod 16 among them)
                tables = dict(maps=[(FAKE_TABLE + 0x200000 * k + p["xlead"], FAKE_TABLE + 0x200000 * k + 0x100000 + p["ylead"]) for k, p in enumerate(call["maps"])])
            sts = [invoke(capi, call, ex, fake_sources(call), FAKE_DST, tables, check=False)]
        assert all(st == capi.ERR_NO_DEVICE for st in sts), (what, [capi.status_string(st) for st in sts])


# ------------------------------------------------------------------------------------------------ reach
@pytest.fixture(scope="module")
def bounds(tmp_path_factory):
    """the five harnesses over csrc/vpf_job_bounds.h in one library, compiled with g++ as they stand"""
    from conftest import native_test_build
    so = str(tmp_path_factory.mktemp("fuzz_bounds") / "libfuzzbounds.so")
    srcs = [os.path.join(ROOT, "tests", "c", f) for f in ("job_bounds_capi.cpp", "letterbox_bounds_capi.cpp", "rois_dev_bounds_capi.cpp", "warp_dev_bounds_capi.cpp",
                                                            "persp_bounds_capi.cpp")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-shared", "-fPIC", "-Wall", "-Werror", "-Wno-unused-function", *native_test_build()[0],
                           "-I" + os.path.join(ROOT, "videoprocessingframework_amd", "csrc"), *srcs, "-o", so, "-lm"])
    L = C.CDLL(so)
    u32, fp, dp, ip = C.c_uint32, C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int)
    L.jb_warp_strip_max.argtypes, L.jb_warp_strip_max.restype = [], u32
    L.jb_roi_strip_need.argtypes, L.jb_roi_strip_need.restype = [u32] * 5 + [dp, ip], u32
    L.jb_warp_need.argtypes, L.jb_warp_need.restype = [fp] + [u32] * 4, u32
    L.lb_strip_need.argtypes, L.lb_strip_need.restype = [u32] * 9 + [dp, ip], u32
    L.rd_lds_bytes.argtypes, L.rd_lds_bytes.restype = [u32, u32], u32
    L.rd_tiles.argtypes, L.rd_tiles.restype = [u32] * 6 + [C.POINTER(u32), dp, C.POINTER(C.c_uint8)], u32
    L.rd_box_ok.argtypes, L.rd_box_ok.restype = [C.c_int32] * 5 + [u32] * 3, C.c_int
    L.wd_lds_bytes.argtypes, L.wd_lds_bytes.restype = [C.c_float] + [u32] * 4, u32
    L.wd_largest_tile.argtypes, L.wd_largest_tile.restype = [fp, C.c_int] + [u32] * 4, u32
    L.pb_strip_max.argtypes, L.pb_strip_max.restype = [], u32
    L.pb_need.argtypes, L.pb_need.restype = [fp] + [u32] * 4, u32
    L.pb_tiles.argtypes, L.pb_tiles.restype = [fp, C.c_int] + [u32] * 4 + [C.c_void_p, u32], u32
    L.pb_px_in_window.argtypes, L.pb_px_in_window.restype = [u32] * 4 + [C.c_void_p] * 2 + [u32] * 3 + [C.c_void_p], None
    return L


def job_forms(L, call, job):
    """the forms one job of a call runs under the default policy: a subset of {"staged", "per_tap"} (a device-table job decides per tile)"""
    W, H, dw, dh = call["W"], call["H"], call["dw"], call["dh"]
    conv, staged = C.c_double(), C.c_int()
    if call["entry"] == "rois":
        x, _, w, h = job["rect"]
        L.jb_roi_strip_need(x, w, h, dw, dh, C.byref(conv), C.byref(staged))
        return {"staged" if staged.value else "per_tap"}
    if call["entry"] == "letterbox":
        (x, _, w, h), (ix, iy, iw, ih) = job["rect"], job["dst_rect"]
        L.lb_strip_need(x, w, h, ix, iy, iw, ih, dw, dh, C.byref(conv), C.byref(staged))
        return {"staged" if staged.value else "per_tap"}
    if call["entry"] == "rois_dev":
        x, _, w, h = job["rect"]
        n_tiles = ((dh + 15) // 16) * ((dw + 255) // 256) + 8
        nbytes, convs, flags = (C.c_uint32 * n_tiles)(), (C.c_double * n_tiles)(), (C.c_uint8 * n_tiles)()
        n = L.rd_tiles(x, w, h, dw, dh, L.rd_lds_bytes(dw, dh), nbytes, convs, flags)
        assert 1 <= n <= n_tiles - 8
        return {"staged" if flags[t] else "per_tap" for t in range(n)}
    if call["entry"] == "persp":
        return {"staged" if L.pb_need((C.c_float * 9)(*job["m"]), W, H, dw, dh) <= L.pb_strip_max() else "per_tap"}
    m = (C.c_float * 6)(*job["m"])
    if call["entry"] == "warp":
        return {"staged" if L.jb_warp_need(m, W, H, dw, dh) <= L.jb_warp_strip_max() else "per_tap"}
    largest, lds = L.wd_largest_tile(m, call["mode"], W, H, dw, dh), L.wd_lds_bytes(call["max_step"], W, H, dw, dh)
    return {"staged" if largest <= lds else "per_tap"}


def reaches_right_edge(call, job):
    """a conversion unit next to the frame's right edge takes clamped loads: W is no multiple of 8 and the job samples column W - 1"""
    W, H = call["W"], call["H"]
    if W % 8 == 0:
        return False
    if "rect" in job:
        return job["rect"][0] + job["rect"][2] == W
    if len(job["m"]) == 9:
        sx, sy, front = persp_maps(job["m"], call["dw"], call["dh"], W, H, call["mode"])
    else:
        (sx, sy), front = warp_maps(job["m"], call["dw"], call["dh"], W, H, call["mode"]), True
    inside = front & (sx >= 0) & (sx <= np.float32(W - 1)) & (sy >= 0) & (sy <= np.float32(H - 1))
    return bool((inside & (sx >= np.float32(W - 2))).any())


PERSP_BORDER, PERSP_TAP, PERSP_OUT, PERSP_STAGE = 0, 1, 2, 3   # kPerspTile* of csrc/vpf_job_bounds.h


def persp_tables(L, call):
    """the launcher's split restated (vpf_convert_persp_tensor's chunks, split_jobs of csrc/k_job_launch.h, launch_convert_persp): jobs in chunks of
    82; per chunk the staged jobs are those with pb_need <= pb_strip_max() and the dispatch's LDS is the largest such need
    -> [(staged jobs, LDS bytes, per-tap jobs)] under the default policy"""
    W, H, dw, dh, cap = call["W"], call["H"], call["dw"], call["dh"], L.pb_strip_max()
    out = []
    for at in range(0, len(call["jobs"]), cases.TABLE["persp"]):
        chunk = call["jobs"][at:at + cases.TABLE["persp"]]
        needs = [L.pb_need((C.c_float * 9)(*j["m"]), W, H, dw, dh) for j in chunk]
        out.append(([j for j, n in zip(chunk, needs) if n <= cap], max([n for n in needs if n <= cap], default=0), [j for j, n in zip(chunk, needs) if n > cap]))
    return out


def persp_reach(L):
    """what the perspective family must reach beyond the two dispatches: every tile class of the staged kernel, a staged tile whose strip exceeds the
    LDS of its dispatch, the per-pixel fallback on a truly staged tile, a staged dispatch without LDS, a table of per-tap jobs only, w exactly 0 and
    an infinite coordinate — decided by the kernel's own functions (tests/c/persp_bounds_capi.cpp), on the calls with the tuning knob at 0"""
    calls_with = {c: 0 for c in (PERSP_BORDER, PERSP_TAP, PERSP_OUT, PERSP_STAGE)}
    out_under_constant = over_lds = fallback_calls = fallback_px = no_lds = per_tap_only = zero_w = infinite = 0
    for seed, k, call in all_cases("persp"):
        W, H, dw, dh, mode = call["W"], call["H"], call["dw"], call["dh"], call["mode"]
        for job in call["jobs"]:
            m = np.asarray(job["m"], np.float32)
            dx, dy = np.arange(dw, dtype=np.float32)[None, :], np.arange(dh, dtype=np.float32)[:, None]
            zero_w += bool((((m[6] * dx + m[7] * dy) + m[8]) == 0).any())
            sx, sy, _ = persp_maps(job["m"], dw, dh, W, H, 0)
            infinite += bool(np.isinf(sx).any() or np.isinf(sy).any())
        if call["tune"] != 0:
            continue
        classes, over, flagged = set(), False, 0
        for staged, lds, per_tap in persp_tables(L, call):
            no_lds += bool(staged) and lds == 0
            per_tap_only += bool(per_tap) and not staged
            for job in staged:
                m = (C.c_float * 9)(*job["m"])
                tiles = np.zeros((((dw + 31) // 32) * ((dh + 31) // 32), 10), np.uint32)
                assert L.pb_tiles(m, mode, W, H, dw, dh, tiles.ctypes.data, len(tiles)) == len(tiles)
                sx, sy, front = persp_maps(job["m"], dw, dh, W, H, mode)
                inr = front & (sx >= 0) & (sx <= np.float32(W - 1)) & (sy >= 0) & (sy <= np.float32(H - 1))
                for xs, ys, xe, ye, cls, x_lo, x_hi, y_lo, y_hi, nbytes in tiles.tolist():
                    classes.add(cls)
                    if cls != PERSP_STAGE:
                        continue
                    if nbytes > lds:   # the kernel's `S.bytes > lds_bytes`: this tile samples per tap
                        over = True
                        continue
                    ii = inr[ys:ye + 1, xs:xe + 1]
                    xa = np.ascontiguousarray(sx[ys:ye + 1, xs:xe + 1][ii].astype(np.uint32))
                    ya = np.ascontiguousarray(sy[ys:ye + 1, xs:xe + 1][ii].astype(np.uint32))
                    ok = np.empty(len(xa), np.uint8)
                    L.pb_px_in_window(x_lo, x_hi, y_lo, y_hi, xa.ctypes.data, ya.ctypes.data, len(xa), W, H, ok.ctypes.data)
                    flagged += int((ok == 0).sum())
        for c in classes:
            calls_with[c] += 1
        out_under_constant += PERSP_OUT in classes and mode == 0
        over_lds += over
        fallback_calls += flagged > 0
        fallback_px += flagged
    print("persp calls whose staged dispatches hold a tile of class border / tap / out / stage", [calls_with[c] for c in (0, 1, 2, 3)], "out under CONSTANT",
          out_under_constant, "a staged tile over the dispatch's LDS", over_lds, "the per-pixel fallback on a staged tile: calls", fallback_calls, "pixels", fallback_px,
          "tables: a staged dispatch with 0 bytes of LDS", no_lds, "per-tap jobs only", per_tap_only, "jobs with w == 0 on a pixel", zero_w,
          "with an infinite coordinate", infinite)
    assert all(n >= 5 for n in calls_with.values()) and out_under_constant >= 1, (calls_with, out_under_constant)
    assert over_lds >= 3 and fallback_calls >= 3 and fallback_px >= 20, (over_lds, fallback_calls, fallback_px)
    assert no_lds >= 1 and per_tap_only >= 1 and zero_w >= 1 and infinite >= 1, (no_lds, per_tap_only, zero_w, infinite)


@pytest.mark.parametrize("family", [f for f in cases.FAMILIES if f not in ("whole", "encode", "letterbox_aa", "remap")])
def test_reach(bounds, family):
    """a condition, not a measurement: the fuzz of this entry is worth running only if it holds"""
    share = {"staged": 0, "per_tap": 0}
    seen = dict(sf=set(), dtype=set(), bgr=set(), nhwc=set(), mode=set(), tune=set())
    two_tables = mixed_alignment = right_edge = both_in_one_call = n_jobs = 0
    for seed, k, call in all_cases(family):
        for key in seen:
            if key in call:
                seen[key].add(call[key])
        jobs = every_job(call)
        right_edge += any(reaches_right_edge(call, j) for j in jobs)
        if family in HOST_TABLE:
            two_tables += len(jobs) > cases.TABLE[family]
            mixed_alignment += len({(cases.plane_offsets(call, j)[0][0] % 16, j["layout"]["row"] % 16) for j in jobs}) > 1
        if family == "rois_dev":
            assert call["valid"] == [bool(bounds.rd_box_ok(*b, len(call["frames"]), call["W"], call["H"])) for b in call["boxes"]], cases.describe(call)
        if call["tune"] != 0:
            continue
        forms = [job_forms(bounds, call, j) for j in jobs]
        n_jobs += len(forms)
        for f in share:
            share[f] += sum(f in s for s in forms)
        both_in_one_call += len(set().union(*forms)) == 2 if forms else 0
    print(family, "jobs under the default policy", n_jobs, share, "calls holding both forms", both_in_one_call, "two tables", two_tables,
          "mixed alignment", mixed_alignment, "right edge", right_edge)
    assert share["staged"] >= 0.1 * n_jobs and share["per_tap"] >= 0.1 * n_jobs, (share, n_jobs)
    assert both_in_one_call >= 1
    assert seen["sf"] == set(cases.SOURCES) and seen["dtype"] == {0, 1, 2} and seen["bgr"] == {False, True} and seen["nhwc"] == {False, True}, seen
    assert seen["tune"] == {0, 9}, seen
    assert right_edge >= 1
    if family in ("warp", "warp_dev", "persp"):
        assert seen["mode"] == {0, 1}, seen
    if family == "persp":
        persp_reach(bounds)
    if family in HOST_TABLE:
        assert two_tables >= 1 and mixed_alignment >= 1
    else:
        calls = [c for _, _, c in all_cases(family)]
        assert {c["count"] is None for c in calls} == {False, True}
        assert any(c["count"] is not None and c["count"] < c["max_n"] for c in calls) and any(c["count"] == c["max_n"] for c in calls)
        assert any(c["count"] is not None and c["count"] > c["max_n"] for c in calls) and any(not all(c["valid"]) for c in calls)


@pytest.mark.parametrize("family", ["whole", "encode"])
def test_reach_of_the_single_form_entries(family):
    calls = [c for _, _, c in all_cases(family)]
    for key, want in (("dtype", {0, 1, 2}), ("bgr", {False, True}), ("nhwc", {False, True}), ("tune", {0, 9}), ("batch", {False, True})):
        assert {c[key] for c in calls} == want, key
    if family == "whole":
        assert {c["sf"] for c in calls} == set(cases.SOURCES)
        assert any(len(c["jobs"]) > 32 for c in calls)                                                     # the large frame table
        assert any(c["W"] == 2 * c["dw"] and c["H"] == 2 * c["dh"] for c in calls) and any(c["W"] == 3 * c["dw"] for c in calls)
        assert any(c["W"] % 8 for c in calls)
        assert any(len({(cases.plane_offsets(c, j)[0][0] % 16, j["layout"]["row"] % 16) for j in c["jobs"]}) > 1 for c in calls)
    else:
        assert {c["dst_fmt"] for c in calls} == {"NV12", "YUV420"} and {c["input"] for c in calls} == {"planted", "special"}
        assert any(c["w"] % 2 and c["h"] % 2 for c in calls) and any(c["w"] % 16 == 0 and c["h"] % 2 == 0 and c["src"]["kind"] == "contiguous" for c in calls)


AA_SRC_FC = {"NV12": 0, "YUV420": 1, "P10": 7, "P12": 7}   # FmtClass of csrc/vpf_classes.h, as tests/test_letterbox_aa_cpu.py names them


def aa_tables(aa, call):
    """the launcher's cut restated: the jobs in tables of 82, each planned by aa_plan of csrc/vpf_aa_plan.h (tests/test_letterbox_aa_cpu.py::plan)
    under the default policy -> [(dispatches, which)] per table"""
    from test_letterbox_aa_cpu import plan
    out = []
    for at in range(0, len(call["jobs"]), cases.TABLE["letterbox_aa"]):
        chunk = call["jobs"][at:at + cases.TABLE["letterbox_aa"]]
        geoms = [(j["rect"][2], j["rect"][3], j["dst_rect"][2], j["dst_rect"][3]) for j in chunk]
        ok, _, ds, which = plan(aa, geoms, call["dw"], call["dh"], src_fc=AA_SRC_FC[call["sf"]], nhwc=int(call["nhwc"]), dtype=call["dtype"], variant=0)
        assert ok == 1, cases.describe(call)
        out.append((ds, [int(w) for w in which]))
    return out


def test_reach_letterbox_aa():
    """conditions, decided by aa_plan table by table as the launcher cuts the jobs, counted over the default seeds on the calls with the knob at 0:
    each of {staged under the 64 x 16 tile, staged under the 32 x 8 tile, per tap} holds at least 10 % of the jobs; a call with a staged and a per-tap
    dispatch; a call of two tables, and one whose two tables take different tile shapes or forms; every source format, dtype, channel order and
    layout; both knob values; mixed destination alignment; a rectangle at the right edge of a frame with W % 8 != 0; a picture at an odd ix; a job
    with s < 1 on one axis and s > 3 on the other; a staged job whose tile window is its whole rectangle"""
    from test_letterbox_aa_cpu import AA_GATHER, tiles
    aa = aa_lib()
    T = tiles(aa)
    share = {"tile0": 0, "tile1": 0, "per_tap": 0}
    seen = dict(sf=set(), dtype=set(), bgr=set(), nhwc=set(), tune=set(), cls=set())
    n_jobs = both = two_tables = unlike_tables = mixed_alignment = right_edge = odd_ix = cross = whole_window = 0
    for seed, k, call in all_cases("letterbox_aa"):
        for key in seen:
            seen[key].add(call[key])
        jobs = call["jobs"]
        mixed_alignment += len({(cases.plane_offsets(call, j)[0][0] % 16, j["layout"]["row"] % 16) for j in jobs}) > 1
        if call["tune"] != 0:
            continue
        two_tables += len(jobs) > cases.TABLE["letterbox_aa"]
        right_edge += call["W"] % 8 != 0 and any(j["rect"][0] + j["rect"][2] == call["W"] for j in jobs)
        odd_ix += any(j["dst_rect"][0] % 2 for j in jobs)
        cross += any(min(j["rect"][2] / j["dst_rect"][2], j["rect"][3] / j["dst_rect"][3]) < 1 and max(j["rect"][2] / j["dst_rect"][2], j["rect"][3] / j["dst_rect"][3]) > 3
                     for j in jobs)
        tables = aa_tables(aa, call)
        kinds, at = [], 0
        for ds, which in tables:
            both += len(ds) == 2
            kinds.append(tuple((d["form"], d["tile"]) for d in ds))
            for j, wh in zip(jobs[at:], which):
                d = ds[wh]
                n_jobs += 1
                if d["form"] == AA_GATHER:
                    share["per_tap"] += 1
                    continue
                share[f"tile{d['tile']}"] += 1
                tw, th, _ = T[d["tile"]]
                (_, _, w, h), (_, _, iw, ih) = j["rect"], j["dst_rect"]
                whole_window += aa.aa_c_window_bound(w, iw, tw) == w and aa.aa_c_window_bound(h, ih, th) == h
            at += len(which)
        unlike_tables += len(tables) == 2 and kinds[0] != kinds[1]
    print("letterbox_aa jobs under the default policy", n_jobs, share, "tables with a staged and a per-tap dispatch", both, "calls of two tables", two_tables,
          "of unlike tables", unlike_tables, "mixed alignment", mixed_alignment, "right edge at W % 8 != 0", right_edge, "odd ix", odd_ix,
          "s < 1 on one axis and s > 3 on the other", cross, "staged jobs whose tile window is the whole rectangle", whole_window)
    assert all(v >= 0.1 * n_jobs for v in share.values()), (share, n_jobs)
    assert both >= 1 and two_tables >= 1 and unlike_tables >= 1
    assert seen["sf"] == set(cases.SOURCES) and seen["dtype"] == {0, 1, 2} and seen["bgr"] == {False, True} and seen["nhwc"] == {False, True}, seen
    assert seen["tune"] == {0, 9} and seen["cls"] == set(cases.AA_CLASSES), seen
    assert mixed_alignment >= 1 and right_edge >= 1 and odd_ix >= 1 and cross >= 1 and whole_window >= 1


@pytest.fixture(scope="module")
def rm():
    """tests/c/remap_bounds_capi.cpp: the window a workgroup of k_remap_tile merges, warp_strip, remap_strip_fits and remap_plan, compiled with g++
    as tests/test_remap_tensor_cpu.py compiles it"""
    import tempfile

    from conftest import native_test_build
    with tempfile.TemporaryDirectory(prefix="fuzz_rm") as tmp:
        so = os.path.join(tmp, "libremapbounds.so")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-shared", "-fPIC", "-Wall", "-Werror", "-Wno-unused-function", *native_test_build()[0],
                               "-I" + os.path.join(ROOT, "videoprocessingframework_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "c", "remap_bounds_capi.cpp"), "-o", so, "-lm"])
        L = C.CDLL(so)
    u32, vp = C.c_uint32, C.c_void_p
    L.rm_tile_window.argtypes, L.rm_tile_window.restype = [vp, vp, u32, u32, u32, u32, u32, C.c_int, u32, u32, vp], None
    L.rm_strip_fits.argtypes, L.rm_strip_fits.restype = [u32] * 5, C.c_int
    L.rm_plan.argtypes, L.rm_plan.restype = [C.c_int, C.c_int, u32, u32, u32, u32, u32, C.c_float, C.c_int, vp], None
    return L


REMAP_WIN_BYTES, REMAP_LDS_MAX = 32, 64 * 1024   # kRemapWinBytes of csrc/k_convert_remap.hip, kWarpStripMax of csrc/vpf_job_bounds.h


def remap_strip_given(rm, call):
    """the launcher's arithmetic restated (launch_convert_remap): remap_plan's LDS for the hint; the workgroup's eight reduction words ride behind the
    strip — 32 bytes more are asked for where that stays within 64 KiB, and the strip gives them up where it does not -> the kernel's lds_bytes"""
    o = np.zeros(6, np.uint32)
    rm.rm_plan(AA_SRC_FC[call["sf"]], int(call["nhwc"]), call["dtype"], call["W"], call["H"], call["dw"], call["dh"], call["max_step"], call["tune"], o.ctypes.data)
    assert o[0] == 1 and o[3] == cases.TABLE["remap"], cases.describe(call)
    lds = int(o[4])
    lds_all = 0 if not lds else min(lds + REMAP_WIN_BYTES, REMAP_LDS_MAX)
    return lds_all - REMAP_WIN_BYTES if lds_all else 0


def remap_tiles(rm, call, job, strip):
    """per 32 x 32 destination tile of one job, by the kernel's own functions: (outcome, in-range pixels, window (x_lo, x_hi, y_lo, y_hi), strip bytes)
    with outcome "border" (no in-range pixel), "staged", or "per_tap" (the window's strip outgrows what the dispatch was given)"""
    sx, sy = cases.maps_of(call, job)
    W, H, dw, dh, rep = call["W"], call["H"], call["dw"], call["dh"], call["mode"]
    with np.errstate(invalid="ignore"):
        inr = ~(np.isnan(sx) | np.isnan(sy)) if rep else (sx >= 0) & (sx <= np.float32(W - 1)) & (sy >= 0) & (sy <= np.float32(H - 1))
    out = []
    for by in range((dh + 31) // 32):
        for bx in range((dw + 31) // 32):
            o = np.zeros(7, np.uint32)
            rm.rm_tile_window(sx.ctypes.data, sy.ctypes.data, dw, dw, dh, bx, by, rep, W, H, o.ctypes.data)
            n_in = int(inr[32 * by:32 * by + 32, 32 * bx:32 * bx + 32].sum())
            assert bool(o[0]) == (n_in == 0), (bx, by, cases.describe(call))
            win, nbytes = tuple(int(v) for v in o[1:5]), int(o[5]) | int(o[6]) << 32
            out.append(("border" if o[0] else "staged" if rm.rm_strip_fits(*win, strip) else "per_tap", n_in, win, nbytes))
    return out


def test_reach_remap(rm):
    """conditions, decided by the kernel's own functions (tests/c/remap_bounds_capi.cpp) and remap_plan, counted over the default seeds on the calls
    with the knob at 0: each of the three tile outcomes holds at least 10 % of the tiles; both border modes, every source format, dtype, channel
    order and layout, both knob values; a two-table call; a shared map pair; a map base at 4, 8 and 12 mod 16; a tile with exactly one in-range
    pixel; windows that reach beyond column 255 and beyond column 2047 (the upper bits of the packed 16-bit halves); every hint; both named cases"""
    share = {"border": 0, "staged": 0, "per_tap": 0}
    seen = dict(sf=set(), dtype=set(), bgr=set(), nhwc=set(), tune=set(), mode=set())
    kinds, bases, hints = set(), set(), set()
    two_tables = shared = one_pixel = above_255 = above_2047 = mixed_alignment = three_in_one_job = 0
    for seed, k, call in all_cases("remap"):
        for key in seen:
            seen[key].add(call[key])
        jobs = call["jobs"]
        kinds |= {p["kind"] for p in call["maps"]}
        bases |= {p["xlead"] % 16 for p in call["maps"]} | {p["ylead"] % 16 for p in call["maps"]}
        hints.add("none" if call["max_step"] == 0 else "tiny" if call["max_step"] < 0.01 else "fifty" if call["max_step"] == 50.0 else "true")
        two_tables += len(jobs) > cases.TABLE["remap"]
        shared += any(a["maps"] == b["maps"] and a["frame"] != b["frame"] for i, a in enumerate(jobs) for b in jobs[i + 1:])
        mixed_alignment += len({(cases.plane_offsets(call, j)[0][0] % 16, j["layout"]["row"] % 16) for j in jobs}) > 1
        if call["tune"] != 0:
            continue
        strip = remap_strip_given(rm, call)
        for job in jobs:
            tiles = remap_tiles(rm, call, job, strip)
            for outcome, n_in, win, _ in tiles:
                share[outcome] += 1
                one_pixel += n_in == 1
                above_255 += outcome != "border" and win[1] > 255
                above_2047 += outcome != "border" and win[1] > 2047
            three_in_one_job += len({t[0] for t in tiles}) == 3
    n = sum(share.values())
    print("remap tiles under the default policy", n, share, "jobs holding all three outcomes", three_in_one_job, "two tables", two_tables, "calls with a shared pair", shared,
          "mixed alignment", mixed_alignment, "tiles with one in-range pixel", one_pixel, "windows beyond column 255", above_255, "beyond 2047", above_2047, "kinds", sorted(kinds))
    assert all(v >= 0.1 * n for v in share.values()), (share, n)
    assert seen["sf"] == set(cases.SOURCES) and seen["dtype"] == {0, 1, 2} and seen["bgr"] == {False, True} and seen["nhwc"] == {False, True}, seen
    assert seen["tune"] == {0, 9} and seen["mode"] == {0, 1}, seen
    assert two_tables >= 1 and shared >= 1 and mixed_alignment >= 1 and one_pixel >= 1 and above_255 >= 1 and above_2047 >= 1
    assert bases == {0, 4, 8, 12} and hints == {"none", "tiny", "true", "fifty"}, (bases, hints)
    assert kinds == set(cases.REMAP_KINDS) | set(cases.REMAP_NAMED), kinds


def test_remap_named_strips(rm):
    """the two named cases among the default seeds: without a hint the launch gives a strip of 65 536 - 32 bytes (remap_strip_given: the arithmetic
    of launch_convert_remap); tile (0, 0) of strip_65504 spans frame columns 0 .. 351 and rows 0 .. 45 — 46 rows of 32 x 44 + 16 bytes, exactly what
    the launch gives, and it stages —, that of strip_65520 columns 0 .. 247 and rows 0 .. 64 — 65 rows of 32 x 31 + 16 bytes, 16 more, the smallest
    strip above it (a strip is a multiple of 16 bytes, and 65 536 is no odd multiple of one) — and it goes per tap; every other tile is border"""
    found = {name: 0 for name in cases.REMAP_NAMED}
    for seed, k, call in all_cases("remap"):
        for job in call["jobs"]:
            name = call["maps"][job["maps"]]["kind"]
            if name not in cases.REMAP_NAMED:
                continue
            W, H, x_hi, y_hi, nbytes = cases.REMAP_NAMED[name]
            assert (call["W"], call["H"], call["max_step"], call["tune"]) == (W, H, 0.0, 0), cases.describe(call)
            strip = remap_strip_given(rm, call)
            assert strip == 65536 - 32 == 65504
            tiles = remap_tiles(rm, call, job, strip)
            outcome, n_in, win, got = tiles[0]
            assert win == (0, x_hi, 0, y_hi) and got == nbytes == (y_hi + 1) * (32 * ((x_hi >> 3) + 1) + 16) and n_in >= 2, (name, win, got)
            assert outcome == {"strip_65504": "staged", "strip_65520": "per_tap"}[name] and (got <= strip) == (name == "strip_65504")
            assert all(t[0] == "border" for t in tiles[1:]), name
            found[name] += 1
    print("named strips among the default seeds", found)
    assert all(v >= 1 for v in found.values()), found


# ------------------------------------------------------------------------------------------------ the independent link
@pytest.mark.parametrize("family", EXACT_CHAIN)
def test_composed_fp32_reference_is_near_the_exact_chain(oracle, family):
    """every job of every case of the default seeds: the composed FP32 reference (what the GPU must equal bit for bit) against the same composition
    in the oracle's EXACT mode — convert EXACT, crop, resize or remap EXACT with the same float32 maps — at most 2 codes apart: the conversions
    differ by at most 1 (tests/test_oracle_kat.py), a bilinear blend is a convex combination and carries that 1 through unamplified, and the
    fp32 blend against the exact blend of equal inputs adds at most 1.
    Measured maximum over these cases: rois 1, letterbox 1, warp 1, persp 1, remap 1 (the bound stays 2).  The remap's composition is the warp's
    on maps it was handed instead of maps it computed, so the argument applies unchanged; the antialiased letterbox has no EXACT mode in the oracle
    and is tied to the outside by tests/test_letterbox_aa_definition_cpu.py instead."""
    oracle.set_threads(16)
    worst = n = 0
    for seed, k, call in all_cases(family):
        srcs = host_frames(oracle, call)
        fp32, exact = rgb_frames(oracle, call, srcs), rgb_frames(oracle, call, srcs, oracle.EXACT)
        for i, job in enumerate(call["jobs"]):
            a, b = job_u8(oracle, call, job, fp32[job["frame"]]), job_u8_exact(oracle, call, job, exact[job["frame"]])
            d = int(np.abs(a.astype(np.int16) - b.astype(np.int16)).max())
            worst, n = max(worst, d), n + 1
            assert d <= 2, f"seed {seed} case {k} job {i}: {d} codes apart; {cases.describe(call)}"
        if call["sf"] in P16:
            forget_p16()
    print(family, "jobs", n, "largest |FP32 chain - EXACT chain|", worst)
