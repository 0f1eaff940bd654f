"""The policy of the eight per-job tensor launches on the CPU: job_plan (csrc/vpf_job_plan.h), the pure function launch_convert_resize_rois
(csrc/k_convert_roi.hip), launch_convert_letterbox, launch_convert_warp, launch_convert_persp and their _dev forms dispatch on, compiled with g++ as
it stands (tests/c/job_plan_capi.cpp).

1. tests/golden/job_plan_kat.json: launches recorded from the launchers as they were before the policy became a function (hash in the file) —
   label, grid, the dynamic LDS the launch asked for, the epilogue's dtype word, the scalar kernel arguments and, for host tables, which job of the
   call sits in which slot of which table.  The plan, plus nhwc_stage_plan (csrc/vpf_internal.h) restated here, must give each.
2. Every rule, asserted on the plan's fields at a shape on either side of its limit.
3. Refusals and invariants, restated here without the golden file, over a seeded sweep of 30 000 shapes.
4. For every row of the case table of the GPU test (tests/cases_job_families.py) the plan selects what the row claims; labels_of() derives the labels
   the GPU test reads off the selection log.

Channels-last staging "does not fit": the issue asked for recorded rows where strip + staging area exceed 64 KiB.  No launch of these eight reaches
that: a staged ROI / letterbox job converts at most kRoiConvMax = 3 source pixels per destination pixel, so its strip is at most 12 B x the 4 096
pixels of a tile = 49 152 B (the device forms: roi_dev_lds_bytes, the same figure), the f32 staging area is 12 288 B, together 61 440 B; 16-bit rows
do not stage, and the warps never do.  The sweep asserts that bound; the not-fitting branch of nhwc_stage_plan is covered on the restated function
alone (test_stage_plan_restated)."""
import ctypes as C
import json
import os
import random
import struct
import subprocess

import numpy as np
import pytest

import cases_job_families as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROI, LB, WARP, PERSP = range(4)
F32, F16, BF16 = 0, 1, 2
SWAP_RB = 0x80000000
FORM_NAMES = ["k_roi_strip", "k_roi_gather", "k_roi_dev", "k_lb_strip", "k_lb_gather", "k_lb_dev", "k_warp_strip", "k_warp_gather", "k_warp_dev",
              "k_persp_strip", "k_persp_gather", "k_persp_dev"]


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    from conftest import native_test_build
    so = str(tmp_path_factory.mktemp("jp") / "libjobplan.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-shared", "-fPIC", "-Wall", "-Werror", *native_test_build()[0],
                           "-I" + os.path.join(ROOT, "videoprocessingframework_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "job_plan_capi.cpp"), "-o", so, "-lm"])
    lib = C.CDLL(so)
    u32, PU = C.c_uint32, C.POINTER(C.c_uint32)
    lib.jp_plan.argtypes, lib.jp_plan.restype = [PU, C.c_float, PU, PU, C.POINTER(C.c_uint8)], None
    lib.jp_form.argtypes, lib.jp_form.restype = [C.c_int, C.POINTER(C.c_char_p)], C.c_char_p
    lib.jp_limits.argtypes = [PU]
    lib.jp_roi_conv_max.restype = C.c_double
    lib.jp_job_need.argtypes, lib.jp_job_need.restype = [C.c_int, PU, u32, u32, u32, u32, C.POINTER(C.c_double)], u32
    lib.jp_dev_bytes.argtypes, lib.jp_dev_bytes.restype = [C.c_int, C.c_float, u32, u32, u32, u32], u32
    lib.jp_tensor_dmask.argtypes, lib.jp_tensor_dmask.restype = [C.c_int, C.c_int], u32
    return lib


@pytest.fixture(scope="module")
def forms(L):
    out = []
    for f in range(L.jp_forms()):
        args = C.c_char_p()
        out.append((L.jp_form(f, C.byref(args)).decode(), args.value.decode().split()))
    assert [n for n, _ in out] == FORM_NAMES
    return out


@pytest.fixture(scope="module")
def limits(L):
    v = (C.c_uint32 * 9)()
    L.jp_limits(v)
    return dict(caps=list(v[:4]), table_max=v[4], dev_max=v[5], dev_frames=v[6], roi_strip_max=v[7], warp_strip_max=v[8], conv_max=L.jp_roi_conv_max())


def bits(v):
    return struct.unpack("<I", struct.pack("<f", v))[0]


def roi_words(rect, dw, dh, place=(0, 0, 0, 0)):
    """the nine words of a ROI / letterbox job as the C entry forms them: the scale factors are fp32 quotients on the destination's (the picture's) size"""
    x, _, w, h = rect
    iw, ih = (place[2], place[3]) if place[2] else (dw, dh)
    return [x, w, h, bits(np.float32(w) / np.float32(iw)), bits(np.float32(h) / np.float32(ih)), *place]


def mat_words(m):
    return [bits(float(np.float32(v))) for v in m] + [0] * (9 - len(m))


def plan(L, family, dev, src, nhwc, dtype, W, H, dw, dh, knob, geoms=(), max_n=0, n_frames=0, max_step=0.0):
    """-> dict(ok, nd, dmask, d = [dict(form, gx, gy, n, lds, npx)], which)"""
    n = len(geoms)
    head = (C.c_uint32 * 13)(family & 0xFFFFFFFF, int(dev), src & 0xFFFFFFFF, int(nhwc), dtype, W, H, dw, dh, knob & 0xFFFFFFFF, n, max_n, n_frames)
    flat = (C.c_uint32 * max(1, 9 * n))(*[w for g in geoms for w in g])
    out, which = (C.c_uint32 * 15)(), (C.c_uint8 * max(1, n))()
    L.jp_plan(head, max_step, flat, out, which)
    d = [dict(zip(("form", "gx", "gy", "n", "lds", "npx"), out[3 + 6 * k:9 + 6 * k])) for k in range(out[1])]
    return dict(ok=out[0], nd=out[1], dmask=out[2], d=d, which=list(which[:min(n, 96)]))


def nhwc_stage_plan(dtype, lds, npx):
    """csrc/vpf_internal.h with VPF_NHWC_DENSE = 1 | 4 -> (the dynamic LDS to ask for, the epilogue's dtype word)"""
    dt = dtype & 0xFF
    want = True if dt == F32 else bool((1 | 4) & (4 if npx == 8 else 2))
    nbytes = 4 * 64 * 3 * npx * (4 if dt == F32 else 2)
    if not want or lds & 15 or lds + nbytes > 64 * 1024:
        return lds, dtype
    return lds + nbytes, dtype | ((lds // 16 + 1) << 8)


def launch_of(P, k, forms, src, nhwc, dtype, W, H, dw, dh):
    """what dispatch k of a plan launches: (label, grid, dynamic LDS, epilogue dtype, scalar arguments)"""
    d = P["d"][k]
    name, words = forms[d["form"]]
    lds_all, e = nhwc_stage_plan(dtype, d["lds"], d["npx"]) if d["npx"] else (d["lds"], dtype)
    val = dict(W=W, H=H, dw=dw, dh=dh, dmask=P["dmask"], lds=d["lds"])
    return ["(%s<%d, %d>)" % (name, src, 8 if nhwc else 6), [d["gx"], d["gy"], d["n"]], lds_all, e, [val[w] for w in words]]


def test_stage_plan_restated():
    assert nhwc_stage_plan(F32, 4624, 4) == (4624 + 12288, F32 | (290 << 8))
    assert nhwc_stage_plan(F32 | SWAP_RB, 0, 4) == (12288, F32 | SWAP_RB | (1 << 8))
    assert nhwc_stage_plan(F32, 53248, 4) == (65536, F32 | (3329 << 8)) and nhwc_stage_plan(F32, 53264, 4) == (53264, F32)   # strip + area > 64 KiB: no staging
    assert nhwc_stage_plan(F32, 4616, 4) == (4616, F32)                                                                    # an unaligned strip
    assert nhwc_stage_plan(F16, 4624, 4) == (4624, F16) and nhwc_stage_plan(BF16, 0, 4) == (0, BF16)                        # 16-bit rows of the 4-px families
    assert nhwc_stage_plan(F16, 0, 8) == (12288, F16 | (1 << 8))


# ---- 1. the known answers
def test_known_answers(L, forms, limits):
    path = os.path.join(ROOT, "tests", "golden", "job_plan_kat.json")
    doc = json.load(open(path))
    assert len(doc["parent_commit"]) == 40 and 300 <= len(doc["rows"]) <= 1000
    assert os.path.getsize(path) <= max(os.path.getsize(os.path.join(ROOT, "tests", "golden", f)) for f in
                                        ("convert_plan_kat.json", "fused_plan_kat.json", "lzm_launch_kat.json", "resize_plan_kat.json"))
    geoms = doc["geoms"]
    seen = dict(labels=set(), knobs=set(), dtypes=set(), shapes=set(), staged=set(), hints=set(), sizes=set(), stage=set())
    for family, dev, src, nhwc, dtype, W, H, dw, dh, knob, tail, launches in doc["rows"]:
        row = (family, dev, src, nhwc, dtype, W, H, dw, dh, knob, tail)
        if dev:
            P = plan(L, family, True, src, nhwc, dtype, W, H, dw, dh, knob, max_n=tail[0], n_frames=tail[1], max_step=tail[2])
            seen["hints"].add((family, tail[2] > 0))
            seen["sizes"].add(("max_n", tail[0]))
            seen["sizes"].add(("n_frames", tail[1]))
        else:
            P = plan(L, family, False, src, nhwc, dtype, W, H, dw, dh, knob, [geoms[g] for g in tail])
            seen["sizes"].add((family, len(tail)))
        assert P["ok"] and P["nd"] == len(launches), (row, P)
        for k, (label, grid, lds, e, args, slots) in enumerate(launches):
            assert launch_of(P, k, forms, src, nhwc, dtype, W, H, dw, dh) == [label, grid, lds, e, args], (row, k, P)
            if not dev:
                assert [i for i, w in enumerate(P["which"]) if w == k] == slots, (row, k, P["which"])   # call indices, slot by slot
            seen["labels"].add(label)
            if nhwc and family <= LB:
                seen["stage"].add((dtype & 0xFF, lds != P["d"][k]["lds"]))
        if not dev:
            w = P["which"]
            kinds = {FORM_NAMES[P["d"][i]["form"]].split("_")[-1] for i in range(P["nd"])}
            staged = [i for i in range(len(w)) if FORM_NAMES[P["d"][w[i]]["form"]].endswith("strip")]
            contiguous = not staged or staged == list(range(staged[0], staged[-1] + 1))
            seen["shapes"].add((family, "mixed" if len(kinds) == 2 else kinds.pop(), contiguous))
        seen["knobs"].add(knob)
        seen["dtypes"].add(dtype & 0xFF)
    # every one of the 12 kernel families in every (source, layout) instantiation
    assert seen["labels"] == {"(%s<%d, %d>)" % (n, s, d) for n in FORM_NAMES for s in (0, 1, 7) for d in (6, 8)}
    assert seen["knobs"] == {0, 9} and seen["dtypes"] == {F32, F16, BF16}
    for family in range(4):
        assert {(family, "strip", True), (family, "gather", True), (family, "mixed", False)} <= seen["shapes"], seen["shapes"]   # all staged, all per tap, mixed with the staged jobs apart
        assert {(family, 1), (family, limits["caps"][family])} <= seen["sizes"]
    assert {(WARP, False), (WARP, True), (PERSP, False), (PERSP, True)} <= seen["hints"]
    assert {("max_n", 1), ("max_n", 65535), ("n_frames", 1), ("n_frames", 128)} <= seen["sizes"]
    assert seen["stage"] == {(F32, True), (F16, False), (BF16, False)}   # f32 rows stage (the area always fits: the module's docstring), 16-bit rows do not


# ---- 2. the rules
SMALL = dict(W=1920, H=1080, dw=224, dh=224)
ROI_S, ROI_T = roi_words((2, 0, 224, 224), 224, 224), roi_words((3, 0, 1344, 1080), 224, 224)
LB_S, LB_T = roi_words((2, 0, 216, 216), 224, 224, (4, 4, 216, 216)), roi_words((3, 0, 456, 450), 224, 224, (4, 6, 76, 75))
ID, DOWN6 = mat_words((1, 0, 3, 0, 1, 2)), mat_words((6, 0, 0, 0, 6, 1))
IDP, DOWN6P = mat_words((1, 0, 3, 0, 1, 2, 0, 0, 1)), mat_words((6, 0, 0, 0, 6, 1, 0, 0, 1))
STAGED, PER_TAP = [ROI_S, LB_S, ID, IDP], [ROI_T, LB_T, DOWN6, DOWN6P]


def host(L, family, geoms, src=0, nhwc=False, dtype=F32, knob=0, **kw):
    s = dict(SMALL, **kw)
    return plan(L, family, False, src, nhwc, dtype, s["W"], s["H"], s["dw"], s["dh"], knob, geoms)


def devp(L, family, max_n=4, n_frames=2, max_step=0.0, src=0, nhwc=False, dtype=F32, knob=0, **kw):
    s = dict(SMALL, **kw)
    return plan(L, family, True, src, nhwc, dtype, s["W"], s["H"], s["dw"], s["dh"], knob, max_n=max_n, n_frames=n_frames, max_step=max_step)


def test_caps_and_refusals(L, limits):
    assert limits["caps"] == [96, 82, 96, 82] and limits["table_max"] == 96 and limits["dev_max"] == 65535 and limits["dev_frames"] == 128
    for family, cap in enumerate(limits["caps"]):
        assert not host(L, family, [])["ok"]
        assert host(L, family, [STAGED[family]])["ok"]
        P = host(L, family, [STAGED[family]] * cap)
        assert P["ok"] and P["nd"] == 1 and P["d"][0]["n"] == cap
        assert not host(L, family, [STAGED[family]] * (cap + 1))["ok"]
        for max_n, ok in ((0, 0), (1, 1), (65535, 1), (65536, 0)):
            P = devp(L, family, max_n=max_n)
            assert P["ok"] == ok and (not ok or (P["nd"] == 1 and P["d"][0]["n"] == max_n)), (family, max_n)
        for n_frames, ok in ((0, 0), (1, 1), (128, 1), (129, 0)):
            assert devp(L, family, n_frames=n_frames)["ok"] == ok, (family, n_frames)
        for src in range(-1, 10):   # FC_NV12 = 0, FC_YUV420 = 1, FC_P16 = 7
            assert host(L, family, [STAGED[family]], src=src)["ok"] == (src in (0, 1, 7)) == devp(L, family, src=src)["ok"], (family, src)
    assert not plan(L, 4, False, 0, False, F32, 64, 64, 8, 8, 0, [ROI_S])["ok"] and not plan(L, -1, True, 0, False, F32, 64, 64, 8, 8, 0, max_n=1, n_frames=1)["ok"]


def need(L, family, words, W, H, dw, dh):
    conv = C.c_double()
    return L.jp_job_need(family, (C.c_uint32 * 9)(*words), W, H, dw, dh, C.byref(conv)), conv.value


def test_roi_limits_decide_roi_and_letterbox_jobs(L, limits):
    """a 224-wide destination, the rectangle's height growing from 1 x to 4.8 x: staged exactly while the strip fits kRoiStripMax AND converts at most
    kRoiConvMax source pixels per destination pixel — heights on either side of the conversion limit and of the strip limit"""
    assert limits["roi_strip_max"] == 53 * 1024 and limits["conv_max"] == 3.0
    for family in (ROI, LB):
        place = (0, 0, 224, 224) if family == LB else (0, 0, 0, 0)
        flips = over = 0
        for h in range(224, 1080):
            w = roi_words((0, 0, 448, h), 224, 224, place)
            nbytes, conv = need(L, family, w, 1920, 1080, 224, 224)
            P = host(L, family, [w])
            staged = nbytes <= limits["roi_strip_max"] and conv <= limits["conv_max"]
            assert FORM_NAMES[P["d"][0]["form"]].endswith("strip" if staged else "gather"), (family, h, nbytes, conv)
            assert P["d"][0]["lds"] == (nbytes if staged else 0)
            flips += (conv > limits["conv_max"]) and nbytes <= limits["roi_strip_max"]
            over += nbytes > limits["roi_strip_max"]
            # kRoiStripMax never decides alone: conv <= 3 bounds the strip by 12 B x the 4 096 pixels of a tile, below 53 KiB.  The rule keeps both limits.
            assert conv > limits["conv_max"] or nbytes <= 12 * 4096
        assert flips   # the conversion limit decided some of them while the strip still fitted
        assert over   # ... and strips past kRoiStripMax occurred: every one of them also converts more than three pixels per pixel (asserted above)


def test_warp_strip_max_decides_warp_and_perspective_jobs(L, limits):
    assert limits["warp_strip_max"] == 64 * 1024
    for family in (WARP, PERSP):
        sides = set()
        for s in [1.0 + 0.05 * i for i in range(100)]:
            w = mat_words((s, 0, 0, 0, s, 0) + ((0, 0, 1) if family == PERSP else ()))
            nbytes, _ = need(L, family, w, 1920, 1080, 224, 224)
            P = host(L, family, [w])
            staged = nbytes <= limits["warp_strip_max"]
            assert FORM_NAMES[P["d"][0]["form"]].endswith("strip" if staged else "gather") and P["d"][0]["lds"] == (nbytes if staged else 0), (family, s, nbytes)
            sides.add(staged)
        assert sides == {True, False}
    # the horizon through the destination: no bound, the full 64 KiB, staged; wholly behind the plane: 0 bytes, staged with no strip
    P = plan(L, PERSP, False, 0, False, F32, 64, 32, 16, 16, 0, [mat_words((1, 0, 2, 0, 1, 1, 0, -0.1, 1))])
    assert (FORM_NAMES[P["d"][0]["form"]], P["d"][0]["lds"]) == ("k_persp_strip", 65536)
    P = plan(L, PERSP, False, 0, False, F32, 64, 32, 16, 16, 0, [mat_words((1, 0, 2, 0, 1, 1, 0, 0, -1))])
    assert (FORM_NAMES[P["d"][0]["form"]], P["d"][0]["lds"]) == ("k_persp_strip", 0)


def test_knob_9_stages_nothing(L):
    for family in range(4):
        jobs = [STAGED[family], PER_TAP[family], STAGED[family]]
        P = host(L, family, jobs)
        assert [FORM_NAMES[d["form"]].split("_")[-1] for d in P["d"]] == ["strip", "gather"] and P["which"] == [0, 1, 0] and [d["n"] for d in P["d"]] == [2, 1]
        for knob in (4, 8, 40, 43, 1000):   # the other values of the shared key mean the policy
            assert host(L, family, jobs, knob=knob) == P
        P9 = host(L, family, jobs, knob=9)
        assert P9["nd"] == 1 and FORM_NAMES[P9["d"][0]["form"]].endswith("gather") and P9["d"][0]["n"] == 3 and P9["d"][0]["lds"] == 0 and P9["which"] == [0, 0, 0]
        for step in (0.0, 1.5):
            assert devp(L, family, max_step=step)["d"][0]["lds"] > 0 and devp(L, family, max_step=step, knob=9)["d"][0]["lds"] == 0


def test_grids(L):
    """ROI / letterbox: 256 x 16 tiles for the staged and device forms, 256 x 4 (64 lanes x 4 px, four rows) for the per-tap form; the warps: 32 x 32
    tiles in every form — at a size on either side of each tile edge"""
    for dw, dh in ((256, 16), (257, 17), (1, 1), (32, 32), (33, 33), (512, 4), (513, 5)):
        for family in range(4):
            place = (0, 0, dw, dh) if family == LB else (0, 0, 0, 0)
            big = min(1920, 8 * dw), min(1080, 8 * dh)
            jobs = [mat_words((1, 0, 0, 0, 1, 0, 0, 0, 1)[:6 if family == WARP else 9]), mat_words((60, 0, 0, 0, 60, 0, 0, 0, 1)[:6 if family == WARP else 9])] if family >= WARP else \
                   [roi_words((0, 0, min(1920, dw), min(1080, dh)), dw, dh, place), roi_words((0, 0, *big), dw, dh, place)]
            P, D = host(L, family, jobs, dw=dw, dh=dh), devp(L, family, dw=dw, dh=dh)
            tile = ((dw + 31) // 32, (dh + 31) // 32) if family >= WARP else ((dw + 255) // 256, (dh + 15) // 16)
            tap = tile if family >= WARP else (((dw + 3) // 4 + 63) // 64, (dh + 3) // 4)
            for d in P["d"] + D["d"]:
                assert (d["gx"], d["gy"]) == (tap if FORM_NAMES[d["form"]].endswith("gather") else tile), (family, dw, dh, d)
            assert D["d"][0]["n"] == 4
            if (dw, dh) != (1, 1):   # (one pixel has no window to outgrow anything)
                assert {FORM_NAMES[d["form"]].split("_")[-1] for d in P["d"]} == {"strip", "gather"}, (family, dw, dh, P)


def test_staging_pixel_count_and_mask(L):
    for family in range(4):
        for nhwc in (False, True):
            for dtype in (F32, F16, BF16, F32 | SWAP_RB, F16 | SWAP_RB):
                if dtype & SWAP_RB and not nhwc:
                    continue   # the bit is only ever set for a channels-last destination
                P, D = host(L, family, [STAGED[family], PER_TAP[family]], nhwc=nhwc, dtype=dtype), devp(L, family, nhwc=nhwc, dtype=dtype)
                npx = 4 if nhwc and family <= LB else 0   # the warps never name a staging pixel count
                assert [d["npx"] for d in P["d"] + D["d"]] == [npx] * 3, (family, nhwc, dtype)
                mask = 15 if nhwc or dtype == F32 else 7
                assert P["dmask"] == D["dmask"] == mask == L.jp_tensor_dmask(int(nhwc), int(dtype == F32))


# ---- 3. the sweep
def test_seeded_sweep(L, forms, limits):
    rnd = random.Random(24)
    counts = dict(refused=0, mixed=0, dev=0, staged_area=0)
    for it in range(30000):
        family = rnd.choice((ROI, LB, WARP, PERSP, ROI, LB, WARP, PERSP, -1, 4)) if it % 50 == 0 else rnd.randrange(4)
        f = family if 0 <= family < 4 else 0
        dev = rnd.random() < 0.35
        src = rnd.choice((0, 1, 7)) if rnd.random() < 0.95 else rnd.choice((2, 3, 4, 5, 6, 8, -1))
        nhwc, dtype = rnd.random() < 0.5, rnd.choice((F32, F16, BF16))
        if nhwc and rnd.random() < 0.3:
            dtype |= SWAP_RB
        W, H = rnd.choice(((1920, 1080), (3840, 2160), (640, 360), (72, 40), (333, 111), (65536, 16)))
        dw, dh = rnd.choice(((224, 224), (640, 640), (8, 4), (257, 17), (33, 65), (1, 1), (1024, 48), (300, 37)))
        knob = rnd.choice((0, 0, 0, 9, 40))
        cap = limits["caps"][f]
        if dev:
            max_n, n_frames = rnd.choice((0, 1, 2, 100, 65535, 65536, 1 << 20)), rnd.choice((0, 1, 2, 127, 128, 129, 4000))
            step = rnd.choice((0.0, 0.0, 0.25, 1.0, 2.5, 9.0, 1e6, -1.0))
            P = plan(L, family, True, src, nhwc, dtype, W, H, dw, dh, knob, max_n=max_n, n_frames=n_frames, max_step=step)
            refused = not (0 <= family < 4) or src not in (0, 1, 7) or not max_n or max_n > 65535 or not n_frames or n_frames > 128
            assert bool(P["ok"]) == (not refused), (it, family, src, max_n, n_frames)
            if refused:
                counts["refused"] += 1
                assert P["nd"] == 0
                continue
            counts["dev"] += 1
            d = P["d"][0]
            assert P["nd"] == 1 and d["form"] == 3 * family + 2 and d["n"] == max_n
            assert d["lds"] == (0 if knob == 9 else L.jp_dev_bytes(family, step, W, H, dw, dh))
            assert d["lds"] <= (limits["roi_strip_max"] if family <= LB else limits["warp_strip_max"])
            geoms, which = [], []
        else:
            n = rnd.choice((0, 1, 1, 2, 3, 3, 5, 9, cap - 1, cap, cap + 1, 97)) if it % 10 == 0 else rnd.choice((1, 2, 3, 4, 6))
            geoms = []
            for _ in range(n):
                if f <= LB:
                    iw, ih = (rnd.randint(1, dw), rnd.randint(1, dh)) if f == LB else (dw, dh)
                    ix, iy = (rnd.randint(0, dw - iw), rnd.randint(0, dh - ih)) if f == LB else (0, 0)
                    sc = rnd.choice((0.4, 1.0, 1.2, 1.6, 2.2, 3.5, 9.0))
                    w, h = max(1, min(W, int(iw * sc * rnd.uniform(0.8, 1.25)))), max(1, min(H, int(ih * sc * rnd.uniform(0.8, 1.25))))
                    geoms.append(roi_words((rnd.randint(0, W - w), 0, w, h), dw, dh, (ix, iy, iw, ih) if f == LB else (0, 0, 0, 0)))
                else:
                    s, a = rnd.choice((0.5, 1.0, 1.5, 2.5, 4.0, 6.0, 12.0, 50.0)), rnd.uniform(-3.2, 3.2)
                    m = (s * np.cos(a), -s * np.sin(a), rnd.uniform(-50, W), s * np.sin(a), s * np.cos(a), rnd.uniform(-50, H))
                    if f == PERSP:
                        m += (rnd.choice((0.0, 1e-4, -1e-3, 0.01)), rnd.choice((0.0, 2e-4, -0.02, -0.1)), rnd.choice((1.0, 1.0, 1.0, 0.5, -1.0)))
                    geoms.append(mat_words(m))
            P = plan(L, family, False, src, nhwc, dtype, W, H, dw, dh, knob, geoms)
            refused = not (0 <= family < 4) or src not in (0, 1, 7) or not n or n > cap
            assert bool(P["ok"]) == (not refused), (it, family, src, n)
            if refused:
                counts["refused"] += 1
                assert P["nd"] == 0
                continue
            # which jobs the policy stages, restated from the bound functions
            lim = limits["roi_strip_max"] if family <= LB else limits["warp_strip_max"]
            needs = [need(L, family, g, W, H, dw, dh) for g in geoms]
            staged = [knob != 9 and nb <= lim and (family >= WARP or conv <= limits["conv_max"]) for nb, conv in needs]
            ns = sum(staged)
            names = [FORM_NAMES[d["form"]] for d in P["d"]]
            assert names == ([FORM_NAMES[3 * family]] if ns else []) + ([FORM_NAMES[3 * family + 1]] if ns < n else []), (it, names, staged)   # staged comes first
            which = P["which"]
            # every job in exactly one dispatch, staged and per-tap jobs each in call order (slots are filled in call order from `which`)
            assert [names[w].endswith("strip") for w in which] == staged and [which.count(k) for k in range(P["nd"])] == [d["n"] for d in P["d"]]
            for d in P["d"]:
                if FORM_NAMES[d["form"]].endswith("strip"):
                    assert d["lds"] == max(nb for (nb, _), s in zip(needs, staged) if s) <= lim    # the largest staged job's bytes, within the family's limit
                else:
                    assert d["lds"] == 0
            counts["mixed"] += P["nd"] == 2
        assert P["dmask"] == (15 if nhwc or dtype == F32 else 7)
        for k, d in enumerate(P["d"]):
            # the grid covers dw x dh with its family's tile, and no further than one tile
            tw, th = (32, 32) if family >= WARP else ((256, 4) if FORM_NAMES[d["form"]].endswith("gather") else (256, 16))
            assert (d["gx"] - 1) * tw < dw <= d["gx"] * tw and (d["gy"] - 1) * th < dh <= d["gy"] * th, (it, d)
            assert d["npx"] == (4 if nhwc and family <= LB else 0)
            lds_all, e = launch_of(P, k, forms, src, nhwc, dtype, W, H, dw, dh)[2:4]
            assert lds_all <= 64 * 1024 and lds_all >= d["lds"]   # what the launch asks for after staging
            if d["npx"] and (dtype & 0xFF) == F32:
                assert lds_all == d["lds"] + 12288 <= 61440 and e != dtype   # the area always fits behind a ROI / letterbox strip (the module's docstring)
                counts["staged_area"] += 1
            else:
                assert lds_all == d["lds"] and e == dtype
    assert counts["refused"] > 1500 and counts["mixed"] > 1000 and counts["dev"] > 3000 and counts["staged_area"] > 1000, counts


# ---- 4. the case table of the GPU test
def case_geoms(row):
    dw, dh = row["dw"], row["dh"]
    if row["family"] == ROI:
        return [roi_words(r, dw, dh) for r in row["jobs"]]
    if row["family"] == LB:
        return [roi_words(r, dw, dh, p) for r, p in row["jobs"]]
    return [mat_words(m) for m in row["jobs"]]


def case_plans(L, row):
    """the plans of a row's launcher calls: a host call is cut into tables of the family's cap (csrc/vpf_abi.hip)"""
    head = (row["family"], row["dev"], cases.SRC_FC[row["sf"]], row["nhwc"], row["dtype"], row["W"], row["H"], row["dw"], row["dh"], row["knob"])
    if row["dev"]:
        return [plan(L, *head, max_n=len(row["jobs"]), n_frames=1, max_step=row["max_step"])]
    g, cap = case_geoms(row), cases.CAPS[row["family"]]
    return [plan(L, *head, g[b:b + cap]) for b in range(0, len(g), cap)]


def labels_of(L, row):
    """the labels the selection log must show for the row, in launch order — from the plan alone"""
    return ["(%s<%d, %d>)" % (FORM_NAMES[d["form"]], cases.SRC_FC[row["sf"]], 8 if row["nhwc"] else 6) for P in case_plans(L, row) for d in P["d"]]


def test_case_table_selects_what_it_claims(L, limits):
    seen = set()
    assert list(cases.CAPS) == limits["caps"]
    for row in cases.CASES:
        plans = case_plans(L, row)
        assert all(P["ok"] for P in plans), row["name"]
        if row["dev"]:
            d = plans[0]["d"][0]
            assert FORM_NAMES[d["form"]] == FORM_NAMES[3 * row["family"] + 2] and (d["lds"] == 0) == (row["knob"] == 9), row["name"]
        else:
            got = "".join("S" if FORM_NAMES[P["d"][w]["form"]].endswith("strip") else "T" for P in plans for w in P["which"])
            assert got == row["want"], (row["name"], got)
        assert labels_of(L, row) == cases.labels(row), row["name"]
        seen |= set(labels_of(L, row))
    assert seen == {"(%s<%d, %d>)" % (n, s, d) for n in FORM_NAMES for s in (0, 1, 7) for d in (6, 8)}
    by = {r["name"]: r for r in cases.CASES}
    assert len(labels_of(L, by["roi_97"])) == 3 and len(labels_of(L, by["letterbox_83"])) == 3   # two dispatches, then the second table's one job
    # the policy figures the table names (csrc/vpf_job_bounds.h)
    nb, conv = need(L, ROI, roi_words((2, 0, 64, 32), 64, 32), 72, 40, 64, 32)
    assert nb == 4624 and abs(conv - 1.13) < 0.005
    assert abs(need(L, ROI, roi_words((3, 0, 60, 30), 8, 4), 72, 40, 8, 4)[1] - 45) < 0.5
    ident, down5 = (1, 0, 3, 0, 1, 2), (5, 0, 0, 0, 5, 0)
    assert need(L, WARP, mat_words(ident), 64, 32, 16, 8)[0] == 1120 and need(L, PERSP, mat_words(ident + (0, 0, 1)), 64, 32, 16, 8)[0] == 1344
    assert need(L, WARP, mat_words(down5), 160, 160, 32, 32)[0] == 103648 and need(L, PERSP, mat_words(down5 + (0, 0, 1)), 160, 160, 32, 32)[0] == 104960
    assert plan(L, PERSP, False, 0, False, F32, 64, 32, 16, 16, 0, [mat_words(cases.HORIZON)])["d"][0]["lds"] == 65536
