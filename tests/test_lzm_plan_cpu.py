"""Host-side planning of the matrix-core Lanczos launch (csrc/vpf_lzm_plan.h, compiled here with g++: no HIP, no GPU):
  * the launch-shape planner against the measured sweeps in profiles/ — the cost model must keep picking shapes close to the best measured;
  * the weight-table cache against its contract (what makes "a table in use can never change" and "a stream never reads a table whose
    build it is not ordered behind" true);
  * the launch description (lzm_launch: what launch_lanczos_mfma of csrc/k_lanczos_mfma.hip dispatches on) against the launches recorded from the launcher
    as it was before (tests/golden/lzm_launch_kat.json), its refusals in order, the form table, and invariants restated over a seeded sweep."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lzp():
    from conftest import compile_to, native_test_build
    extra, out = native_test_build()
    so = os.path.join(out, "liblzm_plan_capi.so")
    src = os.path.join(ROOT, "tests", "c", "lzm_plan_capi.cpp")
    hdr = os.path.join(ROOT, "videoprocessingframework_amd", "csrc")
    deps = [src, os.path.join(hdr, "vpf_lzm_plan.h"), os.path.join(hdr, "vpf_plan_bounds.h"), os.path.join(hdr, "vpf_classes.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        compile_to(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", *extra, "-I", hdr, src, "-o", so, "-lm", "-pthread"], so)
    L = C.CDLL(so)
    L.lzp_plan.argtypes = [C.c_int, C.POINTER(C.c_uint32), C.c_uint32, C.c_int, C.c_int, C.POINTER(C.c_uint32)]
    L.lzp_cache_new.restype = C.c_void_p
    L.lzp_cache_new.argtypes = [C.c_uint64]
    L.lzp_cache_free.argtypes = [C.c_void_p]
    L.lzp_cache_launch.restype = C.c_uint32
    L.lzp_cache_launch.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_int] + [C.c_uint32] * 5 + [C.c_uint64]
    L.lzp_cache_launch2.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.POINTER(C.c_uint32), C.c_uint64, C.POINTER(C.c_uint32), C.c_uint64, C.POINTER(C.c_uint32)]
    L.lzp_cache_used.restype = C.c_uint64
    L.lzp_cache_used.argtypes = [C.c_void_p, C.c_int]
    L.lzp_cache_entries.restype = C.c_uint32
    L.lzp_cache_entries.argtypes = [C.c_void_p, C.c_int]
    L.lzp_sync_complete.argtypes = [C.c_void_p, C.c_uint64]
    L.lzp_sync_next.restype = C.c_uint64
    L.lzp_sync_next.argtypes = [C.c_void_p]
    L.lzp_sync_live.argtypes = [C.c_void_p]
    L.lzp_sync_reset_device.argtypes = [C.c_void_p, C.c_int]
    L.lzp_sync_stream_states.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64]
    L.lzp_sync_log.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
    L.lzp_ws_get.restype = C.c_uint32
    L.lzp_ws_get.argtypes = [C.POINTER(C.c_uint64), C.c_uint64, C.c_uint64, C.c_int, C.c_int] + [C.c_uint32] * 5 + [C.c_uint64, C.POINTER(C.c_uint32)]
    L.lzp_ws_n.restype = C.c_uint32
    L.lzp_ws_n.argtypes = [C.POINTER(C.c_uint64)]
    L.lzp_table_bytes_bound.restype = C.c_uint64
    L.lzp_table_bytes_bound.argtypes = [C.c_int, C.c_uint32, C.c_uint32]
    L.lzp_launch.argtypes = [C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.c_uint32, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint64)]
    L.lzp_form.restype = C.c_char_p
    L.lzp_form.argtypes = [C.c_int, C.POINTER(C.c_uint32)]
    L.lzp_form_of.argtypes = [C.c_int, C.c_int, C.c_uint32, C.c_int, C.c_int]
    L.lzp_cache_begin.argtypes = [C.c_void_p, C.c_int]
    L.lzp_cache_get.restype = C.c_uint32
    L.lzp_cache_get.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.POINTER(C.c_uint32), C.c_uint64]
    L.lzp_cache_end.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_int]
    assert (L.lzp_launch_head(), L.lzp_launch_plane()) == (len(LAUNCH_HEAD), len(LAUNCH_PLANE) + 2 * len(TABLE_REQ))
    return L


LAUNCH_HEAD = ("why", "form", "tables", "pair", "up2", "gx", "gy", "gz", "rts", "rows", "pitch", "lds", "a2", "lds_tabled", "a2_tabled")
LAUNCH_PLANE = ("sw", "sh", "dw", "dh", "scx", "scy", "by0")
TABLE_REQ = ("kind", "k0", "k1", "k2", "k3", "bytes", "gx", "gy", "cols")
(OK, NO_SWITCHED_OFF, NO_COUNTS, NO_SIZE, NO_ALIGNMENT, NO_PITCH, NO_ROWS, NO_PLAN, NO_PAIR_HALF_TILES, NO_FORM) = range(10)   # LzmDecline
ALIGNED = (0x7F00_0000_0000 | 0x7F80_0000_0000 | 256, 256, 256)   # a frame table that refuses nothing: {OR of pointer | pitch, largest pitches}


def launch(L, planes, n, tune=0, knob=0, pair_build=False, frames=None, njobs=None):
    """lzm_launch (csrc/vpf_lzm_plan.h) -> the description as a dict; planes: [(ch, sw, sh, dw, dh)]; frames: per plane (bits, sp_max, dp_max)"""
    a = (C.c_uint32 * 15)(*[v for p in planes for v in p])
    f = (C.c_uint64 * 9)(*[v for p in (frames or [ALIGNED] * len(planes)) for v in p])
    out = (C.c_uint64 * (len(LAUNCH_HEAD) + 3 * (len(LAUNCH_PLANE) + 2 * len(TABLE_REQ))))()
    L.lzp_launch(len(planes) if njobs is None else njobs, a, f, n, tune, knob, int(pair_build), out)
    d = dict(zip(LAUNCH_HEAD, out))
    d["plane"] = []
    for p in range(len(planes)):
        o = list(out[len(LAUNCH_HEAD) + 25 * p:len(LAUNCH_HEAD) + 25 * (p + 1)])
        q = dict(zip(LAUNCH_PLANE, o))
        q["ctab"], q["rtab"] = dict(zip(TABLE_REQ, o[7:16])), dict(zip(TABLE_REQ, o[16:25]))
        d["plane"].append(q)
    return d


def fbits(a, b):
    """the bits of (float)a / (float)b"""
    return int((np.float32(a) / np.float32(b)).view(np.uint32))


def form(L, f):
    out = (C.c_uint32 * 6)()
    name = L.lzp_form(f, out)
    return dict(name=name.decode(), nt=out[0], pf=out[1], kc=out[2], up2=bool(out[3]), pair=bool(out[4]), max_lds=out[5])


def plan(L, planes, n, forced=0, tables=True, up2=True):
    a = (C.c_uint32 * (5 * len(planes)))(*[v for p in planes for v in p])
    out = (C.c_uint32 * 10)()
    L.lzp_plan(len(planes), a, n, forced, int(tables) | (0 if up2 else 2), out)
    return dict(ok=bool(out[0]), nt=out[1], r=out[2], span=out[3], pitch=out[4], wave_lds=out[5], group_lds=out[6], kc=out[7], rts=out[8], up2=bool(out[9]))


def planes_of(fmt, sw, sh, dw, dh):
    if fmt == "RGB":
        return [(3, sw, sh, dw, dh)]
    if fmt == "Y":
        return [(1, sw, sh, dw, dh)]
    if fmt == "NV12":
        return [(1, sw, sh, dw, dh), (2, sw // 2, sh // 2, dw // 2, dh // 2)]
    return [(1, sw, sh, dw, dh), (1, sw // 2, sh // 2, dw // 2, dh // 2), (1, sw // 2, sh // 2, dw // 2, dh // 2)]


def sweep_lines(name):
    for line in open(os.path.join(ROOT, "profiles", name)):
        m = re.match(r"\[lzm-sweep\] (\w+)\s+(\d+)x(\d+)->(\d+)x(\d+) n=(\d+):", line)
        if m:
            fmt, (sw, sh, dw, dh, nn) = m.group(1), (int(v) for v in m.groups()[1:])
            yield fmt, sw, sh, dw, dh, nn, {(int(a), int(b)): float(c) for a, b, c in re.findall(r"nt(\d) r(\d+)=([\d.]+)", line)}


def sweep_cases():
    """the round-3 sweeps, without their up-scale lines: those kernels were replaced in round 5 (the ring of two; test_planner_on_up_scales)"""
    for n in (32, 8, 1):
        for c in sweep_lines(f"r03_lanczos_shape_sweep_n{n}.txt"):
            if c[1] > c[3]:
                yield c


def pick_time(p, res):
    """the planner's pick read off a sweep at the measured band heights either side of it (outside them: the nearest one)"""
    rs = sorted(r for (nt, r) in res if nt == p["nt"])
    lo = max([r for r in rs if r <= p["r"]], default=rs[0])
    hi = min([r for r in rs if r >= p["r"]], default=rs[-1])
    return res[(p["nt"], lo)] if lo == hi else float(np.interp(p["r"], [lo, hi], [res[(p["nt"], lo)], res[(p["nt"], hi)]]))


def test_planner_stays_close_to_the_best_measured_shape(lzp):
    """For every down-scale case of the three sweeps (RGB / NV12 / YUV420 x two size pairs x 32 / 8 / 1 frames per dispatch) the planner's pick — read
    off the sweep at the measured band heights either side of it — is within 20 % of the best measured shape, 6 % on average.  A change of the
    cost model that loses more than that shows up here, without a GPU."""
    regrets = []
    for fmt, sw, sh, dw, dh, n, res in sweep_cases():
        p = plan(lzp, planes_of(fmt, sw, sh, dw, dh), n)
        assert p["ok"] and p["nt"] in (4, 8) and 2 <= p["r"] <= 64
        rs = sorted(r for (nt, r) in res if nt == p["nt"])
        lo = max([r for r in rs if r <= p["r"]], default=rs[0])      # (outside the measured band heights: the nearest one)
        hi = min([r for r in rs if r >= p["r"]], default=rs[-1])
        t = res[(p["nt"], lo)] if lo == hi else np.interp(p["r"], [lo, hi], [res[(p["nt"], lo)], res[(p["nt"], hi)]])
        regrets.append(t / min(res.values()) - 1.0)
        assert regrets[-1] <= 0.20, (fmt, sw, dw, n, p, t, min(res.values()))
    assert len(regrets) == 18 and float(np.mean(regrets)) <= 0.06, np.mean(regrets)


def test_planner_against_the_round_5_down_scale_sweeps(lzp):
    """The same question asked of sweeps taken with the round's FINAL kernels (profiles/r05_lanczos_shape_sweep_down_n*.txt: RGB / NV12 /
    YUV420 / Y x 1080p -> 720p, 4K -> 1080p, 1080p -> 900p, 4K -> 1440p at 32 / 8 / 1 frames per dispatch — two size pairs and one format the
    round-3 fit never saw): mean regret <= 5 %, worst <= 30 % (Y 4K -> 1440p, where the 0.45 of a 1-channel 4-tile strip is too cheap).  A
    refit of the five constants to these 48 cases gains 0.3 points and loses 3 on the up-scales (tools/lab/fit_lzm_down.py): they stand."""
    regrets = []
    for n in (32, 8, 1):
        for fmt, sw, sh, dw, dh, nn, res in sweep_lines(f"r05_lanczos_shape_sweep_down_n{n}.txt"):
            p = plan(lzp, planes_of(fmt, sw, sh, dw, dh), nn)
            assert p["ok"] and not p["up2"]
            regrets.append(pick_time(p, res) / min(res.values()) - 1.0)
            assert regrets[-1] <= 0.30, (fmt, sw, dw, nn, p, min(res.values()))
    assert len(regrets) == 48 and float(np.mean(regrets)) <= 0.05, (len(regrets), np.mean(regrets))


def test_planner_on_up_scales(lzp):
    """The ring-of-two kernels (round 5) against their own sweeps (profiles/r05_lanczos_shape_sweep_up_n*.txt: RGB / NV12 / YUV420 / Y x five
    up-scales at 32 / 8 / 1 frames per dispatch, four at 64 / 128): 2 x up-scales take 8-tile strips (three workgroups per CU), 1.5 x ones
    4-tile strips — except large launches of them (1440p -> 4K x 32), which take the WIDE 8-tile strips (LzMfma8uw, rows of up to 256 B) —
    within 15 % of the best measured shape everywhere, 4 % on average; and the planner says which kernel it planned for."""
    regrets = []
    for n in (32, 8, 1, 64, 128):
        for fmt, sw, sh, dw, dh, nn, res in sweep_lines(f"r05_lanczos_shape_sweep_up_n{n}.txt"):
            if fmt == "RGB" and nn > 32 and 3 * (sw * sh + dw * dh) > 7_000_000:
                continue   # (frames of that size are dispatched 32 at a time by the ABI: not a launch of nn frames)
            p = plan(lzp, planes_of(fmt, sw, sh, dw, dh), nn)
            assert p["ok"] and p["up2"], (fmt, sw, dw, nn, p)
            regrets.append(pick_time(p, res) / min(res.values()) - 1.0)
            assert regrets[-1] <= 0.15, (fmt, sw, dw, nn, p, min(res.values()))
    assert len(regrets) == 86 and float(np.mean(regrets)) <= 0.04, (len(regrets), np.mean(regrets))
    # which candidates are the ring of two: 2 x -> both strip widths; 1.5 x packed RGB -> the 4-tile strips only; down-scales, and the knob -> none
    assert plan(lzp, planes_of("RGB", 1920, 1080, 3840, 2160), 32)["nt"] == 8
    assert plan(lzp, planes_of("RGB", 1280, 720, 1920, 1080), 32)["nt"] == 4
    assert plan(lzp, planes_of("RGB", 1280, 720, 1920, 1080), 32, forced=8 << 8)["up2"] is False   # (wide 8-tile strips: large launches only)
    big = plan(lzp, planes_of("RGB", 2560, 1440, 3840, 2160), 32)
    assert big["nt"] == 8 and big["up2"] and 128 < big["span"] <= 256
    assert plan(lzp, planes_of("RGB", 2560, 1440, 3840, 2160), 8)["nt"] == 4
    assert plan(lzp, planes_of("RGB", 1280, 720, 1920, 1080), 32, forced=4 << 8)["up2"] is True
    assert plan(lzp, planes_of("RGB", 1920, 1080, 1280, 720), 32)["up2"] is False
    assert plan(lzp, planes_of("RGB", 1920, 1080, 3840, 2160), 32, up2=False)["up2"] is False
    assert plan(lzp, [(3, 1920, 1080, 3840, 1000)], 32)["up2"] is False   # (an up-scale in x only)


def test_planner_on_one_up_scaled_frame_per_dispatch(lzp):
    """Round 6: ONE frame per dispatch (an unmodified PySurfaceResizer.Execute()).  A lone launch is one round of waves and its time is that of the
    fullest CU, so the best band height sits just under a multiple of 256 workgroups; for the ring-of-two kernels (up-scales) on launches whose
    planes have equal strip counts (RGB, Y, NV12) the planner keeps its strip width and re-chooses the band height with an occupancy term fitted to
    the n = 1 sweep (tools/lab/fit_lzm_lone.py): 20 cases, mean regret <= 2.5 %, worst <= 9 % (before: 3.2 % / 13 %); the picks it changes were
    measured band height by band height (profiles/r06_m_lone_upscales.txt).  YUV420 (the first form of the rule lost 9-14 % there), down-scales,
    forced band heights and launches of more than one frame are untouched."""
    regrets = []
    for fmt, sw, sh, dw, dh, nn, res in sweep_lines("r05_lanczos_shape_sweep_up_n1.txt"):
        assert nn == 1
        p = plan(lzp, planes_of(fmt, sw, sh, dw, dh), 1)
        assert p["ok"] and p["up2"] and 2 <= p["r"] <= 64
        regrets.append(pick_time(p, res) / min(res.values()) - 1.0)
        assert regrets[-1] <= 0.09, (fmt, sw, dw, p, min(res.values()))
    assert len(regrets) == 20 and float(np.mean(regrets)) <= 0.025, (len(regrets), np.mean(regrets))
    # the case that motivated it: bands that fill whole multiples of the 256 CUs
    assert plan(lzp, planes_of("RGB", 1920, 1080, 3840, 2160), 1)["r"] == 8      # 45 x 17 = 765 workgroups = 3 per CU (7 tiles: 900; 6: a second round)
    # untouched: a forced band height; launches of more than one frame: the sweep tests above and below (the ring of four at n = 1: the next test)
    assert plan(lzp, planes_of("RGB", 1920, 1080, 3840, 2160), 1, forced=(4 << 8) | 5)["r"] == 5
    assert plan(lzp, planes_of("NV12", 2560, 1440, 3840, 2160), 1)["r"] == 4 and plan(lzp, planes_of("YUV420", 1920, 1080, 3840, 2160), 1)["r"] == 4   # (YUV420: the model's own pick)


def lone_sweep_lines(name):
    """tools/lab/ab/lone_lanczos.py files: one frame per dispatch, knob (nt << 8 | band tiles) -> us; knob 0 (policy) left out"""
    cur, out = None, {}
    for line in open(os.path.join(ROOT, "profiles", name)):
        m = re.match(r"\[lone\] \S+\s+(\w+)\s+(\d+)x(\d+)->(\d+)x(\d+)", line)
        if m:
            cur = (m.group(1),) + tuple(int(v) for v in m.groups()[1:])
            out[cur] = {}
            continue
        m = re.match(r"\[lone\]\s+(0x[0-9a-f]+): ([\d.]+) us", line)
        if m and int(m.group(1), 16):
            out[cur][(int(m.group(1), 16) >> 8, int(m.group(1), 16) & 255)] = float(m.group(2))
    return out


def test_planner_on_one_down_scaled_frame_per_dispatch(lzp):
    """Round 6, the ring of four at n = 1: where the launch fills the chip (more than 384 workgroups as first picked) strip width and band height are
    re-chosen by a model with a ring-fill term, fitted to two boxes' sweeps and cross-validated between them (tools/lab/fit_lzm_lone.py).  Against
    the round-5 sweep (16 cases): mean regret <= 1.5 %, worst <= 7 % (before: 2.8 % / 18 %); against the final tree's own sweep of the 4K cases
    (profiles/r06_p_lone_downscales.txt, every band height measured, 7 cases): mean <= 3.5 %, worst <= 13 % (before: 7.7 % / 21 %)."""
    regrets = []
    for fmt, sw, sh, dw, dh, nn, res in sweep_lines("r05_lanczos_shape_sweep_down_n1.txt"):
        p = plan(lzp, planes_of(fmt, sw, sh, dw, dh), 1)
        assert p["ok"] and not p["up2"] and p["kc"] == 1
        regrets.append(pick_time(p, res) / min(res.values()) - 1.0)
        assert regrets[-1] <= 0.07, (fmt, sw, dw, p, min(res.values()))
    assert len(regrets) == 16 and float(np.mean(regrets)) <= 0.015, np.mean(regrets)
    regrets = []
    for (fmt, sw, sh, dw, dh), res in lone_sweep_lines("r06_p_lone_downscales.txt").items():
        if fmt == "Y" and dw == 1920:
            continue   # (one such plane per dispatch goes to the tile kernel by policy: resize_plan, not this planner)
        p = plan(lzp, planes_of(fmt, sw, sh, dw, dh), 1)
        regrets.append(res[(p["nt"], p["r"])] / min(res.values()) - 1.0)   # (the pick itself was measured)
        assert regrets[-1] <= 0.13, (fmt, sw, dw, p)
    assert len(regrets) == 7 and float(np.mean(regrets)) <= 0.035, np.mean(regrets)
    rgb = plan(lzp, planes_of("RGB", 3840, 2160, 1920, 1080), 1)
    assert (rgb["nt"], rgb["r"]) == (4, 4) and rgb["group_lds"] <= 80 * 1024 and rgb["span"] <= 256   # 23 x 17 = 391 workgroups: 14.2 us against 15.2
    assert plan(lzp, planes_of("YUV420", 1920, 1080, 1600, 900), 1)["r"] == 2      # 323 workgroups: below the gate, the pick stands (6.9 us; bands of 3: 7.6)
    # untouched: any forced shape, launches without tables, more than one frame
    assert plan(lzp, planes_of("RGB", 3840, 2160, 1920, 1080), 1, forced=8 << 8)["nt"] == 8
    assert (plan(lzp, planes_of("RGB", 3840, 2160, 1920, 1080), 1, tables=False)["nt"], plan(lzp, planes_of("RGB", 3840, 2160, 1920, 1080), 2)["nt"]) == (8, 8)


@pytest.mark.parametrize("n,mean_max,worst_max", [(64, 0.06, 0.15), (128, 0.05, 0.15)])
def test_planner_beyond_32_frames_per_dispatch(lzp, n, mean_max, worst_max):
    """Round 5 (up to 128 frames per dispatch): the cost model's large-launch branch (continuous rounds + a tail of one and a half wave lives)
    against the sweeps at 64 and 128 frames (RGB / NV12 / YUV420 / Y x three size pairs each): the pick within 15 % of the best measured
    shape, 5-6 % on average — the round-3 model, asked about such launches, put NV12 and Y 1080p -> 720p on whole-column 4-tile strips
    (46 % / 27 % off the best)."""
    regrets = []
    for fmt, sw, sh, dw, dh, nn, res in sweep_lines(f"r05_lanczos_shape_sweep_n{n}.txt"):
        if sw < dw:
            continue   # (the up-scale lines were measured with the kernels the ring of two replaced: test_planner_on_up_scales)
        p = plan(lzp, planes_of(fmt, sw, sh, dw, dh), nn)
        assert p["ok"] and nn == n
        rs = sorted(r for (nt, r) in res if nt == p["nt"])
        lo = max([r for r in rs if r <= p["r"]], default=rs[0])
        hi = min([r for r in rs if r >= p["r"]], default=rs[-1])
        t = res[(p["nt"], lo)] if lo == hi else np.interp(p["r"], [lo, hi], [res[(p["nt"], lo)], res[(p["nt"], hi)]])
        regrets.append(t / min(res.values()) - 1.0)
        assert regrets[-1] <= worst_max, (fmt, sw, dw, p, t, min(res.values()))
    assert len(regrets) == 8 and float(np.mean(regrets)) <= mean_max, np.mean(regrets)


def test_planner_limits_and_forced_shapes(lzp):
    """What the launcher relies on: the LDS of a workgroup never exceeds 80 KB, the staged row fits the variant's loads, a forced shape is
    honoured when it fits, and shapes outside the kernel's windows are refused (the gather kernel takes them)."""
    rng = np.random.default_rng(5)
    n_ok = n_no = 0
    for _ in range(400):
        ch = int(rng.choice([1, 2, 3]))
        sw, sh = int(rng.integers(16, 4000)), int(rng.integers(8, 2200))
        dw, dh = max(2, int(sw / rng.uniform(0.3, 14.0))), max(2, int(sh / rng.uniform(0.3, 9.0)))   # (refused: beyond ~10 across / ~6 down)
        p = plan(lzp, [(ch, sw, sh, dw, dh)], int(rng.choice([1, 4, 32])))
        if not p["ok"]:
            n_no += 1
            continue
        n_ok += 1
        assert (p["kc"], p["nt"]) in ((1, 8), (1, 4), (2, 4), (3, 2))
        assert p["group_lds"] <= 80 * 1024 and p["span"] <= (8 if p["kc"] >= 2 else 5 if p["nt"] == 8 else 4) * 64 and p["pitch"] >= p["span"] and p["pitch"] % 64 == 32
        if p["kc"] >= 2:  # multi-chunk windows are the fallbacks: no cheaper shape holds this plane's taps
            assert p["pitch"] in (288, 416, 544)
        assert p["group_lds"] == 4 * p["wave_lds"] + 16384 and p["wave_lds"] >= 16 * p["pitch"] + 16 * (16 * p["nt"] + 16)
        assert p["rts"] in (3, 4) and 1 <= p["r"] <= (dh + (1 << p["rts"]) - 1) >> p["rts"]
    assert n_ok > 150 and n_no > 30
    base = [(3, 1920, 1080, 1280, 720)]
    assert plan(lzp, base, 32, (8 << 8) | 5)["r"] == 5 and plan(lzp, base, 32, (8 << 8) | 5)["nt"] == 8
    assert plan(lzp, base, 32, (4 << 8) | 64)["r"] == 45 and plan(lzp, base, 32, (4 << 8))["nt"] == 4   # more tiles than the picture has: one band
    assert plan(lzp, base, 32, 7)["r"] == 7
    net = plan(lzp, [(3, 1920, 1080, 416, 416)], 32)                            # 4.6 x 2.6: the taps of 16 destination bytes do not fit a 64-B window,
    assert net["ok"] and net["kc"] == 2 and net["nt"] == 4 and net["span"] <= 384   # they fit a 128-B one: pass 1 with two K chunks
    assert plan(lzp, base, 32)["kc"] == 1
    res = plan(lzp, [(1, 1920, 1080, 224, 224), (1, 960, 540, 112, 112), (1, 960, 540, 112, 112)], 32)   # the reference's sample: YUV420 1080p -> 224 x 224,
    assert res["ok"] and res["kc"] == 3 and res["nt"] == 2 and res["rts"] == 3 and res["span"] <= 384       # 8.6 x 4.8: 192-B windows, 2-tile strips, half tiles
    assert not plan(lzp, [(3, 1920, 1080, 224, 224)], 32)["ok"] and plan(lzp, [(3, 1920, 1080, 224, 224)], 32, (4 << 8) | 2)["kc"] == 3   # packed RGB: by force only (the tile kernel is faster)
    assert plan(lzp, [(1, 3840, 2160, 416, 416), (2, 1920, 1080, 208, 208)], 32)["kc"] == 3
    assert not plan(lzp, [(3, 1920, 1080, 120, 120)], 32)["ok"]                 # 16 x 9: out of every window
    thumb = plan(lzp, [(3, 1920, 1080, 480, 270)], 32)                          # 4 x 4: a 16-row tile needs more than four source tiles, 8 rows do not
    assert thumb["ok"] and thumb["rts"] == 3 and thumb["kc"] == 2 and plan(lzp, base, 32)["rts"] == 4
    assert plan(lzp, [(1, 1280, 720, 224, 224), (1, 640, 360, 112, 112), (1, 640, 360, 112, 112)], 32)["rts"] == 3   # YUV420 720p -> 224 x 224 (5.7 x 3.2)
    assert not plan(lzp, base + [(1, 1920, 1080, 120, 120)], 32)["ok"]          # one plane out -> the launch is out
    mixed = plan(lzp, [(1, 1920, 1080, 640, 480), (2, 960, 540, 320, 240)], 8)  # NV12 3 x 2.25: both planes on two-chunk windows
    assert mixed["ok"] and mixed["kc"] == 2
    with_t, without = plan(lzp, base, 1, 0, True), plan(lzp, base, 1, 0, False)
    assert without["r"] >= with_t["r"]                                          # a bigger fixed cost per wave never asks for shorter bands


B = 0x80000000


def _log(L, c):
    buf = C.create_string_buffer(1 << 16)
    L.lzp_sync_log(c, buf, len(buf))
    return buf.value.decode().split()


def test_table_cache_contract(lzp):
    """the fallback arena (vpf_lzm_plan.h: LzmTableCache) against a recording stand-in for HIP events: what makes "a launch never reads a table
    whose build it is not ordered behind" and "a table is never overwritten under a kernel that may still read it" true"""
    c = lzp.lzp_cache_new(1 << 20)
    try:
        go = lambda st, dev=0, cap=0, kind=0, k=(3, 1920, 1280, 8), nbytes=100_000: lzp.lzp_cache_launch(c, st, dev, cap, kind, *k, nbytes)
        a = go(0x1000)
        assert a & B and (a & ~B) == 16                      # first use: allocated after the 256 unused bytes, build on this stream
        assert _log(lzp, c) == ["R1@4096d0"]                 # an event behind the build; the launch itself costs no HIP call (the entry remembers its stream)
        assert go(0x1000) == 16                              # same stream again: ordered behind its own build by the stream itself
        assert _log(lzp, c) == []
        assert go(0x2000) == 16                              # another stream: no second build — it WAITS for the build's event
        assert _log(lzp, c) == ["W1@8192"]
        lzp.lzp_sync_complete(c, 1)                          # the build is seen complete once ...
        assert go(0x3000) == 16 and _log(lzp, c) == []       # ... and nobody waits for it again
        assert go(0x2000) == 16 and go(0x1000) == 16
        _log(lzp, c)
        # a capturing stream always queues its own build (a captured build has not run), records nothing (an event recorded there would
        # become a node of the graph), and pins the entry: a graph captured with it replays whenever it likes
        assert go(0x1000, cap=1) == (16 | B) and go(0x1000, cap=1) == (16 | B) and _log(lzp, c) == []
        fresh = go(0x3000, cap=1, k=(1, 640, 320, 4), nbytes=5000)
        assert fresh & B and go(0x3000, k=(1, 640, 320, 4), nbytes=5000) & B   # first met under capture: its build never ran — the plain call builds
        b = go(0x1000, kind=1, k=(1080, 720, 368, 0), nbytes=24_576)
        assert b & B and (b & ~B) == 16 + (100_000 + 255) // 256 * 16 + (5000 + 255) // 256 * 16   # first fit in 256-B steps
        assert go(0x1000, dev=1) == (16 | B)                 # arenas are per device
        used = lzp.lzp_cache_used(c, 0)
        assert go(0x1000, k=(3, 9999, 9999, 8), nbytes=(1 << 20) + 1) == 0      # larger than the arena: no table, no build (the kernel evaluates its weights)
        assert lzp.lzp_cache_used(c, 0) == used               # ... and nothing was taken or evicted for it
        assert go(0x1000, dev=64) == 0 and go(0x1000, dev=-1) == 0
    finally:
        lzp.lzp_cache_free(c)
    z = lzp.lzp_cache_new(0)                                   # VPF_HIP_LANCZOS_TABLE_KB=0
    assert lzp.lzp_cache_launch(z, 1, 0, 0, 0, 3, 1920, 1280, 8, 1000) == 0
    lzp.lzp_cache_free(z)


def test_table_cache_evicts_least_recently_used_behind_its_last_use(lzp):
    """a full arena hands the least recently used entry's space to the new shape — after making the BUILDING stream wait for the event the
    last launch left on that entry (unless that launch is known to have finished) — and never an entry of the launch in progress"""
    c = lzp.lzp_cache_new(256 + 3 * 4096)                      # room for three 4-KiB tables
    try:
        go = lambda st, k, nbytes=4096: lzp.lzp_cache_launch(c, st, 0, 0, 0, k, 1, 1, 8, nbytes)
        offs = [go(0x10, k) & ~B for k in (1, 2, 3)]
        assert offs == [16, 16 + 256, 16 + 512] and lzp.lzp_cache_entries(c, 0) == 3
        go(0x10, 1)                                            # shape 1 is used again: shape 2 is now the oldest
        _log(lzp, c)                                           # (events so far: the three builds = 1, 2, 3)
        d = go(0x20, 4)                                        # a fourth shape, from another stream
        assert d == (offs[1] | B)                              # it took shape 2's place
        lg = _log(lzp, c)
        # stream 0x20 waits for an event recorded just now on the stream that used shape 2 (= behind its last launch) AND for its build
        assert lg[0] == "R4@16d0" and lg[1] == "W4@32" and "W2@32" in lg
        assert go(0x10, 2) & B                                 # shape 2 is gone: it is built again (evicting the oldest: shape 3)
        assert lzp.lzp_cache_entries(c, 0) == 3
        lzp.lzp_sync_complete(c, lzp.lzp_sync_next(c))         # everything queued so far has finished:
        _log(lzp, c)
        lg = _log(lzp, c) if go(0x30, 5) & B else None
        builds_waited = [x for x in lg if x.startswith("W") and int(x[1:].split("@")[0]) <= 6]
        assert lg is not None and not builds_waited           # an eviction then waits for no build any more (only for its readers' streams)
        # an entry that has met more streams than it remembers gets one event per launch instead
        for st in (0x41, 0x42, 0x43, 0x44):
            go(st, 5)
        _log(lzp, c)
        go(0x45, 5)
        assert [x for x in _log(lzp, c) if x.startswith("R") and "@69d0" in x]
        # two tables of ONE launch never evict each other: with room for three, a launch that needs two new ones keeps both
        out = (C.c_uint32 * 2)()
        ka, kb = (C.c_uint32 * 5)(0, 77, 1, 1, 8), (C.c_uint32 * 5)(1, 77, 1, 1, 0)
        lzp.lzp_cache_launch2(c, 0x10, 0, ka, 4096, kb, 4096, out)
        assert out[0] & B and out[1] & B and (out[0] & ~B) != (out[1] & ~B)
        big = (C.c_uint32 * 5)(0, 78, 1, 1, 8)
        lzp.lzp_cache_launch2(c, 0x10, 0, kb, 4096, big, 2 * 4096 + 1, out)     # kb's table is in use by this launch: it may not make room for the big one ...
        assert out[0] == (out[0] & ~B) and out[0] != 0 and out[1] == 0           # ... it is still there, untouched; the big one gets no table (weights in the kernel)
        # 10 000 distinct shapes through an arena that holds three: every one of them gets a table (the arena never "fills up for good")
        for k in range(1000, 11000):
            assert go(0x10, k) & B
        assert lzp.lzp_cache_entries(c, 0) <= 3
        # a device reset: the host forgets the device's tables (static device memory is re-initialised) — the next launch builds again
        last = go(0x10, 10999)
        assert last == (last & ~B)
        lzp.lzp_sync_reset_device(c, 0)
        assert go(0x10, 10999) & B and lzp.lzp_cache_entries(c, 0) == 1
    finally:
        live_before = lzp.lzp_sync_live(c)
        lzp.lzp_cache_free(c)
    assert live_before <= 2 * 3 + 1                            # events are released as entries go: no leak over 10 000 evictions


def test_table_cache_eviction_leaves_foreign_streams_alone_when_it_must(lzp):
    """the streams an entry remembers are somebody else's handles from earlier launches.  At eviction a reader stream that is under
    capture is not recorded on (the record would become a node of that graph): its entry is not a victim for this launch; a handle the
    runtime no longer knows (destroyed stream) is dropped without a record"""
    c = lzp.lzp_cache_new(256 + 2 * 4096)                      # room for two 4-KiB tables
    try:
        go = lambda st, k: lzp.lzp_cache_launch(c, st, 0, 0, 0, k, 1, 1, 8, 4096)
        a, b = go(0x10, 1) & ~B, go(0x20, 2) & ~B              # shape 1 read on stream 0x10 (the older entry), shape 2 on 0x20
        _log(lzp, c)
        lzp.lzp_sync_stream_states(c, 0x10, 0)                 # stream 0x10 has begun a capture since
        d = go(0x30, 3)
        lg = _log(lzp, c)
        assert d == (b | B)                                    # the older entry is left alone: shape 2's place is taken instead ...
        assert not [x for x in lg if x.startswith("R") and "@16d" in x]   # ... and nothing was recorded on the capturing stream
        assert go(0x10, 1) == a                                # shape 1 is still there
        lzp.lzp_sync_stream_states(c, 0, 0x10)                 # capture over, and stream 0x10 has been destroyed
        go(0x30, 3)                                            # (shape 3 is now the most recent: shape 1 is the victim)
        _log(lzp, c)
        e = go(0x40, 4)
        lg = _log(lzp, c)
        assert e == (a | B) and not [x for x in lg if x.startswith("R") and "@16d" in x]   # no record on a handle that names no stream
        # both entries read by capturing streams: no victim — the launch gets no table (weights in the kernel) instead of a wrong one
        lzp.lzp_sync_stream_states(c, 0x30, 0)
        go(0x30, 4)                                            # both live entries (3, 4) have 0x30 among their readers
        assert go(0x50, 5) == 0 and lzp.lzp_cache_entries(c, 0) == 2
        lzp.lzp_sync_stream_states(c, 0, 0)
        assert go(0x50, 5) & B
    finally:
        lzp.lzp_cache_free(c)


def test_workspace_record(lzp):
    """the caller-owned workspace (vpf_workspace.opaque = LzmWorkspace): stream-ordered, no events.  Same shape on the same stream -> no
    rebuild; another stream / a capturing stream / a new shape -> rebuild; no room -> everything is dropped and the region reused from its
    start, except that the entries of the launch in progress are never dropped (the fallback arena serves that table instead)"""
    ws = (C.c_uint64 * 40)()
    region = 256 + 3 * 4096

    def get(st, k, nbytes=4096, cap=0, dev=0, kind=0, launch=None):
        """one lookup; `launch` = the mask of a launch in progress (a fresh one per call otherwise: every lookup its own launch)"""
        m = launch if launch is not None else C.c_uint32(0)
        return lzp.lzp_ws_get(ws, region, st, dev, cap, kind, k, 1, 1, 8, nbytes, C.byref(m))

    assert get(0x10, 1) == (16 | B) and get(0x10, 1) == 16 and get(0x10, 1, kind=1) == ((16 + 256) | B)
    assert get(0x10, 1, cap=1) == (16 | B)                     # captured: build again
    assert get(0x20, 1) == (16 | B) and lzp.lzp_ws_n(ws) == 1  # another stream: nothing in the region is ordered for it — it starts over
    assert get(0x20, 2) & B and get(0x20, 3) & B and lzp.lzp_ws_n(ws) == 3
    assert get(0x20, 4) == (16 | B) and lzp.lzp_ws_n(ws) == 1  # full: reuse from the start (stream order keeps the old readers in front)
    m = C.c_uint32(0)
    assert get(0x20, 5, launch=m) & B and get(0x20, 6, launch=m) & B and m.value == 0b110
    assert get(0x20, 7, launch=m) == 0                         # full AND the entries in it belong to this very launch: not here
    assert get(0x20, 8, nbytes=region) == 0                    # larger than the region: never
    # a launch that HIT an old entry and then misses on a full record must not be handed the hit table's bytes a second time
    m = C.c_uint32(0)
    assert get(0x20, 4, launch=m) == 16 and m.value == 1       # hit: the first entry, at offset 16
    assert get(0x20, 9, launch=m) == 0 and lzp.lzp_ws_n(ws) == 3  # miss on the full record: the fallback arena, nothing dropped
    assert get(0x20, 4, launch=m) == 16 and get(0x20, 5, launch=m) == 16 + 256  # ... and the tables it was given are still there
    assert get(0x20, 9) == (16 | B) and lzp.lzp_ws_n(ws) == 1  # the NEXT launch may start over
    # the same with the entry count as the limit (eight small tables) instead of the bytes
    ws2, m = (C.c_uint64 * 40)(), C.c_uint32(0)
    g2 = lambda k, launch: lzp.lzp_ws_get(ws2, 1 << 20, 0x30, 0, 0, 0, k, 1, 1, 8, 256, C.byref(launch))
    offs = [g2(k, C.c_uint32(0)) & ~B for k in range(8)]
    assert len(set(offs)) == 8 and lzp.lzp_ws_n(ws2) == 8
    assert g2(3, m) == offs[3] and g2(100, m) == 0 and lzp.lzp_ws_n(ws2) == 8 and g2(3, m) == offs[3]
    assert get(0x20, 1, dev=1) == (16 | B)                     # another device: a fresh record


def test_workspace_bound_covers_every_plan(lzp):
    """vpf_resize_workspace_bytes adds lzm_table_bytes_bound over the planes: it must cover what ANY launch shape the planner can pick needs
    (column tables: strips x nt x 2 KiB; row tables: bands x groups per band x 8 KiB)"""
    rng = np.random.default_rng(3)
    for _ in range(300):
        ch = int(rng.choice([1, 2, 3]))
        dw, dh = int(rng.integers(2, 4000)), int(rng.integers(2, 2200))
        bound = lzp.lzp_table_bytes_bound(ch, dw, dh)
        for nt in (4, 8):
            strips = (dw * ch + 16 * nt - 1) // (16 * nt)
            for tiles in (1, 2, 3, 5, 8, 23, 64):
                tiles = min(tiles, (dh + 15) // 16)  # (the planner never asks for more tiles per band than the picture has)
                rows = 16 * tiles
                need = (strips * nt * 2048 + 255) // 256 * 256 + (((dh + rows - 1) // rows) * ((rows + 63) // 64) * 8192 + 255) // 256 * 256
                assert need <= bound, (ch, dw, dh, nt, tiles)
    # ... and what the launch REALLY asks for (lzm_launch's own table requests: x K chunks, half tiles included), per plane, over the seeded sweep
    worst, frames_seen = 0.0, set()
    for planes, n, knob, pair_build, d in launch_sweep(lzp):
        for (ch, _, _, dw, dh), q in zip(planes, d["plane"]):
            need = sum((q[t]["bytes"] + 255) // 256 * 256 for t in ("ctab", "rtab"))
            bound = lzp.lzp_table_bytes_bound(ch, dw, dh)
            assert need <= bound, (planes, n, hex(knob), need, bound)
            worst = max(worst, need / bound)
        frames_seen.add(n)
    assert frames_seen == {1, 2, 8, 32, 33, 128} and 0.5 < worst <= 1.0, (frames_seen, worst)   # (the sweep comes close to the bound)


_SWEEP = []


def launch_sweep(L):
    """[(planes, frames, VPF_TUNE_RESIZE_MFMA, pair form in the build, lzm_launch's answer)] of every call of a seeded sweep that the launcher takes: sizes
    2 .. 4096, one plane of 1 - 3 channels or the planes of NV12 / YUV420, factors from 3 x up to 10 x down on each axis, forced shapes, tables off, no ring
    of two, the lab build's pair form; 1, 2, 8, 32, 33 and 128 frames.  Computed once for the tests below."""
    if _SWEEP:
        return _SWEEP
    rng = np.random.default_rng(21)
    sizes = [2, 16, 61, 64, 224, 256, 416, 640, 720, 1080, 1280, 1920, 2160, 3840, 4096]
    knobs = [0, 0, 0, 0x10000, 0x80000, 8 << 8, 4 << 8, (4 << 8) | 2, (8 << 8) | 5, 7, (8 << 8) | 0x10000, (4 << 8) | 0x80000, 0x20000, 0x20003]
    refused = {}
    for _ in range(9000):
        pick = lambda: int(rng.choice(sizes)) if rng.random() < 0.4 else int(rng.integers(2, 4097))   # noqa: E731
        dw, dh = pick(), pick()
        sw, sh = (min(4096, max(2, int(d * f))) for d, f in zip((dw, dh), np.exp(rng.uniform(np.log(0.33), np.log([10.5, 6.5])))))
        kind = int(rng.integers(5))
        planes = [(kind + 1, sw, sh, dw, dh)] if kind < 3 else [(1, sw, sh, dw, dh), (2, (sw + 1) // 2, (sh + 1) // 2, (dw + 1) // 2, (dh + 1) // 2)] if kind == 3 else \
            [(1, sw, sh, dw, dh)] + [(1, (sw + 1) // 2, (sh + 1) // 2, (dw + 1) // 2, (dh + 1) // 2)] * 2
        n, knob, pair_build = int(rng.choice([1, 2, 8, 32, 33, 128])), int(rng.choice(knobs)), bool(rng.random() < 0.5)
        d = launch(L, planes, n, knob=knob, pair_build=pair_build)
        if d["why"] == OK:
            _SWEEP.append((planes, n, knob, pair_build, d))
        refused[d["why"]] = refused.get(d["why"], 0) + 1
    assert len(_SWEEP) > 4000 and set(refused) == {OK, NO_ROWS, NO_PLAN, NO_PAIR_HALF_TILES}, (len(_SWEEP), refused)
    return _SWEEP


def test_form_table(lzp):
    """the sixteen forms (thirteen in the product build) by name, and lzm_form_of as the one map from a planned shape to a form: every row is reached by
    its own (nt, kc, span, up2, pair) at both ends of the spans its staging loads cover, and by nothing else"""
    names = [form(lzp, f)["name"] for f in range(lzp.lzp_forms())]
    assert names == ["LzMfma8", "LzMfma8n", "LzMfma8w", "LzMfma4", "LzMfma4n", "LzMfma8u", "LzMfma4u", "LzMfma8uw", "LzMfma4k4", "LzMfma4k6", "LzMfma4k8", "LzMfma2k6",
                     "LzMfma2k8", "LzPair", "LzPairN", "LzPairW"] and lzp.lzp_product_forms() == 13
    spans = {1: {2: (16, 128), 4: (129, 256), 5: (257, 320)}, 2: {4: (16, 256), 6: (257, 384), 8: (385, 512)}, 3: {6: (16, 384), 8: (385, 512)}}   # lzm_pf_of
    rows = set()
    for f in range(lzp.lzp_forms()):
        i = form(lzp, f)
        assert i["pair"] == (f >= 13) and not (i["pair"] and i["up2"]) and i["max_lds"] <= 80 * 1024, i
        for span in spans[i["kc"]][i["pf"]]:
            assert lzp.lzp_form_of(i["nt"], i["kc"], span, i["up2"], i["pair"]) == f, (i, span)
        rows.add((i["nt"], i["pf"], i["kc"], i["up2"], i["pair"]))
    assert len(rows) == lzp.lzp_forms()   # no two rows answer the same question
    assert lzp.lzp_form_of(4, 1, 300, 0, 0) == lzp.lzp_forms() and lzp.lzp_form_of(2, 1, 64, 0, 0) == lzp.lzp_forms() and lzp.lzp_form_of(8, 2, 64, 0, 0) == lzp.lzp_forms()
    # no form needs the LDS attribute today: the largest workgroup is LzMfma4k8's (a form that grows past 64 KiB gets it set at the dispatch)
    assert max(form(lzp, f)["max_lds"] for f in range(lzp.lzp_forms())) == form(lzp, names.index("LzMfma4k8"))["max_lds"] == 56320


def test_launch_refusals(lzp):
    """the refusals in the launcher's order: knobs, counts, then per plane size, alignment, the 24- / 32-bit offset limits, the ring's vertical reach; then
    the planner, then the pair form's whole tiles"""
    base, al = [(3, 1920, 1080, 1280, 720)], ALIGNED
    why = lambda planes=base, n=2, frames=None, **kw: launch(lzp, planes, n, frames=frames, **kw)["why"]   # noqa: E731
    assert why() == OK
    assert (why(tune=9), why(tune=40), why(knob=1), why(knob=0x10001), why(tune=43)) == (NO_SWITCHED_OFF,) * 4 + (OK,)
    assert (why(n=0), why(n=129), why(n=128), why(njobs=0), why(njobs=4)) == (NO_COUNTS, NO_COUNTS, OK, NO_COUNTS, NO_COUNTS)
    assert why(n=0, knob=1) == NO_SWITCHED_OFF and why([(3, 1 << 22, 1080, 1280, 720)], n=0) == NO_COUNTS   # (the order)
    for i in range(1, 5):
        big = list(base[0])
        big[i] = 1 << 22
        assert why([tuple(big)], frames=[(al[0] | 8, 256, 256)]) == NO_SIZE
    assert why(frames=[(al[0] | 8, 256, 256)]) == NO_ALIGNMENT and why(frames=[(al[0] | 16, 256, 256)]) == OK
    assert why(frames=[(al[0] | 8, 1 << 24, 256)]) == NO_ALIGNMENT   # (alignment is asked before the pitch)
    low = [(3, 192, 108, 128, 72)]   # (few rows: the 24-bit limit alone)
    assert (why(low, frames=[(al[0], 1 << 24, 256)]), why(low, frames=[(al[0], 256, 1 << 24)]), why(low, frames=[(al[0], (1 << 24) - 16, (1 << 24) - 16)])) == (NO_PITCH, NO_PITCH, OK)
    tall = [(1, 64, 4096, 64, 4000)]   # sh x sp and dh x dp against 2^32
    assert why(tall, frames=[(al[0], 1 << 20, 256)]) == NO_PITCH and why(tall, frames=[(al[0], (1 << 20) - 16, 256)]) == OK
    assert why(tall, frames=[(al[0], 256, (1 << 32) // 4000 // 16 * 16 + 16)]) == NO_PITCH and why(tall, frames=[(al[0], 256, (1 << 32) // 4000 // 16 * 16)]) == OK
    assert why(base + [(1, 1920, 1080, 1280, 720)], frames=[al, (al[0] | 4, 256, 256)]) == NO_ALIGNMENT   # (any plane)
    assert why([(3, 1920, 1080, 120, 120)]) == NO_ROWS and why(frames=[(al[0], 1 << 24, 256)], planes=[(3, 1920, 1080, 120, 120)]) == NO_PITCH
    assert why([(3, 1920, 1080, 224, 400)]) == NO_PLAN   # packed RGB beyond the two-chunk windows: by force only
    assert why([(3, 1920, 1080, 960, 270)], knob=0x20000, pair_build=True) == NO_PAIR_HALF_TILES and why([(3, 1920, 1080, 960, 270)], knob=0x20000) == OK


def test_launch_invariants(lzp):
    """restated without the golden file, over the seeded sweep: the form is a function of the plan's (nt, kc, span, up2) and the pair bit alone, the grid covers
    every destination byte and row of every plane, the by0 are the running band sums, both LDS outcomes fit, the table requests are what the build kernels
    and the cache are keyed by"""
    forms_seen, builds_seen, rts_seen = set(), set(), set()
    for planes, n, knob, pair_build, d in launch_sweep(lzp):
        what = (planes, n, hex(knob), pair_build, d)
        pair = pair_build and bool(knob & 0x20000)
        forced = knob & 0xffff
        P = plan(lzp, planes, n, ((8 << 8) | (forced & 0xff)) if pair else forced, tables=not knob & 0x10000, up2=not pair and not knob & 0x80000)
        assert P["ok"] and d["form"] == lzp.lzp_form_of(P["nt"], P["kc"], P["span"], P["up2"], pair) and (bool(d["pair"]), bool(d["tables"])) == (pair, not knob & 0x10000), what
        f = form(lzp, d["form"])
        assert (f["nt"], f["kc"], f["up2"], f["pair"]) == (P["nt"], P["kc"], P["up2"], pair) and 64 * f["pf"] >= P["span"] and d["pitch"] == 64 * f["pf"] + 32 == P["pitch"], what
        assert d["form"] < (16 if pair_build else 13), what   # a form this build has: the dispatch can launch it, and set its LDS attribute
        forms_seen.add(f["name"])
        rts_seen.add(d["rts"])
        assert d["rts"] == P["rts"] and d["rows"] == P["r"] << P["rts"] and d["gz"] == n and bool(d["up2"]) == P["up2"], what
        by0 = 0
        for (ch, sw, sh, dw, dh), q in zip(planes, d["plane"]):
            strips, bands = -(-dw * ch // (16 * f["nt"])), -(-dh // d["rows"])
            assert (2 if pair else 4) * d["gx"] >= strips and q["by0"] == by0, what   # a workgroup: four strips (the pair form: two)
            assert (q["sw"], q["sh"], q["dw"], q["dh"]) == (sw, sh, dw, dh) and (q["scx"], q["scy"]) == (fbits(sw, dw), fbits(sh, dh)), what
            by0 += bands
            c, r = q["ctab"], q["rtab"]
            groups = -(-d["rows"] // (4 << d["rts"]))   # groups of four tiles per band
            assert (c["kind"], c["k0"], c["k1"], c["k2"], c["k3"]) == (0, ch, sw, dw, f["nt"] | f["kc"] << 8) and (c["gx"], c["gy"]) == (strips, 1), what
            assert c["bytes"] == strips * f["nt"] * f["kc"] * 2048 and c["cols"] == {(8, 1): 0, (4, 2): 1, (2, 3): 2, (4, 1): 3}[(f["nt"], f["kc"])], what
            assert (r["kind"], r["k0"], r["k1"], r["k2"], r["k3"]) == (1, sh, dh, d["rows"], d["rts"] | int(P["up2"]) << 8) and (r["gx"], r["gy"]) == (groups, bands), what
            assert r["bytes"] == bands * groups * 8192, what
            builds_seen.add(c["cols"])
        assert d["gy"] == by0 and d["gx"] == max(-(-(-(-p[3] * p[0] // (16 * f["nt"]))) // (2 if pair else 4)) for p in planes), what
        # the two LDS outcomes
        run = 16 * d["pitch"] + 16 * (16 * f["nt"] + 16)
        assert d["lds_tabled"] <= d["lds"] <= 80 * 1024 and d["a2_tabled"] <= d["a2"] == P["wave_lds"] and d["lds"] <= f["max_lds"], what
        if pair:
            assert d["lds"] == d["lds_tabled"] == f["max_lds"] and d["a2"] == d["a2_tabled"], what
        else:
            assert d["lds"] == P["group_lds"] == 4 * d["a2"] + 16384 and d["lds_tabled"] == 4 * d["a2_tabled"] + 16384, what
            assert d["a2_tabled"] == (min(run, d["a2"]) if d["tables"] else d["a2"]) and d["a2"] >= run, what
    assert forms_seen >= {"LzMfma8", "LzMfma8n", "LzMfma8w", "LzMfma4", "LzMfma4n", "LzMfma8u", "LzMfma4u", "LzMfma4k4", "LzMfma4k6", "LzMfma4k8", "LzMfma2k6",
                          "LzPair", "LzPairN", "LzPairW"}, forms_seen   # (LzMfma8uw: behind the volume gate, below)
    # LzMfma2k8 (spans above 384 B on 2-tile strips) is planned for no shape: a tile's taps fit a 192-B window only where the second tile's window starts
    # less than 192 B behind the first (vpf_bound_lzm_span_win), so such a strip spans at most 384 B.  The form stays in the table and the dispatch
    assert "LzMfma2k8" not in forms_seen
    assert builds_seen == {0, 1, 2, 3} and rts_seen == {3, 4}
    wide = launch(lzp, [(3, 2560, 1440, 3840, 2160)], 32)
    assert form(lzp, wide["form"])["name"] == "LzMfma8uw"
    half = launch(lzp, [(1, 128, 128, 40, 16)], 2)   # the half-tile row of tests/cases_resize_families.py
    assert (form(lzp, half["form"])["name"], half["rts"], half["rows"]) == ("LzMfma4", 3, 16)


ARENA, WORKSPACE, STREAM = 0x7E00_0000_0000, 0x7D00_0000_0000, 0x5000   # the made-up addresses of the recording (the golden file's "layout")


def c_hexfloat(bits):
    """printf("%a") of the float with these bits"""
    m, e = float(np.uint32(bits).view(np.float32)).hex().split("p")
    return m.rstrip("0").rstrip(".") + "p" + e


def replay_launcher(L, row):
    """launch_lanczos_mfma (csrc/k_lanczos_mfma.hip) step by step on lzm_launch's answer: reduce the frame table, plan, hand out the tables — workspace first,
    then the arena, through the real LzmWorkspace / LzmTableCache with the recording stand-in for the events — queue the builds, pick the LDS outcome, dispatch
    -> (what the launcher returns, its selection label, its launches in the golden file's form)"""
    lab, tune, knob, mode, cap, n, njobs, jobs, mis, _, _, _ = row
    frames = []
    for ch, k, sw, _, dw, _ in jobs:
        bits = sp_max = dp_max = 0
        for i in range(n if n <= 128 else 0):
            on = not mis[4] or i + 1 == n
            sp, dp = (ch * sw + 255) // 256 * 256 + (mis[2] if on else 0), (ch * dw + 255) // 256 * 256 + (mis[3] if on else 0)
            bits |= (0x7F00_0000_0000 + (k << 36) + (i << 28) + (mis[0] if on else 0)) | sp | (0x7F80_0000_0000 + (k << 36) + (i << 28) + (mis[1] if on else 0)) | dp
            sp_max, dp_max = max(sp_max, sp), max(dp_max, dp)
        frames.append((bits, sp_max, dp_max))
    d = launch(L, [(j[0], j[2], j[3], j[4], j[5]) for j in jobs], n, tune, knob, bool(lab), frames, njobs)
    if d["why"] != OK:
        return 0, None, []
    f, out, ptrs = form(L, d["form"]), [], []
    cache = L.lzp_cache_new(0 if mode == 1 else 4 << 20)
    ws, touched, locked = (C.c_uint64 * 40)(), C.c_uint32(0), False
    try:
        for q in d["plane"] if d["tables"] else []:
            for t, r in enumerate((q["ctab"], q["rtab"])):
                key = [r[x] for x in ("kind", "k0", "k1", "k2", "k3")]
                h = L.lzp_ws_get(ws, {2: 64 << 20, 3: 256 + 8192, 4: 256 + 65536}[mode], STREAM, 0, cap, *key, r["bytes"], C.byref(touched)) if mode >= 2 else 0
                base = WORKSPACE
                if not h & ~B:
                    if not locked:
                        L.lzp_cache_begin(cache, 0)
                        locked = True
                    h, base = L.lzp_cache_get(cache, STREAM, 0, cap, (C.c_uint32 * 5)(*key), r["bytes"]), ARENA
                ptrs.append(base + 16 * (h & ~B) if h & ~B else 0)
                if h & B:
                    args = [r["k0"], q["sw"], q["dw"], c_hexfloat(q["scx"])] if t == 0 else [q["sh"], q["dh"], c_hexfloat(q["scy"]), d["rows"], d["rts"], d["up2"]]
                    out.append([("cols<%d, %d>" % ((8, 1), (4, 2), (2, 3), (4, 1))[r["cols"]]) if t == 0 else "rows", r["gx"], r["gy"], 1, 64, 0] + [str(a) for a in args] + ["p%x" % ptrs[-1]])
        ctab, rtab = (ptrs[0::2] + [0, 0, 0])[:3], (ptrs[1::2] + [0, 0, 0])[:3]
        if d["pair"] and not (ptrs and all(ptrs)):
            return 0, None, out   # the two-role form reads both tables
        tabled = bool(d["tables"]) and all(ctab[:len(jobs)])
        lds, a2 = (d["lds_tabled"], d["a2_tabled"]) if tabled else (d["lds"], d["a2"])
        table = [w for p in range(3) for w in (([d["plane"][p][x] for x in ("sw", "sh", "dw", "dh", "scx", "scy")] + [0, d["pitch"], d["rows"], a2, d["rts"]]) if p < len(jobs) else [0] * 11)]
        table += ([q["by0"] for q in d["plane"]] + [0, 0])[:3] + ([j[1] for j in jobs] + [0, 0])[:3] + ([j[0] for j in jobs] + [0, 0])[:3] + [len(jobs)]
        out.append(["%s/%d" % (f["name"], 32 if n <= 32 else 128), d["gx"], d["gy"], d["gz"], 256, lds, " ".join("%x" % w for w in table),
                    " ".join("%x %x" % (p & 0xffffffff, p >> 32) for p in ctab + rtab)])
        return 1, "k_lanczos_mfma<%s>" % f["name"], out
    finally:
        if locked:
            L.lzp_cache_end(cache, STREAM, 0, cap, 1)
        L.lzp_cache_free(cache)


def test_recorded_launches(lzp):
    """tests/golden/lzm_launch_kat.json: what launch_lanczos_mfma launched at the commit before its policy became lzm_launch (hash in the file), recorded without
    a device — every build launch and the main launch with grid, block, dynamic LDS and arguments, with tables on, off, a table budget of 0, and with a
    caller's workspace of three sizes; the refusals; the lab build's pair forms.  The launcher's sequence, restated above on the plan, leaves the same lines"""
    doc = json.load(open(os.path.join(ROOT, "tests", "golden", "lzm_launch_kat.json")))
    assert doc["columns"] == ["lab_build", "variant", "mfma", "mode", "capturing", "n", "njobs", "jobs", "misalignment", "ret", "label", "launches"]
    assert len(doc["parent_commit"]) == 40 and 150 <= len(doc["rows"]) <= 400
    labels, builds, outcomes = set(), set(), set()
    for row in doc["rows"]:
        got = replay_launcher(lzp, row)
        assert got == (row[9], row[10], row[11]), (row[:9], got, row[9:])
        labels.add(row[10])
        builds |= {l[0] for l in row[11][:-1]}
        outcomes.add((row[9], row[3], bool(row[2] & 0x10000), len(row[11]) > 1))
    assert labels == {None} | {"k_lanczos_mfma<%s>" % form(lzp, f)["name"] for f in range(16) if f != 12}, labels   # (LzMfma2k8: no shape reaches it)
    assert builds >= {"cols<8, 1>", "cols<4, 2>", "cols<2, 3>", "cols<4, 1>", "rows"}
    assert outcomes >= {(1, 0, False, True), (1, 0, True, False), (1, 1, False, False), (1, 2, False, True), (1, 3, False, True), (0, 0, False, False), (0, 1, False, False)}, outcomes
    assert any(r[0] and r[3] == 1 and not r[9] and r[2] & 0x20000 and not r[1] and not any(r[8]) for r in doc["rows"])   # the pair form without its tables declines
