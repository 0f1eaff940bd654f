"""What the device-resident perspective kernel (k_convert_persp_dev.hip, vpf_convert_persp_tensor_dev) decides for itself, what its launcher sizes
without seeing a matrix and the hint a caller computes, on the CPU: the header the kernel includes on host and device (csrc/vpf_job_bounds.h) is
compiled with g++ as it stands (tests/c/persp_dev_bounds_capi.cpp).
  persp_dev_job_ok     the ONLY thing between an untrusted frame index and nine untrusted floats in device memory and a read outside a frame: against
                       a restatement on Python floats, with every special value in every slot, alone and in pairs, and random bit patterns
  persp_step           the caller's hint for one matrix: the affine entry's hint for a last row (0, 0, 1), at least every sampled gradient sum of a
                       moderate homography, 0 exactly where persp_need has no bound
  persp_dev_lds_bytes  the dynamic LDS from that hint: no staged tile of a matrix the hint covers computes a larger strip for itself (the kernel's own
                       persp_window / warp_strip), unless the bound is the 64 KiB cap — where the kernel samples per tap"""
import ctypes as C
import itertools
import math
import os
import struct
import subprocess

import numpy as np
import pytest

from test_persp_bounds_cpu import moderate
from test_persp_tensor_cpu import NAMED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
LIMIT = 16777216.0  # 2^24 (include/vpf_hip.h)
STRIP_MAX = 64 * 1024
N_RANDOM, N_MODERATE = 4000, 2000


def build_capi(tmp_path_factory):
    from conftest import native_test_build
    so = str(tmp_path_factory.mktemp("pd") / "libperspdevbounds.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-shared", "-fPIC", "-Wall", "-Werror", "-Wno-unused-function", *native_test_build()[0],
                           "-I" + os.path.join(ROOT, "videoprocessingframework_amd", "csrc"), os.path.join(ROOT, "tests", "c", "persp_dev_bounds_capi.cpp"), "-o", so, "-lm"])
    L = C.CDLL(so)
    u32, vp = C.c_uint32, C.c_void_p
    L.pd_strip_max.argtypes, L.pd_strip_max.restype = [], u32
    L.pd_jobs_ok.argtypes, L.pd_jobs_ok.restype = [vp, u32, u32, vp], None
    L.pd_step.argtypes, L.pd_step.restype = [vp, u32, u32], C.c_float
    L.pd_need.argtypes, L.pd_need.restype = [vp] + [u32] * 4, u32
    L.pd_lds_bytes.argtypes, L.pd_lds_bytes.restype = [C.c_float] + [u32] * 4, u32
    L.pd_werr.argtypes, L.pd_werr.restype = [vp, u32, u32], C.c_double
    L.pd_walk.argtypes, L.pd_walk.restype = [vp, C.c_int] + [u32] * 5 + [vp], u32
    assert L.pd_strip_max() == STRIP_MAX
    return L


@pytest.fixture(scope="module")
def pd(tmp_path_factory):
    return build_capi(tmp_path_factory)


def job_ok(frame, m, n_frames):
    """the definition (include/vpf_hip.h) on Python numbers: NaN fails every comparison, an infinity exceeds 2^24"""
    return 0 <= frame < n_frames and all(math.fabs(v) <= LIMIT for v in m)


def bits(v):
    return struct.unpack("<I", struct.pack("<f", v))[0]


def run_guard(pd, rows, n_frames):
    """rows: [(frame, (nine uint32 bit patterns))] -> the guard's answers"""
    arr = np.array([[f & 0xFFFFFFFF, *m] for (f, m) in rows], dtype=np.uint32)
    out = np.empty(len(rows), np.uint8)
    pd.pd_jobs_ok(arr.ctypes.data, len(rows), n_frames, out.ctypes.data)
    return out.astype(bool)


def step_of(pd, m, dw, dh):
    m = np.ascontiguousarray(m, dtype=F)
    return float(pd.pd_step(m.ctypes.data, dw, dh))


def walk(pd, m, rep, W, H, dw, dh, lds=STRIP_MAX):
    """(tiles per class [border, tap, out, stage], staged tiles over `lds`, staged tiles with a pixel outside their window, the largest staged strip)"""
    m = np.ascontiguousarray(m, dtype=F)
    counts = np.zeros(6, np.uint32)
    most = pd.pd_walk(m.ctypes.data, rep, W, H, dw, dh, lds, counts.ctypes.data)
    return counts[:4].tolist(), int(counts[4]), int(counts[5]), int(most)


def test_guard_with_every_special_value_in_every_slot(pd):
    """0, -0.0, +-1, +-2^24, +-nextafter(2^24, inf), +-FLT_MAX, +-inf, NaN, the smallest denormal: in each of the nine slots with the others valid, and
    in every pair of slots, for frames -1, 0, n_frames - 1, n_frames, INT32_MIN, INT32_MAX"""
    above = float(np.nextafter(F(LIMIT), F(np.inf)))
    fmax = float(np.finfo(F).max)
    special = [0.0, -0.0, 1.0, -1.0, LIMIT, -LIMIT, above, -above, fmax, -fmax, math.inf, -math.inf, math.nan, float(np.finfo(F).smallest_subnormal)]
    assert above == 16777218.0 and len(special) == 14
    valid_row = [1.25, -0.5, 100.0, 0.5, 1.25, -7.0, 0.001, -0.002, 1.0]
    for n_frames in (1, 2, 128):
        rows, want = [], []
        for frame in (-1, 0, n_frames - 1, n_frames, I32_MIN, I32_MAX):
            sets = [((a,), (va,)) for a in range(9) for va in special]
            sets += [((a, b), (va, vb)) for a, b in itertools.combinations(range(9), 2) for va in special for vb in special]
            for slots, vals in sets:
                m = list(valid_row)
                for s, v in zip(slots, vals):
                    m[s] = v
                rows.append((frame, tuple(bits(v) for v in m)))
                want.append(job_ok(frame, m, n_frames))
        got = run_guard(pd, rows, n_frames)
        want = np.array(want)
        bad = np.flatnonzero(got != want)
        assert not len(bad), (n_frames, [rows[i] for i in bad[:5]])
        assert want.any() and not want.all()
        assert len(rows) == 6 * (9 * 14 + 36 * 14 * 14)
    # the limit itself is valid, one ulp above it is not; a negative NaN and a NaN with payload are NaN
    ok = tuple(bits(v) for v in valid_row)
    for slot in range(9):
        for pattern, expect in ((bits(LIMIT), True), (bits(-LIMIT), True), (bits(LIMIT) + 1, False), (bits(-LIMIT) + 1, False), (0x7FC00001, False),
                                (0xFFC00000, False), (0x7F800001, False), (0x80000001, True)):
            m = list(ok)
            m[slot] = pattern
            assert bool(run_guard(pd, [(0, tuple(m))], 1)[0]) == expect, (slot, hex(pattern))


def test_guard_on_random_bit_patterns(pd):
    """any 32 bits in every slot; and rows whose coefficients are ordinary, with a few slots replaced by random patterns (so that valid rows occur)"""
    rng = np.random.default_rng(20270)
    n_ok = 0
    for n_frames in (2, 128):
        wild = rng.integers(0, 2 ** 32, size=(N_RANDOM, 9), dtype=np.uint64).astype(np.uint32)
        tame = rng.uniform(-2e7, 2e7, size=(N_RANDOM, 9)).astype(F).view(np.uint32)
        mixed = rng.uniform(-4, 4, size=(N_RANDOM, 9)).astype(F).view(np.uint32).copy()
        hit = rng.random((N_RANDOM, 9)) < 0.06
        mixed[hit] = wild[hit]
        pats = np.concatenate([wild, tame, mixed])
        frames = rng.integers(-2, n_frames + 2, size=len(pats))
        frames[::97] = rng.integers(I32_MIN, I32_MAX + 1, size=len(frames[::97]))
        rows = [(int(f), tuple(int(v) for v in p)) for f, p in zip(frames, pats)]
        got = run_guard(pd, rows, n_frames)
        with np.errstate(invalid="ignore"):   # signalling NaN patterns
            vals = pats.view(F).astype(np.float64)
        want = np.array([job_ok(int(f), [float(v) for v in m], n_frames) for f, m in zip(frames, vals)])
        assert np.array_equal(got, want), [rows[i] for i in np.flatnonzero(got != want)[:5]]
        n_ok += int(want.sum())
    assert n_ok > 1000


def test_step_of_an_affine_matrix_is_the_affine_hint(pd):
    """last row (0, 0, 1): max(|m00| + |m01|, |m10| + |m11|), larger by no more than the rounding slack werr persp_need_count takes off w = 1 (the
    quotient by (1 - werr)^2) and the rounding up to fp32"""
    rng = np.random.default_rng(20271)
    for k in range(1500):
        dw, dh = int(rng.integers(1, 700)), int(rng.integers(1, 700))
        s = math.exp(rng.uniform(math.log(1e-3), math.log(50.0)))
        m = np.array([*(rng.uniform(-s, s, size=2)), rng.uniform(-4000, 4000), *(rng.uniform(-s, s, size=2)), rng.uniform(-4000, 4000), 0, 0, 1], dtype=F)
        if k % 50 == 0:
            m[:6] = (1, 0, 33, 0, 1, 5)
        exact = max(abs(float(m[0])) + abs(float(m[1])), abs(float(m[3])) + abs(float(m[4])))
        werr = pd.pd_werr(m.ctypes.data, dw, dh)
        assert werr == 4.0 * 2.0 ** -23   # (|m20| dw + |m21| dh + |m22| = 1)
        got = step_of(pd, m, dw, dh)
        assert exact <= got <= exact / (1.0 - werr) ** 2 * (1.0 + 2.0 ** -22), (m, dw, dh, got, exact)
    assert 1.0 < step_of(pd, (1, 0, 33, 0, 1, 5, 0, 0, 1), 112, 112) <= 1.0 + 9 * 2.0 ** -23   # 1 / (1 - 2^-21)^2 = 1 + 8 * 2^-23, rounded up


def exact_xy(m, x, y):
    m = [float(v) for v in m]
    w = m[6] * x + m[7] * y + m[8]
    return (m[0] * x + m[1] * y + m[2]) / w, (m[3] * x + m[4] * y + m[5]) / w


def sampled_step(m, dw, dh, rng):
    """the largest central-difference gradient sum |ds/dx| + |ds/dy| of either coordinate over sample points of the destination rectangle
    [0, dw - 1] x [0, dh - 1], in float64; the differences stay inside the rectangle (the mean-value theorem then puts each below the bound)"""
    X, Y = float(dw - 1), float(dh - 1)
    hx, hy = min(0.25, X / 2), min(0.25, Y / 2)
    xs = np.concatenate([[hx, X - hx, hx, X - hx, X / 2], rng.uniform(hx, X - hx, size=40) if X > 0 else np.zeros(40)])
    ys = np.concatenate([[hy, hy, Y - hy, Y - hy, Y / 2], rng.uniform(hy, Y - hy, size=40) if Y > 0 else np.zeros(40)])
    best = 0.0
    gx = [np.zeros_like(xs), np.zeros_like(xs)]
    gy = [np.zeros_like(xs), np.zeros_like(xs)]
    if hx > 0:
        a, b = exact_xy(m, xs + hx, ys), exact_xy(m, xs - hx, ys)
        gx = [np.abs(a[0] - b[0]) / (2 * hx), np.abs(a[1] - b[1]) / (2 * hx)]
    if hy > 0:
        a, b = exact_xy(m, xs, ys + hy), exact_xy(m, xs, ys - hy)
        gy = [np.abs(a[0] - b[0]) / (2 * hy), np.abs(a[1] - b[1]) / (2 * hy)]
    for c in range(2):
        best = max(best, float((gx[c] + gy[c]).max()))
    return best


def test_step_bounds_every_sampled_gradient_of_moderate_homographies(pd):
    """test_persp_bounds_cpu.py's moderate homographies (w within [0.4, 1.6] m22 over the destination): the hint exists and is at least the largest
    central-difference gradient sum sampled over the destination"""
    rng = np.random.default_rng(20272)
    ratios = []
    for k in range(N_MODERATE):
        m, W, H, dw, dh = moderate(rng, k)
        got = step_of(pd, m, dw, dh)
        want = sampled_step(m, dw, dh, rng)
        assert got > 0.0
        assert got >= want * (1.0 - 1e-9), (m, dw, dh, got, want)
        if want > 0:
            ratios.append(got / want)
    print(f"persp_step : sampled gradient sum, {len(ratios)} jobs: median {np.median(ratios):.3f}, max {max(ratios):.3f}")
    assert len(ratios) > 1500 and np.median(ratios) < 1.5


def corners_bounded(m, dw, dh):
    """persp_need's test on the four destination corners, restated in numpy float32 / Python floats: (corners with w > 0, bounded)"""
    m = np.asarray(m, dtype=F)
    ws = [float((m[6] * F(x) + m[7] * F(y)) + m[8]) for x, y in ((0, 0), (dw - 1, 0), (0, dh - 1), (dw - 1, dh - 1))]
    front = [w for w in ws if w > 0]
    werr = 4.0 * 2.0 ** -23 * (abs(float(m[6])) * dw + abs(float(m[7])) * dh + abs(float(m[8])))
    return len(front), len(front) == 4 and min(front) - 2.0 * werr > 0.0


def test_step_is_zero_exactly_where_persp_need_has_no_bound(pd):
    """moderate homographies whose last row is redrawn so that the horizon crosses, touches or misses the destination, and the named matrices of the
    GPU tests: persp_step is 0 where some destination corner has !(w > 0) or the smallest w is not positive after its rounding — there persp_need
    answers the 64 KiB cap (0 bytes when no corner is in front) — and positive everywhere else"""
    rng = np.random.default_rng(20273)
    n_zero = n_cap = n_behind = n_pos = 0
    cases = []
    for k in range(1500):
        m, W, H, dw, dh = moderate(rng, k)
        m = m.copy()
        if k % 3:   # w = m22 (1 - dx / x0 ...): the horizon at a drawn place relative to the destination
            x0, y0 = rng.uniform(-0.5, 2.0) * max(dw - 1, 1), rng.uniform(-0.5, 2.0) * max(dh - 1, 1)
            m[6], m[7] = (-m[8] / F(x0) if k % 2 and x0 else F(0)), (-m[8] / F(y0) if k % 4 < 2 and y0 else F(0))
        if k % 11 == 0:
            m[6:] = -m[6:]
        cases.append((m, W, H, dw, dh))
    cases += [(np.array(m, dtype=F), 131, 79, dw, dh) for name, (m, _, _) in NAMED.items() if name != "denormal w" for dw, dh in ((61, 35), (33, 33), (1, 40))]
    for m, W, H, dw, dh in cases:
        nfront, bounded = corners_bounded(m, dw, dh)
        got, need = step_of(pd, m, dw, dh), pd.pd_need(m.ctypes.data, W, H, dw, dh)
        grad = bool(np.any(m[[0, 1, 3, 4, 6, 7]] != 0))   # (a constant map has the true step 0)
        if not bounded:
            assert got == 0.0, (m, dw, dh, got)
            assert need == (STRIP_MAX if nfront else 0), (m, dw, dh, need)
            n_zero, n_cap, n_behind = n_zero + 1, n_cap + (nfront > 0), n_behind + (nfront == 0)
        elif grad:
            assert got > 0.0 and math.isfinite(got), (m, dw, dh, got)
            n_pos += 1
    print(f"persp_step == 0: {n_zero} of {len(cases)} jobs ({n_cap} with persp_need at the cap, {n_behind} behind the plane), {n_pos} positive")
    assert n_cap > 100 and n_behind > 20 and n_pos > 500
    # a bounded job whose step is no fp32 number (w = 1e-40 everywhere: 1e40 source pixels per step) has no hint to give either
    assert corners_bounded(NAMED["denormal w"][0], 61, 35) == (4, True) and step_of(pd, NAMED["denormal w"][0], 61, 35) == 0.0
    hor, behind, key = (np.array(NAMED[k][0], dtype=F) for k in ("horizon", "behind", "keystone"))
    assert step_of(pd, hor, 64, 48) == 0.0 and step_of(pd, behind, 64, 48) == 0.0 and step_of(pd, key, 64, 48) > 0.0


def test_lds_bound_covers_every_staged_tile_the_hint_covers(pd):
    """the moderate homographies with max_step = their own persp_step, both border modes: the bound is the 64 KiB cap or at least every staged tile's
    strip (persp_window / warp_strip: what the kernel compares with the LDS it was given).  Without a hint the bound is the cap; it never exceeds the cap
    and grows with the hint"""
    rng = np.random.default_rng(20274)
    n_below = n_cap = n_staged = 0
    for k in range(N_MODERATE):
        m, W, H, dw, dh = moderate(rng, k)
        s = step_of(pd, m, dw, dh)
        lds = pd.pd_lds_bytes(s, W, H, dw, dh)
        assert 0 < lds <= STRIP_MAX
        assert pd.pd_lds_bytes(0.0, W, H, dw, dh) == STRIP_MAX
        assert pd.pd_lds_bytes(2.0 * s, W, H, dw, dh) >= lds >= pd.pd_lds_bytes(0.5 * s, W, H, dw, dh)
        for rep in (0, 1):
            cls, over, _, most = walk(pd, m, rep, W, H, dw, dh, lds)
            n_staged += cls[3]
            if lds < STRIP_MAX:
                assert most <= lds and over == 0, (m, W, H, dw, dh, rep, s, most, lds)
        n_below += lds < STRIP_MAX
        n_cap += lds == STRIP_MAX
    print(f"LDS bound: {N_MODERATE} jobs, {n_below} below the cap, {n_cap} at it, {n_staged} staged tiles")
    assert n_below > 1000 and n_staged > 3000


def test_lds_bound_at_the_sizes_the_documents_quote(pd):
    """112 x 112 crops of a 1080p frame under a unit step: 31 + 5 rows of 36 pixels, persp_need's answer for the identity; no hint, a huge hint: the
    cap; a small frame: cut to it"""
    assert pd.pd_lds_bytes(1.0, 1920, 1080, 112, 112) == 36 * (32 * 5 + 16)
    assert pd.pd_lds_bytes(0.0, 1920, 1080, 112, 112) == STRIP_MAX
    assert pd.pd_lds_bytes(-1.0, 1920, 1080, 112, 112) == STRIP_MAX
    assert pd.pd_lds_bytes(1e30, 1920, 1080, 112, 112) == STRIP_MAX
    assert pd.pd_lds_bytes(64.0, 131, 79, 64, 48) == 79 * (32 * 17 + 16)   # clipped to the frame: 79 rows of 131 pixels
