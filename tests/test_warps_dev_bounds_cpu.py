"""What the device-resident warp kernel (k_convert_warp_dev.hip, vpf_convert_warp_tensor_dev) decides for itself and what its launcher sizes without
seeing a matrix, on the CPU: the header the kernel includes on host and device (csrc/vpf_job_bounds.h) is compiled with g++ as it stands
(tests/c/warp_dev_bounds_capi.cpp).
  warp_dev_job_ok      the ONLY thing between an untrusted frame index and six untrusted floats in device memory and a read outside a frame: against
                       a restatement on Python floats, with every special value in every slot, alone and in pairs, and random bit patterns
  warp_dev_lds_bytes   the dynamic LDS from the caller's hint: no tile of any matrix the hint covers computes a larger strip for itself (the
                       kernel's own warp_window / warp_strip), unless the bound is the 64 KiB cap — where the kernel samples per tap"""
import ctypes as C
import itertools
import math
import os
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
LIMIT = 16777216.0  # 2^24 (include/vpf_hip.h)
STRIP_MAX = 64 * 1024
N_RANDOM, N_LDS = 4000, 3000


@pytest.fixture(scope="module")
def wd(tmp_path_factory):
    from conftest import native_test_build
    so = str(tmp_path_factory.mktemp("wd") / "libwarpdevbounds.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-shared", "-fPIC", "-Wall", "-Werror", "-Wno-unused-function", *native_test_build()[0],
                           "-I" + os.path.join(ROOT, "videoprocessingframework_amd", "csrc"), os.path.join(ROOT, "tests", "c", "warp_dev_bounds_capi.cpp"), "-o", so, "-lm"])
    L = C.CDLL(so)
    u32 = C.c_uint32
    L.wd_strip_max.argtypes, L.wd_strip_max.restype = [], u32
    L.wd_jobs_ok.argtypes, L.wd_jobs_ok.restype = [C.c_void_p, u32, u32, C.c_void_p], None
    L.wd_lds_bytes.argtypes, L.wd_lds_bytes.restype = [C.c_float] + [u32] * 4, u32
    L.wd_largest_tile.argtypes, L.wd_largest_tile.restype = [C.POINTER(C.c_float), C.c_int] + [u32] * 4, u32
    assert L.wd_strip_max() == STRIP_MAX
    return L


def job_ok(frame, m, n_frames):
    """the definition (include/vpf_hip.h) on Python numbers: NaN fails every comparison, an infinity exceeds 2^24"""
    return 0 <= frame < n_frames and all(math.fabs(v) <= LIMIT for v in m)


def bits(v):
    return struct.unpack("<I", struct.pack("<f", v))[0]


def run_guard(wd, rows, n_frames):
    """rows: [(frame, (six uint32 bit patterns))] -> the guard's answers"""
    arr = np.array([[f & 0xFFFFFFFF, *m] for (f, m) in rows], dtype=np.uint32)
    out = np.empty(len(rows), np.uint8)
    wd.wd_jobs_ok(arr.ctypes.data, len(rows), n_frames, out.ctypes.data)
    return out.astype(bool)


def test_guard_with_every_special_value_in_every_slot(wd):
    """0, -0.0, +-1, +-2^24, +-nextafter(2^24, inf), +-FLT_MAX, +-inf, NaN, the smallest denormal: in each of the six slots with the others valid, and
    in every pair of slots, for frames -1, 0, n_frames - 1, n_frames, INT32_MIN, INT32_MAX"""
    above = float(np.nextafter(F(LIMIT), F(np.inf)))
    fmax = float(np.finfo(F).max)
    special = [0.0, -0.0, 1.0, -1.0, LIMIT, -LIMIT, above, -above, fmax, -fmax, math.inf, -math.inf, math.nan, float(np.finfo(F).smallest_subnormal)]
    assert above == 16777218.0 and len(special) == 14
    valid_row = [1.25, -0.5, 100.0, 0.5, 1.25, -7.0]
    for n_frames in (1, 2, 128):
        rows, want = [], []
        for frame in (-1, 0, n_frames - 1, n_frames, I32_MIN, I32_MAX):
            sets = [((a,), (va,)) for a in range(6) for va in special]
            sets += [((a, b), (va, vb)) for a, b in itertools.combinations(range(6), 2) for va in special for vb in special]
            for slots, vals in sets:
                m = list(valid_row)
                for s, v in zip(slots, vals):
                    m[s] = v
                rows.append((frame, tuple(bits(v) for v in m)))
                want.append(job_ok(frame, m, n_frames))
        got = run_guard(wd, rows, n_frames)
        want = np.array(want)
        bad = np.flatnonzero(got != want)
        assert not len(bad), (n_frames, [rows[i] for i in bad[:5]])
        assert want.any() and not want.all()
        assert len(rows) == 6 * (6 * 14 + 15 * 14 * 14)
    # the limit itself is valid, one ulp above it is not; a negative NaN and a NaN with payload are NaN
    ok = tuple(bits(v) for v in valid_row)
    for slot in range(6):
        for pattern, expect in ((bits(LIMIT), True), (bits(-LIMIT), True), (bits(LIMIT) + 1, False), (bits(-LIMIT) + 1, False), (0x7FC00001, False),
                                (0xFFC00000, False), (0x7F800001, False), (0x80000001, True)):
            m = list(ok)
            m[slot] = pattern
            assert bool(run_guard(wd, [(0, tuple(m))], 1)[0]) == expect, (slot, hex(pattern))


def test_guard_on_random_bit_patterns(wd):
    """any 32 bits in every slot; and rows whose coefficients are ordinary, with a few slots replaced by random patterns (so that valid rows occur)"""
    rng = np.random.default_rng(20260)
    n_ok = 0
    for n_frames in (2, 128):
        wild = rng.integers(0, 2 ** 32, size=(N_RANDOM, 6), dtype=np.uint64).astype(np.uint32)
        tame = rng.uniform(-3e7, 3e7, size=(N_RANDOM, 6)).astype(F).view(np.uint32)
        mixed = rng.uniform(-4, 4, size=(N_RANDOM, 6)).astype(F).view(np.uint32).copy()
        hit = rng.random((N_RANDOM, 6)) < 0.08
        mixed[hit] = wild[hit]
        pats = np.concatenate([wild, tame, mixed])
        frames = rng.integers(-2, n_frames + 2, size=len(pats))
        frames[::97] = rng.integers(I32_MIN, I32_MAX + 1, size=len(frames[::97]))
        rows = [(int(f), tuple(int(v) for v in p)) for f, p in zip(frames, pats)]
        got = run_guard(wd, rows, n_frames)
        with np.errstate(invalid="ignore"):   # signalling NaN patterns
            vals = pats.view(F).astype(np.float64)
        want = np.array([job_ok(int(f), [float(v) for v in m], n_frames) for f, m in zip(frames, vals)])
        assert np.array_equal(got, want), [rows[i] for i in np.flatnonzero(got != want)[:5]]
        n_ok += int(want.sum())
    assert n_ok > 1000


def lds_cases(rng, n):
    """(s, W, H, dw, dh, matrix as six float32): both row L1 norms <= s in exact arithmetic on the float32 values, |m02| <= W, |m12| <= H"""
    frames = [(131, 79), (130, 78), (1920, 1080), (401, 299), (3840, 2160), (1, 1), (33, 2160), (4096, 3), (640, 480)]
    dsts = [1, 31, 32, 33, 63, 64, 65, 112, 224, 8, 129]
    out = []
    while len(out) < n:
        k = len(out)
        W, H = frames[k % len(frames)] if k % 3 else (int(rng.integers(1, 4097)), int(rng.integers(1, 2161)))
        dw = dsts[k % len(dsts)] if k % 2 else int(rng.integers(1, 257))
        dh = dsts[(k // 3) % len(dsts)] if k % 5 < 2 else int(rng.integers(1, 257))
        s = F(math.exp(rng.uniform(math.log(0.02), math.log(9.0)))) if k % 13 else F([1.0, 0.5, 2.0, math.sqrt(2.0), 2.9][k % 5])
        rows = []
        for _ in range(2):
            cls = int(rng.integers(0, 5))
            if cls == 0:      # a vertex of the L1 ball
                r = [float(s), 0.0] if rng.random() < 0.5 else [0.0, float(s)]
            elif cls == 1:    # on its edge
                t = rng.random()
                r = [float(s) * t, float(s) * (1 - t)]
            elif cls == 2:    # a rotation whose L1 norm is the hint: cos + sin scaled
                a = rng.uniform(0, math.pi / 2)
                q = float(s) / (math.cos(a) + math.sin(a))
                r = [q * math.cos(a), q * math.sin(a)]
            else:             # inside
                t, q = rng.random(), rng.random()
                r = [float(s) * q * t, float(s) * q * (1 - t)]
            r = [F(r[0] * rng.choice([-1.0, 1.0])), F(r[1] * rng.choice([-1.0, 1.0]))]
            while abs(float(r[0])) + abs(float(r[1])) > float(s):   # (float64 sums of two float32 are exact) rounding pushed it out: pull it in
                r = [F(float(r[0]) * (1 - 2.0 ** -20)), F(float(r[1]) * (1 - 2.0 ** -20))]
            rows.append(r)
        tx = F(rng.choice([-W, W, 0])) if k % 7 == 0 else F(rng.uniform(-W, W))
        ty = F(rng.choice([-H, H, 0])) if k % 7 == 1 else F(rng.uniform(-H, H))
        assert abs(float(tx)) <= W and abs(float(ty)) <= H
        out.append((s, W, H, dw, dh, (rows[0][0], rows[0][1], tx, rows[1][0], rows[1][1], ty)))
    return out


def test_lds_bound_covers_every_tile_the_hint_covers(wd):
    """no tile's warp_strip(warp_window(...)).bytes exceeds warp_dev_lds_bytes(s, ...) unless that is the 64 KiB cap, in both border modes; without a
    hint the bound is the cap; it never exceeds the cap and grows with the hint"""
    rng = np.random.default_rng(20261)
    n_below = n_cap = n_nonempty = 0
    for (s, W, H, dw, dh, m) in lds_cases(rng, N_LDS):
        lds = wd.wd_lds_bytes(s, W, H, dw, dh)
        assert 0 < lds <= STRIP_MAX
        assert wd.wd_lds_bytes(0.0, W, H, dw, dh) == STRIP_MAX
        assert wd.wd_lds_bytes(F(2) * s, W, H, dw, dh) >= lds
        arr = (C.c_float * 6)(*[float(v) for v in m])
        for rep in (0, 1):
            most = wd.wd_largest_tile(arr, rep, W, H, dw, dh)
            n_nonempty += most > 0
            if lds < STRIP_MAX:
                assert most <= lds, (float(s), W, H, dw, dh, [float(v) for v in m], rep, most, lds)
        n_below += lds < STRIP_MAX
        n_cap += lds == STRIP_MAX
    print(f"LDS bound: {N_LDS} cases, {n_below} below the cap, {n_cap} at it, {n_nonempty} non-empty calls")
    assert n_below > 1500 and n_cap > 30 and n_nonempty > 3000


def test_lds_bound_at_the_sizes_the_documents_quote(wd):
    """112 x 112 crops of a 1080p frame: a unit-step hint needs 31 + 3 rows of 34 pixels, 34 x (32 x 5 + 16) bytes, far below the default"""
    assert wd.wd_lds_bytes(1.0, 1920, 1080, 112, 112) == 34 * (32 * 5 + 16)
    assert wd.wd_lds_bytes(0.0, 1920, 1080, 112, 112) == STRIP_MAX
    assert wd.wd_lds_bytes(1e30, 1920, 1080, 112, 112) == STRIP_MAX
    assert wd.wd_lds_bytes(64.0, 131, 79, 64, 48) == 79 * (32 * 17 + 16)   # clipped to the frame: 79 rows of 131 pixels


def test_the_gpu_hint_case_holds_tiles_over_the_hint(wd):
    """tests/test_gpu_warps_dev.py::test_the_hint_never_changes_a_pixel: under max_step = 1.0 the 2.9 x down-scale and the 30 degrees x 1.3 rotation of a
    131 x 79 frame into 64 x 48 compute strips beyond the hinted LDS (the in-kernel per-tap branch), the identity does not (the staged branch); with the
    jobs' true step, 2.9, every one of them fits"""
    W, H, dw, dh = 131, 79, 64, 48
    c30, s30 = 1.3 * math.cos(math.radians(30)), 1.3 * math.sin(math.radians(30))
    hinted = wd.wd_lds_bytes(1.0, W, H, dw, dh)
    assert hinted == 34 * (32 * 5 + 16)
    for m, over in (((2.9, 0, -20, 0, 2.9, -10), True), ((c30, -s30, 40, s30, c30, -10), True), ((1, 0, 33, 0, 1, 5), False)):
        arr = (C.c_float * 6)(*[float(v) for v in m])
        for rep in (0, 1):
            most = wd.wd_largest_tile(arr, rep, W, H, dw, dh)
            assert (most > hinted) == over, (m, rep, most, hinted)
            assert 0 < most <= wd.wd_lds_bytes(2.9, W, H, dw, dh) < STRIP_MAX
