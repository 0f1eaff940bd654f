"""The policy of the whole-frame fused launch on the CPU: fused_plan (csrc/vpf_fused_plan.h), the pure function launch_convert_resize
(csrc/k_convert_resize.hip) dispatches on, compiled with g++ as it stands (tests/c/fused_plan_capi.cpp).

1. For every row of the case tables of the GPU tests (tests/cases_fused_families.py) the plan names the instantiation the row names.  Those
   expectations are the GPU tests' own; the addresses are made up the way their child processes allocate (256-B aligned bases plus the row's offset,
   256-B pitches).
2. tests/golden/fused_plan_kat.json: launches recorded from the launcher as it was before the policy became a function (hash in the file), one or two
   per instantiation — label, grid, block, dynamic LDS, the family's trailing scalars.
3. Invariants, restated here without the golden file: the LDS a launch asks for, staging area included, is at most 64 KiB; a workgroup strip is
   vpf_band_rows_exact(4 R) x vpf_bound_fused_rowbytes4 bytes and at most 53 KiB; the grid covers dw x dh x n; the refusals."""
import ctypes as C
import json
import os
import random
import subprocess

import pytest

from cases_fused_families import (BAND, BGR, FAMILIES, GATHER, HALF, LDS, NV12, P16, P16_WHOLE_CASES, PLANAR, RGB, STRIP, TENSOR, TENSOR_NHWC, TENSOR_NHWC_CASES,
                                  TENSOR_OUT_CASES, YUV420, label, label_one)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFUSED, ONE = 0, 0                       # FusedFamily, FusedTable (csrc/vpf_fused_plan.h)
FAMILY = dict(zip(range(1, 7), FAMILIES + ("k_convert_strip",)))   # FUSED_HALF .. FUSED_GATHER, FUSED_STRIP_WAVE (lab builds)
S, D = 0x7F00_0000_0000, 0x7F80_0000_0000   # made-up 256-B aligned bases


def _build(tmp, name, extra):
    from conftest import native_test_build
    so = str(tmp / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-shared", "-fPIC", "-Wall", "-Werror", *extra, *native_test_build()[0],
                           "-I" + os.path.join(ROOT, "videoprocessingframework_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "fused_plan_capi.cpp"), "-o", so, "-lm"])
    L = C.CDLL(so)
    u32, u64 = C.c_uint32, C.c_uint64
    L.fp_plan.argtypes, L.fp_plan.restype = [C.c_int, C.c_int, C.c_int] + [u32] * 6 + [C.c_int, u64, u64, C.POINTER(u32)], None
    L.fp_band_rows_exact.argtypes, L.fp_band_rows_exact.restype = [C.c_int, u32, u32], u32
    L.fp_fused_rowbytes4.argtypes, L.fp_fused_rowbytes4.restype = [u32, u32], u32
    assert (L.fp_small_batch(), L.fp_max_batch()) == (32, 128)
    return L


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("fp"), "libfusedplan.so", [])


@pytest.fixture(scope="module")
def Llab(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("fplab"), "libfusedplan_lab.so", ["-DVPF_LAB_FORMS"])


def plan(L, src, dst, dtype, sw, sh, dw, dh, n, variant, sbits, dbits, epilogue=True):
    out = (C.c_uint32 * 12)()
    L.fp_plan(src, dst, int(epilogue), dtype, sw, sh, dw, dh, n, variant, sbits, dbits, out)
    return dict(zip(("family", "r", "table", "gx", "gy", "gz", "lds", "npx", "vec_ok", "chunks", "tasks", "rowq"), out))


def plan_label(p, src, dst, n):
    family = FAMILY[p["family"]]
    r = p["r"] if family not in (HALF, GATHER) else None
    assert (r is None) == (p["r"] == 0)
    assert p["table"] == ONE or (p["table"] == 1) == (n <= 32)
    return label_one(family, r, src, dst) if p["table"] == ONE else label(family, r, src, dst, n)


def staged_lds(dst, dtype, lds, npx):
    """nhwc_stage_plan (csrc/vpf_internal.h) with VPF_NHWC_DENSE = 1 | 4: f32 rows and the 16-bit rows of the 8-px family leave through a staging
    area of four waves x 64 lanes x 3 npx elements behind the kernel's own LDS, where 64 KiB hold both"""
    if dst != TENSOR_NHWC or not (dtype == 0 or npx == 8):
        return lds
    area = 4 * 64 * 3 * npx * (4 if dtype == 0 else 2)
    return lds if lds % 16 or lds + area > 64 * 1024 else lds + area


def bits(planes):
    v = 0
    for ptr, pitch in planes:
        v |= ptr | pitch
    return v


def test_rows_of_the_gpu_case_tables(L):
    for name, sw, sh, dw, dh, n, variant, off, want in TENSOR_OUT_CASES:     # NV12 -> planar f32, as test_gpu_tensor_out.test_every_family_is_selected calls
        p = (sw + 255) // 256 * 256
        sb = bits([(S + off, p), (S + off + p * sh, p)])
        db = bits([(D + 4 * dw * dh * (3 * i + c), 4 * dw) for i in range(n) for c in range(3)])
        assert plan_label(plan(L, NV12, TENSOR, 0, sw, sh, dw, dh, n, variant, sb, db), NV12, TENSOR, n) == want, name
    for name, sw, sh, dw, dh, n, variant, off, (family, r), p10 in TENSOR_NHWC_CASES:   # NV12 and P10 -> channels-last f32
        for src, e in ((NV12, 1),) + (((P16, 2),) if p10 else ()):
            p = (sw * e + 255) // 256 * 256
            sb = bits([(S + off * e, p), (S + off * e + p * sh, p)])
            db = bits([(D + 12 * dw * dh * i, 12 * dw) for i in range(n)])
            assert plan_label(plan(L, src, TENSOR_NHWC, 0, sw, sh, dw, dh, n, variant, sb, db), src, TENSOR_NHWC, n) == label(family, r, src, TENSOR_NHWC, n), (name, src)
    for name, sw, sh, dw, dh, n, variant, (align, extra), want in P16_WHOLE_CASES:      # P10 -> planar f16
        p = (2 * sw + align - 1) // align * align + extra
        sb = bits([(S, p), (S + p * sh, p)])
        db = bits([(D + 2 * dw * dh * (3 * i + c), 2 * dw) for i in range(n) for c in range(3)])
        assert plan_label(plan(L, P16, TENSOR, 1, sw, sh, dw, dh, n, variant, sb, db), P16, TENSOR, n) == want, name


@pytest.fixture(scope="module")
def kat():
    doc = json.load(open(os.path.join(ROOT, "tests", "golden", "fused_plan_kat.json")))
    assert doc["columns"] == ["src_fc", "dst_fc", "dtype", "sw", "sh", "dw", "dh", "n", "variant", "src_bits", "dst_bits", "label", "gx", "gy", "gz", "lds", "vec_ok",
                              "chunks", "tasks", "rowq"]
    assert doc["block"] == [256, 1, 1] and len(doc["parent_commit"]) == 40   # (every launch of the dispatch: dim3(256), k_job_launch.h)
    assert 400 <= len(doc["rows"]) + len(doc["lab_rows"]) <= 600
    return doc


def check_kat_row(L, row):
    src, dst, dtype, sw, sh, dw, dh, n, variant, sb, db, want, gx, gy, gz, lds, vec_ok, chunks, tasks, rowq = row
    p = plan(L, src, dst, dtype, sw, sh, dw, dh, n, variant, int(sb, 16), int(db, 16))
    assert p["family"] != REFUSED, row
    assert plan_label(p, src, dst, n) == want, (row, p)
    assert (p["gx"], p["gy"], p["gz"]) == (gx, gy, gz), (row, p)
    assert staged_lds(dst, dtype, p["lds"], p["npx"]) == lds, (row, p)
    family = FAMILY[p["family"]]
    assert p["npx"] == (8 if family == HALF else 4)
    if family == HALF:
        assert (p["chunks"], p["tasks"]) == (chunks, tasks), (row, p)
    else:
        assert p["vec_ok"] == vec_ok, (row, p)
    if family not in (HALF, GATHER):
        assert p["rowq"] == rowq, (row, p)
    return want


def test_recorded_launches(L, Llab, kat):
    seen = {check_kat_row(L, row) for row in kat["rows"]}
    assert len(seen) >= 230, len(seen)   # of the 242 instantiations of the product's code object
    for fam in FAMILIES + (HALF + "_one", LDS + "_one"):
        assert any(s.startswith("(" + fam + "<") for s in seen), fam
    lab ={check_kat_row(Llab, row) for row in kat["lab_rows"]}
    assert all(row[8] == 47 for row in kat["lab_rows"]) and any(s.startswith("(k_convert_strip<") for s in lab) and not any(s.startswith("(" + STRIP + "<") for s in lab)
    for row in kat["lab_rows"]:   # the product build does not know variant 47's family
        assert FAMILY[plan(L, *row[:9], int(row[9], 16), int(row[10], 16))["family"]] != "k_convert_strip"


def sweep_inputs(kat):
    rng = random.Random(1805)
    for row in kat["rows"]:
        yield tuple(row[:9]) + (int(row[9], 16), int(row[10], 16))
    sizes = [2, 7, 8, 16, 61, 64, 128, 192, 224, 256, 257, 640, 720, 1080, 1280, 1920, 2160, 3840, 4096]
    for _ in range(4000):
        pick = lambda: rng.choice(sizes) if rng.random() < 0.5 else rng.randrange(2, 4097)   # noqa: E731
        sw, sh, dw, dh = pick(), pick(), pick(), pick()
        k = rng.randrange(4)
        if k == 0:
            sw, sh = 2 * dw, 2 * dh
        elif k == 1:
            sw, sh, dw, dh = 3 * (dw // 2 + 1), 3 * (dh // 2 + 1), 2 * (dw // 2 + 1), 2 * (dh // 2 + 1)
        if rng.random() < 0.6:
            sw = (sw + 7) // 8 * 8
        dst = rng.choice([RGB, BGR, PLANAR, TENSOR, TENSOR_NHWC])
        src = rng.choice([NV12, YUV420, P16] if dst in (TENSOR, TENSOR_NHWC) else [NV12, YUV420])
        yield (src, dst, rng.randrange(3), sw, sh, dw, dh, rng.choice([1, 2, 3, 8, 32, 33, 64, 128]), rng.choice([0, 0, 0, 9, 40, 48, 49]),
               S | rng.choice([0, 0, 0, 1, 2, 8, 16]) | 256, D | rng.choice([0, 0, 4, 8, 16]) | 256)


def test_invariants(L, kat):
    per_family = dict.fromkeys(FAMILIES, 0)
    for src, dst, dtype, sw, sh, dw, dh, n, variant, sb, db in sweep_inputs(kat):
        p = plan(L, src, dst, dtype, sw, sh, dw, dh, n, variant, sb, db)
        what = (src, dst, dtype, sw, sh, dw, dh, n, variant, hex(sb), hex(db), p)
        family = FAMILY[p["family"]]
        per_family[family] += 1
        assert staged_lds(dst, dtype, p["lds"], p["npx"]) <= 64 * 1024 and p["lds"] % 16 == 0, what
        assert p["vec_ok"] == int(db % (16 if dst == TENSOR_NHWC or (dst == TENSOR and dtype == 0) else 8 if dst == TENSOR else 4) == 0), what
        if family == HALF:
            assert (sw, sh) == (2 * dw, 2 * dh) and p["chunks"] * 1024 >= sw and p["tasks"] == p["chunks"] * dh and 4 * p["gx"] >= p["tasks"], what
            assert (p["gy"], p["gz"], p["lds"]) == (n, 1, 0), what
        elif family == STRIP:
            R = p["r"]
            assert R in (2, 4, 8, 16) and p["lds"] == L.fp_band_rows_exact(4 * R, sh, dh) * L.fp_fused_rowbytes4(sw, dw) and p["lds"] <= 53 * 1024, what
            assert p["rowq"] * 16 == L.fp_fused_rowbytes4(sw, dw) and 256 * p["gx"] >= dw and 4 * R * p["gy"] >= dh and p["gz"] == n, what
        elif family == BAND:
            assert p["r"] in (1, 2) and src != P16 and 256 * p["gx"] >= dw and 16 * p["gy"] >= dh and p["gz"] == n, what
        else:
            assert 256 * p["gx"] >= dw and 4 * p["gy"] >= dh and p["gz"] == n, what
            assert (p["r"] in (1, 2) and src != P16 and p["lds"] > 0) if family == LDS else (p["r"], p["lds"], p["rowq"]) == (0, 0, 0), what
        if family in (BAND, LDS):   # a wave's strips: luma + chroma rows of `rowq` 16-B units, in one or two passes of 64 lanes x 16 B
            assert p["lds"] == 4 * (4 if src == NV12 else 6) * 16 * p["rowq"] and p["r"] == (1 if 16 * p["rowq"] <= 1024 else 2), what
        assert (p["table"] == ONE) == (n == 1 and dst in (RGB, BGR, PLANAR) and family in (HALF, LDS)), what
    assert all(per_family.values()), per_family


def test_refusals(L):
    ok = dict(dtype=0, sw=192, sh=48, dw=128, dh=32, n=1, variant=0, sbits=S | 256, dbits=D | 256)
    assert plan(L, NV12, TENSOR, **ok)["family"] != REFUSED and plan(L, P16, TENSOR_NHWC, **ok)["family"] != REFUSED
    for dst in (TENSOR, TENSOR_NHWC):
        assert plan(L, NV12, dst, **ok, epilogue=False)["family"] == REFUSED                # a tensor destination without an epilogue
        assert plan(L, NV12, dst, **dict(ok, n=128))["family"] != REFUSED
        assert plan(L, NV12, dst, **dict(ok, n=129))["family"] == REFUSED                   # ... or with more frames than the large table holds
    for dst in (RGB, BGR, PLANAR):
        assert plan(L, P16, dst, **ok, epilogue=False)["family"] == REFUSED                 # 16-bit sources reach tensors only
        assert plan(L, P16, dst, **ok)["family"] == REFUSED
        assert plan(L, NV12, dst, **ok, epilogue=False)["family"] != REFUSED                # (8-bit destinations have no epilogue)
    for src in (-1, 2, 3, 5, 6, 8, 9):                                                      # FC_YUV444 and everything that is no source class
        for dst in (RGB, PLANAR, TENSOR, TENSOR_NHWC):
            for shape in ({}, dict(sw=256, sh=64), dict(variant=9), dict(variant=49, sw=640, sh=90, dw=256, dh=36)):
                assert plan(L, src, dst, **dict(ok, **shape))["family"] == REFUSED, (src, dst, shape)
