"""The case generator of the seeded differential fuzz of vpf_convert_persp_tensor_dev (tests/test_gpu_persps_dev.py::test_fuzz_persps_dev), importable
without a GPU: tests/test_persps_dev_cases_cpu.py checks on the CPU that it is deterministic, that the library accepts every call and that the
default seeds reach every tile class, the per-tap branch of a staged tile, the per-pixel fallback, invalid jobs, short counts and both kinds of hint.

Built from tests/cases_tensor_fuzz.py as its warp_dev family is: draw_common, draw_warp_shape, draw_homography with its nine classes, dev_geo,
draw_count, settle_sources.  What is added: the matrix stride in floats from {9, 9, 10, 12, 16} (the padding holds NaNs the kernel must not read), the
frame-index stride, a few rows per call the header defines as invalid, and the LDS hint: none, or a TRUE bound of every valid job — the library's
own vpf_persp_max_step of each, the largest times 1 .. 1.5; none as soon as one valid job has no bound.  The hint is never a correctness input, so it
is never drawn short.  One call in eight has the shape the named sawtooth matrix was found for, with that matrix among its jobs: the staged tile
whose in-range pixels leave its window."""
import math
import os

import numpy as np

import cases_tensor_fuzz as base
from cases_tensor_fuzz import ELEM, INT_MAX, INT_MIN, LIMIT, SAWTOOTH, SAWTOOTH_SHAPE, F, _i, _pick, f32, nine
from test_tensor_fuzz_cases_cpu import PARAMS, dev_dst, host_jobs

BASE = 37000
CASES_PER_SEED = 5
DEFAULT_SEEDS = 16
MAT_FLOATS = (9, 9, 10, 12, 16)
INDEX_INTS = (1, 1, 2, 5)


def seeds():
    """VPF_FUZZ_FIRST / VPF_FUZZ_SEEDS as in tests/test_gpu_tensor_fuzz.py; 16 seeds by default"""
    first = int(os.environ.get("VPF_FUZZ_FIRST", "0"))
    return range(first, first + int(os.environ.get("VPF_FUZZ_SEEDS", str(DEFAULT_SEEDS))))


def cases(seed):
    """the calls of one seed, in the order the GPU test runs them"""
    rng = np.random.default_rng(BASE + seed)
    return [persp_dev_case(rng) for _ in range(CASES_PER_SEED)]


def matrix_valid(f, m, n_frames):
    return 0 <= f < n_frames and all(abs(v) <= LIMIT for v in m)  # (NaN fails the comparison)


def true_step(m, dw, dh):
    """vpf_persp_max_step of one valid matrix: 0.0 where it has no bound"""
    from videoprocessingframework_amd import capi
    return capi.persp_max_step(m, dw, dh)


def persp_dev_case(rng):
    call = base.draw_common(rng, "persp_dev")
    steep = base.draw_warp_shape(rng, call)
    named = rng.integers(8) == 0
    if named:
        call["W"], call["H"], call["dw"], call["dh"] = SAWTOOTH_SHAPE
        steep = False
    W, H, dw, dh = call["W"], call["H"], call["dw"], call["dh"]
    n = _i(rng, 1, 14)
    nf = len(call["frames"])
    call["mode"] = _i(rng, 0, 1)
    call["border"] = (_i(rng, 0, 255), _i(rng, 0, 255), _i(rng, 0, 255))
    rows = [(_i(rng, 0, nf - 1), base.draw_homography(rng, W, H, dw, dh, steep, "steep" if steep and rng.integers(3) == 0 else None)) for _ in range(n)]
    if named:
        rows[0] = (rows[0][0], nine(SAWTOOTH))
    # a few entries the header defines as invalid (the spellings of tests/test_gpu_persps_dev.py::test_invalid_entries_take_the_border): the border
    nan, inf, above = math.nan, math.inf, float(np.nextafter(F(LIMIT), F(np.inf)))
    ok = (1, 0, 3, 0, 1, 5, 0, 0, 1)
    bad = [(1, (nan, 0, 33, 0, 1, 5, 0, 0, 1)), (0, (1, inf, 33, 0, 1, 5, 0, 0, 1)), (0, (1, 0, -inf, 0, 1, 5, 0, 0, 1)), (1, (1, 0, 33, above, 1, 5, 0, 0, 1)),
           (1, (1, 0, 33, 0, -above, 5, 0, 0, 1)), (1, (1, 0, 33, 0, 1, nan, 0, 0, 1)), (0, (1, 0, 33, 0, 1, 5, nan, 0, 1)), (1, (1, 0, 33, 0, 1, 5, 0, -inf, 1)),
           (0, (1, 0, 33, 0, 1, 5, 0, 0, above)), (1, (1, 0, 33, 0, 1, 5, 0, 0, inf)), (-1, ok), (nf, ok), (INT_MIN, ok), (INT_MAX, ok), (0, (nan,) * 9)]
    for _ in range(int(rng.integers(3)) if n > 1 else 0):
        f, m = _pick(rng, bad)
        rows[_i(rng, 1 if named else 0, n - 1)] = (f, tuple(float(v) for v in m))
    call["index"] = [f for f, _ in rows]
    call["mats"] = [m for _, m in rows]
    call["valid"] = [matrix_valid(f, m, nf) for f, m in rows]
    call["mat_floats"] = _pick(rng, MAT_FLOATS)   # the matrix stride in floats; the padding holds NaNs the kernel must not read
    call["index_ints"] = _pick(rng, INDEX_INTS)   # the frame-index stride in int32s; the gaps name a frame that does not exist
    call["max_n"] = n
    call["count"] = base.draw_count(rng, n)
    # the LDS hint: none, or a true bound of every valid matrix (none when one of them has no bound)
    scale, hinted = rng.uniform(1.0, 1.5), bool(rng.integers(3))
    steps = [true_step(m, dw, dh) for m, v in zip(call["mats"], call["valid"]) if v]
    call["max_step"] = f32(min(max(steps) * scale, 3.0e38)) if hinted and steps and min(steps) > 0.0 else 0.0
    call["geo"] = base.dev_geo(rng, n, dw, dh, ELEM[call["dtype"]], call["nhwc"])
    return base.settle_sources(call)


# ------------------------------------------------------------------------------------------------ description -> C call (the GPU test and the CPU test)
def invoke(capi, call, ex, srcs, base_addr, tables, check=True):
    """vpf_convert_persp_tensor_dev on a description: srcs = the plane descriptors of its frames, base_addr = the address of its destination buffer,
    tables = the device addresses of mats, index and count (None: no count)"""
    norm = capi.make_tensor_norm(*PARAMS[call["params"]], dtype=call["dtype"], bgr=call["bgr"], nhwc=call["nhwc"])
    planes0, stride = dev_dst(call, base_addr)
    table = capi.make_persps_dev(tables["mats"], call["max_n"], planes0, stride, tables["index"], tables["count"], 4 * call["mat_floats"], 4 * call["index_ints"],
                                 call["max_step"])
    return capi.convert_persp_tensor_dev(ex, getattr(capi, call["sf"]), call["cs"], call["cr"], call["W"], call["H"], call["dw"], call["dh"], capi.make_frame_srcs(srcs),
                                         table, norm, capi.make_warp_opts(call["mode"], call["border"]), check=check)


def invoke_host(capi, call, ex, srcs, base_addr):
    """vpf_convert_persp_tensor on the jobs the device call defines as written and valid (host_jobs), job k at the device call's planes of job k"""
    planes0, stride = dev_dst(call, base_addr)
    norm = capi.make_tensor_norm(*PARAMS[call["params"]], dtype=call["dtype"], bgr=call["bgr"], nhwc=call["nhwc"])
    jobs, _ = host_jobs(call)
    if not jobs:
        return
    arr = capi.make_persps([(srcs[j["frame"]], [(p + k * stride if p else 0, pitch) for p, pitch in planes0], j["m"]) for k, j in jobs])
    capi.convert_persp_tensor(ex, getattr(capi, call["sf"]), call["cs"], call["cr"], call["W"], call["H"], call["dw"], call["dh"], arr, norm,
                              capi.make_warp_opts(call["mode"], call["border"]))
