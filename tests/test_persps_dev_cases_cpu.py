"""The generator of the device-homography fuzz (tests/cases_persps_dev.py), without a GPU: the same seed gives the same description, every call passes
the library's validation (the real entry with fake pointers on a device no machine has must answer VPF_ERR_NO_DEVICE), the hint is none or a true
bound, and — test_reach — the default seeds reach what the GPU test is there to run, decided by the kernel's own functions (csrc/vpf_job_bounds.h
compiled with g++, tests/c/persp_dev_bounds_capi.cpp)."""
import math
import os

import numpy as np
import pytest

import cases_persps_dev as pcases
from cases_tensor_fuzz import ELEM, LIMIT
from test_persps_dev_bounds_cpu import STRIP_MAX, build_capi, walk
from test_tensor_fuzz_cases_cpu import FAKE_DST, FAKE_TABLE, NO_GPU, _lib_or_skip, fake_sources, host_jobs

DEFAULT = range(pcases.DEFAULT_SEEDS)


@pytest.fixture(scope="module")
def pd(tmp_path_factory):
    return build_capi(tmp_path_factory)


def all_cases(seeds=DEFAULT):
    _lib_or_skip()   # (the hint is the library's vpf_persp_max_step)
    return [(seed, k, c) for seed in seeds for k, c in enumerate(pcases.cases(seed))]


def test_same_seed_same_description():
    _lib_or_skip()
    for seed in (0, 7, 15, 499):
        a, b = pcases.cases(seed), pcases.cases(seed)
        assert [repr(c) for c in a] == [repr(c) for c in b]   # (repr: a NaN coefficient is not equal to itself)
        assert len(a) == pcases.CASES_PER_SEED == 5
    assert repr(pcases.cases(0)[0]) != repr(pcases.cases(1)[0])
    assert len(pcases.seeds()) == 16 or "VPF_FUZZ_SEEDS" in os.environ


def test_descriptions_are_valid_and_accepted():
    """tables, strides, layouts and hint of every call of the default seeds and of 100 more; the real entry accepts each"""
    capi = _lib_or_skip()
    ex = capi.make_exec(device=NO_GPU)
    strides = set()
    for seed, k, call in all_cases(range(116)):
        what = f"seed {seed} case {k} {call!r}"
        n, nf, e = call["max_n"], len(call["frames"]), ELEM[call["dtype"]]
        assert call["entry"] == "persp_dev" and 1 <= n <= 14 and len(call["mats"]) == len(call["index"]) == len(call["valid"]) == n, what
        assert call["mat_floats"] in pcases.MAT_FLOATS and call["index_ints"] in pcases.INDEX_INTS, what
        strides.add((call["mat_floats"], call["index_ints"]))
        for f, m, ok in zip(call["index"], call["mats"], call["valid"]):
            assert len(m) == 9, what
            assert ok == (0 <= f < nf and all(abs(v) <= LIMIT for v in m)), what
            if ok:
                assert all(float(np.float32(v)) == v for v in m), what
        g = call["geo"]
        rb = (3 if call["nhwc"] else 1) * call["dw"] * e
        assert g["lead"] % e == 0 and g["row"] % e == 0 and g["row"] >= rb and g["frame"] % e == 0, what
        # the hint: 0 or a TRUE bound of every valid job
        steps = [capi.persp_max_step(m, call["dw"], call["dh"]) for m, ok in zip(call["mats"], call["valid"]) if ok]
        assert call["max_step"] >= 0 and math.isfinite(call["max_step"]), what
        assert call["max_step"] == 0 or (min(steps) > 0 and call["max_step"] >= max(steps)), what
        tables = dict(mats=FAKE_TABLE, index=FAKE_TABLE + 0x10000, count=FAKE_TABLE + 0x20000 if call["count"] is not None else None)
        assert pcases.invoke(capi, call, ex, fake_sources(call), FAKE_DST, tables, check=False) == capi.ERR_NO_DEVICE, what
    assert {s[0] for s in strides} == set(pcases.MAT_FLOATS) and {s[1] for s in strides} == set(pcases.INDEX_INTS)


def test_reach(pd):
    """over the default 16 seeds, on the jobs the kernel runs (below the count, valid), with the LDS the launcher gives the call: a staged tile, a
    horizon tile, a border tile, a nothing-staged tile, a staged tile whose strip exceeds the hinted LDS, a staged tile with an in-range pixel that
    fails persp_px_in_window, an invalid job, a count below max_n, a call with no hint and a call with one"""
    seen = dict.fromkeys(("staged", "horizon", "border", "nothing staged", "strip over the hinted LDS", "pixel outside its window", "invalid job",
                          "count below max_n", "no hint", "hint"), 0)
    for seed, k, call in all_cases():
        W, H, dw, dh = call["W"], call["H"], call["dw"], call["dh"]
        jobs, c = host_jobs(call)
        seen["count below max_n"] += c < call["max_n"]
        seen["invalid job"] += sum(1 for i in range(c) if not call["valid"][i])
        seen["hint" if call["max_step"] > 0 else "no hint"] += 1
        if call["tune"] == 9:
            continue   # no LDS at all: every tile samples per tap
        lds = pd.pd_lds_bytes(call["max_step"], W, H, dw, dh)
        assert 0 < lds <= STRIP_MAX and (call["max_step"] > 0 or lds == STRIP_MAX)
        for _, job in jobs:
            (border, tap, out, stage), over, flagged, _ = walk(pd, job["m"], call["mode"], W, H, dw, dh, lds)
            seen["staged"] += stage - over
            seen["horizon"] += tap
            seen["border"] += border
            seen["nothing staged"] += out
            seen["pixel outside its window"] += flagged
            if call["max_step"] > 0:
                seen["strip over the hinted LDS"] += over
    print(seen)
    missing = [name for name, count in seen.items() if not count]
    assert not missing, (missing, seen)
