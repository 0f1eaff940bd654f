"""CPU checks of tests/cases_mixed_layouts.py and gpu_util.LaidOutPlanes (the cases of tests/test_gpu_mixed_layouts.py): the generator is
deterministic; every description is a call the ABI accepts; planes overlap neither one another nor a canary region; a (P) case has pairwise
different pitches, an (O) case exactly one plane off the A256 rung, and per entry every plane index and every named frame position is the
odd one at least once; LaidOutPlanes round-trips and sees one flipped gap byte; the composed expectation stays within 1 code of EXACT."""
import numpy as np
import pytest

import cases_mixed_layouts as cm
from gpu_util import PAD, TAIL, LaidOutPlanes, plane_geometry


def all_directed(entry):
    return [(key, c) for key in cm.KEYS[entry] for c in cm.directed(entry, key)]


def frame_planes(case, side, i):
    """[(allocation, first byte, pitch, rows, row_bytes, element size)] of frame i, and the allocations' sizes"""
    fmt, w, h = cm.side_shape(case, side)
    ps = cm.plane_shapes(fmt, w, h)
    sizes, planes = plane_geometry([(rows, rb) for rows, rb, _ in ps], *cm.layout_args(case[side][i]))
    return sizes, [pl + (e,) for pl, (_, _, e) in zip(planes, ps)]


def test_the_generator_is_deterministic():
    for entry in cm.ENTRIES:
        assert repr(all_directed(entry)) == repr(all_directed(entry))
        for seed in (0, 5):
            a, b = cm.cases(entry, seed), cm.cases(entry, seed)
            assert repr(a) == repr(b) and len(a) == cm.CASES_PER_SEED[entry]
        assert repr(cm.cases(entry, 0)) != repr(cm.cases(entry, 1))
    assert [t for t, _ in cm.reach_cases()] == [t for t, _ in cm.reach_cases()]
    assert len({t for t, _ in cm.reach_cases()}) == sum(1 for _ in cm.reach_cases())


def abi_arguments(case):
    """the vpf_plane / vpf_frame_io arrays the GPU test hands to the entry (cases_mixed_layouts.launch builds them with capi.planes /
    capi.make_batch, which need no library), on allocations at made-up 256-B aligned addresses: [(vpf_plane[3] src, vpf_plane[3] dst)]"""
    from videoprocessingframework_amd import capi

    descs, base = {}, 0x7F0000000000
    for side in ("src", "dst"):
        descs[side] = []
        for i in range(case["n"]):
            sizes, planes = frame_planes(case, side, i)
            starts = [base + sum((s + 255) // 256 * 256 for s in sizes[:a]) for a in range(len(sizes))]
            base = starts[-1] + (sizes[-1] + 255) // 256 * 256
            descs[side].append([(starts[a] + off, pitch) for a, off, pitch, _, _, _ in planes])
    if case["api"] == "single":
        return [(capi.planes(descs["src"][0]), capi.planes(descs["dst"][0]))]
    return [(f.src, f.dst) for f in capi.make_batch(list(zip(descs["src"], descs["dst"])))]


def accepted(case):
    """what the entries of csrc/vpf_abi.hip ask of a call (planes_ok, dims_ok, the float rule of vpf_resize_batch, the map rules of vpf_remap),
    and `reserved == 0` in every vpf_plane of the arrays the call is made with"""
    what = cm.describe(case)
    for src, dst in abi_arguments(case):
        for side, arr in (("src", src), ("dst", dst)):
            fmt, w, h = cm.side_shape(case, side)
            shapes = cm.plane_shapes(fmt, w, h)
            for k in range(3):
                assert arr[k].reserved == 0, what
                if k < len(shapes):
                    assert arr[k].ptr and arr[k].pitch >= shapes[k][1] and (arr[k].ptr | arr[k].pitch) % shapes[k][2] == 0, what
                else:
                    assert not arr[k].ptr and arr[k].pitch == 0, what
    assert 1 <= case["n"] and len(case["src"]) == len(case["dst"]) == case["n"], what
    assert case["api"] in ("single", "batch", "batch_ws") and (case["api"] != "single" or case["n"] == 1), what
    for k in ("sw", "sh", "dw", "dh"):
        assert 1 <= case[k] <= 65536, what
    if case["kind"] != "S":
        assert case["sw"] <= 1100 and case["sh"] <= 64 and case["dw"] <= 1100 and case["dh"] <= 64, what
    for side in ("src", "dst"):
        for i in range(case["n"]):
            sizes, planes = frame_planes(case, side, i)
            spans = {}
            for a, off, pitch, rows, rb, e in planes:
                assert pitch >= rb and off % e == 0 and pitch % e == 0 and pitch < 2 ** 32, what  # (allocations are 256-B aligned: `off` is the pointer's alignment)
                assert off >= 0 and off + (rows - 1) * pitch + rb <= sizes[a] - TAIL, what        # inside the allocation, the tail canary behind it
                spans.setdefault(a, []).append((off, off + (rows - 1) * pitch + rb))
            for s in spans.values():   # planes of one allocation: one behind the other
                s.sort()
                assert all(s[j][1] <= s[j + 1][0] for j in range(len(s) - 1)), what
    if case["entry"] == "remap":
        m = case["maps"]
        assert case["sf"] in (cm.FMT["RGB"], cm.FMT["BGR"]) and case["sf"] == case["df"], what
        for pitch, off in ((m["xp"], m["xoff"]), (m["yp"], m["yoff"])):
            assert pitch >= 4 * case["dw"] and pitch % 4 == 0 and off % 4 == 0, what


def test_every_case_is_a_call_the_abi_accepts():
    for entry in cm.ENTRIES:
        for _, case in all_directed(entry):
            accepted(case)
        for seed in range(24):
            for case in cm.cases(entry, seed):
                accepted(case)
                assert case["n"] in cm.FUZZ_N and case["variant"] in (0, 40, 9)
                assert case["n"] < 33 or case["sw"] * case["sh"] <= 300 * 16, cm.describe(case)   # small frames in the large batches
    for _, case in cm.reach_cases():
        accepted(case)
    # the plane shapes are the oracle's
    import oracle

    for name, fmt in cm.FMT.items():
        for (w, h) in ((227, 227), (225, 15), (1040, 6), (1, 1)):
            assert [(r, rb) for r, rb, _ in cm.plane_shapes(fmt, w, h)] == [(r, rb * np.dtype(dt).itemsize) for r, rb, dt in oracle.plane_shapes(fmt, w, h)], name


def off_a256(case):
    """[(side, frame, plane)] of the planes that are not on the A256 rung"""
    return [(side, i, k) for side in ("src", "dst") for i in range(case["n"]) for k, t in enumerate(case[side][i]) if tuple(t) != cm.A256]


def test_pitch_only_cases_have_pairwise_different_pitches():
    for entry in cm.ENTRIES:
        ps = [c for _, c in all_directed(entry) if c["kind"] == "P"]
        assert ps and {c["api"] for c in ps} >= {"batch"} and {c["n"] for c in ps} >= {1, 3}
        for case in ps:
            pitches = []
            for side in ("src", "dst"):
                for i in range(case["n"]):
                    for a, off, pitch, rows, rb, e in frame_planes(case, side, i)[1]:
                        assert off == 0 and pitch % 256 == 0
                        pitches.append(pitch)
            assert len(set(pitches)) == len(pitches), cm.describe(case)
            if entry == "remap":
                dw = case["dw"]
                assert case["maps"] == dict(xp=4 * dw + 16, yp=4 * dw + 48, xoff=16, yoff=16)
    # the first planes follow the formula to the letter
    c = cm.pitch_only(cm.uniform(dict(cm.directed("convert", "NV12-RGB")[1])))
    assert [t for fl in c["src"] for t in fl] == [(256, 256 * (1 + k + 3 * i), 0) for i in range(3) for k in range(2)]


def test_one_odd_cases_have_exactly_one_plane_off_a256():
    for entry in cm.ENTRIES:
        cases = [c for _, c in all_directed(entry) if c["kind"] == "O"]
        odd_planes, positions, rungs = set(), set(), set()
        for case in cases:
            odd = case["odd"]
            if odd["side"] == "maps":
                assert not off_a256(case) and case["maps"] != cm.uniform(case)["maps"], cm.describe(case)
                u, m = cm.uniform(case)["maps"], case["maps"]
                assert sum(u[k] != m[k] for k in u) == 1, cm.describe(case)
                odd_planes.add(odd["plane"])
                continue
            assert off_a256(case) == [(odd["side"], odd["frame"], odd["plane"])], cm.describe(case)
            assert tuple(case[odd["side"]][odd["frame"]][odd["plane"]]) == cm.RUNGS[odd["rung"]] and odd["rung"] in cm.LADDER
            odd_planes.add((case["sf"], case["df"], odd["side"], odd["plane"]))
            positions.add((case["n"], odd["frame"]))
            rungs.add(odd["rung"])
        assert rungs == set(cm.LADDER)
        # every plane index of source and destination of every format pair is the odd one at least once
        for _, case in all_directed(entry):
            for side, k, _ in cm.planes_of(case):
                assert (case["sf"], case["df"], side, k) in odd_planes, (entry, case["sf"], case["df"], side, k)
        # and so is every frame position: first, last, middle; alone in the second dispatch of a 32-frame entry; the last slot of the first
        if entry == "remap":   # (its small batch has three frames)
            assert positions >= {(3, 0), (3, 2), (3, 1), (33, 32), (33, 31)}, positions
            assert odd_planes >= {"xmap_rows", "xmap_base", "ymap_rows", "ymap_base"}
        else:
            assert positions >= set(cm.POSITIONS), positions
    # 16-bit and float planes start at the rung of their element size
    assert cm.min_rung(1) == list(cm.LADDER) and cm.min_rung(2) == ["A8", "A4", "A2"] and cm.min_rung(4) == ["A8", "A4"]


def test_the_tiers_of_the_convert_cases():
    assert [cm.tier_of(r, (16, 4)) for r in cm.LADDER] == [1, 1, 0, 0]
    assert [cm.tier_of(r, (8, 2)) for r in cm.LADDER] == [2, 1, 1, 0]
    assert [cm.tier_of(r, (16, 8)) for r in cm.LADDER] == [1, 0, 0, 0]
    assert [cm.tier_of(r, (4,)) for r in cm.LADDER] == [1, 1, 0, 0]
    for _, case in all_directed("convert"):
        if case["kind"] == "O":
            tier, top = case["tier"]
            assert 0 <= tier <= top and (tier < top or case["odd"]["rung"] != "A1")


def test_stacked_cases_lie_like_a_contiguous_tensor():
    seen = set()
    for entry in ("convert", "resize", "fused"):
        for _, case in all_directed(entry):
            if case["kind"] != "S":
                continue
            for side in ("src", "dst"):
                fmt, w, h = cm.side_shape(case, side)
                sizes, planes = frame_planes(case, side, 0)
                seen.add((w, h))
                if len(planes) > 1:
                    assert len(sizes) == 1 and len({p[2] for p in planes}) == 1
                    if len(planes) == 3:   # pitch = row bytes, plane i at base + sum of the planes before it
                        assert planes[0][2] == planes[0][4] and [p[1] for p in planes] == [0, planes[0][3] * planes[0][2], planes[0][3] * planes[0][2] + planes[1][3] * planes[1][2]]
                    else:                  # NV12 / P10: ONE plane of 1.5 H rows with a shared pitch that is odd in elements
                        assert planes[1][1] == planes[0][3] * planes[0][2] and (planes[0][2] // planes[0][5]) % 2 == 1
    assert {(227, 227), (225, 15)} <= seen


@pytest.mark.parametrize("stacked", [False, True])
def test_laid_out_planes_round_trip_and_see_a_flipped_gap_byte(stacked):
    rng = np.random.default_rng(3)
    planes = [rng.integers(0, 256, (7, 13), dtype=np.uint8), rng.integers(0, 256, (4, 7), dtype=np.uint8), rng.integers(0, 65536, (4, 5), dtype=np.uint16)]
    layouts = (2, 2, 6) if stacked else [(256, 0, 0), (1, 1, 1), (2, 2, 2)]
    L = LaidOutPlanes(planes, layouts, stacked, device="cpu")
    got, intact = L.download()
    assert intact and all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(got, planes))
    assert len(L.bufs) == (1 if stacked else 3) and [p for _, p in L.desc()] == ([16, 16, 16] if stacked else [256, 8, 12])
    if stacked:
        base = L.bufs[0].data_ptr()
        assert [p - base for p, _ in L.desc()] == [6, 6 + 7 * 16, 6 + 11 * 16]
    # every class of byte that is not a pixel: the lead, the row padding, the gap behind a short row of a stacked plane, the tail
    sizes, geo = plane_geometry([(7, 13), (4, 7), (4, 10)], layouts, stacked)
    spots = [(geo[1][0], geo[1][1] - 1), (geo[1][0], geo[1][1] + geo[1][4]), (geo[2][0], geo[2][1] + 3 * geo[2][2] + geo[2][4]), (0, sizes[0] - 1)]
    for a, at in spots:
        L.bufs[a][at] ^= 1
        assert not L.download()[1], (a, at)
        L.bufs[a][at] ^= 1
        assert L.download()[1]
    # tight planes (pitch = row bytes) come back as copies too
    T = LaidOutPlanes(planes[:2], [(1, 0, 0), (1, 0, 0)], device="cpu")
    got, intact = T.download()
    assert intact and all(np.array_equal(a, b) for a, b in zip(got, planes)) and [p for _, p in T.desc()] == [13, 7]
    # a pixel may hold the canary's value
    planes[1][...] = PAD
    L.upload(planes)
    got, intact = L.download()
    assert intact and np.array_equal(got[1], planes[1])


def test_the_composed_expectation_stays_within_one_code_of_exact():
    """what the GPU test holds the kernels to, on the CPU: the oracle's FP32 output of the tight planes of a few cases of every entry is within 1
    code of the EXACT planes of cases_mixed_layouts.reference (nearest is exempt, as in tests/test_gpu_parity.py::_resize).  The fused entries:
    EVERY directed case against the EXACT chain; the seeded family per link, the chain within the 2 codes that follow — reference() asserts
    both, and the call that reaches 2 is among the picks"""
    import oracle

    picks = [("convert", "NV12-RGB"), ("convert", "RGB-YUV420"), ("convert", "YUV444-RGB_PLANAR"), ("resize", "NV12-linear"), ("resize", "RGB-lanczos"),
             ("resize", "YUV420-lanczos"), ("fused", "YUV420-RGB_PLANAR"), ("fused", "NV12-BGR"), ("remap", "RGB")]
    calls = []
    for entry, key in picks:
        distinct = {}
        for c in cm.directed(entry, key):
            distinct.setdefault(cm.call_key(c)[2:11], c)
        calls += list(distinct.values())[:6]
    for key in cm.KEYS["fused"]:   # every distinct directed call of the fused entries, every distinct frame
        distinct = {}
        for c in cm.directed("fused", key):
            for j in range(min(c["n"], 3)):
                distinct.setdefault(cm.call_key(c)[2:11] + (j,), dict(c, seed=c["seed"] + j))
        calls += list(distinct.values())
    two = cm.cases("fused", 80)[0]
    calls.append(two)
    for c in calls:
        src = oracle.synth(c["sf"], c["sw"], c["sh"], c["seed"])
        fp32, exact = cm.reference(oracle, c, src, cm.remap_maps(c) if c["entry"] == "remap" else None)
        for a, b in zip(fp32, exact):
            assert int(np.abs(a.astype(np.int16) - b.astype(np.int16)).max()) <= 1, cm.describe(c)
        if c["entry"] == "remap":   # out-of-range pixels keep the fill: the column left of the picture, the row below it
            dw, dh = c["dw"], c["dh"]
            assert (fp32[0].reshape(dh, dw, 3)[:, dw // 3] == 77).all() and (fp32[0].reshape(dh, dw, 3)[dh - 2] == 77).all()
    # the figure of reference()'s docstring
    sf, df, cs, cr, sw, sh, dw, dh = (two[k] for k in ("sf", "df", "cs", "cr", "sw", "sh", "dw", "dh"))
    assert (sf, df, cs, cr, sw, sh, dw, dh) == (cm.FMT["YUV420"], cm.FMT["BGR"], 0, 1, 1040, 48, 700, 32)
    src = oracle.synth(sf, sw, sh, two["seed"])
    d = np.abs(oracle.convert_resize(sf, df, cs, cr, sw, sh, src, dw, dh, oracle.FP32)[1][0].astype(int) - oracle.convert_resize(sf, df, cs, cr, sw, sh, src, dw, dh, oracle.EXACT)[1][0])
    assert d.max() == 2 and int((d == 2).sum()) == 1 and d.size == 67200
