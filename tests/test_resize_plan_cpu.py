"""The policy of the plain resize launches on the CPU: resize_plan (csrc/vpf_resize_plan.h), the pure function launch_resize_planned
(csrc/k_resize.hip) dispatches on, compiled with g++ as it stands (tests/c/resize_plan_capi.cpp).

1. tests/golden/resize_plan_kat.json: the launches of vpf_resize / vpf_resize_batch recorded from the launchers as they were before the policy
   became a function (hash in the file), a dispatch per label, frame-table size and launch order reached — per launch the label, grid, block,
   dynamic LDS and the PlaneGeom / PlaneTable words.  `replay` below walks the plan in the order the dispatch does; where the plan says "matrix
   cores first" the record says whether that launcher took the planes and what ran after it declined.  The record was made without a device,
   where "tile first" and "matrix cores first, declined, then tile" leave the same lines: the two size rules behind THAT choice are asserted on
   the plan's fields on both sides of their limits (test_lanczos_size_rules), and in the sweep.
2. For every row of the case table of the GPU test (tests/cases_resize_families.py) the plan names the launches the row names.
3. Invariants, restated here without the golden file, over a seeded sweep."""
import ctypes as C
import json
import os
import random
import struct
import subprocess

import pytest

from cases_resize_families import CASES, LANCZOS3, LINEAR, MFMA, MP, NEAREST, PB, RGB_32F, RGB_32F_PLANAR, planes_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
(NONE, GATHER, ROWPAIR, BAND, TILE, HALF, HALF3, LZ_MFMA, LZ_TILE, LZ_GATHER, F32_TILE, F32_GATHER) = range(12)   # ResizeFamily (csrc/vpf_resize_plan.h)
FIELDS = ("family", "fallback", "eff", "it", "rows", "p1", "narrow", "multi", "wpb", "lz", "gx", "gy", "gz", "threads", "lds", "scx", "scy", "vec_ok", "a0", "a1", "a2", "a3")
S, D = 0x7F00_0000_0000, 0x7F80_0000_0000   # made-up 256-B aligned bases


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    from conftest import native_test_build
    so = str(tmp_path_factory.mktemp("rp") / "libresizeplan.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-shared", "-fPIC", "-Wall", "-Werror", *native_test_build()[0],
                           "-I" + os.path.join(ROOT, "videoprocessingframework_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "resize_plan_capi.cpp"), "-o", so, "-lm"])
    lib = C.CDLL(so)
    u32, u64 = C.c_uint32, C.c_uint64
    lib.rp_plan.argtypes, lib.rp_plan.restype = [C.c_int, C.c_int, C.c_int, u32, u32, C.POINTER(u32), C.POINTER(u64), C.POINTER(u64), C.POINTER(C.c_int), C.POINTER(u32)], None
    lib.rp_plan_tile.argtypes, lib.rp_plan_tile.restype = [C.c_int, C.c_int, C.c_int, C.POINTER(u32), u32, C.c_int, C.POINTER(u32)], None
    for f, a in (("rp_band_slots", [C.c_int, u32, u32]), ("rp_band_rows_exact", [C.c_int, u32, u32]), ("rp_strip_bytes", [C.c_int, u32, u32, u32]), ("rp_strip_bytes_px4", [u32, u32])):
        getattr(lib, f).argtypes, getattr(lib, f).restype = a, u32
    lib.rp_lzm_form.argtypes, lib.rp_lzm_form.restype = [C.c_int, C.POINTER(u32), C.POINTER(u64), C.POINTER(u32), u32, C.c_int, C.c_int], C.c_char_p
    assert (lib.rp_small_batch(), lib.rp_max_batch(), lib.rp_launch_words()) == (32, 128, len(FIELDS))
    return lib


def jobs_of(fmt, sw, sh, dw, dh):
    """resize_jobs (csrc/vpf_abi.hip): (float surfaces, [(ch, k, sw, sh, dw, dh)])"""
    return fmt in (RGB_32F, RGB_32F_PLANAR), [(ch, k, pw, ph, qw, qh) for k, ((ch, _, pw, ph), (_, _, qw, qh)) in enumerate(zip(planes_of(fmt, sw, sh), planes_of(fmt, dw, dh)))]


def plan(L, f32, interp, jobs, n, call_n, sbits, dbits, knobs, njobs=None):
    flat = (C.c_uint32 * 18)(*[v for j in jobs for v in j])
    out = (C.c_uint32 * (9 + 4 * len(FIELDS)))()
    L.rp_plan(int(f32), interp, len(jobs) if njobs is None else njobs, n, call_n, flat, (C.c_uint64 * 3)(*(list(sbits) + [0, 0, 0])[:3]), (C.c_uint64 * 3)(*(list(dbits) + [0, 0, 0])[:3]),
              (C.c_int * 4)(*knobs), out)
    P = dict(zip(("ok", "single", "all", "lz_tile_all_first", "lz_mfma_all", "lz_tile_all_fallback"), out[:6]), by0=list(out[6:9]))
    launches = [dict(zip(FIELDS, out[9 + len(FIELDS) * i:9 + len(FIELDS) * (i + 1)])) for i in range(4)]
    P["mp"], P["plane"] = launches[0], launches[1:]
    return P


def band_task(ch, l):
    args = [ch, l["rows"], l["it"], l["p1"], "true" if l["multi"] else "false"]
    for default in ("false", 4, 2):   # (clang's spelling: trailing default template arguments are left out)
        if args[-1] == default:
            args.pop()
        else:
            break
    return "RowBandTask<%s>" % ", ".join(str(a) for a in args)


def band_form(l):
    return "RowBand4wm" if l["multi"] else "RowBand%d%s" % (l["rows"], "w" if l["p1"] == 8 else "n" if l["it"] == 1 else "")


def label_of(l, fam, ch, single, every_plane):
    if every_plane:
        return MP({TILE: "TileBl%d" % l["wpb"], LZ_TILE: "TileLz%d" % l["wpb"], ROWPAIR: "RowPair%d" % l["it"]}.get(fam) or band_form(l))
    lz = "true" if l["lz"] else "false"
    if single:
        return {GATHER: "(k_resize<%d, %d>)" % (ch, l["eff"]), ROWPAIR: "(k_resize_lds<%d, %d>)" % (ch, l["it"]), TILE: "(k_resize_tile<%d, %d>)" % (ch, l["wpb"]),
                HALF: "(k_resize_half<%d>)" % ch, HALF3: "k_resize_half3_r16", LZ_TILE: "(k_resize_lztile<%d, %d>)" % (ch, l["wpb"]), LZ_GATHER: "(k_resize_lanczos<%d>)" % ch,
                F32_TILE: "(k_plane_batch<TileTaskF32<%d, %s, %d>>)" % (ch, lz, l["wpb"]), F32_GATHER: "(k_resize_f32<%d, %d>)" % (ch, l["eff"])}[fam]
    return PB({GATHER: "GatherTask<%d, %d>" % (ch, l["eff"]), ROWPAIR: "RowPairTask<%d, %d>" % (ch, l["it"]), TILE: "TileTask<%d, %d>" % (ch, l["wpb"]), HALF: "HalfTask<%d>" % ch,
               HALF3: "Half3R16Task", LZ_TILE: "LanczosTileTask<%d, %d>" % (ch, l["wpb"]), LZ_GATHER: "LanczosGatherTask<%d>" % ch,
               F32_TILE: "TileTaskF32<%d, %s, %d>" % (ch, lz, l["wpb"]), F32_GATHER: "FloatGatherTask<%d, %d>" % (ch, l["eff"]), BAND: band_task(ch, l)}[fam])


def geom(j, pl, l):
    return [j[2], j[3], j[4], j[5], pl["scx"], pl["scy"], pl["vec_ok"], l["a0"], l["a1"], l["a2"], l["a3"]]


def replay(P, jobs, mfma_takes):
    """the launches of launch_resize_planned (csrc/k_resize.hip) in its order; mfma_takes(the jobs it is handed) stands for launch_lanczos_mfma's answer:
    the label of its launch, or None where it declines.
    A launch: [label, gx, gy, gz, block, lds, k, PlaneGeom words] — k = -1, every plane: [PlaneGeom words per plane, by0, k, ch per plane], the used
    part of the PlaneTable — or [the matrix-core launcher's label, planes]"""
    assert P["ok"]
    out = []
    if P["single"]:
        j, l = jobs[0], P["plane"][0]
        fam = l["family"]
        if fam == LZ_MFMA:
            took = mfma_takes([j])
            if took:
                return [[took, 1]]
            fam = l["fallback"]
        return [[label_of(l, fam, j[0], True, False), l["gx"], l["gy"], 1, l["threads"], l["lds"], 0, geom(j, l, l)]]

    def every_plane():
        m = P["mp"]
        table = [[geom(j, pl, m) for j, pl in zip(jobs, P["plane"])], P["by0"][:len(jobs)], [j[1] for j in jobs], [j[0] for j in jobs]]
        return out + [[label_of(m, m["family"], 0, False, True), m["gx"], m["gy"], m["gz"], m["threads"], m["lds"], -1, table]]
    if P["lz_tile_all_first"]:
        return every_plane()
    took = P["lz_mfma_all"] and mfma_takes(jobs)
    if took:
        return [[took, len(jobs)]]
    declined = []
    for p, l in enumerate(P["plane"][:len(jobs)]):
        took = l["family"] == LZ_MFMA and mfma_takes([jobs[p]])
        declined.append(l["family"] == LZ_MFMA and not took)
        if took:
            out.append([took, 1])
    if (P["lz_tile_all_fallback"] and all(declined)) or P["all"]:
        return every_plane()
    for p, (j, l) in enumerate(zip(jobs, P["plane"])):
        fam = l["fallback"] if declined[p] else l["family"]
        if fam != LZ_MFMA:
            out.append([label_of(l, fam, j[0], False, False), l["gx"], l["gy"], l["gz"], l["threads"], l["lds"], j[1], geom(j, l, l)])
    return out


@pytest.fixture(scope="module")
def kat():
    doc = json.load(open(os.path.join(ROOT, "tests", "golden", "resize_plan_kat.json")))
    assert doc["columns"] == ["fmt", "interp", "sw", "sh", "dw", "dh", "n", "call_n", "src_bits", "dst_bits", "knobs", "launches"]
    assert len(doc["parent_commit"]) == 40 and 200 <= len(doc["rows"]) <= 600 and doc["label_prefixes"]["PB:"] == PB("%s") and doc["label_prefixes"]["MP:"] == MP("%s")
    return doc


def same_launch(got, want, prefixes):
    if want[0] == "mfma" or got[0] == "mfma":
        return got == want
    label = prefixes[want[0][:3]] % want[0][3:] if want[0][:3] in prefixes else want[0]
    if want[6] == -1:   # every plane: the PlaneTable's used part
        return got[0] == label and got[1:8] == want[1:8]
    return got[0] == label and got[1:7] == want[1:7] and len(got[7]) == len(want[7]) and all(w is None or g == w for g, w in zip(got[7], want[7]))


def test_recorded_launches(L, kat):
    labels, orders = set(), set()
    for row in kat["rows"]:
        fmt, interp, sw, sh, dw, dh, n, call_n, sb, db, knobs, want = row
        f32, jobs = jobs_of(fmt, sw, sh, dw, dh)
        P = plan(L, f32, interp, jobs, n, call_n, [int(v, 16) for v in sb], [int(v, 16) for v in db], knobs)
        todo = list(want)   # the matrix-core launches come first in a dispatch: the record's head says what that launcher took

        def mfma_takes(js):   # (the record names the launcher, not its form: tests/golden/lzm_launch_kat.json has the forms)
            return "mfma" if todo and todo[0] == ["mfma", len(js)] and todo.pop(0) else None
        got = replay(P, jobs, mfma_takes)
        assert len(got) == len(want) and all(same_launch(g, w, kat["label_prefixes"]) for g, w in zip(got, want)), (row[:11], got, want)
        labels |= {w[0] for w in want}
        orders.add(tuple("mfma" if w[0] == "mfma" else "every" if w[6] == -1 else "plane" for w in want))
    assert len(labels) >= 95, len(labels)
    for order in (("mfma",), ("every",), ("plane",), ("mfma", "mfma", "plane"), ("mfma", "plane"), ("mfma", "plane", "plane"), ("plane", "plane", "plane")):
        assert order in orders, (order, sorted(orders))


def case_bits(fmt, sw, sh, dw, dh, n, off):
    """the planes of a case as the GPU test lays them out: 256-B aligned bases and pitches, the source base `off` bytes further"""
    sp, dp = planes_of(fmt, sw, sh), planes_of(fmt, dw, dh)
    offs = off if isinstance(off, tuple) else (off,) * len(sp)
    return ([S + offs[k] | ((c * e * w + 255) // 256 * 256) for k, (c, e, w, _) in enumerate(sp)], [D | ((c * e * w + 255) // 256 * 256) for c, e, w, _ in dp])


def test_rows_of_the_gpu_case_table(L):
    """... the matrix-core rows by the exact form: lzm_launch (csrc/vpf_lzm_plan.h) is asked what launch_lanczos_mfma is asked — the planes it is handed, the
    frames of the dispatch, the planes' alignment and pitches, the two knobs"""
    seen, forms = set(), set()
    for name, fmt, interp, sw, sh, dw, dh, n, knobs, off, want in CASES:
        f32, jobs = jobs_of(fmt, sw, sh, dw, dh)
        sb, db = case_bits(fmt, sw, sh, dw, dh, n, off)
        got = []
        for base in range(0, n, 32 if interp == LANCZOS3 else 128):   # frames_per_dispatch (csrc/vpf_abi.hip) for planes this small
            m = min(n - base, 32 if interp == LANCZOS3 else 128)
            P = plan(L, f32, interp, jobs, m, n, sb, db, knobs)

            def mfma_takes(js):
                form = L.rp_lzm_form(len(js), (C.c_uint32 * 18)(*[v for j in js for v in j]), (C.c_uint64 * 3)(*[sb[j[1]] | db[j[1]] for j in js]),
                                     (C.c_uint32 * 6)(*[(j[0] * w + 255) // 256 * 256 for j in js for w in (j[2], j[4])]), m, knobs[0], knobs[3])   # (8-bit planes: case_bits)
                return MFMA(form.decode()) if form else None
            got += replay(P, jobs, mfma_takes)
        assert [g[0] for g in got] == want, (name, [g[0] for g in got])
        forms |= {g[0] for g in got if g[0].startswith("k_lanczos_mfma<")}
        seen |= {P["mp"]["family"]} if P["all"] else {l["family"] for l in P["plane"][:len(jobs)]}
    assert seen >= {GATHER, ROWPAIR, BAND, TILE, HALF, HALF3, LZ_MFMA, LZ_TILE, LZ_GATHER, F32_TILE, F32_GATHER}, seen
    assert forms == {MFMA("LzMfma" + f) for f in ("8", "8n", "8w", "4", "4n", "8u", "4u", "4k4", "4k6", "4k8", "2k6")}, forms   # (8uw: large launches only; 2k8: no shape)


def sweep_inputs():
    rng = random.Random(2019)
    sizes = [2, 7, 8, 16, 61, 64, 128, 192, 224, 256, 257, 640, 720, 1080, 1280, 1920, 2160, 3840, 4096]
    for _ in range(6000):
        pick = lambda: rng.choice(sizes) if rng.random() < 0.5 else rng.randrange(2, 4097)   # noqa: E731
        sw, sh, dw, dh = pick(), pick(), pick(), pick()
        k = rng.randrange(7)
        if k == 0:
            sw, sh = 2 * dw, 2 * dh
        elif k == 1:
            sw, sh, dw, dh = 3 * (dw // 2 + 1), 3 * (dh // 2 + 1), 2 * (dw // 2 + 1), 2 * (dh // 2 + 1)
        elif k == 2:
            f = rng.choice([3, 5, 7])
            dw, dh = max(2, dw // f), max(2, dh // f)
            sw, sh = f * dw, (f if rng.random() < 0.7 else rng.choice([1, 2, 3])) * dh
        elif k == 3:
            sw, sh = max(2, dw // rng.choice([2, 3])), max(2, dh // rng.choice([2, 3]))
        elif k == 4:
            f = rng.uniform(2, 8)
            dw, dh = max(2, int(sw / f)), max(2, int(sh / f))
        if max(sw, sh, dw, dh) > 4096:
            continue
        fmt = rng.randrange(1, 11)
        e = 4 if fmt in (RGB_32F, RGB_32F_PLANAR) else 1
        aligned = rng.random() < 0.55
        mis = lambda: 0 if aligned or rng.random() < 0.4 else e * rng.choice([1, 2, 4, 8, 16])   # noqa: E731
        sb = [S | 256 | mis() for _ in range(3)]
        db = [D | 256 | mis() for _ in range(3)]
        knobs = (rng.choice([0, 0, 0, 0, 9, 40, 43]), rng.choice([0, 0, 0, 0, 16 | (8 << 8), 32 | (4 << 8), 8 | (8 << 8)]),
                 rng.choice([0, 0, 0, 0, 1, 2, 4, 8, 16, 0x204, 0x304, 0x104, 0x20000, 0x20008, 0x20010]), rng.choice([0, 0, 0, 1, 0x10000, 0x40000, (4 << 8) | 2]))
        yield fmt, rng.randrange(3), sw, sh, dw, dh, rng.choice([1, 1, 2, 3, 8, 32, 33, 64, 128]), sb, db, knobs


def fl(bits):
    return struct.unpack("<f", struct.pack("<I", bits))[0]


def check_tile(L, l, fam, js, n, knobs, what):
    """a tile shape is what plan_tile gives for these planes and satisfies plan_tile's own limits"""
    elem, lz = (4, bool(l["lz"])) if fam == F32_TILE else (1, fam == LZ_TILE)
    out = (C.c_uint32 * 7)()
    L.rp_plan_tile(knobs[1], int(lz), len(js), (C.c_uint32 * 18)(*[v for j in js for v in j]), n, elem, out)
    ok, ty, nr, lds, rowq, lshift, wpb = out
    assert ok and (l["a0"], l["a1"], l["a2"], l["a3"], l["lds"], l["wpb"], l["threads"]) == (ty, nr, rowq, lshift, lds, wpb, 64 * wpb), what
    assert max(j[3] / j[5] for j in js) <= 48.0, what   # (vertical factors beyond 48: no tile)
    assert 4 <= ty <= 64 and ty % 4 == 0 and wpb in (4, 8) and lds <= 64 * 1024 and rowq <= 128 * elem and (1 << lshift) >= rowq > (1 << lshift) // 2, what
    assert elem == 4 or -(-nr // ((64 * wpb) >> lshift)) <= 6, what   # kTileStagePasses
    if knobs[1]:
        assert (ty, wpb) == (knobs[1] & 0xff, knobs[1] >> 8), what


def check_band(L, l, js, n, what):
    R, rb, slots = l["rows"], 16 * l["a0"], l["a1"]
    scy = max(j[3] / j[5] for j in js)
    bound = max(L.rp_band_slots(R, j[3], j[5]) for j in js)
    assert max(L.rp_strip_bytes(j[0], j[2], j[4], 64 * (l["p1"] if j[0] == 1 else 4)) for j in js) <= 2048, what   # (packed strips of at most two 1-KiB staging passes)
    assert R in (2, 4, 8, 16) and l["lds"] == 4 * slots * rb + 16 and l["lds"] <= 64 * 1024 and l["threads"] == 256, what
    assert slots <= bound and slots == min(bound, max(L.rp_band_rows_exact(R, j[3], j[5]) for j in js)), what
    assert slots <= (16 if l["it"] == 1 else 8) and (l["it"] == 1) == (l["p1"] == 8 or (R >= 8 and rb <= 1024)) and scy <= 2.0, what
    assert (bool(l["multi"]), l["a2"] > 0) == ((R, l["p1"]) == (4, 8),) * 2 and (l["p1"] == 4 or any(j[0] == 1 for j in js)), what
    assert (R, l["it"], l["p1"], bool(l["multi"])) in ((2, 2, 4, False), (4, 2, 4, False), (8, 2, 4, False), (8, 1, 4, False), (16, 1, 4, False), (8, 1, 8, False), (16, 1, 8, False),
                                                        (4, 1, 8, True)), what   # the eight instantiations
    return 4 * R * max(1, l["a2"])   # destination rows per workgroup


def test_invariants(L):
    reached, lz_single = set(), {}
    for fmt, interp, sw, sh, dw, dh, n, sb, db, knobs in sweep_inputs():
        f32, jobs = jobs_of(fmt, sw, sh, dw, dh)
        for m, call_n in ((n, n),) if n != 33 else ((32, 33), (1, 33)):
            P = plan(L, f32, interp, jobs, m, call_n, sb, db, knobs)
            what = (fmt, interp, sw, sh, dw, dh, m, call_n, [hex(v) for v in sb], [hex(v) for v in db], knobs, P)
            forced = (knobs[3] & 0xffff) >= 2 or (knobs[2] & 0xffff) >= 2 or knobs[2] >> 16
            assert P["ok"] and bool(P["single"]) == (call_n == 1 and len(jobs) == 1 and not forced), what
            launches = [(P["mp"], P["mp"]["family"], jobs)] if P["all"] else []
            if P["lz_tile_all_first"] or P["lz_tile_all_fallback"]:   # one Lanczos tile launch for every plane: before, or after, the matrix cores were asked
                launches.append((P["mp"], LZ_TILE, jobs))
                assert not P["all"] and P["mp"]["family"] == LZ_TILE and P["lz_mfma_all"] and all(l["family"] == LZ_MFMA for l in P["plane"][:len(jobs)]), what
            # the 1-MB rule: one small multi-plane frame takes the tile launch for all planes before the matrix cores are asked
            dst_bytes = sum(j[0] * j[4] * j[5] for j in jobs)
            assert bool(P["lz_tile_all_first"]) == bool(m == 1 and len(jobs) > 1 and not knobs[3] & 0xfffff and P["lz_tile_all_fallback"] and dst_bytes <= 1000000), what
            if P["single"] and not f32 and P["plane"][0]["eff"] == LANCZOS3:   # the single-plane rule: tile first below the measured byte limit
                j, l = jobs[0], P["plane"][0]
                small = not knobs[3] & 0xfffff and j[0] * j[2] * j[3] + 6 * j[0] * j[4] * j[5] <= {1: 28000000, 2: 40000000, 3: 51000000}[j[0]]
                assert l["family"] in (LZ_TILE, LZ_MFMA) and l["fallback"] in (LZ_TILE, LZ_GATHER) and (l["family"] == LZ_TILE) == (small and l["fallback"] == LZ_TILE), what
                lz_single[(j[0], l["fallback"] == LZ_TILE, small)] = lz_single.get((j[0], l["fallback"] == LZ_TILE, small), 0) + 1
            if not P["all"] and not P["lz_tile_all_first"]:
                for j, l in zip(jobs, P["plane"]):
                    launches += [(l, l["fallback"] if l["family"] == LZ_MFMA else l["family"], [j])]
                    assert not P["lz_tile_all_fallback"] or l["fallback"] == LZ_TILE, what   # (a tile that takes every plane takes each of them)
            for l, fam, js in launches:
                reached.add(fam)
                odd = all(j[2] % j[4] == 0 and j[3] % j[5] == 0 and (j[2] // j[4]) % 2 and (j[3] // j[5]) % 2 for j in js)
                assert l["lds"] <= 64 * 1024 and l["gz"] == m and l["threads"] == (64 * l["wpb"] if fam in (TILE, LZ_TILE, F32_TILE) else 256), what
                if odd and knobs[0] not in (9, 40) and interp != NEAREST and (f32 or interp == LANCZOS3):
                    assert l["eff"] == NEAREST and fam in (GATHER, F32_GATHER), what   # odd integer factors: the centre sample
                elif len(js) == 1:
                    assert l["eff"] == interp, what
                rows_per_wg = 4
                if fam in (TILE, LZ_TILE, F32_TILE):
                    check_tile(L, l, fam, js, m, knobs, what)
                    rows_per_wg = l["a0"]
                elif fam == BAND:
                    rows_per_wg = check_band(L, l, js, m, what)
                elif fam == ROWPAIR:
                    assert 1 <= l["it"] <= 4 and l["lds"] == 8 * 16 * l["a0"] + 16 and l["it"] == -(-16 * l["a0"] // 1024), what
                    assert 16 * l["a0"] == max(L.rp_strip_bytes(j[0], j[2], j[4], 256) for j in js), what
                elif fam in (HALF, HALF3):
                    j = js[0]
                    assert interp == LINEAR and (j[2], j[3]) == (2 * j[4], 2 * j[5]) and j[4] % 4 == 0 and sb[j[1]] % 8 == 0 and db[j[1]] % (8 if j[0] == 2 else 4) == 0, what
                    if fam == HALF3:
                        assert j[0] == 3 and j[2] % 32 == 0 and (sb[j[1]] | db[j[1]]) % 16 == 0 and l["a0"] * 1024 >= j[2] and l["a1"] == l["a0"] * j[5] and 4 * l["gx"] >= l["a1"], what
                        continue
                else:
                    assert l["lds"] == 0, what
                # the grid covers dw x dh of every plane it takes: 64 columns per workgroup in the tiled, float and Lanczos gather forms, 64 lanes x the
                # pixels per lane in the others (8 in the half kernel's quads ... of 2 x 2 source pixels: dw / 4 lanes)
                cols = {TILE: 64, LZ_TILE: 64, F32_TILE: 64, F32_GATHER: 64, LZ_GATHER: 64, HALF: 256, GATHER: 256, ROWPAIR: 256}
                need_y = 0
                for j in js:
                    c = cols.get(fam) or 64 * (l["p1"] if j[0] == 1 else 4)
                    assert c * l["gx"] >= j[4], what
                    need_y += -(-j[5] // rows_per_wg)
                assert l["gy"] == need_y, what
                if l is P["mp"]:   # plane p's workgroup rows start where plane p - 1's end
                    assert all(P["by0"][p] == sum(-(-j[5] // rows_per_wg) for j in jobs[:p]) for p in range(len(jobs))), what
    assert reached >= {GATHER, ROWPAIR, BAND, TILE, HALF, HALF3, LZ_TILE, LZ_GATHER, F32_TILE, F32_GATHER}, reached
    assert all(lz_single.get((ch, True, small), 0) > 0 for ch in (1, 3) for small in (False, True)), lz_single   # both sides of the single-plane limit, with a tile planned (test_lanczos_size_rules sits ON the limits)


def test_lanczos_size_rules(L):
    """the two measured size rules of the Lanczos order at shapes on both sides of their limits, asserted on the plan's fields: one plane of one
    frame takes the tile kernel FIRST while source bytes + 6 x destination bytes <= 28 / 40 / 51 MB (1 / 2 / 3 channels) and VPF_TUNE_RESIZE_MFMA
    leaves the choice to the policy; one frame of a multi-plane format takes one tile launch for all planes first while its destination is at most 1 MB"""
    al = dict(sbits=[S | 256] * 3, dbits=[D | 256] * 3)

    def single(ch, sw, sh, dw, dh, mfma=0):
        P = plan(L, False, LANCZOS3, [(ch, 0, sw, sh, dw, dh)], 1, 1, knobs=(0, 0, 0, mfma), **al)
        assert P["ok"] and P["single"] and P["plane"][0]["fallback"] == LZ_TILE, (ch, sw, sh, dw, dh, P)
        return P["plane"][0]["family"]
    for ch, limit in ((1, 28000000), (2, 40000000), (3, 51000000)):
        dw, dh = 2000, 1000
        rows = (limit // ch - 6 * dw * dh) // 4000   # 4000-px source rows: the last height on the limit or below it, the next one above
        assert ch * (4000 * rows + 6 * dw * dh) <= limit < ch * (4000 * (rows + 1) + 6 * dw * dh)
        assert single(ch, 4000, rows, dw, dh) == LZ_TILE and single(ch, 4000, rows + 1, dw, dh) == LZ_MFMA, ch
        for knob in (0x10000, 0x40000, 0x80000):   # tables off, "small single planes too", no ring of two: always the matrix cores first
            assert single(ch, 4000, rows, dw, dh, knob) == LZ_MFMA, (ch, knob)
    assert single(3, 1920, 1080, 1280, 720) == LZ_TILE and single(3, 3840, 2160, 1920, 1080) == LZ_MFMA   # 22.8 MB; 62.2 MB
    assert single(1, 1920, 1080, 1280, 720) == LZ_TILE and single(1, 4096, 4096, 1600, 1200) == LZ_MFMA   # 7.6 MB; 28.3 MB

    def frame(fmt, sw, sh, dw, dh, n=1, mfma=0):
        f32, jobs = jobs_of(fmt, sw, sh, dw, dh)
        P = plan(L, f32, LANCZOS3, jobs, n, n, knobs=(0, 0, 0, mfma), **al)
        assert P["ok"] and not P["single"] and P["lz_mfma_all"] and P["lz_tile_all_fallback"], (fmt, sw, sh, dw, dh, n, P)
        return bool(P["lz_tile_all_first"])
    assert frame(3, 1920, 1080, 416, 416) and frame(4, 1920, 1080, 224, 224)             # NV12 -> 416^2: 260 KB; YUV420 -> 224^2: 75 KB
    assert not frame(3, 1920, 1080, 1280, 720) and not frame(4, 1920, 1080, 1280, 720)   # 1080p -> 720p: 1.38 MB, the matrix cores
    assert frame(3, 1920, 1080, 832, 800) and not frame(3, 1920, 1080, 834, 800)         # NV12: 998 400 B; 1 001 600 B (832 x 800 + 2 x 417 x 400)
    assert not frame(3, 1920, 1080, 416, 416, n=2) and not frame(3, 1920, 1080, 416, 416, mfma=0x10000) and not frame(3, 1920, 1080, 416, 416, mfma=0x40000)
    assert not frame(1, 1920, 1080, 416, 416, mfma=(4 << 8) | 2)   # (one plane, the batch kernels forced: no multi-plane rule)


def test_refusals(L):
    f32, jobs = jobs_of(4, 96, 64, 64, 40)
    ok = dict(sbits=[S | 256] * 3, dbits=[D | 256] * 3, knobs=(0, 0, 0, 0))
    assert plan(L, f32, LINEAR, jobs, 2, 2, **ok)["ok"] and plan(L, f32, LINEAR, jobs, 128, 128, **ok)["ok"]
    assert not plan(L, f32, LINEAR, jobs, 0, 0, **ok)["ok"] and not plan(L, f32, LINEAR, jobs, 129, 129, **ok)["ok"]
    for njobs in (-1, 0, 4, 5):
        assert not plan(L, f32, LINEAR, jobs, 2, 2, njobs=njobs, **ok)["ok"]
    for njobs in (1, 2, 3):
        assert plan(L, f32, LINEAR, jobs, 2, 2, njobs=njobs, **ok)["ok"]


def test_tile_vertical_limit(L):
    """no tile beyond a vertical factor of 48.  LDS rules the tall factors out for every tile height the policy picks itself; with 4-row tiles
    forced (VPF_TUNE_RESIZE_TILE = 4 | 8 << 8) a narrow Lanczos plane fits at 48 and at 49, so the limit itself decides"""
    def fallback(sh):
        P = plan(L, False, LANCZOS3, [(1, 0, 64, sh, 256, 100)], 1, 1, [S | 256] * 3, [D | 256] * 3, (0, 4 | (8 << 8), 0, 0))
        return P["plane"][0]["fallback"], P["plane"][0]["lds"]
    assert fallback(4800)[0] == LZ_TILE and fallback(4800)[1] < 60 * 1024 and fallback(4900)[0] == LZ_GATHER
