"""The policy of the convert and relayout launches on the CPU: convert_plan (csrc/vpf_convert_plan.h), the pure function launch_yuv_to_rgb
(csrc/k_yuv2rgb.hip), launch_rgb_to_yuv, launch_tensor_to_yuv (csrc/k_rgb2yuv.hip) and launch_relayout (csrc/k_relayout.hip) dispatch on, compiled
with g++ as it stands (tests/c/convert_plan_capi.cpp).

1. tests/golden/convert_plan_kat.json: dispatches of vpf_convert / vpf_convert_batch / vpf_tensor_convert(_batch) recorded from the launchers as they
   were before the policy became a function (hash in the file), a row per kernel instantiation, label, entry kind and grid form reached — per
   dispatch the instantiation, the grid and the scalar kernel arguments.  The plan must name each.
2. Every limit that is easy to lose, asserted on the plan's fields at a shape on either side of it.
3. Refusals and invariants, restated here without the golden file, over a seeded sweep.
4. For every row of the case table of the GPU test (tests/cases_convert_families.py) the plan names the labels the row names."""
import ctypes as C
import json
import os
import random
import subprocess

import pytest

from cases_convert_families import (BGR, CASES, NV12, P10, P12, RGB, RGB_32F, RGB_32F_PLANAR, RGB_PLANAR, YCBCR, YUV420, YUV444, Y)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YUV2RGB, RGB2YUV, TENSOR2YUV, RELAYOUT = range(4)                           # ConvertLaunchKind
FC_NV12, FC_YUV420, FC_YUV444, FC_RGB, FC_BGR, FC_PLANAR = range(6)         # FmtClass (csrc/vpf_classes.h)
FIELDS = ("ok", "form", "one", "src", "dst", "nts", "ballast", "sub", "mode", "dtype", "nv12", "nhwc", "gx", "gy", "gz", "na", "a0", "a1", "a2", "a3", "a4", "a5",
          "swap_src02", "swap_dst02")
KNOBS = [0, 4, 8, 9, 12, 30, 37, 40, 43, 44, 45, 46, 48, 7]                 # every value vpf_set_tuning takes, and one it does not
RELAYOUT_PAIRS = ([(NV12, YUV420), (YUV420, NV12), (NV12, Y), (Y, YUV444), (RGB, RGB_32F), (RGB_32F, RGB_32F_PLANAR), (P10, NV12), (P12, NV12)] +
                  [(a, b) for a in (RGB, BGR, RGB_PLANAR) for b in (RGB, BGR, RGB_PLANAR) if a != b and (a, b) != (RGB_PLANAR, RGB_PLANAR)] +
                  [(a, Y) for a in (RGB, BGR, RGB_PLANAR)])


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    from conftest import native_test_build
    so = str(tmp_path_factory.mktemp("cp") / "libconvertplan.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-shared", "-fPIC", "-Wall", "-Werror", *native_test_build()[0],
                           "-I" + os.path.join(ROOT, "videoprocessingframework_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "convert_plan_capi.cpp"), "-o", so])
    lib = C.CDLL(so)
    u32, u64 = C.c_uint32, C.c_uint64
    lib.cp_plan.argtypes, lib.cp_plan.restype = [C.c_int, C.c_int, C.c_int, u32, u32, u32, C.POINTER(u64), C.POINTER(u64), C.POINTER(C.c_int), C.POINTER(u32)], None
    lib.cp_form.argtypes, lib.cp_form.restype = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_char_p), C.POINTER(C.c_char_p)], C.c_char_p
    assert lib.cp_plan_words() == len(FIELDS)
    return lib


@pytest.fixture(scope="module")
def forms(L):
    """[(name, has_one, targs words, args words)]: kConvertForms"""
    out = []
    for f in range(L.cp_forms()):
        one, targs, args = C.c_int(), C.c_char_p(), C.c_char_p()
        name = L.cp_form(f, C.byref(one), C.byref(targs), C.byref(args))
        out.append((name.decode(), bool(one.value), targs.value.decode().split(), args.value.decode().split()))
    return out


def plan(L, kind, src, dst, w, h, n, sb=(0, 0, 0), db=(0, 0, 0), knob=0, reused=0, dtype=0, nv12=0, nhwc=0):
    out = (C.c_uint32 * len(FIELDS))()
    L.cp_plan(kind, src, dst, w, h, n, (C.c_uint64 * 3)(*sb), (C.c_uint64 * 3)(*db), (C.c_int * 5)(knob, reused, dtype, int(nv12), int(nhwc)), out)
    P = dict(zip(FIELDS, out))
    P["a"] = [P["a%d" % k] for k in range(P["na"])]
    return P


def kernel_of(P, forms):
    """the template-id of the instantiation the dispatch launches for this plan (k_yuv2rgb.hip, k_rgb2yuv.hip, k_relayout.hip)"""
    name, _, targs, _ = forms[P["form"]]
    vals = []
    for t in targs:
        if t == "ballast" and P["one"]:
            continue
        if t in ("nts", "sub", "nv12", "nhwc"):
            vals.append("true" if P[t] else "false")
        elif t in ("to_planar", "fill"):
            vals.append("true" if P["mode"] else "false")
        else:
            vals.append(t if t.isdigit() else str(P[t]))
    return name + ("_one" if P["one"] else "") + ("<%s>" % ", ".join(vals) if vals else "")


def label_of(P, forms):
    """what the selection log prints: the template-id in brackets; the kernels launched by name (no field among their template arguments) without"""
    by_name = not any(not t.isdigit() for t in forms[P["form"]][2])
    return kernel_of(P, forms) if by_name else "(%s)" % kernel_of(P, forms)


def form_named(forms, name):
    return [f[0] for f in forms].index(name)


# ---- 1. the known answers
def test_known_answers(L, forms):
    doc = json.load(open(os.path.join(ROOT, "tests", "golden", "convert_plan_kat.json")))
    assert doc["columns"] == ["kind", "src", "dst", "w", "h", "n", "src_bits", "dst_bits", "knob", "dst_reused", "dtype", "nv12", "nhwc", "label", "kernel", "grid", "args"]
    assert len(doc["parent_commit"]) == 40 and 300 <= len(doc["rows"]) <= 1000
    kernels = set()
    for kind, src, dst, w, h, n, sb, db, knob, reused, dtype, nv12, nhwc, label, kernel, grid, args in doc["rows"]:
        P = plan(L, kind, src, dst, w, h, n, sb, db, knob, reused, dtype, nv12, nhwc)
        row = (kind, src, dst, w, h, n, sb, db, knob, reused)
        assert P["ok"] and kernel_of(P, forms) == kernel, (row, kernel_of(P, forms), kernel)
        assert [P["gx"], P["gy"], P["gz"]] == grid and P["a"] == args, (row, kernel, P)
        # the old label is the new one with parameter NAMES where the values stand now (SRC, DST, S, OP, FC_RGB ...): same kernel name, same number of arguments
        new = label_of(P, forms)
        assert new.strip("()").split("<")[0] == label.strip("()").split("<")[0] and new.count(",") == label.count(","), (label, new)
        kernels.add(kernel)
    assert len(kernels) == 167   # every instantiation of the three units (80 + 40 + 47 kernels)
    assert {k.split("<")[0].replace("_one", "") for k in kernels} == {f[0] for f in forms}


# ---- 2. the limits
A16 = (0x100, 0x100, 0x100)   # every plane 256-B aligned


def test_variant_normalisation(L, forms):
    f = lambda name: form_named(forms, name)
    p420 = lambda **kw: plan(L, YUV2RGB, kw.pop("src", FC_NV12), kw.pop("dst", FC_RGB), kw.pop("w", 1920), kw.pop("h", 1080), kw.pop("n", 1), A16, A16, **kw)
    # unknown values (and 43, a resize-only hint) fall back to the policy
    for knob in (43, 48, 7, -1, 1000):
        for n in (1, 4):
            for dst in (FC_RGB, FC_PLANAR):
                assert p420(knob=knob, n=n, dst=dst) == p420(knob=0, n=n, dst=dst), knob
    # ... and such a value is no "0" for VPF_EXEC_DST_REUSED, which is looked at first
    assert p420(knob=0, reused=1)["nts"] == 0 and p420(knob=43, reused=1)["nts"] == 1
    assert p420(knob=0, reused=1, dst=FC_PLANAR)["form"] == f("k_nv12_planar_r16") and p420(knob=0, reused=1, dst=FC_PLANAR)["nts"] == 0
    assert p420(knob=0, reused=1, n=3)["nts"] == 0 and p420(knob=0, reused=1, n=4)["nts"] == 1   # n < 4 only
    # the policy: packed single -> p16, packed batch -> p16x with ballast (p16 below 1024 px), planar -> r16
    assert (p420()["form"], p420()["one"], p420()["ballast"]) == (f("k_nv12_rgb_p16"), 1, 0)
    assert (p420(n=4)["form"], p420(n=4)["ballast"]) == (f("k_nv12_rgb_p16x"), 16)
    assert (p420(n=4, w=1008)["form"], p420(n=4, w=1008)["ballast"]) == (f("k_nv12_rgb_p16"), 16)
    assert (p420(n=3)["form"], p420(n=3)["ballast"]) == (f("k_nv12_rgb_p16"), 0)
    assert p420(dst=FC_PLANAR)["form"] == f("k_nv12_planar_r16")
    # 45 / 46 become 8 / 30 where p16x does not apply: below 1024 px, planar outputs
    for knob, ballast in ((45, 0), (46, 16)):
        assert (p420(knob=knob, n=2)["form"], p420(knob=knob, n=2)["ballast"]) == (f("k_nv12_rgb_p16x"), ballast)
        assert (p420(knob=knob, n=2, w=1024, h=2)["form"], p420(knob=knob, n=2, w=1008, h=2)["form"]) == (f("k_nv12_rgb_p16x"), f("k_nv12_rgb_p16"))
        assert p420(knob=knob, n=2, w=1008, h=2)["ballast"] == ballast
        assert (p420(knob=knob, n=2, dst=FC_PLANAR)["form"], p420(knob=knob, n=2, dst=FC_PLANAR)["ballast"]) == (f("k_nv12_rgb_p16"), ballast)
        assert p420(knob=knob)["one"] == 1 and p420(knob=knob)["ballast"] == 0   # the single-frame entry has no ballast argument
    # r16 on a packed destination becomes p4; p16 / r16 on an irregular frame become p4
    for knob in (37, 44):
        assert p420(knob=knob)["form"] == f("k_yuv420_rgb_p4")
        assert (p420(knob=knob, dst=FC_PLANAR)["form"], p420(knob=knob, dst=FC_PLANAR)["nts"]) == (f("k_nv12_planar_r16"), int(knob == 37))
    for knob in (8, 12, 30, 37, 44, 45, 46):
        for kw in (dict(w=1912), dict(h=1079), dict(sb=(0x108, 0x100, 0x100))):
            q = dict(dict(src=FC_NV12, dst=FC_PLANAR, w=1920, h=1080, sb=A16), **kw)
            assert plan(L, YUV2RGB, q["src"], q["dst"], q["w"], q["h"], 2, q["sb"], A16, knob=knob)["form"] == f("k_yuv420_rgb_p4"), (knob, kw)
    # anything that is not 4-B aligned (2-B: YUV420 chroma) becomes generic, whatever was asked
    for knob in KNOBS:
        assert plan(L, YUV2RGB, FC_NV12, FC_RGB, 1920, 1080, 2, (0x100, 0x102, 0), A16, knob=knob)["form"] == f("k_yuv_rgb_generic")
        assert plan(L, YUV2RGB, FC_NV12, FC_RGB, 1920, 1080, 2, A16, (0x101, 0, 0), knob=knob)["form"] == f("k_yuv_rgb_generic")
        want = f("k_yuv_rgb_generic") if knob == 9 else f("k_yuv420_rgb_p4")
        assert plan(L, YUV2RGB, FC_YUV420, FC_RGB, 1920, 1080, 2, (0x100, 0x102, 0x102), A16, knob=knob)["form"] == want
        assert plan(L, YUV2RGB, FC_YUV420, FC_RGB, 1920, 1080, 2, (0x100, 0x101, 0x100), A16, knob=knob)["form"] == f("k_yuv_rgb_generic")
    # YUV420 chroma needs 8 B for p16 / r16, NV12 chroma 16
    assert plan(L, YUV2RGB, FC_YUV420, FC_RGB, 1920, 1080, 1, (0x100, 0x108, 0x108), A16)["form"] == f("k_nv12_rgb_p16")
    assert plan(L, YUV2RGB, FC_NV12, FC_RGB, 1920, 1080, 1, (0x100, 0x108, 0), A16)["form"] == f("k_yuv420_rgb_p4")
    # 40 and 4: p4; 9: generic
    assert p420(knob=40)["form"] == p420(knob=4)["form"] == f("k_yuv420_rgb_p4") and p420(knob=9)["form"] == f("k_yuv_rgb_generic")


def test_size_limits(L, forms):
    f = lambda name: form_named(forms, name)
    # big_single: n < 4 and w * h >= 3 << 20 sends a planar frame from r16 to p16
    for (w, h), n, want in (((2048, 1534), 1, "k_nv12_planar_r16"), ((2048, 1536), 1, "k_nv12_rgb_p16"), ((2048, 1536), 3, "k_nv12_rgb_p16"), ((2048, 1536), 4, "k_nv12_planar_r16"),
                            ((3840, 2160), 1, "k_nv12_rgb_p16"), ((1920, 1080), 1, "k_nv12_planar_r16")):
        assert plan(L, YUV2RGB, FC_NV12, FC_PLANAR, w, h, n, A16, A16)["form"] == f(want), (w, h, n)
    # p16x numbers its blocks in 32 bits: (w / 16) * (h / 2) < 2^30.  The C ABI stops at 65536 x 65536 (2^27 blocks), so only the plan can be asked:
    # 65536 x 524286 is the last even height below the limit
    P = plan(L, YUV2RGB, FC_NV12, FC_RGB, 65536, 524286, 4, A16, A16)
    assert (P["form"], P["a"], P["gx"]) == (f("k_nv12_rgb_p16x"), [4096, 4096 * 262143], 4096 * 262143 // 256)
    P = plan(L, YUV2RGB, FC_NV12, FC_RGB, 65536, 524288, 4, A16, A16)
    assert (P["form"], P["ballast"]) == (f("k_nv12_rgb_p16"), 16)
    assert plan(L, YUV2RGB, FC_NV12, FC_RGB, 65536, 524288, 4, A16, A16, knob=45)["form"] == f("k_nv12_rgb_p16")
    assert plan(L, YUV2RGB, FC_NV12, FC_RGB, 65536, 65536, 4, A16, A16)["form"] == f("k_nv12_rgb_p16x")   # the largest legal frame
    # the 4:4:4 p4 form has the row in blockIdx.y: h <= 65535
    assert plan(L, YUV2RGB, FC_YUV444, FC_RGB, 4, 65535, 1, A16, A16)["form"] == f("k_yuv444_rgb_p4")
    assert plan(L, YUV2RGB, FC_YUV444, FC_RGB, 4, 65536, 1, A16, A16)["form"] == f("k_yuv_rgb_generic")
    assert plan(L, YUV2RGB, FC_YUV444, FC_RGB, 16, 65536, 1, A16, A16)["form"] == f("k_yuv444_rgb_r16")   # (the task kernels are not bound by it)
    # NV12 <-> YUV420 r16 asks w % 32, its p16 form w % 16
    for s, d in ((NV12, YUV420), (YUV420, NV12)):
        assert plan(L, RELAYOUT, s, d, 64, 2, 1, A16, A16)["form"] == f("k_nv12_yuv420_r16")
        assert plan(L, RELAYOUT, s, d, 48, 2, 1, A16, A16)["form"] == f("k_nv12_yuv420_p16")
        assert plan(L, RELAYOUT, s, d, 64, 3, 1, A16, A16)["form"] == plan(L, RELAYOUT, s, d, 40, 2, 1, A16, A16)["form"] == f("k_relayout_generic")
    # RGB_32F -> planar r4 asks w % 4, not w % 16
    assert plan(L, RELAYOUT, RGB_32F, RGB_32F_PLANAR, 20, 3, 1, A16, A16)["form"] == f("k_rgb32f_planar_r4")
    assert plan(L, RELAYOUT, RGB_32F, RGB_32F_PLANAR, 18, 3, 1, A16, A16)["form"] == f("k_relayout_generic")


def test_knob_40_and_9_per_unit(L, forms):
    f = lambda name: form_named(forms, name)
    chain = lambda kind, s, d, w, h, **kw: [forms[plan(L, kind, s, d, w, h, 2, A16, A16, knob=k, **kw)["form"]][0] for k in (0, 40, 9)]
    assert chain(YUV2RGB, FC_NV12, FC_RGB, 16, 2) == ["k_nv12_rgb_p16", "k_yuv420_rgb_p4", "k_yuv_rgb_generic"]
    assert chain(YUV2RGB, FC_YUV444, FC_RGB, 16, 2) == ["k_yuv444_rgb_r16", "k_yuv444_rgb_p4", "k_yuv_rgb_generic"]
    assert chain(RGB2YUV, FC_RGB, FC_YUV420, 16, 2) == ["k_rgb_yuv_r16", "k_rgb_yuv_p4", "k_rgb_yuv_quad"]
    # the tensor launch knows 9 only
    assert chain(TENSOR2YUV, 0, 0, 16, 2, nv12=1) == ["k_tensor_yuv_r", "k_tensor_yuv_r", "k_tensor_yuv_quad"]
    assert chain(RELAYOUT, NV12, YUV420, 32, 2) == ["k_nv12_yuv420_r16", "k_nv12_yuv420_p16", "k_relayout_generic"]
    assert chain(RELAYOUT, RGB, RGB_PLANAR, 16, 2) == ["k_rgb_relayout_r16", "k_rgb_relayout_p4", "k_relayout_generic"]
    assert chain(RELAYOUT, RGB, Y, 16, 2) == ["k_gray_r16", "k_gray_p4", "k_relayout_generic"]
    assert chain(RELAYOUT, RGB, RGB_32F, 16, 2) == ["k_u8_to_f32_x4", "k_u8_to_f32_p4", "k_relayout_generic"]
    assert chain(RELAYOUT, P10, NV12, 16, 2) == ["k_p16_to_8_x16", "k_p16_to_8_p8", "k_relayout_generic"]
    # the plane copies have one fast form, which 40 leaves alone; the float de-interleave has one, which 40 takes away
    assert chain(RELAYOUT, NV12, Y, 16, 2) == chain(RELAYOUT, Y, YUV444, 16, 2) == ["k_copy_plane_p16", "k_copy_plane_p16", "k_relayout_generic"]
    assert chain(RELAYOUT, RGB_32F, RGB_32F_PLANAR, 16, 2) == ["k_rgb32f_planar_r4", "k_relayout_generic", "k_relayout_generic"]
    assert f("k_relayout_generic") == len(forms) - 1


def test_tensor_dtype_is_refused_on_the_fast_path_only(L, forms):
    for dtype in (3, 7, 255):
        assert not plan(L, TENSOR2YUV, 0, 0, 16, 2, 1, A16, A16, dtype=dtype, nv12=1)["ok"]
        for kw in (dict(w=15), dict(h=3), dict(knob=9), dict(sb=(0x104, 0x100, 0x100))):
            q = dict(dict(w=16, h=2, knob=0, sb=A16), **kw)
            P = plan(L, TENSOR2YUV, 0, 0, q["w"], q["h"], 1, q["sb"], A16, knob=q["knob"], dtype=dtype, nv12=1)
            assert P["ok"] and forms[P["form"]][0] == "k_tensor_yuv_quad", (dtype, kw)
    for dtype, px in ((0, 8), (1, 16), (2, 16)):   # a lane's pixels: 8 f32 or 16 f16 / bf16
        P = plan(L, TENSOR2YUV, 0, 0, 1040, 2, 1, A16, A16, dtype=dtype)
        assert P["ok"] and P["a"] == [1040, 2, -(-1040 // (64 * px)), -(-1040 // (64 * px))]


def test_single_frame_entry_asks_the_dispatch(L, forms):
    """vpf_convert_batch cuts 33 frames into dispatches of 32 and 1 and plans each on its own: the last takes the scalar-argument entry"""
    first, last = plan(L, YUV2RGB, FC_NV12, FC_RGB, 16, 2, 32, A16, A16), plan(L, YUV2RGB, FC_NV12, FC_RGB, 16, 2, 1, A16, A16)
    assert (label_of(first, forms), label_of(last, forms)) == ("(k_nv12_rgb_p16<3, true, 16, 0>)", "(k_nv12_rgb_p16_one<3, true, 0>)")


# ---- 3. refusals and invariants over a seeded sweep
def legal(kind, src, dst, w, h, sb, db, knob, dtype, nv12, nhwc):
    """what the launchers refused before the plan (hipErrorInvalidValue), restated"""
    if kind == YUV2RGB:
        return src in (FC_NV12, FC_YUV420, FC_YUV444) and dst in (FC_RGB, FC_BGR, FC_PLANAR)
    if kind == RGB2YUV:
        return src in (FC_RGB, FC_BGR, FC_PLANAR)
    if kind == TENSOR2YUV:
        chroma = [15] if nv12 else [7, 7]
        fast = knob != 9 and w % 16 == 0 and h % 2 == 0 and not any(b & 15 for b in sb[:1 if nhwc else 3]) and not db[0] & 15 and not any(b & m for b, m in zip(db[1:], chroma))
        return dtype in (0, 1, 2) or not fast
    return (src, dst) in RELAYOUT_PAIRS


def preconditions(name, P, kind, src, dst, w, h, n, sb, db):
    """what each kernel family asks of the frames it is launched on (the headers of the kernels): width and height, and per plane the alignment"""
    al = lambda bits, masks: all(not (b & (m - 1)) for b, m in zip(bits, masks))
    planar_s = (kind == RGB2YUV and src == FC_PLANAR) or (kind == RELAYOUT and src == RGB_PLANAR)
    if name in ("k_yuv_rgb_generic", "k_rgb_yuv_quad", "k_tensor_yuv_quad", "k_relayout_generic"):
        return True
    if name in ("k_nv12_planar_r16", "k_nv12_rgb_p16", "k_nv12_rgb_p16x"):
        ok = w % 16 == 0 and h % 2 == 0 and al(sb, [16, 16] if src == FC_NV12 else [16, 8, 8]) and al(db, [16] * (3 if dst == FC_PLANAR else 1))
        if name == "k_nv12_planar_r16":
            ok = ok and dst == FC_PLANAR
        if name == "k_nv12_rgb_p16x":
            ok = ok and dst != FC_PLANAR and w >= 1024 and (w // 16) * (h // 2) < 2 ** 30
        return ok
    if name == "k_yuv420_rgb_p4":
        return al(sb, [4, 4] if src == FC_NV12 else [4, 2, 2]) and al(db, [4] * (3 if dst == FC_PLANAR else 1))
    if name in ("k_yuv444_rgb_r16", "k_yuv444_rgb_p4"):
        m = 16 if name.endswith("r16") else 4
        return w % m == 0 and al(sb, [m] * 3) and al(db, [m] * (3 if dst == FC_PLANAR else 1)) and (m == 16 or h <= 65535)
    if name in ("k_rgb_yuv_r16", "k_rgb_yuv_p4"):
        m, sub = (16 if name.endswith("r16") else 4), dst == FC_YUV420
        return w % m == 0 and (h % 2 == 0 or (m == 16 and not sub)) and al(sb, [m] * (3 if planar_s else 1)) and al(db, [m, m // 2, m // 2] if sub else [m] * 3)
    if name == "k_tensor_yuv_r":
        return w % 16 == 0 and h % 2 == 0 and al(sb, [16] * (1 if P["nhwc"] else 3)) and al(db, [16, 16] if P["nv12"] else [16, 8, 8]) and P["dtype"] in (0, 1, 2)
    if name == "k_nv12_yuv420_r16":
        return w % 32 == 0 and h % 2 == 0 and al(sb, [16] * (2 if src == NV12 else 3)) and al(db, [16] * (3 if src == NV12 else 2))
    if name == "k_nv12_yuv420_p16":
        return w % 16 == 0 and h % 2 == 0 and al(sb, [16, 16] if src == NV12 else [16, 8, 8]) and al(db, [16, 8, 8] if src == NV12 else [16, 16])
    ns, nd = {RGB_PLANAR: 3, NV12: 2, P10: 2, P12: 2}.get(src, 1), {RGB_PLANAR: 3, YUV444: 3, RGB_32F_PLANAR: 3, NV12: 2}.get(dst, 1)
    if dst == Y:
        ns, nd = (3 if src == RGB_PLANAR else 1), 1   # (NV12 -> Y copies the luma plane only)
    wmod, sm, dm = {"k_rgb_relayout_r16": (16, 16, 16), "k_gray_r16": (16, 16, 16), "k_rgb_relayout_p4": (4, 4, 4), "k_gray_p4": (4, 4, 4), "k_copy_plane_p16": (16, 16, 16),
                    "k_u8_to_f32_x4": (16, 4, 16), "k_u8_to_f32_p4": (4, 4, 16), "k_rgb32f_planar_r4": (4, 16, 16), "k_p16_to_8_x16": (16, 16, 16), "k_p16_to_8_p8": (8, 16, 8)}[name]
    return w % wmod == 0 and al(sb[:ns], [sm] * ns) and al(db[:nd], [dm] * nd)


def covers(name, P, w, h, n, dtype):
    """the grid reaches every pixel of every frame: lanes x what a lane (or wave) takes, per family"""
    gx, gy, gz, a = P["gx"], P["gy"], P["gz"], P["a"]
    tasks = lambda chunk_px, rows: (gy, gz) == (n, 1) and a[-2] * chunk_px >= w and a[-1] == a[-2] * rows and 4 * gx >= a[-1]   # a wave per task, 4 waves per workgroup
    groups = lambda px, rows, gpos=2: gz == n and a[gpos] * px >= w and 64 * gx >= a[gpos] and 4 * gy >= rows                       # a lane per group, a wave per row
    ch = (h + 1) // 2
    if name in ("k_yuv_rgb_generic", "k_rgb_yuv_quad", "k_tensor_yuv_quad"):
        return gz == n and 128 * gx >= w and 8 * gy >= h and a == [w, h]
    if name == "k_relayout_generic":
        return gz == n and 64 * gx >= w and 4 * gy >= h and a == [w, h]
    if name == "k_nv12_rgb_p16x":
        return (gy, gz) == (n, 1) and a == [w // 16, (w // 16) * (h // 2)] and 256 * gx >= a[1]
    if name == "k_yuv444_rgb_p4":
        return (gy, gz) == (h, n) and a == [w, h, w // 4] and 256 * gx >= a[2]
    if name == "k_nv12_yuv420_r16":
        return (gy, gz) == (n, 1) and a[:2] == [w, h] and a[2] * 1024 >= w and a[3] == a[2] * h and a[4] * 2048 >= w and a[5] == a[3] + a[4] * (h // 2) and 4 * gx >= a[5]
    if name == "k_p16_to_8_x16":
        return a[:3] == [w, h, ch] and tasks(1024, h + ch)
    if name == "k_p16_to_8_p8":
        return a[:3] == [w, h, ch] and groups(8, h + ch, 3)
    if name == "k_u8_to_f32_x4":
        return a[:2] == [3 * w // 4, h] and (gy, gz) == (n, 1) and a[2] * 256 >= a[0] and a[3] == a[2] * h and 4 * gx >= a[3]
    if name == "k_u8_to_f32_p4":
        return a == [3 * w, h, 3 * w // 4] and gz == n and 64 * gx >= a[2] and 4 * gy >= h
    if a[:2] != [w, h]:
        return False
    if name in ("k_nv12_rgb_p16", "k_rgb_yuv_r16") and (name == "k_nv12_rgb_p16" or P["sub"]):
        return tasks(1024, h // 2)
    if name in ("k_nv12_planar_r16", "k_yuv444_rgb_r16", "k_rgb_yuv_r16", "k_rgb_relayout_r16", "k_gray_r16"):
        return tasks(1024, h)
    if name == "k_rgb32f_planar_r4":
        return tasks(256, h)
    if name == "k_yuv420_rgb_p4":
        return tasks(256, (h + 1) // 2)
    if name == "k_tensor_yuv_r":
        return tasks(64 * (8 if dtype == 0 else 16), h // 2)
    if name in ("k_rgb_yuv_p4", "k_nv12_yuv420_p16"):
        return groups(4 if name == "k_rgb_yuv_p4" else 16, h // 2)
    return groups({"k_rgb_relayout_p4": 4, "k_gray_p4": 4, "k_copy_plane_p16": 16}[name], h)


def test_sweep(L, forms):
    rng = random.Random(22)
    reached = set()
    sizes = [(3, 3), (4, 2), (6, 2), (8, 2), (12, 3), (16, 2), (16, 3), (32, 2), (48, 4), (1008, 4), (1023, 3), (1024, 2), (1040, 10), (1920, 1080), (2048, 1534), (2048, 1536),
             (4, 65535), (4, 65536), (3840, 2160), (65536, 32768)]
    bits = lambda: tuple(0x100 | rng.choice([0, 0, 0, 1, 2, 4, 8, 16]) for _ in range(3))
    for it in range(30000):
        kind = rng.randrange(4)
        if kind == RELAYOUT:
            src, dst = rng.choice(RELAYOUT_PAIRS) if rng.random() < 0.9 else (rng.randrange(18), rng.randrange(18))
        else:
            src, dst = (rng.randrange(-1, 9), rng.randrange(-1, 9)) if rng.random() < 0.1 else \
                {YUV2RGB: (rng.randrange(3), rng.randrange(3, 6)), RGB2YUV: (rng.randrange(3, 6), rng.choice((FC_YUV444, FC_YUV420))), TENSOR2YUV: (0, 0)}[kind]
        (w, h), n = (rng.choice(sizes) if rng.random() < 0.7 else (rng.randrange(1, 4200), rng.randrange(1, 2300))), rng.choice([1, 1, 2, 3, 4, 32])
        same = rng.random() < 0.5
        sb, db = (A16, A16) if same else (bits(), bits())
        knob, reused = rng.choice(KNOBS) if rng.random() < 0.6 else 0, int(rng.random() < 0.3)
        dtype, nv12, nhwc = (rng.randrange(3) if rng.random() < 0.95 else rng.randrange(3, 9)), rng.randrange(2), rng.randrange(2)
        P = plan(L, kind, src, dst, w, h, n, sb, db, knob, reused, dtype, nv12, nhwc)
        what = (kind, src, dst, w, h, n, sb, db, knob, reused, dtype, nv12, nhwc)
        assert bool(P["ok"]) == legal(kind, src, dst, w, h, sb, db, knob, dtype, nv12, nhwc), what
        if not P["ok"]:
            continue
        name, has_one = forms[P["form"]][0], forms[P["form"]][1]
        assert P["na"] == len(forms[P["form"]][3]), what
        assert P["one"] == int(n == 1 and has_one), what
        assert preconditions(name, P, kind, src, dst, w, h, n, sb, db), (name, what)
        assert covers(name, P, w, h, n, dtype), (name, what, P)
        assert 1 <= P["gx"] < 2 ** 31 and 1 <= P["gy"] <= 65536 and 1 <= P["gz"] <= 65535, (name, what, P)
        assert P["ballast"] in ((0, 16) if name in ("k_nv12_rgb_p16", "k_nv12_rgb_p16x") and not P["one"] else (0,)), what
        assert not (P["ballast"] and not P["nts"]), what   # there is no allocating-store instantiation with ballast
        if kind == RELAYOUT:
            assert (P["swap_dst02"], P["swap_src02"]) == (int((src, dst) == (BGR, RGB_PLANAR)), int((src, dst) == (RGB_PLANAR, BGR))), what
            assert not (name == "k_relayout_generic" and P["mode"] > 12), what   # OP_PLANAR_SWAP has no instantiation
        else:
            assert not P["swap_src02"] and not P["swap_dst02"], what
        # knob 9 means the any-input kernel everywhere
        assert knob != 9 or name in ("k_yuv_rgb_generic", "k_rgb_yuv_quad", "k_tensor_yuv_quad", "k_relayout_generic"), what
        reached.add(name)
    assert reached == {f[0] for f in forms}


# ---- 4. the case table of the GPU test
def row_bytes(fmt, k, w):
    cw = (w + 1) // 2
    return {RGB: 3 * w, BGR: 3 * w, NV12: w if k == 0 else 2 * cw, YUV420: w if k == 0 else cw, YCBCR: w if k == 0 else cw, RGB_32F: 12 * w, RGB_32F_PLANAR: 4 * w,
            P10: 2 * w if k == 0 else 4 * cw, P12: 2 * w if k == 0 else 4 * cw}.get(fmt, w)


def classes_of(sf, df):
    """classify() and the launcher arguments of csrc/vpf_abi.hip"""
    yuv, rgb = {NV12: FC_NV12, YUV420: FC_YUV420, YUV444: FC_YUV444}, {RGB: FC_RGB, BGR: FC_BGR, RGB_PLANAR: FC_PLANAR}
    if sf in yuv and df in rgb:
        return YUV2RGB, yuv[sf], rgb[df]
    if sf in rgb and df in (YUV444, YUV420, YCBCR):
        return RGB2YUV, rgb[sf], FC_YUV444 if df == YUV444 else FC_YUV420
    return RELAYOUT, sf, df


def test_case_table(L, forms):
    reached = set()
    for name, entry, src, dst, w, h, n, knob, reused, soff, doff, labels in CASES:
        got = []
        for base in range(0, n, 32):   # vpf_convert_batch, vpf_tensor_convert_batch: 32 frames per dispatch
            m = min(32, n - base)
            db = [0x100 | doff] * 3
            if entry == "tensor":
                dtype, nhwc, _ = src
                P = plan(L, TENSOR2YUV, 0, 0, w, h, m, [0x100 | soff * (4 if dtype == 0 else 2)] * 3, db, knob, 0, dtype, dst == NV12, nhwc)
            else:
                kind, s, d = classes_of(src, dst)
                P = plan(L, kind, s, d, w, h, m, [0x100 | soff] * 3, db, knob, reused)
            assert P["ok"], name
            got.append(label_of(P, forms))
            reached.add(forms[P["form"]][0])
        assert got == labels, (name, got)
    assert reached == {f[0] for f in forms}   # every row of kConvertForms is reached by a legal call
