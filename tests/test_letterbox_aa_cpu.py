"""The antialiased letterbox into the tensor (vpf_convert_letterbox_tensor_aa, PySurfaceConvertResizer.ExecuteLetterboxAAToTensor,
letterbox_to_normalized_tensor(antialias=True)), without a GPU.  tests/c/aa_ref_capi.cpp compiles csrc/vpf_aa_plan.h — the header the kernels
include — with g++ -O2 -ffp-contract=off: the window properties the staged kernel relies on, the definition (aa_ref) against torch's antialias=True
and PIL's BILINEAR, constant sources, the properties of the launch plan over a generated grid, the refusals of the entry before any device access
and the register statistics of the twelve kernel instantiations.

Measured by test_cross_check_against_torch_and_pil (share of a case's bytes that differ by one LSB; no byte differs by more), noise / ramp:
  (h, w -> oh, ow)         torch float      PIL
  216, 384 ->  36,  64     0.00 / 0.00 %     8.7 / 20.1 %
  135, 240 ->  14,  14     0.00 / 0.00 %     5.3 /  2.4 %
   37,  53 ->   7,   9     0.00 / 0.00 %     7.4 /  4.8 %
   64,  96 ->  21,  32     0.00 / 0.00 %    10.3 /  2.4 %
   45,  80 ->  45,  13     0.00 / 0.57 %     0.0 /  1.7 %
   30,  30 ->  40,  11     0.00 / 0.00 %    20.3 /  6.1 %
   33,  47 ->  32,  46     0.02 / 0.00 %    18.8 /  8.8 %
   50,  70 ->   1,   1     0.00 / 0.00 %     0.0 /  0.0 %
   17,  19 ->   5,  19     0.00 / 0.00 %     0.0 /  0.0 %
(the test prints these figures; the conditions it asserts — 1 LSB everywhere, at most 2 % against torch's float path — are fixed)"""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from test_roi_tensor_cpu import _norm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
FC_NV12, FC_YUV420, FC_P16 = 0, 1, 7
AA_STRIP, AA_GATHER = 0, 1


def build_aa(tmp_dir):
    """tests/c/aa_ref_capi.cpp as a shared object with its prototypes set (the GPU tests use it too)"""
    from conftest import native_test_build
    so = os.path.join(str(tmp_dir), "libaaref.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-Wall", "-Werror", "-Wno-unused-function", *native_test_build()[0],
                           "-I" + os.path.join(ROOT, "videoprocessingframework_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "aa_ref_capi.cpp"), "-o", so, "-lm"])
    L = C.CDLL(so)
    u32, vp = C.c_uint32, C.c_void_p
    L.aa_c_axis.argtypes, L.aa_c_axis.restype = [u32, u32, vp], None
    L.aa_c_windows.argtypes, L.aa_c_windows.restype = [u32, u32, vp, vp, vp, vp, vp], None
    L.aa_c_window_bound.argtypes, L.aa_c_window_bound.restype = [u32, u32, u32], u32
    L.aa_c_strip_bytes.argtypes, L.aa_c_strip_bytes.restype = [u32, u32], u32
    L.aa_c_tile.argtypes, L.aa_c_tile.restype = [u32, vp], None
    for f in (L.aa_c_tiles, L.aa_c_cap, L.aa_c_strip_max):
        f.argtypes, f.restype = [], u32
    L.aa_c_plan.argtypes, L.aa_c_plan.restype = [C.c_int, C.c_int, u32, u32, u32, C.c_int, u32, vp, vp, vp], None
    L.aa_ref.argtypes, L.aa_ref.restype = [vp, vp, vp, u32, u32, u32, u32, u32, u32, u32, vp], None
    return L


@pytest.fixture(scope="module")
def aa(tmp_path_factory):
    return build_aa(tmp_path_factory.mktemp("aa"))


def windows(aa, n_in, n_out):
    lo, hi = np.empty(n_out, np.uint32), np.empty(n_out, np.uint32)
    S, c, cov = np.empty(n_out, F32), np.empty(n_out, F32), np.empty(n_in, np.uint8)
    aa.aa_c_windows(n_in, n_out, lo.ctypes.data, hi.ctypes.data, S.ctypes.data, c.ctypes.data, cov.ctypes.data)
    return lo.astype(np.int64), hi.astype(np.int64), S, c, cov


def aa_ref(aa, rgb, rect, iw, ih):
    """rgb: three [H, W] byte planes (or one [3, H, W] array) of the frame -> [3, ih, iw] bytes of the definition"""
    planes = [np.ascontiguousarray(p, dtype=np.uint8) for p in rgb]
    H, W = planes[0].shape
    x, y, w, h = rect
    assert x + w <= W and y + h <= H
    out = np.empty((3, ih, iw), np.uint8)
    aa.aa_ref(planes[0].ctypes.data, planes[1].ctypes.data, planes[2].ctypes.data, W, x, y, w, h, iw, ih, out.ctypes.data)
    return out


def tiles(aa):
    out = []
    for t in range(aa.aa_c_tiles()):
        o = np.zeros(3, np.uint32)
        aa.aa_c_tile(t, o.ctypes.data)
        out.append(tuple(int(v) for v in o))
    return out


def plan(aa, geoms, dw, dh, src_fc=FC_NV12, nhwc=0, dtype=0, variant=0, n=None):
    """-> (ok, dmask, [dispatch dicts], which)"""
    g = np.ascontiguousarray(np.array(geoms, np.uint32).reshape(-1, 4))
    n = len(g) if n is None else n
    out, which = np.zeros(15, np.uint32), np.full(max(n, 1) + 128, 255, np.uint8)
    aa.aa_c_plan(src_fc, nhwc, dtype, dw, dh, variant, n, g.ctypes.data, out.ctypes.data, which.ctypes.data)
    ds = [dict(zip(("form", "gx", "gy", "n", "tile", "lds"), (int(v) for v in out[3 + 6 * k:9 + 6 * k]))) for k in range(int(out[1]))]
    return int(out[0]), int(out[2]), ds, which[:n].copy()


# ------------------------------------------------------------------------------------------------ 1. the window
def test_window_properties(aa):
    """0 <= lo < hi <= in, hi - lo <= 2 ceil(fs) + 2, S >= 0.5, lo and hi non-decreasing in d (the staged kernel takes the windows of a tile's first
    and last pixel for the tile's); for s >= 1 every source index has a positive weight in at least one window"""
    pairs = [(i, o) for i in range(1, 161) for o in range(1, 49)] + [(3840, 640), (3840, 224), (2160, 360), (1920, 1), (1, 64)]
    ax = np.zeros(3, F32)
    for n_in, n_out in pairs:
        lo, hi, S, c, cov = windows(aa, n_in, n_out)
        aa.aa_c_axis(n_in, n_out, ax.ctypes.data)
        s, fs, inv = (float(v) for v in ax)
        assert F32(s) == F32(n_in) / F32(n_out) and fs == max(s, 1.0) and F32(inv) == F32(1.0) / F32(fs)
        assert (0 <= lo).all() and (lo < hi).all() and (hi <= n_in).all(), (n_in, n_out)
        assert (hi - lo <= 2 * math.ceil(fs) + 2).all(), (n_in, n_out)
        assert (S >= 0.5).all(), (n_in, n_out, float(S.min()))
        assert (np.diff(lo) >= 0).all() and (np.diff(hi) >= 0).all(), (n_in, n_out)
        if s >= 1.0:
            assert cov.all(), (n_in, n_out, np.flatnonzero(cov == 0)[:4])


# ------------------------------------------------------------------------------------------------ 2. torch and PIL
CROSS = [(216, 384, 36, 64), (135, 240, 14, 14), (37, 53, 7, 9), (64, 96, 21, 32), (45, 80, 45, 13), (30, 30, 40, 11), (33, 47, 32, 46), (50, 70, 1, 1),
         (17, 19, 5, 19)]


def _image(kind, h, w, seed):
    if kind == "noise":
        return np.random.default_rng(seed).integers(0, 256, (3, h, w), dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    return np.stack([(xx * 255 // max(w - 1, 1)), (yy * 255 // max(h - 1, 1)), ((xx + yy) * 7 % 256)]).astype(np.uint8)


@pytest.mark.parametrize("kind", ["noise", "ramp"])
def test_cross_check_against_torch_and_pil(aa, kind):
    """aa_ref against F.interpolate(float, mode="bilinear", antialias=True) rounded half up — every byte within 1 LSB, at most 2 % of a case's bytes
    different — and against PIL.Image.resize(BILINEAR), which rounds to bytes between its passes — every byte within 1 LSB.  The shares are printed
    (the module docstring and DESIGN.md 4.26 quote them)"""
    torch = pytest.importorskip("torch")
    Image = pytest.importorskip("PIL.Image")
    import torch.nn.functional as F

    for k, (h, w, oh, ow) in enumerate(CROSS):
        img = _image(kind, h, w, 100 + k)
        got = aa_ref(aa, img, (0, 0, w, h), ow, oh).astype(np.int32)
        t = F.interpolate(torch.from_numpy(img.astype(np.float32))[None], size=(oh, ow), mode="bilinear", antialias=True, align_corners=False)[0]
        tf = np.clip(np.floor(t.numpy().astype(np.float64) + 0.5), 0, 255).astype(np.int32)
        pil = np.stack([np.asarray(Image.fromarray(img[c]).resize((ow, oh), Image.BILINEAR)) for c in range(3)]).astype(np.int32)
        dt, dp = np.abs(got - tf), np.abs(got - pil)
        print(f"{kind} {h},{w}->{oh},{ow}: torch-float max {dt.max()} share {100.0 * (dt != 0).mean():.2f} %   PIL max {dp.max()} share {100.0 * (dp != 0).mean():.1f} %")
        assert dt.max() <= 1 and (dt != 0).mean() <= 0.02, (kind, h, w, oh, ow, int(dt.max()), float((dt != 0).mean()))
        assert dp.max() <= 1, (kind, h, w, oh, ow, int(dp.max()))


# ------------------------------------------------------------------------------------------------ 3. constants
def test_constant_source_gives_the_converted_byte(aa, oracle):
    """every (Y, U, V) on a grid of step 51, converted by the oracle's vpf_convert, through ratios 0.75, 1, 2.5, 6.3 and 17 on both axes: every picture
    pixel is exactly the converted byte (the weights are normalised by their own sum, so a constant survives the two folds)"""
    o = oracle
    vals = list(range(0, 256, 51))
    combos = [(y, u, v) for y in vals for u in vals for v in vals]
    W = 2 * len(combos)
    Y = np.repeat(np.array([c[0] for c in combos], np.uint8), 2)[None].repeat(2, 0)
    UV = np.array([[c[1], c[2]] for c in combos], np.uint8).reshape(1, W)
    triples = set()
    for cs, cr in ((0, 0), (1, 1)):
        st, rgb = o.convert(o.NV12, o.RGB_PLANAR, cs, cr, W, 2, [np.ascontiguousarray(Y), np.ascontiguousarray(UV)], o.FP32)
        assert st == 0
        triples |= {(int(rgb[0][0, 2 * i]), int(rgb[1][0, 2 * i]), int(rgb[2][0, 2 * i])) for i in range(len(combos))}
    assert len(triples) > 100
    for n_in, n_out in ((6, 8), (8, 8), (20, 8), (63, 10), (68, 4)):
        for t in sorted(triples):
            img = np.empty((3, n_in, n_in), np.uint8)
            for c in range(3):
                img[c] = t[c]
            got = aa_ref(aa, img, (0, 0, n_in, n_in), n_out, n_out)
            assert all((got[c] == t[c]).all() for c in range(3)), (n_in, n_out, t)


# ------------------------------------------------------------------------------------------------ 4. the plan
def _exact_tile_bytes(aa, n_in, n_out, td_w):
    """the widest window any run of td_w consecutive picture pixels has: (pixels, strip units for an even and for an odd rectangle origin)"""
    lo, hi, _, _, _ = windows(aa, n_in, n_out)
    a = np.arange(n_out)
    b = np.minimum(a + td_w - 1, n_out - 1)
    px = int((hi[b] - lo[a]).max())
    ng = 0
    for x in (0, 1):
        first, last = x + lo[a], x + hi[b] - 1
        ng = max(ng, int((((last - (first & ~1)) >> 3) + 1).max()))
    return px, ng


def test_plan_properties_over_a_grid(aa):
    """sources 1080p and 4K, destinations 224 and 640, rectangles from 8 px to the whole frame, both layouts: the launch never asks for more than 64 KiB;
    the strip a staged dispatch gets holds the exact window (walked with aa_window over every run of tile-width pixels, both parities of the
    rectangle's origin) of every tile of every one of its jobs; the grid covers the plane exactly; every job is in exactly one dispatch and keeps call
    order; knob 9 gives only the per-tap dispatch; both forms are reached"""
    cap, smax, T = aa.aa_c_cap(), aa.aa_c_strip_max(), tiles(aa)
    assert smax == 64 * 1024 and all(tw // npx * th == 256 for tw, th, npx in T)
    rng = np.random.default_rng(2026)
    exact = {}
    n_staged = n_gather = 0
    for (W, H) in ((1920, 1080), (3840, 2160)):
        for d in (224, 640):
            for nhwc in (0, 1):
                for size in (8, 24, 100, 224, 500, 900, 1500, None):
                    geoms = []
                    for j in range(10):
                        if size is None:
                            w, h = W, H
                        else:
                            w, h = min(W, int(size * rng.uniform(0.7, 1.5))), min(H, int(size * rng.uniform(0.7, 1.5)))
                        iw, ih = int(rng.integers(1, d + 1)), int(rng.integers(1, d + 1))
                        if j % 3 == 2:  # a thumbnail: large factors
                            iw, ih = int(rng.integers(1, d // 8 + 1)), int(rng.integers(1, d // 8 + 1))
                        elif rng.uniform() < 0.5:  # an aspect-preserving fit, as a caller computes it
                            if w * d >= h * d:
                                iw, ih = d, min(max((2 * h * d + w) // (2 * w), 1), d)
                            else:
                                ih, iw = d, min(max((2 * w * d + h) // (2 * h), 1), d)
                        geoms.append((w, h, iw, ih))
                    for variant in (0, 9):
                        ok, dmask, ds, which = plan(aa, geoms, d, d, nhwc=nhwc, variant=variant)
                        assert ok == 1 and dmask == 15 and 1 <= len(ds) <= 2
                        assert sum(x["n"] for x in ds) == len(geoms) and set(which) <= set(range(len(ds)))
                        assert [int((which == k).sum()) for k in range(len(ds))] == [x["n"] for x in ds]
                        if len(ds) == 2:
                            assert (ds[0]["form"], ds[1]["form"]) == (AA_STRIP, AA_GATHER)
                        if variant == 9:
                            assert len(ds) == 1 and ds[0]["form"] == AA_GATHER and ds[0]["lds"] == 0 and (which == 0).all()
                            continue
                        for k, x in enumerate(ds):
                            assert x["lds"] <= smax
                            if x["form"] == AA_GATHER:
                                assert (x["gx"], x["gy"], x["lds"]) == (((d + 3) // 4 + 63) // 64, (d + 3) // 4, 0)
                                n_gather += x["n"]
                                continue
                            tw, th, _ = T[x["tile"]]
                            assert (x["gx"], x["gy"]) == ((d + tw - 1) // tw, (d + th - 1) // th) and x["lds"] > 0
                            n_staged += x["n"]
                            for (w, h, iw, ih), wh in zip(geoms, which):
                                if wh != k:
                                    continue
                                for key in ((w, iw, tw), (h, ih, th)):
                                    if key not in exact:
                                        exact[key] = _exact_tile_bytes(aa, *key)
                                (px_x, ng), (px_y, _) = exact[(w, iw, tw)], exact[(h, ih, th)]
                                assert px_x <= aa.aa_c_window_bound(w, iw, tw) and px_y <= aa.aa_c_window_bound(h, ih, th), (w, h, iw, ih, x)
                                assert px_y * 32 * ng <= x["lds"], (w, h, iw, ih, x, px_y, ng)
                        # a job the plan sends per tap fits under no tile shape
                        for (w, h, iw, ih), wh in zip(geoms, which):
                            if ds[wh]["form"] == AA_GATHER:
                                tw, th, _ = T[-1]
                                assert aa.aa_c_strip_bytes(aa.aa_c_window_bound(w, iw, tw), aa.aa_c_window_bound(h, ih, th)) > smax
    print("staged jobs", n_staged, "per-tap jobs", n_gather)
    assert n_staged > 100 and n_gather > 100
    # the shapes of the issue: 4K -> 640 x 640 letterboxed (6 x) stages under the small tile, 1080p -> 640 (3 x) under the large one, 4K -> 224 (17 x) per tap
    assert plan(aa, [(3840, 2160, 640, 360)], 640, 640)[2] == [dict(form=AA_STRIP, gx=20, gy=80, n=1, tile=1, lds=plan(aa, [(3840, 2160, 640, 360)], 640, 640)[2][0]["lds"])]
    assert plan(aa, [(1920, 1080, 640, 360)], 640, 640)[2][0]["tile"] == 0
    assert plan(aa, [(3840, 2160, 224, 126)], 224, 224)[2][0]["form"] == AA_GATHER
    # call order inside a dispatch: `which` is all the launcher uses, and it appends job i behind the earlier jobs of its dispatch
    ok, _, ds, which = plan(aa, [(100, 100, 50, 50), (3840, 2160, 10, 10), (90, 90, 50, 50), (3840, 2160, 12, 12)], 64, 64)
    assert ok and list(which) == [0, 1, 0, 1] and [x["n"] for x in ds] == [2, 2]
    # refusals
    g = [(100, 100, 50, 50)]
    assert plan(aa, g * cap, 64, 64)[0] == 1 and plan(aa, g * (cap + 1), 64, 64)[0] == 0 and plan(aa, g, 64, 64, n=0)[0] == 0
    assert all(plan(aa, g, 64, 64, src_fc=fc)[0] == 1 for fc in (FC_NV12, FC_YUV420, FC_P16))
    assert all(plan(aa, g, 64, 64, src_fc=fc)[0] == 0 for fc in (2, 3, 4, 5, 6, 8, -1))
    assert plan(aa, g, 0, 64)[0] == 0 and plan(aa, g, 64, 65537)[0] == 0 and plan(aa, [(100, 100, 65, 50)], 64, 64)[0] == 0 and plan(aa, [(0, 100, 50, 50)], 64, 64)[0] == 0
    assert [plan(aa, g, 64, 64, nhwc=n, dtype=d)[1] for n in (0, 1) for d in (0, 1, 2)] == [15, 7, 7, 15, 15, 15]


# ------------------------------------------------------------------------------------------------ 5. the entry
def test_symbols_and_bindings_exist(capi):
    assert "vpf_convert_letterbox_tensor_aa" in capi.EXPORTS and hasattr(capi.lib(), "vpf_convert_letterbox_tensor_aa")
    nm = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert " vpf_convert_letterbox_tensor_aa\n" in nm
    assert callable(capi.convert_letterbox_tensor_aa)
    stubs = subprocess.run(["nm", "-C", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for src_fc in (FC_NV12, FC_YUV420, FC_P16):
        for dst_fc in (6, 8):  # FC_TENSOR, FC_TENSOR_NHWC
            for k in ("k_lbaa_strip", "k_lbaa_gather"):
                assert f"{k}<{src_fc}, {dst_fc}>" in stubs, (k, src_fc, dst_fc)
    sys.path.insert(0, os.path.join(ROOT, "videoprocessingframework_amd"))
    nvc = pytest.importorskip("PyNvCodec")
    assert hasattr(nvc.PySurfaceConvertResizer, "ExecuteLetterboxAAToTensor")
    stub = open(os.path.join(ROOT, "videoprocessingframework_amd", "PyNvCodec", "__init__.pyi")).read()
    assert "def ExecuteLetterboxAAToTensor(" in stub
    import inspect

    pytest.importorskip("torch")
    from videoprocessingframework_amd import PytorchNvCodec as pnc
    p = inspect.signature(pnc.letterbox_to_normalized_tensor).parameters["antialias"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False
    h = open(os.path.join(ROOT, "include", "vpf_hip.h")).read()
    assert h.index("VPF_API vpf_status vpf_convert_letterbox_tensor_aa(") > h.index("VPF_API vpf_status vpf_convert_letterbox_tensor(")


def test_validation_without_gpu(capi):
    """every refusal of vpf_convert_letterbox_tensor, answered by the antialiased entry before any device access: the plane pointers below are fake"""
    ex = capi.make_exec()
    W, H, dw, dh = 64, 32, 16, 8
    src = [(0x100000, 64), (0x200000, 64)]
    f32 = [(0x400000, 64), (0x500000, 64), (0x600000, 64)]  # dw * 4 = 64
    f16 = [(0x400000, 32), (0x500000, 32), (0x600000, 32)]
    rect, drect = (3, 5, 20, 10), (2, 1, 9, 5)

    def call(dst=f32, norm=None, sf=capi.NV12, cs=1, cr=0, s=src, size=(W, H, dw, dh), r=rect, d=drect, jobs=None, opts=None):
        jobs = capi.make_letterbox_jobs([(s, dst, r, d)] if jobs is None else jobs)
        return capi.convert_letterbox_tensor_aa(ex, sf, cs, cr, size[0], size[1], size[2], size[3], jobs, _norm(capi) if norm is None else norm, opts, check=False)

    for d in ((2, 1, 0, 5), (2, 1, 9, 0), (0, 0, 0, 0)):
        assert call(d=d) == capi.ERR_BAD_ARG, d
    for d in ((8, 1, 9, 5), (2, 4, 9, 5), (16, 0, 1, 1), (0, 8, 1, 1), (0, 0, 17, 8), (0, 0, 16, 9), (0xFFFFFFFF, 0, 2, 2), (0, 0xFFFFFFF0, 2, 0x20),
              (2, 0, 0xFFFFFFFF, 1)):
        assert call(d=d) == capi.ERR_BAD_ARG, d
    bad_opts = capi.make_letterbox_opts((1, 2, 3))
    bad_opts.reserved = 1
    assert call(opts=bad_opts) == capi.ERR_BAD_ARG
    assert call(sf=capi.RGB) == capi.ERR_UNSUPPORTED
    assert call(sf=capi.YUV444) == capi.ERR_UNSUPPORTED
    assert call(cs=2) == capi.ERR_UNSUPPORTED
    assert call(cr=2) == capi.ERR_UNSUPPORTED
    assert call(norm=_norm(capi, dtype=3)) == capi.ERR_UNSUPPORTED
    assert call(norm=_norm(capi, dtype=0xFFFFFFFF)) == capi.ERR_UNSUPPORTED
    assert call(norm=_norm(capi, flags=2)) == capi.ERR_UNSUPPORTED      # no flag bit asks for the filter: unknown bits stay unsupported
    assert call(norm=_norm(capi, flags=8)) == capi.ERR_UNSUPPORTED
    assert call(norm=_norm(capi, flags=capi.TENSOR_BGR | 0x80000000)) == capi.ERR_UNSUPPORTED
    L, Cb = capi.lib(), capi.C.byref
    good = capi.make_letterbox_jobs([(src, f32, rect, drect)] * 3)
    args = (capi.NV12, 1, 0, capi.Size(W, H), capi.Size(dw, dh), 3)
    assert L.vpf_convert_letterbox_tensor_aa(None, *args, good, Cb(_norm(capi)), None) == capi.ERR_BAD_ARG
    assert L.vpf_convert_letterbox_tensor_aa(Cb(ex), *args, None, Cb(_norm(capi)), None) == capi.ERR_BAD_ARG
    assert L.vpf_convert_letterbox_tensor_aa(Cb(ex), *args, good, None, None) == capi.ERR_BAD_ARG
    assert call(s=[(0, 64), (0x200000, 64)]) == capi.ERR_BAD_ARG
    assert call(s=src[:1]) == capi.ERR_BAD_ARG
    assert call(dst=f32[:2]) == capi.ERR_BAD_ARG
    assert capi.convert_letterbox_tensor_aa(ex, capi.NV12, 1, 0, W, H, dw, dh, good, _norm(capi), n=0, check=False) == capi.ERR_BAD_ARG
    for size in ((0, H, dw, dh), (W, 0, dw, dh), (W, H, 0, dh), (W, H, dw, 0), (70000, H, dw, dh), (W, H, 70000, dh)):
        assert call(size=size) == capi.ERR_BAD_ARG, size
    for r in ((3, 5, 0, 10), (3, 5, 20, 0), (45, 5, 20, 10), (3, 23, 20, 10), (0xFFFFFFFF, 0, 2, 2)):
        assert call(r=r) == capi.ERR_BAD_ARG, r
    assert call(s=[(0x100000, 63), (0x200000, 64)]) == capi.ERR_BAD_ARG
    for dt, planes, elem in ((capi.TENSOR_F32, f32, 4), (capi.TENSOR_F16, f16, 2)):
        for k in range(3):
            p = list(planes)
            p[k] = (planes[k][0] + 1, planes[k][1])
            assert call(dst=p, norm=_norm(capi, dtype=dt)) == capi.ERR_BAD_ARG, (dt, k, "pointer")
            p[k] = (planes[k][0], dw * elem - elem)
            assert call(dst=p, norm=_norm(capi, dtype=dt)) == capi.ERR_BAD_ARG, (dt, k, "short pitch")
    nhwc = _norm(capi, flags=capi.TENSOR_NHWC)
    assert call(dst=[(0x400000, 3 * dw * 4 - 4), (0, 0), (0, 0)], norm=nhwc) == capi.ERR_BAD_ARG
    for bad in (math.nan, math.inf):
        sc = [0.01, bad, 0.01]
        assert call(norm=_norm(capi, scale=sc)) == capi.ERR_BAD_ARG
        assert call(norm=_norm(capi, bias=sc)) == capi.ERR_BAD_ARG
    # one bad job among good ones, beyond the first two job tables: everything is validated before the first launch
    jobs = [(src, f32, rect, drect)] * 200 + [(src, f32, rect, (8, 1, 9, 5))]
    assert call(jobs=jobs) == capi.ERR_BAD_ARG
    with pytest.raises(capi.VpfError):
        capi.convert_letterbox_tensor_aa(ex, capi.NV12, 1, 0, W, H, dw, dh, capi.make_letterbox_jobs([(src, f32, rect, (8, 1, 9, 5))]), _norm(capi))


# ------------------------------------------------------------------------------------------------ 6. registers
@pytest.mark.timeout(900)
def test_the_twelve_instantiations_spill_nothing_and_use_no_scratch():
    """resource metadata of the code object only (tools/isa_stats.spills): both forms, both layouts, NV12, YUV420 and P10 / P12 — no spilled register
    (vector or scalar), no scratch, at most 128 VGPRs (two workgroups of 256 lanes per SIMD)"""
    import re

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_stats

    rows = [r for r in isa_stats.spills(os.path.join(ROOT, "videoprocessingframework_amd", "csrc", "k_convert_letterbox_aa.hip"))
            if re.search(r"k_lbaa_(strip|gather)<[017], [68]>", r[0])]
    assert len(rows) == 12 and len({r[0] for r in rows}) == 12, [r[0] for r in rows]
    for name, vgpr, vspill, sspill, scratch in rows:
        print(name[:100], "vgpr", vgpr)
        assert vspill == 0 and sspill == 0 and scratch == 0, (name, vgpr, vspill, sspill, scratch)
        assert vgpr <= 128, (name, vgpr)
