"""The antialiased letterbox's definition against three things that do not share its code, without a GPU.

aa_ref (tests/c/aa_ref_capi.cpp) is the ground truth of every GPU test of vpf_convert_letterbox_tensor_aa, and it compiles csrc/vpf_aa_plan.h — the
header the kernels include: a slip in aa_window, aa_weight or aa_pixel would be shared by the kernels and their reference.  Here:

  1. tests/aa_definition.py::aa_definition_u8 — the comment of include/vpf_hip.h restated in numpy float32 as two passes, with an fma built from
     float64 (checked bit for bit against libm's fmaf, float32 midpoints included) — must equal aa_ref BYTE FOR BYTE on every job of the
     letterbox_aa family's 64 default seeds (tests/cases_tensor_fuzz.py) and on an axis grid: every (in, out) of 1 .. 160 x 1 .. 48 and four large
     pairs, as in x 1 -> out x 1 and 1 x in -> 1 x out strips of noise.  No tolerance: a difference means the header's text and csrc/vpf_aa_plan.h
     disagree, and the text is the contract.
  2. aa_ref against triangle_f64_u8, the plain float64 triangle filter: no byte more than 1 apart on every job of the default seeds (the claim of
     DESIGN.md 4.26).  Measured share of differing bytes (printed, not asserted): 0.07 % of 4 891 479 bytes.
  3. aa_ref against torch's F.interpolate(float64, mode="bilinear", antialias=True) rounded half up, on the jobs whose picture is wider AND taller
     than one pixel: no byte more than 1 apart, and at most 2 % of all compared bytes, summed over the family, differ (the project's figure of
     tests/test_letterbox_aa_cpu.py, on the aggregate so that a 1 x 2 picture cannot fail on one tie).  Measured: 0.07 % of 4 862 169 bytes.

Which pictures torch gets wrong (torch 2.10, CPU, float64 and float32 alike; test_torch_deviates_on_one_pixel_wide_pictures): a picture ONE PIXEL
WIDE whose height is resampled — iw == 1, ih > 1 and ih != h, up-scaled or down-scaled, whatever the rectangle's width (w == 1 included) — is up to
158 codes off the float64 filter on noise, where the definition is within 1.  The transpose (ih == 1, the width resampled) is right, as are
iw == 1 with ih == h and 1 x 1 pictures.  The family's torch comparison leaves out every picture with iw == 1 or ih == 1."""
import ctypes as C
import ctypes.util

import numpy as np
import pytest

import cases_tensor_fuzz as cases
from aa_definition import aa_definition_u8, fmaf32, triangle_f64_u8
from test_letterbox_aa_cpu import aa_ref, build_aa
from test_tensor_fuzz_cases_cpu import SEEDS, forget_p16, host_frames, rgb_frames

F32 = np.float32
P16 = ("P10", "P12")


@pytest.fixture(scope="module")
def aa(tmp_path_factory):
    return build_aa(tmp_path_factory.mktemp("aa_def"))


# ------------------------------------------------------------------------------------------------ the fma
def adversarial_triples(rng, n):
    """a * b + c that lands ON a float32 midpoint between c and its neighbour (ties to even), and a hair below and above it — by a factor of
    1 -+ 2^-46 of half an ulp: 2^-70 of c, which the float64 sum cannot hold, so that a cast of the float64 a * b + c rounds twice"""
    c = (rng.integers(1 << 23, 1 << 24, n).astype(np.float64) * 2.0 ** rng.integers(-40, 40, n)).astype(F32)   # 24-bit mantissas, odd and even
    e = np.frexp(c.astype(np.float64))[1] - 1                  # c = 1.m x 2^e: half an ulp is 2^(e - 24)
    k = rng.integers(-20, 20, n)
    a0, b0 = np.ldexp(1.0, k), np.ldexp(1.0, e - 24 - k)
    up, dn = 1.0 + 2.0 ** -23, 1.0 - 2.0 ** -23
    out = []
    for fa, fb in ((1.0, 1.0), (up, dn), (up, up), (dn, dn), (up, 1.0), (dn, 1.0)):
        for sign in (1.0, -1.0):
            for csign in (1.0, -1.0):
                out.append(((a0 * fa).astype(F32), (sign * b0 * fb).astype(F32), (csign * c).astype(F32)))
    return tuple(np.concatenate([t[i] for t in out]) for i in range(3))


def test_fmaf32_is_libm_fmaf():
    """bit for bit, on random triples of several magnitudes, on products that cancel the addend, and on the adversarial midpoints"""
    libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.fmaf.argtypes, libm.fmaf.restype = [C.c_float] * 3, C.c_float
    rng = np.random.default_rng(77)
    sets = [adversarial_triples(rng, 600)]
    for scale in (1.0, 1e-3, 1e4):
        sets.append(tuple((rng.standard_normal(3000) * s).astype(F32) for s in (scale, 1.0, scale)))
    a, b = rng.standard_normal(3000).astype(F32), rng.standard_normal(3000).astype(F32)
    sets.append((a, b, (-(a * b)).astype(F32)))                                           # a * b + c cancels to the product's rounding error
    w = rng.integers(0, 1 << 24, 3000).astype(np.float64) * 2.0 ** -24                    # the folds' own operands: weights, bytes, accumulators
    sets.append((w.astype(F32), rng.integers(0, 256, 3000).astype(F32), (rng.uniform(0, 2000, 3000)).astype(F32)))
    wrong_naive = 0
    for a, b, c in sets:
        got = fmaf32(a, b, c)
        want = np.array([libm.fmaf(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], F32)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), [(x, y, z) for x, y, z, g, v in zip(a, b, c, got, want) if g != v][:3]
        naive = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)
        wrong_naive += int((naive.view(np.uint32) != want.view(np.uint32)).sum())
    print("triples on which the cast of the float64 a * b + c is NOT fmaf:", wrong_naive)
    assert wrong_naive > 100   # the adversarial set does its work: the correction is needed, and checked


# ------------------------------------------------------------------------------------------------ the axis grid
GRID = [(i, o) for i in range(1, 161) for o in range(1, 49)] + [(3840, 640), (2160, 360), (1920, 1), (1, 64)]


def test_definition_equals_aa_ref_on_the_axis_grid(aa):
    rng = np.random.default_rng(4026)
    for n_in, n_out in GRID:
        row = rng.integers(0, 256, (3, 1, n_in), dtype=np.uint8)
        col = np.ascontiguousarray(row.transpose(0, 2, 1))
        for img, rect, iw, ih in ((row, (0, 0, n_in, 1), n_out, 1), (col, (0, 0, 1, n_in), 1, n_out)):
            want, got = aa_ref(aa, img, rect, iw, ih), aa_definition_u8(img, rect, iw, ih)
            assert np.array_equal(got, want), (n_in, n_out, rect, np.argwhere(got != want)[:4].tolist())


# ------------------------------------------------------------------------------------------------ the family's jobs
def torch_f64_u8(torch, rgb, rect, iw, ih, dtype=None):
    import torch.nn.functional as Fn
    x, y, w, h = rect
    t = torch.from_numpy(np.stack(rgb)[:, y:y + h, x:x + w].astype(np.float64)).to(dtype or torch.float64)
    t = Fn.interpolate(t[None], size=(ih, iw), mode="bilinear", antialias=True, align_corners=False)[0]
    return np.clip(np.floor(t.numpy().astype(np.float64) + 0.5), 0, 255).astype(np.uint8)


@pytest.fixture(scope="module")
def family_pass(aa, oracle):
    """ONE pass over every job of the default seeds: aa_ref against the definition, the float64 filter and torch; what each test below asserts"""
    try:
        import torch
    except ImportError:
        torch = None
    oracle.set_threads(16)
    out = dict(jobs=0, unequal=[], f64_far=[], f64_bytes=0, f64_diff=0, torch_far=[], torch_bytes=0, torch_diff=0, torch=torch is not None)
    done = {}
    for seed in SEEDS:
        for k, call in enumerate(cases.cases("letterbox_aa", seed)):
            rgb = rgb_frames(oracle, call, host_frames(oracle, call))
            done.clear()
            for i, job in enumerate(call["jobs"]):
                rect, (_, _, iw, ih) = job["rect"], job["dst_rect"]
                key = (job["frame"], rect, iw, ih)
                if key in done:
                    continue
                done[key] = True
                what = f"seed {seed} case {k} job {i} frame {call['W']} x {call['H']} rect {rect} -> {iw} x {ih}"
                frame = rgb[job["frame"]]
                ref = aa_ref(aa, frame, rect, iw, ih)
                out["jobs"] += 1
                if not np.array_equal(aa_definition_u8(frame, rect, iw, ih), ref):
                    out["unequal"].append(what)
                d = np.abs(ref.astype(np.int16) - triangle_f64_u8(frame, rect, iw, ih).astype(np.int16))
                out["f64_bytes"], out["f64_diff"] = out["f64_bytes"] + d.size, out["f64_diff"] + int((d != 0).sum())
                if d.max() > 1:
                    out["f64_far"].append((what, int(d.max())))
                if torch is not None and iw > 1 and ih > 1:
                    d = np.abs(ref.astype(np.int16) - torch_f64_u8(torch, frame, rect, iw, ih).astype(np.int16))
                    out["torch_bytes"], out["torch_diff"] = out["torch_bytes"] + d.size, out["torch_diff"] + int((d != 0).sum())
                    if d.max() > 1:
                        out["torch_far"].append((what, int(d.max())))
            if call["sf"] in P16:
                forget_p16()
    return out


def test_definition_equals_aa_ref_on_the_family(family_pass):
    """byte for byte, every distinct (frame, rectangle, picture) of every call of the 64 default seeds"""
    print("letterbox_aa: distinct jobs compared", family_pass["jobs"])
    assert family_pass["jobs"] > 1000 and not family_pass["unequal"], family_pass["unequal"][:5]


def test_aa_ref_is_within_one_of_the_float64_filter(family_pass):
    """a condition: no byte more than 1 from the plain float64 triangle filter.  The share of differing bytes is a measurement"""
    p = family_pass
    print(f"aa_ref against the float64 triangle filter: {p['f64_diff']} of {p['f64_bytes']} bytes differ ({100.0 * p['f64_diff'] / p['f64_bytes']:.2f} %)")
    assert not p["f64_far"], p["f64_far"][:5]


def test_aa_ref_against_torch(family_pass):
    """pictures wider and taller than one pixel: no byte more than 1 from torch's float64 path rounded half up, at most 2 % of ALL compared bytes differ"""
    pytest.importorskip("torch")
    p = family_pass
    print(f"aa_ref against torch float64: {p['torch_diff']} of {p['torch_bytes']} bytes differ ({100.0 * p['torch_diff'] / max(p['torch_bytes'], 1):.2f} %)")
    assert p["torch_bytes"] > 100000 and not p["torch_far"], p["torch_far"][:5]
    assert p["torch_diff"] <= 0.02 * p["torch_bytes"]


def test_torch_deviates_on_one_pixel_wide_pictures(aa):
    """why the comparison above leaves pictures of one pixel's width out: on 7 x 3 -> 1 x 5 (and 7 x 2 -> 1 x 3, 60 x 52 -> 1 x 64, 1 x 9 -> 1 x 4)
    torch is many codes off the float64 triangle filter, in float64 and float32 alike, while aa_ref EQUALS the float64 filter there; the transposed
    shapes, and a width of one with the height kept, are within 1 of torch"""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(5)
    for w, h, iw, ih in ((7, 3, 1, 5), (7, 2, 1, 3), (60, 52, 1, 64), (1, 9, 1, 4)):
        img = rng.integers(0, 256, (3, h, w), dtype=np.uint8)
        f64, ref = triangle_f64_u8(img, (0, 0, w, h), iw, ih), aa_ref(aa, img, (0, 0, w, h), iw, ih)
        assert np.abs(ref.astype(np.int16) - f64.astype(np.int16)).max() <= 1, (w, h, iw, ih)
        if (w, h, iw, ih) == (7, 3, 1, 5):
            assert np.array_equal(ref, f64)
        for dtype in (torch.float64, torch.float32):
            off = int(np.abs(torch_f64_u8(torch, img, (0, 0, w, h), iw, ih, dtype).astype(np.int16) - f64.astype(np.int16)).max())
            print(f"{w} x {h} -> {iw} x {ih} {dtype}: torch is {off} codes off the float64 filter")
            assert off > 1, (w, h, iw, ih, dtype, off)
        # the transpose, and the same width of one with the height kept: torch agrees
        t = np.ascontiguousarray(img.transpose(0, 2, 1))
        for im, (ww, hh, ow, oh) in ((t, (h, w, ih, iw)), (img, (w, h, 1, h))):
            d = np.abs(torch_f64_u8(torch, im, (0, 0, ww, hh), ow, oh).astype(np.int16) - triangle_f64_u8(im, (0, 0, ww, hh), ow, oh).astype(np.int16))
            assert d.max() <= 1, (ww, hh, ow, oh)
