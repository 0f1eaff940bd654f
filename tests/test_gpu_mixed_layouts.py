"""-m gpu: the 8-bit entries of the C ABI on planes that do NOT all lie alike (tests/cases_mixed_layouts.py): per call every plane of every
frame gets a pointer alignment and a pitch of its own — pitch-only (P), one odd plane (O), stacked in one allocation (S), and a seeded family.

Bar, per case: BIT-EXACT against the oracle's FP32 mode on the tight planes; within 1 LSB of its EXACT mode for the converters and the linear /
Lanczos filters (the bar of _convert / _resize in tests/test_gpu_parity.py; nearest is exempt as there; the fused entries' SEEDED family:
per link, see cases_mixed_layouts.reference); every byte that is not a pixel — row padding, lead, tail, the gaps of stacked planes —
untouched on every destination AND every source; remap destinations start filled with 77 and out-of-range pixels keep it.  test_reach_of_the_cases reads the launch log of a child process: a test of layouts proves nothing unless the
layouts really steer the kernel selection."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # -m gpu on a box without a GPU: fail loudly rather than pass vacuously
    pytest.skip("no GPU visible", allow_module_level=True)

import cases_mixed_layouts as cm  # noqa: E402
from gpu_util import LaidOutPlanes, stream_handle  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_FIRST = int(os.environ.get("VPF_FUZZ_FIRST", "0"))
_FUZZ_SEEDS = range(_FIRST, _FIRST + int(os.environ.get("VPF_FUZZ_SEEDS", "16")))  # the directed cases carry the weight
FILL = 77
_WANT = {}


def expected(oracle, case, j):
    """(tight source planes, FP32 planes, EXACT planes) of distinct frame j of the call: computed once, shared, never written to"""
    key = (case["entry"], case["sf"], case["df"], case["cs"], case["cr"], case["interp"], case["sw"], case["sh"], case["dw"], case["dh"], case["seed"], j, case["kind"] == "F")
    if key not in _WANT:
        src = oracle.synth(case["sf"], case["sw"], case["sh"], case["seed"] + j)
        maps = cm.remap_maps(case) if case["entry"] == "remap" else None
        fp32, exact = cm.reference(oracle, case, src, maps)
        for p in src + fp32 + exact:
            p.setflags(write=False)
        _WANT[key] = (src, fp32, exact)
    return _WANT[key]


def device_maps(case):
    """the two maps where case["maps"] puts them: (keep-alive, xmap pointer, ymap pointer)"""
    m, keep, ptrs = case["maps"], [], []
    for a, pitch, off in zip(cm.remap_maps(case), (m["xp"], m["yp"]), (m["xoff"], m["yoff"])):
        h = np.zeros(off + case["dh"] * pitch + 64, np.uint8)
        np.lib.stride_tricks.as_strided(h[off:], shape=(case["dh"], 4 * case["dw"]), strides=(pitch, 1))[...] = a.view(np.uint8)
        t = torch.from_numpy(h).cuda()
        assert t.data_ptr() % 256 == 0
        keep.append(t)
        ptrs.append(t.data_ptr() + off)
    return keep, ptrs[0], ptrs[1]


def run_case(capi, oracle, case):
    what = cm.describe(case)
    n, distinct = case["n"], min(case["n"], 3)
    df, dw, dh = cm.side_shape(case, "dst")
    S, D = [], []
    for i in range(n):
        layouts, stacked = cm.layout_args(case["src"][i])
        S.append(LaidOutPlanes(expected(oracle, case, i % distinct)[0], layouts, stacked))
        layouts, stacked = cm.layout_args(case["dst"][i])
        D.append(LaidOutPlanes(oracle.alloc(df, dw, dh, fill=FILL if case["entry"] == "remap" else None), layouts, stacked))
    keep, maps = None, None
    if case["entry"] == "remap":
        keep, *maps = device_maps(case)
    elif case["api"] == "batch_ws":
        nbytes = capi.resize_workspace_bytes(case["sf"], case["interp"], case["sw"], case["sh"], dw, dh)
        keep = torch.zeros(nbytes + 256, dtype=torch.uint8, device="cuda")
        maps = capi.make_workspace((keep.data_ptr() + 255) // 256 * 256, nbytes)
    torch.cuda.synchronize()
    st = cm.launch(capi, capi.make_exec(stream_handle()), case, [s.desc() for s in S], [d.desc() for d in D], maps)
    torch.cuda.synchronize()
    assert st == capi.OK, f"status {st}: {what}"
    for i in range(n):
        src, want, exact = expected(oracle, case, i % distinct)
        got, intact = D[i].download()
        assert intact, f"frame {i}: wrote outside the destination's pixels: {what}"
        back, intact = S[i].download()
        assert intact and all(np.array_equal(a, b) for a, b in zip(back, src)), f"frame {i}: the source changed: {what}"
        for k, (g, w, e) in enumerate(zip(got, want, exact)):
            if not np.array_equal(g, w):
                d = np.argwhere(g != w)
                first = tuple(d[0])
                raise AssertionError(f"frame {i} plane {k} differs at {len(d)} of {g.size} elements; first at {first}: got {g[first]} want {w[first]}: {what}")
            if g.dtype == np.uint8 and not (case["entry"] == "resize" and case["interp"] == cm.NEAREST):
                err = int(np.abs(g.astype(np.int16) - e.astype(np.int16)).max())
                assert err <= 1, f"frame {i} plane {k}: {err} LSB from EXACT: {what}"


@pytest.mark.parametrize("key", cm.KEYS["convert"])
def test_convert_mixed_layouts(capi, oracle, key):
    for case in cm.directed("convert", key):
        run_case(capi, oracle, case)


@pytest.mark.parametrize("key", cm.KEYS["resize"])
def test_resize_batch_mixed_layouts(capi, oracle, key):
    for case in cm.directed("resize", key):
        run_case(capi, oracle, case)


@pytest.mark.parametrize("key", cm.KEYS["fused"])
def test_convert_resize_mixed_layouts(capi, oracle, key):
    for case in cm.directed("fused", key):
        run_case(capi, oracle, case)


@pytest.mark.parametrize("key", cm.KEYS["remap"])
def test_remap_mixed_layouts(capi, oracle, key):
    for case in cm.directed("remap", key):
        run_case(capi, oracle, case)


@pytest.mark.parametrize("seed", _FUZZ_SEEDS)  # soak: VPF_FUZZ_SEEDS=500 (VPF_FUZZ_FIRST=n: seeds n .. n + VPF_FUZZ_SEEDS - 1, fresh cases)
@pytest.mark.parametrize("entry", cm.ENTRIES)
def test_fuzz_mixed_layouts(capi, oracle, entry, seed):
    for case in cm.cases(entry, seed):
        run_case(capi, oracle, case)


def test_contiguous_tensor_through_the_python_api(oracle):
    """PytorchNvCodec.surface_from_tensor wraps a contiguous [3, 227, 227] uint8 tensor as RGB_PLANAR with pitch 227 and planes at
    base + i * 227 * 227: three planes in three alignment classes.  PySurfaceConverter takes RGB_PLANAR -> YUV420 as a pair of its own
    (Tasks.cpp: rgb_planar_yuv420), so the RGB -> YUV launcher — the one with the per-plane chroma masks — reads the three planes directly;
    then YUV420 -> NV12.  The encode sample's route RGB_PLANAR -> RGB -> YUV420 -> NV12 is the second chain (the de-interleaving kernel reads
    them), PySurfaceResizer the third.  Each equals the oracle's pixels."""
    sys.path.insert(0, os.path.join(ROOT, "videoprocessingframework_amd"))
    import PyNvCodec as nvc
    import PytorchNvCodec as pnvc

    PF, w, h = nvc.PixelFormat, 227, 227
    pln = oracle.synth(oracle.RGB_PLANAR, w, h, 500)
    t = torch.from_numpy(np.stack(pln)).cuda()
    assert t.is_contiguous() and len({(t.data_ptr() + i * w * h) % 4 for i in range(3)}) == 3
    torch.cuda.synchronize()
    surf = pnvc.surface_from_tensor(t)
    assert surf.Format() == PF.RGB_PLANAR and surf.PlanePtr().GpuMem() == t.data_ptr()
    cc = nvc.ColorspaceConversionContext(nvc.ColorSpace.BT_601, nvc.ColorRange.MPEG)

    def download(s):
        out = np.zeros(1, np.uint8)
        assert nvc.PySurfaceDownloader(s.Width(), s.Height(), s.Format(), 0).DownloadSingleSurface(s, out)
        return out

    def flat(planes):
        return np.concatenate([p.reshape(-1) for p in planes])

    yuv = nvc.PySurfaceConverter(w, h, PF.RGB_PLANAR, PF.YUV420, 0).Execute(surf, cc)
    _, b = oracle.convert(oracle.RGB_PLANAR, oracle.YUV420, 0, 0, w, h, pln)
    assert np.array_equal(download(yuv), flat(b))
    nv12 = nvc.PySurfaceConverter(w, h, PF.YUV420, PF.NV12, 0).Execute(yuv, cc)
    _, c = oracle.convert(oracle.YUV420, oracle.NV12, 0, 0, w, h, b)
    assert np.array_equal(download(nv12), flat(c))
    rgb = nvc.PySurfaceConverter(w, h, PF.RGB_PLANAR, PF.RGB, 0).Execute(surf, cc)
    yuv = nvc.PySurfaceConverter(w, h, PF.RGB, PF.YUV420, 0).Execute(rgb, cc)
    nv12 = nvc.PySurfaceConverter(w, h, PF.YUV420, PF.NV12, 0).Execute(yuv, cc)
    _, a = oracle.convert(oracle.RGB_PLANAR, oracle.RGB, 0, 0, w, h, pln)
    _, b = oracle.convert(oracle.RGB, oracle.YUV420, 0, 0, w, h, a)
    _, c = oracle.convert(oracle.YUV420, oracle.NV12, 0, 0, w, h, b)
    assert np.array_equal(download(nv12), flat(c))
    small = nvc.PySurfaceResizer(113, 113, PF.RGB_PLANAR, 0).Execute(surf)
    _, want = oracle.resize(oracle.RGB_PLANAR, oracle.LANCZOS3, w, h, pln, 113, 113)   # (the resizer's filter, as the reference's: Lanczos)
    assert np.array_equal(download(small), flat(want))
    assert np.array_equal(t.cpu().numpy(), np.stack(pln))   # the wrapped tensor is a source only


# ------------------------------------------------------------------------------------------------ reach
_CHILD = """
import sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import torch
from videoprocessingframework_amd import capi
import cases_mixed_layouts as cm
from gpu_util import plane_geometry
ex = capi.make_exec(torch.cuda.current_stream().cuda_stream)
keep = []
def alloc(nbytes):
    t = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    assert t.data_ptr() % 256 == 0
    keep.append(t)
    return t.data_ptr()
def descs(case, side):
    fmt, w, h = cm.side_shape(case, side)
    shapes = [(rows, rb) for rows, rb, _ in cm.plane_shapes(fmt, w, h)]
    out = []
    for fl in case[side]:
        sizes, planes = plane_geometry(shapes, *cm.layout_args(fl))
        bases = [alloc(s) for s in sizes]
        out.append([(bases[a] + off, pitch) for a, off, pitch, _, _ in planes])
    return out
for tag, case in cm.reach_cases():
    del keep[:]
    maps = None
    if case["entry"] == "remap":
        m = case["maps"]
        maps = (alloc(m["xoff"] + case["dh"] * m["xp"] + 64) + m["xoff"], alloc(m["yoff"] + case["dh"] * m["yp"] + 64) + m["yoff"])
    S, D = descs(case, "src"), descs(case, "dst")
    torch.cuda.synchronize()
    print("CASE " + tag, file=sys.stderr, flush=True)
    st = cm.launch(capi, ex, case, S, D, maps)
    torch.cuda.synchronize()
    assert st == capi.OK, (st, tag)
print("done")
"""


def test_reach_of_the_cases():
    """What the cases reach, from the launch log (VPF_HIP_LOG=2) of a child that makes every directed call once on zero-filled planes:
    - a (P) case logs exactly the launches of the same call on uniform A256 planes: a pitch never changes the kernel;
    - vpf_convert(_batch): ONE odd plane takes the same kernel as the uniform call exactly when it is on the top tier of its gate's thresholds
      (cases_mixed_layouts.CONVERT), and two rungs of one plane take the same kernel exactly when they are on the same tier;
    - the other entries: an odd plane on the bottom rung of its ladder (A1; float planes A4) takes another kernel than the uniform call, unless its gate only sets a runtime
      flag of the same kernel (flag_only) or the uniform call already takes the most general kernel — which is read from the launcher
      itself: the log of the uniform call under the forced-generic tuning value 9;
    - per entry and format family (resize: per filter) some (O) case leaves the uniform call's kernel, wherever there is one to leave;
    - Lanczos NV12 with only the UV source plane odd: the matrix-core kernel AND a gather launch (the per-plane fallback of
      launch_resize_planned); bilinear YUV420 with one odd chroma plane: more than one launch where the uniform call makes one."""
    code = _CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, VPF_HIP_LOG="2"), timeout=600)
    assert r.returncode == 0 and "done" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    logs, tag = {}, None
    for line in r.stderr.splitlines():
        if line.startswith("CASE "):
            tag = line[5:]
            logs[tag] = []
        elif line.startswith("libvpfhip: launch ") and tag is not None:
            logs[tag].append(line[len("libvpfhip: launch "):])
    for entry, names in cm.kernels_seen(logs).items():
        print(f"reach of {entry}: {len(names)} kernels: {', '.join(names)}")
    cm.check_reach(logs)
