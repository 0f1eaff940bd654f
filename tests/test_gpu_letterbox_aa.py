"""The antialiased letterbox into the tensor on the MI355X: vpf_convert_letterbox_tensor_aa, PySurfaceConvertResizer.ExecuteLetterboxAAToTensor and
PytorchNvCodec.letterbox_to_normalized_tensor(antialias=True).

Ground truth is the definition, composed: the CPU oracle's conversion of the whole frame to RGB_PLANAR (P10: of the narrowed planes), aa_ref of
tests/c/aa_ref_capi.cpp — csrc/vpf_aa_plan.h, the header the kernels include, compiled with g++ -ffp-contract=off — on the job's rectangle, the pad
around it (place of tests/test_gpu_letterbox_tensor.py) and reference_bits of tests/test_gpu_tensor_out.py.  Every element of every output must be
bit-identical; there is no tolerance.  Sources and destinations live in gpu_util.LaidOutPlanes: every byte that is no element of a destination —
row padding, leads, tails, the sources' own — must still hold the canary afterwards."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import test_gpu_p16_tensor as p16
from gpu_util import LaidOutPlanes, stream_handle
from test_gpu_letterbox_tensor import place
from test_gpu_tensor_nhwc import hwc
from test_gpu_tensor_out import ELEM, PARAMS, assert_bits, reference_bits
from test_letterbox_aa_cpu import AA_GATHER, AA_STRIP, aa_ref, build_aa, plan

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = (114, 7, 250)   # three different values: a channel mix-up shows
NPDT = {0: np.uint32, 1: np.uint16, 2: np.uint16}

# (name, source, colour space, range, frame, destination, dtype, bgr, nhwc, destination layout (align, extra, offset))
CASES = [
    ("nv12", "NV12", 1, 0, (194, 130), (70, 37), 0, False, False, (64, 0, 0)),
    ("nv12_nhwc", "NV12", 1, 0, (194, 130), (70, 37), 0, False, True, (64, 0, 0)),
    ("yuv420", "YUV420", 0, 1, (193, 129), (64, 48), 0, False, False, (64, 0, 0)),
    ("yuv420_nhwc", "YUV420", 0, 1, (193, 129), (64, 48), 0, False, True, (4, 4, 4)),
    ("p10", "P10", 1, 0, (193, 129), (70, 37), 0, False, False, (4, 8, 4)),
    ("p10_nhwc", "P10", 1, 0, (193, 129), (70, 37), 0, False, True, (64, 0, 0)),
    ("nv12_f16", "NV12", 1, 1, (193, 129), (64, 48), 1, False, False, (64, 0, 0)),
    ("yuv420_bf16", "YUV420", 1, 0, (194, 130), (70, 37), 2, False, False, (64, 0, 0)),
    ("p10_bgr", "P10", 0, 0, (194, 130), (64, 48), 0, True, False, (64, 0, 0)),
    ("nv12_nhwc_bgr_f16", "NV12", 1, 0, (194, 130), (64, 48), 1, True, True, (64, 0, 0)),
]
CASE = {c[0]: c for c in CASES}


@pytest.fixture(scope="module")
def orc(oracle):
    oracle.set_threads(16)
    return oracle


@pytest.fixture(scope="module")
def aa(tmp_path_factory):
    return build_aa(tmp_path_factory.mktemp("aa_gpu"))


def mixed_jobs(capi, W, H, dw, dh):
    """(rect, dst_rect) of one call: the whole frame letterboxed by the fit; 2.5 x down at an odd x, y with odd w, h and an odd ix; 6.3 x down; down
    in x and up in y; a 1 x 1 picture of the whole frame (every pixel of the rectangle is a tap); a 1 x 1 rectangle — the frame's last pixel, under
    the odd chroma edge — blown up to 5 x 5; a picture that covers the whole plane; a picture of one column at the plane's last column"""
    return [((0, 0, W, H), capi.letterbox_fit(W, H, dw, dh)),
            ((7, 5, 75, 45), (3, 2, 30, 18)),
            ((1, 2, 189, 126), (5, 4, 30, 20)),
            ((10, 11, 120, 10), (0, 0, 40, 25)),
            ((0, 0, W, H), (dw - 2, 1, 1, 1)),
            ((W - 1, H - 1, 1, 1), (2, 3, 5, 5)),
            ((3, 1, 150, 100), (0, 0, dw, dh)),
            ((20, 0, 9, H), (dw - 1, 0, 1, dh))]


_SRC, _REF, _RUN = {}, {}, {}


def source(orc, sf, cs, cr, W, H, seed=0):
    """(host planes, LaidOutPlanes on the device at odd pitches and offsets, the oracle's RGB_PLANAR planes), once per key"""
    key = (sf, cs, cr, W, H, seed)
    if key not in _SRC:
        if sf == "P10":
            host, rgb = p16.p16_frame(orc, "P10", W, H, seed), p16.rgb_of(orc, "P10", cs, cr, W, H, seed)
            lay = (64, 2, 2)   # 16-bit samples: rows 2-B aligned and no more
        else:
            host = orc.synth(getattr(orc, sf), W, H, 9100 + 13 * seed + W)
            st, rgb = orc.convert(getattr(orc, sf), orc.RGB_PLANAR, cs, cr, W, H, host, orc.FP32)
            assert st == 0
            lay = (64, 3, 1)
        _SRC[key] = (host, LaidOutPlanes(host, [lay] * len(host)), rgb)
    return _SRC[key]


def ref_u8(aa, orc, sf, cs, cr, W, H, rect, drect, dw, dh, bgr=False, seed=0, pad=PAD):
    """[3, dh, dw] reference bytes of one job (kernel channel order R G B, the pad of its output channel), computed once and never modified"""
    key = (sf, cs, cr, W, H, rect, drect, dw, dh, bgr, seed, pad)
    if key not in _REF:
        inner = aa_ref(aa, source(orc, sf, cs, cr, W, H, seed)[2], rect, drect[2], drect[3])
        _REF[key] = place(inner, drect, dw, dh, pad, bgr)
        _REF[key].setflags(write=False)
    return _REF[key]


class Dst:
    """n jobs' destination planes in ONE canary-filled allocation (LaidOutPlanes, stacked): three planes of dw elements per row, or one of 3 dw"""

    def __init__(self, n, dw, dh, dtype, nhwc, layout):
        self.n, self.nhwc = n, nhwc
        shape = (dh, 3 * dw) if nhwc else (dh, dw)
        self.per = 1 if nhwc else 3
        self.lay = LaidOutPlanes([np.full(shape, 0xCDCDCDCD if dtype == 0 else 0xCDCD, NPDT[dtype]) for _ in range(n * self.per)], layout, stacked=True)
        self.dw, self.dh = dw, dh

    def planes(self, i):
        d = self.lay.desc()[i * self.per:(i + 1) * self.per]
        return d + [(0, 0)] * (3 - len(d))

    def frames(self):
        """-> (bit patterns [n, 3, dh, dw] or [n, dh, dw, 3], canaries intact)"""
        planes, intact = self.lay.download()
        if self.nhwc:
            return np.stack([p.reshape(self.dh, self.dw, 3) for p in planes]), intact
        return np.stack(planes).reshape(self.n, 3, self.dh, self.dw), intact


def call_aa(capi, sf, cs, cr, W, H, dw, dh, jobs, dtype, bgr, nhwc, dst, variant=None, pad=PAD, first=0):
    """jobs: [(LaidOutPlanes of the frame, rect, dst_rect)]; job i writes dst.planes(first + i)"""
    norm = capi.make_tensor_norm(*PARAMS["imagenet"], dtype=dtype, bgr=bgr, nhwc=nhwc)
    arr = capi.make_letterbox_jobs([(dev.desc(), dst.planes(first + i), rect, drect) for i, (dev, rect, drect) in enumerate(jobs)])
    prev = capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, variant) if variant is not None else None
    try:
        capi.convert_letterbox_tensor_aa(capi.make_exec(stream_handle()), getattr(capi, sf), cs, cr, W, H, dw, dh, arr, norm, capi.make_letterbox_opts(pad))
        torch.cuda.synchronize()
    finally:
        if variant is not None:
            capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, prev)


def run_case(capi, orc, name, variant, jobs=None):
    """the bits one call of the case's mixed jobs writes, once per (case, knob); the sources' and the destination's canaries are checked here"""
    key = (name, variant, None if jobs is None else tuple(jobs))
    if key not in _RUN:
        _, sf, cs, cr, (W, H), (dw, dh), dtype, bgr, nhwc, layout = CASE[name]
        dev = source(orc, sf, cs, cr, W, H)[1]
        jobs = mixed_jobs(capi, W, H, dw, dh) if jobs is None else jobs
        dst = Dst(len(jobs), dw, dh, dtype, nhwc, layout)
        call_aa(capi, sf, cs, cr, W, H, dw, dh, [(dev, r, d) for r, d in jobs], dtype, bgr, nhwc, dst, variant=variant)
        got, intact = dst.frames()
        assert intact, (name, variant, "a byte outside the destinations changed")
        assert dev.download()[1], (name, variant, "a byte around the source changed")
        got.setflags(write=False)
        _RUN[key] = got
    return _RUN[key]


def check_case(capi, orc, aa, name, got, jobs=None):
    _, sf, cs, cr, (W, H), (dw, dh), dtype, bgr, nhwc, _ = CASE[name]
    jobs = mixed_jobs(capi, W, H, dw, dh) if jobs is None else jobs
    for i, (rect, drect) in enumerate(jobs):
        want = reference_bits(ref_u8(aa, orc, sf, cs, cr, W, H, rect, drect, dw, dh, bgr), *PARAMS["imagenet"], dtype, bgr)
        assert_bits(got[i], hwc(want) if nhwc else want, f"{name} job {i} rect {rect} -> dst_rect {drect}")


def job_geoms(jobs):
    return [(r[2], r[3], d[2], d[3]) for r, d in jobs]


# ------------------------------------------------------------------------------------------------ 1. one call of mixed jobs
@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_one_call_of_mixed_jobs(capi, orc, aa, name):
    """eight jobs of every kind in one call, per source class and layout: the plan stages seven of them under the 32 x 8 tile (the 6.3 x job does not
    fit the 64 x 16 one) and sends the 1 x 1 picture of the whole frame per tap"""
    _, sf, cs, cr, (W, H), (dw, dh), dtype, bgr, nhwc, _ = CASE[name]
    jobs = mixed_jobs(capi, W, H, dw, dh)
    ok, _, ds, which = plan(aa, job_geoms(jobs), dw, dh, nhwc=int(nhwc), dtype=dtype)
    assert ok and [d["form"] for d in ds] == [AA_STRIP, AA_GATHER] and ds[0]["tile"] == 1 and list(which) == [0, 0, 0, 0, 1, 0, 0, 0]
    check_case(capi, orc, aa, name, run_case(capi, orc, name, None))


@pytest.mark.parametrize("name", ["nv12", "yuv420_nhwc", "p10", "nv12_f16"])
def test_the_large_tile(capi, orc, aa, name):
    """the same call without the 6.3 x job and the 1 x 1 picture: one staged dispatch under the 64 x 16 tile, four pixels per lane (the 16-B / 8-B
    stores of an aligned tensor, element stores of the others)"""
    _, sf, cs, cr, (W, H), (dw, dh), dtype, bgr, nhwc, _ = CASE[name]
    jobs = [j for k, j in enumerate(mixed_jobs(capi, W, H, dw, dh)) if k not in (2, 4)]
    ok, _, ds, which = plan(aa, job_geoms(jobs), dw, dh, nhwc=int(nhwc), dtype=dtype)
    assert ok and len(ds) == 1 and ds[0]["form"] == AA_STRIP and ds[0]["tile"] == 0
    check_case(capi, orc, aa, name, run_case(capi, orc, name, None, jobs), jobs)


# ------------------------------------------------------------------------------------------------ 2. staged = per tap
@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_staged_equals_per_tap(capi, orc, aa, name):
    """the same calls under VPF_TUNE_NV12_RGB_VARIANT = 9 (every job per tap; the knob is reset in call_aa's finally): identical bits"""
    per_tap = run_case(capi, orc, name, 9)
    check_case(capi, orc, aa, name, per_tap)
    assert np.array_equal(per_tap, run_case(capi, orc, name, None))


# ------------------------------------------------------------------------------------------------ 3. the table cut
def test_jobs_over_the_table_cap(capi, orc, aa):
    """cap + 1 jobs into 8 x 8 f32 destinations, rectangles and pictures of their own: the second job table holds one job.  The first, a middle and
    the last job against single-job calls and against the reference"""
    W, H, dw, dh, sf = 194, 130, 8, 8, "NV12"
    cap = aa.aa_c_cap()
    assert cap == 82
    dev = source(orc, sf, 1, 0, W, H)[1]
    jobs = []
    for i in range(cap + 1):
        iw, ih = 1 + i % 8, 1 + (3 * i) % 8
        jobs.append(((i, i % 50, 20 + i, 17 + (5 * i) % 60), ((7 * i) % (dw - iw + 1), (5 * i) % (dh - ih + 1), iw, ih)))
    dst = Dst(len(jobs), dw, dh, 0, False, (64, 0, 0))
    call_aa(capi, sf, 1, 0, W, H, dw, dh, [(dev, r, d) for r, d in jobs], 0, False, False, dst)
    got, intact = dst.frames()
    assert intact
    single = Dst(3, dw, dh, 0, False, (64, 0, 0))
    picks = [0, cap // 2, cap]
    for k, i in enumerate(picks):
        call_aa(capi, sf, 1, 0, W, H, dw, dh, [(dev, *jobs[i])], 0, False, False, single, first=k)
    one, intact = single.frames()
    assert intact
    for k, i in enumerate(picks):
        assert np.array_equal(got[i], one[k]), i
        want = reference_bits(ref_u8(aa, orc, sf, 1, 0, W, H, jobs[i][0], jobs[i][1], dw, dh), *PARAMS["imagenet"], 0, False)
        assert_bits(got[i], want, f"job {i}")


# ------------------------------------------------------------------------------------------------ 4. reach
def _reach_child():
    """runs in a child process under VPF_HIP_LOG=2: the mixed call of case nv12 with the default policy and under knob 9"""
    import oracle as orc
    from videoprocessingframework_amd import capi

    capi.lib()
    for label, variant in (("default", None), ("knob9", 9)):
        print("CASE", label, file=sys.stderr, flush=True)
        run_case(capi, orc, "nv12", variant)
    print("done")


def test_reach_of_both_forms():
    """a child process with VPF_HIP_LOG=2: the mixed call launches k_lbaa_strip and then k_lbaa_gather, under knob 9 only k_lbaa_gather"""
    code = f"import sys; sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, 'tests')!r}]; import test_gpu_letterbox_aa as t; t._reach_child()"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, VPF_HIP_LOG="2"), timeout=300)
    assert r.returncode == 0 and "done" in r.stdout, r.stdout + r.stderr
    logs = {}
    for chunk in r.stderr.split("CASE ")[1:]:
        label, rest = chunk.split("\n", 1)
        logs[label.strip()] = [l for l in rest.split("\n") if "libvpfhip: launch" in l]
    print(logs)
    assert len(logs["default"]) == 2 and "k_lbaa_strip<0, 6>" in logs["default"][0] and "k_lbaa_gather<0, 6>" in logs["default"][1]
    assert len(logs["knob9"]) == 1 and "k_lbaa_gather<0, 6>" in logs["knob9"][0]


# ------------------------------------------------------------------------------------------------ 5. Python
def _nvc():
    sys.path.insert(0, os.path.join(ROOT, "videoprocessingframework_amd"))
    import PyNvCodec as nvc
    from videoprocessingframework_amd import PytorchNvCodec as pnc

    return nvc, pnc


def test_python_layers(capi, orc, aa):
    """ExecuteLetterboxAAToTensor and letterbox_to_normalized_tensor(antialias=True) give the bits of the C call (and of the reference), rois=None with
    the fit and explicit rois / dst_rects; antialias=False gives the bits of vpf_convert_letterbox_tensor; `out` reused gives the same bits again"""
    nvc, pnc = _nvc()
    PF = nvc.PixelFormat
    W, H, dw, dh = 194, 130, 64, 48
    mean, std = PARAMS["imagenet"]
    cc = nvc.ColorspaceConversionContext(nvc.ColorSpace.BT_709, nvc.ColorRange.JPEG)
    hosts = [source(orc, "NV12", 1, 1, W, H, seed) for seed in range(2)]
    up = nvc.PyFrameUploader(W, H, PF.NV12, 0)
    surfs = [up.UploadSingleFrame(np.concatenate([p.reshape(-1) for p in h[0]])).Clone(0) for h in hosts]
    torch.cuda.synchronize()
    rs = nvc.PySurfaceConvertResizer(W, H, PF.NV12, dw, dh, PF.RGB_PLANAR, 0)
    rois = [(1, 7, 5, 75, 45), (0, 0, 0, W, H), (0, 1, 2, 189, 126)]
    drects = [(3, 2, 30, 18), (0, 0, dw, dh), (5, 4, 30, 20)]

    def c_call(entry, jobs, dtype=0, bgr=False, pad=PAD):
        out = torch.zeros((len(jobs), 3, dh, dw), dtype={0: torch.float32, 1: torch.float16}[dtype], device="cuda")
        e = ELEM[dtype]
        arr = capi.make_letterbox_jobs([(hosts[k][1].desc(), [(out[i, c].data_ptr(), dw * e) for c in range(3)], r, d) for i, (k, r, d) in enumerate(jobs)])
        entry(capi.make_exec(stream_handle()), capi.NV12, 1, 1, W, H, dw, dh, arr, capi.make_tensor_norm(mean, std, dtype=dtype, bgr=bgr), capi.make_letterbox_opts(pad))
        torch.cuda.synchronize()
        return out

    # rois=None: the fit of the whole frame
    fit = capi.letterbox_fit(W, H, dw, dh)
    out, placement = pnc.letterbox_to_normalized_tensor(rs, surfs, mean, std, cc_ctx=cc, antialias=True)
    torch.cuda.synchronize()
    assert placement.tolist() == [list(fit)] * 2
    want = c_call(capi.convert_letterbox_tensor_aa, [(k, (0, 0, W, H), fit) for k in range(2)], pad=(114, 114, 114))
    assert torch.equal(out.view(torch.int32), want.view(torch.int32))
    got = out.cpu().numpy().view(np.uint32)
    for k in range(2):
        assert_bits(got[k], reference_bits(ref_u8(aa, orc, "NV12", 1, 1, W, H, (0, 0, W, H), fit, dw, dh, seed=k, pad=(114, 114, 114)), mean, std, 0, False), f"fit {k}")
    # explicit rois and dst_rects, f16, B G R, `out` reused twice
    jobs = [(r[0], tuple(r[1:]), d) for r, d in zip(rois, drects)]
    want = c_call(capi.convert_letterbox_tensor_aa, jobs, dtype=1, bgr=True)
    view = torch.zeros((len(rois), 3, dh, dw), dtype=torch.float16, device="cuda")
    for _ in range(2):
        res, placement = pnc.letterbox_to_normalized_tensor(rs, surfs, mean, std, rois=rois, dst_rects=drects, pad=PAD, dtype=torch.float16, bgr=True, out=view,
                                                            cc_ctx=cc, antialias=True)
        torch.cuda.synchronize()
        assert res.data_ptr() == view.data_ptr() and placement.tolist() == [list(d) for d in drects]
        assert torch.equal(view.view(torch.int16), want.view(torch.int16))
    h = view.cpu().numpy().view(np.uint16)
    for i, (k, r, d) in enumerate(jobs):
        assert_bits(h[i], reference_bits(ref_u8(aa, orc, "NV12", 1, 1, W, H, r, d, dw, dh, True, seed=k), mean, std, 1, True), f"python job {i}")
    # the binding itself
    raw = torch.zeros((len(rois), 3, dh, dw), dtype=torch.float16, device="cuda")
    with pnc._on_task_stream(rs, raw.device):
        assert rs.ExecuteLetterboxAAToTensor(surfs, rois, drects, raw.data_ptr(), 1, list(mean), list(std), cc, True, list(PAD))
    torch.cuda.synchronize()
    assert torch.equal(raw.view(torch.int16), want.view(torch.int16))
    # antialias=False: the function as it was
    plain, _ = pnc.letterbox_to_normalized_tensor(rs, surfs, mean, std, rois=rois, dst_rects=drects, pad=PAD, cc_ctx=cc)
    dflt, _ = pnc.letterbox_to_normalized_tensor(rs, surfs, mean, std, rois=rois, dst_rects=drects, pad=PAD, cc_ctx=cc, antialias=False)
    torch.cuda.synchronize()
    want = c_call(capi.convert_letterbox_tensor, jobs)
    assert torch.equal(plain.view(torch.int32), want.view(torch.int32)) and torch.equal(dflt.view(torch.int32), want.view(torch.int32))
    aa_out, _ = pnc.letterbox_to_normalized_tensor(rs, surfs, mean, std, rois=rois, dst_rects=drects, pad=PAD, cc_ctx=cc, antialias=True)
    torch.cuda.synchronize()
    assert not torch.equal(aa_out.view(torch.int32), want.view(torch.int32))   # 6.3 x down: another filter, other bytes
