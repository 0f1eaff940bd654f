"""The fused multi-ROI perspective warp into a normalised tensor on the MI355X: vpf_convert_persp_tensor.

Ground truth is the CPU oracle, composed as the definition says (tests/test_persp_tensor_cpu.py::persp_reference_u8, whose premise is checked there):
oracle.convert(frame -> RGB_PLANAR, FP32) of the WHOLE frame, float32 maps written as the definition with numpy (rounded-affine nx, ny, w, IEEE
divisions; pixels with !(w > 0) out of range under CONSTANT, overwritten with the border under REPLICATE), oracle.remap(RGB, FP32) into a destination
pre-filled with the border, then reference_bits of tests/test_gpu_tensor_out.py.  Every element of every output must be bit-identical; there is no
tolerance.  Destinations hold canaries around every plane, which must survive.  Matrices with the last row (0, 0, 1) must also equal what
vpf_convert_warp_tensor itself writes, called in the same test."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import test_gpu_p16_tensor as p16
import test_gpu_warp_tensor as warp
from gpu_util import DevPlanes, stream_handle
from test_gpu_tensor_nhwc import NhwcBuf, hwc
from test_gpu_tensor_out import ELEM, PARAMS, TensorBuf, assert_bits, reference_bits
from test_persp_tensor_cpu import NAMED, persp_reference_u8

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAME_SIZES = [(131, 79), (130, 78)]
PERSP_CAP = 82  # jobs per job table (kPerspBatch, vpf_internal.h)
BORDER = warp.BORDER


@pytest.fixture(scope="module")
def orc(oracle):
    oracle.set_threads(16)
    return oracle


def lifted(W, H, dw, dh):
    """every matrix of the affine geometry test with the last row (0, 0, 1)"""
    return [tuple(m) + (0, 0, 1) for m in warp.geometry_jobs(W, H, dw, dh)]


def matrices(W, H, dw, dh):
    return [m for (m, _, _) in NAMED.values()] + lifted(W, H, dw, dh)


_REFS = {}


def ref_u8(orc, sf, cs, cr, W, H, m, dw, dh, border, mode, seed=0, rgb=None):
    """[3, dh, dw] reference bytes (R G B) of one job, computed once and shared (never modified)"""
    key = (sf, cs, cr, W, H, seed, tuple(float(np.float32(v)) for v in m), dw, dh, tuple(border), mode)
    if key not in _REFS:
        _REFS[key] = persp_reference_u8(orc, sf, cs, cr, W, H, m, dw, dh, border, mode, rgb=warp.rgb_of(orc, sf, cs, cr, W, H, seed) if rgb is None else rgb)
        _REFS[key].setflags(write=False)
    return _REFS[key]


def want_bits(orc, sf, cs, cr, W, H, m, dw, dh, border, mode, params, dtype, bgr, seed=0, rgb=None):
    """border is per output channel: with B G R planes, output channel c is R G B channel 2 - c"""
    rgb_border = tuple(border[::-1]) if bgr else tuple(border)
    return reference_bits(ref_u8(orc, sf, cs, cr, W, H, m, dw, dh, rgb_border, mode, seed, rgb), *PARAMS[params], dtype, bgr)


def run_persps(capi, sf, cs, cr, W, H, dw, dh, jobs, dtype, bgr, params, buf, border=BORDER, mode=0, nhwc=False):
    """jobs: [(DevPlanes of the frame, matrix)]; job i writes buf.planes(i); `border` is per OUTPUT channel"""
    norm = capi.make_tensor_norm(*PARAMS[params], dtype=dtype, bgr=bgr, nhwc=nhwc)
    table = capi.make_persps([(dev.desc(), buf.planes(i), m) for i, (dev, m) in enumerate(jobs)])
    capi.convert_persp_tensor(capi.make_exec(stream_handle()), getattr(capi, sf), cs, cr, W, H, dw, dh, table, norm, capi.make_warp_opts(mode, border))
    torch.cuda.synchronize()


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("sf", ["NV12", "YUV420"])
@pytest.mark.parametrize("W,H", FRAME_SIZES)
def test_geometry(capi, orc, sf, W, H, mode):
    """one call to 61 x 35 f32 with every named matrix (keystone, x 3.7, strong perspective, down-scale, the horizon inside the destination and on a
    pixel column, huge and infinite coordinates, w < 0 everywhere, cancellation) and every affine one with the last row (0, 0, 1), per border mode;
    the latter equal vpf_convert_warp_tensor's own output too"""
    dw, dh, cs, cr = 61, 35, 1, 0
    dev = warp.frame(orc, sf, W, H)[1]
    ms = matrices(W, H, dw, dh)
    buf = TensorBuf(len(ms), dw, dh, 4)
    run_persps(capi, sf, cs, cr, W, H, dw, dh, [(dev, m) for m in ms], 0, False, "imagenet", buf, mode=mode)
    got, intact = buf.frames()
    assert intact
    for i, m in enumerate(ms):
        assert_bits(got[i], want_bits(orc, sf, cs, cr, W, H, m, dw, dh, BORDER, mode, "imagenet", 0, False), f"{sf} {W}x{H} mode {mode} job {i} {m}")
    aff = warp.geometry_jobs(W, H, dw, dh)
    abuf = TensorBuf(len(aff), dw, dh, 4)
    warp.run_warps(capi, sf, cs, cr, W, H, dw, dh, [(dev, m) for m in aff], 0, False, "imagenet", abuf, mode=mode)
    agot, intact = abuf.frames()
    assert intact
    assert np.array_equal(agot, got[len(NAMED):]), "last row (0, 0, 1) != vpf_convert_warp_tensor"


@pytest.mark.parametrize("dw,dh", [(64, 48), (33, 33), (1, 1), (1, 40), (100, 70)])
def test_destination_sizes(capi, orc, dw, dh):
    """tile edges and scalar tails: whole tiles, one pixel past a tile (33 x 33: a tile row of ONE row, where the sawtooth matrix sends in-range pixels
    outside the window their tile staged — the per-pixel fallback runs), one pixel, width 1, 4 x 3 tiles; both modes, both 8-bit sources"""
    W, H = 131, 79
    for sf in ("NV12", "YUV420"):
        dev = warp.frame(orc, sf, W, H)[1]
        ms = matrices(W, H, dw, dh)
        for mode in (0, 1):
            buf = TensorBuf(len(ms), dw, dh, 4)
            run_persps(capi, sf, 1, 0, W, H, dw, dh, [(dev, m) for m in ms], 0, False, "imagenet", buf, mode=mode)
            got, intact = buf.frames()
            assert intact
            for i, m in enumerate(ms):
                assert_bits(got[i], want_bits(orc, sf, 1, 0, W, H, m, dw, dh, BORDER, mode, "imagenet", 0, False), f"{sf} {dw}x{dh} mode {mode} job {i} {m}")


# (source, dtype, B G R, channels-last, border mode, parameter set, colour space, range): each value of each parameter at least once
LAYOUT_CASES = [("NV12", 1, True, False, 1, "unit", 1, 1), ("YUV420", 2, False, False, 0, "symmetric", 0, 1), ("NV12", 0, True, True, 0, "imagenet", 1, 0),
                ("YUV420", 1, False, True, 1, "imagenet", 0, 0), ("NV12", 2, True, True, 1, "unit", 1, 1)]


@pytest.mark.parametrize("sf,dtype,bgr,nhwc,mode,params,cs,cr", LAYOUT_CASES)
def test_dtypes_channel_orders_and_layouts(capi, orc, sf, dtype, bgr, nhwc, mode, params, cs, cr):
    """f16 / bf16 / f32, R G B and B G R with a per-channel border (proves the border's channel order), planar and channels-last"""
    W, H, dw, dh = 131, 79, 61, 35
    dev = warp.frame(orc, sf, W, H)[1]
    ms = matrices(W, H, dw, dh)
    buf = (NhwcBuf if nhwc else TensorBuf)(len(ms), dw, dh, ELEM[dtype])
    run_persps(capi, sf, cs, cr, W, H, dw, dh, [(dev, m) for m in ms], dtype, bgr, params, buf, mode=mode, nhwc=nhwc)
    got, intact = buf.frames()
    assert intact
    for i, m in enumerate(ms):
        want = want_bits(orc, sf, cs, cr, W, H, m, dw, dh, BORDER, mode, params, dtype, bgr)
        assert_bits(got[i], hwc(want) if nhwc else want, f"{sf} dtype{dtype} bgr{bgr} nhwc{nhwc} mode{mode} job {i} {m}")


def test_p10(capi, orc):
    """P10 frames, narrowed at the load: the NV12 reference on the narrowed frame; the default policy under CONSTANT, the per-tap form under REPLICATE"""
    W, H, dw, dh, cs, cr = 131, 79, 61, 35, 1, 0
    dev = DevPlanes(p16.p16_frame(orc, "P10", W, H, 1), align=64, extra=2)
    rgb = p16.rgb_of(orc, "P10", cs, cr, W, H, 1)
    ms = matrices(W, H, dw, dh)
    for variant in (0, 9):
        buf = TensorBuf(len(ms), dw, dh, 4)
        prev = capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, variant)
        try:
            run_persps(capi, "P10", cs, cr, W, H, dw, dh, [(dev, m) for m in ms], 0, False, "imagenet", buf, mode=variant % 2)
        finally:
            capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, prev)
        got, intact = buf.frames()
        assert intact
        for i, m in enumerate(ms):
            want = reference_bits(persp_reference_u8(orc, "NV12", cs, cr, W, H, m, dw, dh, BORDER, variant % 2, rgb=rgb), *PARAMS["imagenet"], 0, False)
            assert_bits(got[i], want, f"P10 variant {variant} job {i} {m}")


@pytest.mark.parametrize("sf", ["NV12", "YUV420"])
def test_both_forms_identical(capi, orc, sf):
    """one job set under the default policy and under tuning 9 (per tap everywhere): equal GPU buffers, each equal to the oracle"""
    W, H, dw, dh = 131, 79, 64, 48
    dev = warp.frame(orc, sf, W, H)[1]
    ms = matrices(W, H, dw, dh) + [NAMED["sawtooth"][0]]
    bufs = []
    for variant in (0, 9):
        buf = TensorBuf(len(ms), dw, dh, 2)
        prev = capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, variant)
        try:
            run_persps(capi, sf, 0, 1, W, H, dw, dh, [(dev, m) for m in ms], 1, False, "symmetric", buf)
        finally:
            capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, prev)
        got, intact = buf.frames()
        assert intact
        for i, m in enumerate(ms):
            assert_bits(got[i], want_bits(orc, sf, 0, 1, W, H, m, dw, dh, BORDER, 0, "symmetric", 1, False), f"{sf} variant {variant} job {i}")
        bufs.append(buf)
    assert bool((bufs[0].buf == bufs[1].buf).all())


def test_kernel_selection_log(capi, orc):
    """a child process with VPF_HIP_LOG=2: a keystone job takes the staged kernel; a 6 x down-scale, whose bound (100 KiB on a 256 x 128 frame) exceeds
    the 64 KiB limit, the per-tap kernel; both in one call: two dispatches; a horizon job runs in the staged kernel, whose tiles decide for
    themselves; under tuning 9 everything samples per tap.  The horizon job on a real frame equals the oracle."""
    key, hor = NAMED["keystone"][0], NAMED["horizon"][0]
    down = (6, 0, 3, 0, 6, 1, 0.001, 0, 1)
    code = f"""
import sys
sys.path.insert(0, {ROOT!r})
import torch
from videoprocessingframework_amd import capi
W, H, dw, dh = 256, 128, 64, 48
y, uv = torch.zeros((H, W), dtype=torch.uint8, device="cuda"), torch.zeros((H // 2, W), dtype=torch.uint8, device="cuda")
src = [(y.data_ptr(), W), (uv.data_ptr(), W)]
ex = capi.make_exec(torch.cuda.current_stream().cuda_stream)
norm = capi.make_tensor_norm({PARAMS["imagenet"][0]!r}, {PARAMS["imagenet"][1]!r})
key, down, hor = {key!r}, {down!r}, {hor!r}
for name, ms, variant in (("key", [key], 0), ("down", [down], 0), ("mixed", [key, down], 0), ("horizon", [hor], 0), ("key9", [key], 9)):
    out = torch.zeros((len(ms), 3, dh, dw), dtype=torch.float32, device="cuda")
    prev = capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, variant)
    print("CASE", name, file=sys.stderr, flush=True)
    capi.convert_persp_tensor(ex, capi.NV12, 1, 0, W, H, dw, dh,
                              capi.make_persps([(src, [(out[i, c].data_ptr(), 4 * dw) for c in range(3)], m) for i, m in enumerate(ms)]), norm)
    torch.cuda.synchronize()
    capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, prev)
print("done")
"""
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, VPF_HIP_LOG="2"), timeout=120)
    assert r.returncode == 0 and "done" in r.stdout, r.stdout + r.stderr
    logs = {}
    for chunk in r.stderr.split("CASE ")[1:]:
        name, rest = chunk.split("\n", 1)
        logs[name.strip()] = [l for l in rest.split("\n") if "libvpfhip: launch" in l]
    print(logs)
    assert len(logs["key"]) == 1 and "k_persp_strip<" in logs["key"][0]
    assert len(logs["down"]) == 1 and "k_persp_gather<" in logs["down"][0]
    assert len(logs["mixed"]) == 2 and "k_persp_strip<" in logs["mixed"][0] and "k_persp_gather<" in logs["mixed"][1]  # one call, both forms
    assert len(logs["horizon"]) == 1 and "k_persp_strip<" in logs["horizon"][0]
    assert len(logs["key9"]) == 1 and "k_persp_gather<" in logs["key9"][0]
    W, H, dw, dh = 131, 79, 100, 70  # the horizon at dx = 33.3 of 4 x 3 tiles: staged, per-tap and border tiles in one job
    dev = warp.frame(orc, "NV12", W, H)[1]
    buf = TensorBuf(1, dw, dh, 4)
    run_persps(capi, "NV12", 1, 0, W, H, dw, dh, [(dev, hor)], 0, False, "imagenet", buf)
    got, intact = buf.frames()
    assert intact
    assert_bits(got[0], want_bits(orc, "NV12", 1, 0, W, H, hor, dw, dh, BORDER, 0, "imagenet", 0, False), "horizon 100 x 70")


def test_job_tables(capi, orc):
    """83 jobs (two job tables) over two frames of 401 x 299, staged and per-tap jobs mixed (the 7 x down-scales outgrow the LDS bound), keystones of
    both signs, odd and even offsets: outputs land in job order"""
    W, H, dw, dh, sf = 401, 299, 33, 20, "NV12"
    devs = [warp.frame(orc, sf, W, H, seed)[1] for seed in range(2)]
    rng = np.random.default_rng(16)
    ms = [m for (m, _, _) in NAMED.values()]
    while len(ms) < PERSP_CAP + 1:
        a, s = float(rng.uniform(0, 2 * np.pi)), float(rng.choice([0.5, 1.0, 1.4, 3.2, 7.0]))
        g = float(rng.choice([0.5, 1.0, 2.5]))
        ms.append(tuple(g * v for v in (s * np.cos(a), -s * np.sin(a), float(rng.integers(-10, W)), s * np.sin(a), s * np.cos(a), float(rng.integers(-10, H)),
                                        float(rng.uniform(-0.012, 0.012)), float(rng.uniform(-0.02, 0.02)), 1.0)))
    assert len(ms) == PERSP_CAP + 1
    jobs = [(devs[i % 2], m) for i, m in enumerate(ms)]
    buf = TensorBuf(len(jobs), dw, dh, 4)
    run_persps(capi, sf, 1, 0, W, H, dw, dh, jobs, 0, False, "imagenet", buf, mode=1)
    got, intact = buf.frames()
    assert intact
    for i, m in enumerate(ms):
        assert_bits(got[i], want_bits(orc, sf, 1, 0, W, H, m, dw, dh, BORDER, 1, "imagenet", 0, False, seed=i % 2), f"job {i} {m}")


def test_python_path(capi, orc):
    """persps_to_normalized_tensor on quads_to_homographies == the C-ABI result on the same float32 matrices (and the oracle): a new tensor, `out` as
    a channels-last f16 B G R slice from a side stream, K = 0"""
    nvc, pnc = warp._nvc()
    PF = nvc.PixelFormat
    W, H, dw, dh = 130, 78, 61, 35
    mean, std = PARAMS["imagenet"]
    cc = nvc.ColorspaceConversionContext(nvc.ColorSpace.BT_709, nvc.ColorRange.JPEG)
    surfs = [warp._upload(nvc, warp.frame(orc, "NV12", W, H, seed)[0], W, H) for seed in range(2)]
    torch.cuda.synchronize()
    quads = np.array([[[10, 5], [100, 12], [110, 70], [4, 60]], [[30, 2], [90, 2], [90, 50], [30, 50]], [[120, 70], [20, 75], [5, 3], [125, 8]],
                      [[-20, 10], [60, -5], [150, 90], [10, 60]]], dtype=np.float64)
    hs = pnc.quads_to_homographies(quads, (dw, dh))
    ms = [tuple(float(v) for v in h.reshape(9)) for h in hs.numpy()]
    index = [i % 2 for i in range(len(ms))]
    rs = nvc.PySurfaceConvertResizer(W, H, PF.NV12, dw, dh, PF.RGB_PLANAR, 0)  # its own non-blocking stream
    out = pnc.persps_to_normalized_tensor(rs, surfs, index, hs, mean, std, border=BORDER, cc_ctx=cc)
    consumed = out * 1.0  # on torch's current stream, no synchronize in between
    assert tuple(out.shape) == (len(ms), 3, dh, dw) and out.dtype == torch.float32
    got = consumed.cpu().numpy().view(np.uint32)
    for i, m in enumerate(ms):
        assert_bits(got[i], want_bits(orc, "NV12", 1, 1, W, H, m, dw, dh, BORDER, 0, "imagenet", 0, False, seed=index[i]), f"new tensor, job {i}")
    devs = [warp.frame(orc, "NV12", W, H, seed)[1] for seed in range(2)]
    buf = TensorBuf(len(ms), dw, dh, 4)
    run_persps(capi, "NV12", 1, 1, W, H, dw, dh, [(devs[index[i]], m) for i, m in enumerate(ms)], 0, False, "imagenet", buf)
    assert np.array_equal(buf.frames()[0], got)
    # [K, 9] float64, f16, B G R, replicate, channels-last, into a slice of a larger batch whose other frames keep their canary bits, from a side stream
    big = torch.full((len(ms) + 3, 3, dh, dw), 0x3C3C, dtype=torch.int16, device="cuda").contiguous(memory_format=torch.channels_last)
    view = big.view(torch.float16)[2:2 + len(ms)]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        res = pnc.persps_to_normalized_tensor(rs, surfs, torch.tensor(index), hs.to(torch.float64).reshape(-1, 9), mean, std, dtype=torch.float16, bgr=True,
                                              border=BORDER, border_mode="replicate", out=view, cc_ctx=cc, channels_last=True)
        after = big.clone()  # ordered behind the call on the side stream
    side.synchronize()
    assert res.data_ptr() == view.data_ptr()
    h = after.cpu().numpy().view(np.uint16)
    assert (h[:2] == 0x3C3C).all() and (h[2 + len(ms):] == 0x3C3C).all()
    for i, m in enumerate(ms):
        assert_bits(h[2 + i], want_bits(orc, "NV12", 1, 1, W, H, m, dw, dh, BORDER, 1, "imagenet", 1, True, seed=index[i]), f"slice, job {i}")
    empty = pnc.persps_to_normalized_tensor(rs, surfs, [], [], mean, std, dtype=torch.bfloat16)
    assert tuple(empty.shape) == (0, 3, dh, dw) and empty.dtype == torch.bfloat16
    with pytest.raises(ValueError, match=r"\.cpu\(\)"):
        pnc.persps_to_normalized_tensor(rs, surfs, index, hs.cuda(), mean, std)
    # quads on the device: the same matrices within float32 rounding of a float64 solve
    dev_hs = pnc.quads_to_homographies(torch.tensor(quads, device="cuda"), (dw, dh))
    assert dev_hs.is_cuda and torch.allclose(dev_hs.cpu(), hs, rtol=1e-5, atol=1e-5)
