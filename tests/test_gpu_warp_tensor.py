"""The fused multi-ROI affine warp into a normalised tensor on the MI355X: vpf_convert_warp_tensor.

Ground truth is the CPU oracle, composed as the definition says (tests/test_warp_tensor_cpu.py::warp_reference_u8, whose premise is checked there):
oracle.convert(frame -> RGB_PLANAR, FP32) of the WHOLE frame once per (frame, matrix), float32 maps written as the definition, oracle.remap(RGB,
FP32) into a destination pre-filled with the border, then reference_bits of tests/test_gpu_tensor_out.py.  Every element of every output must be
bit-identical; there is no tolerance.  Destinations hold canaries around every plane, which must survive."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from gpu_util import DevPlanes, stream_handle
from test_gpu_tensor_out import ELEM, MATRICES, PARAMS, TensorBuf, assert_bits, reference_bits
from test_warp_tensor_cpu import warp_reference_u8

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAME_SIZES = [(131, 79), (130, 78)]
WARP_CAP = 96  # jobs per job table (kWarpBatch, vpf_internal.h)
BORDER = (7, 114, 250)
_C30, _S30 = 1.3 * math.cos(math.radians(30)), 1.3 * math.sin(math.radians(30))


def geometry_jobs(W, H, dw, dh):
    """the matrices of the geometry test on a W x H frame for a dw x dh destination"""
    return [
        (1, 0, 33, 0, 1, 5),                        # identity at (33, 5)
        (1, 0, W - dw, 0, 1, H - dh),               # touching the right and bottom edges: sx hits W - 1 exactly
        (1, 0, W - dw + 0.5, 0, 1, H - dh + 0.5),   # half a pixel further: the last column and row are just outside
        (_C30, -_S30, 40, _S30, _C30, -10),         # rotation 30 degrees x 1.3
        (0, -1, 70, 1, 0, 3),                       # 90 degrees
        (-1, 0, 100, 0, 1, 2),                      # horizontal flip
        (1, 0.35, 10, 0.2, 1, 4),                   # shear
        (2.9, 0, -20, 0, 2.9, -10),                 # down-scale 2.9
        (0.37, 0, 20.25, 0, 0.37, 11.5),            # up-scale
        (0, 0, 5.5, 0, 0, 7.25),                    # the all-zero linear part: every pixel samples (5.5, 7.25)
        (1, 0, 500, 0, 1, 0),                       # wholly outside
    ]


@pytest.fixture(scope="module")
def orc(oracle):
    oracle.set_threads(16)
    return oracle


_FRAMES, _RGB, _REFS = {}, {}, {}


def frame(orc, sf, W, H, seed=0):
    """(host planes, device planes) of one synthetic frame, once per (format, size, seed)"""
    key = (sf, W, H, seed)
    if key not in _FRAMES:
        src = orc.synth(getattr(orc, sf), W, H, 8800 + 13 * seed + W)
        _FRAMES[key] = (src, DevPlanes(src, align=64, extra=3))  # odd pitches: rows start at every alignment
    return _FRAMES[key]


def rgb_of(orc, sf, cs, cr, W, H, seed=0):
    fk = (sf, cs, cr, W, H, seed)
    if fk not in _RGB:
        st, rgb = orc.convert(getattr(orc, sf), orc.RGB_PLANAR, cs, cr, W, H, frame(orc, sf, W, H, seed)[0], orc.FP32)
        assert st == 0
        _RGB[fk] = rgb
    return _RGB[fk]


def ref_u8(orc, sf, cs, cr, W, H, m, dw, dh, border, mode, seed=0):
    """[3, dh, dw] reference bytes (R G B) of one job, computed once and shared (never modified)"""
    key = (sf, cs, cr, W, H, seed, tuple(float(np.float32(v)) for v in m), dw, dh, tuple(border), mode)
    if key not in _REFS:
        _REFS[key] = warp_reference_u8(orc, sf, cs, cr, W, H, m, dw, dh, border, mode, rgb=rgb_of(orc, sf, cs, cr, W, H, seed))
        _REFS[key].setflags(write=False)
    return _REFS[key]


def run_warps(capi, sf, cs, cr, W, H, dw, dh, jobs, dtype, bgr, params, buf, border=BORDER, mode=0):
    """jobs: [(DevPlanes of the frame, matrix)]; job i writes buf.planes(i); `border` is per OUTPUT channel"""
    mean, std = PARAMS[params]
    norm = capi.make_tensor_norm(mean, std, dtype=dtype, bgr=bgr)
    warps = capi.make_warps([(dev.desc(), buf.planes(i), m) for i, (dev, m) in enumerate(jobs)])
    capi.convert_warp_tensor(capi.make_exec(stream_handle()), getattr(capi, sf), cs, cr, W, H, dw, dh, warps, norm, capi.make_warp_opts(mode, border))
    torch.cuda.synchronize()


def want_bits(orc, sf, cs, cr, W, H, m, dw, dh, border, mode, params, dtype, bgr, seed=0):
    """border is per output channel: with B G R planes, output channel c is R G B channel 2 - c"""
    rgb_border = tuple(border[::-1]) if bgr else tuple(border)
    return reference_bits(ref_u8(orc, sf, cs, cr, W, H, m, dw, dh, rgb_border, mode, seed), *PARAMS[params], dtype, bgr)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("sf", ["NV12", "YUV420"])
@pytest.mark.parametrize("W,H", FRAME_SIZES)
def test_geometry(capi, orc, sf, W, H, mode):
    """one call to 61 x 35 f32 with every matrix of geometry_jobs, per border mode"""
    dw, dh, cs, cr = 61, 35, 1, 0
    dev = frame(orc, sf, W, H)[1]
    ms = geometry_jobs(W, H, dw, dh)
    buf = TensorBuf(len(ms), dw, dh, 4)
    run_warps(capi, sf, cs, cr, W, H, dw, dh, [(dev, m) for m in ms], 0, False, "imagenet", buf, mode=mode)
    got, intact = buf.frames()
    assert intact
    for i, m in enumerate(ms):
        assert_bits(got[i], want_bits(orc, sf, cs, cr, W, H, m, dw, dh, BORDER, mode, "imagenet", 0, False), f"{sf} {W}x{H} mode {mode} job {i} {m}")


@pytest.mark.parametrize("dw,dh", [(64, 48), (33, 33), (1, 1), (1, 40)])
def test_destination_sizes(capi, orc, dw, dh):
    """tile edges and scalar tails: whole tiles, one pixel past a tile, one pixel, width 1"""
    W, H = 131, 79
    for sf in ("NV12", "YUV420"):
        dev = frame(orc, sf, W, H)[1]
        ms = geometry_jobs(W, H, dw, dh)
        for mode in (0, 1):
            buf = TensorBuf(len(ms), dw, dh, 4)
            run_warps(capi, sf, 1, 0, W, H, dw, dh, [(dev, m) for m in ms], 0, False, "imagenet", buf, mode=mode)
            got, intact = buf.frames()
            assert intact
            for i, m in enumerate(ms):
                assert_bits(got[i], want_bits(orc, sf, 1, 0, W, H, m, dw, dh, BORDER, mode, "imagenet", 0, False), f"{sf} {dw}x{dh} mode {mode} job {i}")


@pytest.mark.parametrize("sf", ["NV12", "YUV420"])
@pytest.mark.parametrize("W,H", FRAME_SIZES)
def test_identity_translation_is_the_plain_conversion(capi, orc, sf, W, H):
    """identity + integer translation at odd offsets: the bytes of the plain conversion, compared directly"""
    dw, dh = 61, 35
    dev = frame(orc, sf, W, H)[1]
    offs = [(33, 5), (17, 9), (W - dw, H - dh), (1, 43)]
    buf = TensorBuf(len(offs), dw, dh, 4)
    run_warps(capi, sf, 1, 0, W, H, dw, dh, [(dev, (1, 0, x, 0, 1, y)) for x, y in offs], 0, False, "unit", buf)
    got, intact = buf.frames()
    assert intact
    rgb = rgb_of(orc, sf, 1, 0, W, H)
    for i, (x, y) in enumerate(offs):
        plain = np.stack([p[y:y + dh, x:x + dw] for p in rgb])
        assert_bits(got[i], reference_bits(plain, *PARAMS["unit"], 0, False), f"{sf} {W}x{H} identity at {(x, y)} == plain conversion")


@pytest.mark.parametrize("sf", ["NV12", "YUV420"])
def test_dtypes_and_channel_orders(capi, orc, sf):
    """three dtypes, R G B and B G R with a per-channel border (proves the border's channel order), both modes"""
    W, H, dw, dh = 131, 79, 61, 35
    dev = frame(orc, sf, W, H)[1]
    ms = geometry_jobs(W, H, dw, dh)[2:8]
    for dtype in (0, 1, 2):
        for bgr in (False, True):
            params = ("imagenet", "unit", "symmetric")[(dtype + bgr) % 3]
            mode = (dtype + bgr) % 2
            buf = TensorBuf(len(ms), dw, dh, ELEM[dtype])
            run_warps(capi, sf, 1, 1, W, H, dw, dh, [(dev, m) for m in ms], dtype, bgr, params, buf, mode=mode)
            got, intact = buf.frames()
            assert intact
            for i, m in enumerate(ms):
                assert_bits(got[i], want_bits(orc, sf, 1, 1, W, H, m, dw, dh, BORDER, mode, params, dtype, bgr), f"{sf} dtype{dtype} bgr{bgr} job {i}")


@pytest.mark.parametrize("cs,cr", MATRICES)
def test_matrices_f16(capi, orc, cs, cr):
    W, H, dw, dh = 130, 78, 61, 35
    for sf in ("NV12", "YUV420"):
        dev = frame(orc, sf, W, H)[1]
        ms = geometry_jobs(W, H, dw, dh)[2:8]
        buf = TensorBuf(len(ms), dw, dh, 2)
        run_warps(capi, sf, cs, cr, W, H, dw, dh, [(dev, m) for m in ms], 1, False, "imagenet", buf)
        got, intact = buf.frames()
        assert intact
        for i, m in enumerate(ms):
            assert_bits(got[i], want_bits(orc, sf, cs, cr, W, H, m, dw, dh, BORDER, 0, "imagenet", 1, False), f"{sf} cs{cs} cr{cr} job {i}")


@pytest.mark.parametrize("dw", [61, 64, 1])
@pytest.mark.parametrize("dtype", [0, 1])
def test_destination_layouts(capi, orc, dw, dtype):
    """the four destination layouts of the ROI test: contiguous, one element off the vector alignment, padded, padded to 64 bytes"""
    W, H, dh, sf = 131, 79, 37, "NV12"
    e = ELEM[dtype]
    dev = frame(orc, sf, W, H)[1]
    ms = geometry_jobs(W, H, dw, dh)[2:5]
    layouts = {"contiguous": dict(lead=256),
               "off_by_one_element": dict(lead=256 + e),
               "padded": dict(row=dw * e + 16 + e, plane=dh * (dw * e + 16 + e) + 40 * e, frame=3 * (dh * (dw * e + 16 + e) + 40 * e) + 8 * e, lead=24 * e),
               "padded64": dict(row=dw * e + 64, plane=dh * (dw * e + 64) + 64, frame=3 * (dh * (dw * e + 64) + 64) + 256, lead=512)}
    for lname, geo in layouts.items():
        buf = TensorBuf(len(ms), dw, dh, e, **geo)
        run_warps(capi, sf, 1, 0, W, H, dw, dh, [(dev, m) for m in ms], dtype, False, "imagenet", buf)
        got, intact = buf.frames()
        assert intact, (lname, dw, dtype)
        for i, m in enumerate(ms):
            assert_bits(got[i], want_bits(orc, sf, 1, 0, W, H, m, dw, dh, BORDER, 0, "imagenet", dtype, False), f"{lname} dw{dw} dtype{dtype} job {i}")


@pytest.mark.parametrize("sf", ["NV12", "YUV420"])
def test_both_forms_identical(capi, orc, sf):
    """one job set under the default policy and under tuning 9 (gather everywhere): equal GPU buffers, each equal to the oracle"""
    W, H, dw, dh = 131, 79, 64, 48
    dev = frame(orc, sf, W, H)[1]
    ms = geometry_jobs(W, H, dw, dh)
    bufs = []
    for variant in (0, 9):
        buf = TensorBuf(len(ms), dw, dh, 2)
        prev = capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, variant)
        try:
            run_warps(capi, sf, 0, 1, W, H, dw, dh, [(dev, m) for m in ms], 1, False, "symmetric", buf)
        finally:
            capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, prev)
        got, intact = buf.frames()
        assert intact
        for i, m in enumerate(ms):
            assert_bits(got[i], want_bits(orc, sf, 0, 1, W, H, m, dw, dh, BORDER, 0, "symmetric", 1, False), f"{sf} variant {variant} job {i}")
        bufs.append(buf)
    assert bool((bufs[0].buf == bufs[1].buf).all())


def test_kernel_selection_log():
    """a child process with VPF_HIP_LOG=2: an identity job takes the staged kernel; the policy sends a job to the gather kernel when a tile's strip
    outgrows the LDS limit (no break-even in converted pixels is recorded), so the gather job here is a 6 x down-scale, whose 32 x 32
    tile spans the frame's 128 rows x 189 columns (84 KiB against the 64 KiB limit); both in one call; under tuning 9 everything gathers"""
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
for name, ms, variant in (("ident", [(1, 0, 33, 0, 1, 5)], 0), ("down", [(6, 0, 3, 0, 6, 1)], 0), ("mixed", [(1, 0, 33, 0, 1, 5), (6, 0, 3, 0, 6, 1)], 0),
                          ("ident9", [(1, 0, 33, 0, 1, 5)], 9)):
    out = torch.zeros((len(ms), 3, dh, dw), dtype=torch.float32, device="cuda")
    prev = capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, variant)
    print("CASE", name, file=sys.stderr, flush=True)
    capi.convert_warp_tensor(ex, capi.NV12, 1, 0, W, H, dw, dh,
                             capi.make_warps([(src, [(out[i, c].data_ptr(), 4 * dw) for c in range(3)], m) for i, m in enumerate(ms)]), norm)
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
    assert len(logs["ident"]) == 1 and "k_warp_strip<" in logs["ident"][0]
    assert len(logs["down"]) == 1 and "k_warp_gather<" in logs["down"][0]
    assert len(logs["mixed"]) == 2 and "k_warp_strip<" in logs["mixed"][0] and "k_warp_gather<" in logs["mixed"][1]  # one call, both forms
    assert len(logs["ident9"]) == 1 and "k_warp_gather<" in logs["ident9"][0]


def test_job_tables(capi, orc):
    """97 jobs (two job tables) over two frames, staged and gather jobs mixed (400 x 300 frames: on the 131 x 79 ones every window fits the LDS, so
    nothing would gather; the 7 x down-scales here outgrow it), odd and even offsets: outputs land in job order"""
    W, H, dw, dh, sf = 401, 299, 33, 20, "NV12"
    devs = [frame(orc, sf, W, H, seed)[1] for seed in range(2)]
    rng = np.random.default_rng(11)
    ms = geometry_jobs(W, H, dw, dh)
    while len(ms) < WARP_CAP + 1:
        a, s = float(rng.uniform(0, 2 * math.pi)), float(rng.choice([0.5, 1.0, 1.4, 3.2, 7.0]))
        ms.append((s * math.cos(a), -s * math.sin(a), float(rng.integers(-10, W)), s * math.sin(a), s * math.cos(a), float(rng.integers(-10, H))))
    jobs = [(devs[i % 2], m) for i, m in enumerate(ms)]
    buf = TensorBuf(len(jobs), dw, dh, 4)
    run_warps(capi, sf, 1, 0, W, H, dw, dh, jobs, 0, False, "imagenet", buf, mode=1)
    got, intact = buf.frames()
    assert intact
    for i, m in enumerate(ms):
        assert_bits(got[i], want_bits(orc, sf, 1, 0, W, H, m, dw, dh, BORDER, 1, "imagenet", 0, False, seed=i % 2), f"job {i} {m}")


def _nvc():
    sys.path.insert(0, os.path.join(ROOT, "videoprocessingframework_amd"))
    import PyNvCodec as nvc
    from videoprocessingframework_amd import PytorchNvCodec as pnc

    return nvc, pnc


def _upload(nvc, planes, w, h):
    up = nvc.PyFrameUploader(w, h, nvc.PixelFormat.NV12, 0)
    return up.UploadSingleFrame(np.concatenate([p.reshape(-1) for p in planes])).Clone(0)


def test_python_path(capi, orc):
    """warps_to_normalized_tensor == the C-ABI result (through the oracle): a new tensor from a resizer on its own stream, consumed on torch's
    current stream without a host synchronisation; `out` as a slice of a larger batch; enqueued from a non-default torch stream; K = 0"""
    nvc, pnc = _nvc()
    PF = nvc.PixelFormat
    W, H, dw, dh = 130, 78, 61, 35
    mean, std = PARAMS["imagenet"]
    cc = nvc.ColorspaceConversionContext(nvc.ColorSpace.BT_709, nvc.ColorRange.JPEG)
    surfs = [_upload(nvc, frame(orc, "NV12", W, H, seed)[0], W, H) for seed in range(2)]
    torch.cuda.synchronize()
    ms = geometry_jobs(W, H, dw, dh)[1:8]
    index = [i % 2 for i in range(len(ms))]
    mats = np.array(ms, dtype=np.float64).reshape(-1, 2, 3)
    rs = nvc.PySurfaceConvertResizer(W, H, PF.NV12, dw, dh, PF.RGB_PLANAR, 0)  # its own non-blocking stream
    out = pnc.warps_to_normalized_tensor(rs, surfs, index, mats, mean, std, border=BORDER, cc_ctx=cc)
    consumed = out * 1.0  # on torch's current stream, no synchronize in between
    assert tuple(out.shape) == (len(ms), 3, dh, dw) and out.dtype == torch.float32
    got = consumed.cpu().numpy().view(np.uint32)
    for i, m in enumerate(ms):
        assert_bits(got[i], want_bits(orc, "NV12", 1, 1, W, H, m, dw, dh, BORDER, 0, "imagenet", 0, False, seed=index[i]), f"new tensor, job {i}")
    # the same jobs through the C ABI on the same frames: equal bits
    devs = [frame(orc, "NV12", W, H, seed)[1] for seed in range(2)]
    buf = TensorBuf(len(ms), dw, dh, 4)
    run_warps(capi, "NV12", 1, 1, W, H, dw, dh, [(devs[index[i]], m) for i, m in enumerate(ms)], 0, False, "imagenet", buf)
    assert np.array_equal(buf.frames()[0], got)
    # a float32 tensor [K, 2, 3], f16, B G R, replicate, into a slice of a larger batch whose other frames keep their canary bits, from a side stream
    big = torch.full((len(ms) + 3, 3, dh, dw), 0x3C3C, dtype=torch.int16, device="cuda")
    view = big.view(torch.float16)[2:2 + len(ms)]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        res = pnc.warps_to_normalized_tensor(rs, surfs, torch.tensor(index), torch.tensor(mats, dtype=torch.float32), mean, std, dtype=torch.float16, bgr=True,
                                             border=BORDER, border_mode="replicate", out=view, cc_ctx=cc)
        after = big.clone()  # ordered behind the call on the side stream
    side.synchronize()
    assert res.data_ptr() == view.data_ptr()
    h = after.cpu().numpy().view(np.uint16)
    assert (h[:2] == 0x3C3C).all() and (h[2 + len(ms):] == 0x3C3C).all()
    for i, m in enumerate(ms):
        assert_bits(h[2 + i], want_bits(orc, "NV12", 1, 1, W, H, m, dw, dh, BORDER, 1, "imagenet", 1, True, seed=index[i]), f"slice, job {i}")
    # K = 0: an empty tensor, nothing launched
    empty = pnc.warps_to_normalized_tensor(rs, surfs, [], [], mean, std, dtype=torch.bfloat16)
    assert tuple(empty.shape) == (0, 3, dh, dw) and empty.dtype == torch.bfloat16
    assert tuple(pnc.warps_to_normalized_tensor(rs, surfs, [], torch.empty((0, 2, 3)), mean, std).shape) == (0, 3, dh, dw)
    with pytest.raises(ValueError, match=r"\.cpu\(\)"):
        pnc.warps_to_normalized_tensor(rs, surfs, index, torch.tensor(mats, device="cuda"), mean, std)
    with pytest.raises(ValueError):
        pnc.warps_to_normalized_tensor(rs, surfs, index, mats, mean, std, out=torch.empty((len(ms), 3, dh, dw), dtype=torch.float16, device="cuda"))
