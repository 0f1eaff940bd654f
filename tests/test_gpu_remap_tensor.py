"""The fused per-pixel remap into a normalised tensor on the MI355X: vpf_convert_remap_tensor, PySurfaceConvertResizer.ExecuteRemapToTensor and
PytorchNvCodec.remap_to_normalized_tensor.

Ground truth is the CPU oracle, composed as the definition says (tests/test_remap_tensor_cpu.py::remap_reference_u8, whose premise is checked there):
oracle.convert(frame -> RGB_PLANAR, FP32) of the WHOLE frame, oracle.remap(RGB, FP32) on the maps under test (clamped first under REPLICATE, NaN
staying NaN) into a destination pre-filled with the border, then reference_bits of tests/test_gpu_tensor_out.py; P10 / P12 as
tests/test_gpu_p16_tensor.py composes them.  Every element of every output must be bit-identical; there is no tolerance.  Destinations hold
canaries around every plane, which must survive; the maps' padding holds NaN bit patterns."""
import math
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
from test_gpu_tensor_out import CANARY, ELEM, MATRICES, PARAMS, TensorBuf, assert_bits, reference_bits
from test_remap_tensor_cpu import remap_reference_u8, sprinkle
from test_warp_tensor_cpu import warp_maps

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
FRAME_SIZES = [(131, 79), (130, 78)]
REMAP_CAP = 96  # jobs per job table (kRemapBatch, vpf_classes.h)
BORDER = (7, 114, 250)
_FIRST = int(os.environ.get("VPF_FUZZ_FIRST", "0"))
_FUZZ_SEEDS = range(_FIRST, _FIRST + int(os.environ.get("VPF_FUZZ_SEEDS", "16")))


@pytest.fixture(scope="module")
def orc(oracle):
    oracle.set_threads(16)
    return oracle


class DevMaps:
    """a pair of float32 maps [dh, dw] in device memory, each in an allocation of its own: row y at lead + y * pitch (bytes); everything that is no
    coordinate holds 0xFF bytes — NaNs, which would show in the output if the kernel read them as coordinates"""

    def __init__(self, sx, sy, xpitch=0, ypitch=0, xlead=0, ylead=0):
        self.shape = sx.shape
        self.bufs, self.desc = [], []
        for m, pitch, lead in ((sx, xpitch, xlead), (sy, ypitch, ylead)):
            dh, dw = m.shape
            pitch = pitch or 4 * dw
            buf = torch.empty(lead + dh * pitch + 64, dtype=torch.uint8, device="cuda")
            self.bufs.append(buf)
            self.desc.append((buf.data_ptr() + lead, pitch, lead))
        self.upload(sx, sy)

    def upload(self, sx, sy):
        """new coordinates into the SAME device buffers (a captured graph keeps their addresses)"""
        for m, buf, (_, pitch, lead) in zip((sx, sy), self.bufs, self.desc):
            dh, dw = m.shape
            h = np.full(buf.numel(), 0xFF, np.uint8)
            np.lib.stride_tricks.as_strided(h[lead:], shape=(dh, 4 * dw), strides=(pitch, 1))[:] = np.ascontiguousarray(m, dtype=F32).view(np.uint8).reshape(dh, 4 * dw)
            buf.copy_(torch.from_numpy(h), non_blocking=False)

    def x(self):
        return self.desc[0][:2]

    def y(self):
        return self.desc[1][:2]


def barrel_maps(W, H, dw, dh, k1=-0.32, k2=0.09):
    """undistort_maps of a camera whose principal point is the frame's centre, onto a dw x dh view of the whole frame"""
    from videoprocessingframework_amd import PytorchNvCodec as pnc

    K = [[0.8 * W, 0, (W - 1) / 2], [0, 0.8 * W, (H - 1) / 2], [0, 0, 1]]
    Kn = [[0.8 * W * dw / W, 0, (dw - 1) / 2], [0, 0.8 * W * dh / H, (dh - 1) / 2], [0, 0, 1]]
    sx, sy = pnc.undistort_maps(K, (k1, k2, 0.002, -0.001, 0.01), (dw, dh), new_camera_matrix=Kn)
    return sx.numpy().copy(), sy.numpy().copy()


def random_maps(W, H, dw, dh, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-5, W + 5, (dh, dw)).astype(F32), rng.uniform(-5, H + 5, (dh, dw)).astype(F32)


def make_buf(n, dw, dh, dtype, nhwc, **geo):
    return NhwcBuf(n, dw, dh, ELEM[dtype], **geo) if nhwc else TensorBuf(n, dw, dh, ELEM[dtype], **geo)


def run_remap(capi, sf, cs, cr, W, H, dw, dh, jobs, dtype, bgr, params, buf, border=BORDER, mode=0, max_step=0.0, nhwc=False, stream=None):
    """jobs: [(DevPlanes of the frame, DevMaps)]; job i writes buf.planes(i); `border` is per OUTPUT channel"""
    norm = capi.make_tensor_norm(*PARAMS[params], dtype=dtype, bgr=bgr, nhwc=nhwc)
    table = capi.make_remap_jobs([(dev.desc(), buf.planes(i), maps.x(), maps.y()) for i, (dev, maps) in enumerate(jobs)])
    capi.convert_remap_tensor(capi.make_exec(stream if stream is not None else stream_handle()), getattr(capi, sf), cs, cr, W, H, dw, dh, table, norm,
                              capi.make_remap_opts(mode, border, max_step))
    if stream is None:
        torch.cuda.synchronize()


def want_bits(orc, sf, cs, cr, W, H, sx, sy, border, mode, params, dtype, bgr, seed=0, nhwc=False, rgb=None):
    """border is per output channel: with B G R order, output channel c is R G B channel 2 - c"""
    rgb_border = tuple(border[::-1]) if bgr else tuple(border)
    rgb = warp.rgb_of(orc, sf, cs, cr, W, H, seed) if rgb is None else rgb
    bits = reference_bits(remap_reference_u8(orc, sf, cs, cr, W, H, sx, sy, rgb_border, mode, rgb=rgb), *PARAMS[params], dtype, bgr)
    return hwc(bits) if nhwc else bits


def check_one(capi, orc, sf, W, H, sx, sy, what, cs=1, cr=0, dtype=0, bgr=False, params="imagenet", mode=0, border=BORDER, nhwc=False, max_step=0.0, maps=None):
    """one job through the entry, against the reference; -> the output bits"""
    dh, dw = sx.shape
    buf = make_buf(1, dw, dh, dtype, nhwc)
    run_remap(capi, sf, cs, cr, W, H, dw, dh, [(warp.frame(orc, sf, W, H)[1], maps or DevMaps(sx, sy))], dtype, bgr, params, buf, border, mode, max_step, nhwc)
    got, intact = buf.frames()
    assert intact, what
    assert_bits(got[0], want_bits(orc, sf, cs, cr, W, H, sx, sy, border, mode, params, dtype, bgr, nhwc=nhwc), what)
    return got[0]


# ------------------------------------------------------------------------------------------------ affine maps
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("sf", ["NV12", "YUV420"])
@pytest.mark.parametrize("W,H", FRAME_SIZES)
def test_affine_maps_equal_the_reference_and_the_warp_entry(capi, orc, sf, W, H, mode):
    """the matrices of the warp test's geometry_jobs written out as maps (unclamped: the kernel clamps under REPLICATE), one call to 61 x 35 f32: the
    reference's bits AND the bits vpf_convert_warp_tensor writes for the matrices"""
    dw, dh, cs, cr = 61, 35, 1, 0
    dev = warp.frame(orc, sf, W, H)[1]
    ms = warp.geometry_jobs(W, H, dw, dh)
    pairs = [warp_maps(m, dw, dh, W, H, 0) for m in ms]
    buf, wbuf = TensorBuf(len(ms), dw, dh, 4), TensorBuf(len(ms), dw, dh, 4)
    run_remap(capi, sf, cs, cr, W, H, dw, dh, [(dev, DevMaps(sx, sy)) for sx, sy in pairs], 0, False, "imagenet", buf, mode=mode)
    warp.run_warps(capi, sf, cs, cr, W, H, dw, dh, [(dev, m) for m in ms], 0, False, "imagenet", wbuf, mode=mode)
    got, intact = buf.frames()
    assert intact
    for i, (m, (sx, sy)) in enumerate(zip(ms, pairs)):
        assert_bits(got[i], want_bits(orc, sf, cs, cr, W, H, sx, sy, BORDER, mode, "imagenet", 0, False), f"{sf} {W}x{H} mode {mode} job {i} {m}")
    assert torch.equal(buf.buf, wbuf.buf)


# ------------------------------------------------------------------------------------------------ map kinds
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("sf", ["NV12", "YUV420"])
@pytest.mark.parametrize("W,H", FRAME_SIZES)
def test_barrel_and_random_maps(capi, orc, sf, W, H, mode):
    """a barrel map from undistort_maps (smooth, leaving the frame at the corners) and a seeded random map with every pixel anywhere in
    [-5, W + 5] x [-5, H + 5]: every tile's window is the whole frame, whose strip (79 rows x 560 B) still fits 64 KiB"""
    for name, (sx, sy) in (("barrel", barrel_maps(W, H, 61, 35)), ("random", random_maps(W, H, 64, 48, 31))):
        check_one(capi, orc, sf, W, H, sx, sy, f"{name} {sf} {W}x{H} mode {mode}", mode=mode)


@pytest.mark.parametrize("mode", [0, 1])
def test_random_map_on_a_frame_that_cannot_fit_goes_per_tap(capi, orc, mode):
    """the same random map on one 640 x 360 frame: the window is the whole frame, 360 rows x 2 576 B — no LDS holds it, the tile samples per tap"""
    W, H = 640, 360
    sx, sy = random_maps(W, H, 64, 48, 31)
    check_one(capi, orc, "NV12", W, H, sx, sy, f"random 640x360 mode {mode}", mode=mode)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("bgr", [False, True])
@pytest.mark.parametrize("sf", ["NV12", "YUV420"])
def test_special_values(capi, orc, sf, bgr, mode):
    """NaN in sx only, in sy only and in both, +-inf, -0.0, 0, W - 1, the next float above it, H - 1, +-1e30, denormals — sprinkled into a smooth map;
    a per-channel border and B G R prove the border's channel order"""
    for W, H in FRAME_SIZES:
        sx, sy = sprinkle(*warp_maps((0.9, -0.3, 30.0, 0.3, 0.9, 2.0), 61, 35, W, H, 0), W, H, 5)
        assert np.isnan(sx).sum() == 2 and np.isnan(sy).sum() == 2 and np.isinf(sx).sum() == 2 and (sx == F32(1e30)).sum() == 1
        check_one(capi, orc, sf, W, H, sx, sy, f"special {sf} {W}x{H} bgr{bgr} mode {mode}", bgr=bgr, mode=mode, params="symmetric")


@pytest.mark.parametrize("mode", [0, 1])
def test_tile_cases(capi, orc, mode):
    """a tile with exactly one in-range pixel (every other coordinate NaN or left of the frame), a map wholly out of range, a map of all NaN"""
    W, H, dw, dh, sf = 131, 79, 64, 48, "NV12"
    nan = np.full((dh, dw), np.nan, F32)
    one_x, one_y = np.full((dh, dw), -7.0, F32), nan.copy()
    one_x[40, 50], one_y[40, 50] = F32(W - 1), F32(33.5)
    one_x[:, :32] = np.nan
    got = check_one(capi, orc, sf, W, H, one_x, one_y, f"one pixel mode {mode}", mode=mode)
    border_bits = reference_bits(np.broadcast_to(np.array(BORDER, np.uint8)[:, None, None], (3, dh, dw)), *PARAMS["imagenet"], 0, False)
    assert all(tuple(p) == (40, 50) for p in np.argwhere((got != border_bits).any(axis=0)))
    out_x, out_y = np.full((dh, dw), W + 0.5, F32), np.full((dh, dw), -0.25, F32)
    got = check_one(capi, orc, sf, W, H, out_x, out_y, f"out of range mode {mode}", mode=mode)
    assert mode == 1 or np.array_equal(got, border_bits)
    got = check_one(capi, orc, sf, W, H, nan, nan, f"all NaN mode {mode}", mode=mode)
    assert np.array_equal(got, border_bits)  # both modes


@pytest.mark.parametrize("dw,dh", [(64, 48), (33, 33), (1, 1), (1, 40), (3, 2)])
def test_destination_sizes(capi, orc, dw, dh):
    """tile edges and scalar tails: whole tiles, one pixel past a tile, one pixel, width 1, three pixels"""
    W, H = 131, 79
    for sf in ("NV12", "YUV420"):
        for mode in (0, 1):
            for name, (sx, sy) in (("barrel", barrel_maps(W, H, dw, dh)), ("random", random_maps(W, H, dw, dh, 7))):
                check_one(capi, orc, sf, W, H, sx, sy, f"{name} {sf} {dw}x{dh} mode {mode}", mode=mode)


@pytest.mark.parametrize("dw", [61, 64, 3])
def test_map_layouts(capi, orc, dw):
    """padded pitches, xmap and ymap with different pitches, a map base at 4 mod 16 bytes (the dword-load path), dw that is no multiple of 4"""
    W, H, dh, sf = 131, 79, 37, "NV12"
    sx, sy = sprinkle(*barrel_maps(W, H, dw, dh), W, H, 9)
    layouts = {"tight": dict(), "padded16": dict(xpitch=4 * dw + 16 - (4 * dw) % 16 + 16, ypitch=4 * dw + 16 - (4 * dw) % 16 + 16), "padded4": dict(xpitch=4 * dw + 4, ypitch=4 * dw + 4),
               "different": dict(xpitch=4 * dw + 64, ypitch=4 * dw + 12), "base4": dict(xlead=4, ylead=4), "base4_x_only": dict(xlead=4, xpitch=4 * dw + 32),
               "base8_12": dict(xlead=8, ylead=12, ypitch=4 * dw + 20)}
    outs = []
    for lname, geo in layouts.items():
        maps = DevMaps(sx, sy, **geo)
        assert (maps.x()[0] % 16, maps.y()[0] % 16) == (geo.get("xlead", 0), geo.get("ylead", 0))
        outs.append(check_one(capi, orc, sf, W, H, sx, sy, f"{lname} dw{dw}", mode=1, maps=maps))
    assert all(np.array_equal(outs[0], o) for o in outs)


@pytest.mark.parametrize("sf", ["NV12", "YUV420"])
def test_every_form_gives_the_same_bits(capi, orc, sf):
    """the same calls with no hint, with max_step = 1e-3 (no window fits: per tap), with the maps_max_step hint, and under knob 9: four identical
    buffers, each equal to the reference"""
    from videoprocessingframework_amd import PytorchNvCodec as pnc

    W, H, dw, dh = 131, 79, 64, 48
    dev = warp.frame(orc, sf, W, H)[1]
    affine = warp_maps((1.3, 0.2, -4.0, -0.1, 1.2, 3.0), dw, dh, W, H, 0)
    pairs = [barrel_maps(W, H, dw, dh), random_maps(W, H, dw, dh, 3), sprinkle(*affine, W, H, 1)]
    maps = [DevMaps(sx, sy) for sx, sy in pairs]
    hint = max(pnc.maps_max_step(*pairs[0]), pnc.maps_max_step(*affine))  # (of the smooth maps: the random one has no useful bound, and needs none)
    assert 1.5 <= hint < 50.0
    bufs = []
    for name, step, variant in (("no hint", 0.0, 0), ("tiny hint", 1e-3, 0), ("true hint", hint, 0), ("knob 9", 0.0, 9)):
        buf = TensorBuf(len(maps), dw, dh, 2)
        prev = capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, variant)
        try:
            run_remap(capi, sf, 0, 1, W, H, dw, dh, [(dev, m) for m in maps], 1, False, "symmetric", buf, max_step=step)
        finally:
            capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, prev)
        got, intact = buf.frames()
        assert intact, name
        for i, (sx, sy) in enumerate(pairs):
            assert_bits(got[i], want_bits(orc, sf, 0, 1, W, H, sx, sy, BORDER, 0, "symmetric", 1, False), f"{sf} {name} job {i}")
        bufs.append(buf)
    assert all(bool((bufs[0].buf == b.buf).all()) for b in bufs[1:])


def test_kernel_selection_log():
    """a child process with VPF_HIP_LOG=2: one launch per job table names k_remap_tile with its source class and layout — 97 jobs take two"""
    code = f"""
import sys
sys.path.insert(0, {ROOT!r})
import torch
from videoprocessingframework_amd import capi
W, H, dw, dh = 256, 128, 64, 48
y, uv = torch.zeros((H, W), dtype=torch.uint8, device="cuda"), torch.zeros((H // 2, W), dtype=torch.uint8, device="cuda")
src = [(y.data_ptr(), W), (uv.data_ptr(), W)]
xm, ym = torch.zeros((dh, dw), device="cuda"), torch.zeros((dh, dw), device="cuda")
ex = capi.make_exec(torch.cuda.current_stream().cuda_stream)
for name, n, nhwc in (("one", 1, False), ("nhwc", 1, True), ("tables", 97, False)):
    norm = capi.make_tensor_norm({PARAMS["imagenet"][0]!r}, {PARAMS["imagenet"][1]!r}, nhwc=nhwc)
    out = torch.zeros((n, 3, dh, dw), dtype=torch.float32, device="cuda")
    dst = [[(out[i].data_ptr(), 12 * dw)] if nhwc else [(out[i, c].data_ptr(), 4 * dw) for c in range(3)] for i in range(n)]
    print("CASE", name, file=sys.stderr, flush=True)
    capi.convert_remap_tensor(ex, capi.NV12, 1, 0, W, H, dw, dh, capi.make_remap_jobs([(src, d, (xm.data_ptr(), 4 * dw), (ym.data_ptr(), 4 * dw)) for d in dst]), norm)
    torch.cuda.synchronize()
print("done")
"""
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, VPF_HIP_LOG="2"), timeout=120)
    assert r.returncode == 0 and "done" in r.stdout, r.stdout + r.stderr
    logs = {}
    for chunk in r.stderr.split("CASE ")[1:]:
        name, rest = chunk.split("\n", 1)
        logs[name.strip()] = [l for l in rest.split("\n") if "libvpfhip: launch" in l]
    print(logs)
    assert len(logs["one"]) == 1 and "(k_remap_tile<0, 6>)" in logs["one"][0]
    assert len(logs["nhwc"]) == 1 and "(k_remap_tile<0, 8>)" in logs["nhwc"][0]
    assert len(logs["tables"]) == 2 and all("(k_remap_tile<0, 6>)" in l for l in logs["tables"])


# ------------------------------------------------------------------------------------------------ tables and options
def test_job_tables(capi, orc):
    """97 jobs of 8 x 4 (two job tables) with two map pairs alternating over three frames: outputs land in job order"""
    W, H, dw, dh, sf = 131, 79, 8, 4, "NV12"
    devs = [warp.frame(orc, sf, W, H, seed)[1] for seed in range(3)]
    pairs = [sprinkle(*random_maps(W, H, dw, dh, 21), W, H, 2), warp_maps((9.0, 1.5, 3.0, -2.0, 11.0, 30.0), dw, dh, W, H, 0)]
    maps = [DevMaps(sx, sy) for sx, sy in pairs]
    n = REMAP_CAP + 1
    buf = TensorBuf(n, dw, dh, 4)
    run_remap(capi, sf, 1, 0, W, H, dw, dh, [(devs[i % 3], maps[i % 2]) for i in range(n)], 0, False, "imagenet", buf, mode=1)
    got, intact = buf.frames()
    assert intact
    want = {(f, k): want_bits(orc, sf, 1, 0, W, H, *pairs[k], BORDER, 1, "imagenet", 0, False, seed=f) for f in range(3) for k in range(2)}
    assert len({w.tobytes() for w in want.values()}) == 6
    for i in range(n):
        assert_bits(got[i], want[(i % 3, i % 2)], f"job {i}")


@pytest.mark.parametrize("sf", ["NV12", "YUV420"])
def test_dtypes_channel_orders_and_layouts(capi, orc, sf):
    """three dtypes, R G B and B G R with a per-channel border, planar and channels-last, both modes"""
    W, H, dw, dh = 131, 79, 61, 35
    dev = warp.frame(orc, sf, W, H)[1]
    pairs = [sprinkle(*barrel_maps(W, H, dw, dh), W, H, 4), random_maps(W, H, dw, dh, 12)]
    maps = [DevMaps(sx, sy) for sx, sy in pairs]
    for dtype in (0, 1, 2):
        for bgr in (False, True):
            for nhwc in (False, True):
                params = ("imagenet", "unit", "symmetric")[(dtype + bgr) % 3]
                mode = (dtype + bgr + nhwc) % 2
                buf = make_buf(len(maps), dw, dh, dtype, nhwc)
                run_remap(capi, sf, 1, 1, W, H, dw, dh, [(dev, m) for m in maps], dtype, bgr, params, buf, mode=mode, nhwc=nhwc)
                got, intact = buf.frames()
                assert intact
                for i, (sx, sy) in enumerate(pairs):
                    assert_bits(got[i], want_bits(orc, sf, 1, 1, W, H, sx, sy, BORDER, mode, params, dtype, bgr, nhwc=nhwc), f"{sf} dtype{dtype} bgr{bgr} nhwc{nhwc} job {i}")


@pytest.mark.parametrize("cs,cr", MATRICES)
def test_matrices_f16(capi, orc, cs, cr):
    W, H, dw, dh = 130, 78, 61, 35
    sx, sy = sprinkle(*barrel_maps(W, H, dw, dh), W, H, 6)
    for sf in ("NV12", "YUV420"):
        check_one(capi, orc, sf, W, H, sx, sy, f"{sf} cs{cs} cr{cr}", cs=cs, cr=cr, dtype=1)


@pytest.mark.parametrize("fmt,nhwc", [("P10", False), ("P12", True)])
def test_p10_p12(capi, orc, fmt, nhwc):
    """P10 / P12 frames: every sample narrowed to 8 bits at the load — the reference samples the conversion of the NV12 frame the narrowing gives
    (tests/test_gpu_p16_tensor.py); staged and per tap"""
    W, H, dw, dh, cs, cr = 131, 79, 61, 35, 1, 0
    dev = DevPlanes(p16.p16_frame(orc, fmt, W, H, 1), align=64, extra=2)
    rgb = p16.rgb_of(orc, fmt, cs, cr, W, H, 1)
    pairs = [sprinkle(*barrel_maps(W, H, dw, dh), W, H, 8), random_maps(W, H, dw, dh, 14)]
    maps = [DevMaps(sx, sy) for sx, sy in pairs]
    for variant in (0, 9):
        buf = make_buf(len(maps), dw, dh, 0, nhwc)
        prev = capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, variant)
        try:
            run_remap(capi, fmt, cs, cr, W, H, dw, dh, [(dev, m) for m in maps], 0, False, "imagenet", buf, mode=1, nhwc=nhwc)
        finally:
            capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, prev)
        got, intact = buf.frames()
        assert intact
        for i, (sx, sy) in enumerate(pairs):
            assert_bits(got[i], want_bits(orc, "NV12", cs, cr, W, H, sx, sy, BORDER, 1, "imagenet", 0, False, nhwc=nhwc, rgb=rgb), f"{fmt} variant {variant} job {i}")


# ------------------------------------------------------------------------------------------------ graph replay
def test_graph_replays_with_live_maps(capi, orc):
    """one call captured on a side stream (one stream, no parallel branches; called once eagerly first), replayed three times; the maps are overwritten
    in place on that stream between the replays: each replay is the reference of THAT replay's maps"""
    W, H, dw, dh, sf = 131, 79, 64, 48, "NV12"
    dev = warp.frame(orc, sf, W, H)[1]
    sets = [barrel_maps(W, H, dw, dh), sprinkle(*random_maps(W, H, dw, dh, 5), W, H, 3)]
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        live = DevMaps(*sets[0])
        staged = [[b.clone() for b in DevMaps(sx, sy).bufs] for sx, sy in sets]
        buf = TensorBuf(1, dw, dh, 4)
        run_remap(capi, sf, 1, 0, W, H, dw, dh, [(dev, live)], 0, False, "imagenet", buf, stream=st.cuda_stream)  # (eager once: the code object is loaded)
        st.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st):
            run_remap(capi, sf, 1, 0, W, H, dw, dh, [(dev, live)], 0, False, "imagenet", buf, stream=st.cuda_stream)
        for rep in (1, 0, 1):
            for b, s in zip(live.bufs, staged[rep]):
                b.copy_(s)
            buf.buf.fill_(CANARY)
            graph.replay()
            st.synchronize()
            got, intact = buf.frames()
            assert intact, rep
            assert_bits(got[0], want_bits(orc, sf, 1, 0, W, H, *sets[rep], BORDER, 0, "imagenet", 0, False), f"replay with maps {rep}")


# ------------------------------------------------------------------------------------------------ the Python path
def _nvc():
    sys.path.insert(0, os.path.join(ROOT, "videoprocessingframework_amd"))
    import PyNvCodec as nvc
    from videoprocessingframework_amd import PytorchNvCodec as pnc

    return nvc, pnc


def _upload(nvc, planes, w, h):
    up = nvc.PyFrameUploader(w, h, nvc.PixelFormat.NV12, 0)
    return up.UploadSingleFrame(np.concatenate([p.reshape(-1) for p in planes])).Clone(0)


def test_python_path(capi, orc):
    """remap_to_normalized_tensor: shared maps and a pair per frame (a slice of a wider tensor: padded rows), a new tensor consumed on torch's current
    stream without a host synchronisation, `out` as a slice of a larger batch from a side stream, channels-last, a hint; N = 0; ValueErrors"""
    nvc, pnc = _nvc()
    PF = nvc.PixelFormat
    W, H, dw, dh = 130, 78, 61, 35  # (even: a semi-planar Surface of the Task layer is one plane, chroma rows included)
    mean, std = PARAMS["imagenet"]
    cc = nvc.ColorspaceConversionContext(nvc.ColorSpace.BT_709, nvc.ColorRange.JPEG)
    surfs = [_upload(nvc, warp.frame(orc, "NV12", W, H, seed)[0], W, H) for seed in range(3)]
    torch.cuda.synchronize()
    pairs = [sprinkle(*barrel_maps(W, H, dw, dh), W, H, 2), random_maps(W, H, dw, dh, 8), warp_maps((1.1, 0.3, 2.0, -0.2, 0.9, 9.0), dw, dh, W, H, 0)]
    rs = nvc.PySurfaceConvertResizer(W, H, PF.NV12, dw, dh, PF.RGB_PLANAR, 0)  # its own non-blocking stream
    # one pair shared by three frames
    sx, sy = pairs[0]
    out = pnc.remap_to_normalized_tensor(rs, surfs, torch.from_numpy(sx).cuda(), torch.from_numpy(sy).cuda(), mean, std, border=BORDER, cc_ctx=cc)
    consumed = out * 1.0  # on torch's current stream, no synchronize in between
    assert tuple(out.shape) == (3, 3, dh, dw) and out.dtype == torch.float32
    got = consumed.cpu().numpy().view(np.uint32)
    for i in range(3):
        assert_bits(got[i], want_bits(orc, "NV12", 1, 1, W, H, sx, sy, BORDER, 0, "imagenet", 0, False, seed=i), f"shared maps, frame {i}")
    # a pair per frame, rows padded (a slice of a wider tensor), f16, B G R, replicate, a hint, into a slice of a larger batch, from a side stream
    wide_x, wide_y = torch.full((3, dh, dw + 7), float("nan"), device="cuda"), torch.full((3, dh, dw + 7), float("nan"), device="cuda")
    for i, (px, py) in enumerate(pairs):
        wide_x[i, :, 3:3 + dw], wide_y[i, :, 3:3 + dw] = torch.from_numpy(px).cuda(), torch.from_numpy(py).cuda()
    xm, ym = wide_x[:, :, 3:3 + dw], wide_y[:, :, 3:3 + dw]
    big = torch.full((6, 3, dh, dw), 0x3C3C, dtype=torch.int16, device="cuda")
    view = big.view(torch.float16)[2:5]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        res = pnc.remap_to_normalized_tensor(rs, surfs, xm, ym, mean, std, max_step=2.0, dtype=torch.float16, bgr=True, border=BORDER, border_mode="replicate",
                                             out=view, cc_ctx=cc)
        after = big.clone()  # ordered behind the call on the side stream
    side.synchronize()
    assert res.data_ptr() == view.data_ptr()
    h = after.cpu().numpy().view(np.uint16)
    assert (h[:2] == 0x3C3C).all() and (h[5:] == 0x3C3C).all()
    for i, (px, py) in enumerate(pairs):
        assert_bits(h[2 + i], want_bits(orc, "NV12", 1, 1, W, H, px, py, BORDER, 1, "imagenet", 1, True, seed=i), f"per-frame maps, frame {i}")
    # channels-last: a logical [N, 3, dh, dw] in torch.channels_last memory
    cl = pnc.remap_to_normalized_tensor(rs, surfs, xm, ym, mean, std, border=BORDER, cc_ctx=cc, channels_last=True)
    assert tuple(cl.shape) == (3, 3, dh, dw) and cl.is_contiguous(memory_format=torch.channels_last)
    g = cl.cpu().numpy().view(np.uint32)
    for i, (px, py) in enumerate(pairs):
        assert_bits(g[i], want_bits(orc, "NV12", 1, 1, W, H, px, py, BORDER, 0, "imagenet", 0, False, seed=i), f"channels-last, frame {i}")
    # N = 0: an empty tensor, nothing launched
    assert tuple(pnc.remap_to_normalized_tensor(rs, [], xm[:0], ym[:0], mean, std).shape) == (0, 3, dh, dw)
    good = torch.zeros((dh, dw), device="cuda")
    for bx, by in ((good.cpu(), good), (good, good.double()), (good[:, :-1], good[:, :-1]), (good.t().contiguous().t(), good), (xm[:2], ym[:2]), (xm, good),
                   (xm, wide_y[:, :, 0:dw].contiguous())):
        with pytest.raises(ValueError):
            pnc.remap_to_normalized_tensor(rs, surfs, bx, by, mean, std)
    with pytest.raises(ValueError):
        pnc.remap_to_normalized_tensor(rs, surfs, good, good, mean, std, out=torch.empty((3, 3, dh, dw), dtype=torch.float16, device="cuda"))


# ------------------------------------------------------------------------------------------------ seeded calls
@pytest.mark.parametrize("seed", _FUZZ_SEEDS)  # soak: VPF_FUZZ_SEEDS=500 (VPF_FUZZ_FIRST=n: seeds n .. n + VPF_FUZZ_SEEDS - 1, fresh cases)
def test_seeded_calls(capi, orc, seed):
    """per call: frame, source format, destination size, map kind, pitches and base alignment, border mode, dtype, channel order, layout, hint and
    knob are drawn from the seed; two jobs per call share a frame; every job is bit-identical to the reference"""
    rng = np.random.default_rng(86000 + seed)
    for case in range(3):
        W, H = FRAME_SIZES[int(rng.integers(2))]
        sf = ("NV12", "YUV420")[int(rng.integers(2))]
        dw, dh = int(rng.integers(1, 80)), int(rng.integers(1, 70))
        mode, dtype, bgr, nhwc = int(rng.integers(2)), int(rng.integers(3)), bool(rng.integers(2)), bool(rng.integers(2))
        cs, cr = MATRICES[int(rng.integers(4))]
        step = (0.0, 1e-3, 1.0, 3.0, 50.0)[int(rng.integers(5))]
        variant = 9 if rng.integers(6) == 0 else 0
        pairs, kinds = [], []
        for _ in range(2):
            kind = ("barrel", "random", "affine", "outside", "nan")[int(rng.choice(5, p=[0.3, 0.25, 0.25, 0.1, 0.1]))]
            if kind == "barrel":
                sx, sy = barrel_maps(W, H, dw, dh, k1=float(rng.uniform(-0.4, 0.3)), k2=float(rng.uniform(-0.1, 0.1)))
            elif kind == "random":
                sx, sy = random_maps(W, H, dw, dh, int(rng.integers(1 << 30)))
            elif kind == "affine":
                a, s = float(rng.uniform(0, 2 * math.pi)), float(rng.choice([0.5, 1.0, 1.4, 3.2]))
                sx, sy = warp_maps((s * math.cos(a), -s * math.sin(a), float(rng.integers(-10, W)), s * math.sin(a), s * math.cos(a), float(rng.integers(-10, H))), dw, dh, W, H, 0)
            elif kind == "outside":
                sx, sy = np.full((dh, dw), -3.5, F32), np.full((dh, dw), H / 2, F32)
            else:
                sx, sy = np.full((dh, dw), np.nan, F32), np.full((dh, dw), np.nan, F32)
            if rng.integers(2):
                sx, sy = sprinkle(sx, sy, W, H, int(rng.integers(1 << 30)))
            pairs.append((sx, sy))
            kinds.append(kind)
        geo = [dict(xpitch=4 * dw + 4 * int(rng.integers(0, 9)), ypitch=4 * dw + 4 * int(rng.integers(0, 9)), xlead=4 * int(rng.integers(0, 4)), ylead=4 * int(rng.integers(0, 4)))
               for _ in pairs]
        what = f"seed {seed} case {case}: {sf} {W}x{H} -> {dw}x{dh} kinds {kinds} maps {geo} mode {mode} dtype {dtype} bgr {bgr} nhwc {nhwc} cs{cs} cr{cr} step {step} variant {variant}"
        dev = warp.frame(orc, sf, W, H)[1]
        buf = make_buf(len(pairs), dw, dh, dtype, nhwc)
        prev = capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, variant)
        try:
            run_remap(capi, sf, cs, cr, W, H, dw, dh, [(dev, DevMaps(sx, sy, **g)) for (sx, sy), g in zip(pairs, geo)], dtype, bgr, "imagenet", buf, mode=mode,
                      max_step=step, nhwc=nhwc)
        finally:
            capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, prev)
        got, intact = buf.frames()
        assert intact, what
        for i, (sx, sy) in enumerate(pairs):
            assert_bits(got[i], want_bits(orc, sf, cs, cr, W, H, sx, sy, BORDER, mode, "imagenet", dtype, bgr, nhwc=nhwc), f"{what}, job {i}")
