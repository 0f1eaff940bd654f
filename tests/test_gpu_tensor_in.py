"""The planar float tensor -> NV12 / YUV420 path on the MI355X: vpf_tensor_convert(_batch), PyTensorToSurface and
PytorchNvCodec.from_normalized_tensor.

Ground truth comes from the CPU only: the numpy restatement of the quantiser (tests/test_tensor_in_cpu.py::quantise_numpy:
v = fl32(fl32(x * scale) + bias), clamp to [0, 255] with NaN -> 0, rint), then oracle.convert(RGB_PLANAR -> YUV420, BT.601, range, mode=FP32),
then oracle.convert(YUV420 -> NV12).  Every output byte must be identical: no tolerance, no excluded cases.  Bytes around every destination
plane hold canaries that must come back untouched (the pad byte of odd-width chroma rows included).  Pixel parity with the reference's NPP
chain is unpinned: NPP has no such call, the definition is this project's."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from gpu_util import DevPlanes, assert_planes_equal, stream_handle
from test_tensor_in_cpu import PARAM_SETS, denorm_scale_bias_f32, quantise_numpy, special_values_f32

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = 0xCD
TDT = {0: torch.float32, 1: torch.float16, 2: torch.bfloat16}
ELEM = {0: 4, 1: 2, 2: 2}
PARAMS = {name: (mean, std) for name, mean, std in PARAM_SETS}
FAST_SIZES = [(3840, 2160), (1920, 1080), (1280, 720)]
GENERIC_SIZES = [(1918, 1080), (1917, 1079), (35, 3), (2, 2), (1, 1)]
FAST, GENERIC = "k_tensor_yuv_r<", "k_tensor_yuv_quad<"


@pytest.fixture(scope="module")
def orc(oracle):
    oracle.set_threads(16)
    return oracle


_INPUTS = {}


def tensor_input(w, h, seed, params, dtype):
    """-> (torch CPU tensor [3, h, w] of the dtype, the same widened exactly to float32 numpy).  Standard-normal input for ImageNet mean / std
    (about 5 % of the elements quantise to 0 and 2 % to 255), N(0.5, 0.35) for mean 0 / std 1: both clamps are exercised."""
    key = (w, h, seed, params, dtype)
    if key not in _INPUTS:
        rng = np.random.default_rng(seed)
        x = rng.standard_normal((3, h, w), dtype=np.float32)
        if params != "imagenet":
            x = x * np.float32(0.35) + np.float32(0.5)
        t = torch.from_numpy(x).to(TDT[dtype])
        if len(_INPUTS) > 24:
            _INPUTS.clear()
        _INPUTS[key] = (t, t.to(torch.float32).numpy())
    return _INPUTS[key]


def reference(orc, widened, scale, bias, bgr, cr, dst_fmt):
    """widened: [3, h, w] float32 in input-plane order -> the NV12 / YUV420 planes, on the CPU"""
    _, h, w = widened.shape
    u8 = quantise_numpy(widened, scale, bias)
    rgb = [np.ascontiguousarray(p) for p in (u8[::-1] if bgr else u8)]
    st, yuv = orc.convert(orc.RGB_PLANAR, orc.YUV420, 0, cr, w, h, rgb, mode=orc.FP32)
    assert st == 0
    if dst_fmt == "YUV420":
        return yuv
    st, nv = orc.convert(orc.YUV420, orc.NV12, 0, cr, w, h, yuv, mode=orc.FP32)
    assert st == 0
    return nv


class TensorSrc:
    """n frames of three planes of float elements in one device byte buffer: plane (i, c) at lead + i frame + c plane, rows `row` bytes apart"""

    def __init__(self, frames, row=0, plane=0, frame=0, lead=0):
        n, (_, h, w), e = len(frames), frames[0].shape, frames[0].element_size()
        self.row = row or w * e
        self.plane = plane or h * self.row
        self.frame = frame or 3 * self.plane
        self.lead, self.n = lead, n
        size = lead + (n - 1) * self.frame + 2 * self.plane + (h - 1) * self.row + w * e + 64
        host = np.full((size,), 0xA5, dtype=np.uint8)
        for i, f in enumerate(frames):
            raw = f.contiguous().view(torch.uint8).numpy().reshape(3, h, w * e)
            for c in range(3):
                off = lead + i * self.frame + c * self.plane
                np.lib.stride_tricks.as_strided(host[off:], shape=(h, w * e), strides=(self.row, 1))[:] = raw[c]
        self.buf = torch.from_numpy(host).cuda()

    def planes(self, i):
        base = self.buf.data_ptr() + self.lead + i * self.frame
        return [(base + c * self.plane, self.row) for c in range(3)]


def dst_planes(orc, dst_fmt, w, h, **geo):
    return DevPlanes(orc.alloc(getattr(orc, dst_fmt), w, h, fill=CANARY), **geo)


def run_capi(capi, dst_fmt, cr, w, h, src, dsts, dtype, bgr, scale, bias, batch=True, frames=None):
    dn = capi.make_tensor_denorm(dtype=dtype, bgr=bgr, scale=[float(s) for s in scale], bias=[float(b) for b in bias])
    ex = capi.make_exec(stream_handle())
    frames = list(range(len(dsts))) if frames is None else frames
    if batch:
        capi.tensor_convert_batch(ex, getattr(capi, dst_fmt), 0, cr, w, h, capi.make_batch([(src.planes(f), d.desc()) for f, d in zip(frames, dsts)]), dn)
    else:
        assert len(dsts) == 1
        capi.tensor_convert(ex, getattr(capi, dst_fmt), 0, cr, w, h, src.planes(frames[0]), dsts[0].desc(), dn)
    torch.cuda.synchronize()


def check(dst, want, what):
    got, intact = dst.download()
    assert intact, f"{what}: bytes outside the destination planes were written"
    assert_planes_equal(got, want, what)
    return got


def selection_log(cases):
    """cases: (name, w, h, dtype, nv12, variant, src offset in elements, dst offset in bytes) -> {name: [launch lines]} from a child process
    under VPF_HIP_LOG=2"""
    code = f"""
import sys
sys.path.insert(0, {ROOT!r})
import torch
from videoprocessingframework_amd import capi
ex = capi.make_exec(torch.cuda.current_stream().cuda_stream)
for name, w, h, dtype, nv12, variant, soff, doff in {cases!r}:
    e = 4 if dtype == 0 else 2
    src = torch.zeros(3 * h * w * e + 64, dtype=torch.uint8, device="cuda")
    dst = torch.zeros(2 * (h + 1) * (w + 1) + 64, dtype=torch.uint8, device="cuda")
    s = [(src.data_ptr() + soff * e + c * h * w * e, w * e) for c in range(3)]
    cw, ch = (w + 1) // 2, (h + 1) // 2
    d0 = dst.data_ptr() + doff
    d = [(d0, w), (d0 + w * h, 2 * cw)] if nv12 else [(d0, w), (d0 + w * h, cw), (d0 + w * h + cw * ch, cw)]
    prev = capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, variant)
    print("CASE", name, file=sys.stderr, flush=True)
    capi.tensor_convert(ex, capi.NV12 if nv12 else capi.YUV420, 0, 1, w, h, s, d, capi.make_tensor_denorm((0, 0, 0), (1, 1, 1), dtype=dtype))
    torch.cuda.synchronize()
    capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, prev)
print("done")
"""
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, VPF_HIP_LOG="2"), timeout=300)
    assert r.returncode == 0 and "done" in r.stdout, r.stdout + r.stderr
    logs = {}
    for chunk in r.stderr.split("CASE ")[1:]:
        name, rest = chunk.split("\n", 1)
        logs[name.strip()] = [l for l in rest.split("\n") if "libvpfhip: launch" in l]
    return logs


def test_kernel_selection():
    """the kernel-selection log names the fast kernel for the decoder / model shapes in every dtype and both destinations, and the quad kernel
    for odd or unaligned shapes, for a source one element off 16-B alignment, for an offset destination and under the forced variant 9"""
    cases, want = [], {}
    for w, h in FAST_SIZES:
        for dtype in (0, 1, 2):
            for nv12 in (True, False):
                name = f"fast_{w}x{h}_{dtype}_{int(nv12)}"
                cases.append((name, w, h, dtype, nv12, 0, 0, 0))
                want[name] = (FAST, f"k_tensor_yuv_r<{dtype}, {'true' if nv12 else 'false'}, false>")  # <dtype, NV12, NHWC> as the code object has them
    for w, h in GENERIC_SIZES:
        for nv12 in (True, False):
            name = f"generic_{w}x{h}_{int(nv12)}"
            cases.append((name, w, h, (w + h) % 3, nv12, 0, 0, 0))
            want[name] = (GENERIC, f"k_tensor_yuv_quad<{'true' if nv12 else 'false'}, false>")
    cases += [("forced", 1280, 720, 0, True, 9, 0, 0), ("src_off", 1280, 720, 1, True, 0, 1, 0), ("dst_off", 1280, 720, 2, False, 0, 0, 8),
              ("yuv420_8B_chroma", 1296, 720, 0, False, 0, 0, 0)]
    want.update(forced=(GENERIC, "k_tensor_yuv_quad<true, false>"), src_off=(GENERIC, "k_tensor_yuv_quad<true, false>"), dst_off=(GENERIC, "k_tensor_yuv_quad<false, false>"),
                yuv420_8B_chroma=(FAST, "k_tensor_yuv_r<0, false, false>"))  # 1296 / 2 = 648: chroma rows 8-B, not 16-B aligned
    logs = selection_log(cases)
    for name, (family, exact) in want.items():
        lines = logs[name]
        print(name, lines)
        assert len(lines) == 1 and family in lines[0] and exact in lines[0], (name, exact, lines)


def _combos(full):
    """(destination, range, dtype, bgr, parameter set): all 48, or 12 that walk through the four (order, parameter set) pairs"""
    out = []
    for i, (dst_fmt, cr, dtype) in enumerate(itertools.product(("NV12", "YUV420"), (0, 1), (0, 1, 2))):
        for j, (bgr, params) in enumerate(itertools.product((False, True), ("imagenet", "unit"))):
            if full or j == i % 4:
                out.append((dst_fmt, cr, dtype, bgr, params))
    return out


@pytest.mark.parametrize("w,h", FAST_SIZES + GENERIC_SIZES, ids=lambda v: str(v))
def test_sizes_destinations_ranges_dtypes_orders(capi, orc, w, h):
    """both destinations x both ranges x three dtypes, with RGB / BGR order and the two parameter sets fully crossed up to 720p (walking through
    the four pairs at the larger sizes), contiguous NCHW, single-frame and batch entry: bit-identical, canaries intact"""
    full = w * h <= 1280 * 720
    combos = _combos(full)
    assert {c[0] for c in combos} == {"NV12", "YUV420"} and {c[3] for c in combos} == {False, True} and {c[4] for c in combos} == {"imagenet", "unit"}
    for k, (dst_fmt, cr, dtype, bgr, params) in enumerate(combos):
        scale, bias = denorm_scale_bias_f32(*PARAMS[params])
        t, widened = tensor_input(w, h, 7000 + w + dtype, params, dtype)
        src = TensorSrc([t])
        dst = dst_planes(orc, dst_fmt, w, h)
        run_capi(capi, dst_fmt, cr, w, h, src, [dst], dtype, bgr, scale, bias, batch=k % 2 == 0)
        check(dst, reference(orc, widened, scale, bias, bgr, cr, dst_fmt), f"{w}x{h} {dst_fmt} cr{cr} dtype{dtype} bgr{bgr} {params}")


def test_forced_generic_path_equals_the_fast_path(capi, orc):
    w, h = 1280, 720
    for dst_fmt, cr, dtype, bgr, params in _combos(False):
        scale, bias = denorm_scale_bias_f32(*PARAMS[params])
        t, widened = tensor_input(w, h, 7100 + dtype, params, dtype)
        src = TensorSrc([t])
        fast, slow = dst_planes(orc, dst_fmt, w, h), dst_planes(orc, dst_fmt, w, h)
        run_capi(capi, dst_fmt, cr, w, h, src, [fast], dtype, bgr, scale, bias)
        prev = capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, 9)
        try:
            run_capi(capi, dst_fmt, cr, w, h, src, [slow], dtype, bgr, scale, bias)
        finally:
            capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, prev)
        what = f"forced {dst_fmt} cr{cr} dtype{dtype} bgr{bgr} {params}"
        want = reference(orc, widened, scale, bias, bgr, cr, dst_fmt)
        a = check(fast, want, what + " fast")
        b = check(slow, want, what + " generic")
        assert_planes_equal(a, b, what)


@pytest.mark.parametrize("w,h", [(1280, 720), (320, 182), (35, 3)], ids=lambda v: str(v))
def test_layouts(capi, orc, w, h):
    """source: contiguous NCHW, a slice of a larger batch tensor, rows padded by 64 B (still the fast path where the shape allows) and by 16 B +
    one element (element accesses), a base one element off 16-B alignment; destination: 256-B pitches, tight pitches + 3 with the planes one
    byte off, 16-B offsets.  Three frames each, every dtype"""
    n = 3
    for dtype in (0, 1, 2):
        e = ELEM[dtype]
        frames = [tensor_input(w, h, 7200 + j, "imagenet", dtype) for j in range(n)]
        scale, bias = denorm_scale_bias_f32(*PARAMS["imagenet"])
        big = [frames[j % n][0] for j in range(n + 4)]
        src_layouts = {
            "contiguous": (TensorSrc([f[0] for f in frames]), [0, 1, 2]),
            "slice": (TensorSrc(big), [2, 3, 4]),
            "padded64": (TensorSrc([f[0] for f in frames], row=w * e + 64, plane=h * (w * e + 64) + 64, frame=3 * (h * (w * e + 64) + 64) + 256, lead=512), [0, 1, 2]),
            "padded_elem": (TensorSrc([f[0] for f in frames], row=w * e + 16 + e, plane=h * (w * e + 16 + e) + 40 * e, frame=3 * (h * (w * e + 16 + e) + 40 * e) + 8 * e,
                                      lead=24 * e), [0, 1, 2]),
            "one_off": (TensorSrc([f[0] for f in frames], lead=e), [0, 1, 2]),
        }
        dst_layouts = {"pitch256": dict(), "tight_off1": dict(align=1, extra=3, offset=1), "off16": dict(align=16, extra=16, offset=16)}
        for k, (sname, (src, idx)) in enumerate(src_layouts.items()):
            for j, (dname, geo) in enumerate(dst_layouts.items()):
                dst_fmt, cr, bgr = ("NV12", "YUV420")[(k + j) % 2], (k + j + dtype) % 2, (k + dtype) % 2 == 1
                dsts = [dst_planes(orc, dst_fmt, w, h, **geo) for _ in range(n)]
                run_capi(capi, dst_fmt, cr, w, h, src, dsts, dtype, bgr, scale, bias, frames=idx)
                for i in range(n):
                    want = reference(orc, frames[idx[i] % n][1], scale, bias, bgr, cr, dst_fmt)
                    check(dsts[i], want, f"{w}x{h} dtype{dtype} src {sname} dst {dname} {dst_fmt} cr{cr} bgr{bgr} frame {i}")


@pytest.mark.parametrize("n", [1, 3, 32, 33, 129])
def test_batch_sizes(capi, orc, n):
    """n across the 32-frame dispatch boundary, on a fast-path shape and a generic one, every dtype, each frame into its own surface"""
    for w, h in ((320, 180), (34, 6)):
        for dtype in (0, 1, 2):
            dst_fmt, cr, bgr = ("NV12", "YUV420")[dtype % 2], (dtype + n) % 2, dtype == 1
            frames = [tensor_input(w, h, 7300 + j, "unit", dtype) for j in range(5)]
            scale, bias = denorm_scale_bias_f32(*PARAMS["unit"])
            src = TensorSrc([f[0] for f in frames])
            idx = [(3 * i + i // 5) % 5 for i in range(n)]
            dsts = [dst_planes(orc, dst_fmt, w, h) for _ in range(n)]
            run_capi(capi, dst_fmt, cr, w, h, src, dsts, dtype, bgr, scale, bias, batch=n > 1, frames=idx)
            refs = [reference(orc, f[1], scale, bias, bgr, cr, dst_fmt) for f in frames]
            for i in range(n):
                check(dsts[i], refs[idx[i]], f"n{n} {w}x{h} dtype{dtype} frame {i}")


def test_special_values(capi, orc):
    """+-0, +-inf, NaN, +-3e38, every tie k + 0.5 (identity parameters scale 1 / bias 0: v = x), values around both clamps, fp32 and f16
    subnormals, in all three planes at shifted positions: through the fast kernel (64 x 16) and the quad kernel (35 x 9), every dtype"""
    sp = special_values_f32()
    one, zero = np.ones(3, np.float32), np.zeros(3, np.float32)
    for w, h in ((64, 16), (35, 9)):
        base = np.resize(sp, w * h)
        x = np.stack([np.roll(base, 7 * c).reshape(h, w) for c in range(3)])
        for dtype in (0, 1, 2):
            with np.errstate(all="ignore"):
                t = torch.from_numpy(x).to(TDT[dtype])
            widened = t.to(torch.float32).numpy()
            assert np.isnan(widened).any() and np.isinf(widened).any()
            if dtype == 1:
                sub = np.abs(t.numpy().view(np.uint16) & 0x7FFF)
                assert ((sub > 0) & (sub < 0x0400)).any()  # f16 subnormals are in
            src = TensorSrc([t])
            for dst_fmt in ("NV12", "YUV420"):
                for cr in (0, 1):
                    for sc, bi in ((one, zero), denorm_scale_bias_f32(*PARAMS["imagenet"])):
                        dst = dst_planes(orc, dst_fmt, w, h)
                        run_capi(capi, dst_fmt, cr, w, h, src, [dst], dtype, False, sc, bi, batch=False)
                        check(dst, reference(orc, widened, sc, bi, False, cr, dst_fmt), f"special {w}x{h} dtype{dtype} {dst_fmt} cr{cr} scale {sc[0]}")


def test_the_two_step_chain_on_the_device_gives_the_same_nv12(capi, orc):
    """the definition from the other side: the product's own vpf_convert(RGB_PLANAR -> YUV420) + vpf_convert(YUV420 -> NV12) on the quantised
    bytes equal the fused call"""
    for w, h in ((1280, 720), (1917, 1079)):
        for dtype, cr, bgr in ((0, 1, False), (1, 0, True), (2, 1, True)):
            scale, bias = denorm_scale_bias_f32(*PARAMS["imagenet"])
            t, widened = tensor_input(w, h, 7400, "imagenet", dtype)
            fused = dst_planes(orc, "NV12", w, h)
            run_capi(capi, "NV12", cr, w, h, TensorSrc([t]), [fused], dtype, bgr, scale, bias)
            u8 = quantise_numpy(widened, scale, bias)
            rgb = DevPlanes([np.ascontiguousarray(p) for p in (u8[::-1] if bgr else u8)])
            yuv, nv = dst_planes(orc, "YUV420", w, h), dst_planes(orc, "NV12", w, h)
            ex = capi.make_exec(stream_handle())
            capi.convert(ex, capi.RGB_PLANAR, capi.YUV420, 0, cr, w, h, rgb.desc(), yuv.desc())
            capi.convert(ex, capi.YUV420, capi.NV12, 0, cr, w, h, yuv.desc(), nv.desc())
            torch.cuda.synchronize()
            a, ia = fused.download()
            b, ib = nv.download()
            assert ia and ib
            assert_planes_equal(a, b, f"fused vs two-step {w}x{h} dtype{dtype}")


def _nvc():
    sys.path.insert(0, os.path.join(ROOT, "videoprocessingframework_amd"))
    import PyNvCodec as nvc
    from videoprocessingframework_amd import PytorchNvCodec as pnc

    return nvc, pnc


def surface_planes(pnc, orc, surf, fmt, w, h):
    """device views (no copy) of the surface's planes at their tight sizes: consumed by torch ops on torch's current stream"""
    out = []
    for k, (rows, rb, _) in enumerate(orc.plane_shapes(getattr(orc, fmt), w, h)):
        p = surf.PlanePtr(k)
        out.append(pnc.view_plane(p.GpuMem(), rb, rows, p.Pitch(), owner=surf))
    return out


def test_python_path_on_a_side_stream(orc):
    """PyTensorToSurface.Execute / ExecuteBatch and from_normalized_tensor while torch works on a non-default stream: the tensor is produced on
    that stream right before the call and the surfaces are read by torch ops on it right after, no host synchronisation in between"""
    nvc, pnc = _nvc()
    PF = nvc.PixelFormat
    w, h, n = 1280, 720, 5
    mean, std = PARAMS["imagenet"]
    scale, bias = denorm_scale_bias_f32(mean, std)
    st = torch.cuda.Stream()
    for dtype, fmt, cr, bgr in ((0, "NV12", 1, False), (1, "YUV420", 0, True), (2, "NV12", 0, False)):
        frames = [tensor_input(w, h, 7500 + i, "imagenet", dtype) for i in range(n)]
        host = torch.stack([f[0] for f in frames]).pin_memory()
        cc = nvc.ColorspaceConversionContext(nvc.ColorSpace.BT_601, nvc.ColorRange.JPEG if cr else nvc.ColorRange.MPEG)
        conv = nvc.PyTensorToSurface(w, h, getattr(PF, fmt), 0)  # the converter's own stream
        assert conv.Stream() != st.cuda_stream
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            x = host.to("cuda", non_blocking=True)
            big = torch.zeros((n + 2, 3, h, w), dtype=TDT[dtype], device="cuda")
            big[1:1 + n] = x  # produced on `st`: the converter's stream has to wait for it
            surfs = pnc.from_normalized_tensor(conv, big[1:1 + n], mean, std, bgr=bgr, cc_ctx=None if cr == 1 else cc)  # no context: JPEG range
            got = [[p.clone() for p in surface_planes(pnc, orc, s, fmt, w, h)] for s in surfs]  # consumed on `st` right away
            # out= given, a [3, H, W] tensor, and the default colour context (JPEG range)
            mine = [nvc.Surface.Make(getattr(PF, fmt), w, h, 0)]
            res = pnc.from_normalized_tensor(conv, big[2], mean, std, bgr=bgr, out=mine)
            assert len(res) == 1 and res[0] is mine[0]
            one = [p.clone() for p in surface_planes(pnc, orc, mine[0], fmt, w, h)]
        st.synchronize()
        for i in range(n):
            want = reference(orc, frames[i][1], scale, bias, bgr, cr, fmt)
            assert_planes_equal([g.cpu().numpy() for g in got[i]], want, f"from_normalized_tensor dtype{dtype} {fmt} frame {i}")
        assert_planes_equal([g.cpu().numpy() for g in one], reference(orc, frames[1][1], scale, bias, bgr, 1, fmt), f"out= dtype{dtype} {fmt}")
        # the binding itself, built on torch's side stream: Execute (own surface) and ExecuteBatch (caller's surfaces), stream-ordered with torch
        conv2 = nvc.PyTensorToSurface(w, h, getattr(PF, fmt), 0, st.cuda_stream)
        assert conv2.Stream() == st.cuda_stream and tuple(conv2.Size()) == (w, h) and conv2.Format() == getattr(PF, fmt)
        outs = [nvc.Surface.Make(getattr(PF, fmt), w, h, 0) for _ in range(n)]
        with torch.cuda.stream(st):
            y = host.to("cuda", non_blocking=True) * 1.0
            s1 = conv2.Execute(y[3].data_ptr(), dtype, list(mean), list(std), cc, bgr)
            assert not s1.Empty() and s1.Format() == getattr(PF, fmt)
            first = [p.clone() for p in surface_planes(pnc, orc, s1, fmt, w, h)]
            assert conv2.ExecuteBatch(y.data_ptr(), outs, dtype, list(mean), list(std), cc, bgr)
            rest = [[p.clone() for p in surface_planes(pnc, orc, s, fmt, w, h)] for s in outs]
        st.synchronize()
        assert_planes_equal([g.cpu().numpy() for g in first], reference(orc, frames[3][1], scale, bias, bgr, cr, fmt), f"Execute dtype{dtype} {fmt}")
        for i in range(n):
            assert_planes_equal([g.cpu().numpy() for g in rest[i]], reference(orc, frames[i][1], scale, bias, bgr, cr, fmt), f"ExecuteBatch dtype{dtype} frame {i}")
        # refusals on the device path: BT.709 context, surfaces of another size
        with pytest.raises(RuntimeError):
            pnc.from_normalized_tensor(conv, big[1:1 + n], mean, std, cc_ctx=nvc.ColorspaceConversionContext(nvc.ColorSpace.BT_709, nvc.ColorRange.MPEG))
        with pytest.raises(RuntimeError):
            pnc.from_normalized_tensor(conv, big[1:2], mean, std, out=[nvc.Surface.Make(getattr(PF, fmt), w, h + 2, 0)])
        with pytest.raises(ValueError):
            pnc.from_normalized_tensor(conv, big[1:1 + n], mean, std, out=mine)
        with pytest.raises(ValueError):
            pnc.from_normalized_tensor(conv, big[1:1 + n].transpose(2, 3), mean, std)
        torch.cuda.synchronize()


def test_expanded_tensors_are_refused_and_their_contiguous_copies_convert(orc):
    """a zero stride would be read by the binding as "contiguous" (an out-of-bounds read with wrong pixels), so expand()ed channels, frames
    and rows are refused on the device path too; the .contiguous() copy of a one-channel output shown as three planes converts, bit for bit"""
    nvc, pnc = _nvc()
    PF = nvc.PixelFormat
    w, h, n = 320, 180, 2
    mean, std = PARAMS["imagenet"]
    scale, bias = denorm_scale_bias_f32(mean, std)
    conv = nvc.PyTensorToSurface(w, h, PF.NV12, 0)
    assert conv.Device() == 0
    frames = [tensor_input(w, h, 7800 + i, "imagenet", 0) for i in range(n)]
    gray = torch.stack([f[0][:1] for f in frames]).cuda()  # [n, 1, h, w]
    shown = gray.expand(-1, 3, -1, -1)
    assert shown.stride(1) == 0
    for bad in (shown, shown[0], gray[:1].expand(n, -1, -1, -1).expand(-1, 3, -1, -1), gray[:, :, :1].expand(-1, 3, h, -1)):
        with pytest.raises(ValueError, match="contiguous"):
            pnc.from_normalized_tensor(conv, bad, mean, std)
    surfs = pnc.from_normalized_tensor(conv, shown.contiguous(), mean, std)
    got = [[p.clone() for p in surface_planes(pnc, orc, s, "NV12", w, h)] for s in surfs]
    torch.cuda.synchronize()
    for i in range(n):
        widened = np.repeat(frames[i][1][:1], 3, axis=0)
        assert_planes_equal([g.cpu().numpy() for g in got[i]], reference(orc, widened, scale, bias, False, 1, "NV12"), f"expanded gray frame {i}")
    # a single frame and a single row: the strides of one-element dimensions are never walked, whatever torch reports for them
    one = pnc.from_normalized_tensor(conv, gray[1:2].expand(-1, 3, -1, -1).contiguous()[0], mean, std)
    got1 = [p.clone() for p in surface_planes(pnc, orc, one[0], "NV12", w, h)]
    torch.cuda.synchronize()
    assert_planes_equal([g.cpu().numpy() for g in got1], reference(orc, np.repeat(frames[1][1][:1], 3, axis=0), scale, bias, False, 1, "NV12"), "single frame")


def test_graph_capture(orc):
    """the batched call captured in a torch.cuda.graph on one stream (the converter's), replayed twice into cleared surfaces"""
    nvc, pnc = _nvc()
    PF = nvc.PixelFormat
    w, h, n = 640, 360, 9  # 640 % 16 == 0: the fast kernel; 33 frames would be two dispatches, 9 is one
    mean, std = PARAMS["unit"]
    scale, bias = denorm_scale_bias_f32(mean, std)
    st = torch.cuda.Stream()
    conv = nvc.PyTensorToSurface(w, h, PF.NV12, 0, st.cuda_stream)
    frames = [tensor_input(w, h, 7600 + i, "unit", 1) for i in range(n)]
    x = torch.stack([f[0] for f in frames]).cuda()
    surfs = [nvc.Surface.Make(PF.NV12, w, h, 0) for _ in range(n)]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        pnc.from_normalized_tensor(conv, x, mean, std, out=surfs)
    for rep in range(2):
        for s in surfs:
            for p in surface_planes(pnc, orc, s, "NV12", w, h):
                p.fill_(0)
        torch.cuda.synchronize()
        g.replay()
        st.synchronize()
        torch.cuda.synchronize()
        for i in range(n):
            got = [p.cpu().numpy() for p in surface_planes(pnc, orc, surfs[i], "NV12", w, h)]
            assert_planes_equal(got, reference(orc, frames[i][1], scale, bias, False, 1, "NV12"), f"graph replay {rep} frame {i}")


def test_round_trip_keeps_luma_within_one(orc):
    """A sanity check, not a parity claim: NV12 -> to_normalized_tensor (equal size, BT.601 JPEG, f32) -> from_normalized_tensor (JPEG) -> NV12.

    Bound on luma, derived: the frame's chroma is constant and mild (|U - 128|, |V - 128| <= 16) and 64 <= Y <= 192, so no channel clamps.
    Forward, each of R G B is the real value r* of the BT.601 JPEG matrix rounded to 8 bits: |R - r*| <= 0.5.  The normalisation and its
    inverse return that byte exactly (tests/test_tensor_in_cpu.py::test_mean_std_to_scale_bias: every code survives the fp32 round trip).
    Back, Y' = floor(0.299 R + 0.587 G + 0.114 B + 0.5).  The reals satisfy 0.299 r* + 0.587 g* + 0.114 b* = Y + m with |m| <= 0.00037 x 16 +
    0.00019 x 16 < 0.01 (the published decimal matrices are not exact inverses), so |0.299 R + 0.587 G + 0.114 B - Y| <= 0.5 x (0.299 + 0.587 +
    0.114) + 0.01 + fp32 noise < 1, and the second rounding lands on Y - 1, Y or Y + 1: |Y' - Y| <= 1."""
    nvc, pnc = _nvc()
    PF = nvc.PixelFormat
    w, h = 1280, 720
    mean, std = PARAMS["imagenet"]
    rng = np.random.default_rng(7700)
    y = rng.integers(64, 193, size=(h, w), dtype=np.uint8)
    uv = np.empty((h // 2, w), np.uint8)
    uv[:, 0::2], uv[:, 1::2] = 128 + 13, 128 - 16
    up = nvc.PyFrameUploader(w, h, PF.NV12, 0)
    surf = up.UploadSingleFrame(np.concatenate([y.reshape(-1), uv.reshape(-1)])).Clone(0)
    torch.cuda.synchronize()
    cc = nvc.ColorspaceConversionContext(nvc.ColorSpace.BT_601, nvc.ColorRange.JPEG)
    fwd = nvc.PySurfaceConvertResizer(w, h, PF.NV12, w, h, PF.RGB_PLANAR, 0)
    back = nvc.PyTensorToSurface(w, h, PF.NV12, 0)
    x = pnc.to_normalized_tensor(fwd, [surf], mean, std, cc_ctx=cc)
    out = pnc.from_normalized_tensor(back, x, mean, std, cc_ctx=cc)
    planes = [p.clone() for p in surface_planes(pnc, orc, out[0], "NV12", w, h)]
    torch.cuda.synchronize()
    y2 = planes[0].cpu().numpy().astype(np.int32)
    worst = int(np.abs(y2 - y.astype(np.int32)).max())
    print("round trip: largest |Y' - Y| =", worst, "; share of exact luma", float((y2 == y).mean()))
    assert worst <= 1
