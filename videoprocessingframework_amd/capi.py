"""ctypes binding of the C ABI in include/vpf_hip.h (libvpfhip.so).

This is the thinnest possible Python view of the drop-in boundary: it passes raw device pointers,
pitches and a hipStream_t, exactly as the reference's Task layer hands them to NPP
(src/TC/src/TasksColorCvt.cpp:122-182).  There is no CPU fallback: if libvpfhip.so is missing or a
launch fails, these functions raise.
"""
from __future__ import annotations

import ctypes as C
import os

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "libvpfhip.so")

# Pixel_Format (reference: src/TC/inc/MemoryInterfaces.hpp:30-49)
UNDEFINED, Y, RGB, NV12, YUV420, RGB_PLANAR, BGR, YCBCR, YUV444, RGB_32F, RGB_32F_PLANAR, YUV422, P10, P12 = range(14)
YUV444_10bit, YUV420_10bit, NV12_PLANAR, GRAY12 = 14, 15, 16, 17
BT_601, BT_709, CS_UNSPEC = 0, 1, 2
MPEG, JPEG, CR_UDEF = 0, 1, 2
INTERP_NEAREST, INTERP_LINEAR, INTERP_LANCZOS3 = 0, 1, 2
OK, ERR_UNSUPPORTED, ERR_BAD_ARG, ERR_LAUNCH, ERR_NO_DEVICE = range(5)
TUNE_NV12_RGB_VARIANT = 1
TUNE_RESIZE_TILE = 2
TUNE_RESIZE_BAND = 3
TUNE_RESIZE_MFMA = 5

EXPORTS = [
    "vpf_convert", "vpf_convert_batch", "vpf_convert_supported", "vpf_resize", "vpf_remap", "vpf_convert_resize",
    "vpf_convert_resize_batch", "vpf_resize_batch", "vpf_remap_batch", "vpf_resize_ws", "vpf_resize_batch_ws", "vpf_resize_workspace_bytes",
    "vpf_status_string", "vpf_version", "vpf_device_count", "vpf_set_tuning", "vpf_trace_push", "vpf_trace_pop",
    "vpf_convert_resize_tensor", "vpf_convert_resize_tensor_batch", "vpf_convert_resize_tensor_rois", "vpf_convert_warp_tensor",
    "vpf_tensor_convert_supported", "vpf_tensor_convert", "vpf_tensor_convert_batch",
    "vpf_convert_letterbox_tensor", "vpf_letterbox_fit", "vpf_convert_resize_tensor_rois_dev", "vpf_convert_warp_tensor_dev",
    "vpf_convert_persp_tensor", "vpf_convert_letterbox_tensor_dev", "vpf_convert_persp_tensor_dev", "vpf_persp_max_step",
    "vpf_convert_remap_tensor", "vpf_convert_letterbox_tensor_aa",
]
TENSOR_F32, TENSOR_F16, TENSOR_BF16 = 0, 1, 2
TENSOR_BGR = 1
TENSOR_NHWC = 4  # one interleaved plane [H, W, 3] per frame (dst[0] / src[0]) instead of three planes


class Workspace(C.Structure):
    """vpf_workspace: caller-owned scratch region for per-shape filter tables (include/vpf_hip.h); `opaque` starts zeroed"""
    _fields_ = [("ptr", C.c_void_p), ("bytes", C.c_uint64), ("opaque", C.c_uint64 * 40)]


class Plane(C.Structure):
    _fields_ = [("ptr", C.c_void_p), ("pitch", C.c_uint32), ("reserved", C.c_uint32)]


class Size(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32)]


class Exec(C.Structure):
    _fields_ = [("device", C.c_int32), ("flags", C.c_uint32), ("stream", C.c_void_p)]


class FrameIO(C.Structure):
    _fields_ = [("src", Plane * 3), ("dst", Plane * 3)]


class Rect(C.Structure):
    _fields_ = [("x", C.c_uint32), ("y", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32)]


class RoiIO(C.Structure):
    """vpf_roi_io: one job of vpf_convert_resize_tensor_rois — the WHOLE source frame's planes, the destination planes, the rectangle"""
    _fields_ = [("src", Plane * 3), ("dst", Plane * 3), ("rect", Rect)]


class WarpIO(C.Structure):
    """vpf_warp_io: one job of vpf_convert_warp_tensor — the WHOLE source frame's planes, the destination planes, the inverse 2 x 3 matrix"""
    _fields_ = [("src", Plane * 3), ("dst", Plane * 3), ("m", C.c_float * 6)]


class PerspIO(C.Structure):
    """vpf_persp_io: one job of vpf_convert_persp_tensor — the WHOLE source frame's planes, the destination planes, the inverse 3 x 3 matrix"""
    _fields_ = [("src", Plane * 3), ("dst", Plane * 3), ("m", C.c_float * 9), ("reserved", C.c_uint32)]


class WarpOpts(C.Structure):
    """vpf_warp_opts: border mode (WARP_CONSTANT / WARP_REPLICATE) and the border bytes per output channel"""
    _fields_ = [("border_mode", C.c_uint32), ("border", C.c_uint8 * 3), ("reserved", C.c_uint8)]


WARP_CONSTANT, WARP_REPLICATE = 0, 1


class RemapIO(C.Structure):
    """vpf_remap_io: one job of vpf_convert_remap_tensor — the WHOLE source frame's planes, the destination planes, the job's two coordinate maps
    (DEVICE addresses) and their pitches in bytes"""
    _fields_ = [("src", Plane * 3), ("dst", Plane * 3), ("xmap", C.c_void_p), ("ymap", C.c_void_p), ("xmap_pitch", C.c_uint32), ("ymap_pitch", C.c_uint32)]


class RemapOpts(C.Structure):
    """vpf_remap_opts: vpf_warp_opts plus the LDS hint (0: none)"""
    _fields_ = [("border_mode", C.c_uint32), ("border", C.c_uint8 * 3), ("reserved", C.c_uint8), ("max_step", C.c_float), ("reserved2", C.c_uint32)]


class LetterboxIO(C.Structure):
    """vpf_letterbox_io: one job of vpf_convert_letterbox_tensor — the WHOLE source frame's planes, the WHOLE destination planes, the source
    rectangle and where the picture goes inside the destination"""
    _fields_ = [("src", Plane * 3), ("dst", Plane * 3), ("rect", Rect), ("dst_rect", Rect)]


class LetterboxOpts(C.Structure):
    """vpf_letterbox_opts: the pad bytes per output channel"""
    _fields_ = [("pad", C.c_uint8 * 3), ("reserved", C.c_uint8)]


class RoiDev(C.Structure):
    """vpf_roi_dev: one box of vpf_convert_resize_tensor_rois_dev as it lies in DEVICE memory — a row of a torch.int32 [K, 5] tensor"""
    _fields_ = [("frame", C.c_int32), ("x", C.c_int32), ("y", C.c_int32), ("width", C.c_int32), ("height", C.c_int32)]


class FrameSrc(C.Structure):
    """vpf_frame_src: the planes of one WHOLE source frame"""
    _fields_ = [("src", Plane * 3)]


class RoisDev(C.Structure):
    """vpf_rois_dev: where the boxes and their count lie (device pointers), how many jobs the dispatch holds, job 0's planes and the stride"""
    _fields_ = [("boxes", C.c_void_p), ("count", C.c_void_p), ("box_stride", C.c_uint32), ("max_n", C.c_uint32), ("dst", Plane * 3),
                ("dst_job_stride", C.c_uint64)]


class LetterboxDev(C.Structure):
    """vpf_letterbox_dev: where the boxes, the optional placements and the count lie (device pointers), how many jobs the dispatch holds, job 0's WHOLE
    planes and the stride"""
    _fields_ = [("boxes", C.c_void_p), ("dst_rects", C.c_void_p), ("count", C.c_void_p), ("box_stride", C.c_uint32), ("rect_stride", C.c_uint32),
                ("max_n", C.c_uint32), ("reserved", C.c_uint32), ("dst", Plane * 3), ("dst_job_stride", C.c_uint64)]


class WarpsDev(C.Structure):
    """vpf_warps_dev: where the matrices, their frame indices and the count lie (device pointers), how many jobs the dispatch holds, the LDS hint, job 0's
    planes and the stride"""
    _fields_ = [("matrices", C.c_void_p), ("frame_index", C.c_void_p), ("count", C.c_void_p), ("matrix_stride", C.c_uint32), ("frame_stride", C.c_uint32),
                ("max_n", C.c_uint32), ("max_step", C.c_float), ("dst", Plane * 3), ("dst_job_stride", C.c_uint64)]


class PerspsDev(C.Structure):
    """vpf_persps_dev: vpf_warps_dev with nine floats per job (the inverse 3 x 3 matrix): the same 96 bytes"""
    _fields_ = WarpsDev._fields_


class TensorNorm(C.Structure):
    """vpf_tensor_norm: out[c] = round_to_dtype(fmaf(u8[c], scale[c], bias[c])) (include/vpf_hip.h)"""
    _fields_ = [("scale", C.c_float * 3), ("bias", C.c_float * 3), ("dtype", C.c_uint32), ("flags", C.c_uint32)]


def norm_params(mean, std):
    """torchvision's normalize(mean, std) after a division by 255 as (scale, bias): scale = 1 / (255 std), bias = -mean / std, computed in
    double and rounded to fp32 (the ctypes fields round).  std must be > 0 and every value finite."""
    import math

    mean, std = [float(m) for m in mean], [float(s) for s in std]
    if len(mean) != 3 or len(std) != 3:
        raise ValueError("mean and std need three values each")
    if not all(math.isfinite(v) for v in mean + std) or min(std) <= 0:
        raise ValueError("mean must be finite and std finite and > 0")
    return [1.0 / (255.0 * s) for s in std], [-m / s for m, s in zip(mean, std)]


def denorm_params(mean, std):
    """the way back (vpf_tensor_convert): a tensor normalised with torchvision's normalize(mean, std) of [0, 1] pixels -> 8-bit codes,
    as (scale, bias): scale = 255 std, bias = 255 mean, computed in double and rounded to fp32 (the ctypes fields round).  std must be > 0
    and every value finite."""
    import math

    mean, std = [float(m) for m in mean], [float(s) for s in std]
    if len(mean) != 3 or len(std) != 3:
        raise ValueError("mean and std need three values each")
    if not all(math.isfinite(v) for v in mean + std) or min(std) <= 0:
        raise ValueError("mean must be finite and std finite and > 0")
    return [255.0 * s for s in std], [255.0 * m for m in mean]


def make_tensor_denorm(mean=None, std=None, dtype=TENSOR_F32, bgr=False, scale=None, bias=None, nhwc=False) -> TensorNorm:
    """vpf_tensor_norm for vpf_tensor_convert from mean / std (denorm_params) or from raw scale / bias (passed through unchecked)"""
    if scale is None:
        scale, bias = denorm_params(mean, std)
    return make_tensor_norm(dtype=dtype, bgr=bgr, scale=scale, bias=bias, nhwc=nhwc)


def make_tensor_norm(mean=None, std=None, dtype=TENSOR_F32, bgr=False, scale=None, bias=None, nhwc=False) -> TensorNorm:
    """vpf_tensor_norm from mean / std (norm_params) or from raw scale / bias (passed through unchecked: the library validates them)"""
    if scale is None:
        scale, bias = norm_params(mean, std)
    n = TensorNorm()
    for c in range(3):
        n.scale[c], n.bias[c] = scale[c], bias[c]
    n.dtype, n.flags = dtype, (TENSOR_BGR if bgr else 0) | (TENSOR_NHWC if nhwc else 0)
    return n


class VpfError(RuntimeError):
    def __init__(self, status: int, what: str):
        self.status = status
        super().__init__(f"{what}: {status_string(status)} (vpf_status {status})")


_lib = None


def lib() -> C.CDLL:
    """Load libvpfhip.so; raises (never falls back) when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} not found: build it with `python -m videoprocessingframework_amd._build` "
                "(there is no CPU fallback for the conversion path)")
        from ._hip_runtime import preload

        preload()  # one HIP runtime per process, whatever the import order relative to torch
        L = C.CDLL(LIB_PATH)
        PP, PE, PF = C.POINTER(Plane), C.POINTER(Exec), C.POINTER(FrameIO)
        L.vpf_convert.argtypes = [PE, C.c_int, C.c_int, C.c_int, C.c_int, Size, PP, PP]
        L.vpf_convert_batch.argtypes = [PE, C.c_int, C.c_int, C.c_int, C.c_int, Size, C.c_uint32, PF]
        L.vpf_convert_supported.argtypes = [C.c_int] * 4
        L.vpf_resize.argtypes = [PE, C.c_int, C.c_int, Size, PP, Size, PP]
        L.vpf_remap.argtypes = [PE, C.c_int, Size, PP, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, Size, PP]
        L.vpf_convert_resize.argtypes = [PE, C.c_int, C.c_int, C.c_int, C.c_int, Size, PP, Size, PP]
        L.vpf_convert_resize_batch.argtypes = [PE, C.c_int, C.c_int, C.c_int, C.c_int, Size, Size, C.c_uint32, PF]
        L.vpf_resize_batch.argtypes = [PE, C.c_int, C.c_int, Size, Size, C.c_uint32, PF]
        L.vpf_remap_batch.argtypes = [PE, C.c_int, Size, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, Size, C.c_uint32, PF]
        L.vpf_resize_ws.argtypes = [PE, C.c_int, C.c_int, Size, PP, Size, PP, C.POINTER(Workspace)]
        L.vpf_resize_batch_ws.argtypes = [PE, C.c_int, C.c_int, Size, Size, C.c_uint32, PF, C.POINTER(Workspace)]
        L.vpf_resize_workspace_bytes.argtypes = [C.c_int, C.c_int, Size, Size]
        L.vpf_resize_workspace_bytes.restype = C.c_uint64
        PN = C.POINTER(TensorNorm)
        L.vpf_convert_resize_tensor.argtypes = [PE, C.c_int, C.c_int, C.c_int, Size, PP, Size, PP, PN]
        L.vpf_convert_resize_tensor_batch.argtypes = [PE, C.c_int, C.c_int, C.c_int, Size, Size, C.c_uint32, PF, PN]
        L.vpf_convert_resize_tensor_rois.argtypes = [PE, C.c_int, C.c_int, C.c_int, Size, Size, C.c_uint32, C.POINTER(RoiIO), PN]
        L.vpf_convert_warp_tensor.argtypes = [PE, C.c_int, C.c_int, C.c_int, Size, Size, C.c_uint32, C.POINTER(WarpIO), PN, C.POINTER(WarpOpts)]
        L.vpf_convert_persp_tensor.argtypes = [PE, C.c_int, C.c_int, C.c_int, Size, Size, C.c_uint32, C.POINTER(PerspIO), PN, C.POINTER(WarpOpts)]
        L.vpf_convert_letterbox_tensor.argtypes = [PE, C.c_int, C.c_int, C.c_int, Size, Size, C.c_uint32, C.POINTER(LetterboxIO), PN,
                                                   C.POINTER(LetterboxOpts)]
        L.vpf_convert_letterbox_tensor_aa.argtypes = L.vpf_convert_letterbox_tensor.argtypes
        L.vpf_convert_resize_tensor_rois_dev.argtypes = [PE, C.c_int, C.c_int, C.c_int, Size, Size, C.c_uint32, C.POINTER(FrameSrc), C.POINTER(RoisDev), PN]
        L.vpf_convert_warp_tensor_dev.argtypes = [PE, C.c_int, C.c_int, C.c_int, Size, Size, C.c_uint32, C.POINTER(FrameSrc), C.POINTER(WarpsDev), PN,
                                                  C.POINTER(WarpOpts)]
        L.vpf_convert_persp_tensor_dev.argtypes = [PE, C.c_int, C.c_int, C.c_int, Size, Size, C.c_uint32, C.POINTER(FrameSrc), C.POINTER(PerspsDev), PN,
                                                   C.POINTER(WarpOpts)]
        L.vpf_convert_remap_tensor.argtypes = [PE, C.c_int, C.c_int, C.c_int, Size, Size, C.c_uint32, C.POINTER(RemapIO), PN, C.POINTER(RemapOpts)]
        L.vpf_persp_max_step.argtypes = [C.POINTER(C.c_float), Size]
        L.vpf_persp_max_step.restype = C.c_float
        L.vpf_convert_letterbox_tensor_dev.argtypes = [PE, C.c_int, C.c_int, C.c_int, Size, Size, C.c_uint32, C.POINTER(FrameSrc), C.POINTER(LetterboxDev), PN,
                                                       C.POINTER(LetterboxOpts)]
        L.vpf_letterbox_fit.argtypes = [Size, Size]
        L.vpf_letterbox_fit.restype = Rect
        L.vpf_tensor_convert_supported.argtypes = [C.c_int] * 3
        L.vpf_tensor_convert.argtypes = [PE, C.c_int, C.c_int, C.c_int, Size, PP, PP, PN]
        L.vpf_tensor_convert_batch.argtypes = [PE, C.c_int, C.c_int, C.c_int, Size, C.c_uint32, PF, PN]
        L.vpf_status_string.argtypes = [C.c_int]
        L.vpf_status_string.restype = C.c_char_p
        L.vpf_version.restype = C.c_char_p
        L.vpf_set_tuning.argtypes = [C.c_int, C.c_int]
        _lib = L
    return _lib


def status_string(s: int) -> str:
    return lib().vpf_status_string(s).decode()


def version() -> str:
    return lib().vpf_version().decode()


def device_count() -> int:
    return lib().vpf_device_count()


def set_tuning(key: int, value: int) -> int:
    return lib().vpf_set_tuning(key, value)


def convert_supported(src_fmt, dst_fmt, cs, cr) -> bool:
    return bool(lib().vpf_convert_supported(src_fmt, dst_fmt, cs, cr))


EXEC_DST_REUSED = 1


def make_exec(stream: int = 0, device: int = -1, flags: int = 0) -> Exec:
    return Exec(device, flags, stream or None)


def planes(desc) -> "C.Array[Plane]":
    """desc: iterable of (device_ptr, pitch_bytes), at most 3; an array built earlier is passed through (callers in a
    per-frame loop build their descriptors once)."""
    if isinstance(desc, Plane * 3):
        return desc
    p = (Plane * 3)()
    for i, (ptr, pitch) in enumerate(desc):
        p[i].ptr, p[i].pitch = ptr, pitch
    return p


def _check(st: int, what: str):
    if st != OK:
        raise VpfError(st, what)


def convert(ex: Exec, src_fmt, dst_fmt, cs, cr, w, h, src, dst, check=True) -> int:
    st = lib().vpf_convert(C.byref(ex), src_fmt, dst_fmt, cs, cr, Size(w, h), planes(src), planes(dst))
    if check:
        _check(st, "vpf_convert")
    return st


def make_batch(frames) -> "C.Array[FrameIO]":
    """frames: list of (src_desc, dst_desc) with desc as in planes()."""
    arr = (FrameIO * len(frames))()
    for i, (s, d) in enumerate(frames):
        s, d = planes(s), planes(d)  # accepts (ptr, pitch) lists and prebuilt Plane arrays alike
        for k in range(3):
            arr[i].src[k].ptr, arr[i].src[k].pitch = s[k].ptr, s[k].pitch
            arr[i].dst[k].ptr, arr[i].dst[k].pitch = d[k].ptr, d[k].pitch
    return arr


def convert_batch(ex: Exec, src_fmt, dst_fmt, cs, cr, w, h, batch, n=None, check=True) -> int:
    st = lib().vpf_convert_batch(C.byref(ex), src_fmt, dst_fmt, cs, cr, Size(w, h), len(batch) if n is None else n, batch)
    if check:
        _check(st, "vpf_convert_batch")
    return st


def resize(ex: Exec, fmt, interp, sw, sh, src, dw, dh, dst, check=True) -> int:
    st = lib().vpf_resize(C.byref(ex), fmt, interp, Size(sw, sh), planes(src), Size(dw, dh), planes(dst))
    if check:
        _check(st, "vpf_resize")
    return st


def resize_batch(ex: Exec, fmt, interp, sw, sh, dw, dh, batch, n=None, check=True) -> int:
    """batch: FrameIO array from make_batch(); every plane of every frame in as few dispatches as possible"""
    st = lib().vpf_resize_batch(C.byref(ex), fmt, interp, Size(sw, sh), Size(dw, dh), len(batch) if n is None else n, batch)
    if check:
        _check(st, "vpf_resize_batch")
    return st


def resize_workspace_bytes(fmt, interp, sw, sh, dw, dh) -> int:
    return int(lib().vpf_resize_workspace_bytes(fmt, interp, Size(sw, sh), Size(dw, dh)))


def make_workspace(ptr: int, nbytes: int) -> Workspace:
    """a zeroed vpf_workspace over `nbytes` of device memory at `ptr` (256-B aligned), which the caller keeps alive"""
    ws = Workspace()
    ws.ptr, ws.bytes = ptr, nbytes
    return ws


def resize_ws(ex: Exec, fmt, interp, sw, sh, src, dw, dh, dst, ws, check=True) -> int:
    st = lib().vpf_resize_ws(C.byref(ex), fmt, interp, Size(sw, sh), planes(src), Size(dw, dh), planes(dst), C.byref(ws) if ws is not None else None)
    if check:
        _check(st, "vpf_resize_ws")
    return st


def resize_batch_ws(ex: Exec, fmt, interp, sw, sh, dw, dh, batch, ws, n=None, check=True) -> int:
    st = lib().vpf_resize_batch_ws(C.byref(ex), fmt, interp, Size(sw, sh), Size(dw, dh), len(batch) if n is None else n, batch,
                                   C.byref(ws) if ws is not None else None)
    if check:
        _check(st, "vpf_resize_batch_ws")
    return st


def remap_batch(ex: Exec, fmt, sw, sh, xmap_ptr, xmap_pitch, ymap_ptr, ymap_pitch, dw, dh, batch, n=None, check=True) -> int:
    st = lib().vpf_remap_batch(C.byref(ex), fmt, Size(sw, sh), xmap_ptr, xmap_pitch, ymap_ptr, ymap_pitch, Size(dw, dh), len(batch) if n is None else n, batch)
    if check:
        _check(st, "vpf_remap_batch")
    return st


def remap(ex: Exec, fmt, sw, sh, src, xmap_ptr, xmap_pitch, ymap_ptr, ymap_pitch, dw, dh, dst, check=True) -> int:
    st = lib().vpf_remap(C.byref(ex), fmt, Size(sw, sh), planes([src]), xmap_ptr, xmap_pitch, ymap_ptr, ymap_pitch,
                         Size(dw, dh), planes([dst]))
    if check:
        _check(st, "vpf_remap")
    return st


def convert_resize(ex: Exec, src_fmt, dst_fmt, cs, cr, sw, sh, src, dw, dh, dst, check=True) -> int:
    st = lib().vpf_convert_resize(C.byref(ex), src_fmt, dst_fmt, cs, cr, Size(sw, sh), planes(src), Size(dw, dh),
                                  planes(dst))
    if check:
        _check(st, "vpf_convert_resize")
    return st


def convert_resize_batch(ex: Exec, src_fmt, dst_fmt, cs, cr, sw, sh, dw, dh, batch, n=None, check=True) -> int:
    st = lib().vpf_convert_resize_batch(C.byref(ex), src_fmt, dst_fmt, cs, cr, Size(sw, sh), Size(dw, dh),
                                        len(batch) if n is None else n, batch)
    if check:
        _check(st, "vpf_convert_resize_batch")
    return st


def convert_resize_tensor(ex: Exec, src_fmt, cs, cr, sw, sh, src, dw, dh, dst, norm: TensorNorm, check=True) -> int:
    """dst: the three planes (ptr, pitch in bytes) of the tensor frame in output channel order"""
    st = lib().vpf_convert_resize_tensor(C.byref(ex), src_fmt, cs, cr, Size(sw, sh), planes(src), Size(dw, dh), planes(dst), C.byref(norm))
    if check:
        _check(st, "vpf_convert_resize_tensor")
    return st


def convert_resize_tensor_batch(ex: Exec, src_fmt, cs, cr, sw, sh, dw, dh, batch, norm: TensorNorm, n=None, check=True) -> int:
    st = lib().vpf_convert_resize_tensor_batch(C.byref(ex), src_fmt, cs, cr, Size(sw, sh), Size(dw, dh), len(batch) if n is None else n, batch,
                                               C.byref(norm))
    if check:
        _check(st, "vpf_convert_resize_tensor_batch")
    return st


def make_rois(jobs) -> "C.Array[RoiIO]":
    """jobs: list of (src_desc, dst_desc, (x, y, w, h)) with desc as in planes(); src_desc = the planes of the WHOLE frame"""
    arr = (RoiIO * len(jobs))()
    for i, (s, d, rect) in enumerate(jobs):
        s, d = planes(s), planes(d)
        for k in range(3):
            arr[i].src[k].ptr, arr[i].src[k].pitch = s[k].ptr, s[k].pitch
            arr[i].dst[k].ptr, arr[i].dst[k].pitch = d[k].ptr, d[k].pitch
        arr[i].rect.x, arr[i].rect.y, arr[i].rect.width, arr[i].rect.height = rect
    return arr


def convert_resize_tensor_rois(ex: Exec, src_fmt, cs, cr, sw, sh, dw, dh, rois, norm: TensorNorm, n=None, check=True) -> int:
    """rois: RoiIO array from make_rois(); every rectangle resized to dw x dh and normalised, 96 jobs per job table"""
    st = lib().vpf_convert_resize_tensor_rois(C.byref(ex), src_fmt, cs, cr, Size(sw, sh), Size(dw, dh), len(rois) if n is None else n, rois,
                                              C.byref(norm) if norm is not None else None)
    if check:
        _check(st, "vpf_convert_resize_tensor_rois")
    return st


def make_frame_srcs(frames) -> "C.Array[FrameSrc]":
    """frames: list of src_desc as in planes(): the planes of each WHOLE frame"""
    arr = (FrameSrc * len(frames))()
    for i, s in enumerate(frames):
        s = planes(s)
        for k in range(3):
            arr[i].src[k].ptr, arr[i].src[k].pitch = s[k].ptr, s[k].pitch
    return arr


def make_rois_dev(boxes_ptr, max_n, dst, dst_job_stride, count_ptr=None, box_stride=20) -> RoisDev:
    """vpf_rois_dev: boxes_ptr / count_ptr are DEVICE addresses (count_ptr None: max_n jobs), dst = job 0's planes as in planes(), dst_job_stride =
    bytes from one job's planes to the next's"""
    t = RoisDev()
    t.boxes, t.count, t.box_stride, t.max_n, t.dst_job_stride = boxes_ptr or None, count_ptr or None, box_stride, max_n, dst_job_stride
    d = planes(dst)
    for k in range(3):
        t.dst[k].ptr, t.dst[k].pitch = d[k].ptr, d[k].pitch
    return t


def convert_resize_tensor_rois_dev(ex: Exec, src_fmt, cs, cr, sw, sh, dw, dh, frames, table: RoisDev, norm: TensorNorm, n_frames=None, check=True) -> int:
    """frames: FrameSrc array from make_frame_srcs() (at most 128), table: make_rois_dev(); the kernel reads boxes and count when it runs on
    ex.stream: no sync, no copy, capturable"""
    st = lib().vpf_convert_resize_tensor_rois_dev(C.byref(ex) if ex is not None else None, src_fmt, cs, cr, Size(sw, sh), Size(dw, dh),
                                                  (len(frames) if frames is not None else 0) if n_frames is None else n_frames, frames,
                                                  C.byref(table) if table is not None else None, C.byref(norm) if norm is not None else None)
    if check:
        _check(st, "vpf_convert_resize_tensor_rois_dev")
    return st


def make_warps(jobs) -> "C.Array[WarpIO]":
    """jobs: list of (src_desc, dst_desc, m) with desc as in planes(); src_desc = the planes of the WHOLE frame, m = six floats
    (m00 m01 m02 m10 m11 m12) or a 2 x 3 nested sequence: destination pixel -> source coordinates"""
    arr = (WarpIO * len(jobs))()
    for i, (s, d, m) in enumerate(jobs):
        s, d = planes(s), planes(d)
        for k in range(3):
            arr[i].src[k].ptr, arr[i].src[k].pitch = s[k].ptr, s[k].pitch
            arr[i].dst[k].ptr, arr[i].dst[k].pitch = d[k].ptr, d[k].pitch
        flat = [v for row in m for v in row] if len(m) == 2 else list(m)
        for k in range(6):
            arr[i].m[k] = flat[k]
    return arr


def make_warp_opts(border_mode=WARP_CONSTANT, border=(0, 0, 0)) -> WarpOpts:
    o = WarpOpts()
    o.border_mode = border_mode
    for k in range(3):
        o.border[k] = border[k]
    return o


def convert_warp_tensor(ex: Exec, src_fmt, cs, cr, sw, sh, dw, dh, warps, norm: TensorNorm, opts: WarpOpts = None, n=None, check=True) -> int:
    """warps: WarpIO array from make_warps(); every job sampled through its matrix into dw x dh and normalised, 96 jobs per job table"""
    st = lib().vpf_convert_warp_tensor(C.byref(ex), src_fmt, cs, cr, Size(sw, sh), Size(dw, dh), len(warps) if n is None else n, warps,
                                       C.byref(norm) if norm is not None else None, C.byref(opts) if opts is not None else None)
    if check:
        _check(st, "vpf_convert_warp_tensor")
    return st


def make_remap_jobs(jobs) -> "C.Array[RemapIO]":
    """jobs: list of (src_desc, dst_desc, (xmap_ptr, xmap_pitch), (ymap_ptr, ymap_pitch)) with desc as in planes(); src_desc = the planes of the WHOLE
    frame, the map pointers DEVICE addresses of float32 rows, the pitches in bytes"""
    arr = (RemapIO * len(jobs))()
    for i, (s, d, xm, ym) in enumerate(jobs):
        s, d = planes(s), planes(d)
        for k in range(3):
            arr[i].src[k].ptr, arr[i].src[k].pitch = s[k].ptr, s[k].pitch
            arr[i].dst[k].ptr, arr[i].dst[k].pitch = d[k].ptr, d[k].pitch
        arr[i].xmap, arr[i].xmap_pitch = xm[0] or None, xm[1]
        arr[i].ymap, arr[i].ymap_pitch = ym[0] or None, ym[1]
    return arr


def make_remap_opts(border_mode=WARP_CONSTANT, border=(0, 0, 0), max_step=0.0) -> RemapOpts:
    o = RemapOpts()
    o.border_mode, o.max_step = border_mode, max_step
    for k in range(3):
        o.border[k] = border[k]
    return o


def convert_remap_tensor(ex: Exec, src_fmt, cs, cr, sw, sh, dw, dh, jobs, norm: TensorNorm, opts: RemapOpts = None, n=None, check=True) -> int:
    """jobs: RemapIO array from make_remap_jobs(); every job sampled through its pair of device maps into dw x dh and normalised, 96 jobs per job
    table; the kernel reads the maps when it runs on ex.stream: no sync, no copy, capturable"""
    st = lib().vpf_convert_remap_tensor(C.byref(ex) if ex is not None else None, src_fmt, cs, cr, Size(sw, sh), Size(dw, dh),
                                        (len(jobs) if jobs is not None else 0) if n is None else n, jobs,
                                        C.byref(norm) if norm is not None else None, C.byref(opts) if opts is not None else None)
    if check:
        _check(st, "vpf_convert_remap_tensor")
    return st


def make_persps(jobs) -> "C.Array[PerspIO]":
    """jobs: list of (src_desc, dst_desc, m) with desc as in planes(); src_desc = the planes of the WHOLE frame, m = nine floats
    (m00 m01 m02 m10 m11 m12 m20 m21 m22) or a 3 x 3 nested sequence: destination pixel -> homogeneous source coordinates"""
    arr = (PerspIO * len(jobs))()
    for i, (s, d, m) in enumerate(jobs):
        s, d = planes(s), planes(d)
        for k in range(3):
            arr[i].src[k].ptr, arr[i].src[k].pitch = s[k].ptr, s[k].pitch
            arr[i].dst[k].ptr, arr[i].dst[k].pitch = d[k].ptr, d[k].pitch
        flat = [v for row in m for v in row] if len(m) == 3 else list(m)
        for k in range(9):
            arr[i].m[k] = flat[k]
    return arr


def convert_persp_tensor(ex: Exec, src_fmt, cs, cr, sw, sh, dw, dh, persps, norm: TensorNorm, opts: WarpOpts = None, n=None, check=True) -> int:
    """persps: PerspIO array from make_persps(); every job sampled through its 3 x 3 matrix into dw x dh and normalised, 82 jobs per job table"""
    st = lib().vpf_convert_persp_tensor(C.byref(ex), src_fmt, cs, cr, Size(sw, sh), Size(dw, dh), len(persps) if n is None else n, persps,
                                        C.byref(norm) if norm is not None else None, C.byref(opts) if opts is not None else None)
    if check:
        _check(st, "vpf_convert_persp_tensor")
    return st


def letterbox_fit(w, h, dw, dh):
    """vpf_letterbox_fit: the aspect-preserving, centred placement (ix, iy, iw, ih) of a w x h rectangle inside dw x dh (host only)"""
    r = lib().vpf_letterbox_fit(Size(w, h), Size(dw, dh))
    return (r.x, r.y, r.width, r.height)


def make_letterbox_jobs(jobs) -> "C.Array[LetterboxIO]":
    """jobs: list of (src_desc, dst_desc, (x, y, w, h), (ix, iy, iw, ih)) with desc as in planes(); src_desc = the planes of the WHOLE frame,
    dst_desc = the WHOLE destination planes of the job"""
    arr = (LetterboxIO * len(jobs))()
    for i, (s, d, rect, dst_rect) in enumerate(jobs):
        s, d = planes(s), planes(d)
        for k in range(3):
            arr[i].src[k].ptr, arr[i].src[k].pitch = s[k].ptr, s[k].pitch
            arr[i].dst[k].ptr, arr[i].dst[k].pitch = d[k].ptr, d[k].pitch
        arr[i].rect.x, arr[i].rect.y, arr[i].rect.width, arr[i].rect.height = rect
        arr[i].dst_rect.x, arr[i].dst_rect.y, arr[i].dst_rect.width, arr[i].dst_rect.height = dst_rect
    return arr


def make_letterbox_opts(pad=(0, 0, 0)) -> LetterboxOpts:
    o = LetterboxOpts()
    for k in range(3):
        o.pad[k] = pad[k]
    return o


def convert_letterbox_tensor(ex: Exec, src_fmt, cs, cr, sw, sh, dw, dh, jobs, norm: TensorNorm, opts: LetterboxOpts = None, n=None, check=True) -> int:
    """jobs: LetterboxIO array from make_letterbox_jobs(); every rectangle resized into its dst_rect of the dw x dh planes, the rest padded, 82
    jobs per job table"""
    st = lib().vpf_convert_letterbox_tensor(C.byref(ex), src_fmt, cs, cr, Size(sw, sh), Size(dw, dh), len(jobs) if n is None else n, jobs,
                                            C.byref(norm) if norm is not None else None, C.byref(opts) if opts is not None else None)
    if check:
        _check(st, "vpf_convert_letterbox_tensor")
    return st


def convert_letterbox_tensor_aa(ex: Exec, src_fmt, cs, cr, sw, sh, dw, dh, jobs, norm: TensorNorm, opts: LetterboxOpts = None, n=None, check=True) -> int:
    """convert_letterbox_tensor's arguments; inside its dst_rect every rectangle goes through the triangle filter whose support grows with the scale
    (PIL's BILINEAR, torch's antialias=True) instead of the bare bilinear pair"""
    st = lib().vpf_convert_letterbox_tensor_aa(C.byref(ex) if ex is not None else None, src_fmt, cs, cr, Size(sw, sh), Size(dw, dh),
                                               len(jobs) if n is None else n, jobs, C.byref(norm) if norm is not None else None,
                                               C.byref(opts) if opts is not None else None)
    if check:
        _check(st, "vpf_convert_letterbox_tensor_aa")
    return st


def make_letterbox_dev(boxes_ptr, max_n, dst, dst_job_stride, count_ptr=None, dst_rects_ptr=None, box_stride=20, rect_stride=16, reserved=0) -> LetterboxDev:
    """vpf_letterbox_dev: boxes_ptr / dst_rects_ptr / count_ptr are DEVICE addresses (dst_rects_ptr None: the kernel fits every box into the plane;
    count_ptr None: max_n jobs), dst = job 0's WHOLE planes as in planes(), dst_job_stride = bytes from one job's planes to the next's"""
    t = LetterboxDev()
    t.boxes, t.dst_rects, t.count = boxes_ptr or None, dst_rects_ptr or None, count_ptr or None
    t.box_stride, t.rect_stride, t.max_n, t.reserved, t.dst_job_stride = box_stride, rect_stride, max_n, reserved, dst_job_stride
    d = planes(dst)
    for k in range(3):
        t.dst[k].ptr, t.dst[k].pitch = d[k].ptr, d[k].pitch
    return t


def convert_letterbox_tensor_dev(ex: Exec, src_fmt, cs, cr, sw, sh, dw, dh, frames, table: LetterboxDev, norm: TensorNorm, opts: LetterboxOpts = None,
                                 n_frames=None, check=True) -> int:
    """frames: FrameSrc array from make_frame_srcs() (at most 128), table: make_letterbox_dev(), opts: make_letterbox_opts() or None; the kernel reads
    boxes, placements and count when it runs on ex.stream: no sync, no copy, capturable"""
    st = lib().vpf_convert_letterbox_tensor_dev(C.byref(ex) if ex is not None else None, src_fmt, cs, cr, Size(sw, sh), Size(dw, dh),
                                                (len(frames) if frames is not None else 0) if n_frames is None else n_frames, frames,
                                                C.byref(table) if table is not None else None, C.byref(norm) if norm is not None else None,
                                                C.byref(opts) if opts is not None else None)
    if check:
        _check(st, "vpf_convert_letterbox_tensor_dev")
    return st


def tensor_convert_supported(dst_fmt, cs, cr) -> bool:
    return bool(lib().vpf_tensor_convert_supported(dst_fmt, cs, cr))


def tensor_convert(ex: Exec, dst_fmt, cs, cr, w, h, src, dst, denorm: TensorNorm, check=True) -> int:
    """src: the three planes (ptr, pitch in bytes) of the tensor frame in input channel order; dst: the NV12 / YUV420 planes"""
    st = lib().vpf_tensor_convert(C.byref(ex), dst_fmt, cs, cr, Size(w, h), planes(src), planes(dst), C.byref(denorm))
    if check:
        _check(st, "vpf_tensor_convert")
    return st


def tensor_convert_batch(ex: Exec, dst_fmt, cs, cr, w, h, batch, denorm: TensorNorm, n=None, check=True) -> int:
    st = lib().vpf_tensor_convert_batch(C.byref(ex), dst_fmt, cs, cr, Size(w, h), len(batch) if n is None else n, batch, C.byref(denorm))
    if check:
        _check(st, "vpf_tensor_convert_batch")
    return st


def make_warps_dev(matrices_ptr, max_n, dst, dst_job_stride, frame_index_ptr=None, count_ptr=None, matrix_stride=24, frame_stride=4, max_step=0.0) -> WarpsDev:
    """vpf_warps_dev: matrices_ptr / frame_index_ptr / count_ptr are DEVICE addresses (frame_index_ptr None: every job samples frame 0; count_ptr None:
    max_n jobs), dst = job 0's planes as in planes(), dst_job_stride = bytes from one job's planes to the next's, max_step = the LDS hint (0: none)"""
    t = WarpsDev()
    t.matrices, t.frame_index, t.count = matrices_ptr or None, frame_index_ptr or None, count_ptr or None
    t.matrix_stride, t.frame_stride, t.max_n, t.max_step, t.dst_job_stride = matrix_stride, frame_stride, max_n, max_step, dst_job_stride
    d = planes(dst)
    for k in range(3):
        t.dst[k].ptr, t.dst[k].pitch = d[k].ptr, d[k].pitch
    return t


def convert_warp_tensor_dev(ex: Exec, src_fmt, cs, cr, sw, sh, dw, dh, frames, table: WarpsDev, norm: TensorNorm, opts=None, n_frames=None, check=True) -> int:
    """frames: FrameSrc array from make_frame_srcs() (at most 128), table: make_warps_dev(), opts: make_warp_opts() or None; the kernel reads matrices,
    frame indices and count when it runs on ex.stream: no sync, no copy, capturable"""
    st = lib().vpf_convert_warp_tensor_dev(C.byref(ex) if ex is not None else None, src_fmt, cs, cr, Size(sw, sh), Size(dw, dh),
                                           (len(frames) if frames is not None else 0) if n_frames is None else n_frames, frames,
                                           C.byref(table) if table is not None else None, C.byref(norm) if norm is not None else None,
                                           C.byref(opts) if opts is not None else None)
    if check:
        _check(st, "vpf_convert_warp_tensor_dev")
    return st


def make_persps_dev(matrices_ptr, max_n, dst, dst_job_stride, frame_index_ptr=None, count_ptr=None, matrix_stride=36, frame_stride=4, max_step=0.0) -> PerspsDev:
    """vpf_persps_dev: make_warps_dev() for nine floats per job (matrix_stride from 36 up); max_step = the LDS hint (persp_max_step(); 0: none)"""
    t = PerspsDev()
    t.matrices, t.frame_index, t.count = matrices_ptr or None, frame_index_ptr or None, count_ptr or None
    t.matrix_stride, t.frame_stride, t.max_n, t.max_step, t.dst_job_stride = matrix_stride, frame_stride, max_n, max_step, dst_job_stride
    d = planes(dst)
    for k in range(3):
        t.dst[k].ptr, t.dst[k].pitch = d[k].ptr, d[k].pitch
    return t


def convert_persp_tensor_dev(ex: Exec, src_fmt, cs, cr, sw, sh, dw, dh, frames, table: PerspsDev, norm: TensorNorm, opts=None, n_frames=None, check=True) -> int:
    """frames: FrameSrc array from make_frame_srcs() (at most 128), table: make_persps_dev(), opts: make_warp_opts() or None; the kernel reads matrices,
    frame indices and count when it runs on ex.stream: no sync, no copy, capturable"""
    st = lib().vpf_convert_persp_tensor_dev(C.byref(ex) if ex is not None else None, src_fmt, cs, cr, Size(sw, sh), Size(dw, dh),
                                            (len(frames) if frames is not None else 0) if n_frames is None else n_frames, frames,
                                            C.byref(table) if table is not None else None, C.byref(norm) if norm is not None else None,
                                            C.byref(opts) if opts is not None else None)
    if check:
        _check(st, "vpf_convert_persp_tensor_dev")
    return st


def persp_max_step(m, dw, dh) -> float:
    """vpf_persp_max_step: the LDS hint of ONE inverse 3 x 3 matrix (nine floats) for a dw x dh destination, 0.0 where it has no bound"""
    return float(lib().vpf_persp_max_step((C.c_float * 9)(*[float(v) for v in m]), Size(dw, dh)))
