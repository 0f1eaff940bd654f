"""PytorchNvCodec — pitched device memory <-> torch.Tensor on torch-ROCm.

Function surface of the reference's src/PytorchNvCodec/src/PytorchNvCodec.cpp:141-258:
  makefromDevicePtrUint8 / DptrToTensor (ptr, width, height, pitch, elem_size[, stream]) -> torch.uint8 [height, width]
  TensorToDptr (tensor, ptr, width, height, pitch, elem_size[, stream])
The reference allocates a tensor and cudaMemcpy2D's into it (:36-87) — a copy.  Here the pitched plane is first
exposed to torch as a ZERO-COPY strided view (through __cuda_array_interface__, strides = (pitch, 1)), and the
reference-named functions are that view plus one strided D2D copy on the requested stream; `view_plane` /
`view_surface_planar` hand out the zero-copy view itself (config 5 of BASELINE.json), removing 2 x 3 B/px of traffic.

torch is plumbing here (allocation, streams); no pixel arithmetic happens in this module.
"""
from __future__ import annotations

import operator
import sys
from typing import TYPE_CHECKING, overload

import torch


class _DevMem:
    """Minimal __cuda_array_interface__ carrier for a pitched uint8 region that someone else owns."""

    def __init__(self, ptr: int, height: int, width: int, pitch: int, owner=None):
        self.owner = owner  # keeps the Surface alive while torch holds the view
        self.__cuda_array_interface__ = {
            "shape": (height, width), "typestr": "|u1", "data": (int(ptr), False), "strides": (int(pitch), 1), "version": 2,
        }


def _check(ptr, elem_size, fn):
    if elem_size != 1:
        raise RuntimeError(f"{fn}: only torch.uint8 data type is supported")  # PytorchNvCodec.cpp:40-45
    if not ptr:
        raise RuntimeError(f"{fn}: Video frame has void device ptr.")


def view_plane(ptr: int, width: int, height: int, pitch: int, owner=None, device=None) -> torch.Tensor:
    """Zero-copy torch.uint8 view [height, width] with strides (pitch, 1) of pitched device memory."""
    _check(ptr, 1, "view_plane")
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    return torch.as_tensor(_DevMem(ptr, height, width, pitch, owner), device=dev)


def view_surface_planar(surface, gpu_id: int | None = None) -> torch.Tensor:
    """Zero-copy [3, H, W] uint8 view of an RGB_PLANAR / YUV444 Surface (one W x 3H allocation, plane i at
    base + i*H*pitch — reference layout MemoryInterfaces.cpp:1593-1600)."""
    p = surface.PlanePtr()
    h3, w, pitch = p.Height(), p.Width(), p.Pitch()
    flat = view_plane(p.GpuMem(), w, h3, pitch, owner=surface, device=None if gpu_id is None else f"cuda:{gpu_id}")
    return flat.view(3, h3 // 3, w) if pitch == w else flat.as_strided((3, h3 // 3, w), ((h3 // 3) * pitch, pitch, 1))


def _on_stream(stream: int):
    if not stream:
        return torch.cuda.stream(torch.cuda.current_stream())
    return torch.cuda.stream(torch.cuda.ExternalStream(int(stream)))


def DptrToTensor(ptr: int, width: int, height: int, pitch: int, elem_size: int, stream: int = 0) -> torch.Tensor:
    """New contiguous torch.uint8 tensor [height, width] holding a copy of the pitched plane."""
    _check(ptr, elem_size, "makefromDevicePtrUint8")
    if not stream:
        # The plane was usually written a moment ago by a converter on ITS stream (the per-GPU stream of the gpu_id
        # constructors is non-blocking, like the reference's: PyNvCodec.cpp:107).  The reference's stream-less overload is a
        # blocking cudaMemcpy2D that nothing orders after that stream; here the device is drained first, so the copy can
        # never read a half-written surface.  Pass `stream` (the converter's) to stay asynchronous.
        torch.cuda.synchronize()
    with _on_stream(stream):
        out = view_plane(ptr, width, height, pitch).contiguous().clone() if pitch == width else view_plane(ptr, width, height, pitch).contiguous()
    if not stream:
        torch.cuda.current_stream().synchronize()  # the reference's stream-less overload is cudaMemcpy2D (blocking)
    return out


makefromDevicePtrUint8 = DptrToTensor


def TensorToDptr(tensor: torch.Tensor, ptr: int, width: int, height: int, pitch: int, elem_size: int, stream: int = 0) -> None:
    """Copy a torch.uint8 tensor of width*height elements into pitched device memory."""
    _check(ptr, elem_size, "copytoDevicePtrUint8")
    if tensor.dtype != torch.uint8 or not tensor.is_cuda:
        raise RuntimeError("copytoDevicePtrUint8: need a CUDA/HIP torch.uint8 tensor")
    if tensor.numel() != width * height:
        raise RuntimeError("copytoDevicePtrUint8: tensor has the wrong number of elements")
    if not stream:
        torch.cuda.synchronize()  # earlier readers / writers of the destination surface on other streams (see DptrToTensor)
    with _on_stream(stream):
        view_plane(ptr, width, height, pitch, device=tensor.device).copy_(tensor.reshape(height, width))
    if not stream:
        torch.cuda.current_stream().synchronize()


def surface_from_tensor(tensor: torch.Tensor, fmt=None):
    """Wrap a contiguous CUDA/HIP uint8 tensor as a non-owning PyNvCodec.Surface — the converter then writes straight into
    the tensor (`PySurfaceConverter.ExecuteBatch([src], [surface_from_tensor(t)])`), no copy at all.
      [3, H, W] -> RGB_PLANAR (default) or YUV444;   [H, W, 3] -> RGB (default) or BGR;   [H, W] -> Y
    The tensor is kept alive by the returned Surface.  Stream ordering is the caller's, exactly as with the reference:
    kernels that produced / will consume the tensor on torch's stream are not ordered against a converter running on its
    own stream — build the converter on `torch.cuda.current_stream().cuda_stream` or synchronise in between."""
    try:
        import PyNvCodec as nvc
    except ImportError:  # package-relative import when used as videoprocessingframework_amd.PytorchNvCodec
        from .. import PyNvCodec as nvc
    if tensor.dtype != torch.uint8 or not tensor.is_cuda or not tensor.is_contiguous():
        raise RuntimeError("surface_from_tensor: need a contiguous CUDA/HIP torch.uint8 tensor")
    PF = nvc.PixelFormat
    if tensor.dim() == 3 and tensor.shape[0] == 3:
        f, (h, w), pitch = (fmt or PF.RGB_PLANAR), tensor.shape[1:], tensor.shape[2]
    elif tensor.dim() == 3 and tensor.shape[2] == 3:
        f, (h, w), pitch = (fmt or PF.RGB), tensor.shape[:2], 3 * tensor.shape[1]
    elif tensor.dim() == 2:
        f, (h, w), pitch = (fmt or PF.Y), tensor.shape, tensor.shape[1]
    else:
        raise RuntimeError("surface_from_tensor: expected [3,H,W], [H,W,3] or [H,W]")
    s = nvc.Surface.Wrap(f, int(w), int(h), int(pitch), tensor.data_ptr())
    s._owner = tensor
    return s


_TENSOR_DTYPES = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}  # vpf_tensor_dtype

if TYPE_CHECKING:  # the two call forms of the four tensor functions: the planar one, unchanged, and the one that names the memory layout
    @overload
    def to_normalized_tensor(resizer, surfaces, mean, std, dtype=torch.float32, bgr=False, out=None, cc_ctx=None) -> torch.Tensor: ...
    @overload
    def to_normalized_tensor(resizer, surfaces, mean, std, dtype=torch.float32, bgr=False, out=None, cc_ctx=None, *, channels_last: bool) -> torch.Tensor: ...
    @overload
    def rois_to_normalized_tensor(resizer, surfaces, rois, mean, std, dtype=torch.float32, bgr=False, out=None, cc_ctx=None) -> torch.Tensor: ...
    @overload
    def rois_to_normalized_tensor(resizer, surfaces, rois, mean, std, dtype=torch.float32, bgr=False, out=None, cc_ctx=None, *, channels_last: bool) -> torch.Tensor: ...
    @overload
    def warps_to_normalized_tensor(resizer, surfaces, surface_index, matrices, mean, std, dtype=torch.float32, bgr=False, border=(0, 0, 0), border_mode="constant", out=None, cc_ctx=None) -> torch.Tensor: ...
    @overload
    def warps_to_normalized_tensor(resizer, surfaces, surface_index, matrices, mean, std, dtype=torch.float32, bgr=False, border=(0, 0, 0), border_mode="constant", out=None, cc_ctx=None, *, channels_last: bool) -> torch.Tensor: ...
    @overload
    def persps_to_normalized_tensor(resizer, surfaces, surface_index, matrices, mean, std, dtype=torch.float32, bgr=False, border=(0, 0, 0), border_mode="constant", out=None, cc_ctx=None) -> torch.Tensor: ...
    @overload
    def persps_to_normalized_tensor(resizer, surfaces, surface_index, matrices, mean, std, dtype=torch.float32, bgr=False, border=(0, 0, 0), border_mode="constant", out=None, cc_ctx=None, *, channels_last: bool) -> torch.Tensor: ...
    @overload
    def from_normalized_tensor(converter, tensor, mean, std, bgr=False, cc_ctx=None, out=None) -> list: ...
    @overload
    def from_normalized_tensor(converter, tensor, mean, std, bgr=False, cc_ctx=None, out=None, *, channels_last: bool) -> list: ...


def _channels_last_strides(fn, t, what):
    """(frame, row) strides in elements of a logical [N, 3, H, W] tensor in torch.channels_last memory: strides (s0, 1, s2, 3) with s2 >= 3 W and
    s0 >= H s2 (a slice of a larger batch and padded rows qualify); ValueError naming the strides otherwise.  Dimensions of one element are
    never walked: their strides are not looked at."""
    n, _, h, w = t.shape
    s0, s1, s2, s3 = t.stride()
    if s1 != 1 or (w > 1 and s3 != 3) or (h > 1 and s2 < 3 * w) or (n > 1 and s0 < h * (s2 if h > 1 else 3 * w)):
        raise ValueError(f"{fn}: channels_last=True needs {what} in torch.channels_last memory format: strides (s0, 1, s2, 3) with s2 >= {3 * w} and "
                         f"s0 >= {h} * s2, got strides {tuple(t.stride())}")
    return (s0 if n > 1 else 0), (s2 if h > 1 else 0)


def _tensor_out(fn, out, n, h, w, dtype, channels_last, device=None):
    """the destination of a *_to_normalized_tensor call and its (frame, plane, row) strides in elements: the checked `out`, or a new [n, 3, h, w] tensor
    on `device` (None: torch's current device), in torch.channels_last memory format when channels_last says so (the plane stride is 0 then)"""
    given = out is not None
    if not given:
        device = torch.device("cuda", torch.cuda.current_device()) if device is None else device
        out = torch.empty((n, 3, h, w), dtype=dtype, device=device, memory_format=torch.channels_last if channels_last else torch.contiguous_format)
    elif out.dtype != dtype or not out.is_cuda or tuple(out.shape) != (n, 3, h, w):
        raise ValueError(f"{fn}: out must be a {dtype} device tensor of shape {(n, 3, h, w)}, got {out.dtype} {tuple(out.shape)} on {out.device}")
    s0, s1, s2, s3 = out.stride()
    if channels_last:
        (s0, s2), s1 = _channels_last_strides(fn, out, "out"), 0
    elif given and (s3 != 1 or s2 < w or (h > 1 and s1 < h * s2) or (n > 1 and s0 < 3 * s1) or min(s0, s1, s2) <= 0):
        raise ValueError(f"{fn}: out needs unit stride along W and non-overlapping rows, planes and frames, got strides {out.stride()}")
    return out, s0, s1, s2


class _on_task_stream:
    """Context manager: under torch.cuda.device(device) the body runs between two waits.  The stream of `task` (a resizer / converter) waits for
    torch's current stream — the allocation, the producers and the earlier users of the tensors come first —, and torch's current stream then waits
    for what the body put on the task's (not after an exception).  `as` gives the task's stream, or None when it IS torch's current stream and there
    is nothing to order.  (A class, not a contextlib generator: that costs a microsecond per call, 5 % of a device-table call.)"""
    __slots__ = ("task", "guard", "cur", "side")

    def __init__(self, task, device):
        self.task, self.guard = task, torch.cuda.device(device)

    def __enter__(self):
        self.guard.__enter__()
        try:
            self.cur = torch.cuda.current_stream()
            ts = int(self.task.Stream())
            self.side = torch.cuda.ExternalStream(ts) if ts != self.cur.cuda_stream else None
            if self.side is not None:
                self.side.wait_stream(self.cur)
        except BaseException:
            self.guard.__exit__(*sys.exc_info())  # never leave the caller on another device
            raise
        return self.side

    def __exit__(self, exc_type, exc, tb):
        try:
            if exc_type is None and self.side is not None:
                self.cur.wait_stream(self.side)
        finally:
            self.guard.__exit__(exc_type, exc, tb)
        return False


_RESIZER_REFUSED = "the surfaces do not match the resizer (format / size) or the colour context was refused"
_CONVERTER_REFUSED = "the surfaces do not match the converter (format / size), the tensor layout was refused or the colour context was refused"


def _refused(fn, why):
    raise RuntimeError(f"{fn}: {why}")


def to_normalized_tensor(resizer, surfaces, mean, std, dtype=torch.float32, bgr=False, out=None, cc_ctx=None, channels_last=False) -> torch.Tensor:
    """NV12 / YUV420 (or P10 / P12) surfaces -> the normalised float tensor [N, 3, H, W] a DNN consumes, in one pass of the fused kernels
    (PySurfaceConvertResizer.ExecuteToTensor): the RGB_PLANAR bytes of resizer.ExecuteBatch, divided by 255 and normalised with
    torchvision's mean / std (one fp32 fma per element, scale = 1 / (255 std), bias = -mean / std), rounded to `dtype` (float32, float16,
    bfloat16).  mean / std are per output channel (B G R order when bgr=True).

    `out`: a tensor to write into (dtype, device and shape must match, the last dimension contiguous; row, plane and frame strides are
    free: a slice of a larger batch or padded rows work), else a new one on torch's current device.  The kernel runs on the resizer's
    stream after torch's current stream has reached this call, and torch's current stream waits for it: the result can be used on the
    current stream right away, no host synchronisation.  The surfaces themselves are ordered as for every Execute (the caller's business).

    channels_last=True (here, in rois_to_normalized_tensor and in warps_to_normalized_tensor): the same values, written by the kernels straight
    into torch.channels_last memory (NHWC) — the returned tensor still has the logical shape [N, 3, H, W], and
    is_contiguous(memory_format=torch.channels_last) holds for a new one.  `out` then needs strides (s0, 1, s2, 3) with s2 >= 3 W and
    s0 >= H s2 (a slice of a channels-last batch and padded rows qualify), else ValueError.  The layout is what this argument says, never
    inferred from the strides of `out`."""
    if dtype not in _TENSOR_DTYPES:
        raise ValueError(f"to_normalized_tensor: dtype must be one of {list(_TENSOR_DTYPES)}")
    surfaces = list(surfaces)
    n = len(surfaces)
    w, h = resizer.DstSize()
    out, s0, s1, s2 = _tensor_out("to_normalized_tensor", out, n, h, w, dtype, channels_last)
    if n == 0:
        return out
    elem = out.element_size()
    with _on_task_stream(resizer, out.device):
        ok = resizer.ExecuteToTensor(surfaces, out.data_ptr(), _TENSOR_DTYPES[dtype], [float(m) for m in mean], [float(v) for v in std], cc_ctx,
                                     bool(bgr), s2 * elem, s1 * elem, s0 * elem, bool(channels_last))
    if not ok:
        _refused("to_normalized_tensor", _RESIZER_REFUSED)
    return out


def _rois_list(rois, surfaces, fn):
    """rois -> list of 5-tuples of Python ints, validated against the surfaces: ValueError for a device tensor, a non-integer dtype, a shape other
    than [K, 5], a surface index out of range, an empty rectangle or one that leaves its surface"""
    if isinstance(rois, torch.Tensor):
        if rois.device.type != "cpu":
            raise ValueError(f"{fn}: rois must live on the host (the job table is built on the CPU): pass rois.cpu()")
        if rois.dtype.is_floating_point or rois.dtype.is_complex or rois.dtype == torch.bool:
            raise ValueError(f"{fn}: rois must hold integers, got {rois.dtype}")
        if rois.dim() != 2 or rois.shape[1] != 5:
            raise ValueError(f"{fn}: a rois tensor must have shape [K, 5], got {tuple(rois.shape)}")
        rois = rois.tolist()
    elif hasattr(rois, "dtype") and hasattr(rois, "tolist"):  # numpy.ndarray
        if getattr(rois.dtype, "kind", "") not in "iu":
            raise ValueError(f"{fn}: rois must hold integers, got {rois.dtype}")
        if rois.ndim != 2 or rois.shape[1] != 5:
            raise ValueError(f"{fn}: a rois array must have shape [K, 5], got {tuple(rois.shape)}")
        rois = rois.tolist()
    out = []
    for i, r in enumerate(rois):
        r = tuple(r)
        if len(r) != 5:
            raise ValueError(f"{fn}: rois[{i}] must be (surface_index, x, y, w, h), got {r}")
        try:
            k, x, y, w, h = (operator.index(v) for v in r)  # Python and numpy integers; a float is refused, never truncated
        except TypeError:
            raise ValueError(f"{fn}: rois[{i}] must hold integers, got {r}") from None
        if not 0 <= k < len(surfaces):
            raise ValueError(f"{fn}: rois[{i}] names surface {k}, there are {len(surfaces)}")
        sw, sh = surfaces[k].Width(), surfaces[k].Height()
        if x < 0 or y < 0 or w < 1 or h < 1 or x + w > sw or y + h > sh:
            raise ValueError(f"{fn}: rois[{i}] = (x {x}, y {y}, w {w}, h {h}) is empty or leaves its {sw} x {sh} surface (nothing is clipped silently)")
        out.append((k, x, y, w, h))
    return out


def rois_to_normalized_tensor(resizer, surfaces, rois, mean, std, dtype=torch.float32, bgr=False, out=None, cc_ctx=None, channels_last=False) -> torch.Tensor:
    """K rectangles of NV12 / YUV420 (or P10 / P12) surfaces -> the normalised float tensor [K, 3, dh, dw] a second-stage network (classifier, ReID, face net
    behind a detector) consumes, in one dispatch per 96 regions (PySurfaceConvertResizer.ExecuteRoisToTensor, vpf_convert_resize_tensor_rois).
    `rois`: a sequence of (surface_index, x, y, w, h) integer 5-tuples, or a CPU integer tensor / ndarray [K, 5]; x, y, w, h in luma pixels of
    surfaces[surface_index], any integer offset (odd ones too), the rectangle inside the surface.  Every region is resized (bilinear, taps
    clamped at the RECTANGLE's edges) to the resizer's destination size and normalised exactly as to_normalized_tensor does; a rectangle that
    is the whole surface gives to_normalized_tensor's bits.

    `out`, channels_last, the returned tensor and the stream ordering: exactly as to_normalized_tensor.  ValueError for rois on the device (pass .cpu()), a
    non-integer dtype, a bad surface index or a rectangle that is empty or leaves its surface.  K == 0 returns an empty tensor without a launch."""
    fn = "rois_to_normalized_tensor"
    if dtype not in _TENSOR_DTYPES:
        raise ValueError(f"{fn}: dtype must be one of {list(_TENSOR_DTYPES)}")
    surfaces = list(surfaces)
    jobs = _rois_list(rois, surfaces, fn)
    n = len(jobs)
    w, h = resizer.DstSize()
    out, s0, s1, s2 = _tensor_out(fn, out, n, h, w, dtype, channels_last)
    if n == 0:
        return out
    elem = out.element_size()
    with _on_task_stream(resizer, out.device):
        ok = resizer.ExecuteRoisToTensor(surfaces, jobs, out.data_ptr(), _TENSOR_DTYPES[dtype], [float(m) for m in mean], [float(v) for v in std], cc_ctx,
                                         bool(bgr), s2 * elem, s1 * elem, s0 * elem, bool(channels_last))
    if not ok:
        _refused(fn, _RESIZER_REFUSED)
    return out


def boxes_to_rois(boxes_xyxy, frame_index, width, height) -> torch.Tensor:
    """A detector's float boxes [K, 4] (x1, y1, x2, y2, in pixels of a width x height frame) and integer frame indices [K] -> the int32 [K, 5] table
    (frame, x, y, w, h) device_rois_to_normalized_tensor takes.  Pure torch, on whatever device the boxes live on: no sync.  The rectangle is the
    box rounded OUTWARDS and clipped to the frame: x = clamp(floor(x1), 0, W - 1), w = clamp(ceil(x2), x + 1, W) - x, y and h likewise — always at
    least one pixel, always inside the frame.  A box with a NaN coordinate gets w = h = 0: an invalid box, whose output frame is normalised zeros."""
    b = torch.as_tensor(boxes_xyxy)
    if b.dim() != 2 or b.shape[1] != 4 or not b.dtype.is_floating_point:
        raise ValueError(f"boxes_to_rois: boxes_xyxy must be a float tensor of shape [K, 4], got {b.dtype} {tuple(b.shape)}")
    f = torch.as_tensor(frame_index, device=b.device)
    if f.dim() != 1 or f.shape[0] != b.shape[0] or f.dtype.is_floating_point or f.dtype.is_complex or f.dtype == torch.bool:
        raise ValueError(f"boxes_to_rois: frame_index must be an integer tensor of shape [{b.shape[0]}], got {f.dtype} {tuple(f.shape)}")
    W, H = int(width), int(height)
    if W < 1 or H < 1:
        raise ValueError("boxes_to_rois: width and height must be at least 1")
    b = b.to(torch.float64)  # exact for every float dtype; the clamps come before the conversion to integers
    bad = torch.isnan(b).any(dim=1)
    b = torch.nan_to_num(b, nan=0.0)
    x = b[:, 0].floor().clamp(0, W - 1).to(torch.int64)
    y = b[:, 1].floor().clamp(0, H - 1).to(torch.int64)
    x2 = torch.minimum(torch.maximum(b[:, 2].ceil().clamp(0, W).to(torch.int64), x + 1), torch.full_like(x, W))
    y2 = torch.minimum(torch.maximum(b[:, 3].ceil().clamp(0, H).to(torch.int64), y + 1), torch.full_like(y, H))
    w = torch.where(bad, torch.zeros_like(x), x2 - x)
    h = torch.where(bad, torch.zeros_like(y), y2 - y)
    return torch.stack([f.to(torch.int64), x, y, w, h], dim=1).to(torch.int32)


def device_rois_to_normalized_tensor(resizer, surfaces, boxes, mean, std, count=None, dtype=torch.float32, bgr=False, out=None, cc_ctx=None,
                                     channels_last=False) -> torch.Tensor:
    """rois_to_normalized_tensor for boxes that never leave the GPU (PySurfaceConvertResizer.ExecuteRoisDevToTensor, vpf_convert_resize_tensor_rois_dev):
    no synchronisation, no copy of the boxes to the host, one dispatch, and the call can be captured in a graph that replays with the boxes and the
    count of replay time.
    `boxes`: a device torch.int32 tensor [K, 5] of (surface_index, x, y, w, h) rows (last stride 1, row stride >= 5: a slice of a wider table works),
    e.g. boxes_to_rois(...) of a detector's output; `count`: a device torch.int32 tensor of ONE element (how many rows are valid: NMS's count), or
    None for all K.  At most 128 surfaces, K at most 65535.  Returns [K, 3, dh, dw]:
      rows below the count with a valid box    the bits rois_to_normalized_tensor gives for that rectangle;
      rows below the count with an invalid box (empty, negative, leaving its surface, no such surface)   normalised zeros, round(-mean / std): nothing is
                                               clipped and no surface is read;
      rows at or behind the count              NOT WRITTEN: undefined in a fresh tensor (torch.empty), unchanged in `out`.
    The kernel reads boxes and count when it runs; this function orders it behind torch's current stream, where their producer ran.  `out`,
    channels_last, dtype, bgr, the returned tensor and the stream ordering: as rois_to_normalized_tensor.  ValueError for boxes or count on the host or on
    another device than `out`, another dtype or shape."""
    fn = "device_rois_to_normalized_tensor"
    if dtype not in _TENSOR_DTYPES:
        raise ValueError(f"{fn}: dtype must be one of {list(_TENSOR_DTYPES)}")
    surfaces = list(surfaces)
    if not 1 <= len(surfaces) <= 128:
        raise ValueError(f"{fn}: 1 .. 128 surfaces per call, got {len(surfaces)}")
    if not isinstance(boxes, torch.Tensor) or not boxes.is_cuda:
        raise ValueError(f"{fn}: boxes must be a device tensor (for host boxes there is rois_to_normalized_tensor)")
    if boxes.dtype != torch.int32 or boxes.dim() != 2 or boxes.shape[1] != 5:
        raise ValueError(f"{fn}: boxes must be torch.int32 of shape [K, 5], got {boxes.dtype} {tuple(boxes.shape)}")
    n = boxes.shape[0]
    if n > 65535:
        raise ValueError(f"{fn}: at most 65535 boxes per call, got {n}")
    if boxes.stride(1) != 1 or (n > 1 and boxes.stride(0) < 5):
        raise ValueError(f"{fn}: boxes needs unit stride along its rows and a row stride of at least 5, got strides {boxes.stride()}")
    if count is not None:
        if not isinstance(count, torch.Tensor) or not count.is_cuda or count.dtype != torch.int32 or count.numel() != 1:
            raise ValueError(f"{fn}: count must be a device torch.int32 tensor of one element, or None")
        if count.device != boxes.device:
            raise ValueError(f"{fn}: count lives on {count.device}, boxes on {boxes.device}")
    w, h = resizer.DstSize()
    if out is not None and isinstance(out, torch.Tensor) and out.is_cuda and out.device != boxes.device:
        raise ValueError(f"{fn}: out lives on {out.device}, boxes on {boxes.device}")
    out, s0, s1, s2 = _tensor_out(fn, out, n, h, w, dtype, channels_last, boxes.device)
    if n == 0:
        return out
    elem = out.element_size()
    with _on_task_stream(resizer, out.device):
        ok = resizer.ExecuteRoisDevToTensor(surfaces, boxes.data_ptr(), n, count.data_ptr() if count is not None else 0, out.data_ptr(), _TENSOR_DTYPES[dtype],
                                            [float(m) for m in mean], [float(v) for v in std], cc_ctx, bool(bgr), s2 * elem, s1 * elem,
                                            (s0 if n > 1 else 0) * elem, bool(channels_last), 4 * (boxes.stride(0) if n > 1 else 5))
    if not ok:
        _refused(fn, _RESIZER_REFUSED)
    return out


_WARP_MODES = {"constant": 0, "replicate": 1}


def _matrices_list(matrices, fn, rows=2):
    """matrices -> list of six-float lists (rounded to float32 once): ValueError for a device tensor, a non-float dtype, a shape other than
    [K, 2, 3], a coefficient that is not finite or exceeds 2^24 in magnitude.  rows = 3: nine-float lists from [K, 3, 3] or [K, 9]"""
    import numpy as np

    if isinstance(matrices, torch.Tensor):
        if matrices.device.type != "cpu":
            raise ValueError(f"{fn}: matrices must live on the host (the job table is built on the CPU): pass matrices.cpu()")
        if not matrices.dtype.is_floating_point:
            raise ValueError(f"{fn}: matrices must hold floats, got {matrices.dtype}")
        arr = matrices.detach().to(torch.float64).numpy()
    else:
        arr = np.asarray(matrices)
        if arr.size and arr.dtype.kind != "f" and not (arr.dtype.kind in "iu" and not hasattr(matrices, "dtype")):
            raise ValueError(f"{fn}: matrices must hold floats, got {arr.dtype}")
    if arr.size == 0 and arr.ndim <= 1:
        arr = arr.reshape(0, rows, 3)
    if rows == 3 and arr.ndim == 2 and arr.shape[1] == 9:
        arr = arr.reshape(-1, 3, 3)
    if arr.ndim != 3 or tuple(arr.shape[1:]) != (rows, 3):
        raise ValueError(f"{fn}: matrices must have shape [K, {rows}, 3]{' or [K, 9]' if rows == 3 else ''}, got {tuple(arr.shape)}")
    with np.errstate(over="ignore", invalid="ignore"):
        arr = arr.astype(np.float32)
    if not bool((np.abs(arr) <= np.float32(2.0 ** 24)).all()):
        raise ValueError(f"{fn}: every matrix coefficient must be finite and at most 2^24 in magnitude")
    return [[float(v) for v in m.reshape(3 * rows)] for m in arr]


def warps_to_normalized_tensor(resizer, surfaces, surface_index, matrices, mean, std, dtype=torch.float32, bgr=False, border=(0, 0, 0), border_mode="constant", out=None, cc_ctx=None, channels_last=False) -> torch.Tensor:
    """K affine warps of NV12 / YUV420 (or P10 / P12) surfaces -> the normalised float tensor [K, 3, dh, dw] a network behind a detector consumes (aligned faces,
    rotated text boxes, oriented detections), in one dispatch per 96 regions (PySurfaceConvertResizer.ExecuteWarpsToTensor, vpf_convert_warp_tensor).
    `matrices`: a host [K, 2, 3] float tensor, ndarray or nested sequence (float64 is rounded to float32 once); matrices[i] is the INVERSE map of
    job i: it takes a destination pixel (dx, dy) to source coordinates in luma pixels of surfaces[surface_index[i]], the convention of remap's
    maps.  Pixels that fall outside the surface take `border` (per output channel, 0..255) under border_mode "constant" and the nearest edge
    pixel under "replicate".  Normalisation, `out`, channels_last, the returned tensor and the stream ordering: exactly as to_normalized_tensor.

    ValueError for matrices on the device (pass .cpu()), a wrong shape, a non-float dtype, a coefficient that is not finite or exceeds 2^24, a
    bad surface index, a border value outside 0..255, an unknown mode.  K == 0 returns an empty tensor without a launch."""
    fn = "warps_to_normalized_tensor"
    if dtype not in _TENSOR_DTYPES:
        raise ValueError(f"{fn}: dtype must be one of {list(_TENSOR_DTYPES)}")
    if border_mode not in _WARP_MODES:
        raise ValueError(f"{fn}: border_mode must be one of {list(_WARP_MODES)}, got {border_mode!r}")
    try:
        border = [operator.index(v) for v in border]
    except TypeError:
        raise ValueError(f"{fn}: border must hold three integers, got {border!r}") from None
    if len(border) != 3 or any(not 0 <= v <= 255 for v in border):
        raise ValueError(f"{fn}: border must hold three values in 0..255, got {border}")
    surfaces = list(surfaces)
    jobs = _matrices_list(matrices, fn)
    if isinstance(surface_index, torch.Tensor):
        if surface_index.device.type != "cpu":
            raise ValueError(f"{fn}: surface_index must live on the host: pass surface_index.cpu()")
        surface_index = surface_index.tolist()
    try:
        index = [operator.index(v) for v in surface_index]
    except TypeError:
        raise ValueError(f"{fn}: surface_index must hold integers") from None
    if len(index) != len(jobs):
        raise ValueError(f"{fn}: {len(index)} surface indices for {len(jobs)} matrices")
    for i, k in enumerate(index):
        if not 0 <= k < len(surfaces):
            raise ValueError(f"{fn}: surface_index[{i}] names surface {k}, there are {len(surfaces)}")
    n = len(jobs)
    w, h = resizer.DstSize()
    out, s0, s1, s2 = _tensor_out(fn, out, n, h, w, dtype, channels_last)
    if n == 0:
        return out
    elem = out.element_size()
    with _on_task_stream(resizer, out.device):
        ok = resizer.ExecuteWarpsToTensor(surfaces, index, jobs, out.data_ptr(), _TENSOR_DTYPES[dtype], [float(m) for m in mean], [float(v) for v in std],
                                          cc_ctx, bool(bgr), border, _WARP_MODES[border_mode], s2 * elem, s1 * elem, s0 * elem, bool(channels_last))
    if not ok:
        _refused(fn, _RESIZER_REFUSED)
    return out


def persps_to_normalized_tensor(resizer, surfaces, surface_index, matrices, mean, std, dtype=torch.float32, bgr=False, border=(0, 0, 0), border_mode="constant", out=None, cc_ctx=None, channels_last=False) -> torch.Tensor:
    """K perspective warps (3 x 3 homographies) of NV12 / YUV420 (or P10 / P12) surfaces -> the normalised float tensor [K, 3, dh, dw]: documents, plates,
    signs and screens seen at an angle, bird's-eye views, ground-plane registration, in one dispatch per 82 regions
    (PySurfaceConvertResizer.ExecutePerspsToTensor, vpf_convert_persp_tensor).
    `matrices`: a host [K, 3, 3] or [K, 9] float tensor, ndarray or nested sequence (float64 is rounded to float32 once), e.g. quads_to_homographies(...);
    matrices[i] is the INVERSE map of job i: destination pixel (dx, dy) -> (nx, ny, w), source coordinates (nx / w, ny / w) in luma pixels of
    surfaces[surface_index[i]].  A pixel with w <= 0 (behind the plane, on the horizon) takes `border` under BOTH border modes; everything else —
    border, border_mode, normalisation, `out`, channels_last, the returned tensor and the stream ordering — exactly as warps_to_normalized_tensor, whose
    bits this function gives for matrices with the last row (0, 0, 1).

    ValueError for matrices on the device (pass .cpu()), a wrong shape, a non-float dtype, a coefficient that is not finite or exceeds 2^24, a
    bad surface index, a border value outside 0..255, an unknown mode.  K == 0 returns an empty tensor without a launch."""
    fn = "persps_to_normalized_tensor"
    if dtype not in _TENSOR_DTYPES:
        raise ValueError(f"{fn}: dtype must be one of {list(_TENSOR_DTYPES)}")
    if border_mode not in _WARP_MODES:
        raise ValueError(f"{fn}: border_mode must be one of {list(_WARP_MODES)}, got {border_mode!r}")
    try:
        border = [operator.index(v) for v in border]
    except TypeError:
        raise ValueError(f"{fn}: border must hold three integers, got {border!r}") from None
    if len(border) != 3 or any(not 0 <= v <= 255 for v in border):
        raise ValueError(f"{fn}: border must hold three values in 0..255, got {border}")
    surfaces = list(surfaces)
    jobs = _matrices_list(matrices, fn, rows=3)
    if isinstance(surface_index, torch.Tensor):
        if surface_index.device.type != "cpu":
            raise ValueError(f"{fn}: surface_index must live on the host: pass surface_index.cpu()")
        surface_index = surface_index.tolist()
    try:
        index = [operator.index(v) for v in surface_index]
    except TypeError:
        raise ValueError(f"{fn}: surface_index must hold integers") from None
    if len(index) != len(jobs):
        raise ValueError(f"{fn}: {len(index)} surface indices for {len(jobs)} matrices")
    for i, k in enumerate(index):
        if not 0 <= k < len(surfaces):
            raise ValueError(f"{fn}: surface_index[{i}] names surface {k}, there are {len(surfaces)}")
    n = len(jobs)
    w, h = resizer.DstSize()
    out, s0, s1, s2 = _tensor_out(fn, out, n, h, w, dtype, channels_last)
    if n == 0:
        return out
    elem = out.element_size()
    with _on_task_stream(resizer, out.device):
        ok = resizer.ExecutePerspsToTensor(surfaces, index, jobs, out.data_ptr(), _TENSOR_DTYPES[dtype], [float(m) for m in mean], [float(v) for v in std],
                                           cc_ctx, bool(bgr), border, _WARP_MODES[border_mode], s2 * elem, s1 * elem, s0 * elem, bool(channels_last))
    if not ok:
        _refused(fn, _RESIZER_REFUSED)
    return out


def quads_to_homographies(quads, size) -> torch.Tensor:
    """Source quadrilaterals [K, 4, 2] (x, y in luma pixel indices; corners in the order top-left, top-right, bottom-right, bottom-left) -> the float32
    [K, 3, 3] inverse matrices persps_to_normalized_tensor takes for a destination of size = (dw, dh): matrix k sends the destination corners (0, 0),
    (dw - 1, 0), (dw - 1, dh - 1), (0, dh - 1) to quad k's corners.  Solved in float64 with m22 = 1 (destination (0, 0) maps to a finite point, so that
    normalisation always exists), rounded to float32 once.  Pure torch, on whatever device the quads live on.  A degenerate quad (three corners on a
    line) has no homography: its matrix holds non-finite values or torch.linalg.solve raises (on a device input that check is a synchronisation:
    quads_to_homographies_unchecked has none).  ValueError for another shape or dw, dh below 2."""
    return _quads_to_homographies("quads_to_homographies", quads, size, True)


def quads_to_homographies_unchecked(quads, size) -> torch.Tensor:
    """quads_to_homographies through torch.linalg.solve_ex(..., check_errors=False): the same factorisation without the read-back of its status, so it
    never synchronises on a device input — what feeds device_persps_to_normalized_tensor.  Proper quads give the tensor quads_to_homographies gives; a
    degenerate quad raises nothing and yields whatever the factorisation yields, which that entry either refuses as an invalid job (a coefficient that
    is not finite or exceeds 2^24: the normalised border) or samples as a legal matrix — it never reads outside a frame."""
    return _quads_to_homographies("quads_to_homographies_unchecked", quads, size, False)


def _quads_to_homographies(fn, quads, size, check_errors):
    q = torch.as_tensor(quads)
    if q.dim() != 3 or tuple(q.shape[1:]) != (4, 2):
        raise ValueError(f"{fn}: quads must have shape [K, 4, 2], got {tuple(q.shape)}")
    try:
        dw, dh = (operator.index(v) for v in size)
    except (TypeError, ValueError):
        raise ValueError(f"{fn}: size must be (dw, dh), two integers, got {size!r}") from None
    if dw < 2 or dh < 2:
        raise ValueError(f"{fn}: the destination corners must be four different points: dw and dh at least 2, got {(dw, dh)}")
    q = q.to(torch.float64)
    k = q.shape[0]
    if k == 0:
        return torch.zeros((0, 3, 3), dtype=torch.float32, device=q.device)
    d = torch.tensor([[0, 0], [dw - 1, 0], [dw - 1, dh - 1], [0, dh - 1]], dtype=torch.float64, device=q.device)
    # per corner two rows of A h = b, h = (m00 m01 m02 m10 m11 m12 m20 m21):  m00 dx + m01 dy + m02 - X (m20 dx + m21 dy) = X, likewise Y
    a = torch.zeros((k, 8, 8), dtype=torch.float64, device=q.device)
    a[:, 0::2, 0:2] = d
    a[:, 0::2, 2] = 1.0
    a[:, 1::2, 3:5] = d
    a[:, 1::2, 5] = 1.0
    a[:, 0::2, 6:8] = -q[:, :, 0:1] * d
    a[:, 1::2, 6:8] = -q[:, :, 1:2] * d
    b = q.reshape(k, 8, 1)
    h = (torch.linalg.solve(a, b) if check_errors else torch.linalg.solve_ex(a, b, check_errors=False).result).reshape(k, 8)
    return torch.cat([h, torch.ones((k, 1), dtype=torch.float64, device=q.device)], dim=1).to(torch.float32).reshape(k, 3, 3)


def rotated_boxes_to_warps(boxes_cxcywha, dw, dh) -> torch.Tensor:
    """An oriented detector's boxes [K, 5] (cx, cy, w, h, angle in radians; frame pixels with pixel centres at index + 0.5) -> the float32 [K, 2, 3]
    inverse matrices device_warps_to_normalized_tensor (and warps_to_normalized_tensor) take for a dw x dh destination.  Pure torch, on whatever
    device the boxes live on: no sync.  The resize convention: destination pixel (dx, dy) samples
      u = (dx + 0.5) w / dw - w / 2,  v = (dy + 0.5) h / dh - h / 2,  sx = cx + u cos a - v sin a - 0.5,  sy = cy + u sin a + v cos a - 0.5
    so m00 = (w / dw) cos a, m01 = -(h / dh) sin a, m10 = (w / dw) sin a, m11 = (h / dh) cos a and m02, m12 the constants that remain.  A row with a
    non-finite value gives a non-finite matrix: an invalid job, whose output frame is the normalised border."""
    b = torch.as_tensor(boxes_cxcywha)
    if b.dim() != 2 or b.shape[1] != 5 or not b.dtype.is_floating_point:
        raise ValueError(f"rotated_boxes_to_warps: boxes must be a float tensor of shape [K, 5], got {b.dtype} {tuple(b.shape)}")
    dw, dh = int(dw), int(dh)
    if dw < 1 or dh < 1:
        raise ValueError("rotated_boxes_to_warps: dw and dh must be at least 1")
    b = b.to(torch.float32)
    cx, cy, w, h, a = b.unbind(dim=1)
    ax, ay = w / dw, h / dh                      # source pixels per destination pixel along the box's own axes
    cos, sin = torch.cos(a), torch.sin(a)
    m00, m01, m10, m11 = ax * cos, -(ay * sin), ax * sin, ay * cos
    u0, v0 = 0.5 * ax - 0.5 * w, 0.5 * ay - 0.5 * h  # u, v of destination pixel (0, 0)
    m02 = cx + u0 * cos - v0 * sin - 0.5
    m12 = cy + u0 * sin + v0 * cos - 0.5
    return torch.stack([m00, m01, m02, m10, m11, m12], dim=1).reshape(-1, 2, 3)


def device_warps_to_normalized_tensor(resizer, surfaces, matrices, mean, std, surface_index=None, count=None, max_step=None, dtype=torch.float32, bgr=False,
                                      border=(0, 0, 0), border_mode="constant", out=None, cc_ctx=None, channels_last=False) -> torch.Tensor:
    """warps_to_normalized_tensor for matrices that never leave the GPU (PySurfaceConvertResizer.ExecuteWarpsDevToTensor, vpf_convert_warp_tensor_dev):
    no synchronisation, no copy of the matrices to the host, one dispatch, and the call can be captured in a graph that replays with the matrices,
    surface indices and count of replay time.
    `matrices`: a device torch.float32 tensor [K, 2, 3] or [K, 6] whose six elements per job are contiguous (any row stride of at least 6: a slice of a
    wider tensor works), e.g. rotated_boxes_to_warps(...) of a detector's output; `surface_index`: a device torch.int32 tensor [K] (any stride), or
    None: every job samples surfaces[0]; `count`: a device torch.int32 tensor of ONE element (how many rows are valid), or None for all K.
    `max_step`: a bound on |m00| + |m01| and |m10| + |m11| (source pixels per destination pixel step; sqrt(2) s for a 45 degree crop at scale s) that
    sizes the kernel's LDS; None: the 64 KiB default.  It never changes a pixel.  At most 128 surfaces, K at most 65535.  Returns [K, 3, dh, dw]:
      rows below the count with a valid job    the bits warps_to_normalized_tensor gives for that matrix;
      rows below the count with an invalid job (a coefficient that is not finite or exceeds 2^24, no such surface)   the normalised border in both
                                               modes: no surface is read;
      rows at or behind the count              NOT WRITTEN: undefined in a fresh tensor (torch.empty), unchanged in `out`.
    The kernel reads the tables when it runs; this function orders it behind torch's current stream, where their producer ran.  border, border_mode,
    `out`, channels_last, dtype, bgr, the returned tensor and the stream ordering: as warps_to_normalized_tensor.  ValueError for matrices,
    surface_index or count on the host or on another device than each other or `out`, another dtype or shape."""
    return _device_matrices_to_tensor("device_warps_to_normalized_tensor", False, resizer, surfaces, matrices, mean, std, surface_index, count, max_step, dtype, bgr,
                                      border, border_mode, out, cc_ctx, channels_last)


def _device_matrices_to_tensor(fn, persp, resizer, surfaces, matrices, mean, std, surface_index, count, max_step, dtype, bgr, border, border_mode, out, cc_ctx,
                               channels_last):
    """device_warps_to_normalized_tensor (persp False: [K, 2, 3] / [K, 6]) and device_persps_to_normalized_tensor (persp True: [K, 3, 3] / [K, 9]): the
    same checks, the same tables, another kernel"""
    rows, nc = (3, 9) if persp else (2, 6)
    if dtype not in _TENSOR_DTYPES:
        raise ValueError(f"{fn}: dtype must be one of {list(_TENSOR_DTYPES)}")
    if border_mode not in _WARP_MODES:
        raise ValueError(f"{fn}: border_mode must be one of {list(_WARP_MODES)}, got {border_mode!r}")
    try:
        border = [operator.index(v) for v in border]
    except TypeError:
        raise ValueError(f"{fn}: border must hold three integers, got {border!r}") from None
    if len(border) != 3 or any(not 0 <= v <= 255 for v in border):
        raise ValueError(f"{fn}: border must hold three values in 0..255, got {border}")
    surfaces = list(surfaces)
    if not 1 <= len(surfaces) <= 128:
        raise ValueError(f"{fn}: 1 .. 128 surfaces per call, got {len(surfaces)}")
    if not isinstance(matrices, torch.Tensor) or not matrices.is_cuda:
        raise ValueError(f"{fn}: matrices must be a device tensor (for host matrices there is {'persps' if persp else 'warps'}_to_normalized_tensor)")
    if matrices.dtype != torch.float32 or not ((matrices.dim() == 3 and tuple(matrices.shape[1:]) == (rows, 3)) or (matrices.dim() == 2 and matrices.shape[1] == nc)):
        raise ValueError(f"{fn}: matrices must be torch.float32 of shape [K, {rows}, 3] or [K, {nc}], got {matrices.dtype} {tuple(matrices.shape)}")
    n = matrices.shape[0]
    if n > 65535:
        raise ValueError(f"{fn}: at most 65535 matrices per call, got {n}")
    inner = matrices.stride()[1:]
    if inner != ((3, 1) if matrices.dim() == 3 else (1,)) or (n > 1 and matrices.stride(0) < nc):
        raise ValueError(f"{fn}: the {'nine' if persp else 'six'} elements of a matrix must be contiguous and the row stride at least {nc}, got strides {matrices.stride()}")
    if surface_index is not None:
        if not isinstance(surface_index, torch.Tensor) or not surface_index.is_cuda or surface_index.dtype != torch.int32 or tuple(surface_index.shape) != (n,):
            raise ValueError(f"{fn}: surface_index must be a device torch.int32 tensor of shape [{n}], or None")
        if surface_index.device != matrices.device:
            raise ValueError(f"{fn}: surface_index lives on {surface_index.device}, matrices on {matrices.device}")
        if n > 1 and surface_index.stride(0) < 1:
            raise ValueError(f"{fn}: surface_index needs a positive stride, got {surface_index.stride()}")
    if count is not None:
        if not isinstance(count, torch.Tensor) or not count.is_cuda or count.dtype != torch.int32 or count.numel() != 1:
            raise ValueError(f"{fn}: count must be a device torch.int32 tensor of one element, or None")
        if count.device != matrices.device:
            raise ValueError(f"{fn}: count lives on {count.device}, matrices on {matrices.device}")
    if max_step is None:
        max_step = 0.0
    max_step = float(max_step)
    if not (max_step >= 0.0 and max_step < float("inf")):
        raise ValueError(f"{fn}: max_step must be finite and not negative, got {max_step}")
    w, h = resizer.DstSize()
    if out is not None and isinstance(out, torch.Tensor) and out.is_cuda and out.device != matrices.device:
        raise ValueError(f"{fn}: out lives on {out.device}, matrices on {matrices.device}")
    out, s0, s1, s2 = _tensor_out(fn, out, n, h, w, dtype, channels_last, matrices.device)
    if n == 0:
        return out
    elem = out.element_size()
    with _on_task_stream(resizer, out.device):
        execute = resizer.ExecutePerspsDevToTensor if persp else resizer.ExecuteWarpsDevToTensor
        ok = execute(surfaces, matrices.data_ptr(), n, surface_index.data_ptr() if surface_index is not None else 0,
                     count.data_ptr() if count is not None else 0, out.data_ptr(), _TENSOR_DTYPES[dtype], [float(m) for m in mean],
                     [float(v) for v in std], cc_ctx, bool(bgr), border, _WARP_MODES[border_mode], s2 * elem, s1 * elem,
                     (s0 if n > 1 else 0) * elem, bool(channels_last), 4 * (matrices.stride(0) if n > 1 else nc),
                     4 * (surface_index.stride(0) if surface_index is not None and n > 1 else 1), max_step)
    if not ok:
        _refused(fn, _RESIZER_REFUSED)
    return out


def device_persps_to_normalized_tensor(resizer, surfaces, matrices, mean, std, surface_index=None, count=None, max_step=None, dtype=torch.float32, bgr=False,
                                       border=(0, 0, 0), border_mode="constant", out=None, cc_ctx=None, channels_last=False) -> torch.Tensor:
    """persps_to_normalized_tensor for homographies that never leave the GPU (PySurfaceConvertResizer.ExecutePerspsDevToTensor,
    vpf_convert_persp_tensor_dev): no synchronisation, no copy of the matrices to the host, one dispatch, capturable in a graph that replays with the
    matrices, surface indices and count of replay time.
    `matrices`: a device torch.float32 tensor [K, 3, 3] or [K, 9] whose nine elements per job are contiguous (any row stride of at least 9: a slice of a
    wider table works), e.g. quads_to_homographies_unchecked(corners, size) of a corner-regression network's output.  `surface_index`, `count`
    and the three kinds of rows (valid: persps_to_normalized_tensor's bits; invalid — a coefficient that is not finite or exceeds 2^24, no such surface —:
    the normalised border in both modes; at or behind the count: NOT WRITTEN) exactly as device_warps_to_normalized_tensor.
    `max_step`: a bound on the source pixels per destination pixel step over every job and pixel (homographies_max_step of matrices of the kind the
    pipeline produces, calibrated offline) that sizes the kernel's LDS; None: the 64 KiB default.  It never changes a pixel.  ValueError as
    device_warps_to_normalized_tensor."""
    return _device_matrices_to_tensor("device_persps_to_normalized_tensor", True, resizer, surfaces, matrices, mean, std, surface_index, count, max_step, dtype, bgr,
                                      border, border_mode, out, cc_ctx, channels_last)


def homographies_max_step(matrices, dw, dh) -> float:
    """The `max_step` hint of device_persps_to_normalized_tensor for HOST matrices ([K, 3, 3] or [K, 9], as persps_to_normalized_tensor takes them) and a
    dw x dh destination: the maximum of vpf_persp_max_step (PyNvCodec.PerspMaxStep) over them — for every matrix the bound, over the whole destination,
    on |d sx / d dx| + |d sx / d dy| and |d sy / d dx| + |d sy / d dy|.  0.0 (no hint) as soon as one matrix has no bound (a destination corner at or
    behind the horizon), and for K == 0.  Meant for calibration, offline: pass the largest value seen to the device entry."""
    fn = "homographies_max_step"
    jobs = _matrices_list(matrices, fn, rows=3)
    try:
        dw, dh = operator.index(dw), operator.index(dh)
    except TypeError:
        raise ValueError(f"{fn}: dw and dh must be integers") from None
    if not (1 <= dw <= 65536 and 1 <= dh <= 65536):
        raise ValueError(f"{fn}: dw and dh must lie in 1 .. 65536, got {(dw, dh)}")
    try:
        import PyNvCodec as nvc
    except ImportError:  # package-relative import when used as videoprocessingframework_amd.PytorchNvCodec
        from .. import PyNvCodec as nvc
    best = 0.0
    for m in jobs:
        step = float(nvc.PerspMaxStep(m, dw, dh))
        if step == 0.0:
            return 0.0
        best = max(best, step)
    return best


def _check_map(fn, name, m, w, h):
    """one coordinate map of remap_to_normalized_tensor: a device float32 tensor [h, w] or [N, h, w] with unit stride along its rows"""
    if not isinstance(m, torch.Tensor) or not m.is_cuda:
        raise ValueError(f"{fn}: {name} must be a device tensor (the kernel reads the maps from device memory)")
    if m.dtype != torch.float32 or m.dim() not in (2, 3) or tuple(m.shape[-2:]) != (h, w):
        raise ValueError(f"{fn}: {name} must be torch.float32 of shape [{h}, {w}] or [N, {h}, {w}], got {m.dtype} {tuple(m.shape)}")
    if (w > 1 and m.stride(-1) != 1) or (h > 1 and m.stride(-2) < w):
        raise ValueError(f"{fn}: {name} needs unit stride along its rows and a row stride of at least {w}, got strides {m.stride()}")


def remap_to_normalized_tensor(resizer, surfaces, xmap, ymap, mean, std, max_step=None, dtype=torch.float32, bgr=False, border=(0, 0, 0),
                               border_mode="constant", out=None, cc_ctx=None, channels_last=False) -> torch.Tensor:
    """N NV12 / YUV420 (or P10 / P12) surfaces, each sampled through a per-pixel coordinate map -> the normalised float tensor [N, 3, dh, dw]: lens
    undistortion, fisheye and surround-view rigs, rectification, flow-driven warps — one pass instead of convert, remap and a normalise chain
    (PySurfaceConvertResizer.ExecuteRemapToTensor, vpf_convert_remap_tensor).
    `xmap`, `ymap`: device torch.float32 tensors [dh, dw] (one pair shared by every surface: one camera, a batch of its frames) or [N, dh, dw] (a pair
    per surface: a rig, a flow field per frame); last stride 1, any row stride (a slice of a wider tensor works), e.g. undistort_maps(...).  Output
    pixel (x, y) of frame i samples surfaces[i] at (xmap[y][x], ymap[y][x]) in luma pixels, remap's convention.  A pixel whose coordinate is NaN
    takes `border` under BOTH border modes (how calibration tools mark invalid pixels); every other pixel outside the surface takes `border`
    (per output channel, 0..255) under "constant" and the nearest edge pixel under "replicate".
    `max_step`: a bound on the source pixels per destination pixel step of the maps (maps_max_step, calibrated offline) that sizes the kernel's
    LDS; None: the 64 KiB default.  It never changes a pixel.
    The kernel reads the maps when it runs: no synchronisation, no copy to the host, and a captured graph replays with the maps of replay time.
    This function orders the call behind torch's current stream, where the maps' producer ran.  Normalisation, `out`, channels_last, the returned
    tensor and the stream ordering: exactly as to_normalized_tensor.

    ValueError for maps on the host or on another device than each other or `out`, another dtype or shape, a border value outside 0..255, an
    unknown mode, a bad max_step.  N == 0 returns an empty tensor without a launch."""
    fn = "remap_to_normalized_tensor"
    if dtype not in _TENSOR_DTYPES:
        raise ValueError(f"{fn}: dtype must be one of {list(_TENSOR_DTYPES)}")
    if border_mode not in _WARP_MODES:
        raise ValueError(f"{fn}: border_mode must be one of {list(_WARP_MODES)}, got {border_mode!r}")
    try:
        border = [operator.index(v) for v in border]
    except TypeError:
        raise ValueError(f"{fn}: border must hold three integers, got {border!r}") from None
    if len(border) != 3 or any(not 0 <= v <= 255 for v in border):
        raise ValueError(f"{fn}: border must hold three values in 0..255, got {border}")
    if max_step is None:
        max_step = 0.0
    max_step = float(max_step)
    if not (max_step >= 0.0 and max_step < float("inf")):
        raise ValueError(f"{fn}: max_step must be finite and not negative, got {max_step}")
    surfaces = list(surfaces)
    n = len(surfaces)
    w, h = resizer.DstSize()
    _check_map(fn, "xmap", xmap, w, h)
    _check_map(fn, "ymap", ymap, w, h)
    if xmap.device != ymap.device:
        raise ValueError(f"{fn}: xmap lives on {xmap.device}, ymap on {ymap.device}")
    if xmap.dim() != ymap.dim():
        raise ValueError(f"{fn}: xmap and ymap must both be shared [{h}, {w}] or both per frame [N, {h}, {w}]")
    map_stride = 0
    if xmap.dim() == 3:
        if xmap.shape[0] != n or ymap.shape[0] != n:
            raise ValueError(f"{fn}: {n} surfaces need maps of shape [{n}, {h}, {w}], got {tuple(xmap.shape)} and {tuple(ymap.shape)}")
        if n > 1:
            if xmap.stride(0) != ymap.stride(0):
                raise ValueError(f"{fn}: xmap and ymap need the same stride from frame to frame, got {xmap.stride(0)} and {ymap.stride(0)}")
            map_stride = 4 * xmap.stride(0)
    if out is not None and isinstance(out, torch.Tensor) and out.is_cuda and out.device != xmap.device:
        raise ValueError(f"{fn}: out lives on {out.device}, the maps on {xmap.device}")
    out, s0, s1, s2 = _tensor_out(fn, out, n, h, w, dtype, channels_last, xmap.device)
    if n == 0:
        return out
    elem = out.element_size()
    with _on_task_stream(resizer, out.device):
        ok = resizer.ExecuteRemapToTensor(surfaces, xmap.data_ptr(), ymap.data_ptr(), out.data_ptr(), _TENSOR_DTYPES[dtype], [float(m) for m in mean],
                                          [float(v) for v in std], cc_ctx, bool(bgr), border, _WARP_MODES[border_mode], s2 * elem, s1 * elem, s0 * elem,
                                          bool(channels_last), 4 * (xmap.stride(-2) if h > 1 else w), 4 * (ymap.stride(-2) if h > 1 else w), map_stride, max_step)
    if not ok:
        _refused(fn, _RESIZER_REFUSED)
    return out


def maps_max_step(xmap, ymap) -> float:
    """The `max_step` hint of remap_to_normalized_tensor for given maps ([dh, dw] or [N, dh, dw], host or device): the maximum over their pixels of
    |s[y][x + 1] - s[y][x]| + |s[y + 1][x] - s[y][x]| for s = xmap and for s = ymap — the source pixels per destination pixel step —, differences
    that are not finite (a NaN or an infinity on either side) or that leave the map counting as 0; computed in float64 and rounded UP to float32.
    0.0 for maps without a finite difference.  It reads the result back, so it SYNCHRONISES on device maps: meant for calibration, offline — pass
    the largest value seen to remap_to_normalized_tensor."""
    fn = "maps_max_step"
    best = 0.0
    for name, m in (("xmap", xmap), ("ymap", ymap)):
        m = torch.as_tensor(m)
        if not m.dtype.is_floating_point or m.dim() not in (2, 3):
            raise ValueError(f"{fn}: {name} must be a float tensor of shape [dh, dw] or [N, dh, dw], got {m.dtype} {tuple(m.shape)}")
        if m.numel() == 0:
            continue
        s = m.detach().to(torch.float64)
        step = torch.zeros_like(s)
        dx = (s[..., :, 1:] - s[..., :, :-1]).abs()
        dy = (s[..., 1:, :] - s[..., :-1, :]).abs()
        step[..., :, :-1] += torch.where(torch.isfinite(dx), dx, torch.zeros_like(dx))
        step[..., :-1, :] += torch.where(torch.isfinite(dy), dy, torch.zeros_like(dy))
        best = max(best, float(step.max()))
    r = torch.tensor(best, dtype=torch.float64).to(torch.float32)
    if float(r) < best:
        r = torch.nextafter(r, torch.tensor(float("inf"), dtype=torch.float32))
    return float(r)


def undistort_maps(camera_matrix, dist_coeffs, size, new_camera_matrix=None, device=None):
    """The (xmap, ymap) pair remap_to_normalized_tensor takes to undistort a camera: float32 tensors [dh, dw] on `device` for size = (dw, dh), from the
    Brown-Conrady model with dist_coeffs = (k1, k2, p1, p2[, k3]).  For destination pixel (u, v), with (fx', fy', cx', cy') from new_camera_matrix
    (default: camera_matrix) and (fx, fy, cx, cy) from camera_matrix (3 x 3: fx = [0][0], fy = [1][1], cx = [0][2], cy = [1][2]):
      x = (u - cx') / fx',  y = (v - cy') / fy',  r2 = x^2 + y^2,  rad = 1 + k1 r2 + k2 r2^2 + k3 r2^3
      xd = x rad + 2 p1 x y + p2 (r2 + 2 x^2),  yd = y rad + p1 (r2 + 2 y^2) + 2 p2 x y
      sx = fx xd + cx,  sy = fy yd + cy
    computed in float64 on the host and rounded to float32 once.  ValueError for another shape, a non-finite value, fx' or fy' of 0."""
    fn = "undistort_maps"
    import numpy as np

    def host64(v):
        if isinstance(v, torch.Tensor):
            v = v.detach().cpu().numpy()
        return torch.from_numpy(np.array(v, dtype=np.float64))

    K = host64(camera_matrix)
    Kn = K if new_camera_matrix is None else host64(new_camera_matrix)
    d = host64(dist_coeffs).reshape(-1)
    if tuple(K.shape) != (3, 3) or tuple(Kn.shape) != (3, 3):
        raise ValueError(f"{fn}: camera matrices must have shape [3, 3], got {tuple(K.shape)} and {tuple(Kn.shape)}")
    if d.numel() not in (4, 5):
        raise ValueError(f"{fn}: dist_coeffs must hold (k1, k2, p1, p2) or (k1, k2, p1, p2, k3), got {d.numel()} values")
    if not bool(torch.isfinite(K).all() and torch.isfinite(Kn).all() and torch.isfinite(d).all()):
        raise ValueError(f"{fn}: camera matrices and dist_coeffs must be finite")
    try:
        dw, dh = (operator.index(v) for v in size)
    except (TypeError, ValueError):
        raise ValueError(f"{fn}: size must be (dw, dh), two integers") from None
    if not (1 <= dw <= 65536 and 1 <= dh <= 65536):
        raise ValueError(f"{fn}: dw and dh must lie in 1 .. 65536, got {(dw, dh)}")
    fx, fy, cx, cy = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
    fxn, fyn, cxn, cyn = float(Kn[0, 0]), float(Kn[1, 1]), float(Kn[0, 2]), float(Kn[1, 2])
    if fxn == 0.0 or fyn == 0.0:
        raise ValueError(f"{fn}: the focal lengths of the new camera matrix must not be 0")
    k1, k2, p1, p2 = (float(v) for v in d[:4])
    k3 = float(d[4]) if d.numel() == 5 else 0.0
    u = torch.arange(dw, dtype=torch.float64)[None, :]
    v = torch.arange(dh, dtype=torch.float64)[:, None]
    x = ((u - cxn) / fxn).expand(dh, dw)
    y = ((v - cyn) / fyn).expand(dh, dw)
    r2 = x * x + y * y
    rad = 1.0 + k1 * r2 + k2 * (r2 * r2) + k3 * (r2 * r2 * r2)
    xd = x * rad + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * (x * x))
    yd = y * rad + p1 * (r2 + 2.0 * (y * y)) + 2.0 * p2 * x * y
    sx = (fx * xd + cx).to(torch.float32).contiguous()
    sy = (fy * yd + cy).to(torch.float32).contiguous()
    if device is not None:
        sx, sy = sx.to(device), sy.to(device)
    return sx, sy


def _dst_rects_list(dst_rects, n, w, h, fn):
    """dst_rects -> list of n 4-tuples of Python ints inside the w x h destination: ValueError for a device tensor, a non-integer dtype, another
    length than the rois', an empty rectangle or one that leaves the destination"""
    if isinstance(dst_rects, torch.Tensor):
        if dst_rects.device.type != "cpu":
            raise ValueError(f"{fn}: dst_rects must live on the host (the job table is built on the CPU): pass dst_rects.cpu()")
        if dst_rects.dtype.is_floating_point or dst_rects.dtype.is_complex or dst_rects.dtype == torch.bool:
            raise ValueError(f"{fn}: dst_rects must hold integers, got {dst_rects.dtype}")
        dst_rects = dst_rects.tolist()
    elif hasattr(dst_rects, "dtype") and hasattr(dst_rects, "tolist"):  # numpy.ndarray
        if getattr(dst_rects.dtype, "kind", "") not in "iu":
            raise ValueError(f"{fn}: dst_rects must hold integers, got {dst_rects.dtype}")
        dst_rects = dst_rects.tolist()
    dst_rects = list(dst_rects)
    if len(dst_rects) != n:
        raise ValueError(f"{fn}: {len(dst_rects)} dst_rects for {n} rois")
    out = []
    for i, r in enumerate(dst_rects):
        r = tuple(r)
        try:
            if len(r) != 4:
                raise TypeError
            ix, iy, iw, ih = (operator.index(v) for v in r)
        except TypeError:
            raise ValueError(f"{fn}: dst_rects[{i}] must be four integers (ix, iy, iw, ih), got {r}") from None
        if ix < 0 or iy < 0 or iw < 1 or ih < 1 or ix + iw > w or iy + ih > h:
            raise ValueError(f"{fn}: dst_rects[{i}] = (ix {ix}, iy {iy}, iw {iw}, ih {ih}) is empty or leaves the {w} x {h} destination")
        out.append((ix, iy, iw, ih))
    return out


def letterbox_to_normalized_tensor(resizer, surfaces, mean, std, rois=None, dst_rects=None, pad=(114, 114, 114), dtype=torch.float32, bgr=False, out=None,
                                   cc_ctx=None, channels_last=False, *, antialias=False):
    """Letterbox: K rectangles of NV12 / YUV420 (or P10 / P12) surfaces, each resized into a rectangle of its own inside its [3, dh, dw] frame and the
    rest of the frame padded with a constant — the aspect-preserving input of a detector (YOLO's 114-grey letterbox) and of ReID / face / OCR networks
    that take padded crops —, normalised, in one dispatch per 82 jobs (PySurfaceConvertResizer.ExecuteLetterboxToTensor, vpf_convert_letterbox_tensor).
    `rois` as in rois_to_normalized_tensor; None: one job per surface, the whole frame.  `dst_rects`: per job (ix, iy, iw, ih) in destination pixels,
    inside the resizer's destination size (a sequence of integer 4-tuples or a CPU integer tensor / ndarray [K, 4]); None: the aspect-preserving,
    centred fit of each job's rectangle (PyNvCodec.LetterboxFit: integer arithmetic, round half up).  `pad`: three values 0..255, per output channel
    (B G R order when bgr=True), written THROUGH the normalisation like every pixel.

    Returns (tensor, placement): the [K, 3, dh, dw] tensor and a CPU int64 tensor [K, 4] of the destination rectangles used.  Inside its rectangle a
    job holds the bits rois_to_normalized_tensor gives for a resizer of size (iw, ih); a dst_rect that is the whole destination gives
    rois_to_normalized_tensor's bits.  The map back to frame coordinates, for a detector's boxes (likewise y with rect.y, iy, h, ih):
        x_frame = rect.x + (x_dst - ix + 0.5) * w / iw - 0.5

    `out`, channels_last and the stream ordering: exactly as to_normalized_tensor.  ValueError for what rois_to_normalized_tensor refuses, for a pad
    that is not three integers in 0..255, for rois and dst_rects of different lengths and for a dst_rect that is empty or leaves the destination.
    K == 0 returns an empty tensor and an empty placement without a launch.

    antialias=True (keyword only): inside its rectangle a job goes through the triangle filter whose support grows with the scale — PIL's
    Image.resize(BILINEAR) and F.interpolate(mode="bilinear", antialias=True), within 1 LSB of either — instead of the bare bilinear pair, which past a
    2 x down-scale skips source pixels (PySurfaceConvertResizer.ExecuteLetterboxAAToTensor, vpf_convert_letterbox_tensor_aa).  With rois=None and
    dst_rects = the whole destination, [(0, 0, dw, dh)] * K, this is the antialiased whole-frame call; with rois and that dst_rects the antialiased
    ROI call.  The same arguments, refusals and return value; the default, antialias=False, is bit for bit what it was."""
    fn = "letterbox_to_normalized_tensor"
    try:
        import PyNvCodec as nvc
    except ImportError:  # package-relative import when used as videoprocessingframework_amd.PytorchNvCodec
        from .. import PyNvCodec as nvc
    if dtype not in _TENSOR_DTYPES:
        raise ValueError(f"{fn}: dtype must be one of {list(_TENSOR_DTYPES)}")
    try:
        pad = [operator.index(v) for v in pad]
    except TypeError:
        raise ValueError(f"{fn}: pad must hold three integers, got {pad!r}") from None
    if len(pad) != 3 or any(not 0 <= v <= 255 for v in pad):
        raise ValueError(f"{fn}: pad must hold three values in 0..255, got {pad}")
    surfaces = list(surfaces)
    if rois is None:
        rois = [(i, 0, 0, s.Width(), s.Height()) for i, s in enumerate(surfaces)]
    jobs = _rois_list(rois, surfaces, fn)
    n = len(jobs)
    w, h = resizer.DstSize()
    if dst_rects is None:
        rects = [tuple(int(v) for v in nvc.LetterboxFit(j[3], j[4], w, h)) for j in jobs]
    else:
        rects = _dst_rects_list(dst_rects, n, w, h, fn)
    placement = torch.tensor(rects, dtype=torch.int64).reshape(n, 4)
    out, s0, s1, s2 = _tensor_out(fn, out, n, h, w, dtype, channels_last)
    if n == 0:
        return out, placement
    elem = out.element_size()
    with _on_task_stream(resizer, out.device):
        execute = resizer.ExecuteLetterboxAAToTensor if antialias else resizer.ExecuteLetterboxToTensor
        ok = execute(surfaces, jobs, rects, out.data_ptr(), _TENSOR_DTYPES[dtype], [float(m) for m in mean], [float(v) for v in std],
                     cc_ctx, bool(bgr), pad, s2 * elem, s1 * elem, s0 * elem, bool(channels_last))
    if not ok:
        _refused(fn, _RESIZER_REFUSED)
    return out, placement


def letterbox_fit_boxes(boxes, dw, dh) -> torch.Tensor:
    """The placements device_letterbox_to_normalized_tensor computes for itself when it gets no dst_rects, as a table: `boxes` = the integer [K, 5] table
    of (surface_index, x, y, w, h) rows -> a torch.int32 [K, 4] table of (ix, iy, iw, ih), row k = the aspect-preserving, centred fit of a w x h picture
    inside dw x dh (PyNvCodec.LetterboxFit, vpf_letterbox_fit: integer arithmetic, round half up).  Pure torch in int64, on whatever device the boxes
    live on: no sync.  A row with w < 1 or h < 1 gives zeros — as a dst_rects row an invalid placement, whose output frame is the normalised pad.
    What a caller needs to map a keypoint or a box of the crop's network back (x_frame = x + (x_dst - ix + 0.5) * w / iw - 0.5, likewise y), and as an
    explicit `dst_rects` it reproduces the dst_rects=None path bit for bit."""
    fn = "letterbox_fit_boxes"
    b = torch.as_tensor(boxes)
    if b.dim() != 2 or b.shape[1] != 5 or b.dtype.is_floating_point or b.dtype.is_complex or b.dtype == torch.bool:
        raise ValueError(f"{fn}: boxes must be an integer tensor of shape [K, 5], got {b.dtype} {tuple(b.shape)}")
    DW, DH = int(dw), int(dh)
    if not (1 <= DW <= 65536 and 1 <= DH <= 65536):
        raise ValueError(f"{fn}: dw and dh must lie in 1 .. 65536, got {DW} x {DH}")
    w, h = b[:, 3].to(torch.int64), b[:, 4].to(torch.int64)
    bad = (w < 1) | (h < 1)
    one = torch.ones_like(w)
    w, h = torch.where(bad, one, w), torch.where(bad, one, h)  # (no division by zero; the row is zeroed below)
    wide = w * DH >= h * DW  # width-limited
    num = torch.where(wide, 2 * h * DW + w, 2 * w * DH + h)
    den = torch.where(wide, 2 * w, 2 * h)
    q = torch.div(num, den, rounding_mode="floor").clamp(min=1)  # round half up; all operands positive
    q = torch.minimum(q, torch.where(wide, DH * one, DW * one))
    iw, ih = torch.where(wide, DW * one, q), torch.where(wide, q, DH * one)
    ix, iy = torch.div(DW - iw, 2, rounding_mode="floor"), torch.div(DH - ih, 2, rounding_mode="floor")
    out = torch.stack([ix, iy, iw, ih], dim=1)
    return torch.where(bad[:, None], torch.zeros_like(out), out).to(torch.int32)


def device_letterbox_to_normalized_tensor(resizer, surfaces, boxes, mean, std, count=None, dst_rects=None, pad=(114, 114, 114), dtype=torch.float32,
                                          bgr=False, out=None, cc_ctx=None, channels_last=False) -> torch.Tensor:
    """letterbox_to_normalized_tensor for boxes that never leave the GPU (PySurfaceConvertResizer.ExecuteLetterboxDevToTensor,
    vpf_convert_letterbox_tensor_dev): the padded ReID / face / OCR crops behind a detector and its NMS, without synchronisation, without a copy of the
    boxes to the host, in one dispatch, and capturable in a graph that replays with the boxes, placements and count of replay time.
    `boxes` and `count` as in device_rois_to_normalized_tensor.  `dst_rects`: a device torch.int32 tensor [K, 4] of (ix, iy, iw, ih) rows on the boxes'
    device (last stride 1, row stride >= 4), or None: the kernel fits every box into the resizer's destination size itself, aspect-preserving and
    centred — letterbox_fit_boxes(boxes, dw, dh) is that table, for the way back.  `pad` as in letterbox_to_normalized_tensor.  Returns [K, 3, dh, dw]:
      rows below the count, valid box and placement      the bits letterbox_to_normalized_tensor gives for that rectangle and placement;
      rows below the count, invalid box or placement     the normalised pad in every element: nothing is clipped and no surface is read;
      rows at or behind the count                        NOT WRITTEN: undefined in a fresh tensor (torch.empty), unchanged in `out`.
    `out`, channels_last, dtype, bgr, the returned tensor and the stream ordering: as device_rois_to_normalized_tensor.  ValueError for what that
    function refuses, for a bad pad, and for dst_rects on the host or on another device than the boxes, of another dtype or shape."""
    fn = "device_letterbox_to_normalized_tensor"
    if dtype not in _TENSOR_DTYPES:
        raise ValueError(f"{fn}: dtype must be one of {list(_TENSOR_DTYPES)}")
    try:
        pad = [operator.index(v) for v in pad]
    except TypeError:
        raise ValueError(f"{fn}: pad must hold three integers, got {pad!r}") from None
    if len(pad) != 3 or any(not 0 <= v <= 255 for v in pad):
        raise ValueError(f"{fn}: pad must hold three values in 0..255, got {pad}")
    surfaces = list(surfaces)
    if not 1 <= len(surfaces) <= 128:
        raise ValueError(f"{fn}: 1 .. 128 surfaces per call, got {len(surfaces)}")
    if not isinstance(boxes, torch.Tensor) or not boxes.is_cuda:
        raise ValueError(f"{fn}: boxes must be a device tensor (for host boxes there is letterbox_to_normalized_tensor)")
    if boxes.dtype != torch.int32 or boxes.dim() != 2 or boxes.shape[1] != 5:
        raise ValueError(f"{fn}: boxes must be torch.int32 of shape [K, 5], got {boxes.dtype} {tuple(boxes.shape)}")
    n = boxes.shape[0]
    if n > 65535:
        raise ValueError(f"{fn}: at most 65535 boxes per call, got {n}")
    if boxes.stride(1) != 1 or (n > 1 and boxes.stride(0) < 5):
        raise ValueError(f"{fn}: boxes needs unit stride along its rows and a row stride of at least 5, got strides {boxes.stride()}")
    if count is not None:
        if not isinstance(count, torch.Tensor) or not count.is_cuda or count.dtype != torch.int32 or count.numel() != 1:
            raise ValueError(f"{fn}: count must be a device torch.int32 tensor of one element, or None")
        if count.device != boxes.device:
            raise ValueError(f"{fn}: count lives on {count.device}, boxes on {boxes.device}")
    if dst_rects is not None:
        if not isinstance(dst_rects, torch.Tensor) or not dst_rects.is_cuda:
            raise ValueError(f"{fn}: dst_rects must be a device tensor, or None (for host placements there is letterbox_to_normalized_tensor)")
        if dst_rects.dtype != torch.int32 or dst_rects.dim() != 2 or tuple(dst_rects.shape) != (n, 4):
            raise ValueError(f"{fn}: dst_rects must be torch.int32 of shape [{n}, 4], got {dst_rects.dtype} {tuple(dst_rects.shape)}")
        if dst_rects.device != boxes.device:
            raise ValueError(f"{fn}: dst_rects lives on {dst_rects.device}, boxes on {boxes.device}")
        if dst_rects.stride(1) != 1 or (n > 1 and dst_rects.stride(0) < 4):
            raise ValueError(f"{fn}: dst_rects needs unit stride along its rows and a row stride of at least 4, got strides {dst_rects.stride()}")
    w, h = resizer.DstSize()
    if out is not None and isinstance(out, torch.Tensor) and out.is_cuda and out.device != boxes.device:
        raise ValueError(f"{fn}: out lives on {out.device}, boxes on {boxes.device}")
    out, s0, s1, s2 = _tensor_out(fn, out, n, h, w, dtype, channels_last, boxes.device)
    if n == 0:
        return out
    elem = out.element_size()
    with _on_task_stream(resizer, out.device):
        ok = resizer.ExecuteLetterboxDevToTensor(surfaces, boxes.data_ptr(), n, count.data_ptr() if count is not None else 0,
                                                 dst_rects.data_ptr() if dst_rects is not None else 0, out.data_ptr(), _TENSOR_DTYPES[dtype],
                                                 [float(m) for m in mean], [float(v) for v in std], cc_ctx, bool(bgr), pad, s2 * elem, s1 * elem,
                                                 (s0 if n > 1 else 0) * elem, bool(channels_last), 4 * (boxes.stride(0) if n > 1 else 5),
                                                 4 * (dst_rects.stride(0) if dst_rects is not None and n > 1 else 4))
    if not ok:
        _refused(fn, _RESIZER_REFUSED)
    return out


def from_normalized_tensor(converter, tensor, mean, std, bgr=False, cc_ctx=None, out=None, channels_last=False):
    """A model's output -> NV12 / YUV420 surfaces for the encoder, in one pass (PyTensorToSurface.ExecuteBatch): `tensor` is [N, 3, H, W] or
    [3, H, W] of float32 / float16 / bfloat16 on the device, normalised with torchvision's mean / std (per input plane; B G R planes when
    bgr=True).  Every element goes through x * (255 std) + (255 mean) in fp32 (a multiply, then an add), is clamped to [0, 255] (NaN -> 0) and
    rounded to nearest even; the surface bytes are those of PySurfaceConverter RGB_PLANAR -> YUV420 (-> NV12) on these planes (BT.601; JPEG
    range unless cc_ctx says MPEG).

    The tensor needs unit stride along W and positive row, plane and frame strides, rows at least W elements apart; beyond that the strides
    are free (a slice of a larger batch, padded rows).  A zero stride (an expand()ed channel, frame or row) is refused with a ValueError:
    call .contiguous() first.  The tensor must live on the converter's GPU.  Returns the list of surfaces: `out` (N surfaces of the
    converter's size and format) if given, else new ones on that GPU.  The kernel runs on the converter's stream after torch's current stream
    has reached this call, and torch's current stream waits for it: the surfaces can be used on the current stream right away, no host
    synchronisation.

    channels_last=True: `tensor` (still of logical shape [N, 3, H, W]) lies in torch.channels_last memory — what a channels-last model
    returns — and is read as it is, without a .contiguous() copy: strides (s0, 1, s2, 3) with s2 >= 3 W and s0 >= H s2, anything else is a
    ValueError.  The surfaces are byte for byte those of the planar call on tensor.contiguous().  The layout is what this argument says, never
    inferred from the strides."""
    try:
        import PyNvCodec as nvc
    except ImportError:  # package-relative import when used as videoprocessingframework_amd.PytorchNvCodec
        from .. import PyNvCodec as nvc
    if not isinstance(tensor, torch.Tensor) or tensor.dtype not in _TENSOR_DTYPES:
        raise ValueError(f"from_normalized_tensor: tensor must be a torch tensor of one of {list(_TENSOR_DTYPES)}")
    if tensor.dim() == 3:
        tensor = tensor.unsqueeze(0)
    w, h = converter.Size()
    if tensor.dim() != 4 or tuple(tensor.shape[1:]) != (3, h, w):
        raise ValueError(f"from_normalized_tensor: tensor must have shape [N, 3, {h}, {w}] or [3, {h}, {w}], got {tuple(tensor.shape)}")
    n = tensor.shape[0]
    s0, s1, s2, s3 = tensor.stride()
    if channels_last:
        (s0, s2), s1, s3 = _channels_last_strides("from_normalized_tensor", tensor, "the tensor"), 1, 1
    # The binding reads a stride of 0 as "contiguous", so a zero (or negative) stride of a dimension that is really walked must not reach it;
    # a dimension of one element is never walked, and goes down as 0 = default.
    if not channels_last and ((w > 1 and s3 != 1) or (h > 1 and s2 < w) or s1 <= 0 or (n > 1 and s0 <= 0)):
        raise ValueError(f"from_normalized_tensor: tensor needs unit stride along W, rows at least {w} elements apart and positive plane and frame "
                         f"strides (an expanded tensor needs .contiguous() first), got strides {tensor.stride()}")
    if h == 1:
        s2 = 0
    if n == 1:
        s0 = 0
    dev = converter.Device()
    if not tensor.is_cuda or (dev >= 0 and tensor.device.index != dev):
        raise ValueError(f"from_normalized_tensor: tensor must be a device tensor" + (f" on GPU {dev}" if dev >= 0 else "") + f", got one on {tensor.device}")
    if out is not None:
        out = list(out)
        if len(out) != n:
            raise ValueError(f"from_normalized_tensor: out must hold {n} surfaces, got {len(out)}")
    if n == 0:
        return []
    elem = tensor.element_size()
    if out is None:
        with torch.cuda.device(tensor.device):
            out = [nvc.Surface.Make(converter.Format(), w, h, dev if dev >= 0 else tensor.device.index) for _ in range(n)]
    with _on_task_stream(converter, tensor.device) as side:
        ok = converter.ExecuteBatch(tensor.data_ptr(), out, _TENSOR_DTYPES[tensor.dtype], [float(m) for m in mean], [float(v) for v in std], cc_ctx,
                                    bool(bgr), s2 * elem, (0 if channels_last else s1) * elem, s0 * elem, bool(channels_last))
        if side is not None:
            tensor.record_stream(side)  # the caching allocator must not hand the tensor's memory out before the converter has read it
    if not ok:
        _refused("from_normalized_tensor", _CONVERTER_REFUSED)
    return out
