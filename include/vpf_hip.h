/*
 * vpf_hip.h — C ABI of libvpfhip: MI355X (gfx950) surface conversion / resize / remap.
 *
 * This is the drop-in boundary.  In the reference (NVIDIA/VideoProcessingFramework) the
 * C++ Task layer calls closed-source NPP at exactly this edge:
 *
 *   reference caller                                      reference callee (NPP)            replaced by
 *   ----------------------------------------------------  --------------------------------  -------------------
 *   nv12_rgb::Execute        src/TC/src/TasksColorCvt.cpp:122-182  nppiNV12ToRGB_*_8u_P2C3R_Ctx     vpf_convert
 *   nv12_bgr::Execute        TasksColorCvt.cpp:53-108             nppiNV12ToBGR_*_8u_P2C3R_Ctx     vpf_convert
 *   nv12_yuv420::Execute     TasksColorCvt.cpp:196-240            nppiNV12ToYUV420 / nppiYCbCr420  vpf_convert
 *   yuv420_nv12::Execute     TasksColorCvt.cpp:945-975            nppiYCbCr420_8u_P3P2R            vpf_convert
 *   yuv420_rgb/_bgr          TasksColorCvt.cpp:322-369,383-430    nppiYUV420ToRGB / YCbCr420ToRGB  vpf_convert
 *   rgb8_deinterleave/_inter TasksColorCvt.cpp:1059-1088,1102-1131 nppiCopy_8u_C3P3R / _P3C3R      vpf_convert
 *   rgb_bgr / bgr_rgb        TasksColorCvt.cpp:1145-1170,1184-1209 nppiSwapChannels_8u_C3R         vpf_convert
 *   (all other *_Impl in TasksColorCvt.cpp:245-1300)                                               vpf_convert
 *   NppResizeSurfacePacked3C_Impl::Run   src/TC/src/Tasks.cpp:1162-1203  nppiResize_8u_C3R         vpf_resize
 *   NppResizeSurfacePlanar_Impl::Run     Tasks.cpp:1217-1261             nppiResize_8u_C1R         vpf_resize
 *   NppResizeSurfacePacked32F3C_Impl / NppResizeSurface32FPlanar_Impl  Tasks.cpp:1334-1445  nppiResize_32f_C3R / _C1R  vpf_resize
 *   NppRemapSurfacePacked3C_Impl::Run    Tasks.cpp:1555-1602             nppiRemap_8u_C3R          vpf_remap
 *
 * Like the NPP `_Ctx` entry points it replaces, every function here takes raw device pointers,
 * byte pitches, a size, and the stream to launch on; it owns nothing, allocates nothing, never
 * synchronises, and reports failure through its return code (no C++ exceptions cross this edge).
 * All launches are asynchronous on `exec->stream`.
 *
 * Pure C: usable from C, C++, ctypes, cgo, JNI, ... No torch / HIP types in any signature
 * (`stream` is a hipStream_t passed as void*).
 */
#ifndef VPF_HIP_H_
#define VPF_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define VPF_API __attribute__((visibility("default")))
#else
#define VPF_API
#endif

/* Pixel formats. Numeric values are the reference's `Pixel_Format`
 * (src/TC/inc/MemoryInterfaces.hpp:30-49); they are part of the Python ABI. */
typedef enum vpf_pixel_format {
  VPF_FMT_UNDEFINED = 0,
  VPF_FMT_Y = 1,
  VPF_FMT_RGB = 2,
  VPF_FMT_NV12 = 3,
  VPF_FMT_YUV420 = 4,
  VPF_FMT_RGB_PLANAR = 5,
  VPF_FMT_BGR = 6,
  VPF_FMT_YCBCR = 7,
  VPF_FMT_YUV444 = 8,
  VPF_FMT_RGB_32F = 9,
  VPF_FMT_RGB_32F_PLANAR = 10,
  VPF_FMT_YUV422 = 11,
  VPF_FMT_P10 = 12,
  VPF_FMT_P12 = 13,
  VPF_FMT_YUV444_10bit = 14,
  VPF_FMT_YUV420_10bit = 15,
  VPF_FMT_NV12_PLANAR = 16,
  VPF_FMT_GRAY12 = 17
} vpf_pixel_format;

/* src/TC/inc/MemoryInterfaces.hpp:51-61 */
typedef enum vpf_color_space { VPF_BT_601 = 0, VPF_BT_709 = 1, VPF_CS_UNSPEC = 2 } vpf_color_space;
typedef enum vpf_color_range { VPF_MPEG = 0, VPF_JPEG = 1, VPF_CR_UDEF = 2 } vpf_color_range;

typedef enum vpf_interp {
  VPF_INTERP_NEAREST = 0,
  VPF_INTERP_LINEAR = 1,
  VPF_INTERP_LANCZOS3 = 2
} vpf_interp;

typedef enum vpf_status {
  VPF_OK = 0,
  VPF_ERR_UNSUPPORTED = 1, /* format pair / matrix not implemented              */
  VPF_ERR_BAD_ARG = 2,     /* null pointer, zero size, pitch < row bytes, ...    */
  VPF_ERR_LAUNCH = 3,      /* HIP runtime reported an error at launch            */
  VPF_ERR_NO_DEVICE = 4    /* no usable gfx950 device                            */
} vpf_status;

/* One 2-D plane in device memory.  `pitch` is in bytes.  16 bytes, no implicit padding. */
typedef struct vpf_plane {
  void* ptr;
  uint32_t pitch;
  uint32_t reserved; /* must be 0 */
} vpf_plane;

/* Size in pixels of the full-resolution image (plane 0 for YUV formats).  1 .. 65536 per dimension; anything else is
 * VPF_ERR_BAD_ARG (row-byte and offset arithmetic is 32-bit). */
typedef struct vpf_size {
  uint32_t width;
  uint32_t height;
} vpf_size;

/* Where and on which stream to run.  Replaces NppStreamContext
 * (src/TC/src/NppCommon.cpp:10-60).  device < 0 means "current device". */
typedef struct vpf_exec {
  int32_t device;
  uint32_t flags; /* 0 or VPF_EXEC_* hints below; unknown bits are ignored */
  void* stream;   /* hipStream_t; NULL = default stream */
} vpf_exec;

/* Hint: the destination is read again right away (the next kernel of a per-frame chain).  MI355X has a 256 MiB
 * last-level Infinity Cache; by default the converters stream their output past it with non-temporal stores (fastest
 * when nothing re-reads it, e.g. 32-frame batches).  With this flag the single-frame NV12 -> RGB / BGR / RGB_PLANAR
 * kernels use allocating stores instead, so a consumer launched next finds its input on chip (measured: 4K NV12 -> RGB ->
 * RGB_PLANAR 17.7 -> 16.4 us per frame; the converter alone is ~12 % slower).  Pixels are identical either way. */
#define VPF_EXEC_DST_REUSED 1u

/*
 * Plane conventions for `src[]` / `dst[]` (unused entries are ignored, may be zeroed):
 *   Y                      [0] = W x H bytes
 *   NV12                   [0] = Y  (W x H), [1] = interleaved UV (2*ceil(W/2) bytes x ceil(H/2) rows)
 *   YUV420, YCBCR          [0] = Y, [1] = U (ceil(W/2) x ceil(H/2)), [2] = V
 *   YUV444, RGB_PLANAR     [0],[1],[2] = three W x H planes (the reference stacks them in one
 *                          allocation, plane i at base + i*H*pitch: MemoryInterfaces.cpp:1593-1600;
 *                          the caller resolves that to three pointers)
 *   RGB, BGR               [0] = packed 3 bytes / pixel (3W bytes x H)
 *   RGB_32F                [0] = packed 3 floats / pixel; RGB_32F_PLANAR: three float planes
 *   P10, P12               [0] = Y 16-bit, [1] = interleaved UV 16-bit (MSB-aligned samples)
 */

/* Colour / layout conversion of one frame.  Replaces every nppi* call in TasksColorCvt.cpp. */
VPF_API vpf_status vpf_convert(const vpf_exec* exec, int src_fmt, int dst_fmt, int color_space,
                               int color_range, vpf_size size, const vpf_plane src[3],
                               const vpf_plane dst[3]);

typedef struct vpf_frame_io {
  vpf_plane src[3];
  vpf_plane dst[3];
} vpf_frame_io;

/* The same conversion over `n` independent frames of identical size/format, dispatched as few
 * launches as possible (one per 32 frames).  `frames` is a HOST array, consumed before return.
 * Exists because a 4K frame is ~5 us of HBM time, the same order as a kernel boundary. */
VPF_API vpf_status vpf_convert_batch(const vpf_exec* exec, int src_fmt, int dst_fmt,
                                     int color_space, int color_range, vpf_size size, uint32_t n,
                                     const vpf_frame_io* frames);

/* 1 if vpf_convert implements (src_fmt,dst_fmt) under (color_space,color_range), else 0.
 * Pure host logic; callable without a GPU. */
VPF_API int vpf_convert_supported(int src_fmt, int dst_fmt, int color_space, int color_range);

/* Whole-image resize.  `fmt` in {RGB, BGR, Y, YUV420, YCBCR, YUV444, RGB_PLANAR, NV12, RGB_32F,
 * RGB_32F_PLANAR}; every plane is resized independently (chroma planes at their own resolution).
 * Replaces nppiResize_8u_C3R / _C1R (Tasks.cpp:1193,1227-1253) and nppiResize_32f_C3R / _C1R
 * (Tasks.cpp:1376,1434; float results are neither rounded nor clamped, rows must be 4-B aligned). */
VPF_API vpf_status vpf_resize(const vpf_exec* exec, int fmt, int interp, vpf_size src_size,
                              const vpf_plane src[3], vpf_size dst_size, const vpf_plane dst[3]);

/* The same resize over `n` independent same-shape frames, every plane of every frame in as few dispatches as possible (one per 128
 * frames when a frame moves at most 7 000 000 bytes, source + destination — Y / NV12 / YUV420 at 1080p -> 720p and smaller —, one per 64
 * frames for bilinear / nearest frames of up to 10 000 000 bytes — packed RGB 1080p <-> 720p —, else one
 * per 32 frames; when all planes take the same kernel family — always the case for NV12 / YUV420 / planar surfaces allocated by this
 * library — one dispatch carries every plane).  A 720p plane is 2-3 us of GPU work, the same order as a kernel boundary: per-frame, per-plane dispatch leaves the chip
 * idle most of the time.  `frames` is a HOST array consumed before return.  vpf_resize is this call with n = 1. */
VPF_API vpf_status vpf_resize_batch(const vpf_exec* exec, int fmt, int interp, vpf_size src_size, vpf_size dst_size, uint32_t n,
                                    const vpf_frame_io* frames);

/* Scratch memory for the resize filters that keep per-shape operand tables (today: LANCZOS3 on 8-bit surfaces — column / row weight
 * operands of the matrix-core kernel, built once per (source size, destination size) by two small kernels and read by every later call).
 * NPP's pattern for this is a caller-provided buffer (nppiResizeGetBufferSize-style calls next to the NppResize*_Impl classes'
 * own destination surface, Tasks.cpp:1134-1150); here:
 *   - the caller owns `ptr` (device memory, 256-B aligned, `bytes` long) AND this struct: zero `opaque` once, then pass the same struct
 *     with every call that should share the tables.  The library records in `opaque` which tables the region holds.
 *   - a workspace is used on ONE stream at a time (its builds and its launches are ordered by that stream); a call on another stream, or
 *     while the stream is being captured, or with a shape the region does not hold, rebuilds (a few microseconds) — never an error.
 *   - too small a region (or ws == NULL, or the plain vpf_resize / vpf_resize_batch): the library's own small static arena is used
 *     instead (4 MiB per device, least-recently-used eviction); shapes that fit neither evaluate their weights inside the kernel.
 * Pixels are identical on every path.  Freeing `ptr` is the caller's business, after the stream has finished with it. */
typedef struct vpf_workspace {
  void* ptr;
  uint64_t bytes;
  uint64_t opaque[40];
} vpf_workspace;

/* Bytes of workspace that hold the tables of this resize for any batch size (0: this (fmt, interp, sizes) keeps no tables).
 * Pure host logic; callable without a GPU. */
VPF_API uint64_t vpf_resize_workspace_bytes(int fmt, int interp, vpf_size src_size, vpf_size dst_size);

/* vpf_resize / vpf_resize_batch with a caller-owned workspace (may be NULL). */
VPF_API vpf_status vpf_resize_ws(const vpf_exec* exec, int fmt, int interp, vpf_size src_size, const vpf_plane src[3], vpf_size dst_size,
                                 const vpf_plane dst[3], vpf_workspace* ws);
VPF_API vpf_status vpf_resize_batch_ws(const vpf_exec* exec, int fmt, int interp, vpf_size src_size, vpf_size dst_size, uint32_t n,
                                       const vpf_frame_io* frames, vpf_workspace* ws);

/* Per-pixel remap with bilinear sampling, packed RGB/BGR only (Tasks.cpp:1555-1602,
 * nppiRemap_8u_C3R + NPPI_INTER_LINEAR).  xmap/ymap are device pointers to float32 rows of
 * dst_size.width entries, row pitch in bytes.  Destination pixels whose source coordinate lies
 * outside [0,W-1]x[0,H-1] are left untouched. */
VPF_API vpf_status vpf_remap(const vpf_exec* exec, int fmt, vpf_size src_size, const vpf_plane* src,
                             const float* xmap, uint32_t xmap_pitch, const float* ymap,
                             uint32_t ymap_pitch, vpf_size dst_size, const vpf_plane* dst);

/* One pair of maps applied to `n` independent same-shape frames in one dispatch per 32 frames (a camera-undistortion map is the
 * same for every frame of a stream; frames after the first find the maps in the Infinity Cache).  frames[i].src[0] / dst[0] only. */
VPF_API vpf_status vpf_remap_batch(const vpf_exec* exec, int fmt, vpf_size src_size, const float* xmap, uint32_t xmap_pitch, const float* ymap,
                                   uint32_t ymap_pitch, vpf_size dst_size, uint32_t n, const vpf_frame_io* frames);

/* Fused NV12 -> bilinear resize -> packed RGB/BGR / RGB_PLANAR in one pass: reads only the source
 * texels it needs (BASELINE.md config 3 "fused").  Result is defined as: convert every NV12 texel
 * with vpf_convert's arithmetic, then vpf_resize(LINEAR) of the RGB image. */
VPF_API vpf_status vpf_convert_resize(const vpf_exec* exec, int src_fmt, int dst_fmt,
                                      int color_space, int color_range, vpf_size src_size,
                                      const vpf_plane src[3], vpf_size dst_size,
                                      const vpf_plane dst[3]);

/* The same over `n` independent same-shape frames in as few dispatches as possible (one per 128 frames when a frame moves at most
 * 7 000 000 bytes, source + destination — up to 1080p -> 720p —, one per 64 frames up to 10 000 000 bytes — 720p -> 1080p —, else one per 32 frames): a 720p output is ~2 us of HBM time, far below
 * a kernel boundary, so per-frame dispatch leaves the GPU mostly idle. */
VPF_API vpf_status vpf_convert_resize_batch(const vpf_exec* exec, int src_fmt, int dst_fmt, int color_space,
                                            int color_range, vpf_size src_size, vpf_size dst_size, uint32_t n,
                                            const vpf_frame_io* frames);

/*
 * Fused NV12 / YUV420 -> bilinear resize -> normalised planar tensor (what a DNN consumes: float [N, 3, H, W]) in one pass.
 * For every destination pixel and channel c, with u8[c] the byte vpf_convert_resize(..., RGB_PLANAR, ...) writes:
 *   out[c] = round_to_dtype(fmaf(u8[c], scale[c], bias[c]))     one fp32 fused multiply-add, then round-to-nearest-even to f16 / bf16
 * (torchvision's normalize(mean, std) after a division by 255: scale = 1 / (255 std), bias = -mean / std, both rounded to fp32).
 * dst[0..2] are the three planes of the frame in output channel order (R G B, or B G R with VPF_TENSOR_BGR; scale[c] / bias[c] belong to
 * output channel c): dst_size.width elements per row, `pitch` in bytes.  Plane pointers and pitches must be multiples of the element size
 * and pitch >= width x element size (contiguous NCHW, a slice of a larger batch tensor and padded rows are all such planes).
 * Unknown dtype or flag bits: VPF_ERR_UNSUPPORTED; a non-finite scale / bias or a misaligned plane: VPF_ERR_BAD_ARG.
 *
 * 10 / 12-bit sources: src_fmt = VPF_FMT_P10 / VPF_FMT_P12 (16-bit MSB-aligned semi-planar, what HEVC Main10 / AV1 / HDR decoders hand over) is
 * accepted by this entry, its batch form, vpf_convert_resize_tensor_rois and vpf_convert_warp_tensor — and by these four only.  src[0] = Y, W samples
 * of 2 bytes per row; src[1] = interleaved U V, 2 ceil(W / 2) samples per row, ceil(H / 2) rows; `pitch` in bytes; plane pointers and pitches
 * must be multiples of 2 (else VPF_ERR_BAD_ARG, like short pitches).  Every luma and chroma sample v is first replaced by
 * min(255, (v + 128) >> 8) — what vpf_convert(P10 | P12 -> NV12) writes; P10 and P12 are the same code: the low bits take part in the rounding —
 * and everything downstream is the NV12 definition: the output is bit-identical to the same entry for VPF_FMT_NV12 on the planes
 * vpf_convert(P10 | P12 -> NV12) writes for that frame, without that pass over the whole frame.  This is deliberately NOT a full-precision
 * conversion (the 10 bits fed into the matrix): that would be a definition with nothing to test it against.  vpf_convert_resize(_batch),
 * vpf_convert_supported and vpf_resize answer for P10 / P12 as before.
 *
 * Channels-last (NHWC, torch.channels_last) tensors: flags | VPF_TENSOR_NHWC, accepted by this entry, its batch form,
 * vpf_convert_resize_tensor_rois, vpf_convert_warp_tensor (destination) and vpf_tensor_convert(_batch) (source), for every source format, dtype
 * and channel order they take.  dst[0] (src[0] on the way back) is then the ONE interleaved plane of the frame or job: element (y, x, c) lies at
 * ptr + y * pitch + (3 x + c) * element size, c in output channel order (R G B, or B G R with VPF_TENSOR_BGR; scale[c], bias[c] and the warp's
 * border[c] belong to channel c as ever).  dst[1] and dst[2] are ignored and may be zero.  ptr and pitch must be multiples of the element size
 * and pitch >= 3 x width x element size (else VPF_ERR_BAD_ARG).  Element (y, x, c) is bit for bit the element (c, y, x) the same call writes
 * without the flag, and vpf_tensor_convert's output is bit for bit the planar call's on the de-interleaved planes.  Flag bits other than
 * VPF_TENSOR_BGR | VPF_TENSOR_NHWC (2 included): VPF_ERR_UNSUPPORTED.
 */
typedef enum vpf_tensor_dtype { VPF_TENSOR_F32 = 0, VPF_TENSOR_F16 = 1, VPF_TENSOR_BF16 = 2 } vpf_tensor_dtype;
#define VPF_TENSOR_BGR 1u  /* vpf_tensor_norm.flags: channel order B G R */
#define VPF_TENSOR_NHWC 4u /* vpf_tensor_norm.flags: one interleaved plane [H, W, 3] per frame instead of three planes */
typedef struct vpf_tensor_norm {
  float scale[3];
  float bias[3];
  uint32_t dtype; /* vpf_tensor_dtype */
  uint32_t flags; /* 0 or any of VPF_TENSOR_BGR | VPF_TENSOR_NHWC */
} vpf_tensor_norm;
VPF_API vpf_status vpf_convert_resize_tensor(const vpf_exec* exec, int src_fmt, int color_space, int color_range, vpf_size src_size,
                                             const vpf_plane src[3], vpf_size dst_size, const vpf_plane dst[3], const vpf_tensor_norm* norm);
/* The same over `n` same-shape frames; frames per dispatch as vpf_convert_resize_batch, counted with the tensor's real bytes (source +
 * 3 x width x height x element size per frame). */
VPF_API vpf_status vpf_convert_resize_tensor_batch(const vpf_exec* exec, int src_fmt, int color_space, int color_range, vpf_size src_size,
                                                   vpf_size dst_size, uint32_t n, const vpf_frame_io* frames, const vpf_tensor_norm* norm);

/*
 * Fused multi-ROI crop + bilinear resize -> normalised planar tensor: `n` rectangles of decoded NV12 / YUV420 frames (or P10 / P12 ones,
 * narrowed to 8 bits at the load: "10 / 12-bit sources" at vpf_convert_resize_tensor — a region costs the bytes it touches, not a pass over the
 * whole 16-bit frame), each resized to the ONE
 * size dst_size and normalised, in one dispatch (what a classifier / ReID / face network behind a detector consumes: float [K, 3, dh, dw]).
 * A job = (the planes of a WHOLE frame of src_size = (W, H), rect = (x, y, w, h) in luma pixels of that frame, three destination planes);
 * w, h >= 1, x + w <= W, y + h <= H, any integer x, y (odd ones too); many jobs may name the same frame.  For destination pixel (dx, dy), channel c:
 *   tx = tap(dx, (float)w / (float)dw, w), ty = tap(dy, (float)h / (float)dh, h): vpf_resize(LINEAR)'s fp32 sampling — s = (d + 0.5) * scale - 0.5
 *        clamped to [0, size - 1]; i0 = floor(s), i1 = min(i0 + 1, size - 1), f = s - i0 — on the RECTANGLE's size: taps clamp at the
 *        rectangle's edges, nothing outside the rectangle contributes;
 *   the four texels are frame pixels (x + tx.i0|i1, y + ty.i0|i1), each converted with vpf_convert's arithmetic for (src_fmt -> RGB_PLANAR,
 *        color_space, color_range) including its 8-bit rounding; chroma is taken at absolute ((x + i) >> 1, (y + j) >> 1);
 *   u8  = trunc(fma(fy, bot - top, top) + 0.5), top = fma(fx, p01 - p00, p00), bot = fma(fx, p11 - p10, p10);
 *   out = round_to_dtype(fmaf(u8, scale[c], bias[c]))              exactly vpf_convert_resize_tensor's epilogue (dtype, VPF_TENSOR_BGR, plane rules).
 * Equivalently u8 is the byte vpf_resize(RGB_PLANAR, LINEAR, (w, h) -> dst_size) writes when fed the planes of vpf_convert(frame -> RGB_PLANAR)
 * advanced by y * pitch + x; with rect = the whole frame the output is bit-identical to vpf_convert_resize_tensor.
 * `rois` is a HOST array, consumed before return; 96 jobs travel per job table, each table in at most two dispatches (jobs whose source window
 * is converted once into LDS and blended from there, and jobs with large down-scale factors that convert per tap: identical bits).
 * Unsupported format / matrix / dtype / flag: VPF_ERR_UNSUPPORTED as vpf_convert_resize_tensor.  Null pointers, n == 0, bad sizes, an empty
 * rect, a rect that leaves the frame (no silent clipping), short pitches, misaligned planes, non-finite scale / bias: VPF_ERR_BAD_ARG — all
 * checked before any device access.
 */
typedef struct vpf_rect {
  uint32_t x, y, width, height;
} vpf_rect;
typedef struct vpf_roi_io {
  vpf_plane src[3]; /* the WHOLE frame's planes */
  vpf_plane dst[3];
  vpf_rect rect;
} vpf_roi_io; /* 112 bytes, no implicit padding */
VPF_API vpf_status vpf_convert_resize_tensor_rois(const vpf_exec* exec, int src_fmt, int color_space, int color_range, vpf_size src_size,
                                                  vpf_size dst_size, uint32_t n, const vpf_roi_io* rois, const vpf_tensor_norm* norm);

/*
 * The same with the rectangles in DEVICE memory: what stands behind a detector and its NMS that run on the GPU.  No sync, no copy of the boxes to the
 * host, and a captured graph replays with the boxes and the count of REPLAY time.
 * `frames` is a HOST array of the planes of n_frames (1 .. 128) WHOLE frames of src_size = (W, H), consumed before return.  table->boxes points to
 * DEVICE memory: entry k = five int32 (frame, x, y, width, height) at byte k * box_stride (a row of a torch.int32 [K, 5] tensor: box_stride = 20;
 * any multiple of 4 from 20 up: padded tables); table->count to ONE device int32, or NULL.  The kernel reads both WHEN IT RUNS on exec->stream; the
 * host never dereferences them: the caller orders their producer before this call on that stream (or makes the stream wait for it).
 *   c = clamp(*count, 0, max_n); count == NULL: c = max_n.  max_n (1 .. 65535) is the size of the dispatch.
 *   job k < c with a VALID box — 0 <= frame < n_frames, width >= 1, height >= 1, x >= 0, y >= 0, x + width <= W, y + height <= H, evaluated without
 *        overflow for any five ints —: every element of its planes is bit for bit what vpf_convert_resize_tensor_rois writes for (frames[frame],
 *        rect = (x, y, width, height), planes dst[c].ptr + k * dst_job_stride with dst[c].pitch), for the same src_fmt (NV12, YUV420, P10, P12),
 *        dtype, VPF_TENSOR_BGR, VPF_TENSOR_NHWC (dst[0] = the one interleaved plane of job 0) and colour rules;
 *   job k < c with an INVALID box: every element of its planes takes the epilogue of byte 0, round_to_dtype(fmaf(0, scale[c], bias[c])) —
 *        vpf_convert_letterbox_tensor's default pad.  No clipping, and no byte of any frame is read;
 *   job k >= c: NOTHING is written — a call costs c regions, not max_n; those rows of a fresh tensor stay undefined.
 * Nothing outside the planes of jobs < c is ever written.  One dispatch; every workgroup decides for its own tile of 16 x 256 destination pixels
 * whether its source window is converted once into LDS or sampled per tap (identical bits; the host-table entry decides per job).
 * Checked on the host before any device access, with the ROI entry's answers: unsupported format / matrix / dtype / flag: VPF_ERR_UNSUPPORTED; null
 * pointers (exec, frames, table, table->boxes, norm), bad sizes, short source pitches, misaligned source (P10 / P12) or destination planes, non-finite
 * scale / bias, n_frames outside 1 .. 128, max_n outside 1 .. 65535, boxes or count not 4-byte aligned, box_stride < 20 or not a multiple of 4,
 * dst_job_stride not a multiple of the element size: VPF_ERR_BAD_ARG.  Whatever the boxes hold, the call returns VPF_OK.
 * Under stream capture the frame and destination pointers are baked into the graph, as in every entry; boxes and count are read at every replay.
 */
typedef struct vpf_roi_dev {
  int32_t frame, x, y, width, height;
} vpf_roi_dev; /* 20 bytes: a row of a torch.int32 [K, 5] tensor */
typedef struct vpf_frame_src {
  vpf_plane src[3]; /* the WHOLE frame's planes */
} vpf_frame_src; /* 48 bytes */
typedef struct vpf_rois_dev {
  const vpf_roi_dev* boxes; /* DEVICE memory, 4-byte aligned */
  const int32_t* count;     /* DEVICE memory, or NULL = max_n */
  uint32_t box_stride;      /* bytes between entries: >= 20, multiple of 4 */
  uint32_t max_n;           /* 1 .. 65535: grid z */
  vpf_plane dst[3];         /* planes of job 0 (one plane with VPF_TENSOR_NHWC) */
  uint64_t dst_job_stride;  /* bytes from job k's planes to job k + 1's: multiple of the element size */
} vpf_rois_dev; /* 80 bytes, no implicit padding */
VPF_API vpf_status vpf_convert_resize_tensor_rois_dev(const vpf_exec* exec, int src_fmt, int color_space, int color_range, vpf_size src_size,
                                                      vpf_size dst_size, uint32_t n_frames, const vpf_frame_src* frames, const vpf_rois_dev* table,
                                                      const vpf_tensor_norm* norm);

/*
 * Letterbox into the tensor — fused multi-ROI crop + bilinear resize with PLACEMENT and PADDING: vpf_convert_resize_tensor_rois with a destination
 * rectangle per job.  What a detector-style network takes first (resize to fit, centre, pad the rest with a constant: YOLO's 114-grey letterbox),
 * and what ReID / face / OCR crops padded to the input aspect need behind it: `n` jobs of K different aspect ratios in one dispatch.
 * A job = (the planes of a WHOLE frame of src_size = (W, H), rect = (x, y, w, h) in luma pixels of that frame — vpf_roi_io.rect's rules —, the
 * planes of the WHOLE dst_size = (dw, dh) of this job, dst_rect = (ix, iy, iw, ih) in destination pixels: where the picture goes); iw, ih >= 1,
 * ix + iw <= dw, iy + ih <= dh; different jobs may have different dst_rects.  For destination pixel (dx, dy) of the plane, channel c:
 *   inside  (ix <= dx < ix + iw && iy <= dy < iy + ih): u8[c] is the byte vpf_convert_resize_tensor_rois defines for rect -> (iw, ih) at pixel
 *        (dx - ix, dy - iy): tx = tap(dx - ix, (float)w / (float)iw, w), ty = tap(dy - iy, (float)h / (float)ih, h) on the RECTANGLE's size (taps
 *        clamp at the rectangle's edges), the four texels frame pixels (x + tx.i0|i1, y + ty.i0|i1) converted with vpf_convert's arithmetic, chroma
 *        at absolute ((x + i) >> 1, (y + j) >> 1), u8 = trunc(fma(fy, bot - top, top) + 0.5) with the same top and bot;
 *   outside: u8[c] = pad[c], unblended (pad[c] belongs to OUTPUT channel c, like scale[c], bias[c] and the warp's border[c]);
 *   out = round_to_dtype(fmaf(u8[c], scale[c], bias[c]))           exactly vpf_convert_resize_tensor's epilogue (dtype, flags, plane rules).
 * Equivalently: every plane of the job filled with the epilogue of `pad`, then vpf_convert_resize_tensor_rois(dst_size = (iw, ih)) on the job's
 * planes advanced by iy * pitch + ix * element size (3 * ix elements with VPF_TENSOR_NHWC) — bit-identical to that, without the misaligned slice and
 * without writing the picture's elements twice.  With dst_rect = (0, 0, dw, dh) the output is bit-identical to vpf_convert_resize_tensor_rois.
 * Every element of every job's dst_size planes is written exactly once, and nothing else is written.
 * It accepts what the ROI entry accepts: NV12 / YUV420 / P10 / P12 sources (16-bit samples narrowed at the load), f32 / f16 / bf16,
 * VPF_TENSOR_BGR, VPF_TENSOR_NHWC (dst[0] = the one interleaved plane of the job), the same colour rules.  `jobs` is a HOST array, consumed before
 * return; 82 jobs travel per job table, each table in at most two dispatches (jobs whose source window is converted once into LDS and blended from
 * there, and jobs with large down-scale factors that convert per tap: identical bits).  opts == NULL means pad 0 0 0.
 * Refusals are the ROI entry's, plus VPF_ERR_BAD_ARG for an empty dst_rect, a dst_rect that leaves dst_size (no silent clipping) and a non-zero
 * `reserved` — all checked before any device access.
 *
 * vpf_letterbox_fit (host only, callable without a GPU): the aspect-preserving, centred dst_rect of a w x h rectangle inside dw x dh, in integer
 * arithmetic with 64-bit products.  w * dh >= h * dw (width-limited): iw = dw, ih = clamp((2 h dw + w) / (2 w), 1, dh) (round half up); otherwise
 * ih = dh, iw = clamp((2 w dh + h) / (2 h), 1, dw); ix = (dw - iw) / 2, iy = (dh - ih) / 2, rounded down.  1920 x 1080 into 640 x 640 gives
 * (0, 140, 640, 360).  A zero size gives (0, 0, 0, 0).  Destination pixel x_dst of the picture shows frame coordinate
 * x_frame = rect.x + (x_dst - ix + 0.5) * w / iw - 0.5 (likewise y): the way back for a detector's boxes.
 */
typedef struct vpf_letterbox_io {
  vpf_plane src[3];  /* the WHOLE frame's planes */
  vpf_plane dst[3];  /* the WHOLE dst_size planes of this job (one plane with VPF_TENSOR_NHWC) */
  vpf_rect rect;     /* source rectangle, luma pixels of the frame (vpf_roi_io.rect's rules) */
  vpf_rect dst_rect; /* where the picture goes inside dst_size, destination pixels */
} vpf_letterbox_io; /* 128 bytes, no implicit padding */
typedef struct vpf_letterbox_opts {
  uint8_t pad[3];   /* per output channel */
  uint8_t reserved; /* must be 0 */
} vpf_letterbox_opts; /* 4 bytes */
VPF_API vpf_status vpf_convert_letterbox_tensor(const vpf_exec* exec, int src_fmt, int color_space, int color_range, vpf_size src_size,
                                                vpf_size dst_size, uint32_t n, const vpf_letterbox_io* jobs, const vpf_tensor_norm* norm,
                                                const vpf_letterbox_opts* opts);
VPF_API vpf_rect vpf_letterbox_fit(vpf_size src, vpf_size dst); /* host only */

/*
 * The same with the boxes in DEVICE memory: the padded ReID / face / OCR crops behind a detector and its NMS that run on the GPU.  No sync, no copy of
 * the boxes to the host, and a captured graph replays with the boxes, placements and count of REPLAY time.  Where vpf_convert_resize_tensor_rois_dev
 * stretches every box to dst_size, this entry keeps its aspect: the kernel fits the box into the plane itself, because only the kernel sees the box.
 * `frames` is a HOST array of the planes of n_frames (1 .. 128) WHOLE frames of src_size = (W, H) (vpf_frame_src), consumed before return.
 * table->boxes points to DEVICE memory: entry k = five int32 (frame, x, y, width, height) at byte k * box_stride (vpf_roi_dev: a row of a torch.int32
 * [K, 5] tensor; any multiple of 4 from 20 up); table->dst_rects to job k's placement, four int32 (ix, iy, iw, ih) at byte k * rect_stride (a row of a
 * torch.int32 [K, 4] tensor: 16; any multiple of 4 from 16 up), or NULL: the kernel fits; table->count to ONE device int32, or NULL.  The kernel reads
 * all three WHEN IT RUNS on exec->stream; the host never dereferences them: the caller orders their producer before this call on that stream.
 *   c = clamp(*count, 0, max_n); count == NULL: c = max_n.  max_n (1 .. 65535) is the size of the dispatch.
 *   job k < c, VALID — the box passes vpf_convert_resize_tensor_rois_dev's test, and with dst_rects also iw >= 1, ih >= 1, ix >= 0, iy >= 0,
 *        ix + iw <= dw, iy + ih <= dh, evaluated without overflow for any four ints —: every element of the job's WHOLE dst_size planes (dst[c].ptr +
 *        k * dst_job_stride with dst[c].pitch) is bit for bit what vpf_convert_letterbox_tensor writes for (frames[frame], rect = (x, y, width,
 *        height), dst_rect), where dst_rect = vpf_letterbox_fit((width, height), dst_size) when dst_rects == NULL and the row's four ints otherwise;
 *        for the same src_fmt (NV12, YUV420, P10, P12), dtype, VPF_TENSOR_BGR, VPF_TENSOR_NHWC (dst[0] = the one interleaved plane of job 0), pad and
 *        colour rules;
 *   job k < c, INVALID (the box or the placement): every element of its planes takes the epilogue of pad[c], round_to_dtype(fmaf(pad[c], scale[c],
 *        bias[c])) (0 0 0 when opts == NULL) — what a letterbox job leaves where there is no picture.  No byte of any frame is read;
 *   job k >= c: NOTHING is written, and neither its box nor its placement is read — the tables may be shorter than max_n.
 * Every element of every job < c is written exactly once, and nothing else is written.  One dispatch over (16 x 256 tiles of the destination plane,
 * max_n); every workgroup decides for its own tile whether it is pad, or its source window is converted once into LDS or sampled per tap (identical
 * bits; the host-table entry decides per job).
 * Checked on the host before any device access, with vpf_convert_resize_tensor_rois_dev's list and answers, plus VPF_ERR_BAD_ARG for dst_rects not
 * 4-byte aligned, rect_stride < 16 or not a multiple of 4 (with dst_rects), and a non-zero `reserved`, here or in opts.  Whatever the device tables
 * hold, the call returns VPF_OK.  Under stream capture the frame and destination pointers are baked into the graph, as in every entry; boxes,
 * placements and count are read at every replay.
 */
typedef struct vpf_letterbox_dev {
  const vpf_roi_dev* boxes; /* DEVICE: (frame, x, y, width, height), entry k at byte k * box_stride */
  const int32_t* dst_rects; /* DEVICE: (ix, iy, iw, ih) of job k at byte k * rect_stride, or NULL = fit in the kernel */
  const int32_t* count;     /* DEVICE: one int32, or NULL = max_n */
  uint32_t box_stride;      /* >= 20, multiple of 4 */
  uint32_t rect_stride;     /* >= 16, multiple of 4; ignored when dst_rects == NULL */
  uint32_t max_n;           /* 1 .. 65535: grid z */
  uint32_t reserved;        /* must be 0 */
  vpf_plane dst[3];         /* WHOLE dst_size planes of job 0 (one plane with VPF_TENSOR_NHWC) */
  uint64_t dst_job_stride;  /* bytes from job k's planes to job k + 1's: multiple of the element size */
} vpf_letterbox_dev; /* 96 bytes, no implicit padding */
VPF_API vpf_status vpf_convert_letterbox_tensor_dev(const vpf_exec* exec, int src_fmt, int color_space, int color_range, vpf_size src_size,
                                                    vpf_size dst_size, uint32_t n_frames, const vpf_frame_src* frames, const vpf_letterbox_dev* table,
                                                    const vpf_tensor_norm* norm, const vpf_letterbox_opts* opts);

/*
 * Fused multi-ROI affine warp -> normalised planar tensor: `n` crops of decoded NV12 / YUV420 frames (or P10 / P12 ones, narrowed to 8 bits at the
 * load: "10 / 12-bit sources" at vpf_convert_resize_tensor) that are NOT axis-aligned (aligned faces, rotated
 * text boxes, oriented detections, flips, shears), each sampled through a 2 x 3 matrix of its own into the ONE size dst_size and normalised, in
 * one dispatch: float [K, 3, dh, dw].  A job = (the planes of a WHOLE frame of src_size = (W, H), m[6] = (m00 m01 m02; m10 m11 m12), three
 * destination planes).  The matrix is the INVERSE map: it takes a destination pixel to source coordinates in luma pixels of that frame; coordinates
 * are pixel indices, the convention of vpf_remap's maps.  For destination pixel (dx, dy), channel c — every operation a separately rounded fp32
 * operation in this order, no fma:
 *   sx = (m00 * (float)dx + m01 * (float)dy) + m02,  sy = (m10 * (float)dx + m11 * (float)dy) + m12;
 *   VPF_WARP_CONSTANT: the pixel is in range when sx >= 0 && sx <= (float)(W - 1) && sy >= 0 && sy <= (float)(H - 1) (vpf_remap's test: -0.0 is in
 *        range); a pixel out of range takes u8[c] = border[c], unblended (border[c] belongs to OUTPUT channel c, like scale[c] and bias[c]);
 *   VPF_WARP_REPLICATE: sx = min(max(sx, 0), W - 1), sy = min(max(sy, 0), H - 1) first, so every pixel is in range;
 *   in range: x0 = (int)sx, x1 = min(x0 + 1, W - 1), fx = sx - (float)x0, likewise y (vpf_remap's sampling); the four texels are frame pixels
 *        (x0|x1, y0|y1), each converted with vpf_convert's arithmetic for (src_fmt -> RGB_PLANAR, color_space, color_range) including its 8-bit
 *        rounding, chroma taken at (x >> 1, y >> 1);
 *   u8  = trunc(fma(fy, bot - top, top) + 0.5), top = fma(fx, p01 - p00, p00), bot = fma(fx, p11 - p10, p10);
 *   out = round_to_dtype(fmaf(u8, scale[c], bias[c]))              exactly vpf_convert_resize_tensor's epilogue (dtype, VPF_TENSOR_BGR, plane rules).
 * Equivalently u8 is the byte vpf_remap(RGB) writes when its source is vpf_convert(frame -> RGB), its maps hold the sx, sy above and its
 * destination was pre-filled with `border`.  Resize and remap use different coordinate conventions: a caller who wants vpf_resize's sampling of
 * a rectangle (x, y, w, h) folds it into the matrix (m00 = s, m02 = 0.5 s - 0.5 + x with s = w / dw); bit-equality with
 * vpf_convert_resize_tensor_rois is not promised for such matrices.  A job whose footprint lies wholly outside the frame is legal: it writes the
 * border (the edge pixels under REPLICATE).
 * `jobs` is a HOST array, consumed before return; 96 jobs travel per job table, each table in at most two dispatches (jobs whose tiles' source
 * windows are converted once into LDS and blended from there, and jobs that convert per tap — down-scales: identical bits).
 * opts == NULL means VPF_WARP_CONSTANT with border 0 0 0.  Unsupported format / matrix / dtype / flag as vpf_convert_resize_tensor, or an unknown
 * border mode: VPF_ERR_UNSUPPORTED.  Null pointers, n == 0, bad sizes, short pitches, misaligned planes, non-finite scale / bias, non-zero
 * reserved fields, a matrix coefficient that is not finite or exceeds 2^24 in magnitude (so sx, sy stay finite and no NaN arises):
 * VPF_ERR_BAD_ARG — all checked before any device access.
 */
#define VPF_WARP_CONSTANT 0u
#define VPF_WARP_REPLICATE 1u
typedef struct vpf_warp_io {
  vpf_plane src[3]; /* the WHOLE frame's planes */
  vpf_plane dst[3];
  float m[6]; /* m00 m01 m02 m10 m11 m12: destination pixel -> source coordinates */
} vpf_warp_io; /* 120 bytes, no implicit padding */
typedef struct vpf_warp_opts {
  uint32_t border_mode; /* VPF_WARP_* */
  uint8_t border[3];    /* per output channel, VPF_WARP_CONSTANT */
  uint8_t reserved;     /* must be 0 */
} vpf_warp_opts; /* 8 bytes */
VPF_API vpf_status vpf_convert_warp_tensor(const vpf_exec* exec, int src_fmt, int color_space, int color_range, vpf_size src_size, vpf_size dst_size,
                                           uint32_t n, const vpf_warp_io* jobs, const vpf_tensor_norm* norm, const vpf_warp_opts* opts);

/*
 * The same with the matrices in DEVICE memory: what stands behind a landmark network (face alignment) or an oriented-box head that runs on the GPU.
 * No sync, no copy of the matrices to the host, and a captured graph replays with the matrices, frame indices and count of REPLAY time.
 * `frames` is a HOST array of the planes of n_frames (1 .. 128) WHOLE frames of src_size = (W, H) (vpf_frame_src), consumed before return.
 * table->matrices points to DEVICE memory: job k = six floats m00 m01 m02 m10 m11 m12 at byte k * matrix_stride (a row of a float32 [K, 2, 3] or
 * [K, 6] tensor: matrix_stride = 24; any multiple of 4 from 24 up: padded tables); table->frame_index to job k's frame, one int32 at byte
 * k * frame_stride (a multiple of 4 from 4 up), or NULL: every job samples frames[0]; table->count to ONE device int32, or NULL.  The kernel reads
 * all three WHEN IT RUNS on exec->stream; the host never dereferences them: the caller orders their producer before this call on that stream (or
 * makes the stream wait for it).
 *   c = clamp(*count, 0, max_n); count == NULL: c = max_n.  max_n (1 .. 65535) is the size of the dispatch.
 *   job k < c with a VALID entry — 0 <= frame < n_frames and fabsf(m) <= 2^24 for each of the six coefficients (vpf_convert_warp_tensor's rule: NaN
 *        and the infinities fail it) —: every element of its planes is bit for bit what vpf_convert_warp_tensor writes for (frames[frame], m, planes
 *        dst[c].ptr + k * dst_job_stride with dst[c].pitch), for the same src_fmt (NV12, YUV420, P10, P12), dtype, VPF_TENSOR_BGR, VPF_TENSOR_NHWC
 *        (dst[0] = the one interleaved plane of job 0), border mode, border and colour rules;
 *   job k < c with an INVALID entry: every element of its planes takes the epilogue of border[c], round_to_dtype(fmaf(border[c], scale[c], bias[c]))
 *        (0 0 0 when opts == NULL) — in BOTH border modes: what a valid job wholly outside the frame writes under VPF_WARP_CONSTANT.  No byte of
 *        any frame is read;
 *   job k >= c: NOTHING is written, and neither its matrix nor its frame index is read — the tables may be shorter than max_n.
 * Nothing outside the planes of jobs < c is ever written.  One dispatch over (32 x 32 destination tiles, max_n); every workgroup decides for its own
 * tile whether its source window is converted once into LDS or sampled per tap (identical bits).
 * max_step is the LDS hint.  The host cannot see the matrices, so the caller bounds them: max_step >= |m00| + |m01| and >= |m10| + |m11|, the source
 * pixels per destination pixel step (a crop rotated by 45 degrees at scale s: sqrt(2) s).  The dispatch takes the LDS that covers every tile of every
 * such matrix with |m02| <= W, |m12| <= H, at most 64 KiB; max_step == 0: no hint, 64 KiB.  The hint is never a correctness input: a tile whose window
 * outgrows the LDS it was given is sampled per tap, with identical bits — a wrong hint costs time, not pixels.
 * Checked on the host before any device access, with the warp entry's answers: unsupported format / matrix / dtype / flag / border mode:
 * VPF_ERR_UNSUPPORTED; null pointers (exec, frames, table, table->matrices, norm), bad sizes, short source pitches, misaligned source (P10 / P12) or
 * destination planes, non-finite scale / bias, non-zero reserved fields, n_frames outside 1 .. 128, max_n outside 1 .. 65535, matrices, frame_index or
 * count not 4-byte aligned, matrix_stride < 24 or not a multiple of 4, frame_stride < 4 or not a multiple of 4 (with a frame_index), dst_job_stride
 * not a multiple of the element size, max_step negative or not finite: VPF_ERR_BAD_ARG.  Whatever the device tables hold, the call returns VPF_OK.
 * Under stream capture the frame and destination pointers are baked into the graph, as in every entry; matrices, frame indices and count are read at
 * every replay.
 */
typedef struct vpf_warps_dev {
  const float* matrices;      /* DEVICE: job k = six floats m00 m01 m02 m10 m11 m12 at byte k * matrix_stride */
  const int32_t* frame_index; /* DEVICE: job k's frame at byte k * frame_stride; NULL = every job samples frames[0] */
  const int32_t* count;       /* DEVICE: one int32, or NULL = max_n */
  uint32_t matrix_stride;     /* >= 24, multiple of 4 (a row of a float32 [K, 2, 3] / [K, 6] tensor: 24) */
  uint32_t frame_stride;      /* >= 4, multiple of 4; ignored when frame_index == NULL */
  uint32_t max_n;             /* 1 .. 65535: grid z */
  float max_step;             /* LDS hint, see above; 0 = none */
  vpf_plane dst[3];           /* planes of job 0 (one plane with VPF_TENSOR_NHWC) */
  uint64_t dst_job_stride;    /* bytes from job k's planes to job k + 1's: multiple of the element size */
} vpf_warps_dev; /* 96 bytes, no implicit padding */
VPF_API vpf_status vpf_convert_warp_tensor_dev(const vpf_exec* exec, int src_fmt, int color_space, int color_range, vpf_size src_size, vpf_size dst_size,
                                               uint32_t n_frames, const vpf_frame_src* frames, const vpf_warps_dev* table, const vpf_tensor_norm* norm,
                                               const vpf_warp_opts* opts);

/*
 * Fused multi-ROI perspective warp (3 x 3 homography) -> normalised tensor: vpf_convert_warp_tensor for crops seen at an angle — a document, plate,
 * sign or screen rectified from its four corners, a bird's-eye view from a calibrated camera, ground-plane registration.  A job = (the planes of a
 * WHOLE frame of src_size = (W, H), m[9] = (m00 m01 m02; m10 m11 m12; m20 m21 m22), the destination planes).  The matrix is the INVERSE map:
 * destination pixel -> source luma pixel indices, vpf_remap's convention.  For destination pixel (dx, dy) — every operation a separately rounded
 * fp32 operation in this order, no fma, the division IEEE round-to-nearest, denormals kept:
 *   nx = (m00 * (float)dx + m01 * (float)dy) + m02,  ny = (m10 * (float)dx + m11 * (float)dy) + m12,  w = (m20 * (float)dx + m21 * (float)dy) + m22;
 *   !(w > 0): the pixel takes u8[c] = border[c], unblended, in BOTH border modes (it lies behind the plane or on the horizon);
 *   else sx = nx / w, sy = ny / w, then exactly vpf_convert_warp_tensor from its range test on: VPF_WARP_CONSTANT's range test (-0.0 in range, +inf
 *        out of range), VPF_WARP_REPLICATE's max-then-min, the sampling with chroma at (x >> 1, y >> 1), the blend, the truncation, the epilogue,
 *        dtype, VPF_TENSOR_BGR, VPF_TENSOR_NHWC, the narrowing of P10 / P12.
 * With w > 0 and finite coefficients neither 0 / 0 nor inf / inf arises: no NaN exists.  sx = +-inf is legal: the border under CONSTANT, the edge
 * under REPLICATE.  With the last row (0, 0, 1) w is exactly 1 and every element is bit for bit what vpf_convert_warp_tensor writes for the first
 * six coefficients.  Equivalently u8 is the byte vpf_remap(RGB) writes when its source is vpf_convert(frame -> RGB), its maps hold the sx, sy above
 * with the !(w > 0) pixels set out of range (CONSTANT) or overwritten with the border afterwards (REPLICATE), and its destination was pre-filled
 * with `border`.  A matrix whose w is <= 0 everywhere, the zero last row included, is legal and writes the border.
 * `jobs` is a HOST array, consumed before return; 82 jobs travel per job table, each table in at most two dispatches (jobs whose tiles may convert
 * their source windows once into LDS, and jobs that convert per tap: identical bits).  opts as in vpf_convert_warp_tensor.
 * Unsupported format / matrix / dtype / flag or an unknown border mode: VPF_ERR_UNSUPPORTED.  Null pointers, n == 0, bad sizes, short pitches,
 * misaligned planes, non-finite scale / bias, non-zero reserved fields (the job's included), one of the nine coefficients not finite or above 2^24
 * in magnitude: VPF_ERR_BAD_ARG — all checked before any device access.
 */
typedef struct vpf_persp_io {
  vpf_plane src[3]; /* the WHOLE frame's planes */
  vpf_plane dst[3];
  float m[9];        /* m00 m01 m02 m10 m11 m12 m20 m21 m22: destination pixel -> homogeneous source coordinates */
  uint32_t reserved; /* must be 0 */
} vpf_persp_io; /* 136 bytes, no implicit padding */
VPF_API vpf_status vpf_convert_persp_tensor(const vpf_exec* exec, int src_fmt, int color_space, int color_range, vpf_size src_size, vpf_size dst_size,
                                            uint32_t n, const vpf_persp_io* jobs, const vpf_tensor_norm* norm, const vpf_warp_opts* opts);

/*
 * The same with the homographies in DEVICE memory: what stands behind a corner-regression network (four corners per document, plate or screen) whose
 * 3 x 3 matrices are solved on the GPU.  The contract is vpf_convert_warp_tensor_dev's, word for word, with nine coefficients: no sync, no copy of
 * the matrices to the host, and a captured graph replays with the matrices, frame indices and count of REPLAY time.
 * `frames` is a HOST array of the planes of n_frames (1 .. 128) WHOLE frames of src_size = (W, H), consumed before return.  table->matrices points
 * to DEVICE memory: job k = nine floats m00 m01 m02 m10 m11 m12 m20 m21 m22 at byte k * matrix_stride (a row of a float32 [K, 3, 3] or [K, 9]
 * tensor: 36; any multiple of 4 from 36 up: padded tables); table->frame_index to job k's frame, one int32 at byte k * frame_stride (a multiple of 4
 * from 4 up), or NULL: every job samples frames[0]; table->count to ONE device int32, or NULL.  The kernel reads all three WHEN IT RUNS on
 * exec->stream; the host never dereferences them.
 *   c = clamp(*count, 0, max_n); count == NULL: c = max_n.  max_n (1 .. 65535) is the size of the dispatch.
 *   job k < c with a VALID entry — 0 <= frame < n_frames and fabsf(m) <= 2^24 for each of the nine coefficients (NaN and the infinities fail it) —:
 *        every element of its planes is bit for bit what vpf_convert_persp_tensor writes for (frames[frame], m, planes dst[c].ptr + k * dst_job_stride
 *        with dst[c].pitch), for the same src_fmt (NV12, YUV420, P10, P12), dtype, VPF_TENSOR_BGR, VPF_TENSOR_NHWC, border mode, border and colour
 *        rules.  A valid matrix whose w is <= 0 everywhere is legal and writes the border, as there;
 *   job k < c with an INVALID entry: every element of its planes is round_to_dtype(fmaf(border[c], scale[c], bias[c])) (border 0 0 0 when
 *        opts == NULL), in BOTH border modes.  No byte of any frame is read;
 *   job k >= c: NOTHING is written, and neither its matrix nor its frame index is read — the tables may be shorter than max_n.
 * Nothing outside the planes of jobs < c is ever written.  One dispatch over (32 x 32 destination tiles, max_n); every workgroup decides for its own
 * tile whether it is the border, sampled per tap or converted once into LDS (identical bits).
 * max_step is the LDS hint, the affine entry's generalised: a bound, over every valid job and every destination pixel, on
 * |d sx / d dx| + |d sx / d dy| and on |d sy / d dx| + |d sy / d dy|, the source pixels per destination pixel step (a last row (0, 0, 1):
 * |m00| + |m01| and |m10| + |m11|).  vpf_persp_max_step returns that bound for ONE host matrix and destination size, or 0 where it has none (some
 * destination corner with w <= 0): a caller calibrates offline, on matrices of the kind the pipeline produces, and passes the maximum.  The dispatch
 * takes the LDS of a window of max_step * 31 + 5 pixels per axis (and a rounding slack), cut to the frame, at most 64 KiB; max_step == 0: no hint,
 * 64 KiB.  Never a correctness input: a tile whose window outgrows the LDS it was given is sampled per tap, with identical bits.
 * Checked on the host before any device access, with vpf_convert_warp_tensor_dev's list and answers (matrix_stride < 36 in place of < 24).  Whatever
 * the device tables hold, the call returns VPF_OK.
 */
typedef struct vpf_persps_dev {
  const float* matrices;      /* DEVICE: job k = nine floats m00 .. m22 at byte k * matrix_stride */
  const int32_t* frame_index; /* DEVICE: job k's frame at byte k * frame_stride; NULL = every job samples frames[0] */
  const int32_t* count;       /* DEVICE: one int32, or NULL = max_n */
  uint32_t matrix_stride;     /* >= 36, multiple of 4 (a row of a float32 [K, 3, 3] / [K, 9] tensor: 36) */
  uint32_t frame_stride;      /* >= 4, multiple of 4; ignored when frame_index == NULL */
  uint32_t max_n;             /* 1 .. 65535: grid z */
  float max_step;             /* LDS hint, see above; 0 = none */
  vpf_plane dst[3];           /* planes of job 0 (one plane with VPF_TENSOR_NHWC) */
  uint64_t dst_job_stride;    /* bytes from job k's planes to job k + 1's: multiple of the element size */
} vpf_persps_dev; /* 96 bytes, no implicit padding: the layout of vpf_warps_dev */
VPF_API vpf_status vpf_convert_persp_tensor_dev(const vpf_exec* exec, int src_fmt, int color_space, int color_range, vpf_size src_size, vpf_size dst_size,
                                                uint32_t n_frames, const vpf_frame_src* frames, const vpf_persps_dev* table, const vpf_tensor_norm* norm,
                                                const vpf_warp_opts* opts);
VPF_API float vpf_persp_max_step(const float m[9], vpf_size dst); /* host only; 0: no bound (also for a null, non-finite or oversized input) */

/*
 * Fused per-pixel remap -> normalised tensor: vpf_convert_warp_tensor for geometry no matrix describes — lens undistortion, fisheye and
 * surround-view rigs, rectification, flow-driven warps, stabilisation.  One pass instead of vpf_convert(-> RGB), vpf_remap and a normalise chain.
 * The call takes `n` jobs.  A job = (the planes of a WHOLE frame of src_size = (W, H), its destination planes, a pair of maps of dst_size).  Many
 * jobs may name the same frame or the same maps: one camera with a batch of frames shares its maps, a rig gives every camera its own.
 * For destination pixel (dx, dy):
 *   sx = xmap[dy][dx], sy = ymap[dy][dx], both fp32, used as loaded (row dy of a map at (char*)map + dy * pitch, dst_size.width floats);
 *   sx or sy NaN: the pixel takes u8[c] = border[c], unblended, in BOTH border modes (the perspective entry's !(w > 0) rule; calibration tools
 *        mark invalid pixels this way);
 *   else exactly vpf_convert_warp_tensor from its range test on: VPF_WARP_CONSTANT's test (-0.0 is in range, +-inf out of range),
 *        VPF_WARP_REPLICATE's max-then-min (+-inf goes to the edge), the sampling x0 = (int)sx, x1 = min(x0 + 1, W - 1), fx = sx - (float)x0,
 *        every texel converted with vpf_convert's arithmetic and chroma read at (x >> 1, y >> 1), u8 = trunc(fma(fy, bot - top, top) + 0.5), the
 *        epilogue, dtype, VPF_TENSOR_BGR, VPF_TENSOR_NHWC and the narrowing of P10 / P12.
 * Equivalently u8 is the byte vpf_remap(RGB) writes when its source is vpf_convert(frame -> RGB), its maps are these maps — clamped first under
 * REPLICATE, NaN staying NaN — and its destination was pre-filled with `border`.  On maps written as sx = (m00 dx + m01 dy) + m02 (sy likewise)
 * the output is bit for bit vpf_convert_warp_tensor's for that matrix.  Every element of every job's planes is written exactly once, nothing
 * else is written (vpf_remap leaves out-of-range pixels untouched; a fresh tensor has nothing to keep, hence the border).
 * The maps are DEVICE data: the kernel reads them when it runs on exec->stream, the host never dereferences them, and under stream capture they
 * are read at every replay (a flow field rewritten between replays is legal).  Whatever the maps hold, the call returns VPF_OK and no byte
 * outside a frame is read: the kernel makes every coordinate safe before it becomes an index (csrc/k_convert_remap.hip).
 * `jobs` is a HOST array, consumed before return; 96 jobs travel per job table, one dispatch per table over (32 x 32 destination tiles, jobs):
 * every workgroup merges the taps of its tile's in-range pixels into the tile's exact source window and decides for itself — the border, the
 * window converted once into LDS, or four conversions per pixel (identical bits).
 * max_step is vpf_convert_warp_tensor_dev's LDS hint: a bound on the source pixels per destination pixel step of the maps,
 * |d sx / d dx| + |d sx / d dy| and the same for sy.  The dispatch takes the LDS that covers every tile of such maps, at most 64 KiB;
 * max_step == 0: no hint, 64 KiB.  Never a correctness input: a tile whose window outgrows the LDS it was given is sampled per tap, with
 * identical bits.
 * opts == NULL means VPF_WARP_CONSTANT with border 0 0 0 and no hint.  Checked on the host before any device access, with the warp entry's list
 * and answers: unsupported format / matrix / dtype / flag / border mode: VPF_ERR_UNSUPPORTED; null pointers, n == 0, bad sizes, short pitches,
 * misaligned planes, non-finite scale / bias, non-zero reserved fields (the planes', opts->reserved, opts->reserved2), a null xmap / ymap, a map
 * pointer or pitch that is not a multiple of 4, a map pitch below 4 * dst_size.width, a max_step that is negative or not finite: VPF_ERR_BAD_ARG.
 */
typedef struct vpf_remap_io {
  vpf_plane src[3];     /* the WHOLE frame's planes (NV12, YUV420, P10, P12) */
  vpf_plane dst[3];     /* three planes; one interleaved plane with VPF_TENSOR_NHWC */
  const float* xmap;    /* DEVICE: row dy at (char*)xmap + dy * xmap_pitch, dst_size.width floats */
  const float* ymap;    /* DEVICE, likewise */
  uint32_t xmap_pitch, ymap_pitch; /* bytes */
} vpf_remap_io;         /* 120 bytes, no implicit padding */
typedef struct vpf_remap_opts {
  uint32_t border_mode; /* VPF_WARP_CONSTANT | VPF_WARP_REPLICATE */
  uint8_t border[3];    /* per OUTPUT channel */
  uint8_t reserved;     /* 0 */
  float max_step;       /* LDS hint, 0 = none */
  uint32_t reserved2;   /* 0 */
} vpf_remap_opts;       /* 16 bytes */
VPF_API vpf_status vpf_convert_remap_tensor(const vpf_exec* exec, int src_fmt, int color_space, int color_range, vpf_size src_size, vpf_size dst_size,
                                            uint32_t n, const vpf_remap_io* jobs, const vpf_tensor_norm* norm, const vpf_remap_opts* opts);

/*
 * ANTIALIASED letterbox into the tensor: vpf_convert_letterbox_tensor's jobs, options, plane rules and refusals, unchanged, with the bare bilinear
 * pair replaced by the TRIANGLE filter whose support grows with the scale — the filter of PIL's Image.resize(BILINEAR) and of torch's
 * F.interpolate(mode="bilinear", antialias=True), what training pipelines resize with.  Past a 2 x down-scale the bilinear pair skips source pixels
 * (4K -> 640 x 640 is 6 x: two of every six per axis reach the output); here every source pixel of the rectangle contributes.  With dst_rect =
 * the whole destination a job is an antialiased ROI, with rect = the whole frame as well the antialiased whole-frame call.
 * A job has the source rectangle (x, y, w, h) and the picture (ix, iy, iw, ih).  Per axis, in = w or h and out = iw or ih; every operation below
 * is an individually rounded fp32 operation, the three divisions IEEE-rounded:
 *   s = (float)in / (float)out        fs = max(s, 1.0f)       inv = 1.0f / fs
 *   for destination index d of the picture:
 *     c  = ((float)d + 0.5f) * s
 *     lo = max(0,  (int)((c - fs) + 0.5f))          (C truncation, then the clamp)
 *     hi = min(in, (int)((c + fs) + 0.5f))          taps k = lo .. hi-1
 *     t_k = max(0.0f, 1.0f - fabsf(((float)k + 0.5f) - c) * inv)       (multiply and subtract rounded separately)
 *     S = t_lo + ... + t_(hi-1)  (plain adds, ascending)               r = 1.0f / S
 * hi > lo and S >= 0.5 always hold: the pixel nearest c has t >= 0.5.  P[ch](i, j) is the byte vpf_convert(src_fmt -> RGB_PLANAR, color_space,
 * color_range) gives frame pixel (x + i, y + j), as a float; chroma at absolute ((x + i) >> 1, (y + j) >> 1), as in the ROI entry.  Nothing
 * outside the rectangle contributes.  Horizontal first, then vertical, with no rounding to a byte in between (as torch's float path):
 *   H(j, dx)[ch]  = r_x(dx) * fold_k fmaf(tx_k, P[ch](lo_x + k, j), acc)         acc from 0.0f, k ascending
 *   V(dx, dy)[ch] = r_y(dy) * fold_j fmaf(ty_j, H(lo_y + j, dx)[ch], acc)        acc from 0.0f, j ascending
 *   u8  = min(255.0f, truncf(V + 0.5f))
 *   out = round_to_dtype(fmaf(u8, scale[c], bias[c]))                            exactly vpf_convert_resize_tensor's epilogue
 * Outside the picture an element takes pad[c] and the epilogue.  Every element of every job's dst_size planes is written exactly once, and nothing
 * else is written.  On an axis with s <= 1 the window is the two or three nearest pixels: the result is within 1 LSB of
 * vpf_convert_letterbox_tensor there, and is NOT claimed bit-identical to it.  The bytes are within 1 LSB of the plain float64 triangle filter
 * (weights normalised by their sum, rounded half up) everywhere, and of torch's float path rounded half up for pictures wider and taller than one
 * pixel (torch itself leaves the filter on a picture one pixel wide whose height is resampled), equal in all but a fraction of a percent; against
 * PIL's and torch's uint8 paths, which round to bytes between the passes, within 1 LSB on the measured shapes (shares: DESIGN.md 4.26).
 * It accepts NV12 / YUV420 / P10 / P12 sources (16-bit samples narrowed at the load), f32 / f16 / bf16, VPF_TENSOR_BGR, VPF_TENSOR_NHWC.  `jobs` is
 * a HOST array, consumed before return; 82 jobs travel per job table, each table in at most two dispatches (jobs whose tiles convert their source
 * window once into LDS and fold from there, and jobs beyond about 6.8 x that convert per tap: identical bits).  opts == NULL means pad 0 0 0.
 */
VPF_API vpf_status vpf_convert_letterbox_tensor_aa(const vpf_exec* exec, int src_fmt, int color_space, int color_range, vpf_size src_size,
                                                   vpf_size dst_size, uint32_t n, const vpf_letterbox_io* jobs, const vpf_tensor_norm* norm,
                                                   const vpf_letterbox_opts* opts);

/*
 * Fused planar float tensor -> NV12 / YUV420 in one pass: the way back from a model's output ([N, 3, H, W] f32 / f16 / bf16) to what an
 * encoder takes.  src[0..2] are the three planes of the frame in input channel order (R G B, or B G R with VPF_TENSOR_BGR; scale[c] / bias[c]
 * belong to input plane c), size.width elements per row, `pitch` in bytes; dst is NV12 ([0], [1]) or YUV420 ([0..2]).
 * For every element x of plane c, widened exactly to fp32 when f16 / bf16:
 *   v  = x * scale[c] + bias[c]            two separately rounded fp32 operations (a multiply, then an add: not an fma)
 *   q  = fminf(fmaxf(v, 0), 255)           IEEE maxNum / minNum: NaN -> 0, -inf -> 0, +inf -> 255
 *   u8 = (uint8) rint(q)                   round to nearest, ties to even
 * and the destination bytes are exactly those of vpf_convert(RGB_PLANAR -> YUV420, BT_601, color_range) on the three u8 planes, followed by
 * vpf_convert(YUV420 -> NV12) for NV12 (chroma = the matrix rows applied to the mean of each 2x2 quad, edge quads replicated on odd sizes,
 * NV12 chroma rows of 2 ceil(width / 2) bytes).  To undo torchvision's normalize(mean, std) of [0, 1] pixels: scale = 255 std, bias = 255 mean.
 * Colour models: what vpf_convert(RGB_PLANAR, YUV420) accepts (BT.601, MPEG or JPEG range); anything else, a destination other than NV12 /
 * YUV420, an unknown dtype or flag bit: VPF_ERR_UNSUPPORTED.  A null pointer, a non-finite scale / bias, a source pointer or pitch that is not
 * a multiple of the element size, or pitch < width x element size: VPF_ERR_BAD_ARG.  Destinations: as vpf_convert (any alignment).
 */
VPF_API int vpf_tensor_convert_supported(int dst_fmt, int color_space, int color_range); /* host only */
VPF_API vpf_status vpf_tensor_convert(const vpf_exec* exec, int dst_fmt, int color_space, int color_range, vpf_size size,
                                      const vpf_plane src[3], const vpf_plane dst[3], const vpf_tensor_norm* denorm);
/* The same over `n` same-shape frames (frames[i].src = the tensor planes, frames[i].dst = the picture), 32 frames per dispatch. */
VPF_API vpf_status vpf_tensor_convert_batch(const vpf_exec* exec, int dst_fmt, int color_space, int color_range, vpf_size size,
                                            uint32_t n, const vpf_frame_io* frames, const vpf_tensor_norm* denorm);

VPF_API const char* vpf_status_string(int status);
VPF_API const char* vpf_version(void);
/* hipGetDeviceCount; 0 when no GPU / no driver (never fails). Replaces GetNumGpus
 * (src/PyNvCodec/src/PyNvCodec.cpp:427-429). */
VPF_API int vpf_device_count(void);

/* Tracing (additive): with VPF_HIP_ROCTX=1 in the environment every entry point above runs inside a roctx range of its own name
 * and every kernel selection leaves a roctx marker, visible in `rocprofv3 --marker-trace`; VPF_HIP_LOG=2 prints the selected kernel
 * of every launch on stderr (=1: errors only).  Both replace the reference's compile-time NvtxMark (src/TC/inc/Tasks.hpp:27-52).
 * vpf_trace_push / vpf_trace_pop let a caller (the Task layer) open ranges of its own through the same switch. */
VPF_API int vpf_trace_push(const char* name);
VPF_API void vpf_trace_pop(int opened);

/* Tuning hook used by tests / benchmarks to select a kernel family (process-wide; 0 = default policy).  A hint, never a
 * correctness switch: every accepted value produces identical pixels and silently falls back where it does not apply.
 *   0        default policy (fastest applicable kernel per call)
 *   9        the any-size / any-alignment generic kernels everywhere (byte accesses, gather resize / remap)
 *   40       the narrower fast paths instead of the 16-px "r16" / tiled / quad kernels (A/B runs, test coverage)
 *   43       resize: the tiled separable kernel for bilinear down-scales as well (default: up-scales only)
 *   48       fused convert + resize: the workgroup-shared strip also beyond ~2x down-scales, where the policy takes the per-tap kernel
 *   49       fused convert + resize: the per-tap kernel's row-band form (four rows per wave) at every general factor and launch size
 *            (policy: beyond ~2x, on launches of >= 2048 workgroups)
 *   4, 8, 12, 30, 37, 44, 45, 46   one named NV12 / YUV420 -> RGB kernel of the default policy's set (csrc/vpf_convert_plan.h plan_420)
 * Any other value is rejected: -1 is returned and nothing changes.  This library holds the kernels some policy path can select, nothing
 * else: the experimental kernels and bandwidth probes of round 1 live in tools/lab/libvpfhip_lab.so, and the kernel FORMS that were
 * measured and lost — the fused kernel's per-wave strips (variant 47), the two-role Lanczos form (VPF_TUNE_RESIZE_MFMA | 0x20000), the
 * persistent launch of the band kernels (VPF_TUNE_RESIZE_BAND | 0x10000 [| 0x40000 | 0x80000]) — in tools/lab/libvpfhip_forms.so, a build of
 * these same sources with -DVPF_LAB_FORMS that accepts those values (tools/lab/build_lab.py).  Not part of the reference surface.
 * Returns the previous value. */
VPF_API int vpf_set_tuning(int key, int value);
#define VPF_TUNE_NV12_RGB_VARIANT 1
#define VPF_TUNE_RESIZE_TILE 2 /* shape of the tiled resize kernels for measurement sweeps: 0 = policy, else rows-per-tile | waves-per-workgroup << 8
                                  (rows 4..64 in steps of 4, waves 4 or 8); same pixels whatever the shape */
#define VPF_TUNE_RESIZE_MFMA 5 /* 8-bit Lanczos-3 on the matrix cores (k_lanczos_mfma.hip): 0 = policy, 1 = never (the tiled / gather kernels take Lanczos), else
                                  N-tiles per wave (0 = policy, 4 or 8) << 8 | destination 16-row tiles per band (0 = policy, 1..64); | 0x10000: the kernel
                                  evaluates its filter weights itself instead of loading the per-shape tables (the path taken when no table fits);
                                  | 0x40000: one small plane per dispatch takes the matrix-core kernel too (the policy sends it to
                                  the tile kernel, whose single-launch latency is lower); | 0x80000: up-scales march with the ring of four source tiles like
                                  everything else (policy: a ring of two, one K chunk in pass 2); same pixels whatever the value */
#define VPF_TUNE_RESIZE_BAND 3 /* destination rows per wave of the row-pair bilinear kernels: 0 = policy, 1, 2, 4, 8 or 16; 4 | nb << 8 (nb = 1..8): the march form
                                  (nb 4-row bands per wave, 8 pixels per lane on 1-channel planes) where it applies; | 0x20000: 8 pixels per lane on every 1-channel
                                  plane of a band launch however well 512-column chunks fill its rows (policy: only at >= 80 % fill); same pixels
                                  whatever the value */

#ifdef __cplusplus
}
#endif
#endif /* VPF_HIP_H_ */
