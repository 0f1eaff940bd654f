// vpf_internal.h — shared between the translation units of libvpfhip (gfx950 only).
#pragma once
#include <cstring>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vpf_classes.h"
#include "vpf_hip.h"

namespace vpf {

// ------------------------------------------------------------------------------------------
// YUV -> RGB coefficients in the form the kernels consume.  Biases fold the luma offset and the
// chroma -128, so a pixel costs one FMA per channel:
//   rc = fma(V, rv, br);  gc = fma(U, gu, fma(V, gv, bg));  bc = fma(U, bu, bb)     (per chroma sample)
//   R = sat_rne(fma(Y, cy, rc)); G = sat_rne(fma(Y, cy, gc)); B = sat_rne(fma(Y, cy, bc))
// sat_rne = saturate to [0,255], round to nearest even (v_cvt_pk_u8_f32)
// ------------------------------------------------------------------------------------------
struct Yuv2RgbCoef {
  float cy, rv, gu, gv, bu, br, bg, bb;
};
// RGB -> YUV: out_k = sat_trunc(fma(R, m[k][0], fma(G, m[k][1], fma(B, m[k][2], d[k]))))
struct Rgb2YuvCoef {
  float m[3][3];
  float d[3];
};
bool make_yuv2rgb(int color_space, int color_range, Yuv2RgbCoef* out);
bool make_rgb2yuv(int color_range, Rgb2YuvCoef* out);

// The frame table of a batched launch travels in the kernarg segment (no device-side table to manage).  Two sizes since round 5:
//   BatchArgs   32 frames x 72 B = 2.3 KiB — every converter and remap kernel, and every resize / fused launch of up to 32 frames (one
//               frame per dispatch included: the unmodified per-Execute() API);
//   BatchArgsL  128 frames = 9 KiB — resize and fused launches of 33 .. 128 frames.  A batch of small planes is 25-50 us of kernel per 32
//               frames; every dispatch boundary costs ~3 us of idle chip plus a tail of partly empty CUs of about one wave life
//               (profiles/r05_wave_times.txt): four times the frames per dispatch amortise both.
// The kernarg segment is write-combined host memory: a launch pays ~0.2 us of HOST time per KiB of argument (9 KiB: + 1.3-2 us per call,
// profiles/r05_abi_launch_rate_9k_kernarg.txt) — nothing against a 128-frame dispatch, 40-70 % of a single frame's issue time.  Hence
// two instantiations of the resize / fused batch kernels (template parameter BA) instead of one large table for everybody.
// (kSmallBatch = 32, kMaxBatch = 128: vpf_classes.h)
struct FrameDesc {
  const uint8_t* s[3];
  uint8_t* d[3];
  uint32_t sp[3];
  uint32_t dp[3];
};
template <int CAP>
struct BatchArgsT {
  FrameDesc f[CAP];
};
using BatchArgs = BatchArgsT<kSmallBatch>;
using BatchArgsL = BatchArgsT<kMaxBatch>;
// the small table of a launch of n <= kSmallBatch frames (host side: the launchers pass BatchArgsL around and cut it down at the launch)
inline BatchArgs small_batch(const BatchArgsL& a, uint32_t n) {
  BatchArgs s;
  std::memcpy(s.f, a.f, (size_t)(n < (uint32_t)kSmallBatch ? n : (uint32_t)kSmallBatch) * sizeof(FrameDesc));
  return s;
}
// Single-frame kernel entries (one Execute() = one launch) take the frame as SCALAR arguments, source side and task
// counts first: the library is built with -amdgpu-kernarg-preload-count=16, so the dispatcher hands those to the wave in
// SGPRs and its first loads do not wait for a scalar-cache round trip to the kernarg segment (a by-value BatchArgs is
// never preloaded).  Worth 0.5-0.8 us per launch on kernels that last 4-7 us.
#define VPF_ONE_SRC_PARAMS const uint8_t *s0, const uint8_t *s1, const uint8_t *s2, uint32_t sp0, uint32_t sp1, uint32_t sp2
#define VPF_ONE_DST_PARAMS uint8_t *d0, uint8_t *d1, uint8_t *d2, uint32_t dp0, uint32_t dp1, uint32_t dp2
#define VPF_ONE_FRAME FrameDesc{{s0, s1, s2}, {d0, d1, d2}, {sp0, sp1, sp2}, {dp0, dp1, dp2}}
#define VPF_ONE_SRC_ARGS(f) (f).s[0], (f).s[1], (f).s[2], (f).sp[0], (f).sp[1], (f).sp[2]
#define VPF_ONE_DST_ARGS(f) (f).d[0], (f).d[1], (f).d[2], (f).dp[0], (f).dp[1], (f).dp[2]

// (FmtClass — FC_NV12 ... FC_TENSOR_NHWC: vpf_classes.h)
// The epilogue of an FC_TENSOR launch: out[c] = to_dtype(fma(u8[c], scale[c], bias[c])).  It travels behind the frame table (BatchArgsTE), so
// the 8-bit instantiations keep their kernarg layout.  Channel order is the kernels' R G B; BGR is the host's swap of planes and parameters.
// FC_TENSOR_NHWC has one plane, so B G R order cannot be a swap of planes there: the host still swaps the parameters (scale / bias / border stay
// in kernel channel order) and sets kEpiSwapRB in `dtype`; the epilogue then puts kernel channel ch into slot 2 - ch (wave-uniform).  FC_TENSOR
// launches never carry the bit: their kernels compare `dtype` as a whole.
constexpr uint32_t kEpiSwapRB = 0x80000000u;
// ... and where the launch has room, the wave's interleaved row leaves through LDS as dense stores (k_fused_common.h): bits 8 .. 20 of `dtype` = 1 +
// the offset of the staging area in the launch's dynamic LDS, in 16-B units (0: none, store per lane).  Per wave 64 lanes x 3 NPX elements.
constexpr uint32_t kEpiDtypeMask = 0xffu, kEpiStageShift = 8, kEpiStageMask = 0x1fffu << kEpiStageShift;
// Which rows take the dense form: 1 = f32 rows, 2 = f16 / bf16 rows of the families with four pixels per lane, 4 = f16 / bf16 rows of
// k_convert_half (eight pixels per lane).  Measured per family with builds of mask 0 and 7 (profiles/r11_tensor_nhwc.txt): without
// 1 f32 rows are 4-37 % slower in the 4-px families and ~8 x slower in k_convert_half; with 2 the 16-bit rows of the strip and per-tap kernels
// are slower (two 12-B stores per lane beat 8-B LDS writes plus 1.5 dense stores); without 4 k_convert_half's 16-bit rows are ~1.6 x slower.
#ifndef VPF_NHWC_DENSE
#define VPF_NHWC_DENSE (1 | 4)
#endif
struct TensorEpi {
  float scale[3], bias[3];
  uint32_t dtype;  // VPF_TENSOR_*: wave-uniform branch of the epilogue (FC_TENSOR_NHWC: | kEpiSwapRB)
  uint32_t pad;
};
static_assert(sizeof(TensorEpi) == 32, "the epilogue rides behind the frame and job tables: its size is part of their layout");
// The staging plan of an FC_TENSOR_NHWC launch whose kernel uses `lds` bytes of dynamic LDS itself and gives a lane `npx` pixels: the epilogue to
// pass (e with the area's place) and the dynamic LDS to ask for.  No room under the 64 KiB a workgroup may take: no staging, the same kernel.
inline uint32_t nhwc_stage_plan(const TensorEpi& te, uint32_t lds, uint32_t npx, TensorEpi* e) {
  *e = te;
  const uint32_t dt = te.dtype & kEpiDtypeMask;
  const bool want = dt == VPF_TENSOR_F32 ? ((VPF_NHWC_DENSE) & 1) != 0 : ((VPF_NHWC_DENSE) & (npx == 8 ? 4 : 2)) != 0;
  const uint32_t bytes = 4u * 64u * 3u * npx * (dt == VPF_TENSOR_F32 ? 4u : 2u);
  if (!want || (lds & 15u) || lds + bytes > 64u * 1024u) return lds;
  e->dtype |= (lds / 16u + 1u) << kEpiStageShift;
  return lds + bytes;
}
template <int CAP>
struct BatchArgsTE {
  FrameDesc f[CAP];
  TensorEpi e;
};

// The job table of a multi-ROI launch (vpf_convert_resize_tensor_rois, k_convert_roi.hip): per job the planes of the WHOLE source frame and
// of the destination, the rectangle in luma pixels of the frame, and the job's own scale factors (computed on the host as every launcher
// does: (float)w / (float)dw).  96 jobs x 96 B + the epilogue = the 9 248 B of BatchArgsTE<kMaxBatch>, the largest argument block measured.
// (kRoiBatch = 96, kLetterboxBatch = 82, kWarpBatch = 96, kPerspBatch = 82, kRoiDevFrames = 128: vpf_classes.h — the HIP-free launch policy of these
// tables, vpf_job_plan.h, names them too)
struct RoiDesc {
  FrameDesc f;
  uint32_t x, y, w, h;
  float scx, scy;
};
struct RoiArgs {
  RoiDesc j[kRoiBatch];
  TensorEpi e;
};
static_assert(sizeof(RoiDesc) == 96 && sizeof(RoiArgs) <= sizeof(BatchArgsTE<kMaxBatch>), "the ROI job table must not outgrow the largest frame table");

// The arguments of a multi-ROI launch whose rectangles live in DEVICE memory (vpf_convert_resize_tensor_rois_dev, k_convert_roi_dev.hip): no job
// table — the source planes of up to 128 frames (40 B each), where the boxes and their count lie, and job 0's destination planes with the stride
// from job to job.  The kernel reads (frame, x, y, w, h) of job blockIdx.z when it runs.  5 224 B, below the largest argument block.
struct FrameSrcDesc {
  const uint8_t* s[3];
  uint32_t sp[3];
  uint32_t pad;
};
struct RoiDevArgs {
  FrameSrcDesc f[kRoiDevFrames];
  const int32_t* boxes;  // device: five ints per job, box_stride bytes apart
  const int32_t* count;  // device, or null: max_n
  uint8_t* d[3];         // job 0's planes (kernel channel order); job k's lie k * job_stride bytes further
  uint64_t job_stride;
  uint32_t dp[3];
  uint32_t box_stride, max_n, n_frames;
  TensorEpi e;
};
static_assert(sizeof(FrameSrcDesc) == 40 && sizeof(RoiDevArgs) == 128 * 40 + 104 && sizeof(RoiDevArgs) <= sizeof(BatchArgsTE<kMaxBatch>),
              "the device-ROI arguments must not outgrow the largest frame table");

// The job table of a letterbox launch (vpf_convert_letterbox_tensor, k_convert_letterbox.hip): a RoiDesc — its scale factors are the rectangle's over
// the PICTURE's size, (float)w / (float)iw — plus where the picture goes inside the destination plane.  The rectangle travels as four 32-bit fields:
// 112 B per job, 82 jobs + the epilogue = 9 216 B, within the 9 248 B of BatchArgsTE<kMaxBatch>.  (Packed as 16-bit pairs — iw - 1, ih - 1: sizes
// run to 65536 — it would keep 96 jobs per table at the price of an unpack per field in every wave; a call of 96 jobs then takes two tables
// instead of one, which the job-table test crosses either way.)  The three pad bytes (kernel channel order R G B) travel in TensorEpi::pad:
// pad = pad[0] | pad[1] << 8 | pad[2] << 16, bits 24 .. 31 zero.  The NHWC staging plan lives in TensorEpi::dtype (nhwc_stage_plan): no collision.
struct LetterboxDesc {
  RoiDesc r;
  uint32_t ix, iy, iw, ih;
};
struct LetterboxArgs {
  LetterboxDesc j[kLetterboxBatch];
  TensorEpi e;
};
static_assert(sizeof(LetterboxDesc) == 112 && sizeof(LetterboxArgs) == 82 * 112 + 32 && sizeof(LetterboxArgs) <= sizeof(BatchArgsTE<kMaxBatch>),
              "the letterbox job table must not outgrow the largest frame table");

// The arguments of a letterbox launch whose boxes live in DEVICE memory (vpf_convert_letterbox_tensor_dev, k_convert_letterbox_dev.hip): RoiDevArgs plus
// where the optional placements lie.  The kernel reads (frame, x, y, w, h) and, with `rects`, (ix, iy, iw, ih) of job blockIdx.z when it runs; without,
// it fits the box into the plane itself (letterbox_fit_ints, vpf_job_bounds.h).  The pad bytes travel in TensorEpi::pad as in LetterboxArgs.
// 5 240 B, below the largest argument block.
struct LetterboxDevArgs {
  FrameSrcDesc f[kRoiDevFrames];
  const int32_t* boxes;  // device: five ints per job, box_stride bytes apart
  const int32_t* rects;  // device: four ints per job, rect_stride bytes apart; null: the kernel fits
  const int32_t* count;  // device, or null: max_n
  uint8_t* d[3];         // job 0's WHOLE planes (kernel channel order); job k's lie k * job_stride bytes further
  uint64_t job_stride;
  uint32_t dp[3];
  uint32_t box_stride, rect_stride, max_n, n_frames, pad;
  TensorEpi e;
};
static_assert(sizeof(LetterboxDevArgs) == 128 * 40 + 120 && sizeof(LetterboxDevArgs) <= sizeof(BatchArgsTE<kMaxBatch>),
              "the device-letterbox arguments must not outgrow the largest frame table");

// The job table of a multi-ROI affine warp (vpf_convert_warp_tensor, k_convert_warp.hip): per job the planes of the WHOLE source frame and of the
// destination and the inverse matrix m = (m00 m01 m02; m10 m11 m12), destination pixel -> source coordinates in luma pixels.  96 B like RoiDesc,
// so the same 96 jobs per table.  The three border bytes (kernel channel order R G B) and the border mode travel in TensorEpi::pad:
// pad = border[0] | border[1] << 8 | border[2] << 16 | mode << 24.
struct WarpDesc {
  FrameDesc f;
  float m[6];
};
struct WarpArgs {
  WarpDesc j[kWarpBatch];
  TensorEpi e;
};
static_assert(sizeof(WarpDesc) == 96 && sizeof(WarpArgs) <= sizeof(BatchArgsTE<kMaxBatch>), "the warp job table must not outgrow the largest frame table");

// The job table of a multi-ROI perspective warp (vpf_convert_persp_tensor, k_convert_persp.hip): WarpDesc with the inverse 3 x 3 matrix
// m = (m00 m01 m02; m10 m11 m12; m20 m21 m22).  72 + 36 B, 112 with the tail padding of the pointers' alignment: 82 jobs per table, the letterbox
// table's 9 216 B.  Border bytes and mode travel in TensorEpi::pad as in WarpArgs.
struct PerspDesc {
  FrameDesc f;
  float m[9];
};
struct PerspArgs {
  PerspDesc j[kPerspBatch];
  TensorEpi e;
};
static_assert(sizeof(PerspDesc) == 112 && sizeof(PerspArgs) == 82 * 112 + 32 && sizeof(PerspArgs) <= sizeof(BatchArgsTE<kMaxBatch>),
              "the perspective job table must not outgrow the largest frame table");

// The arguments of a warp launch whose matrices live in DEVICE memory (vpf_convert_warp_tensor_dev, k_convert_warp_dev.hip; vpf_convert_persp_tensor_dev,
// k_convert_persp_dev.hip: nine floats per job): the shape of RoiDevArgs —
// the source planes of up to 128 frames, where the matrices, the frame indices and the count lie, and job 0's destination planes with the stride
// from job to job.  The kernel reads (frame, m[6] or m[9]) of job blockIdx.z when it runs.  Border bytes and mode travel in TensorEpi::pad as in WarpArgs.
// 5 240 B, below the largest argument block.
struct WarpDevArgs {
  FrameSrcDesc f[kRoiDevFrames];
  const float* matrices;       // device: six (affine) or nine (perspective) floats per job, matrix_stride bytes apart
  const int32_t* frame_index;  // device: one int per job, frame_stride bytes apart; null: every job samples f[0]
  const int32_t* count;        // device, or null: max_n
  uint8_t* d[3];               // job 0's planes (kernel channel order); job k's lie k * job_stride bytes further
  uint64_t job_stride;
  uint32_t dp[3];
  uint32_t matrix_stride, frame_stride, max_n, n_frames, pad;
  TensorEpi e;
};
static_assert(sizeof(WarpDevArgs) == 128 * 40 + 120 && sizeof(WarpDevArgs) <= sizeof(BatchArgsTE<kMaxBatch>),
              "the device-warp arguments must not outgrow the largest frame table");

// The job table of a per-pixel remap into a tensor (vpf_convert_remap_tensor, k_convert_remap.hip): per job the planes of the WHOLE source frame and
// of the destination, and where the job's two coordinate maps lie in DEVICE memory — row dy of a map at byte dy * pitch, dw floats.  96 B like
// WarpDesc, so the same 96 jobs per table.  Border bytes and mode travel in TensorEpi::pad as in WarpArgs.
struct RemapDesc {
  FrameDesc f;
  const float* xm;  // device
  const float* ym;  // device
  uint32_t xp, yp;  // bytes
};
struct RemapArgs {
  RemapDesc j[kRemapBatch];
  TensorEpi e;
};
static_assert(sizeof(RemapDesc) == 96 && sizeof(RemapArgs) <= sizeof(BatchArgsTE<kMaxBatch>), "the remap job table must not outgrow the largest frame table");

// The prologue of a tensor -> NV12 / YUV420 launch (vpf_tensor_convert): q[c] = rint(clamp(x[c] * scale[c] + bias[c], 0, 255)) feeds the RGB -> YUV
// arithmetic.  Channel order is the kernels' R G B; BGR is the host's swap of planes and parameters.
struct TensorPro {
  float scale[3], bias[3];
  uint32_t dtype;  // VPF_TENSOR_*: template parameter of the fast kernel, wave-uniform branch of the quad kernel
  uint32_t pad;    // the NHWC kernels: 1 = kernel channel ch is read from slot 2 - ch of the interleaved plane (B G R order); else 0
};

// launchers (one per translation unit); all asynchronous on `st`
hipError_t launch_yuv_to_rgb(hipStream_t st, int src_fc, int dst_fc, const Yuv2RgbCoef& c, uint32_t w,
                             uint32_t h, uint32_t n, const BatchArgs& a, int variant, bool dst_reused = false);
hipError_t launch_rgb_to_yuv(hipStream_t st, int src_fc, int dst_fc /*FC_YUV444|FC_YUV420*/,
                             const Rgb2YuvCoef& c, uint32_t w, uint32_t h, uint32_t n, const BatchArgs& a);
// three planes of f32 / f16 / bf16 (FrameDesc::s, R G B) -> NV12 (d[0], d[1]) or YUV420 (d[0..2]); k_rgb2yuv.hip
// nhwc: ONE interleaved plane of w x 3 elements per row (FrameDesc::s[0]; t.pad = 1 for B G R order) instead of the three planes
hipError_t launch_tensor_to_yuv(hipStream_t st, bool nv12, const Rgb2YuvCoef& c, const TensorPro& t, uint32_t w, uint32_t h, uint32_t n,
                                const BatchArgs& a, bool nhwc = false);
hipError_t launch_relayout(hipStream_t st, int src_fmt, int dst_fmt, uint32_t w, uint32_t h, uint32_t n,
                           const BatchArgs& a);
// (ResizeJob, one plane of a resize: vpf_classes.h)
// all planes of a format (8-bit, or f32: float surfaces) over n <= kMaxBatch same-shape frames in as few launches as possible, one plane of one
// frame through the scalar-argument entries: whatever resize_plan (vpf_resize_plan.h) names; `call_n`: the frames of the whole call this dispatch
// is a part of; k_resize.hip
hipError_t launch_resize_planned(hipStream_t st, bool f32, int interp, int njobs, const ResizeJob* jobs, uint32_t n, const BatchArgsL& a, uint32_t call_n);
// 8-bit Lanczos-3 on the matrix cores (k_lanczos_mfma.hip): every plane in `jobs` over n frames in ONE dispatch; false when it does not apply
// (window / ring bounds of vpf_plan_bounds.h, 16-B aligned rows) and nothing was launched
bool launch_lanczos_mfma(hipStream_t st, int njobs, const ResizeJob* jobs, uint32_t n, const BatchArgsL& a);
// the caller-owned table workspace of the vpf_resize_ws / vpf_resize_batch_ws call the current thread is inside (nullptr: none)
void set_lanczos_workspace(vpf_workspace* ws);
uint64_t lanczos_table_bytes_bound(int ch, uint32_t dw, uint32_t dh);  // upper bound of one plane's table bytes under any launch shape
hipError_t launch_remap(hipStream_t st, uint32_t sw, uint32_t sh, const uint8_t* src, uint32_t spitch,
                        const float* xmap, uint32_t xpitch, const float* ymap, uint32_t ypitch, uint32_t dw,
                        uint32_t dh, uint8_t* dst, uint32_t dpitch);
hipError_t launch_remap_batch(hipStream_t st, uint32_t sw, uint32_t sh, const float* xmap, uint32_t xpitch, const float* ymap, uint32_t ypitch,
                              uint32_t dw, uint32_t dh, uint32_t n, const BatchArgs& a);
// dst_fc == FC_TENSOR / FC_TENSOR_NHWC take `te` (the element size sets the destination alignment tests); every other class ignores it
hipError_t launch_convert_resize(hipStream_t st, int src_fc, int dst_fc, const Yuv2RgbCoef& c, uint32_t sw,
                                 uint32_t sh, uint32_t n, const BatchArgsL& a, uint32_t dw, uint32_t dh, const TensorEpi* te = nullptr);
// The eight per-job launchers below dispatch on job_plan (vpf_job_plan.h): refusals, staged or per tap, grids and LDS are stated there.
// n <= kRoiBatch jobs on frames `W` pixels wide -> FC_TENSOR planes of dw x dh: at most two dispatches (staged jobs, gather jobs); k_convert_roi.hip
// (nhwc: FC_TENSOR_NHWC planes, one per job, here and in launch_convert_warp)
hipError_t launch_convert_resize_rois(hipStream_t st, int src_fc, const Yuv2RgbCoef& c, uint32_t W, uint32_t n, const RoiDesc* jobs, uint32_t dw,
                                      uint32_t dh, const TensorEpi& te, bool nhwc = false);
// n <= kWarpBatch jobs on frames of W x H pixels -> FC_TENSOR planes of dw x dh: at most two dispatches (staged jobs, gather jobs); `te.pad`
// carries border and mode (WarpArgs); k_convert_warp.hip
hipError_t launch_convert_warp(hipStream_t st, int src_fc, const Yuv2RgbCoef& c, uint32_t W, uint32_t H, uint32_t n, const WarpDesc* jobs, uint32_t dw,
                               uint32_t dh, const TensorEpi& te, bool nhwc = false);
// n <= kPerspBatch jobs on frames of W x H pixels -> FC_TENSOR (nhwc: FC_TENSOR_NHWC) planes of dw x dh: at most two dispatches (jobs whose
// tiles may stage, per-tap jobs); `te.pad` carries border and mode; k_convert_persp.hip
hipError_t launch_convert_persp(hipStream_t st, int src_fc, const Yuv2RgbCoef& c, uint32_t W, uint32_t H, uint32_t n, const PerspDesc* jobs, uint32_t dw,
                                uint32_t dh, const TensorEpi& te, bool nhwc = false);
// n <= kLetterboxBatch jobs on frames `W` pixels wide -> FC_TENSOR (nhwc: FC_TENSOR_NHWC) planes of dw x dh, the picture at each job's (ix, iy, iw, ih)
// and `te.pad` everywhere else: at most two dispatches (staged jobs, gather jobs); k_convert_letterbox.hip
hipError_t launch_convert_letterbox(hipStream_t st, int src_fc, const Yuv2RgbCoef& c, uint32_t W, uint32_t n, const LetterboxDesc* jobs, uint32_t dw,
                                    uint32_t dh, const TensorEpi& te, bool nhwc = false);
// the same jobs through the triangle filter whose support grows with the scale (vpf_convert_letterbox_tensor_aa): at most two dispatches, staged jobs
// and per-tap jobs, by aa_plan (vpf_aa_plan.h); k_convert_letterbox_aa.hip
hipError_t launch_convert_letterbox_aa(hipStream_t st, int src_fc, const Yuv2RgbCoef& c, uint32_t W, uint32_t n, const LetterboxDesc* jobs, uint32_t dw,
                                       uint32_t dh, const TensorEpi& te, bool nhwc = false);
// up to a.max_n jobs whose rectangles the kernel reads from device memory, on frames of W x H pixels -> FC_TENSOR (nhwc: FC_TENSOR_NHWC) planes of
// dw x dh: ONE dispatch, every tile staged or per tap by its own window; a.e is set here; k_convert_roi_dev.hip
hipError_t launch_convert_resize_rois_dev(hipStream_t st, int src_fc, const Yuv2RgbCoef& c, uint32_t W, uint32_t H, RoiDevArgs& a, uint32_t dw, uint32_t dh,
                                          const TensorEpi& te, bool nhwc = false);
// up to a.max_n letterbox jobs whose boxes (and, with a.rects, placements) the kernel reads from device memory, on frames of W x H pixels -> FC_TENSOR
// (nhwc: FC_TENSOR_NHWC) planes of dw x dh: ONE dispatch, every tile padded, staged or per tap by its own window; `te.pad` carries the pad bytes;
// a.e is set here; k_convert_letterbox_dev.hip
hipError_t launch_convert_letterbox_dev(hipStream_t st, int src_fc, const Yuv2RgbCoef& c, uint32_t W, uint32_t H, LetterboxDevArgs& a, uint32_t dw,
                                        uint32_t dh, const TensorEpi& te, bool nhwc = false);
// up to a.max_n jobs whose matrices the kernel reads from device memory, on frames of W x H pixels -> FC_TENSOR (nhwc: FC_TENSOR_NHWC) planes of
// dw x dh: ONE dispatch, every tile staged or per tap by its own window; `max_step` sizes the dynamic LDS (warp_dev_lds_bytes, vpf_job_bounds.h);
// `te.pad` carries border and mode; a.e is set here; k_convert_warp_dev.hip
hipError_t launch_convert_warp_dev(hipStream_t st, int src_fc, const Yuv2RgbCoef& c, uint32_t W, uint32_t H, WarpDevArgs& a, uint32_t dw, uint32_t dh,
                                   float max_step, const TensorEpi& te, bool nhwc = false);
// the same for homographies (nine floats per job): ONE dispatch, every tile border, per tap or staged by its own corners; `max_step` sizes the
// dynamic LDS (persp_dev_lds_bytes, vpf_job_bounds.h); k_convert_persp_dev.hip
hipError_t launch_convert_persp_dev(hipStream_t st, int src_fc, const Yuv2RgbCoef& c, uint32_t W, uint32_t H, WarpDevArgs& a, uint32_t dw, uint32_t dh,
                                    float max_step, const TensorEpi& te, bool nhwc = false);
// n <= kRemapBatch jobs on frames of W x H pixels, each through its own pair of device maps -> FC_TENSOR (nhwc: FC_TENSOR_NHWC) planes of dw x dh:
// ONE dispatch (remap_plan, vpf_remap_plan.h), every tile border, staged or per tap by the exact window of the coordinates it loaded; `max_step`
// sizes the dynamic LDS; `te.pad` carries border and mode; k_convert_remap.hip
hipError_t launch_convert_remap(hipStream_t st, int src_fc, const Yuv2RgbCoef& c, uint32_t W, uint32_t H, uint32_t n, const RemapDesc* jobs, uint32_t dw,
                                uint32_t dh, float max_step, const TensorEpi& te, bool nhwc = false);

int tuning(int key);

// Diagnostics (both off by default, one relaxed atomic load per call when off):
//   VPF_HIP_LOG=1    launch / runtime errors on stderr;  VPF_HIP_LOG=2  also which kernel every launch selected
//   VPF_HIP_ROCTX=1  a roctx range around every C-ABI entry and a marker per kernel selection (rocprofv3 --marker-trace shows them
//                    next to the kernels) — the counterpart of the reference's NvtxMark (src/TC/inc/Tasks.hpp:27-52, USE_NVTX);
//                    librocprofiler-sdk-roctx is dlopen()ed on first use, so there is no link-time dependency
int log_level();
void note_kernel(const char* kernel_expr);  // called by VPF_LAUNCH when log_level() >= 2 or roctx is on
bool trace_on();
void trace_push(const char* name);
void trace_pop();
struct Mark {
  bool on;
  explicit Mark(const char* name) : on(trace_on()) { if (on) trace_push(name); }
  ~Mark() { if (on) trace_pop(); }
  Mark(const Mark&) = delete;
  Mark& operator=(const Mark&) = delete;
};

// hipGetLastError() is sticky per thread: an unrelated earlier failure (e.g. a caller's bad memcpy) would be
// reported by the check that follows a launch.  Clear it first so the check sees this launch only.
#define VPF_LAUNCH(K, ...)                                               \
  do {                                                                   \
    if (vpf::log_level() >= 2 || vpf::trace_on()) vpf::note_kernel(#K);  \
    (void)hipGetLastError();                                             \
    hipLaunchKernelGGL(K, __VA_ARGS__);                                  \
  } while (0)

}  // namespace vpf
