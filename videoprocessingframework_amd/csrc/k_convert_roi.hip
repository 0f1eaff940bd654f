// k_convert_roi.hip — fused multi-ROI crop + bilinear resize of NV12 / YUV420 into a normalised planar tensor (gfx950):
// vpf_convert_resize_tensor_rois.  One dispatch serves many jobs; a job = (whole source frame, rectangle at ANY integer offset, three
// destination planes), every job with scale factors of its own (RoiDesc, vpf_internal.h).  Grid z = job.
//   k_roi_strip    the staged form: a workgroup owns (job, 16 destination rows, 256 destination columns); it converts that band's source
//                  window once into an LDS strip of four-byte RGB pixels (the strip of k_convert_strip_wg) and blends from bytes
//   k_roi_gather   per-tap texel_rgb: jobs whose window does not pay or does not fit (large down-scales), VPF_TUNE_NV12_RGB_VARIANT = 9
// Definition (include/vpf_hip.h): taps are make_tap<LINEAR> on the RECTANGLE's size (they clamp at its edges), texels are frame pixels
// (x + i, y + j) converted with vpf_convert's arithmetic — chroma at absolute ((x + i) >> 1, (y + j) >> 1) —, then bilerp, truncation
// and the tensor epilogue.  Both kernels run exactly those fp32 operations in that order: identical bits.
// P10 / P12 frames (FC_P16) take the same two kernels: their 16-bit samples are narrowed to 8 bits at the load (k_fused_common.h).
#include "k_bilinear_blend.h"
#include "k_fused_common.h"
#include "k_job_launch.h"
#include "vpf_job_bounds.h"  // kRoiBandRows: shared with the launch policy (vpf_job_plan.h) and the CPU property tests

namespace vpf {

// ------------------------------------------------------------------------------------------
// The staged form.  convert_strip_wg_task (k_convert_resize.hip) with per-job geometry: the strip's pixels are ABSOLUTE frame pixels
// [base_px, ..) x rows [y + R_lo, y + R_hi], base_px = the even pixel at or below the first tap (a conversion unit = 8 pixels x 2 luma
// rows under ONE chroma row, so units start on chroma pairs of the frame, whatever the parity of the rectangle's corner); the blend
// addresses them through rectangle-relative taps.  A unit that would read past the frame's right edge takes byte loads clamped to the
// row's last sample instead of the 8-byte ones (its surplus pixels are converted and never blended): no byte outside the frame's own
// rows is read.  Rows need no clamp: every row of the window lies in the rectangle, every chroma row under it in the frame.
// ------------------------------------------------------------------------------------------
template <int SRC, int DST>  // DST = FC_TENSOR: three planes per job; FC_TENSOR_NHWC: one interleaved plane
__global__ __launch_bounds__(256) void k_roi_strip(const RoiArgs args, const Yuv2RgbCoef c, uint32_t W, uint32_t dw, uint32_t dh, uint32_t dmask,
                                                   uint32_t lds_bytes) {
  constexpr int R = kRoiBandRows;
  const RoiDesc& J = args.j[blockIdx.z];
  const FrameDesc& f = J.f;
  const uint32_t rx = J.x, ry = J.y, rw = J.w, rh = J.h;
  const float scx = J.scx, scy = J.scy;
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63, tid = threadIdx.x;
  const uint32_t Y0 = blockIdx.y * (4 * R), xs = blockIdx.x * 256;  // the grid covers the destination exactly: Y0 < dh, xs < dw
  const uint32_t Y1 = (Y0 + 4 * R - 1 < dh - 1) ? Y0 + 4 * R - 1 : dh - 1, xe = (xs + 255 < dw - 1) ? xs + 255 : dw - 1;
  const uint32_t first = rx + make_tap<VPF_INTERP_LINEAR>(xs, scx, rw).i0, last = rx + make_tap<VPF_INTERP_LINEAR>(xe, scx, rw).i1;  // frame pixels
  const uint32_t base_px = first & ~1u;
  const uint32_t R_lo_rel = __builtin_amdgcn_readfirstlane(make_tap<VPF_INTERP_LINEAR>(Y0, scy, rh).i0);
  const uint32_t R_lo = ry + R_lo_rel, R_hi = ry + __builtin_amdgcn_readfirstlane(make_tap<VPF_INTERP_LINEAR>(Y1, scy, rh).i1);  // frame rows
  uint8_t* const strip = reinterpret_cast<uint8_t*>(dyn_strip);
  const uint32_t ng = ((last - base_px) >> 3) + 1;
  const uint32_t rowbytes = 32u * ng + 16u;  // whole units + the second tap's dword behind the last pixel (weight 0 there)
  if ((R_hi - R_lo + 1) * rowbytes > lds_bytes) return;  // (never: the launcher sized the strip with this arithmetic, launch_convert_resize_rois)
  strip_fill_window<SRC>(f, c, W, strip, base_px, R_lo, R_hi, ng, rowbytes, tid);  // (k_fused_common.h: shared with k_warp_strip)
  __syncthreads();
  const uint32_t ya = Y0 + wv * R;
  if (ya > Y1) return;
  const uint32_t yb = (ya + R - 1 < Y1) ? ya + R - 1 : Y1;
  const Tap row_taps = band_row_taps(ya, yb, scy, rh);  // every lane of the wave still active here
  const uint32_t x0 = xs + lane * 4;
  if (x0 >= dw) return;
  const uint32_t nv = dw - x0 < 4 ? dw - x0 : 4;
  bool vec = nv == 4;
#pragma unroll
  for (int ch = 0; ch < (DST == FC_TENSOR_NHWC ? 1 : 3); ch++) vec = vec && ((((uintptr_t)f.d[ch] | f.dp[ch]) & dmask) == 0);
  const ColTapsX T = make_col_taps_x(base_px - rx, x0, dw, rw, scx);  // tap offsets from the strip's first pixel (frame pixel base_px = rectangle pixel base_px - x, modulo 2^32)
  const TensorEpi te = args.e;
  band_blend_rows<3, R>(strip, rowbytes, R_lo_rel, ya, yb, row_taps, T, [&](uint32_t y, const float* o) {  // o: pixel-major R G B, + 0.5 added
    if constexpr (DST == FC_TENSOR_NHWC) {
      tensor_store4_nhwc_trunc<false>(f.d[0] + (size_t)y * f.dp[0], x0, o, 1, 3, te, vec, nv, wv, lane);
    } else {
#pragma unroll
      for (int ch = 0; ch < 3; ch++) tensor_store4_trunc<false>(f.d[ch] + (size_t)y * f.dp[ch], x0, o + ch, 3, te, ch, vec, nv);
    }
  });
}

// ------------------------------------------------------------------------------------------
// The gather form: k_convert_resize with per-job geometry (four lanes-rows x 64 lanes x 4 pixels per workgroup).
// ------------------------------------------------------------------------------------------
template <int SRC, int DST>  // (FC_TENSOR_NHWC: four waves per SIMD asked for — the YUV420 instantiation stays within 128 VGPRs, the planar one takes 136)
__global__ __launch_bounds__(256, (DST == FC_TENSOR_NHWC ? 4 : 1)) void k_roi_gather(const RoiArgs args, const Yuv2RgbCoef c, uint32_t dw, uint32_t dh,
                                                                                     uint32_t dmask) {
  const RoiDesc& J = args.j[blockIdx.z];
  const FrameDesc& f = J.f;
  const uint32_t x0 = (blockIdx.x * 64 + (threadIdx.x & 63)) * 4;
  const uint32_t y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x0 >= dw || y >= dh) return;
  const Tap ty = make_tap<VPF_INTERP_LINEAR>(y, J.scy, J.h);
  float o[3][4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const Tap tx = make_tap<VPF_INTERP_LINEAR>((x0 + k < dw) ? x0 + k : dw - 1, J.scx, J.w);
    float p00[3], p01[3], p10[3], p11[3];
    texel_rgb<SRC>(f, c, J.x + tx.i0, J.y + ty.i0, p00);
    texel_rgb<SRC>(f, c, J.x + tx.i1, J.y + ty.i0, p01);
    texel_rgb<SRC>(f, c, J.x + tx.i0, J.y + ty.i1, p10);
    texel_rgb<SRC>(f, c, J.x + tx.i1, J.y + ty.i1, p11);
#pragma unroll
    for (int ch = 0; ch < 3; ch++) o[ch][k] = bilerp(p00[ch], p01[ch], p10[ch], p11[ch], tx.f, ty.f);
  }
  const uint32_t nv = dw - x0 < 4 ? dw - x0 : 4;
  bool vec = nv == 4;
#pragma unroll
  for (int ch = 0; ch < (DST == FC_TENSOR_NHWC ? 1 : 3); ch++) vec = vec && ((((uintptr_t)f.d[ch] | f.dp[ch]) & dmask) == 0);
  if constexpr (DST == FC_TENSOR_NHWC) {
    tensor_store4_nhwc_trunc<false>(f.d[0] + (size_t)y * f.dp[0], x0, &o[0][0], 4, 1, args.e, vec, nv,
                                    __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), threadIdx.x & 63);
  } else {
    for (int ch = 0; ch < 3; ch++) tensor_store4_trunc<false>(f.d[ch] + (size_t)y * f.dp[ch], x0, o[ch], 1, args.e, ch, vec, nv);
  }
}

// ------------------------------------------------------------------------------------------
// Host side: fill the shape, ask job_plan (vpf_job_plan.h: the cap, staged or per tap per job — roi_strip_need and the policy's two limits,
// vpf_job_bounds.h —, the grids, the strip's bytes, the channels-last staging), fill the two tables from it and launch what it names.
// ------------------------------------------------------------------------------------------
hipError_t launch_convert_resize_rois(hipStream_t st, int src_fc, const Yuv2RgbCoef& c, uint32_t W, uint32_t n, const RoiDesc* jobs, uint32_t dw,
                                      uint32_t dh, const TensorEpi& te, bool nhwc) {
  JobShape q;
  job_shape(q, JOB_ROI, false, src_fc, nhwc, te, W, 0u, dw, dh);
  job_shape_jobs(q, jobs, n, [](JobGeom& g, const RoiDesc& j) { g.x = j.x; g.w = j.w; g.h = j.h; g.scx = j.scx; g.scy = j.scy; });
  const JobPlan p = job_plan(q);
  if (!p.ok) return hipErrorInvalidValue;
  RoiArgs t[2];
  fill_job_tables(p, jobs, n, te, t);
  hipError_t e = hipSuccess;
  for (int k = 0; k < p.nd && e == hipSuccess; k++) {  // staged first; its error returns before the per-tap launch
    const JobDispatch& d = p.d[k];
    const dim3 grid(d.gx, d.gy, d.n);
    const uint32_t lds_all = job_launch_lds(d, te, t[k]);
    with_src_dst(src_fc, nhwc, [&](auto S, auto D) {
      if (d.form == JF_ROI_STRIP) VPF_LAUNCH_T(k_roi_strip, (S, D), grid, lds_all, st, t[k], c, W, dw, dh, p.dmask, d.lds);
      else VPF_LAUNCH_T(k_roi_gather, (S, D), grid, lds_all, st, t[k], c, dw, dh, p.dmask);
      e = hipGetLastError();
    });
  }
  return e;
}

}  // namespace vpf
