// k_convert_roi.hip — fused multi-ROI crop + bilinear resize of NV12 / YUV420 into a normalised planar tensor (gfx950):
// vpf_convert_resize_tensor_rois.  One dispatch serves many jobs; a job = (whole source frame, rectangle at ANY integer offset, three
// destination planes), every job with scale factors of its own (RoiDesc, vpf_internal.h).  Grid z = job.
//   k_roi_strip    the staged form: a workgroup owns (job, 16 destination rows, 256 destination columns); it converts that band's source
//                  window once into an LDS strip of four-byte RGB pixels (the strip of k_convert_strip_wg) and blends from bytes
//   k_roi_gather   per-tap texel_rgb: jobs whose window does not pay or does not fit (large down-scales), VPF_TUNE_NV12_RGB_VARIANT = 9
// Definition (include/vpf_hip.h): taps are make_tap<LINEAR> on the RECTANGLE's size (they clamp at its edges), texels are frame pixels
// (x + i, y + j) converted with vpf_convert's arithmetic — chroma at absolute ((x + i) >> 1, (y + j) >> 1) —, then bilerp, truncation
// and the tensor epilogue.  Both kernels run exactly those fp32 operations in that order: identical bits.  The staged body is roi_strip_tile
// (k_convert_roi_common.h), which k_roi_dev runs as well; the per-tap pixel is typed here and in k_roi_dev.
// P10 / P12 frames (FC_P16) take the same two kernels: their 16-bit samples are narrowed to 8 bits at the load (k_fused_common.h).
#include "k_convert_roi_common.h"
#include "k_dev_table.h"  // tile_window_uniform
#include "k_job_launch.h"
#include "vpf_job_bounds.h"  // kRoiBandRows, roi_tile_window: shared with the launch policy (vpf_job_plan.h) and the CPU property tests

namespace vpf {

// ------------------------------------------------------------------------------------------
// The staged form: the tile's window (roi_tile_window, vpf_job_bounds.h: what the launch policy sized the strip with), then roi_strip_tile
// (k_convert_roi_common.h).
// ------------------------------------------------------------------------------------------
template <int SRC, int DST>  // DST = FC_TENSOR: three planes per job; FC_TENSOR_NHWC: one interleaved plane
__global__ __launch_bounds__(256) void k_roi_strip(const RoiArgs args, const Yuv2RgbCoef c, uint32_t W, uint32_t dw, uint32_t dh, uint32_t dmask,
                                                   uint32_t lds_bytes) {
  constexpr int R = kRoiBandRows;
  const RoiDesc& J = args.j[blockIdx.z];
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63, tid = threadIdx.x;
  const uint32_t Y0 = blockIdx.y * (4 * R), xs = blockIdx.x * 256;  // the grid covers the destination exactly: Y0 < dh, xs < dw
  const uint32_t Y1 = (Y0 + 4 * R - 1 < dh - 1) ? Y0 + 4 * R - 1 : dh - 1, xe = (xs + 255 < dw - 1) ? xs + 255 : dw - 1;
  RoiTileWin win = roi_tile_window(J.x, J.w, J.h, J.scx, J.scy, xs, xe, Y0, Y1);
  tile_window_uniform(win);
  if (win.rows * win.rowbytes > lds_bytes) return;  // (never: the launcher sized the strip with this arithmetic, launch_convert_resize_rois)
  const uint32_t ya = Y0 + wv * R, yb = (ya + R - 1 < Y1) ? ya + R - 1 : Y1;  // this wave's rows (none when ya > Y1)
  const uint32_t x0 = xs + lane * 4;                                        // this lane's four columns (none when x0 >= dw)
  const uint32_t nv = x0 < dw ? (dw - x0 < 4 ? dw - x0 : 4) : 0;
  roi_strip_tile<SRC, DST>(J.f, c, W, J.x, J.y, J.w, J.h, J.scx, J.scy, win, dw, ya, yb, x0, nv, tensor_vec_ok<DST>(J.f, nv, dmask), wv, lane, tid, args.e);
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
