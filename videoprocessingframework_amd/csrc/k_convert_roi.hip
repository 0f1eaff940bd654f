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
#include "vpf_job_bounds.h"  // kRoiBandRows, roi_strip_need, the policy's limits: shared with the CPU property test

namespace vpf {

// ------------------------------------------------------------------------------------------
// The staged form.  convert_strip_wg_task (k_convert_resize.hip) with per-job geometry: the strip's pixels are ABSOLUTE frame pixels
// [base_px, ..) x rows [y + R_lo, y + R_hi], base_px = the even pixel at or below the first tap (a conversion unit = 8 pixels x 2 luma
// rows under ONE chroma row, so units start on chroma pairs of the frame, whatever the parity of the rectangle's corner); the blend
// addresses them through rectangle-relative taps.  A unit that would read past the frame's right edge takes byte loads clamped to the
// row's last sample instead of the 8-byte ones (its surplus pixels are converted and never blended): no byte outside the frame's own
// rows is read.  Rows need no clamp: every row of the window lies in the rectangle, every chroma row under it in the frame.
// ------------------------------------------------------------------------------------------
// (DST = FC_TENSOR: three planes per job, k_roi_strip; FC_TENSOR_NHWC: one interleaved plane, k_roi_strip_nhwc)
template <int SRC>
__global__ __launch_bounds__(256) void k_roi_strip(const RoiArgs args, const Yuv2RgbCoef c, uint32_t W, uint32_t dw, uint32_t dh, uint32_t dmask,
                                                   uint32_t lds_bytes) {
  constexpr int DST = FC_TENSOR;
#include "k_convert_roi_strip_body.h"
}
template <int SRC>
__global__ __launch_bounds__(256) void k_roi_strip_nhwc(const RoiArgs args, const Yuv2RgbCoef c, uint32_t W, uint32_t dw, uint32_t dh, uint32_t dmask,
                                                   uint32_t lds_bytes) {
  constexpr int DST = FC_TENSOR_NHWC;  // one interleaved plane per job
#include "k_convert_roi_strip_body.h"
}

// ------------------------------------------------------------------------------------------
// The gather form: k_convert_resize with per-job geometry (four lanes-rows x 64 lanes x 4 pixels per workgroup).
// ------------------------------------------------------------------------------------------
template <int SRC>
__global__ __launch_bounds__(256) void k_roi_gather(const RoiArgs args, const Yuv2RgbCoef c, uint32_t dw, uint32_t dh, uint32_t dmask) {
  constexpr int DST = FC_TENSOR;
#include "k_convert_roi_gather_body.h"
}
template <int SRC>  // (four waves per SIMD asked for: the YUV420 instantiation stays within 128 VGPRs — the planar one takes 136)
__global__ __launch_bounds__(256, 4) void k_roi_gather_nhwc(const RoiArgs args, const Yuv2RgbCoef c, uint32_t dw, uint32_t dh, uint32_t dmask) {
  constexpr int DST = FC_TENSOR_NHWC;
#include "k_convert_roi_gather_body.h"
}

// ------------------------------------------------------------------------------------------
// Host side.  The strip a staged job needs is WALKED with the kernel's own fp32 tap arithmetic (vpf_lin_i0 = make_tap's i0), chunk by
// chunk and band by band, like vpf_band_rows_exact: a bound that is a row short would be silent corruption (roi_strip_need,
// vpf_job_bounds.h; tests/test_job_bounds_cpu.py).
// ------------------------------------------------------------------------------------------
hipError_t launch_convert_resize_rois(hipStream_t st, int src_fc, const Yuv2RgbCoef& c, uint32_t W, uint32_t n, const RoiDesc* jobs, uint32_t dw,
                                      uint32_t dh, const TensorEpi& te, bool nhwc) {
  if (!n || n > (uint32_t)kRoiBatch || (src_fc != FC_NV12 && src_fc != FC_YUV420 && src_fc != FC_P16)) return hipErrorInvalidValue;
  const uint32_t dmask = nhwc || te.dtype == VPF_TENSOR_F32 ? 15u : 7u;  // 4 px x element size per lane and plane: what the vector stores need (one interleaved plane: 16 B)
  // staged: the window fits a strip that leaves three workgroups per CU and converts at most three source pixels per destination pixel
  // (the measured break-even of the strip against the per-tap kernels, launch_convert_resize); everything else gathers
  const bool all_gather = tuning(VPF_TUNE_NV12_RGB_VARIANT) == 9;
  RoiArgs as, ag;  // (entries beyond a table's jobs are never read: blockIdx.z runs over its jobs)
  std::memset(&as, 0, sizeof(as));
  std::memset(&ag, 0, sizeof(ag));
  as.e = ag.e = te;  // (one interleaved plane: the staging plan of each dispatch follows below, nhwc_stage_plan)
  uint32_t ns = 0, ngat = 0, lds = 0;
  for (uint32_t i = 0; i < n; i++) {
    const RoiDesc& j = jobs[i];
    const RoiStripNeed need = all_gather ? RoiStripNeed{0u, 1e9} : roi_strip_need(j.x, j.w, j.h, j.scx, j.scy, dw, dh);
    if (!all_gather && roi_job_staged(need)) {
      as.j[ns++] = jobs[i];
      lds = need.bytes > lds ? need.bytes : lds;
    } else {
      ag.j[ngat++] = jobs[i];
    }
  }
  if (ns) {
    const dim3 grid((dw + 255) / 256, (dh + 4 * kRoiBandRows - 1) / (4 * kRoiBandRows), ns);
    const uint32_t lds_all = nhwc ? nhwc_stage_plan(te, lds, 4, &as.e) : lds;  // the strip, then the waves' staging area where both fit
#define VPF_ROIS(S) do { if (nhwc) VPF_LAUNCH((k_roi_strip_nhwc<S>), grid, dim3(256), lds_all, st, as, c, W, dw, dh, dmask, lds); \
                         else VPF_LAUNCH((k_roi_strip<S>), grid, dim3(256), lds, st, as, c, W, dw, dh, dmask, lds); } while (0)
    if (src_fc == FC_NV12) VPF_ROIS(FC_NV12); else if (src_fc == FC_P16) VPF_ROIS(FC_P16); else VPF_ROIS(FC_YUV420);
#undef VPF_ROIS
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if (ngat) {
    const dim3 grid(((dw + 3) / 4 + 63) / 64, (dh + 3) / 4, ngat);
    const uint32_t lds_g = nhwc ? nhwc_stage_plan(te, 0u, 4, &ag.e) : 0u;
#define VPF_ROIG(S) do { if (nhwc) VPF_LAUNCH((k_roi_gather_nhwc<S>), grid, dim3(256), lds_g, st, ag, c, dw, dh, dmask); \
                         else VPF_LAUNCH((k_roi_gather<S>), grid, dim3(256), 0, st, ag, c, dw, dh, dmask); } while (0)
    if (src_fc == FC_NV12) VPF_ROIG(FC_NV12); else if (src_fc == FC_P16) VPF_ROIG(FC_P16); else VPF_ROIG(FC_YUV420);
#undef VPF_ROIG
    return hipGetLastError();
  }
  return hipSuccess;
}

}  // namespace vpf
