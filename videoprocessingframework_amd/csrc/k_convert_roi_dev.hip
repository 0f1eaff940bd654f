// k_convert_roi_dev.hip — the multi-ROI crop + bilinear resize of k_convert_roi.hip with the rectangles in DEVICE memory (gfx950):
// vpf_convert_resize_tensor_rois_dev.  A detector and its NMS leave their boxes on the GPU; this kernel reads (frame, x, y, w, h) of job blockIdx.z and
// the job count WHEN IT RUNS, so the call needs no sync and no copy to the host, and a captured graph replays with the boxes of replay time.
//   k_roi_dev / k_roi_dev_nhwc   ONE dispatch over (tiles of 16 destination rows x 256 columns, max_n jobs).  A workgroup loads the count (jobs at or
//                  behind it write nothing), loads its box, runs the guard (roi_dev_box_ok: an invalid box reads no frame and writes the epilogue
//                  of byte 0), computes the job's scale factors — the correctly rounded fp32 quotients the host entry computes: no fast-math, no
//                  contraction in this translation unit — and then decides for ITS TILE (roi_tile_need, vpf_job_bounds.h): the staged form of
//                  k_roi_strip where the tile's strip fits the dispatch's LDS and converts at most kRoiConvMax source pixels per destination
//                  pixel, k_roi_gather's per-tap pixel otherwise.  A workgroup-uniform branch, as in k_warp_strip.
// Both forms run k_convert_roi.hip's fp32 operations in its order (VPF_STRIP_FILL_WINDOW, band_blend_rows, texel_rgb, the tensor_store4* epilogues):
// identical bits to vpf_convert_resize_tensor_rois on the same rectangles, whichever form either entry picks.
#include "k_bilinear_blend.h"
#include "k_fused_common.h"
#include "vpf_job_bounds.h"  // roi_dev_box_ok, roi_tile_window, roi_tile_need_of, roi_tile_staged: shared with the CPU tests

namespace vpf {

template <int SRC>
__global__ __launch_bounds__(256) void k_roi_dev(const RoiDevArgs args, const Yuv2RgbCoef c, uint32_t W, uint32_t H, uint32_t dw, uint32_t dh, uint32_t dmask,
                                                 uint32_t lds_bytes) {
  constexpr int DST = FC_TENSOR;
#include "k_convert_roi_dev_body.h"
}
template <int SRC>
__global__ __launch_bounds__(256) void k_roi_dev_nhwc(const RoiDevArgs args, const Yuv2RgbCoef c, uint32_t W, uint32_t H, uint32_t dw, uint32_t dh,
                                                      uint32_t dmask, uint32_t lds_bytes) {
  constexpr int DST = FC_TENSOR_NHWC;  // one interleaved plane per job
#include "k_convert_roi_dev_body.h"
}

// ------------------------------------------------------------------------------------------
// Host side.  No rectangle is known here: the dynamic LDS is the most a staged tile of this destination size can need (roi_dev_lds_bytes: the
// conversion limit bounds the strip), 0 under VPF_TUNE_NV12_RGB_VARIANT = 9 — no strip fits then, every tile samples per tap.
// ------------------------------------------------------------------------------------------
hipError_t launch_convert_resize_rois_dev(hipStream_t st, int src_fc, const Yuv2RgbCoef& c, uint32_t W, uint32_t H, RoiDevArgs& a, uint32_t dw, uint32_t dh,
                                          const TensorEpi& te, bool nhwc) {
  if (!a.max_n || a.max_n > 65535u || !a.n_frames || a.n_frames > (uint32_t)kRoiDevFrames || (src_fc != FC_NV12 && src_fc != FC_YUV420 && src_fc != FC_P16))
    return hipErrorInvalidValue;
  const uint32_t dmask = nhwc || te.dtype == VPF_TENSOR_F32 ? 15u : 7u;  // 4 px x element size per lane and plane: what the vector stores need (one interleaved plane: 16 B)
  const uint32_t lds = tuning(VPF_TUNE_NV12_RGB_VARIANT) == 9 ? 0u : roi_dev_lds_bytes(dw, dh);
  a.e = te;
  const uint32_t lds_all = nhwc ? nhwc_stage_plan(te, lds, 4, &a.e) : lds;  // the strip, then the waves' staging area where both fit
  const dim3 grid((dw + 255) / 256, (dh + 4 * kRoiBandRows - 1) / (4 * kRoiBandRows), a.max_n);
#define VPF_ROID(S) do { if (nhwc) VPF_LAUNCH((k_roi_dev_nhwc<S>), grid, dim3(256), lds_all, st, a, c, W, H, dw, dh, dmask, lds); \
                         else VPF_LAUNCH((k_roi_dev<S>), grid, dim3(256), lds_all, st, a, c, W, H, dw, dh, dmask, lds); } while (0)
  if (src_fc == FC_NV12) VPF_ROID(FC_NV12); else if (src_fc == FC_P16) VPF_ROID(FC_P16); else VPF_ROID(FC_YUV420);
#undef VPF_ROID
  return hipGetLastError();
}

}  // namespace vpf
