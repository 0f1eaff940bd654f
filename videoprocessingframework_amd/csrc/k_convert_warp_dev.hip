// k_convert_warp_dev.hip — the multi-ROI affine warp of k_convert_warp.hip with the matrices in DEVICE memory (gfx950): vpf_convert_warp_tensor_dev.
// A landmark network or an oriented-box head leaves its 2 x 3 matrices on the GPU; this kernel reads (frame, m[6]) of job blockIdx.z and the job count
// WHEN IT RUNS, so the call needs no sync and no copy to the host, and a captured graph replays with the matrices of replay time.
//   k_warp_dev / k_warp_dev_nhwc   ONE dispatch over (32 x 32 destination tiles, max_n jobs).  A workgroup loads the count (jobs at or behind it write
//                  nothing), loads its frame index and six floats wave-uniformly, runs the guard (warp_dev_job_ok, vpf_job_bounds.h: an invalid job
//                  reads no frame and writes the epilogue of the border in both modes), assembles the job as the host entry's table would hold it and
//                  runs k_warp_strip's body (k_convert_warp_strip_body.h): the tile's window from the matrix, the strip staged in LDS where it fits
//                  the bytes the dispatch was given, warp_gather4's per-tap pixels where it does not — a workgroup-uniform branch.
// Both forms run k_convert_warp.hip's fp32 operations in its order: identical bits to vpf_convert_warp_tensor on the same matrices, whichever form
// either entry picks.  The LDS is sized from the caller's hint (warp_dev_lds_bytes): a wrong hint costs time, not pixels.
#include <cmath>

#include "k_convert_warp_common.h"

namespace vpf {

// the job's four pixels of this lane filled with the border (an invalid job: both modes)
template <int DST>
VPF_DEV void warp_dev_fill4(const FrameDesc& f, const TensorEpi& te, uint32_t dw, uint32_t dmask, uint32_t x0, uint32_t y) {
  const uint32_t nv = dw - x0 < 4 ? dw - x0 : 4;
  bool vec = nv == 4;
#pragma unroll
  for (int ch = 0; ch < (DST == FC_TENSOR_NHWC ? 1 : 3); ch++) vec = vec && ((((uintptr_t)f.d[ch] | f.dp[ch]) & dmask) == 0);
  float u[3][4];
#pragma unroll
  for (int ch = 0; ch < 3; ch++)
#pragma unroll
    for (int k = 0; k < 4; k++) u[ch][k] = warp_border(te, ch);
  warp_store4<DST>(f, x0, y, u, te, vec, nv);
}

template <int SRC>
__global__ __launch_bounds__(256) void k_warp_dev(const WarpDevArgs args, const Yuv2RgbCoef c, uint32_t W, uint32_t H, uint32_t dw, uint32_t dh,
                                                  uint32_t dmask, uint32_t lds_bytes) {
  constexpr int DST = FC_TENSOR;
#include "k_convert_warp_dev_body.h"
}
template <int SRC>
__global__ __launch_bounds__(256) void k_warp_dev_nhwc(const WarpDevArgs args, const Yuv2RgbCoef c, uint32_t W, uint32_t H, uint32_t dw, uint32_t dh,
                                                       uint32_t dmask, uint32_t lds_bytes) {
  constexpr int DST = FC_TENSOR_NHWC;  // one interleaved plane per job
#include "k_convert_warp_dev_body.h"
}

// ------------------------------------------------------------------------------------------
// Host side.  No matrix is known here: the dynamic LDS comes from the caller's hint (warp_dev_lds_bytes; no hint: kWarpStripMax), 0 under
// VPF_TUNE_NV12_RGB_VARIANT = 9 — no strip fits then, every tile samples per tap.
// ------------------------------------------------------------------------------------------
hipError_t launch_convert_warp_dev(hipStream_t st, int src_fc, const Yuv2RgbCoef& c, uint32_t W, uint32_t H, WarpDevArgs& a, uint32_t dw, uint32_t dh,
                                   float max_step, const TensorEpi& te, bool nhwc) {
  if (!a.max_n || a.max_n > 65535u || !a.n_frames || a.n_frames > (uint32_t)kRoiDevFrames || (src_fc != FC_NV12 && src_fc != FC_YUV420 && src_fc != FC_P16))
    return hipErrorInvalidValue;
  const uint32_t dmask = nhwc || te.dtype == VPF_TENSOR_F32 ? 15u : 7u;  // 4 px x element size per lane and plane: what the vector stores need (one interleaved plane: 16 B)
  const uint32_t lds = tuning(VPF_TUNE_NV12_RGB_VARIANT) == 9 ? 0u : warp_dev_lds_bytes(max_step, W, H, dw, dh);
  a.e = te;
  const dim3 grid((dw + kWarpTileW - 1) / kWarpTileW, (dh + kWarpTileH - 1) / kWarpTileH, a.max_n);
#define VPF_WARPD(S) do { if (nhwc) VPF_LAUNCH((k_warp_dev_nhwc<S>), grid, dim3(256), lds, st, a, c, W, H, dw, dh, dmask, lds); \
                          else VPF_LAUNCH((k_warp_dev<S>), grid, dim3(256), lds, st, a, c, W, H, dw, dh, dmask, lds); } while (0)
  if (src_fc == FC_NV12) VPF_WARPD(FC_NV12); else if (src_fc == FC_P16) VPF_WARPD(FC_P16); else VPF_WARPD(FC_YUV420);
#undef VPF_WARPD
  return hipGetLastError();
}

}  // namespace vpf
