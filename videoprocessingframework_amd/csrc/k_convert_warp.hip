// k_convert_warp.hip — fused multi-ROI affine warp of NV12 / YUV420 into a normalised planar tensor (gfx950): vpf_convert_warp_tensor.
// One dispatch serves many jobs; a job = (whole source frame, inverse 2 x 3 matrix, three destination planes) (WarpDesc, vpf_internal.h).
// Grid = (destination tiles of 32 x 32, job); a lane owns four consecutive pixels of one row, a workgroup 8 lanes x 32 rows.
//   k_warp_strip    the staged form: the workgroup takes the bounding box of its tile's taps from the tile's four corners, converts that
//                   source window once into an LDS strip of four-byte RGB pixels (VPF_STRIP_FILL_WINDOW, the fill stage of k_roi_strip) and
//                   blends every pixel from bytes at per-pixel taps
//   k_warp_gather   per-tap texel_rgb: jobs whose tile windows do not fit 64 KiB of LDS (large down-scales), VPF_TUNE_NV12_RGB_VARIANT = 9
// Definition (include/vpf_hip.h): sx = (m00 dx + m01 dy) + m02, sy likewise, every operation rounded on its own (-ffp-contract=off), then
// vpf_remap's range test and sampling on frame pixels converted with vpf_convert's arithmetic, bilerp, truncation, the tensor epilogue.
// Both kernels run exactly those fp32 operations in that order: identical bits.
// P10 / P12 frames (FC_P16) take the same two kernels: their 16-bit samples are narrowed to 8 bits at the load (k_fused_common.h).
#include <cmath>

#include "k_convert_warp_common.h"

namespace vpf {

// The tile (kWarpTileW x kWarpTileH), the coordinates (warp_xy), a tile's source window and strip (warp_window, warp_strip) and the launcher's bound
// (warp_need, kWarpStripMax) stand in vpf_job_bounds.h: host, device and the CPU property test (tests/test_job_bounds_cpu.py) share them.

// warp_rep, warp_border, warp_store4 and warp_gather4 (the per-tap form of a lane's four pixels) stand in k_convert_warp_common.h: the device-table
// kernel (k_convert_warp_dev.hip) runs them too.

// ------------------------------------------------------------------------------------------
// The staged form.  The window is wave-uniform (block indices and kernel arguments only).  A tile whose window is empty writes the border; a
// tile whose strip would not fit the LDS it was given — never: the launcher's bound covers every tile (warp_need) — takes the per-tap
// form instead of writing from a short strip.
// ------------------------------------------------------------------------------------------
// (DST = FC_TENSOR: three planes per job, k_warp_strip; FC_TENSOR_NHWC: one interleaved plane, k_warp_strip_nhwc)
template <int SRC>
__global__ __launch_bounds__(256) void k_warp_strip(const WarpArgs args, const Yuv2RgbCoef c, uint32_t W, uint32_t H, uint32_t dw, uint32_t dh,
                                                    uint32_t dmask, uint32_t lds_bytes) {
  constexpr int DST = FC_TENSOR;
  const WarpDesc& J = args.j[blockIdx.z];
#include "k_convert_warp_strip_body.h"
}
template <int SRC>
__global__ __launch_bounds__(256) void k_warp_strip_nhwc(const WarpArgs args, const Yuv2RgbCoef c, uint32_t W, uint32_t H, uint32_t dw, uint32_t dh,
                                                    uint32_t dmask, uint32_t lds_bytes) {
  constexpr int DST = FC_TENSOR_NHWC;  // one interleaved plane per job
  const WarpDesc& J = args.j[blockIdx.z];
#include "k_convert_warp_strip_body.h"
}

// ------------------------------------------------------------------------------------------
// The gather form: the same tile and lane assignment, four texel_rgb per pixel.
// ------------------------------------------------------------------------------------------
template <int SRC>
__global__ __launch_bounds__(256) void k_warp_gather(const WarpArgs args, const Yuv2RgbCoef c, uint32_t W, uint32_t H, uint32_t dw, uint32_t dh,
                                                     uint32_t dmask) {
  const uint32_t x0 = blockIdx.x * kWarpTileW + (threadIdx.x % kWarpLanesX) * 4, y = blockIdx.y * kWarpTileH + threadIdx.x / kWarpLanesX;
  if (x0 >= dw || y >= dh) return;
  warp_gather4<SRC>(args.j[blockIdx.z], c, args.e, W, H, dw, dmask, x0, y);
}
template <int SRC>
__global__ __launch_bounds__(256) void k_warp_gather_nhwc(const WarpArgs args, const Yuv2RgbCoef c, uint32_t W, uint32_t H, uint32_t dw, uint32_t dh,
                                                          uint32_t dmask) {
  const uint32_t x0 = blockIdx.x * kWarpTileW + (threadIdx.x % kWarpLanesX) * 4, y = blockIdx.y * kWarpTileH + threadIdx.x / kWarpLanesX;
  if (x0 >= dw || y >= dh) return;
  warp_gather4<SRC, FC_TENSOR_NHWC>(args.j[blockIdx.z], c, args.e, W, H, dw, dmask, x0, y);
}

// ------------------------------------------------------------------------------------------
// Host side.  The dynamic LDS of a dispatch is an UPPER BOUND of every tile's strip, from the matrix alone, O(1) per job: warp_need and the
// policy's limit kWarpStripMax, vpf_job_bounds.h.
// ------------------------------------------------------------------------------------------
hipError_t launch_convert_warp(hipStream_t st, int src_fc, const Yuv2RgbCoef& c, uint32_t W, uint32_t H, uint32_t n, const WarpDesc* jobs, uint32_t dw,
                               uint32_t dh, const TensorEpi& te, bool nhwc) {
  if (!n || n > (uint32_t)kWarpBatch || (src_fc != FC_NV12 && src_fc != FC_YUV420 && src_fc != FC_P16)) return hipErrorInvalidValue;
  const uint32_t dmask = nhwc || te.dtype == VPF_TENSOR_F32 ? 15u : 7u;  // 4 px x element size per lane and plane: what the vector stores need (one interleaved plane: 16 B)
  const int tune = tuning(VPF_TUNE_NV12_RGB_VARIANT);
  const bool all_gather = tune == 9;
  WarpArgs as, ag;  // (entries beyond a table's jobs are never read: blockIdx.z runs over its jobs)
  std::memset(&as, 0, sizeof(as));
  std::memset(&ag, 0, sizeof(ag));
  as.e = ag.e = te;
  uint32_t ns = 0, ngat = 0, lds = 0;
  for (uint32_t i = 0; i < n; i++) {
    const WarpNeed need = all_gather ? WarpNeed{0u} : warp_need(jobs[i].m, W, H, dw, dh);
    if (!all_gather && need.bytes <= kWarpStripMax) {
      as.j[ns++] = jobs[i];
      lds = need.bytes > lds ? need.bytes : lds;
    } else {
      ag.j[ngat++] = jobs[i];
    }
  }
  const uint32_t gx = (dw + kWarpTileW - 1) / kWarpTileW, gy = (dh + kWarpTileH - 1) / kWarpTileH;
  if (ns) {
#define VPF_WARPS(S) do { if (nhwc) VPF_LAUNCH((k_warp_strip_nhwc<S>), dim3(gx, gy, ns), dim3(256), lds, st, as, c, W, H, dw, dh, dmask, lds); \
                          else VPF_LAUNCH((k_warp_strip<S>), dim3(gx, gy, ns), dim3(256), lds, st, as, c, W, H, dw, dh, dmask, lds); } while (0)
    if (src_fc == FC_NV12) VPF_WARPS(FC_NV12); else if (src_fc == FC_P16) VPF_WARPS(FC_P16); else VPF_WARPS(FC_YUV420);
#undef VPF_WARPS
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if (ngat) {
#define VPF_WARPG(S) do { if (nhwc) VPF_LAUNCH((k_warp_gather_nhwc<S>), dim3(gx, gy, ngat), dim3(256), 0, st, ag, c, W, H, dw, dh, dmask); \
                          else VPF_LAUNCH((k_warp_gather<S>), dim3(gx, gy, ngat), dim3(256), 0, st, ag, c, W, H, dw, dh, dmask); } while (0)
    if (src_fc == FC_NV12) VPF_WARPG(FC_NV12); else if (src_fc == FC_P16) VPF_WARPG(FC_P16); else VPF_WARPG(FC_YUV420);
#undef VPF_WARPG
    return hipGetLastError();
  }
  return hipSuccess;
}

}  // namespace vpf
