// k_convert_warp.hip — fused multi-ROI affine warp of NV12 / YUV420 into a normalised planar tensor (gfx950): vpf_convert_warp_tensor.
// One dispatch serves many jobs; a job = (whole source frame, inverse 2 x 3 matrix, three destination planes) (WarpDesc, vpf_internal.h).
// Grid = (destination tiles of 32 x 32, job); a lane owns four consecutive pixels of one row, a workgroup 8 lanes x 32 rows.
//   k_warp_strip    the staged form: the workgroup takes the bounding box of its tile's taps from the tile's four corners, converts that
//                   source window once into an LDS strip of four-byte RGB pixels (strip_fill_window, the fill stage of k_roi_strip) and
//                   blends every pixel from bytes at per-pixel taps
//   k_warp_gather   per-tap texel_rgb: jobs whose tile windows do not fit 64 KiB of LDS (large down-scales), VPF_TUNE_NV12_RGB_VARIANT = 9
// Definition (include/vpf_hip.h): sx = (m00 dx + m01 dy) + m02, sy likewise, every operation rounded on its own (-ffp-contract=off), then
// vpf_remap's range test and sampling on frame pixels converted with vpf_convert's arithmetic, bilerp, truncation, the tensor epilogue.
// Both kernels run exactly those fp32 operations in that order: identical bits.
// P10 / P12 frames (FC_P16) take the same two kernels: their 16-bit samples are narrowed to 8 bits at the load (k_fused_common.h).
#include <cmath>

#include "k_convert_warp_common.h"
#include "k_job_launch.h"

namespace vpf {

// The tile (kWarpTileW x kWarpTileH), the coordinates (warp_xy), a tile's source window and strip (warp_window, warp_strip) and the bound of a job's
// strip (warp_need, kWarpStripMax) stand in vpf_job_bounds.h: host, device and the CPU property test (tests/test_job_bounds_cpu.py) share them; the
// launch policy that applies the bound is job_plan (vpf_job_plan.h).

// warp_rep, warp_border, warp_store4, warp_gather4 (the per-tap form of a lane's four pixels) and warp_strip_tile (the staged form of a workgroup's
// tile) stand in k_convert_warp_common.h: the device-table kernel (k_convert_warp_dev.hip) runs them too.

template <int SRC, int DST>  // DST = FC_TENSOR: three planes per job; FC_TENSOR_NHWC: one interleaved plane
__global__ __launch_bounds__(256) void k_warp_strip(const WarpArgs args, const Yuv2RgbCoef c, uint32_t W, uint32_t H, uint32_t dw, uint32_t dh,
                                                    uint32_t dmask, uint32_t lds_bytes) {
  const TensorEpi te = args.e;
  warp_strip_tile<SRC, DST>(args.j[blockIdx.z], te, c, W, H, dw, dh, dmask, lds_bytes);
}

// ------------------------------------------------------------------------------------------
// The gather form: the same tile and lane assignment, four texel_rgb per pixel.
// ------------------------------------------------------------------------------------------
template <int SRC, int DST>
__global__ __launch_bounds__(256) void k_warp_gather(const WarpArgs args, const Yuv2RgbCoef c, uint32_t W, uint32_t H, uint32_t dw, uint32_t dh,
                                                     uint32_t dmask) {
  const uint32_t x0 = blockIdx.x * kWarpTileW + (threadIdx.x % kWarpLanesX) * 4, y = blockIdx.y * kWarpTileH + threadIdx.x / kWarpLanesX;
  if (x0 >= dw || y >= dh) return;
  warp_gather4<SRC, DST>(args.j[blockIdx.z], c, args.e, W, H, dw, dmask, x0, y);
}

// ------------------------------------------------------------------------------------------
// Host side: fill the shape, ask job_plan (vpf_job_plan.h: the cap, staged or per tap per job — warp_need against kWarpStripMax, vpf_job_bounds.h —,
// the tile grid, the strip's bytes), fill the two tables from it and launch what it names.
// ------------------------------------------------------------------------------------------
hipError_t launch_convert_warp(hipStream_t st, int src_fc, const Yuv2RgbCoef& c, uint32_t W, uint32_t H, uint32_t n, const WarpDesc* jobs, uint32_t dw,
                               uint32_t dh, const TensorEpi& te, bool nhwc) {
  JobShape q;
  job_shape(q, JOB_WARP, false, src_fc, nhwc, te, W, H, dw, dh);
  job_shape_jobs(q, jobs, n, [](JobGeom& g, const WarpDesc& j) { for (int k = 0; k < 6; k++) g.m[k] = j.m[k]; });
  const JobPlan p = job_plan(q);
  if (!p.ok) return hipErrorInvalidValue;
  WarpArgs t[2];
  fill_job_tables(p, jobs, n, te, t);
  hipError_t e = hipSuccess;
  for (int k = 0; k < p.nd && e == hipSuccess; k++) {  // staged first; its error returns before the per-tap launch
    const JobDispatch& d = p.d[k];
    const dim3 grid(d.gx, d.gy, d.n);
    const uint32_t lds_all = job_launch_lds(d, te, t[k]);
    with_src_dst(src_fc, nhwc, [&](auto S, auto D) {
      if (d.form == JF_WARP_STRIP) VPF_LAUNCH_T(k_warp_strip, (S, D), grid, lds_all, st, t[k], c, W, H, dw, dh, p.dmask, d.lds);
      else VPF_LAUNCH_T(k_warp_gather, (S, D), grid, lds_all, st, t[k], c, W, H, dw, dh, p.dmask);
      e = hipGetLastError();
    });
  }
  return e;
}

}  // namespace vpf
