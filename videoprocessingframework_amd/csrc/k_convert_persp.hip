// k_convert_persp.hip — fused multi-ROI perspective warp (3 x 3 homography) of NV12 / YUV420 / P10 / P12 into a normalised tensor (gfx950):
// vpf_convert_persp_tensor.  The affine entry's tile, lane assignment, strip, blend and epilogue (k_convert_warp.hip); the coordinates are new.
// Grid = (destination tiles of 32 x 32, job); a lane owns four consecutive pixels of one row, a workgroup 8 lanes x 32 rows.
//   k_persp_strip    the staged form.  A tile whose four corners have w > 0 (then every pixel has: w is rounded-affine, monotone along both axes)
//                    converts the corners' bounding box, one pixel wider per side, into an LDS strip of four-byte RGB pixels
//                    (strip_fill_window), one barrier, and blends from bytes.  Every in-range pixel tests its taps against that window
//                    (persp_px_in_window): fl(fl(nx) / fl(w)) is not monotone, so the corner box is a guess; a pixel outside it is sampled per tap.
//                    A tile the horizon crosses or touches samples per tap; one wholly behind the plane writes the border; one whose strip exceeds
//                    the LDS of the dispatch samples per tap.  All workgroup-uniform branches.
//   k_persp_gather   per-tap texel_rgb: jobs whose bound (persp_need) exceeds 64 KiB of LDS, VPF_TUNE_NV12_RGB_VARIANT = 9
// Definition (include/vpf_hip.h): nx, ny, w rounded-affine, sx = nx / w, sy = ny / w as IEEE divisions (the compiler's v_div_scale / v_div_fmas /
// v_div_fixup sequence: correctly rounded, denormals kept; never v_rcp_f32 and a multiply), !(w > 0) -> border; from the range test on the affine
// entry.  Both kernels run exactly those fp32 operations in that order (-ffp-contract=off): identical bits.
#include <cmath>

#include "k_convert_warp_common.h"
#include "k_job_launch.h"

namespace vpf {

// ------------------------------------------------------------------------------------------
// The staged form (DST = FC_TENSOR: three planes per job; FC_TENSOR_NHWC: one interleaved plane): persp_strip_tile, k_convert_warp_common.h — the
// device-table kernel (k_convert_persp_dev.hip) runs it too, as persp_tap and persp_gather4 of the gather form.  What differs from the affine kernel
// (k_warp_strip): the tile's class (persp_window: border, per tap, nothing staged, staged), and the per-pixel test of an in-range pixel's taps against
// the window the tile staged (persp_px_in_window) — the affine kernel's "an in-range coordinate lies inside the window" does not hold for a rounded
// quotient, so a pixel that fails the test is sampled per tap instead of being pulled into the window.
// ------------------------------------------------------------------------------------------
template <int SRC, int DST>
__global__ __launch_bounds__(256) void k_persp_strip(const PerspArgs args, const Yuv2RgbCoef c, uint32_t W, uint32_t H, uint32_t dw, uint32_t dh,
                                                     uint32_t dmask, uint32_t lds_bytes) {
  const TensorEpi te = args.e;
  persp_strip_tile<SRC, DST>(args.j[blockIdx.z], te, c, W, H, dw, dh, dmask, lds_bytes);
}

// ------------------------------------------------------------------------------------------
// The gather form: the same tile and lane assignment, four texel_rgb per pixel.
// ------------------------------------------------------------------------------------------
template <int SRC, int DST>
__global__ __launch_bounds__(256) void k_persp_gather(const PerspArgs args, const Yuv2RgbCoef c, uint32_t W, uint32_t H, uint32_t dw, uint32_t dh,
                                                      uint32_t dmask) {
  const uint32_t x0 = blockIdx.x * kWarpTileW + (threadIdx.x % kWarpLanesX) * 4, y = blockIdx.y * kWarpTileH + threadIdx.x / kWarpLanesX;
  if (x0 >= dw || y >= dh) return;
  persp_gather4<SRC, DST>(args.j[blockIdx.z], c, args.e, W, H, dw, dmask, x0, y);
}

// ------------------------------------------------------------------------------------------
// Host side: launch_convert_warp with the perspective family of job_plan (vpf_job_plan.h, where the reason for two dispatches per table stands):
// persp_need against kWarpStripMax (vpf_job_bounds.h).
// ------------------------------------------------------------------------------------------
hipError_t launch_convert_persp(hipStream_t st, int src_fc, const Yuv2RgbCoef& c, uint32_t W, uint32_t H, uint32_t n, const PerspDesc* jobs, uint32_t dw,
                                uint32_t dh, const TensorEpi& te, bool nhwc) {
  JobShape q;
  job_shape(q, JOB_PERSP, false, src_fc, nhwc, te, W, H, dw, dh);
  job_shape_jobs(q, jobs, n, [](JobGeom& g, const PerspDesc& j) { for (int k = 0; k < 9; k++) g.m[k] = j.m[k]; });
  const JobPlan p = job_plan(q);
  if (!p.ok) return hipErrorInvalidValue;
  PerspArgs t[2];
  fill_job_tables(p, jobs, n, te, t);
  hipError_t e = hipSuccess;
  for (int k = 0; k < p.nd && e == hipSuccess; k++) {  // staged first; its error returns before the per-tap launch
    const JobDispatch& d = p.d[k];
    const dim3 grid(d.gx, d.gy, d.n);
    const uint32_t lds_all = job_launch_lds(d, te, t[k]);
    with_src_dst(src_fc, nhwc, [&](auto S, auto D) {
      if (d.form == JF_PERSP_STRIP) VPF_LAUNCH_T(k_persp_strip, (S, D), grid, lds_all, st, t[k], c, W, H, dw, dh, p.dmask, d.lds);
      else VPF_LAUNCH_T(k_persp_gather, (S, D), grid, lds_all, st, t[k], c, W, H, dw, dh, p.dmask);
      e = hipGetLastError();
    });
  }
  return e;
}

}  // namespace vpf
