// k_convert_warp_dev.hip — the multi-ROI affine warp of k_convert_warp.hip with the matrices in DEVICE memory (gfx950): vpf_convert_warp_tensor_dev.
// A landmark network or an oriented-box head leaves its 2 x 3 matrices on the GPU; this kernel reads (frame, m[6]) of job blockIdx.z and the job count
// WHEN IT RUNS, so the call needs no sync and no copy to the host, and a captured graph replays with the matrices of replay time.
//   k_warp_dev     ONE dispatch over (32 x 32 destination tiles, max_n jobs).  A workgroup loads the count (jobs at or behind it write
//                  nothing), loads its frame index and six floats wave-uniformly, runs the guard (warp_dev_job_ok, vpf_job_bounds.h: an invalid job
//                  reads no frame and writes the epilogue of the border in both modes), assembles the job as the host entry's table would hold it and
//                  runs k_warp_strip's tile (warp_strip_tile, k_convert_warp_common.h): the tile's window from the matrix, the strip staged in LDS where it fits
//                  the bytes the dispatch was given, warp_gather4's per-tap pixels where it does not — a workgroup-uniform branch.
// Both forms run k_convert_warp.hip's fp32 operations in its order: identical bits to vpf_convert_warp_tensor on the same matrices, whichever form
// either entry picks.  The LDS is sized from the caller's hint (warp_dev_lds_bytes): a wrong hint costs time, not pixels.
#include <cmath>

#include "k_convert_warp_common.h"
#include "k_dev_table.h"
#include "k_job_launch.h"

namespace vpf {

// the job's four pixels of this lane filled with the border (an invalid job: both modes)
template <int DST>
VPF_DEV void warp_dev_fill4(const FrameDesc& f, const TensorEpi& te, uint32_t dw, uint32_t dmask, uint32_t x0, uint32_t y) {
  const uint32_t nv = dw - x0 < 4 ? dw - x0 : 4;
  const bool vec = tensor_vec_ok<DST>(f, nv, dmask);
  float u[3][4];
#pragma unroll
  for (int ch = 0; ch < 3; ch++)
#pragma unroll
    for (int k = 0; k < 4; k++) u[ch][k] = warp_border(te, ch);
  warp_store4<DST>(f, x0, y, u, te, vec, nv);
}

template <int SRC, int DST>  // DST = FC_TENSOR: three planes per job; FC_TENSOR_NHWC: one interleaved plane
__global__ __launch_bounds__(256) void k_warp_dev(const WarpDevArgs args, const Yuv2RgbCoef c, uint32_t W, uint32_t H, uint32_t dw, uint32_t dh,
                                                  uint32_t dmask, uint32_t lds_bytes) {
  // a prologue that turns the device tables into the WarpDesc the host entry would have put into its job table, then k_warp_strip's tile
  // 1. the count: jobs at or behind it write nothing and read neither matrix nor frame index
  if (blockIdx.z >= dev_job_count(args.count, args.max_n)) return;
  // 2. the frame index and the six floats of this job, wave-uniform: the window arithmetic below stays scalar
  WarpDesc J;
  int32_t dv_frame = 0;
  if (args.frame_index)
    dv_frame = __builtin_amdgcn_readfirstlane(
        *reinterpret_cast<const int32_t*>(reinterpret_cast<const uint8_t*>(args.frame_index) + (size_t)blockIdx.z * args.frame_stride));
  {
    const uint32_t* const mp = reinterpret_cast<const uint32_t*>(reinterpret_cast<const uint8_t*>(args.matrices) + (size_t)blockIdx.z * args.matrix_stride);
#pragma unroll
    for (int k = 0; k < 6; k++) J.m[k] = __uint_as_float(__builtin_amdgcn_readfirstlane(mp[k]));
  }
  // the job's destination planes and every pitch live in vector registers (an opaque zero added to them): they feed per-lane addresses only, and the
  // matrix read above — which, unlike a job table in the kernel arguments, cannot be loaded again where it is used — needs their scalar registers:
  // without this the planar kernels spill 8 - 13 scalar registers
  uint32_t dv_zero = 0;
  asm("" : "+v"(dv_zero));
  dev_dst_planes<DST>(args, blockIdx.z, J.f, dv_zero);
  // 3. the guard (vpf_job_bounds.h): an invalid job reads no frame; its tile takes the epilogue of the border, in both modes
  if (!warp_dev_job_ok(dv_frame, J.m, args.n_frames)) {
    const uint32_t fx0 = blockIdx.x * kWarpTileW + (threadIdx.x % kWarpLanesX) * 4, fy = blockIdx.y * kWarpTileH + threadIdx.x / kWarpLanesX;
    if (fx0 < dw && fy < dh) warp_dev_fill4<DST>(J.f, args.e, dw, dmask, fx0, fy);
    return;
  }
  // 4. the job as the host entry's table holds it
  {
    const FrameSrcDesc& fs = args.f[dv_frame];
#pragma unroll
    for (int ch = 0; ch < 3; ch++) { J.f.s[ch] = fs.s[ch]; J.f.sp[ch] = fs.sp[ch] + dv_zero; }
  }
  // 5. k_warp_strip from here on: the tile's window, staged where its strip fits lds_bytes, per tap where it does not
  const TensorEpi te = args.e;
  warp_strip_tile<SRC, DST>(J, te, c, W, H, dw, dh, dmask, lds_bytes);
}

// ------------------------------------------------------------------------------------------
// Host side.  No matrix is known here: job_plan (vpf_job_plan.h) sizes the ONE dispatch's LDS from the caller's hint (warp_dev_lds_bytes,
// vpf_job_bounds.h; no hint: kWarpStripMax), nothing under VPF_TUNE_NV12_RGB_VARIANT = 9 — no strip fits then, every tile samples per tap.
// ------------------------------------------------------------------------------------------
hipError_t launch_convert_warp_dev(hipStream_t st, int src_fc, const Yuv2RgbCoef& c, uint32_t W, uint32_t H, WarpDevArgs& a, uint32_t dw, uint32_t dh,
                                   float max_step, const TensorEpi& te, bool nhwc) {
  JobShape q;
  job_shape(q, JOB_WARP, true, src_fc, nhwc, te, W, H, dw, dh);
  job_shape_dev(q, a.max_n, a.n_frames, max_step);
  const JobPlan p = job_plan(q);
  if (!p.ok) return hipErrorInvalidValue;
  const JobDispatch& d = p.d[0];
  const dim3 grid(d.gx, d.gy, d.n);
  const uint32_t lds_all = job_launch_lds(d, te, a);  // (sets a.e)
  hipError_t e = hipSuccess;
  with_src_dst(src_fc, nhwc, [&](auto S, auto D) { VPF_LAUNCH_T(k_warp_dev, (S, D), grid, lds_all, st, a, c, W, H, dw, dh, p.dmask, d.lds); e = hipGetLastError(); });
  return e;
}

}  // namespace vpf
