// The body of k_warp_dev / k_warp_dev_nhwc (k_convert_warp_dev.hip), included into both with DST = FC_TENSOR / FC_TENSOR_NHWC in scope: a prologue that
// turns the device tables into the WarpDesc the host entry would have put into its job table, then k_warp_strip's own body.
  // 1. the count: jobs at or behind it write nothing and read neither matrix nor frame index
  uint32_t dv_cnt = args.max_n;
  if (args.count) {
    const int32_t v = __builtin_amdgcn_readfirstlane(*args.count);
    dv_cnt = v < 0 ? 0u : ((uint32_t)v < args.max_n ? (uint32_t)v : args.max_n);
  }
  if (blockIdx.z >= dv_cnt) return;
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
#pragma unroll
  for (int ch = 0; ch < 3; ch++) {
    J.f.d[ch] = (DST == FC_TENSOR_NHWC && ch) ? nullptr : args.d[ch] + ((size_t)blockIdx.z * args.job_stride + dv_zero);
    J.f.dp[ch] = args.dp[ch] + dv_zero;
  }
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
#include "k_convert_warp_strip_body.h"
