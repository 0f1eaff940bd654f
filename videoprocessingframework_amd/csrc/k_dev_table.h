// k_dev_table.h — the prologue the device-table kernels share (k_roi_dev, k_lb_dev, k_warp_dev, k_persp_dev): the job count, the five ints of a box,
// the job's destination planes; and the wave-uniform form of a tile's window (k_roi_dev, k_lb_dev), which the host-table kernel k_roi_strip takes as well.
// Forced inline; every value read from a table is wave-uniform (readfirstlane), so the arithmetic on it stays scalar.
#ifndef VPF_K_DEV_TABLE_H_
#define VPF_K_DEV_TABLE_H_
#include "vpf_device.h"
#include "vpf_internal.h"
#include "vpf_job_bounds.h"

namespace vpf {

// the number of jobs of this dispatch: the device's count clamped to 0 .. max_n, max_n where there is none.  Jobs at or behind it write nothing.
VPF_DEV uint32_t dev_job_count(const int32_t* count, uint32_t max_n) {
  uint32_t cnt = max_n;
  if (count) {
    const int32_t v = __builtin_amdgcn_readfirstlane(*count);
    cnt = v < 0 ? 0u : ((uint32_t)v < max_n ? (uint32_t)v : max_n);
  }
  return cnt;
}
// the five untrusted ints (frame, x, y, w, h) of a job, `stride` bytes apart
struct DevBox5 { int32_t f, x, y, w, h; };
VPF_DEV DevBox5 dev_box5(const int32_t* boxes, uint32_t stride, uint32_t job) {
  const int32_t* const bp = reinterpret_cast<const int32_t*>(reinterpret_cast<const uint8_t*>(boxes) + (size_t)job * stride);
  return DevBox5{__builtin_amdgcn_readfirstlane(bp[0]), __builtin_amdgcn_readfirstlane(bp[1]), __builtin_amdgcn_readfirstlane(bp[2]),
                 __builtin_amdgcn_readfirstlane(bp[3]), __builtin_amdgcn_readfirstlane(bp[4])};
}
// the destination planes and pitches of a job (args: d[3], job_stride, dp[3]).  `zero`: the warp kernels' opaque per-lane zero, which moves planes
// and pitches to vector registers; the others pass none
template <int DST, class Args>
VPF_DEV void dev_dst_planes(const Args& args, uint32_t job, FrameDesc& f, uint32_t zero = 0u) {
#pragma unroll
  for (int ch = 0; ch < 3; ch++) {
    f.d[ch] = (DST == FC_TENSOR_NHWC && ch) ? nullptr : args.d[ch] + ((size_t)job * args.job_stride + zero);
    f.dp[ch] = args.dp[ch] + zero;
  }
}
// A tile's window (roi_tile_window, letterbox_tile_window) depends on block indices and the job alone: its four values as wave-uniform ones, the
// strip's layout derived from them again
VPF_DEV void tile_window_uniform(RoiTileWin& win) {
  win.first = __builtin_amdgcn_readfirstlane(win.first); win.last = __builtin_amdgcn_readfirstlane(win.last);
  win.lo = __builtin_amdgcn_readfirstlane(win.lo); win.hi = __builtin_amdgcn_readfirstlane(win.hi);
  win.base_px = win.first & ~1u; win.ng = ((win.last - win.base_px) >> 3) + 1u; win.rowbytes = 32u * win.ng + 16u; win.rows = win.hi - win.lo + 1u;
}

}  // namespace vpf
#endif  // VPF_K_DEV_TABLE_H_
