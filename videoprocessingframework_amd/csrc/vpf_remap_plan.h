// vpf_remap_plan.h — the launch of the per-pixel remap into a tensor (vpf_convert_remap_tensor, launch_convert_remap of k_convert_remap.hip) as one
// pure function: the refusal, or the ONE dispatch of a job table — its grid, the jobs a table holds, the strip bytes the kernel is told and the
// destination alignment mask.  No HIP in here: the launcher includes it and only dispatches on the result, and tests/test_remap_tensor_cpu.py
// compiles the same header with g++ (tests/c/remap_bounds_capi.cpp).  A sibling of job_plan (vpf_job_plan.h), not a family of it: the host never sees
// a coordinate, so there is nothing to decide per job — staged, per tap or border is the kernel's decision per tile, from the exact window of the
// coordinates it loaded (remap_tap, vpf_job_bounds.h).
#pragma once
#include <stdint.h>

#include "vpf_classes.h"
#include "vpf_hip.h"
#include "vpf_job_bounds.h"

namespace vpf {

struct RemapPlan {
  bool ok;          // false: refused (hipErrorInvalidValue), nothing is launched
  uint32_t gx, gy;  // the grid, of 256-lane workgroups over 32 x 32 destination tiles (kWarpTileW x kWarpTileH); z = the table's jobs
  uint32_t per;     // jobs per table: kRemapBatch
  uint32_t lds;     // the strip: the kernel's `lds_bytes` argument and the launch's dynamic LDS
  uint32_t dmask;   // destination alignment the vector stores need (vpf_tensor_dmask, vpf_plan_bounds.h)
};

// `max_step`: the caller's bound on the source pixels per destination pixel step of its maps (0: none) — the device-table warp's hint and its
// bound (warp_dev_lds_bytes: kWarpStripMax without a hint).  `variant` = 9 (VPF_TUNE_NV12_RGB_VARIANT, the any-input generic forms): no LDS, so no
// tile's strip fits and every tile samples per tap.
inline RemapPlan remap_plan(int src_fc, bool nhwc, uint32_t dtype, uint32_t W, uint32_t H, uint32_t dw, uint32_t dh, float max_step, int variant) {
  RemapPlan p{};
  if (src_fc != FC_NV12 && src_fc != FC_YUV420 && src_fc != FC_P16) return p;
  if (!W || !H || !dw || !dh || W > 65536u || H > 65536u || dw > 65536u || dh > 65536u) return p;
  p.ok = true;
  p.gx = (dw + kWarpTileW - 1) / kWarpTileW;
  p.gy = (dh + kWarpTileH - 1) / kWarpTileH;
  p.per = (uint32_t)kRemapBatch;
  p.lds = variant == 9 ? 0u : warp_dev_lds_bytes(max_step, W, H, dw, dh);
  p.dmask = vpf_tensor_dmask(nhwc, dtype == VPF_TENSOR_F32);
  return p;
}

}  // namespace vpf
