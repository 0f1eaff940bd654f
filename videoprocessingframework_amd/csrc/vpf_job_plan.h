// vpf_job_plan.h — the policy of the eight per-job tensor launches (vpf_convert_resize_tensor_rois, vpf_convert_letterbox_tensor,
// vpf_convert_warp_tensor, vpf_convert_persp_tensor and their _dev forms: launch_convert_resize_rois of k_convert_roi.hip, launch_convert_letterbox of
// k_convert_letterbox.hip, launch_convert_warp of k_convert_warp.hip, launch_convert_persp of k_convert_persp.hip, and the launch_*_dev of the four
// k_convert_*_dev.hip) as ONE pure function: the refusal, or up to two dispatches in launch order — each a row of kJobForms, its grid, its job count,
// the strip bytes its kernel is told and the pixels per lane of its channels-last staging — the destination alignment mask, and for a host table
// which dispatch every job belongs to.  No HIP in here, no global, no allocation, no pointer: the launchers include it and only dispatch on the
// result (k_job_launch.h fills the tables from it), and tests/test_job_plan_cpu.py compiles the same header with g++ (tests/c/job_plan_capi.cpp).
// The strip sizing itself — what a job or a tile needs — stays in vpf_job_bounds.h; this header says how the launches combine it.  The measured
// reasons stand next to the rule they justify.
#pragma once
#include <stdint.h>

#include "vpf_classes.h"
#include "vpf_hip.h"
#include "vpf_job_bounds.h"

namespace vpf {

enum JobFamily : int { JOB_ROI = 0, JOB_LETTERBOX, JOB_WARP, JOB_PERSP, JOB_FAMILIES };

// Kernel families, one row of kJobForms each: per entry the staged form (a workgroup converts its tile's source window once into an LDS strip and
// blends from bytes), the per-tap form (four texel_rgb per pixel) and the device-table form (ONE dispatch, staged or per tap decided per tile).
enum JobForm : int {
  JF_ROI_STRIP = 0, JF_ROI_GATHER, JF_ROI_DEV,
  JF_LB_STRIP, JF_LB_GATHER, JF_LB_DEV,
  JF_WARP_STRIP, JF_WARP_GATHER, JF_WARP_DEV,
  JF_PERSP_STRIP, JF_PERSP_GATHER, JF_PERSP_DEV,
  JOB_FORMS
};
// name: what the selection log prints in front of the template arguments <source class, FC_TENSOR / FC_TENSOR_NHWC>; args: the scalar kernel
// arguments behind the table and the coefficients, in the kernel's order (lds: JobDispatch::lds, the bytes of the strip — NOT what the launch asks for)
struct JobFormInfo { const char* name; const char* args; };
constexpr JobFormInfo kJobForms[JOB_FORMS] = {
    {"k_roi_strip", "W dw dh dmask lds"},     {"k_roi_gather", "dw dh dmask"},        {"k_roi_dev", "W H dw dh dmask lds"},
    {"k_lb_strip", "W dw dh dmask lds"},      {"k_lb_gather", "dw dh dmask"},         {"k_lb_dev", "W H dw dh dmask lds"},
    {"k_warp_strip", "W H dw dh dmask lds"},  {"k_warp_gather", "W H dw dh dmask"},   {"k_warp_dev", "W H dw dh dmask lds"},
    {"k_persp_strip", "W H dw dh dmask lds"}, {"k_persp_gather", "W H dw dh dmask"},  {"k_persp_dev", "W H dw dh dmask lds"},
};

// Jobs per host table: what fits the 9 248 B of the largest argument block measured (the tables and their descriptors: vpf_internal.h) — 96 jobs of
// 96 B (ROI, warp), 82 of 112 B (letterbox, perspective).  vpf_abi.hip cuts a call into tables of these sizes.  A device table has no job table in
// the arguments: blockIdx.z is the job, up to 65535 of them, over the source planes of up to kRoiDevFrames frames.
constexpr uint32_t kJobTableCap[JOB_FAMILIES] = {(uint32_t)kRoiBatch, (uint32_t)kLetterboxBatch, (uint32_t)kWarpBatch, (uint32_t)kPerspBatch};
constexpr uint32_t kJobTableMax = 96;  // the largest of them: the size of the fixed per-job arrays below
constexpr uint32_t kJobDevMax = 65535u;
static_assert(kRoiBatch <= (int)kJobTableMax && kLetterboxBatch <= (int)kJobTableMax && kWarpBatch <= (int)kJobTableMax && kPerspBatch <= (int)kJobTableMax,
              "JobShape::g and JobPlan::which hold a whole table of every family");

// The geometry of one job the policy looks at: the rectangle (its row offset does not matter: roi_strip_need) and the scale factors as the entry
// passes them (JOB_ROI), the placement of the picture as well (JOB_LETTERBOX), or the six / nine coefficients (JOB_WARP / JOB_PERSP)
struct JobGeom {
  uint32_t x, w, h;
  float scx, scy;
  uint32_t ix, iy, iw, ih;
  float m[9];
};
struct JobShape {
  int family;  // JobFamily
  bool dev;    // the job table lives in device memory (the _dev entries)
  int src_fc;  // FmtClass of the frames
  bool nhwc;   // FC_TENSOR_NHWC: one interleaved plane per job; else FC_TENSOR: three planes
  uint32_t dtype;  // TensorEpi::dtype as the caller passes it (compared whole: kEpiSwapRB is only ever set for a channels-last destination, where
                   // the mask is 15 whatever the dtype)
  uint32_t W, H, dw, dh;
  int variant;  // tuning(VPF_TUNE_NV12_RGB_VARIANT), read once by the caller
  // host table
  uint32_t n;
  JobGeom g[kJobTableMax];  // the first min(n, kJobTableMax) are looked at, and only the members of the family
  // device table
  uint32_t max_n, n_frames;
  float max_step;  // JOB_WARP / JOB_PERSP: the caller's hint, 0 = none
};
struct JobDispatch {
  int form;         // JobForm
  uint32_t gx, gy;  // the grid, of 256-lane workgroups; z = n
  uint32_t n;       // jobs: the table's job count (host) or max_n (device)
  uint32_t lds;     // the strip: the kernel's `lds_bytes` argument, and its own share of the launch's dynamic LDS (0: the per-tap forms)
  uint32_t stage_npx;  // != 0: a channels-last launch of a family that stages its interleaved rows — the pixels per lane for nhwc_stage_plan
                       // (vpf_internal.h), which adds the waves' staging area behind `lds` where both fit 64 KiB; 0: the launch asks for `lds`
};
struct JobPlan {
  bool ok;  // false: refused (hipErrorInvalidValue), nothing is launched
  int nd;   // dispatches, in launch order: the staged one first — its error returns before the per-tap launch
  JobDispatch d[2];
  uint32_t dmask;  // destination alignment the vector stores need (vpf_tensor_dmask, vpf_plan_bounds.h)
  uint8_t which[kJobTableMax];  // host table: the dispatch (index into d) of job i; the jobs of a dispatch keep their call order in its table
};

namespace job_detail {
// The strip a host-table job would stage, or kJobPerTap for a job that samples per tap.
//   ROI, letterbox: staged where the window — WALKED with the kernel's own fp32 tap arithmetic, chunk by chunk and band by band — fits a strip that
//     leaves three workgroups per CU (kRoiStripMax) and converts at most three source pixels per destination pixel (kRoiConvMax, the measured
//     break-even of the strip against the per-tap kernels: the whole-frame fused launch's rule, vpf_fused_plan.h); large down-scales gather.  The
//     letterbox walks the tiles of the PLANE that meet the picture.
//   warp, perspective: staged wherever the O(1) bound of a tile's strip fits kWarpStripMax (64 KiB, two workgroups per CU: no break-even in
//     converted pixels is reached before the strip outgrows the LDS, vpf_job_bounds.h).  Two dispatches per table rather than one with a per-tile
//     decision: the host has the matrices, so a large down-scale is known before the launch and its tiles run the small per-tap kernel at full
//     occupancy instead of the staged kernel holding LDS it cannot use.  What the host cannot know — the horizon inside a tile, a strip past the
//     bound — the staged kernels decide per tile.
constexpr uint32_t kJobPerTap = ~0u;
inline uint32_t staged_bytes(const JobShape& q, const JobGeom& j) {
  switch (q.family) {
    case JOB_ROI: {
      const RoiStripNeed need = roi_strip_need(j.x, j.w, j.h, j.scx, j.scy, q.dw, q.dh);
      return roi_job_staged(need) ? need.bytes : kJobPerTap;
    }
    case JOB_LETTERBOX: {
      const RoiStripNeed need = letterbox_strip_need(j.x, j.w, j.h, j.scx, j.scy, j.ix, j.iy, j.iw, j.ih, q.dw, q.dh);
      return roi_job_staged(need) ? need.bytes : kJobPerTap;
    }
    case JOB_WARP: {
      const WarpNeed need = warp_need(j.m, q.W, q.H, q.dw, q.dh);
      return need.bytes <= kWarpStripMax ? need.bytes : kJobPerTap;
    }
    default: {
      const WarpNeed need = persp_need(j.m, q.W, q.H, q.dw, q.dh);
      return need.bytes <= kWarpStripMax ? need.bytes : kJobPerTap;
    }
  }
}
// The dynamic LDS of a device-table dispatch, whose jobs nobody has seen: the most a staged tile of this destination size can need (ROI, letterbox:
// the conversion limit bounds the strip, roi_dev_lds_bytes), the bound of the caller's hint (the warps; no hint: kWarpStripMax)
inline uint32_t dev_bytes(const JobShape& q) {
  switch (q.family) {
    case JOB_ROI: case JOB_LETTERBOX: return roi_dev_lds_bytes(q.dw, q.dh);
    case JOB_WARP: return warp_dev_lds_bytes(q.max_step, q.W, q.H, q.dw, q.dh);
    default: return persp_dev_lds_bytes(q.max_step, q.W, q.H, q.dw, q.dh);
  }
}
}  // namespace job_detail

inline JobPlan job_plan(const JobShape& q) {
  JobPlan p{};
  if (q.family < 0 || q.family >= JOB_FAMILIES) return p;
  if (q.src_fc != FC_NV12 && q.src_fc != FC_YUV420 && q.src_fc != FC_P16) return p;  // the source classes the job kernels are instantiated for
  if (q.dev ? !q.max_n || q.max_n > kJobDevMax || !q.n_frames || q.n_frames > (uint32_t)kRoiDevFrames : !q.n || q.n > kJobTableCap[q.family]) return p;
  p.ok = true;
  p.dmask = vpf_tensor_dmask(q.nhwc, q.dtype == VPF_TENSOR_F32);
  const bool warp = q.family == JOB_WARP || q.family == JOB_PERSP;
  // VPF_TUNE_NV12_RGB_VARIANT = 9, the any-input generic forms: no strip anywhere — every host job goes to the per-tap dispatch, a device dispatch
  // gets no LDS, so no tile's strip fits and every tile samples per tap
  const bool all_per_tap = q.variant == 9;
  // Grids.  ROI and letterbox, staged and device forms: a workgroup owns 16 destination rows (four waves x kRoiBandRows) x 256 columns; their
  // per-tap form is the whole-frame gather kernel's: four rows x 64 lanes x 4 pixels.  Every form of the two warps: 32 x 32 tiles (close to
  // square keeps a rotated footprint's bounding box small, vpf_job_bounds.h).
  const uint32_t tile_gx = warp ? (q.dw + kWarpTileW - 1) / kWarpTileW : (q.dw + 255) / 256;
  const uint32_t tile_gy = warp ? (q.dh + kWarpTileH - 1) / kWarpTileH : (q.dh + 4 * kRoiBandRows - 1) / (4 * kRoiBandRows);
  const uint32_t tap_gx = warp ? tile_gx : ((q.dw + 3) / 4 + 63) / 64, tap_gy = warp ? tile_gy : (q.dh + 3) / 4;
  // Channels-last staging: ROI and letterbox hand a lane four consecutive pixels of a row through tensor_store4_nhwc*, whose f32 rows leave through
  // the waves' staging area as dense stores (k_fused_common.h) — in the staged, the per-tap and the device form.  The warps' epilogue (warp_store4)
  // stores per lane and never stages.
  const uint32_t npx = q.nhwc && !warp ? 4u : 0u;
  const int f0 = 3 * q.family;  // the family's rows of kJobForms: strip, gather, dev
  if (q.dev) {
    p.nd = 1;
    p.d[0] = JobDispatch{f0 + 2, tile_gx, tile_gy, q.max_n, all_per_tap ? 0u : job_detail::dev_bytes(q), npx};
    return p;
  }
  uint32_t ns = 0, lds = 0;
  for (uint32_t i = 0; i < q.n; i++) {  // ONE pass over the jobs
    const uint32_t bytes = all_per_tap ? job_detail::kJobPerTap : job_detail::staged_bytes(q, q.g[i]);
    p.which[i] = bytes == job_detail::kJobPerTap;  // (0 = staged for now)
    if (bytes != job_detail::kJobPerTap) {
      ns++;
      lds = bytes > lds ? bytes : lds;  // the staged dispatch's strip: the largest staged job's
    }
  }
  if (ns) p.d[p.nd++] = JobDispatch{f0, tile_gx, tile_gy, ns, lds, npx};
  if (ns != q.n) p.d[p.nd++] = JobDispatch{f0 + 1, tap_gx, tap_gy, q.n - ns, 0u, npx};
  if (!ns)  // the per-tap dispatch is the only one: d[0]
    for (uint32_t i = 0; i < q.n; i++) p.which[i] = 0;
  return p;
}

}  // namespace vpf
