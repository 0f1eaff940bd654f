// vpf_classes.h — the format classes, frame-table sizes and resize-kernel constants both the launchers and kernels (vpf_internal.h) and the
// HIP-free planning headers (vpf_fused_plan.h, vpf_resize_plan.h, vpf_job_plan.h, compiled with plain g++ by the CPU tests) name.  No HIP in here.
#pragma once
#include <stdint.h>

namespace vpf {

// frames per frame table: the small and the large one (the tables themselves, and why there are two: vpf_internal.h)
constexpr int kSmallBatch = 32;
constexpr int kMaxBatch = 128;
// jobs per job table of the per-job tensor entries and frames per device-table call (the tables, and why these sizes: vpf_internal.h; the launch
// policy that refuses above them: vpf_job_plan.h)
constexpr int kRoiBatch = 96, kLetterboxBatch = 82, kWarpBatch = 96, kPerspBatch = 82;
constexpr int kRemapBatch = 96;  // jobs per table of the per-pixel remap entry (vpf_remap_plan.h: a launch of its own, no family of job_plan)
constexpr int kRoiDevFrames = 128;

enum FmtClass : int {
  FC_NV12 = 0,    // Y + interleaved UV, 4:2:0
  FC_YUV420 = 1,  // Y + U + V planes, 4:2:0
  FC_YUV444 = 2,  // three full planes
  FC_RGB = 3,     // packed R,G,B
  FC_BGR = 4,     // packed B,G,R
  FC_PLANAR = 5,  // three full planes R,G,B
  FC_TENSOR = 6,  // three full planes of f32 / f16 / bf16: the FC_PLANAR bytes through one fma each (vpf_convert_resize_tensor)
  FC_P16 = 7,     // P10 / P12: Y + interleaved UV of 16-bit MSB-aligned samples, 4:2:0 — a SOURCE class of the fused tensor entries only: every
                  // sample is narrowed to 8 bits at the load (p16_to_8, vpf_device.h), from there the code is FC_NV12's
  FC_TENSOR_NHWC = 8,  // FC_TENSOR's elements in ONE interleaved plane per frame (VPF_TENSOR_NHWC): element (y, x, c) at d[0] + y dp[0] + (3 x + c) elem
};

// one plane of a resize: `ch` interleaved channels (for float surfaces: floats per pixel), `k` = plane index in FrameDesc
struct ResizeJob {
  int ch, k;
  uint32_t sw, sh, dw, dh;
};

// What the plain resize kernels (k_bilinear_blend.h, k_resize.hip) and the policy that sizes their launches (vpf_resize_plan.h) both name:
constexpr uint32_t kResizeRowBytes = 4096;  // largest strip (IT = 4 dense 1-KiB loads per source row)
constexpr int kBandSlots = 8;  // source rows a wave's strips can hold (twice as many when a strip is a single 1-KiB staging pass: IT = 1)
constexpr int band_px(int ch, int p1) { return ch == 1 ? p1 : 4; }  // pixels per lane of a row-band launch: P1 on 1-channel planes, else 4
constexpr uint32_t kLzStripQ = 128;  // at most 2 KiB of source bytes per row of a tile
constexpr int kTileStagePasses = 6;  // staging loads a thread may have in flight (the policy sizes tiles accordingly)

}  // namespace vpf
