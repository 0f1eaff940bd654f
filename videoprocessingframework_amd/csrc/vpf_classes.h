// vpf_classes.h — the format classes and frame-table sizes both the launchers (vpf_internal.h) and the HIP-free planning headers
// (vpf_fused_plan.h, compiled with plain g++ by the CPU tests) name.  No HIP in here.
#pragma once

namespace vpf {

// frames per frame table: the small and the large one (the tables themselves, and why there are two: vpf_internal.h)
constexpr int kSmallBatch = 32;
constexpr int kMaxBatch = 128;

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

}  // namespace vpf
