// k_convert_warp_common.h — the device helpers the affine-warp translation units share (k_convert_warp.hip: the host-table kernels;
// k_convert_warp_dev.hip: the device-table kernel): border mode and bytes out of TensorEpi::pad, the four-pixel store through the tensor epilogue,
// and the per-tap form of a lane's four pixels.  Forced inline everywhere: the text moved here from k_convert_warp.hip unchanged, and the four
// kernels of that file compile to the instructions they had before.
#ifndef VPF_K_CONVERT_WARP_COMMON_H_
#define VPF_K_CONVERT_WARP_COMMON_H_
#include "k_bilinear_blend.h"
#include "k_fused_common.h"
#include "vpf_job_bounds.h"

namespace vpf {

VPF_DEV bool warp_rep(const TensorEpi& e) { return (e.pad >> 24) == VPF_WARP_REPLICATE; }
VPF_DEV float warp_border(const TensorEpi& e, int ch) { return (float)((e.pad >> (8 * ch)) & 0xffu); }

// the lane's four pixels u[ch][k] through the tensor epilogue.  FC_TENSOR_NHWC: per-lane vector stores — a tile row is 8 lanes, 384 B of f32, so a
// store instruction of a wave covers eight rows' runs whatever the form; nothing to stage
template <int DST>
VPF_DEV void warp_store4(const FrameDesc& f, uint32_t x0, uint32_t y, const float (&u)[3][4], const TensorEpi& te, bool vec, uint32_t nv) {
  if constexpr (DST == FC_TENSOR_NHWC) {
    tensor_store_nhwc<false, 4>(f.d[0] + (size_t)y * f.dp[0], x0, u, te, vec, nv, kNoStage, 0u);
  } else {
    for (int ch = 0; ch < 3; ch++) tensor_store4<false>(f.d[ch] + (size_t)y * f.dp[ch], x0, u[ch], te, ch, vec, nv);
  }
}
// four pixels of a lane through the per-tap form, stored through the tensor epilogue
template <int SRC, int DST = FC_TENSOR>
VPF_DEV void warp_gather4(const WarpDesc& J, const Yuv2RgbCoef& c, const TensorEpi& te, uint32_t W, uint32_t H, uint32_t dw, uint32_t dmask, uint32_t x0,
                          uint32_t y) {
  const FrameDesc& f = J.f;
  const bool rep = warp_rep(te);
  const float wmax = (float)(W - 1), hmax = (float)(H - 1);
  float u[3][4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const WarpXY s = warp_xy(J.m, (x0 + k < dw) ? x0 + k : dw - 1, y, rep, wmax, hmax);
    const bool in = s.sx >= 0.f && s.sx <= wmax && s.sy >= 0.f && s.sy <= hmax;
    const float cx = __builtin_amdgcn_fmed3f(s.sx, 0.f, wmax), cy = __builtin_amdgcn_fmed3f(s.sy, 0.f, hmax);  // == sx, sy when in range
    const uint32_t xa = (uint32_t)(int)cx, ya = (uint32_t)(int)cy;
    const uint32_t xb = xa + 1 < W ? xa + 1 : W - 1, yb = ya + 1 < H ? ya + 1 : H - 1;
    const float fx = cx - (float)xa, fy = cy - (float)ya;
    float p00[3], p01[3], p10[3], p11[3];
    texel_rgb<SRC>(f, c, xa, ya, p00);
    texel_rgb<SRC>(f, c, xb, ya, p01);
    texel_rgb<SRC>(f, c, xa, yb, p10);
    texel_rgb<SRC>(f, c, xb, yb, p11);
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
      const float v = __builtin_truncf(bilerp(p00[ch], p01[ch], p10[ch], p11[ch], fx, fy));
      u[ch][k] = in ? v : warp_border(te, ch);
    }
  }
  const uint32_t nv = dw - x0 < 4 ? dw - x0 : 4;
  bool vec = nv == 4;
#pragma unroll
  for (int ch = 0; ch < (DST == FC_TENSOR_NHWC ? 1 : 3); ch++) vec = vec && ((((uintptr_t)f.d[ch] | f.dp[ch]) & dmask) == 0);
  warp_store4<DST>(f, x0, y, u, te, vec, nv);
}

}  // namespace vpf
#endif  // VPF_K_CONVERT_WARP_COMMON_H_
