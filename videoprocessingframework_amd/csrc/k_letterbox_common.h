// k_letterbox_common.h — what the two letterbox translation units share on the device (k_convert_letterbox.hip: the host-table kernels;
// k_convert_letterbox_dev.hip: the device-table kernel): the pad bytes out of TensorEpi::pad, the four-pixel store through the tensor epilogue and
// the pad rows of a lane.
#ifndef VPF_K_LETTERBOX_COMMON_H_
#define VPF_K_LETTERBOX_COMMON_H_
#include "k_bilinear_blend.h"
#include "k_fused_common.h"

namespace vpf {

VPF_DEV float lb_pad(const TensorEpi& e, int ch) { return (float)((e.pad >> (8 * ch)) & 0xffu); }

// the lane's four pixels u[ch][k] (8-bit values) of plane row y through the tensor epilogue; wv, lane: tensor_store_nhwc's (a wave's lanes are one
// run of a row in both kernels)
template <int DST>
VPF_DEV void lb_store4(const FrameDesc& f, uint32_t x0, uint32_t y, const float (&u)[3][4], const TensorEpi& te, bool vec, uint32_t nv, uint32_t wv,
                       uint32_t lane) {
  if constexpr (DST == FC_TENSOR_NHWC) {
    tensor_store_nhwc<false, 4>(f.d[0] + (size_t)y * f.dp[0], x0, u, te, vec, nv, wv, lane);
  } else {
#pragma unroll
    for (int ch = 0; ch < 3; ch++) tensor_store4<false>(f.d[ch] + (size_t)y * f.dp[ch], x0, u[ch], te, ch, vec, nv);
  }
}
// rows ya .. yb of the lane's four columns, except rows ra .. rb (ra > rb: none excepted), take the pad.  The values do not depend on the row: their
// epilogue (one fma and one conversion per channel) is computed once per lane, the loop stores.
template <int DST>
VPF_DEV void lb_pad_rows(const FrameDesc& f, uint32_t x0, uint32_t ya, uint32_t yb, uint32_t ra, uint32_t rb, const TensorEpi& te, bool vec,
                         uint32_t nv, uint32_t wv, uint32_t lane) {
  float u[3][4];
#pragma unroll
  for (int ch = 0; ch < 3; ch++)
#pragma unroll
    for (int k = 0; k < 4; k++) u[ch][k] = lb_pad(te, ch);
  for (uint32_t y = ya; y <= yb; y++) {
    if (y >= ra && y <= rb) continue;
    lb_store4<DST>(f, x0, y, u, te, vec, nv, wv, lane);
  }
}

}  // namespace vpf

#endif  // VPF_K_LETTERBOX_COMMON_H_
