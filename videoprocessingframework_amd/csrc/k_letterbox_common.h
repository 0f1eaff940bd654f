// k_letterbox_common.h — what the letterbox translation units share on the device (k_convert_letterbox.hip: the host-table kernels;
// k_convert_letterbox_dev.hip: the device-table kernel; k_convert_letterbox_aa.hip takes the pad and the store): the pad bytes out of TensorEpi::pad,
// the four-pixel store through the tensor epilogue, the pad rows of a lane, and lb_gather4, the per-tap form of a lane's four pixels of one row
// (k_lb_gather's wave, k_lb_dev's row loop): one text, so a per-tap tile of the device-table entry gives the bits of its host-table twin because
// both run this function.  Every value comes in as a parameter; forced inline everywhere.  The staged tile is typed in both units:
// shared, k_lb_strip ran up to 6 % slower.
#ifndef VPF_K_LETTERBOX_COMMON_H_
#define VPF_K_LETTERBOX_COMMON_H_
#include "k_bilinear_blend.h"
#include "k_fused_common.h"

namespace vpf {

VPF_DEV float lb_pad(const TensorEpi& e, int ch) { return (float)((e.pad >> (8 * ch)) & 0xffu); }
// a lane's four pixels, all pad
VPF_DEV void lb_fill_pad(float (&u)[3][4], const TensorEpi& te) {
#pragma unroll
  for (int ch = 0; ch < 3; ch++)
#pragma unroll
    for (int k = 0; k < 4; k++) u[ch][k] = lb_pad(te, ch);
}

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
  lb_fill_pad(u, te);
  for (uint32_t y = ya; y <= yb; y++) {
    if (y >= ra && y <= rb) continue;
    lb_store4<DST>(f, x0, y, u, te, vec, nv, wv, lane);
  }
}

// ------------------------------------------------------------------------------------------
// The per-tap form: plane row y's four pixels of a lane.  `live`: the row and some of the lane's columns lie in the picture — otherwise nothing is
// loaded and the lane stores the pad.  tx[k], in[k]: the column taps on the rectangle (a column outside the picture: the taps of the nearest picture
// column, texels of the rectangle) and whether column x0 + k is picture; ty: the row's tap.  k_roi_gather's pixel — texel_rgb at absolute frame
// coordinates, bilerp, truncation — on the picture, all four pixels' texels in flight together.
// ------------------------------------------------------------------------------------------
template <int SRC, int DST>
VPF_DEV void lb_gather4(const FrameDesc& f, const Yuv2RgbCoef& c, uint32_t rx, uint32_t ry, const Tap (&tx)[4], const bool (&in)[4], const Tap& ty, bool live,
                        uint32_t x0, uint32_t y, const TensorEpi& te, bool vec, uint32_t nv, uint32_t wv, uint32_t lane) {
  float u[3][4];
  lb_fill_pad(u, te);
  if (live) {
#pragma unroll
    for (int k = 0; k < 4; k++) {
      float p00[3], p01[3], p10[3], p11[3];
      texel_rgb<SRC>(f, c, rx + tx[k].i0, ry + ty.i0, p00);
      texel_rgb<SRC>(f, c, rx + tx[k].i1, ry + ty.i0, p01);
      texel_rgb<SRC>(f, c, rx + tx[k].i0, ry + ty.i1, p10);
      texel_rgb<SRC>(f, c, rx + tx[k].i1, ry + ty.i1, p11);
#pragma unroll
      for (int ch = 0; ch < 3; ch++) {
        const float v = __builtin_truncf(bilerp(p00[ch], p01[ch], p10[ch], p11[ch], tx[k].f, ty.f));
        u[ch][k] = in[k] ? v : u[ch][k];
      }
    }
  }
  lb_store4<DST>(f, x0, y, u, te, vec, nv, wv, lane);
}

}  // namespace vpf

#endif  // VPF_K_LETTERBOX_COMMON_H_
