// k_convert_warp_common.h — the device helpers the warp translation units share (k_convert_warp.hip, k_convert_persp.hip: the host-table kernels;
// k_convert_warp_dev.hip, k_convert_persp_dev.hip: the device-table kernels): border mode and bytes out of TensorEpi::pad, the four-pixel store
// through the tensor epilogue, the per-tap form of a lane's four pixels and the staged form of a workgroup's tile — warp_gather4 / warp_strip_tile (the
// whole of k_warp_strip, the tail of k_warp_dev) and, for the perspective warp, persp_tap / persp_gather4 / persp_strip_tile (the whole of
// k_persp_strip, the tail of k_persp_dev).  Forced inline everywhere.
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
  const bool vec = tensor_vec_ok<DST>(f, nv, dmask);
  warp_store4<DST>(f, x0, y, u, te, vec, nv);
}

// ------------------------------------------------------------------------------------------
// The staged form of a workgroup's tile (k_warp_strip on the job of its table, k_warp_dev on the job it assembled from the device tables).  The
// window is wave-uniform (block indices and kernel arguments only).  A tile whose window is empty writes the border; a tile whose strip would not
// fit the LDS it was given — never in k_warp_strip: the launcher's bound covers every tile (warp_need) — takes the per-tap form instead of
// writing from a short strip.  Every lane of the workgroup calls this (one barrier inside).
// ------------------------------------------------------------------------------------------
template <int SRC, int DST>
VPF_DEV void warp_strip_tile(const WarpDesc& J, const TensorEpi& te, const Yuv2RgbCoef& c, uint32_t W, uint32_t H, uint32_t dw, uint32_t dh, uint32_t dmask,
                             uint32_t lds_bytes) {
  const FrameDesc& f = J.f;
  const bool rep = warp_rep(te);
  const uint32_t tid = threadIdx.x;
  const uint32_t xs = blockIdx.x * kWarpTileW, ys = blockIdx.y * kWarpTileH;  // the grid covers the destination exactly: xs < dw, ys < dh
  const uint32_t xe = (xs + kWarpTileW - 1 < dw - 1) ? xs + kWarpTileW - 1 : dw - 1, ye = (ys + kWarpTileH - 1 < dh - 1) ? ys + kWarpTileH - 1 : dh - 1;
  const uint32_t x0 = xs + (tid % kWarpLanesX) * 4, y = ys + tid / kWarpLanesX;
  const bool mine = x0 < dw && y < dh;
  WarpWin w = warp_window(J.m, xs, xe, ys, ye, rep, W, H);
  w.x_lo = __builtin_amdgcn_readfirstlane(w.x_lo); w.x_hi = __builtin_amdgcn_readfirstlane(w.x_hi);
  w.y_lo = __builtin_amdgcn_readfirstlane(w.y_lo); w.y_hi = __builtin_amdgcn_readfirstlane(w.y_hi);
  const uint32_t nv = dw - x0 < 4 ? dw - x0 : 4;
  const bool vec = tensor_vec_ok<DST>(f, nv, dmask);
  if (w.empty) {  // (CONSTANT only: a clamped coordinate is always in range)
    if (!mine) return;
    if constexpr (DST == FC_TENSOR_NHWC) {
      float u[3][4];
#pragma unroll
      for (int ch = 0; ch < 3; ch++)
#pragma unroll
        for (int k = 0; k < 4; k++) u[ch][k] = warp_border(te, ch);
      warp_store4<DST>(f, x0, y, u, te, vec, nv);
    } else {
#pragma unroll
      for (int ch = 0; ch < 3; ch++) {
        const float b = warp_border(te, ch), u[4] = {b, b, b, b};
        tensor_store4<false>(f.d[ch] + (size_t)y * f.dp[ch], x0, u, te, ch, vec, nv);
      }
    }
    return;
  }
  const WarpStrip S = warp_strip(w);
  if (S.bytes > lds_bytes) {
    if (mine) warp_gather4<SRC, DST>(J, c, te, W, H, dw, dmask, x0, y);
    return;
  }
  uint8_t* const strip = reinterpret_cast<uint8_t*>(dyn_strip);
  strip_fill_window<SRC>(f, c, W, strip, S.base_px, w.y_lo, w.y_hi, S.ng, S.rowbytes, tid);
  __syncthreads();
  if (!mine) return;
  const float wmax = (float)(W - 1), hmax = (float)(H - 1);
  const float xlf = (float)w.x_lo, xhf = (float)w.x_hi, ylf = (float)w.y_lo, yhf = (float)w.y_hi;
  float u[3][4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const WarpXY s = warp_xy(J.m, (x0 + k < dw) ? x0 + k : dw - 1, y, rep, wmax, hmax);
    const bool in = s.sx >= 0.f && s.sx <= wmax && s.sy >= 0.f && s.sy <= hmax;
    // an in-range coordinate lies inside the window, so pulling it to the window leaves it unchanged; every other one reads some pixel of
    // the strip and is replaced by the border.  x1 = min(x0 + 1, x_hi) is min(x0 + 1, W - 1) for an in-range pixel (x_hi = min(floor + 1, W - 1)).
    const float cx = __builtin_amdgcn_fmed3f(s.sx, xlf, xhf), cy = __builtin_amdgcn_fmed3f(s.sy, ylf, yhf);
    const uint32_t xa = (uint32_t)(int)cx, ya = (uint32_t)(int)cy;
    const uint32_t xb = xa + 1 < w.x_hi ? xa + 1 : w.x_hi, yb = ya + 1 < w.y_hi ? ya + 1 : w.y_hi;
    const float fx = cx - (float)xa, fy = cy - (float)ya;
    const uint8_t* const ra = strip + (ya - w.y_lo) * S.rowbytes, * const rb = strip + (yb - w.y_lo) * S.rowbytes;
    const uint32_t oa = 4 * (xa - S.base_px), ob = 4 * (xb - S.base_px);
    const uint32_t q00 = *reinterpret_cast<const uint32_t*>(ra + oa), q01 = *reinterpret_cast<const uint32_t*>(ra + ob);
    const uint32_t q10 = *reinterpret_cast<const uint32_t*>(rb + oa), q11 = *reinterpret_cast<const uint32_t*>(rb + ob);
    const float v[3] = {__builtin_truncf(bilerp(ubyte<0>(q00), ubyte<0>(q01), ubyte<0>(q10), ubyte<0>(q11), fx, fy)),
                        __builtin_truncf(bilerp(ubyte<1>(q00), ubyte<1>(q01), ubyte<1>(q10), ubyte<1>(q11), fx, fy)),
                        __builtin_truncf(bilerp(ubyte<2>(q00), ubyte<2>(q01), ubyte<2>(q10), ubyte<2>(q11), fx, fy))};
#pragma unroll
    for (int ch = 0; ch < 3; ch++) u[ch][k] = in ? v[ch] : warp_border(te, ch);
  }
  if constexpr (DST == FC_TENSOR_NHWC) warp_store4<DST>(f, x0, y, u, te, vec, nv);
  else for (int ch = 0; ch < 3; ch++) tensor_store4<false>(f.d[ch] + (size_t)y * f.dp[ch], x0, u[ch], te, ch, vec, nv);
}

// one pixel at the in-range coordinate (cx, cy) through the per-tap form: warp_gather4's sampling
template <int SRC>
VPF_DEV void persp_tap(const FrameDesc& f, const Yuv2RgbCoef& c, float cx, float cy, uint32_t W, uint32_t H, float (&v)[3]) {
  const uint32_t xa = (uint32_t)(int)cx, ya = (uint32_t)(int)cy;
  const uint32_t xb = xa + 1 < W ? xa + 1 : W - 1, yb = ya + 1 < H ? ya + 1 : H - 1;
  const float fx = cx - (float)xa, fy = cy - (float)ya;
  float p00[3], p01[3], p10[3], p11[3];
  texel_rgb<SRC>(f, c, xa, ya, p00);
  texel_rgb<SRC>(f, c, xb, ya, p01);
  texel_rgb<SRC>(f, c, xa, yb, p10);
  texel_rgb<SRC>(f, c, xb, yb, p11);
#pragma unroll
  for (int ch = 0; ch < 3; ch++) v[ch] = __builtin_truncf(bilerp(p00[ch], p01[ch], p10[ch], p11[ch], fx, fy));
}
// four pixels of a lane through the per-tap form, stored through the tensor epilogue (warp_gather4 with the perspective coordinates: the taps of a
// pixel that takes the border are clamped into the frame and loaded all the same, so the four pixels' loads overlap)
template <int SRC, int DST>
VPF_DEV void persp_gather4(const PerspDesc& J, const Yuv2RgbCoef& c, const TensorEpi& te, uint32_t W, uint32_t H, uint32_t dw, uint32_t dmask, uint32_t x0,
                           uint32_t y) {
  const FrameDesc& f = J.f;
  const bool rep = warp_rep(te);
  const float wmax = (float)(W - 1), hmax = (float)(H - 1);
  float u[3][4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const PerspXY s = persp_xy(J.m, (x0 + k < dw) ? x0 + k : dw - 1, y, rep, wmax, hmax);
    const bool in = s.front && s.sx >= 0.f && s.sx <= wmax && s.sy >= 0.f && s.sy <= hmax;
    float v[3];
    persp_tap<SRC>(f, c, __builtin_amdgcn_fmed3f(s.sx, 0.f, wmax), __builtin_amdgcn_fmed3f(s.sy, 0.f, hmax), W, H, v);  // == sx, sy when in range
#pragma unroll
    for (int ch = 0; ch < 3; ch++) u[ch][k] = in ? v[ch] : warp_border(te, ch);
  }
  const uint32_t nv = dw - x0 < 4 ? dw - x0 : 4;
  const bool vec = tensor_vec_ok<DST>(f, nv, dmask);
  warp_store4<DST>(f, x0, y, u, te, vec, nv);
}

// ------------------------------------------------------------------------------------------
// The perspective warp's tile (k_persp_strip on the job of its table, k_persp_dev on the job it assembled from the device tables): the tile's class
// from its four corners (persp_window: border, per tap, nothing staged, staged), the strip staged where it fits the LDS the dispatch was given, the
// per-tap form where it does not, and the per-pixel test of an in-range pixel's taps against the staged window (persp_px_in_window).  All branches
// workgroup-uniform.  Every lane of the workgroup calls this (one barrier inside).
// ------------------------------------------------------------------------------------------
template <int SRC, int DST>
VPF_DEV void persp_strip_tile(const PerspDesc& J, const TensorEpi& te, const Yuv2RgbCoef& c, uint32_t W, uint32_t H, uint32_t dw, uint32_t dh, uint32_t dmask,
                              uint32_t lds_bytes) {
  const FrameDesc& f = J.f;
  const bool rep = warp_rep(te);
  const uint32_t tid = threadIdx.x;
  const uint32_t xs = blockIdx.x * kWarpTileW, ys = blockIdx.y * kWarpTileH;  // the grid covers the destination exactly: xs < dw, ys < dh
  const uint32_t xe = (xs + kWarpTileW - 1 < dw - 1) ? xs + kWarpTileW - 1 : dw - 1, ye = (ys + kWarpTileH - 1 < dh - 1) ? ys + kWarpTileH - 1 : dh - 1;
  const uint32_t x0 = xs + (tid % kWarpLanesX) * 4, y = ys + tid / kWarpLanesX;
  const bool mine = x0 < dw && y < dh;
  PerspWin pw = persp_window(J.m, xs, xe, ys, ye, rep, W, H);
  pw.cls = __builtin_amdgcn_readfirstlane(pw.cls);
  WarpWin& w = pw.w;
  w.x_lo = __builtin_amdgcn_readfirstlane(w.x_lo); w.x_hi = __builtin_amdgcn_readfirstlane(w.x_hi);
  w.y_lo = __builtin_amdgcn_readfirstlane(w.y_lo); w.y_hi = __builtin_amdgcn_readfirstlane(w.y_hi);
  const uint32_t nv = dw - x0 < 4 ? dw - x0 : 4;
  const bool vec = tensor_vec_ok<DST>(f, nv, dmask);
  if (pw.cls == kPerspTileBorder) {  // behind the plane: both modes
    if (!mine) return;
    float u[3][4];
#pragma unroll
    for (int ch = 0; ch < 3; ch++)
#pragma unroll
      for (int k = 0; k < 4; k++) u[ch][k] = warp_border(te, ch);
    warp_store4<DST>(f, x0, y, u, te, vec, nv);
    return;
  }
  const bool staged = pw.cls == kPerspTileStage;
  const WarpStrip S = warp_strip(w);  // (not staged: the window is 0 .. 0, never read)
  if (pw.cls == kPerspTileTap || (staged && S.bytes > lds_bytes)) {  // the horizon in the tile, or a strip the dispatch has no room for
    if (mine) persp_gather4<SRC, DST>(J, c, te, W, H, dw, dmask, x0, y);
    return;
  }
  uint8_t* const strip = reinterpret_cast<uint8_t*>(dyn_strip);
  if (staged) {
    strip_fill_window<SRC>(f, c, W, strip, S.base_px, w.y_lo, w.y_hi, S.ng, S.rowbytes, tid);
    __syncthreads();
  }
  if (!mine) return;
  const float wmax = (float)(W - 1), hmax = (float)(H - 1);
  float u[3][4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const PerspXY s = persp_xy(J.m, (x0 + k < dw) ? x0 + k : dw - 1, y, rep, wmax, hmax);  // (front: w > 0 on every pixel of this tile)
    const bool in = s.front && s.sx >= 0.f && s.sx <= wmax && s.sy >= 0.f && s.sy <= hmax;
    const float cx = __builtin_amdgcn_fmed3f(s.sx, 0.f, wmax), cy = __builtin_amdgcn_fmed3f(s.sy, 0.f, hmax);  // == sx, sy when in range
    const uint32_t xa0 = (uint32_t)(int)cx, ya0 = (uint32_t)(int)cy;
    const bool inwin = staged && persp_px_in_window(w, xa0, ya0, W, H);
    float v[3] = {0.f, 0.f, 0.f};
    if (staged) {
      // a pixel inside the window keeps its taps (xb = min(xa + 1, W - 1) <= x_hi was tested); every other one reads some pixel of the strip and is
      // replaced below
      const uint32_t xa = xa0 < w.x_lo ? w.x_lo : (xa0 < w.x_hi ? xa0 : w.x_hi), ya = ya0 < w.y_lo ? w.y_lo : (ya0 < w.y_hi ? ya0 : w.y_hi);
      const uint32_t xb = xa + 1 < w.x_hi ? xa + 1 : w.x_hi, yb = ya + 1 < w.y_hi ? ya + 1 : w.y_hi;
      const float fx = cx - (float)xa0, fy = cy - (float)ya0;
      const uint8_t* const ra = strip + (ya - w.y_lo) * S.rowbytes, * const rb = strip + (yb - w.y_lo) * S.rowbytes;
      const uint32_t oa = 4 * (xa - S.base_px), ob = 4 * (xb - S.base_px);
      const uint32_t q00 = *reinterpret_cast<const uint32_t*>(ra + oa), q01 = *reinterpret_cast<const uint32_t*>(ra + ob);
      const uint32_t q10 = *reinterpret_cast<const uint32_t*>(rb + oa), q11 = *reinterpret_cast<const uint32_t*>(rb + ob);
      v[0] = __builtin_truncf(bilerp(ubyte<0>(q00), ubyte<0>(q01), ubyte<0>(q10), ubyte<0>(q11), fx, fy));
      v[1] = __builtin_truncf(bilerp(ubyte<1>(q00), ubyte<1>(q01), ubyte<1>(q10), ubyte<1>(q11), fx, fy));
      v[2] = __builtin_truncf(bilerp(ubyte<2>(q00), ubyte<2>(q01), ubyte<2>(q10), ubyte<2>(q11), fx, fy));
    }
    if (in && !inwin) persp_tap<SRC>(f, c, cx, cy, W, H, v);  // cold: the corner box missed this pixel (or nothing was staged)
#pragma unroll
    for (int ch = 0; ch < 3; ch++) u[ch][k] = in ? v[ch] : warp_border(te, ch);
  }
  warp_store4<DST>(f, x0, y, u, te, vec, nv);
}

}  // namespace vpf
#endif  // VPF_K_CONVERT_WARP_COMMON_H_
