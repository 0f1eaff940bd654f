// k_convert_persp.hip — fused multi-ROI perspective warp (3 x 3 homography) of NV12 / YUV420 / P10 / P12 into a normalised tensor (gfx950):
// vpf_convert_persp_tensor.  The affine entry's tile, lane assignment, strip, blend and epilogue (k_convert_warp.hip); the coordinates are new.
// Grid = (destination tiles of 32 x 32, job); a lane owns four consecutive pixels of one row, a workgroup 8 lanes x 32 rows.
//   k_persp_strip    the staged form.  A tile whose four corners have w > 0 (then every pixel has: w is rounded-affine, monotone along both axes)
//                    converts the corners' bounding box, one pixel wider per side, into an LDS strip of four-byte RGB pixels
//                    (strip_fill_window), one barrier, and blends from bytes.  Every in-range pixel tests its taps against that window
//                    (persp_px_in_window): fl(fl(nx) / fl(w)) is not monotone, so the corner box is a guess; a pixel outside it is sampled per tap.
//                    A tile the horizon crosses or touches samples per tap; one wholly behind the plane writes the border; one whose strip exceeds
//                    the LDS of the dispatch samples per tap.  All workgroup-uniform branches.
//   k_persp_gather   per-tap texel_rgb: jobs whose bound (persp_need) exceeds 64 KiB of LDS, VPF_TUNE_NV12_RGB_VARIANT = 9
// Definition (include/vpf_hip.h): nx, ny, w rounded-affine, sx = nx / w, sy = ny / w as IEEE divisions (the compiler's v_div_scale / v_div_fmas /
// v_div_fixup sequence: correctly rounded, denormals kept; never v_rcp_f32 and a multiply), !(w > 0) -> border; from the range test on the affine
// entry.  Both kernels run exactly those fp32 operations in that order (-ffp-contract=off): identical bits.
#include <cmath>

#include "k_convert_warp_common.h"
#include "k_job_launch.h"

namespace vpf {

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
  bool vec = nv == 4;
#pragma unroll
  for (int ch = 0; ch < (DST == FC_TENSOR_NHWC ? 1 : 3); ch++) vec = vec && ((((uintptr_t)f.d[ch] | f.dp[ch]) & dmask) == 0);
  warp_store4<DST>(f, x0, y, u, te, vec, nv);
}

// ------------------------------------------------------------------------------------------
// The staged form (DST = FC_TENSOR: three planes per job; FC_TENSOR_NHWC: one interleaved plane).  What differs from the affine kernel
// (k_warp_strip): the tile's class (persp_window: border, per tap, nothing staged, staged), and the per-pixel test of an in-range pixel's taps against
// the window the tile staged (persp_px_in_window) — the affine kernel's "an in-range coordinate lies inside the window" does not hold for a rounded
// quotient, so a pixel that fails the test is sampled per tap instead of being pulled into the window.
// ------------------------------------------------------------------------------------------
template <int SRC, int DST>
__global__ __launch_bounds__(256) void k_persp_strip(const PerspArgs args, const Yuv2RgbCoef c, uint32_t W, uint32_t H, uint32_t dw, uint32_t dh,
                                                     uint32_t dmask, uint32_t lds_bytes) {
  const PerspDesc& J = args.j[blockIdx.z];
  const FrameDesc& f = J.f;
  const TensorEpi te = args.e;
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
  bool vec = nv == 4;
#pragma unroll
  for (int ch = 0; ch < (DST == FC_TENSOR_NHWC ? 1 : 3); ch++) vec = vec && ((((uintptr_t)f.d[ch] | f.dp[ch]) & dmask) == 0);
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

// ------------------------------------------------------------------------------------------
// The gather form: the same tile and lane assignment, four texel_rgb per pixel.
// ------------------------------------------------------------------------------------------
template <int SRC, int DST>
__global__ __launch_bounds__(256) void k_persp_gather(const PerspArgs args, const Yuv2RgbCoef c, uint32_t W, uint32_t H, uint32_t dw, uint32_t dh,
                                                      uint32_t dmask) {
  const uint32_t x0 = blockIdx.x * kWarpTileW + (threadIdx.x % kWarpLanesX) * 4, y = blockIdx.y * kWarpTileH + threadIdx.x / kWarpLanesX;
  if (x0 >= dw || y >= dh) return;
  persp_gather4<SRC, DST>(args.j[blockIdx.z], c, args.e, W, H, dw, dmask, x0, y);
}

// ------------------------------------------------------------------------------------------
// Host side: launch_convert_warp's split.  A job whose bound (persp_need, vpf_job_bounds.h) fits kWarpStripMax goes to the staged dispatch, whose
// dynamic LDS is the largest such bound; every other job to the per-tap dispatch.  Two dispatches per table rather than one with a per-tile
// decision: the host has the matrices, so a large down-scale is known before the launch and its tiles run the small per-tap kernel at full
// occupancy instead of the staged kernel holding LDS it cannot use.  What the host cannot know — the horizon inside a tile, a strip past the
// bound — the staged kernel decides per tile.
// ------------------------------------------------------------------------------------------
hipError_t launch_convert_persp(hipStream_t st, int src_fc, const Yuv2RgbCoef& c, uint32_t W, uint32_t H, uint32_t n, const PerspDesc* jobs, uint32_t dw,
                                uint32_t dh, const TensorEpi& te, bool nhwc) {
  if (!n || n > (uint32_t)kPerspBatch || !job_src_ok(src_fc)) return hipErrorInvalidValue;
  const uint32_t dmask = job_dmask(te, nhwc);
  PerspArgs as, ag;
  const JobSplit sp = split_jobs(jobs, n, te, as, ag, [&](const PerspDesc& j) {
    const WarpNeed need = persp_need(j.m, W, H, dw, dh);
    return need.bytes <= kWarpStripMax ? need.bytes : kNotStaged;
  });
  const uint32_t ns = sp.ns, ngat = sp.ngat, lds = sp.lds;
  const uint32_t gx = (dw + kWarpTileW - 1) / kWarpTileW, gy = (dh + kWarpTileH - 1) / kWarpTileH;
  hipError_t e = hipSuccess;
  if (ns) {
    with_src_dst(src_fc, nhwc, [&](auto S, auto D) { VPF_LAUNCH_T(k_persp_strip, (S, D), dim3(gx, gy, ns), lds, st, as, c, W, H, dw, dh, dmask, lds); e = hipGetLastError(); });
    if (e != hipSuccess) return e;
  }
  if (ngat)
    with_src_dst(src_fc, nhwc, [&](auto S, auto D) { VPF_LAUNCH_T(k_persp_gather, (S, D), dim3(gx, gy, ngat), 0u, st, ag, c, W, H, dw, dh, dmask); e = hipGetLastError(); });
  return e;
}

}  // namespace vpf
