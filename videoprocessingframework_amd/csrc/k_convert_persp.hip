// k_convert_persp.hip — fused multi-ROI perspective warp (3 x 3 homography) of NV12 / YUV420 / P10 / P12 into a normalised tensor (gfx950):
// vpf_convert_persp_tensor.  The affine entry's tile, lane assignment, strip, blend and epilogue (k_convert_warp.hip); the coordinates are new.
// Grid = (destination tiles of 32 x 32, job); a lane owns four consecutive pixels of one row, a workgroup 8 lanes x 32 rows.
//   k_persp_strip    the staged form.  A tile whose four corners have w > 0 (then every pixel has: w is rounded-affine, monotone along both axes)
//                    converts the corners' bounding box, one pixel wider per side, into an LDS strip of four-byte RGB pixels
//                    (VPF_STRIP_FILL_WINDOW), one barrier, and blends from bytes.  Every in-range pixel tests its taps against that window
//                    (persp_px_in_window): fl(fl(nx) / fl(w)) is not monotone, so the corner box is a guess; a pixel outside it is sampled per tap.
//                    A tile the horizon crosses or touches samples per tap; one wholly behind the plane writes the border; one whose strip exceeds
//                    the LDS of the dispatch samples per tap.  All workgroup-uniform branches.
//   k_persp_gather   per-tap texel_rgb: jobs whose bound (persp_need) exceeds 64 KiB of LDS, VPF_TUNE_NV12_RGB_VARIANT = 9
// Definition (include/vpf_hip.h): nx, ny, w rounded-affine, sx = nx / w, sy = ny / w as IEEE divisions (the compiler's v_div_scale / v_div_fmas /
// v_div_fixup sequence: correctly rounded, denormals kept; never v_rcp_f32 and a multiply), !(w > 0) -> border; from the range test on the affine
// entry.  Both kernels run exactly those fp32 operations in that order (-ffp-contract=off): identical bits.
#include <cmath>

#include "k_convert_warp_common.h"

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
// The staged form (DST = FC_TENSOR: three planes per job, k_persp_strip; FC_TENSOR_NHWC: one interleaved plane, k_persp_strip_nhwc)
// ------------------------------------------------------------------------------------------
template <int SRC>
__global__ __launch_bounds__(256) void k_persp_strip(const PerspArgs args, const Yuv2RgbCoef c, uint32_t W, uint32_t H, uint32_t dw, uint32_t dh,
                                                     uint32_t dmask, uint32_t lds_bytes) {
  constexpr int DST = FC_TENSOR;
  const PerspDesc& J = args.j[blockIdx.z];
#include "k_convert_persp_strip_body.h"
}
template <int SRC>
__global__ __launch_bounds__(256) void k_persp_strip_nhwc(const PerspArgs args, const Yuv2RgbCoef c, uint32_t W, uint32_t H, uint32_t dw, uint32_t dh,
                                                          uint32_t dmask, uint32_t lds_bytes) {
  constexpr int DST = FC_TENSOR_NHWC;  // one interleaved plane per job
  const PerspDesc& J = args.j[blockIdx.z];
#include "k_convert_persp_strip_body.h"
}

// ------------------------------------------------------------------------------------------
// The gather form: the same tile and lane assignment, four texel_rgb per pixel.
// ------------------------------------------------------------------------------------------
template <int SRC>
__global__ __launch_bounds__(256) void k_persp_gather(const PerspArgs args, const Yuv2RgbCoef c, uint32_t W, uint32_t H, uint32_t dw, uint32_t dh,
                                                      uint32_t dmask) {
  const uint32_t x0 = blockIdx.x * kWarpTileW + (threadIdx.x % kWarpLanesX) * 4, y = blockIdx.y * kWarpTileH + threadIdx.x / kWarpLanesX;
  if (x0 >= dw || y >= dh) return;
  persp_gather4<SRC, FC_TENSOR>(args.j[blockIdx.z], c, args.e, W, H, dw, dmask, x0, y);
}
template <int SRC>
__global__ __launch_bounds__(256) void k_persp_gather_nhwc(const PerspArgs args, const Yuv2RgbCoef c, uint32_t W, uint32_t H, uint32_t dw, uint32_t dh,
                                                           uint32_t dmask) {
  const uint32_t x0 = blockIdx.x * kWarpTileW + (threadIdx.x % kWarpLanesX) * 4, y = blockIdx.y * kWarpTileH + threadIdx.x / kWarpLanesX;
  if (x0 >= dw || y >= dh) return;
  persp_gather4<SRC, FC_TENSOR_NHWC>(args.j[blockIdx.z], c, args.e, W, H, dw, dmask, x0, y);
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
  if (!n || n > (uint32_t)kPerspBatch || (src_fc != FC_NV12 && src_fc != FC_YUV420 && src_fc != FC_P16)) return hipErrorInvalidValue;
  const uint32_t dmask = nhwc || te.dtype == VPF_TENSOR_F32 ? 15u : 7u;  // 4 px x element size per lane and plane: what the vector stores need (one interleaved plane: 16 B)
  const bool all_gather = tuning(VPF_TUNE_NV12_RGB_VARIANT) == 9;
  PerspArgs as, ag;  // (entries beyond a table's jobs are never read: blockIdx.z runs over its jobs)
  std::memset(&as, 0, sizeof(as));
  std::memset(&ag, 0, sizeof(ag));
  as.e = ag.e = te;
  uint32_t ns = 0, ngat = 0, lds = 0;
  for (uint32_t i = 0; i < n; i++) {
    const WarpNeed need = all_gather ? WarpNeed{0u} : persp_need(jobs[i].m, W, H, dw, dh);
    if (!all_gather && need.bytes <= kWarpStripMax) {
      as.j[ns++] = jobs[i];
      lds = need.bytes > lds ? need.bytes : lds;
    } else {
      ag.j[ngat++] = jobs[i];
    }
  }
  const uint32_t gx = (dw + kWarpTileW - 1) / kWarpTileW, gy = (dh + kWarpTileH - 1) / kWarpTileH;
  if (ns) {
#define VPF_PERSPS(S) do { if (nhwc) VPF_LAUNCH((k_persp_strip_nhwc<S>), dim3(gx, gy, ns), dim3(256), lds, st, as, c, W, H, dw, dh, dmask, lds); \
                           else VPF_LAUNCH((k_persp_strip<S>), dim3(gx, gy, ns), dim3(256), lds, st, as, c, W, H, dw, dh, dmask, lds); } while (0)
    if (src_fc == FC_NV12) VPF_PERSPS(FC_NV12); else if (src_fc == FC_P16) VPF_PERSPS(FC_P16); else VPF_PERSPS(FC_YUV420);
#undef VPF_PERSPS
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if (ngat) {
#define VPF_PERSPG(S) do { if (nhwc) VPF_LAUNCH((k_persp_gather_nhwc<S>), dim3(gx, gy, ngat), dim3(256), 0, st, ag, c, W, H, dw, dh, dmask); \
                           else VPF_LAUNCH((k_persp_gather<S>), dim3(gx, gy, ngat), dim3(256), 0, st, ag, c, W, H, dw, dh, dmask); } while (0)
    if (src_fc == FC_NV12) VPF_PERSPG(FC_NV12); else if (src_fc == FC_P16) VPF_PERSPG(FC_P16); else VPF_PERSPG(FC_YUV420);
#undef VPF_PERSPG
    return hipGetLastError();
  }
  return hipSuccess;
}

}  // namespace vpf
