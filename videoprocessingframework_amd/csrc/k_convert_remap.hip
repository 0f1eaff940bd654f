// k_convert_remap.hip — fused per-pixel remap of NV12 / YUV420 / P10 / P12 frames into a normalised tensor (gfx950): vpf_convert_remap_tensor.
// The remaper's way into a tensor: lens undistortion, fisheye and surround-view rigs, rectification, flow-driven warps.  A job = (whole source
// frame, a pair of coordinate maps in DEVICE memory, the destination planes) (RemapDesc, vpf_internal.h); one dispatch per job table.
//   k_remap_tile   Grid = (32 x 32 destination tiles, jobs of the table); a lane owns four consecutive pixels of one row, a workgroup 8 lanes x 32
//                  rows — k_warp_strip's layout.  A workgroup
//                  1. loads its pixels' sx and sy (one 16-B load per lane and map where the address allows, dword loads with the index clamped to
//                     dw - 1 otherwise; allocating loads: a camera's maps are read again by every frame),
//                  2. turns every pair into taps (remap_tap, vpf_job_bounds.h) and merges the taps of its in-range pixels into the tile's EXACT
//                     source window: inside a wave by DPP steps on two packed 16-bit pairs, across the four waves through eight words of LDS and
//                     one barrier,
//                  3. branches, workgroup-uniformly: no in-range pixel — the border; a window whose strip does not fit the LDS of the dispatch — four
//                     texel_rgb per pixel (warp_gather4's body on the loaded coordinates); otherwise the window is converted once into an LDS strip
//                     (strip_fill_window) and every pixel blends from bytes (warp_strip_tile's body).
// All three outcomes store through warp_store4 and run k_convert_warp.hip's fp32 operations in its order from the range test on: identical bits
// whichever form a tile takes, and on maps that hold an affine matrix's coordinates identical bits to vpf_convert_warp_tensor.
//
// WHAT THE MAPS MAY HOLD: anything.  No coordinate becomes an index before remap_tap has made it safe: a NaN in either map is replaced by a select
// (the pixel takes the border in both modes) — never handed to a min, max or median to see what comes back —, REPLICATE's max-then-min puts the
// infinities on the edge, CONSTANT's range test lets -0.0 in and the infinities out, and a coordinate that failed the test is replaced by 0,
// again by a select, BEFORE the float -> int conversion.  The conversion therefore only sees values in [0, W - 1] x [0, H - 1], every tap of every
// pixel lies inside the frame (per-tap form), and in the staged form an in-range pixel's taps lie inside the window by construction of the window
// while every other pixel's are replaced by the window's first texel.  The window's strip is compared with the LDS in 64 bits.  The maps
// themselves are read at rows < dh and columns < dw only, which the host checked against the pitches.
#include <cmath>

#include "k_convert_warp_common.h"
#include "k_job_launch.h"
#include "vpf_remap_plan.h"

namespace vpf {

// The workgroup's eight reduction words (two per wave) lie in the dynamic LDS behind the strip: the launch asks for kRemapWinBytes more than the
// strip where that stays within 64 KiB, and the strip gives them up where it does not (launch_convert_remap).
constexpr uint32_t kRemapWinBytes = 32;

// four coordinates of one map row for the lane's pixels x0 .. x0 + 3 (x0 < dw)
VPF_DEV void remap_load4(const float* map, uint32_t pitch, uint32_t x0, uint32_t y, uint32_t dw, float (&s)[4]) {
  const uint8_t* const row = reinterpret_cast<const uint8_t*>(map) + (size_t)y * pitch;
  const float* const p = reinterpret_cast<const float*>(row) + x0;
  if ((((uintptr_t)p) & 15u) == 0 && x0 + 4 <= dw) {
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    const f32x4 v = *reinterpret_cast<const f32x4*>(p);
    s[0] = v[0]; s[1] = v[1]; s[2] = v[2]; s[3] = v[3];
  } else {
    const float* const r = reinterpret_cast<const float*>(row);
#pragma unroll
    for (int k = 0; k < 4; k++) s[k] = r[x0 + k < dw ? x0 + k : dw - 1];
  }
}

// min of two pairs of 16-bit halves (v_pk_min_u16)
typedef uint16_t remap_u16x2 __attribute__((ext_vector_type(2)));
VPF_DEV uint32_t remap_pk_min(uint32_t a, uint32_t b) {
  return __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_bit_cast(remap_u16x2, a), __builtin_bit_cast(remap_u16x2, b)));
}
template <int CTRL>
VPF_DEV uint32_t remap_dpp(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, CTRL, 0xf, 0xf, false); }
// ... over the wave, every lane active: lane ^ 1 and lane ^ 2 inside a quad, the other quad of eight (row_half_mirror), the other half of sixteen
// (row_mirror) — after each step the lanes that have met hold one value —, then the four rows' values through scalar registers
VPF_DEV uint32_t remap_wave_pk_min(uint32_t v) {
  v = remap_pk_min(v, remap_dpp<0xB1>(v));   // quad_perm [1, 0, 3, 2]
  v = remap_pk_min(v, remap_dpp<0x4E>(v));   // quad_perm [2, 3, 0, 1]
  v = remap_pk_min(v, remap_dpp<0x141>(v));  // row_half_mirror
  v = remap_pk_min(v, remap_dpp<0x140>(v));  // row_mirror
  const uint32_t a = __builtin_amdgcn_readlane(v, 0), b = __builtin_amdgcn_readlane(v, 16), c = __builtin_amdgcn_readlane(v, 32),
                 d = __builtin_amdgcn_readlane(v, 48);
  return remap_pk_min(remap_pk_min(a, b), remap_pk_min(c, d));
}
// A window's axis as one packed word: lo | (0xffff - hi) << 16 — the minimum of both halves merges two of them (pixels run to 65535) — and back.
// No pixel: 0xffffffff, which unpacks to lo = 65535 > hi = 0 (no pixel has x0 > x1).
VPF_DEV uint32_t remap_pack(uint32_t lo, uint32_t hi, bool none) { return none ? 0xffffffffu : (lo | (0xffffu - hi) << 16); }

template <int SRC, int DST>  // DST = FC_TENSOR: three planes per job; FC_TENSOR_NHWC: one interleaved plane
__global__ __launch_bounds__(256) void k_remap_tile(const RemapArgs args, const Yuv2RgbCoef c, uint32_t W, uint32_t H, uint32_t dw, uint32_t dh,
                                                    uint32_t dmask, uint32_t lds_bytes) {
  const RemapDesc& J = args.j[blockIdx.z];
  const FrameDesc& f = J.f;
  const TensorEpi te = args.e;
  const bool rep = warp_rep(te);
  const uint32_t tid = threadIdx.x;
  const uint32_t xs = blockIdx.x * kWarpTileW, ys = blockIdx.y * kWarpTileH;  // the grid covers the destination exactly: xs < dw, ys < dh
  const uint32_t x0 = xs + (tid % kWarpLanesX) * 4, y = ys + tid / kWarpLanesX;
  const bool mine = x0 < dw && y < dh;
  const uint32_t nv = mine ? (dw - x0 < 4 ? dw - x0 : 4) : 0u;
  const bool vec = tensor_vec_ok<DST>(f, nv, dmask);
  // 1. the coordinates
  float sx[4] = {0.f, 0.f, 0.f, 0.f}, sy[4] = {0.f, 0.f, 0.f, 0.f};
  if (mine) {
    remap_load4(J.xm, J.xp, x0, y, dw, sx);
    remap_load4(J.ym, J.yp, x0, y, dw, sy);
  }
  // 2. the taps (pixels at and behind nv repeat the row's last one, or belong to no row: they are not stored and count for no window)
  RemapTap t[4];
  WarpWin lw = remap_win_none();
#pragma unroll
  for (int k = 0; k < 4; k++) {
    t[k] = remap_tap(sx[k], sy[k], rep, W, H);
    if ((uint32_t)k < nv) remap_win_add(lw, t[k]);
  }
  float u[3][4];
  // VPF_TUNE_NV12_RGB_VARIANT = 9: a dispatch without LDS — no strip fits, and nobody needs the window
  WarpWin w = remap_win_none();
  if (lds_bytes != 0u) {  // (a kernel argument: workgroup-uniform)
    const uint32_t px = remap_wave_pk_min(remap_pack(lw.x_lo, lw.x_hi, lw.empty)), py = remap_wave_pk_min(remap_pack(lw.y_lo, lw.y_hi, lw.empty));
    uint32_t* const words = reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(dyn_strip) + lds_bytes);  // behind the strip
    if ((tid & 63u) == 0u) { words[2 * (tid >> 6)] = px; words[2 * (tid >> 6) + 1] = py; }
    __syncthreads();
    uint32_t qx = remap_pk_min(remap_pk_min(words[0], words[2]), remap_pk_min(words[4], words[6]));
    uint32_t qy = remap_pk_min(remap_pk_min(words[1], words[3]), remap_pk_min(words[5], words[7]));
    qx = __builtin_amdgcn_readfirstlane(qx); qy = __builtin_amdgcn_readfirstlane(qy);
    w.x_lo = qx & 0xffffu; w.x_hi = 0xffffu - (qx >> 16);
    w.y_lo = qy & 0xffffu; w.y_hi = 0xffffu - (qy >> 16);
    w.empty = w.x_lo > w.x_hi;
    // 3. no in-range pixel in the tile: the border
    if (w.empty) {
      if (!mine) return;
#pragma unroll
      for (int ch = 0; ch < 3; ch++)
#pragma unroll
        for (int k = 0; k < 4; k++) u[ch][k] = warp_border(te, ch);
      warp_store4<DST>(f, x0, y, u, te, vec, nv);
      return;
    }
  }
  const WarpStrip S = warp_strip(w);  // (no LDS: never read)
  if (lds_bytes == 0u || !remap_strip_fits(S, lds_bytes)) {
    // the per-tap form: the taps of a pixel that takes the border are those of pixel (0, 0) and are loaded all the same, so the four pixels' loads overlap
    if (!mine) return;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const float fx = t[k].cx - (float)t[k].x0, fy = t[k].cy - (float)t[k].y0;
      float p00[3], p01[3], p10[3], p11[3];
      texel_rgb<SRC>(f, c, t[k].x0, t[k].y0, p00);
      texel_rgb<SRC>(f, c, t[k].x1, t[k].y0, p01);
      texel_rgb<SRC>(f, c, t[k].x0, t[k].y1, p10);
      texel_rgb<SRC>(f, c, t[k].x1, t[k].y1, p11);
#pragma unroll
      for (int ch = 0; ch < 3; ch++) {
        const float v = __builtin_truncf(bilerp(p00[ch], p01[ch], p10[ch], p11[ch], fx, fy));
        u[ch][k] = t[k].in ? v : warp_border(te, ch);
      }
    }
    warp_store4<DST>(f, x0, y, u, te, vec, nv);
    return;
  }
  // the staged form: the window once into the strip, every pixel from bytes
  uint8_t* const strip = reinterpret_cast<uint8_t*>(dyn_strip);
  strip_fill_window<SRC>(f, c, W, strip, S.base_px, w.y_lo, w.y_hi, S.ng, S.rowbytes, tid);
  __syncthreads();
  if (!mine) return;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    // an in-range pixel's taps lie in the window (it was merged from them); every other pixel reads the window's first texel and takes the border
    const bool in = t[k].in && (uint32_t)k < nv;
    const uint32_t xa = in ? t[k].x0 : w.x_lo, xb = in ? t[k].x1 : w.x_lo, ya = in ? t[k].y0 : w.y_lo, yb = in ? t[k].y1 : w.y_lo;
    const float fx = t[k].cx - (float)t[k].x0, fy = t[k].cy - (float)t[k].y0;
    const uint8_t* const ra = strip + (ya - w.y_lo) * S.rowbytes, * const rb = strip + (yb - w.y_lo) * S.rowbytes;
    const uint32_t oa = 4 * (xa - S.base_px), ob = 4 * (xb - S.base_px);
    const uint32_t q00 = *reinterpret_cast<const uint32_t*>(ra + oa), q01 = *reinterpret_cast<const uint32_t*>(ra + ob);
    const uint32_t q10 = *reinterpret_cast<const uint32_t*>(rb + oa), q11 = *reinterpret_cast<const uint32_t*>(rb + ob);
    const float v[3] = {__builtin_truncf(bilerp(ubyte<0>(q00), ubyte<0>(q01), ubyte<0>(q10), ubyte<0>(q11), fx, fy)),
                        __builtin_truncf(bilerp(ubyte<1>(q00), ubyte<1>(q01), ubyte<1>(q10), ubyte<1>(q11), fx, fy)),
                        __builtin_truncf(bilerp(ubyte<2>(q00), ubyte<2>(q01), ubyte<2>(q10), ubyte<2>(q11), fx, fy))};
#pragma unroll
    for (int ch = 0; ch < 3; ch++) u[ch][k] = t[k].in ? v[ch] : warp_border(te, ch);
  }
  warp_store4<DST>(f, x0, y, u, te, vec, nv);
}

// ------------------------------------------------------------------------------------------
// Host side.  No coordinate is known here: remap_plan (vpf_remap_plan.h) sizes the ONE dispatch's strip from the caller's hint (warp_dev_lds_bytes,
// vpf_job_bounds.h; no hint: kWarpStripMax), nothing under VPF_TUNE_NV12_RGB_VARIANT = 9.  The reduction words ride behind the strip: the launch
// asks for kRemapWinBytes more where that stays within the 64 KiB a launch takes without an attribute; where it does not (no hint, or a hint whose
// bound reaches the cap) the strip is that much shorter, and a tile whose window needed the last 32 bytes samples per tap — identical bits.
// ------------------------------------------------------------------------------------------
hipError_t launch_convert_remap(hipStream_t st, int src_fc, const Yuv2RgbCoef& c, uint32_t W, uint32_t H, uint32_t n, const RemapDesc* jobs, uint32_t dw,
                                uint32_t dh, float max_step, const TensorEpi& te, bool nhwc) {
  const RemapPlan p = remap_plan(src_fc, nhwc, te.dtype, W, H, dw, dh, max_step, tuning(VPF_TUNE_NV12_RGB_VARIANT));
  if (!p.ok || !n || n > p.per) return hipErrorInvalidValue;
  RemapArgs t;
  std::memset(&t, 0, sizeof(t));
  std::memcpy(t.j, jobs, (size_t)n * sizeof(RemapDesc));  // (entries beyond the table's jobs are never read: blockIdx.z runs over its jobs)
  t.e = te;
  const uint32_t lds_all = !p.lds ? 0u : (p.lds + kRemapWinBytes <= kWarpStripMax ? p.lds + kRemapWinBytes : kWarpStripMax);
  const uint32_t strip = lds_all ? lds_all - kRemapWinBytes : 0u;
  const dim3 grid(p.gx, p.gy, n);
  hipError_t e = hipSuccess;
  with_src_dst(src_fc, nhwc, [&](auto S, auto D) { VPF_LAUNCH_T(k_remap_tile, (S, D), grid, lds_all, st, t, c, W, H, dw, dh, p.dmask, strip); e = hipGetLastError(); });
  return e;
}

}  // namespace vpf
