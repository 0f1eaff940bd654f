// k_resize.hip — nearest / bilinear / Lanczos-3 resize of 8-bit and float surfaces (gfx950): vpf_resize, vpf_resize_batch.
// (Remap lives in k_remap.hip, the fused convert + resize kernels in k_convert_resize.hip; the three share k_bilinear_blend.h.)
//
// Replaces nppiResize_8u_C3R / _C1R (reference: NppResizeSurfacePacked3C_Impl::Run and NppResizeSurfacePlanar_Impl::Run,
// src/TC/src/Tasks.cpp:1162-1203,1217-1261) and nppiResize_32f_C3R / _C1R (:1334-1445).  The reference resizer asks NPP for
// Lanczos (:1190), which is the Task layer's default here too (north_star benchmarks bilinear: VPF_INTERP_LINEAR).
//
// Kernel families; within a filter all are bit-identical to one another (resize_plan, vpf_resize_plan.h, picks; launch_resize_planned at the
// end of this file dispatches on its answer):
//   GatherTask, LanczosGatherTask, FloatGatherTask   gather forms: any size / alignment
//   RowPairTask (k_resize_lds)    a wave stages the two source rows it needs in wave-private LDS strips (dynamic LDS sized per scale
//                                 factor) and picks taps from LDS; taps with weight exactly 0 are skipped
//   RowBandTask                   batches: R destination rows per wave, column taps once, each source row's horizontal lerp once per band
//   TileTask (k_resize_tile), TileTaskF32   tiled + separable: horizontal pass once per (source row, column) into LDS, then the vertical pass
//                                 (8-bit: bilinear up-scales of a single frame; float surfaces: Lanczos-3, bilinear with tuning 43)
//   8-bit Lanczos-3               k_lanczos_mfma.hip (the i8 matrix cores) wherever its tap windows fit (down-scales up to ~6 x, 1- / 2-channel
//                                 planes ~10 x across); LanczosTileTask below beyond them and for one small frame per dispatch;
//                                 LanczosGatherTask for what is left
//   HalfTask, Half3R16Task        exact 2x: quad-structured streaming kernels (no taps, no gathers; integer blend)
//   odd integer factors on both axes   every filter returns the centre sample -> nearest kernel (Lanczos) / RowPairTask's byte-move path
//   packed RGB taps               both taps of a row = 6 contiguous bytes: fetched as ONE 12-B window from the aligned address below
//                                 (global or LDS) and cut out with v_alignbyte_b32
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include <type_traits>
#include <utility>

#include "k_job_launch.h"
#include "k_resize_common.h"
#include "vpf_resize_plan.h"
#ifdef VPF_LAB_FORMS
#include "vpf_persist.h"
#endif

#include <atomic>

namespace vpf {

// CH interleaved channels per pixel (1, 2 or 3); 4 destination pixels per lane
template <int CH, int INTERP>
struct GatherTask {
  static constexpr int kThreads = 256;
  static VPF_DEV void run(const uint8_t* __restrict__ src, uint32_t sp, uint8_t* __restrict__ dst, uint32_t dp, const PlaneGeom& G, uint32_t bx, uint32_t by);
};
template <int CH, int INTERP>
VPF_DEV void GatherTask<CH, INTERP>::run(const uint8_t* __restrict__ src, uint32_t sp, uint8_t* __restrict__ dst, uint32_t dp, const PlaneGeom& G,
                                         uint32_t bx, uint32_t by) {
  const uint32_t sw = G.sw, sh = G.sh, dw = G.dw, dh = G.dh;
  const float scx = G.scx, scy = G.scy;
  const int vec_ok = G.vec_ok;
  const uint32_t gx = bx * 64 + (threadIdx.x & 63);
  const uint32_t y = by * 4 + (threadIdx.x >> 6);
  const uint32_t x0 = gx * 4;
  if (x0 >= dw || y >= dh) return;
  const Tap ty = make_tap<INTERP>(y, scy, sh);
  const uint8_t* r0 = src + (size_t)ty.i0 * sp;
  const uint8_t* r1 = src + (size_t)ty.i1 * sp;
  float o[4 * CH];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const uint32_t x = (x0 + k < dw) ? x0 + k : dw - 1;
    const Tap tx = make_tap<INTERP>(x, scx, sw);
#pragma unroll
    for (int c = 0; c < CH; c++)
      o[k * CH + c] = bilerp(r0[CH * tx.i0 + c], r0[CH * tx.i1 + c], r1[CH * tx.i0 + c], r1[CH * tx.i1 + c], tx.f, ty.f);
  }
  uint8_t* out = dst + (size_t)y * dp + (size_t)CH * x0;
  if (vec_ok && x0 + 4 <= dw) {
    if constexpr (CH == 3) {
      { uint32_t d0, d1, d2; pack12_trunc(o, d0, d1, d2); stg3<true>(out, d0, d1, d2); }
    } else if constexpr (CH == 2) {
      stg<true, u32x2>(out, u32x2{pack4_trunc(o[0], o[1], o[2], o[3]), pack4_trunc(o[4], o[5], o[6], o[7])});
    } else {
      stg<true, uint32_t>(out, pack4_trunc(o[0], o[1], o[2], o[3]));
    }
  } else {
    const uint32_t nv = (dw - x0 < 4 ? dw - x0 : 4) * CH;
    for (uint32_t i = 0; i < nv; i++) out[i] = (uint8_t)sat_trunc(o[i]);
  }
}

template <int CH, int INTERP>
__global__ __launch_bounds__(256) void k_resize(const uint8_t* __restrict__ src, uint32_t sp, uint32_t sw, uint32_t sh,
                                                uint8_t* __restrict__ dst, uint32_t dp, uint32_t dw, uint32_t dh,
                                                float scx, float scy, int vec_ok) {
  GatherTask<CH, INTERP>::run(src, sp, dst, dp, PlaneGeom{sw, sh, dw, dh, scx, scy, vec_ok, 0, 0, 0, 0}, blockIdx.x, blockIdx.y);
}

// ------------------------------------------------------------------------------------------
// Lanczos-3 (VPF_INTERP_LANCZOS3): what the reference's resizer asks NPP for (Tasks.cpp:1190).  Textbook separable
// 6 x 6 taps, weights normalised, indices clamped, no widening when minifying.  sin / cos come from fixed fma
// polynomials and the six taps from angle-addition identities so the host oracle reproduces the weights bit for bit
// (the test oracle restates the same sequence).  Gather kernel: lane = one destination pixel.
// ------------------------------------------------------------------------------------------
VPF_DEV uint32_t pack_i16(int32_t lo, int32_t hi) { return ((uint32_t)lo & 0xffffu) | ((uint32_t)hi << 16); }
typedef short s16x2 __attribute__((ext_vector_type(2)));
VPF_DEV int32_t dot2(uint32_t a, uint32_t b, int32_t c) {  // a.lo * b.lo + a.hi * b.hi + c on int16 halves
  return __builtin_amdgcn_sdot2(__builtin_bit_cast(s16x2, a), __builtin_bit_cast(s16x2, b), c, false);
}
// the first dot of a chain: the VOP3P encoding takes the inline constant 0 as its addend (the compiler only emits the accumulate-in-place
// VOP2 form v_dot2c_i32_i16, which wants a zeroed register per chain: three v_mov_b32 per source row of the tiled kernel)
VPF_DEV int32_t dot2z(uint32_t a, uint32_t b) {
  int32_t r;
  asm("v_dot2_i32_i16 %0, %1, %2, 0" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

template <int CH>
struct LanczosGatherTask {
  static constexpr int kThreads = 256;
  static VPF_DEV void run(const uint8_t* __restrict__ src, uint32_t sp, uint8_t* __restrict__ dst, uint32_t dp, const PlaneGeom& G, uint32_t bx, uint32_t by);
};
template <int CH>
__global__ __launch_bounds__(256) void k_resize_lanczos(const uint8_t* __restrict__ src, uint32_t sp, uint32_t sw, uint32_t sh,
                                                        uint8_t* __restrict__ dst, uint32_t dp, uint32_t dw, uint32_t dh,
                                                        float scx, float scy) {
  LanczosGatherTask<CH>::run(src, sp, dst, dp, PlaneGeom{sw, sh, dw, dh, scx, scy, 0, 0, 0, 0, 0}, blockIdx.x, blockIdx.y);
}
template <int CH>
VPF_DEV void LanczosGatherTask<CH>::run(const uint8_t* __restrict__ src, uint32_t sp, uint8_t* __restrict__ dst, uint32_t dp, const PlaneGeom& G,
                                        uint32_t bx, uint32_t by) {
  const uint32_t sw = G.sw, sh = G.sh, dw = G.dw, dh = G.dh;
  const float scx = G.scx, scy = G.scy;
  const uint32_t x = bx * 64 + (threadIdx.x & 63), y = by * 4 + (threadIdx.x >> 6);
  if (x >= dw || y >= dh) return;
  const QTap tx = quantize_ltap(make_ltap(x, scx)), ty = quantize_ltap(make_ltap(y, scy));
  uint32_t xi[6];
#pragma unroll
  for (int k = 0; k < 6; k++) {
    const int32_t i = tx.i0 + k - 2;
    xi[k] = (uint32_t)(i < 0 ? 0 : (i > (int32_t)sw - 1 ? (int32_t)sw - 1 : i)) * CH;
  }
  // vertical pass on byte-wide partial products (the arithmetic of the matrix-core kernel, restated by the oracle): z = Hr - 8192 and the
  // row's weight q as two signed bytes each, q z without its lowest partial product ql zl; taps the edge clamp puts on the same source row
  // act as one tap with the summed weight
  int32_t acc[CH];
#pragma unroll
  for (int c = 0; c < CH; c++) acc[c] = (1 << 19) + (1 << 11);
  // Horizontal sums of one source row.  The six taps of a pixel are 6 CH CONTIGUOUS bytes (unless the edge clamp folds some of them onto
  // the border pixel), so the fast path fetches them as ONE window of dwords from the 4-B aligned address below the first tap — 1 / 1 / 2
  // load instructions per row for 1 / 2 / 3 channels instead of 6 / 12 / 18 byte loads: with byte loads the kernel was bound by the rate
  // at which the memory pipeline takes instructions, nothing else —, shifts the window down to the first tap with v_alignbyte_b32, spreads
  // two taps of a channel into int16 halves with one v_perm_b32 and takes them two at a time with v_dot2_i32_i16 against the packed Q14
  // weights.  Same exact integer sums as the byte-wise path, which the lanes next to the left / right image edge (clamped taps), windows
  // that would reach past the row's last dword, and rows that are not 4-B aligned keep.
  constexpr int NW = (6 * CH + 3) / 4;        // dwords of tap bytes: 2 / 3 / 5
  constexpr int ND = NW + 1;                  // dwords loaded: the window may start up to 3 bytes below the first tap
  const uint32_t b0 = (uint32_t)CH * (uint32_t)(tx.i0 - 2), a0 = b0 & ~3u;
  const bool lane_fast = (((uintptr_t)src | sp) & 3u) == 0 && tx.i0 - 2 >= 0 && tx.i0 + 3 <= (int32_t)sw - 1 && a0 + 4u * ND <= (((uint32_t)CH * sw + 3u) & ~3u);
  const bool fast = __builtin_amdgcn_ballot_w64(!lane_fast) == 0;  // decided per WAVE: the two waves at a row's ends take the byte-wise path whole, none runs both
  const uint32_t q01 = pack_i16(tx.q[0], tx.q[1]), q23 = pack_i16(tx.q[2], tx.q[3]), q45 = pack_i16(tx.q[4], tx.q[5]);
  auto row_sums = [&](const uint8_t* r, int32_t (&h)[CH]) {
    if (fast) {
      uint32_t d[ND];
      const uint32_t* p = reinterpret_cast<const uint32_t*>(r + a0);
#pragma unroll
      for (int i = 0; i < ND; i++) d[i] = p[i];
      uint32_t w[NW + 1];
#pragma unroll
      for (int i = 0; i < NW; i++) w[i] = __builtin_amdgcn_alignbyte(d[i + 1], d[i], b0 & 3u);
      w[NW] = w[NW - 1];
#pragma unroll
      for (int c = 0; c < CH; c++) {
        uint32_t pr[3];
#pragma unroll
        for (int k = 0; k < 3; k++) {
          const int B0 = 2 * k * CH + c, B1 = (2 * k + 1) * CH + c, W0 = B0 >> 2;                 // tap 2 k in the low half, tap 2 k + 1 in the high half
          const uint32_t sel = (uint32_t)(B0 & 3) | 0x0c00u | ((uint32_t)((B1 >> 2) == W0 ? (B1 & 3) : 4 + (B1 & 3)) << 16) | 0x0c000000u;
          pr[k] = __builtin_amdgcn_perm(w[W0 + 1], w[W0], sel);
        }
        h[c] = dot2(pr[2], q45, dot2(pr[1], q23, dot2z(pr[0], q01)));
      }
    } else {
#pragma unroll
      for (int c = 0; c < CH; c++) {
        int32_t t = 0;  // exact: |t| <= 255 * sum |q| < 2^24
#pragma unroll
        for (int kx = 0; kx < 6; kx++) t += __mul24(tx.q[kx], (int32_t)r[xi[kx] + c]);  // 16-bit x 8-bit: v_mad_i32_i24 (a 32-bit multiply is quarter rate)
        h[c] = t;
      }
    }
  };
  int32_t qrun = 0;
#pragma unroll
  for (int ky = 0; ky < 6; ky++) {
    const int32_t j = ty.i0 + ky - 2, hi = (int32_t)sh - 1;
    const int32_t row = j < 0 ? 0 : (j > hi ? hi : j), nxt = j + 1 < 0 ? 0 : (j + 1 > hi ? hi : j + 1);
    qrun += ty.q[ky];
    if (ky < 5 && nxt == row) continue;  // the run goes on: its last tap carries the sum
    int32_t h[CH];
    row_sums(src + (size_t)row * sp, h);
    const int32_t ql = ((qrun + 128) & 0xff) - 128;
#pragma unroll
    for (int c = 0; c < CH; c++) {
      const int32_t z = ((h[c] + 128) >> 8) - 8192, zl = ((z + 128) & 0xff) - 128;
      acc[c] += (__mul24(qrun, z) - __mul24(ql, zl)) >> 8;  // a multiple of 256: exact (|qrun| < 2^15, |z| < 2^15)
    }
    qrun = 0;
  }
  uint8_t* o = dst + (size_t)y * dp + (size_t)CH * x;
#pragma unroll
  for (int c = 0; c < CH; c++) {
    const int32_t v = acc[c] >> 12;  // (V / 256 + 2^19 + 2^11) >> 12: round half up
    o[c] = (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
  }
}

// ------------------------------------------------------------------------------------------
// LDS-staged variant (the default when it applies): a wave produces 256 consecutive destination pixels of one
// row.  It first copies the two source rows' byte span it needs into a wave-private LDS strip with fully coalesced
// dword loads (each source byte crosses the memory pipeline once, as part of a dense 256-B wave load, instead of
// 24 scattered byte loads per lane), then every lane picks its taps out of LDS with ds_read_u8 (cheap: ~0.6 us of
// LDS issue per 720p frame chip-wide).  Same make_tap / bilerp arithmetic => bit-identical to k_resize.
// Requires: 16-B aligned source rows (pointer and pitch); span of a wave <= kResizeRowBytes (host checks the scale).
// ------------------------------------------------------------------------------------------
template <int CH, int IT /* 1-KiB loads per strip */>
struct RowPairTask {
  static constexpr int kThreads = 256;
  static VPF_DEV void run(const uint8_t* __restrict__ src, uint32_t sp, uint8_t* __restrict__ dst, uint32_t dp, const PlaneGeom& G, uint32_t bx, uint32_t by);
};
template <int CH, int IT>
__global__ __launch_bounds__(256) void k_resize_lds(const uint8_t* __restrict__ src, uint32_t sp, uint32_t sw, uint32_t sh,
                                                    uint8_t* __restrict__ dst, uint32_t dp, uint32_t dw, uint32_t dh,
                                                    float scx, float scy, int vec_ok, uint32_t rowq /* strip size in 16-B units */) {
  RowPairTask<CH, IT>::run(src, sp, dst, dp, PlaneGeom{sw, sh, dw, dh, scx, scy, vec_ok, rowq, 0, 0, 0}, blockIdx.x, blockIdx.y);
}
template <int CH, int IT>
VPF_DEV void RowPairTask<CH, IT>::run(const uint8_t* __restrict__ src, uint32_t sp, uint8_t* __restrict__ dst, uint32_t dp, const PlaneGeom& G,
                                      uint32_t bx, uint32_t by) {
  const uint32_t sw = G.sw, sh = G.sh, dw = G.dw, dh = G.dh, rowq = G.a0;
  const float scx = G.scx, scy = G.scy;
  const int vec_ok = G.vec_ok;
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const uint32_t y = by * 4 + wv;
  if (y >= dh || bx * 256 >= dw) return;
  const uint32_t xs = bx * 256, xe = (xs + 255 < dw - 1) ? xs + 255 : dw - 1;  // this wave's dst columns [xs, xe]
  const Tap ty = make_tap<VPF_INTERP_LINEAR>(y, scy, sh);
  const uint32_t first = make_tap<VPF_INTERP_LINEAR>(xs, scx, sw).i0, last = make_tap<VPF_INTERP_LINEAR>(xe, scx, sw).i1;
  const uint32_t base = (CH * first) & ~15u, nq = (CH * (last + 1) - base + 15) / 16;
  // exact-alignment shortcuts (bit-identical: fma(0, finite, t) == t): fy == 0 for the whole row (odd integer vertical
  // scale, e.g. 4K -> 720p) -> the second source row is neither loaded nor read; fx == 0 in every lane -> one tap per row
  const bool row1 = __builtin_amdgcn_readfirstlane(__float_as_uint(ty.f)) != 0u;
  Span<IT> s0, s1;
  s0.load(src + (size_t)ty.i0 * sp, base, nq, lane);
  if (row1) s1.load(src + (size_t)ty.i1 * sp, base, nq, lane);
  u32x4* st0 = dyn_strip + (wv * 2) * rowq;
  u32x4* st1 = st0 + rowq;
  s0.store(st0, nq, lane);
  if (row1) s1.store(st1, nq, lane);
  wave_lds_sync();
  const uint32_t x0 = xs + lane * 4;
  if (x0 >= dw) return;
  const uint8_t* r0 = reinterpret_cast<const uint8_t*>(st0);
  const uint8_t* r1 = reinterpret_cast<const uint8_t*>(st1);
  if constexpr (CH == 3) {
    // Odd integer scale factors (kernel-uniform on x, row-uniform on y; 4K -> 720p is 3x): every destination pixel IS the
    // source pixel k x + (k - 1) / 2 — exactly, in float as well (all values < 2^24) — and the general path's float round
    // trip (+ 0.5, truncate) returns its bytes unchanged.  So the bytes are moved as bytes: one 8-B LDS window +
    // v_alignbyte_b32 per pixel, three v_perm_b32 per four pixels.
    const uint32_t kx = (uint32_t)scx;
    if (!row1 && (float)kx == scx && (kx & 1u) && sw == kx * dw && vec_ok && x0 + 4 <= dw) {
      uint32_t e[4];
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const uint32_t a = 3 * (kx * (x0 + k) + (kx >> 1)) - base;
        const uint32_t* q = reinterpret_cast<const uint32_t*>(r0 + (a & ~3u));
        e[k] = __builtin_amdgcn_alignbyte(q[1], q[0], a & 3u);  // R G B of the pixel in bytes 0..2
      }
      stg3<true>(dst + (size_t)y * dp + 3 * (size_t)x0, __builtin_amdgcn_perm(e[1], e[0], 0x04020100u),
                  __builtin_amdgcn_perm(e[2], e[1], 0x05040201u), __builtin_amdgcn_perm(e[3], e[2], 0x06050402u));
      return;
    }
  }
  float o[4 * CH];
  const ColTaps<CH> T = make_col_taps<CH>(base, x0, dw, sw, scx);
  rowpair_blend4<CH>(r0, r1, row1, ty.f, T, o);
  store_blend4<CH>(dst + (size_t)y * dp + (size_t)CH * x0, o, vec_ok && x0 + 4 <= dw, dw - x0 < 4 ? dw - x0 : 4);
}

// ------------------------------------------------------------------------------------------
// Row band: the row-pair blend over R consecutive destination rows per wave, for vertical scale factors up to 2 (down) and any up-scale.
// What a row-pair wave spends outside the blend proper — the column taps (53 of its ~360 VALU instructions at CH = 3), the strip
// geometry, a memory round trip — depends on the columns only, and below 2x neighbouring destination rows share source rows.  A band
// wave stages the contiguous source rows [i0(first row), i1(last row)] once (all loads in flight together; the launcher sizes LDS for
// the at most floor((R - 1) scy) + 3 rows of a band), computes the column taps once, and walks down its destination rows keeping the
// HORIZONTAL lerps of the two current source rows in registers: a source row's lerp fma(fx, p1 - p0, p0) is evaluated once per band and
// reused by every destination row that blends it (1.5 evaluations per destination row at a 1.5x down-scale instead of 2, 0.5 at a 2x
// up-scale), leaving fma(fy, bot - top, top) + 0.5 per row.  Same operations on the same operands as bilerp() -> the bytes of
// RowPairTask and of the oracle (zero weights need no special case: fma(0, finite, t) == t and every staged byte is finite).
// Used where the launch still has plenty of workgroups (batches); a single small frame keeps one row per wave.
// ------------------------------------------------------------------------------------------
// destination pixels per lane: 4, or 8 = 512 columns per wave on 1-channel planes in the `P1 = 8` instantiations (a wave's per-row fixed
// work is the same whatever the channel count; the launcher picks them when 512-column chunks fill the planes' rows well)
// (band_px: vpf_classes.h)
template <int CH, int R, int IT = 2 /* 1-KiB staging passes per strip */, int P1 = 4 /* pixels per lane on 1-channel planes */, bool MULTI = false /* several bands per wave */>
struct RowBandTask {
  static constexpr int kThreads = 256;
  static constexpr int kSlots = kBandSlots * 2 / IT < 2 * R + 1 ? kBandSlots * 2 / IT : 2 * R + 1;  // a band touches at most floor((R - 1) scy) + 3 source rows, scy <= 2
  static constexpr int kPx = band_px(CH, P1);
  static constexpr bool kPx4 = CH == 3 && R == 16 && IT == 1;  // strips hold four bytes per pixel (band_rows sizes them: vpf_bound_strip_bytes_px4)
  static VPF_DEV void run(const uint8_t* __restrict__ src, uint32_t sp, uint8_t* __restrict__ dst, uint32_t dp, const PlaneGeom& G, uint32_t bx, uint32_t by) {
    run_w(src, sp, dst, dp, G, bx, by * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6));
  }
  // one wave's share: column chunk bx, wave row wrow
  static VPF_DEV void run_w(const uint8_t* __restrict__ src, uint32_t sp, uint8_t* __restrict__ dst, uint32_t dp, const PlaneGeom& G, uint32_t bx, uint32_t wrow);
#ifdef VPF_LAB_FORMS
  // the persistent launch (k_planes_mp_persist, k_resize_common.h): chunk after chunk while the stream hands out chunks of CH-channel planes
  template <class Stream>
  static VPF_DEV void run_chunks(BandChunk& c, Stream& ts, const PlaneTable& PT);
#endif
};
template <int CH, int R, int IT, int P1, bool MULTI>
VPF_DEV void RowBandTask<CH, R, IT, P1, MULTI>::run_w(const uint8_t* __restrict__ src, uint32_t sp, uint8_t* __restrict__ dst, uint32_t dp, const PlaneGeom& G,
                                           uint32_t bx, uint32_t wrow) {
  constexpr int PX = kPx;
  constexpr uint32_t W = 64 * PX;  // destination columns per wave
  const uint32_t sw = G.sw, sh = G.sh, dw = G.dw, dh = G.dh, rowq = G.a0, slots = G.a1;
  const uint32_t nb = (MULTI && G.a2) ? G.a2 : 1u;  // bands per wave (launcher): the wave walks down nb consecutive bands of its columns
  const float scx = G.scx, scy = G.scy;
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  uint32_t ya = wrow * (R * nb);
  if (ya >= dh || bx * W >= dw) return;
  const uint32_t xs = bx * W, xe = (xs + W - 1 < dw - 1) ? xs + W - 1 : dw - 1;
  const uint32_t first = make_tap<VPF_INTERP_LINEAR>(xs, scx, sw).i0, last = make_tap<VPF_INTERP_LINEAR>(xe, scx, sw).i1;
  // packed RGB in 16-row bands (up-scales: a source pixel is tapped ~4 times per row it is staged): "px4" strips (k_bilinear_blend.h) — pixels
  // [first & ~3, last + 1] widened to R G B x in units of four; else the packed bytes in 16-B units.  (Down-scales tap a staged pixel ~1.3
  // times and pay a third more LDS per row — 1080p -> 720p: four workgroups per CU instead of five, 1.71 -> 2.33 us; profiles/r06_c_*.)
  constexpr bool X4 = kPx4;
  const uint32_t base_px = first & ~3u;
  const uint32_t base = X4 ? 3u * base_px : (CH * first) & ~15u, nq = X4 ? (last + 2 - base_px + 3) / 4 : (CH * (last + 1) - base + 15) / 16;
  const uint32_t lim = (CH * sw + 15u) & ~15u;  // bytes of a source row that may be read
  u32x4* const strips = dyn_strip + (size_t)wv * slots * rowq;
  // the source rows [i0(first row), i1(last row)] of one band (the launcher guarantees r_hi - r_lo < slots <= kSlots) ...
  uint32_t yb, r_lo, r_hi;
  auto rows_of = [&](uint32_t y0) {
    yb = (y0 + R - 1 < dh - 1) ? y0 + R - 1 : dh - 1;
    r_lo = __builtin_amdgcn_readfirstlane(make_tap<VPF_INTERP_LINEAR>(y0, scy, sh).i0);
    r_hi = __builtin_amdgcn_readfirstlane(make_tap<VPF_INTERP_LINEAR>(yb, scy, sh).i1);
  };
  // ... requested (all loads in flight together) ...
  typename std::conditional<X4, Span4<IT>, Span<IT>>::type rows[kSlots];
  auto request = [&]() {
#pragma unroll
    for (int k = 0; k < kSlots; k++)
      if (r_lo + k <= r_hi) {
        if constexpr (X4) rows[k].load(src + (size_t)(r_lo + k) * sp, base, nq, lane, lim);
        else rows[k].load(src + (size_t)(r_lo + k) * sp, base, nq, lane);
      }
  };
  // ... and written to the wave's strips
  auto commit = [&]() {
#pragma unroll
    for (int k = 0; k < kSlots; k++)
      if (r_lo + k <= r_hi) rows[k].store(strips + (size_t)k * rowq, nq, lane);
    wave_lds_sync();
  };
  const uint32_t x0 = xs + lane * PX;
  const bool draws = x0 < dw;  // lanes past the picture's right edge stage, but blend nothing
  const bool vec4 = G.vec_ok && x0 + PX <= dw;
  const uint32_t nv = !draws ? 0u : dw - x0 < (uint32_t)PX ? dw - x0 : (uint32_t)PX;
  rows_of(ya);
  request();
  // once for all rows of all bands (evaluated while the first band's rows are in flight)
  typename std::conditional<X4, ColTapsX, ColTaps<CH, PX>>::type T;
  if constexpr (X4) T = make_col_taps_x(base_px, x0, dw, sw, scx);
  else T = make_col_taps<CH, PX>(base, x0, dw, sw, scx);
  VPF_WAVE_MARK(0);  // (lab builds: setup done)
  // With nb > 1 the source rows of band k + 1 are requested right after band k's have been written to the strips — the registers are free
  // again — and arrive while band k is blended: the wave hides its own memory latency, and its fixed part (task decode, column taps) is
  // paid once per nb bands.  Measured on 1- and 2-channel planes, whose waves are short (profiles/r04_bilinear_ablate.txt: staging, blend
  // and the fixed part are nearly additive there).
  BandWalk<CH, PX> walk;
  for (uint32_t k = 0; k < nb; k++) {
    commit();
    VPF_WAVE_MARK(1);  // (lab builds: the first band's rows have arrived and sit in LDS)
    const Tap row_taps = band_row_taps(ya, yb, scy, sh);  // every lane active here
    const uint32_t ya_k = ya, yb_k = yb, r_lo_k = r_lo;
    ya += R;
    const bool more = k + 1 < nb && ya < dh;
    if (more) { rows_of(ya); request(); }
    if (draws) {
      band_blend_rows<CH, R, PX>(reinterpret_cast<const uint8_t*>(strips), rowq * 16, r_lo_k, ya_k, yb_k, row_taps, T, walk, [&](uint32_t y, const float* o) {
        store_blend4<CH, PX>(dst + (size_t)y * dp + (size_t)CH * x0, o, vec4, nv);
      });
    }
    VPF_WAVE_MARK(2);  // (lab builds: the first band is blended and its stores are issued)
    if (!more) return;
    wave_lds_sync();  // the blend's LDS reads are done before the next band's rows overwrite the strips
  }
}

#ifdef VPF_LAB_FORMS
// The same walk for the persistent launch: a wave works through CHUNKS (runs of bands of one column chunk) that a ChunkStream hands out.  Inside
// a chunk it is the march form; at a chunk's last band the NEXT chunk — any frame, plane (of the same channel count) or column — is fetched from
// the stream and ITS first rows are requested before this band is blended and stored; the column taps and the walk are rebuilt after the blend.
template <int CH, int R, int IT, int P1, bool MULTI>
template <class Stream>
VPF_DEV void RowBandTask<CH, R, IT, P1, MULTI>::run_chunks(BandChunk& c, Stream& ts, const PlaneTable& PT) {
  constexpr int PX = kPx;
  constexpr uint32_t W = 64 * PX;
  constexpr bool X4 = kPx4;
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const uint32_t rowq = PT.g[c.pi].a0, slots = PT.g[c.pi].a1;  // one strip size for the launch
  u32x4* const strips = dyn_strip + (size_t)wv * slots * rowq;
  // the staging side: the chunk whose source rows are being requested ...
  const uint8_t* s_src = nullptr;
  uint32_t s_sp = 0, s_sh = 0, s_dh = 0, s_base = 0, s_nq = 0, s_lim = 0, s_bpx = 0;
  float s_scy = 0.f;
  uint32_t ya = 0, y_end = 0, yb = 0, r_lo = 0, r_hi = 0;
  auto stage_of = [&](const BandChunk& k) {
    const PlaneGeom& g = PT.g[k.pi];
    const uint32_t xs = k.bx * W, xe = (xs + W - 1 < g.dw - 1) ? xs + W - 1 : g.dw - 1;
    const uint32_t first = __builtin_amdgcn_readfirstlane(make_tap<VPF_INTERP_LINEAR>(xs, g.scx, g.sw).i0), last = __builtin_amdgcn_readfirstlane(make_tap<VPF_INTERP_LINEAR>(xe, g.scx, g.sw).i1);
    s_bpx = first & ~3u;
    s_base = X4 ? 3u * s_bpx : (CH * first) & ~15u;
    s_nq = X4 ? (last + 2 - s_bpx + 3) / 4 : (CH * (last + 1) - s_base + 15) / 16;
    s_lim = (CH * g.sw + 15u) & ~15u;
    s_src = k.src; s_sp = k.sp; s_sh = g.sh; s_dh = g.dh; s_scy = g.scy;
    ya = k.band0 * R;
    y_end = (k.band0 + k.nb) * R < g.dh ? (k.band0 + k.nb) * R : g.dh;
  };
  auto rows_of = [&](uint32_t y0) {
    yb = (y0 + R - 1 < s_dh - 1) ? y0 + R - 1 : s_dh - 1;
    r_lo = __builtin_amdgcn_readfirstlane(make_tap<VPF_INTERP_LINEAR>(y0, s_scy, s_sh).i0);
    r_hi = __builtin_amdgcn_readfirstlane(make_tap<VPF_INTERP_LINEAR>(yb, s_scy, s_sh).i1);
  };
  typename std::conditional<X4, Span4<IT>, Span<IT>>::type rows[kSlots];
  auto request = [&]() {
#pragma unroll
    for (int k = 0; k < kSlots; k++)
      if (r_lo + k <= r_hi) {
        if constexpr (X4) rows[k].load(s_src + (size_t)(r_lo + k) * s_sp, s_base, s_nq, lane, s_lim);
        else rows[k].load(s_src + (size_t)(r_lo + k) * s_sp, s_base, s_nq, lane);
      }
  };
  auto commit = [&]() {
#pragma unroll
    for (int k = 0; k < kSlots; k++)
      if (r_lo + k <= r_hi) rows[k].store(strips + (size_t)k * rowq, s_nq, lane);
    wave_lds_sync();
  };
  // ... and the drawing side: the chunk whose bands are being blended
  uint8_t* d_dst = nullptr;
  uint32_t d_dp = 0, d_x0 = 0, d_nv = 0;
  bool d_draws = false, d_vec4 = false;
  typename std::conditional<X4, ColTapsX, ColTaps<CH, PX>>::type T;
  auto draw_of = [&](const BandChunk& k) {  // (after stage_of(k): s_base / s_bpx are k's)
    const PlaneGeom& g = PT.g[k.pi];
    d_x0 = k.bx * W + lane * PX;
    d_draws = d_x0 < g.dw;
    d_vec4 = g.vec_ok && d_x0 + PX <= g.dw;
    d_nv = !d_draws ? 0u : g.dw - d_x0 < (uint32_t)PX ? g.dw - d_x0 : (uint32_t)PX;
    d_dst = k.dst; d_dp = k.dp;
    if constexpr (X4) T = make_col_taps_x(s_bpx, d_x0, g.dw, g.sw, g.scx);
    else T = make_col_taps<CH, PX>(s_base, d_x0, g.dw, g.sw, g.scx);
  };
  stage_of(c);
  rows_of(ya);
  request();
  draw_of(c);
  BandWalk<CH, PX> walk;
  for (;;) {
    commit();
    const Tap row_taps = band_row_taps(ya, yb, s_scy, s_sh);  // every lane active here
    const uint32_t ya_k = ya, yb_k = yb, r_lo_k = r_lo;
    ya += R;
    const bool same = ya < y_end;
    BandChunk nx{nullptr, nullptr, 0, 0, 0, 0, 0, 0};
    bool cross = false;
    if (same) {
      rows_of(ya);
      request();
    } else {
      nx = ts.next();
      cross = nx.nb != 0 && PT.ch[nx.pi] == (uint32_t)CH;
      if (cross) { stage_of(nx); rows_of(ya); request(); }
    }
    if (d_draws) {
      uint8_t* const dst = d_dst;
      const uint32_t dp = d_dp, x0 = d_x0, nv = d_nv;
      const bool vec4 = d_vec4;
      band_blend_rows<CH, R, PX>(reinterpret_cast<const uint8_t*>(strips), rowq * 16, r_lo_k, ya_k, yb_k, row_taps, T, walk, [&](uint32_t y, const float* o) {
        store_blend4<CH, PX>(dst + (size_t)y * dp + (size_t)CH * x0, o, vec4, nv);
      });
    }
    if (!same) {
      if (!cross) { c = nx; return; }  // (the caller's wave_lds_sync stands between this blend and the next task's strips)
      draw_of(nx);
      walk = BandWalk<CH, PX>();
    }
    wave_lds_sync();  // the blend's LDS reads are done before the next band's rows overwrite the strips
  }
}
#endif  // VPF_LAB_FORMS

// ------------------------------------------------------------------------------------------
// Tiled, separable BILINEAR resize for up-scales (8-bit Lanczos-3 lives in k_lanczos_mfma.hip; k_resize_lanczos / k_resize remain the
// any-input gather forms).  The horizontal lerp of (source row r, destination column x) does not depend on the destination row, and
// in an up-scale several destination rows sit between the same two source rows, so a workgroup that owns a tile of 64 columns x TY
// rows computes each of them ONCE:
//   phase 0  the tile's whole source window goes to LDS in one sweep of dense 16-B loads;
//   phase 1  wave w takes source rows w, w + WPB, ...: H[row][channel][column] = fma(fx, p1 - p0, p0) (k_resize's bilerp) as floats in LDS;
//   phase 2  every lane blends two H rows per destination pixel: fma(fy, bottom - top, top) + 0.5, truncating pack.
// Same arithmetic as the gather forms -> bit-identical to them and to the oracle.  2x up-scale: 0.7 horizontal lerps per
// destination pixel instead of 2.
// WPB = waves per workgroup (4 or 8): 8 halves the number of source rows a wave walks through one after the other, which is what
// the duration of a single-frame launch (one round of workgroups, each a chain of dependent steps) is made of.
// TileTaskF32 below is the same tiling for float surfaces (bilinear and Lanczos-3).
// ------------------------------------------------------------------------------------------
// (kLzStripQ = 128: at most 2 KiB of source bytes per row of a tile; kTileStagePasses = 6 staging loads a thread may have in flight: vpf_classes.h)

template <int CH, int WPB>
struct TileTask {
  static constexpr int kThreads = 64 * WPB;
  static VPF_DEV void run(const uint8_t* __restrict__ src, uint32_t sp, uint8_t* __restrict__ dst, uint32_t dp, const PlaneGeom& P, uint32_t bx, uint32_t by);
};
template <int CH, int WPB>
VPF_DEV void TileTask<CH, WPB>::run(const uint8_t* __restrict__ src, uint32_t sp, uint8_t* __restrict__ dst, uint32_t dp, const PlaneGeom& P,
                                    uint32_t bx, uint32_t by) {
  // dynamic LDS: RAW[nr_cap][rowq x 16 B] source bytes | H[nr_cap][CH][64] floats | WY[tile_rows][8] floats (fy, -, ..., top H row, bottom H row)
  constexpr uint32_t T = 64 * WPB;
  const uint32_t sw = P.sw, sh = P.sh, dw = P.dw, dh = P.dh, tile_rows = P.a0, nr_cap = P.a1, rowq = P.a2, lshift = P.a3;
  const float scx = P.scx, scy = P.scy;
  u32x4* const RAW = dyn_strip;
  float* const H = reinterpret_cast<float*>(dyn_strip + (size_t)nr_cap * rowq);
  float* const WY = H + (size_t)nr_cap * CH * 64;
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const uint32_t xf = bx * 64, xl = (xf + 63 < dw - 1) ? xf + 63 : dw - 1;
  if (xf >= dw) return;  // a narrower plane of a multi-plane launch (workgroup-uniform)
  const uint32_t x = xf + lane, xc = x < dw ? x : dw - 1;  // lanes past the right edge compute a duplicate, never stored
  const uint32_t y0 = by * tile_rows, yl = (y0 + tile_rows - 1 < dh - 1) ? y0 + tile_rows - 1 : dh - 1;
  auto clampi = [](int32_t i, int32_t hi) { return (uint32_t)(i < 0 ? 0 : (i > hi ? hi : i)); };
  const int32_t R0 = (int32_t)make_tap<VPF_INTERP_LINEAR>(y0, scy, sh).i0, R1 = (int32_t)make_tap<VPF_INTERP_LINEAR>(yl, scy, sh).i1;
  const uint32_t first = make_tap<VPF_INTERP_LINEAR>(xf, scx, sw).i0, last = make_tap<VPF_INTERP_LINEAR>(xl, scx, sw).i1;
  const uint32_t nrows = (uint32_t)(R1 - R0 + 1);
  const uint32_t base = (CH * first) & ~15u, nq = (CH * (last + 1) - base + 15) / 16;
  // Phase 0: the tile's whole source window goes to LDS in ONE sweep — every 16-B unit of every source row is requested before the
  // first one is waited for, so the workgroup pays one memory latency, not one per source row.  The weights are computed while the
  // loads are in flight.
  const uint32_t scol = threadIdx.x & ((1u << lshift) - 1u), srow0 = threadIdx.x >> lshift, srows = T >> lshift;
  u32x4 stage[kTileStagePasses];
#pragma unroll
  for (int k = 0; k < kTileStagePasses; k++) {
    const uint32_t r = srow0 + k * srows;
    if (r < nrows && scol < nq) stage[k] = ldg<false, u32x4>(src + (size_t)clampi(R0 + (int32_t)r, (int32_t)sh - 1) * sp + base + 16 * scol);
  }
  if (threadIdx.x < tile_rows) {  // vertical weights: one lane per destination row
    const uint32_t y = y0 + threadIdx.x, yc = y < dh ? y : dh - 1;
    const Tap t = make_tap<VPF_INTERP_LINEAR>(yc, scy, sh);
    WY[threadIdx.x * 8] = t.f;
    WY[threadIdx.x * 8 + 6] = __int_as_float((int32_t)t.i0 - R0);
    WY[threadIdx.x * 8 + 7] = __int_as_float((int32_t)t.i1 - R0);
  }
#pragma unroll
  for (int k = 0; k < kTileStagePasses; k++) {
    const uint32_t r = srow0 + k * srows;
    if (r < nrows && scol < nq) RAW[r * rowq + scol] = stage[k];
  }
  __syncthreads();
  const Tap tx = make_tap<VPF_INTERP_LINEAR>(xc, scx, sw);
  const uint32_t xo0 = tx.i0 * CH - base, xo1 = tx.i1 * CH - base;
  const float wx = tx.f;
  // Phase 1, horizontal: wave w takes source rows w, w + WPB, ...; rows are independent of one another (no barrier inside the loop)
  for (uint32_t r = wv; r < nrows; r += WPB) {
    const uint8_t* b = reinterpret_cast<const uint8_t*>(RAW + (size_t)r * rowq);
    if constexpr (CH == 3) {
      float t0[3], t1[3];  // at the right image edge i1 == i0 and the window's second tap is junk with weight exactly 0
      strip_window_taps(b, xo0, t0, t1);
#pragma unroll
      for (int c = 0; c < 3; c++) H[(r * 3 + c) * 64 + lane] = __builtin_fmaf(wx, t1[c] - t0[c], t0[c]);
    } else {
#pragma unroll
      for (int c = 0; c < CH; c++) {
        const float p0 = (float)b[xo0 + c], p1 = (float)b[xo1 + c];
        H[(r * CH + c) * 64 + lane] = __builtin_fmaf(wx, p1 - p0, p0);
      }
    }
  }
  __syncthreads();
  // phase 2: a lane owns 4 consecutive columns of one destination row (a wave = 4 rows x 64 columns): H comes out of LDS
  // as one ds_read_b128 per (tap, channel) and the pixels leave as one 4-12 B vector store per lane
  typedef float f32x4 __attribute__((ext_vector_type(4)));
  const uint32_t cg = lane & 15, rsub = lane >> 4, x0 = xf + 4 * cg;
  for (uint32_t yb = 0; yb < tile_rows; yb += 4 * WPB) {
    const uint32_t yy = yb + wv * 4 + rsub, y = y0 + yy;
    if (yy >= tile_rows || y >= dh || x0 >= dw) continue;
    const uint32_t r0 = (uint32_t)__float_as_int(WY[yy * 8 + 6]), r1 = (uint32_t)__float_as_int(WY[yy * 8 + 7]);
    // packed fp32 (v_pk_fma_f32 / v_pk_add_f32: two independent IEEE operations per instruction at the issue cost of one —
    // tools/probe_valu_rate.hip, profiles/r02_probe_valu_rate.txt); every component goes through exactly the scalar form's
    // operations, so results are bit-identical to it
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    f32x2 acc[CH][2];
    const float fy = WY[yy * 8];
    const f32x2 fy2 = {fy, fy};
#pragma unroll
    for (int c = 0; c < CH; c++) {
      const f32x4 top = *reinterpret_cast<const f32x4*>(&H[(r0 * CH + c) * 64 + 4 * cg]);
      const f32x4 bot = *reinterpret_cast<const f32x4*>(&H[(r1 * CH + c) * 64 + 4 * cg]);
      const f32x2 t0 = {top[0], top[1]}, t1 = {top[2], top[3]}, b0 = {bot[0], bot[1]}, b1 = {bot[2], bot[3]};
      acc[c][0] = __builtin_elementwise_fma(fy2, b0 - t0, t0);
      acc[c][1] = __builtin_elementwise_fma(fy2, b1 - t1, t1);
    }
    float o[4 * CH];  // pixel-major; + 0.5, then the truncating pack of every bilinear kernel
#pragma unroll
    for (int c = 0; c < CH; c++)
#pragma unroll
      for (int hlf = 0; hlf < 2; hlf++) {
        const f32x2 v = acc[c][hlf] + f32x2{0.5f, 0.5f};
        o[(2 * hlf) * CH + c] = v[0]; o[(2 * hlf + 1) * CH + c] = v[1];
      }
    uint8_t* out = dst + (size_t)y * dp + (size_t)CH * x0;
    if (P.vec_ok && x0 + 4 <= dw) {
      if constexpr (CH == 3) {
        { uint32_t d0, d1, d2; pack12_trunc(o, d0, d1, d2); stg3<true>(out, d0, d1, d2); }
      } else if constexpr (CH == 2) {
        stg<true, u32x2>(out, u32x2{pack4_trunc(o[0], o[1], o[2], o[3]), pack4_trunc(o[4], o[5], o[6], o[7])});
      } else {
        stg<true, uint32_t>(out, pack4_trunc(o[0], o[1], o[2], o[3]));
      }
    } else {
      const uint32_t nv = (dw - x0 < 4 ? dw - x0 : 4) * CH;
      for (uint32_t i = 0; i < nv; i++) out[i] = (uint8_t)sat_trunc(o[i]);
    }
  }
}

// The same tiling for 32-bit float surfaces (RGB_32F: CH = 3 interleaved, RGB_32F_PLANAR: CH = 1 per plane; reference
// NppResizeSurfacePacked32F3C_Impl / NppResizeSurface32FPlanar_Impl, Tasks.cpp:1334-1445).  Samples are floats, so both passes are
// fp32 fma chains in FloatGatherTask's order (tap 0 first, row 0 first, accumulators starting at 0; bilinear: its two lerps): results
// are bit-identical to the gather form; nothing is rounded or clamped.  Geometry fields as for TileTask, with 4-byte samples; the
// window is staged in rounds of kTileStagePasses units per thread (a float row is four times as long as a byte row).
template <int CH, bool LZ, int WPB>
struct TileTaskF32 {
  static constexpr int kThreads = 64 * WPB;
  static VPF_DEV void run(const uint8_t* __restrict__ src, uint32_t sp, uint8_t* __restrict__ dst, uint32_t dp, const PlaneGeom& P, uint32_t bx, uint32_t by);
};
template <int CH, bool LZ, int WPB>
VPF_DEV void TileTaskF32<CH, LZ, WPB>::run(const uint8_t* __restrict__ src, uint32_t sp, uint8_t* __restrict__ dst, uint32_t dp, const PlaneGeom& P,
                                           uint32_t bx, uint32_t by) {
  // dynamic LDS: RAW[nr_cap][rowq x 16 B] source floats | H[nr_cap][CH][64] floats | WY[tile_rows][8] floats | WX[7][64] floats (Lanczos)
  constexpr int NT = LZ ? 6 : 2;
  constexpr uint32_t T = 64 * WPB;
  const uint32_t sw = P.sw, sh = P.sh, dw = P.dw, dh = P.dh, tile_rows = P.a0, nr_cap = P.a1, rowq = P.a2, lshift = P.a3;
  const float scx = P.scx, scy = P.scy;
  u32x4* const RAW = dyn_strip;
  float* const H = reinterpret_cast<float*>(dyn_strip + (size_t)nr_cap * rowq);
  float* const WY = H + (size_t)nr_cap * CH * 64;
  float* const WX = WY + (size_t)tile_rows * 8;
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const uint32_t xf = bx * 64, xl = (xf + 63 < dw - 1) ? xf + 63 : dw - 1;
  if (xf >= dw) return;
  const uint32_t x = xf + lane, xc = x < dw ? x : dw - 1;
  const uint32_t y0 = by * tile_rows, yl = (y0 + tile_rows - 1 < dh - 1) ? y0 + tile_rows - 1 : dh - 1;
  auto clampi = [](int32_t i, int32_t hi) { return (uint32_t)(i < 0 ? 0 : (i > hi ? hi : i)); };
  int32_t R0, R1;
  uint32_t first, last;
  if constexpr (LZ) {
    R0 = ltap_i0(y0, scy) - 2; R1 = ltap_i0(yl, scy) + 3;
    first = clampi(ltap_i0(xf, scx) - 2, (int32_t)sw - 1); last = clampi(ltap_i0(xl, scx) + 3, (int32_t)sw - 1);
  } else {
    R0 = (int32_t)make_tap<VPF_INTERP_LINEAR>(y0, scy, sh).i0; R1 = (int32_t)make_tap<VPF_INTERP_LINEAR>(yl, scy, sh).i1;
    first = make_tap<VPF_INTERP_LINEAR>(xf, scx, sw).i0; last = make_tap<VPF_INTERP_LINEAR>(xl, scx, sw).i1;
  }
  const uint32_t nrows = (uint32_t)(R1 - R0 + 1);
  const uint32_t base = (4 * CH * first) & ~15u, nq = (4 * CH * (last + 1) - base + 15) / 16;
  const uint32_t scol = threadIdx.x & ((1u << lshift) - 1u), srow0 = threadIdx.x >> lshift, srows = T >> lshift;
  for (uint32_t rb = 0; rb < nrows; rb += kTileStagePasses * srows) {  // usually one round; the units of a round are all in flight together
    u32x4 stage[kTileStagePasses];
#pragma unroll
    for (int k = 0; k < kTileStagePasses; k++) {
      const uint32_t r = rb + srow0 + k * srows;
      if (r < nrows && scol < nq) stage[k] = ldg<false, u32x4>(src + (size_t)clampi(R0 + (int32_t)r, (int32_t)sh - 1) * sp + base + 16 * scol);
    }
#pragma unroll
    for (int k = 0; k < kTileStagePasses; k++) {
      const uint32_t r = rb + srow0 + k * srows;
      if (r < nrows && scol < nq) RAW[r * rowq + scol] = stage[k];
    }
  }
  const uint32_t vt = LZ ? threadIdx.x - 64 : threadIdx.x;
  if (vt < tile_rows) {
    const uint32_t y = y0 + vt, yc = y < dh ? y : dh - 1;
    if constexpr (LZ) {
      const LTap t = make_ltap(yc, scy);
#pragma unroll
      for (int k = 0; k < 6; k++) WY[vt * 8 + k] = t.w[k];
      WY[vt * 8 + 6] = __int_as_float(t.i0 - 2 - R0);
    } else {
      const Tap t = make_tap<VPF_INTERP_LINEAR>(yc, scy, sh);
      WY[vt * 8] = t.f;
      WY[vt * 8 + 6] = __int_as_float((int32_t)t.i0 - R0);
      WY[vt * 8 + 7] = __int_as_float((int32_t)t.i1 - R0);
    }
  }
  if constexpr (LZ) {
    if (wv == 0) {
      const LTap tx = make_ltap(xc, scx);
#pragma unroll
      for (int k = 0; k < 6; k++) WX[k * 64 + lane] = tx.w[k];
      WX[6 * 64 + lane] = __int_as_float(tx.i0);
    }
  }
  __syncthreads();
  uint32_t xo[NT];  // float index of tap k's first channel inside the staged row
  float wx[NT];
  if constexpr (LZ) {
    const int32_t i0 = __float_as_int(WX[6 * 64 + lane]);
#pragma unroll
    for (int k = 0; k < 6; k++) { xo[k] = (clampi(i0 + k - 2, (int32_t)sw - 1) * 4 * CH - base) >> 2; wx[k] = WX[k * 64 + lane]; }
  } else {
    const Tap tx = make_tap<VPF_INTERP_LINEAR>(xc, scx, sw);
    xo[0] = (tx.i0 * 4 * CH - base) >> 2; xo[1] = (tx.i1 * 4 * CH - base) >> 2; wx[0] = tx.f; wx[1] = 0.f;
  }
  for (uint32_t r = wv; r < nrows; r += WPB) {
    const float* b = reinterpret_cast<const float*>(RAW + (size_t)r * rowq);
    float v[NT][CH];  // all taps requested before the first is used
#pragma unroll
    for (int k = 0; k < NT; k++)
#pragma unroll
      for (int c = 0; c < CH; c++) v[k][c] = b[xo[k] + c];
#pragma unroll
    for (int c = 0; c < CH; c++) {
      float ra;
      if constexpr (LZ) {
        ra = 0.f;
#pragma unroll
        for (int k = 0; k < 6; k++) ra = __builtin_fmaf(wx[k], v[k][c], ra);
      } else {
        ra = __builtin_fmaf(wx[0], v[1][c] - v[0][c], v[0][c]);
      }
      H[(r * CH + c) * 64 + lane] = ra;
    }
  }
  __syncthreads();
  typedef float f32x4 __attribute__((ext_vector_type(4)));
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  const uint32_t cg = lane & 15, rsub = lane >> 4, x0 = xf + 4 * cg;
  for (uint32_t yb = 0; yb < tile_rows; yb += 4 * WPB) {
    const uint32_t yy = yb + wv * 4 + rsub, y = y0 + yy;
    if (yy >= tile_rows || y >= dh || x0 >= dw) continue;
    const uint32_t r0 = (uint32_t)__float_as_int(WY[yy * 8 + 6]);
    f32x2 acc[CH][2];
    if constexpr (LZ) {
#pragma unroll
      for (int c = 0; c < CH; c++) acc[c][0] = acc[c][1] = f32x2{0.f, 0.f};
#pragma unroll
      for (int ky = 0; ky < 6; ky++) {
        const float wy = WY[yy * 8 + ky];
        const f32x2 wy2 = {wy, wy};
#pragma unroll
        for (int c = 0; c < CH; c++) {
          const f32x4 hv = *reinterpret_cast<const f32x4*>(&H[((r0 + ky) * CH + c) * 64 + 4 * cg]);
          acc[c][0] = __builtin_elementwise_fma(wy2, f32x2{hv[0], hv[1]}, acc[c][0]);
          acc[c][1] = __builtin_elementwise_fma(wy2, f32x2{hv[2], hv[3]}, acc[c][1]);
        }
      }
    } else {
      const uint32_t r1 = (uint32_t)__float_as_int(WY[yy * 8 + 7]);
      const float fy = WY[yy * 8];
      const f32x2 fy2 = {fy, fy};
#pragma unroll
      for (int c = 0; c < CH; c++) {
        const f32x4 top = *reinterpret_cast<const f32x4*>(&H[(r0 * CH + c) * 64 + 4 * cg]);
        const f32x4 bot = *reinterpret_cast<const f32x4*>(&H[(r1 * CH + c) * 64 + 4 * cg]);
        const f32x2 t0 = {top[0], top[1]}, t1 = {top[2], top[3]}, b0 = {bot[0], bot[1]}, b1 = {bot[2], bot[3]};
        acc[c][0] = __builtin_elementwise_fma(fy2, b0 - t0, t0);
        acc[c][1] = __builtin_elementwise_fma(fy2, b1 - t1, t1);
      }
    }
    float* out = reinterpret_cast<float*>(dst + (size_t)y * dp) + (size_t)CH * x0;
    float o[4 * CH];  // pixel-major
#pragma unroll
    for (int c = 0; c < CH; c++) { o[c] = acc[c][0][0]; o[CH + c] = acc[c][0][1]; o[2 * CH + c] = acc[c][1][0]; o[3 * CH + c] = acc[c][1][1]; }
    if (P.vec_ok && x0 + 4 <= dw) {  // 16-B aligned rows: CH 16-B stores per lane
#pragma unroll
      for (int q = 0; q < CH; q++) stg<true, f32x4>(out + 4 * q, f32x4{o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]});
    } else {
      const uint32_t nv = (dw - x0 < 4 ? dw - x0 : 4) * CH;
      for (uint32_t i = 0; i < nv; i++) out[i] = o[i];
    }
  }
}
// single plane, single frame: scalar arguments, source side first (kernarg preload: see VPF_ONE_SRC_PARAMS in vpf_internal.h)
template <int CH, int WPB>
__global__ __launch_bounds__(64 * WPB) void k_resize_tile(const uint8_t* __restrict__ src, uint32_t sp, uint32_t sw, uint32_t sh,
                                                          uint8_t* __restrict__ dst, uint32_t dp, uint32_t dw, uint32_t dh,
                                                          float scx, float scy, uint32_t tile_rows, uint32_t nr_cap, uint32_t rowq, uint32_t lshift,
                                                          int vec_ok) {
  TileTask<CH, WPB>::run(src, sp, dst, dp, PlaneGeom{sw, sh, dw, dh, scx, scy, vec_ok, tile_rows, nr_cap, rowq, lshift}, blockIdx.x, blockIdx.y);
}
// ------------------------------------------------------------------------------------------
// Tiled, separable 8-bit LANCZOS-3 for what the matrix-core kernel (k_lanczos_mfma.hip) does not take: packed RGB beyond ~6 x and any plane
// beyond ~10 x across / ~6 x down (its tap windows and its four-tile ring end there), and ONE small frame per dispatch, where this kernel's
// short waves finish sooner than that kernel's latency chain (lanczos_single_prefers_tile and the 1-MB rule of resize_plan, vpf_resize_plan.h).
// Same integer filter definition as that kernel, the gather kernel and the oracle: exact Q14 horizontal sums,
// Hr = (H + 128) >> 8, vertical taps on byte-wide partial products with clamped taps merged per source row.  A workgroup of WPB waves owns
// a tile of 64 columns x TY rows:
//   phase 0  the tile's whole source window goes to LDS in one sweep of dense 16-B loads (edge tiles: the pixels clamped taps fall on are
//            replicated into the rows' margins, so every lane's six taps are contiguous bytes in every tile); wave 0 evaluates the 64
//            column weight sets meanwhile, wave 1 the row sets (merged where the clamp folds taps onto one row, split into signed bytes);
//   phase 1  wave w takes source rows w, w + WPB, ...: aligned dword reads, v_alignbyte_b32, one v_perm_b32 per tap pair, two taps per
//            v_dot2_i32_i16; z = Hr - 8192 goes to LDS as the int16 pair (z, zh) with z = 256 zh + zl;
//   phase 2  a lane owns 4 consecutive columns of one destination row: per vertical tap and channel ONE v_dot2_i32_i16 of (z, zh)
//            against (qh, ql) — qh z + ql zh = (q z - ql zl) >> 8 exactly —, then (acc + 2^19 + 2^11) >> 12, clamped.
// (The gather kernel — a lane per destination pixel, six taps times six rows from global memory — remains for rows that are not 16-B
// aligned and tiles that do not fit LDS.)
// ------------------------------------------------------------------------------------------
template <int CH, int WPB>
struct LanczosTileTask {
  static constexpr int kThreads = 64 * WPB;
  static VPF_DEV void run(const uint8_t* __restrict__ src, uint32_t sp, uint8_t* __restrict__ dst, uint32_t dp, const PlaneGeom& P, uint32_t bx, uint32_t by);
};
template <int CH, int WPB>
VPF_DEV void LanczosTileTask<CH, WPB>::run(const uint8_t* __restrict__ src, uint32_t sp, uint8_t* __restrict__ dst, uint32_t dp, const PlaneGeom& P,
                                           uint32_t bx, uint32_t by) {
  // dynamic LDS: RAW[nr_cap][rowq x 16 B] source bytes | H[nr_cap][CH][64] (z | zh << 16) | WY[tile_rows][8] (six (qh | ql << 16), first H row) | WX[4][64]
  constexpr uint32_t T = 64 * WPB;
  const uint32_t sw = P.sw, sh = P.sh, dw = P.dw, dh = P.dh, tile_rows = P.a0, nr_cap = P.a1, rowq = P.a2, lshift = P.a3;
  const float scx = P.scx, scy = P.scy;
  u32x4* const RAW = dyn_strip;
  uint32_t* const H = reinterpret_cast<uint32_t*>(dyn_strip + (size_t)nr_cap * rowq);
  uint32_t* const WY = H + (size_t)nr_cap * CH * 64;
  uint32_t* const WX = WY + (size_t)tile_rows * 8;  // [4][64]: three Q14 weight pairs and the first tap index of every column
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const uint32_t xf = bx * 64, xl = (xf + 63 < dw - 1) ? xf + 63 : dw - 1;
  if (xf >= dw) return;  // a narrower plane of a multi-plane launch (workgroup-uniform)
  const uint32_t x = xf + lane, xc = x < dw ? x : dw - 1;  // lanes past the right edge compute a duplicate, never stored
  const uint32_t y0 = by * tile_rows, yl = (y0 + tile_rows - 1 < dh - 1) ? y0 + tile_rows - 1 : dh - 1;
  auto clampi = [](int32_t i, int32_t hi) { return (uint32_t)(i < 0 ? 0 : (i > hi ? hi : i)); };
  const int32_t R0 = ltap_i0(y0, scy) - 2, R1 = ltap_i0(yl, scy) + 3;
  const int32_t fv = ltap_i0(xf, scx) - 2, lv = ltap_i0(xl, scx) + 3;  // the tile's VIRTUAL source columns: before 0 / after sw - 1 they are copies of the edge pixel
  const uint32_t first = clampi(fv, (int32_t)sw - 1), last = clampi(lv, (int32_t)sw - 1);
  const uint32_t nrows = (uint32_t)(R1 - R0 + 1);
  const uint32_t base = (CH * first) & ~15u, nq = (CH * (last + 1) - base + 15) / 16;
  const uint32_t scol = threadIdx.x & ((1u << lshift) - 1u), srow0 = threadIdx.x >> lshift, srows = T >> lshift;
  u32x4 stage[kTileStagePasses];
#pragma unroll
  for (int k = 0; k < kTileStagePasses; k++) {
    const uint32_t r = srow0 + k * srows;
    if (r < nrows && scol < nq) stage[k] = ldg<false, u32x4>(src + (size_t)clampi(R0 + (int32_t)r, (int32_t)sh - 1) * sp + base + 16 * scol);
  }
  const uint32_t vt = threadIdx.x - 64;  // lane of wave 1 (and later waves) that owns destination row y0 + vt
  if (vt < tile_rows) {
    const uint32_t y = y0 + vt, yc = y < dh ? y : dh - 1;
    const QTap t = quantize_ltap(make_ltap(yc, scy));
    int32_t q[6];
#pragma unroll
    for (int k = 0; k < 6; k++) q[k] = t.q[k];
#pragma unroll
    for (int k = 0; k < 5; k++)  // taps the clamp folds onto one source row act as ONE tap with the summed weight, carried by the last of them
      if (clampi(t.i0 + k - 2, (int32_t)sh - 1) == clampi(t.i0 + k - 1, (int32_t)sh - 1)) { q[k + 1] += q[k]; q[k] = 0; }
#pragma unroll
    for (int k = 0; k < 6; k++) {
      const int32_t ql = ((q[k] + 128) & 0xff) - 128, qh = (q[k] - ql) >> 8;
      WY[vt * 8 + k] = pack_i16(qh, ql);
    }
    WY[vt * 8 + 6] = (uint32_t)(t.i0 - 2 - R0);
  }
  if (wv == 0) {
    const QTap tx = quantize_ltap(make_ltap(xc, scx));
#pragma unroll
    for (int k = 0; k < 3; k++) WX[k * 64 + lane] = pack_i16(tx.q[2 * k], tx.q[2 * k + 1]);
    WX[3 * 64 + lane] = (uint32_t)tx.i0;
  }
#pragma unroll
  for (int k = 0; k < kTileStagePasses; k++) {
    const uint32_t r = srow0 + k * srows;
    if (r < nrows && scol < nq) RAW[r * rowq + scol + 1] = stage[k];  // rows start one 16-B unit into their LDS row: room for up to 3 replicated pixels on the left
  }
  if (fv < 0 || lv > (int32_t)sw - 1) {  // workgroup-uniform: a tile on the left / right image edge
    __syncthreads();
    const int32_t nl = fv < 0 ? -fv * CH : 0, nr = lv > (int32_t)sw - 1 ? (lv - ((int32_t)sw - 1)) * CH : 0;  // bytes to add on each side (<= 3 px)
    for (uint32_t t = threadIdx.x; t < nrows * 16; t += T) {
      uint8_t* b = reinterpret_cast<uint8_t*>(RAW + (size_t)(t >> 4) * rowq) + 16;
      const int32_t i = (int32_t)(t & 15);
      if (i < nl) b[CH * fv + i] = b[i % CH];                                                    // base == 0 on the left edge
      if (i < nr) b[CH * sw - base + (uint32_t)i] = b[CH * (sw - 1) - base + (uint32_t)i % CH];
    }
  }
  __syncthreads();
  uint32_t qx[3];
  const int32_t i0 = (int32_t)WX[3 * 64 + lane];
  const uint32_t xo0 = (uint32_t)((i0 - 2) * CH - (int32_t)base + 16);  // the six taps are contiguous bytes from here
#pragma unroll
  for (int k = 0; k < 3; k++) qx[k] = WX[k * 64 + lane];
  // Phase 1, horizontal, two source rows per iteration (both rows' LDS reads are in flight before the first is used)
  {
    constexpr int NE = (6 * CH + 3) / 4;  // dwords of the lead-free run
    const uint32_t lead = xo0 & 3u, qoff = xo0 & ~3u;
    auto fetch = [&](uint32_t r, uint32_t* d) {
      const uint32_t* q = reinterpret_cast<const uint32_t*>(reinterpret_cast<const uint8_t*>(RAW + (size_t)r * rowq) + qoff);
#pragma unroll
      for (int i = 0; i <= NE; i++) d[i] = q[i];
    };
    auto hdots = [&](uint32_t r, const uint32_t* d) {
      uint32_t e[NE];
#pragma unroll
      for (int i = 0; i < NE; i++) e[i] = __builtin_amdgcn_alignbyte(d[i + 1], d[i], lead);
#pragma unroll
      for (int c = 0; c < CH; c++) {
        uint32_t p0, p1, p2;  // (tap 0 | tap 1 << 16), (tap 2 | tap 3 << 16), (tap 4 | tap 5 << 16) of channel c
        if constexpr (CH == 3) {  // bytes c, 3 + c | 6 + c, 9 + c | 12 + c, 15 + c of the run
          p0 = __builtin_amdgcn_perm(e[1], e[0], 0x0c000c00u | ((3u + c) << 16) | (uint32_t)c);
          p1 = __builtin_amdgcn_perm(e[2], e[1], 0x0c000c00u | ((5u + c) << 16) | (2u + c));
          p2 = __builtin_amdgcn_perm(e[4], e[3], 0x0c000c00u | ((3u + c) << 16) | (uint32_t)c);
        } else if constexpr (CH == 2) {  // bytes c, 2 + c of dwords 0, 1, 2
          const uint32_t sel = 0x0c000c00u | ((2u + c) << 16) | (uint32_t)c;
          p0 = __builtin_amdgcn_perm(e[0], e[0], sel); p1 = __builtin_amdgcn_perm(e[1], e[1], sel); p2 = __builtin_amdgcn_perm(e[2], e[2], sel);
        } else {  // bytes 0, 1 | 2, 3 | 4, 5
          p0 = __builtin_amdgcn_perm(e[0], e[0], 0x0c010c00u); p1 = __builtin_amdgcn_perm(e[0], e[0], 0x0c030c02u); p2 = __builtin_amdgcn_perm(e[1], e[1], 0x0c010c00u);
        }
        const int32_t h = dot2(p2, qx[2], dot2(p1, qx[1], dot2z(p0, qx[0])));  // exact: |h| < 2^24
        const int32_t z = ((h + 128) >> 8) - 8192, zh = (z + 128) >> 8;
        H[(r * CH + c) * 64 + lane] = pack_i16(z, zh);
      }
    };
    for (uint32_t r = wv; r < nrows; r += 2 * WPB) {
      uint32_t da[NE + 1], db[NE + 1];
      const bool two = r + WPB < nrows;  // wave-uniform
      fetch(r, da);
      if (two) fetch(r + WPB, db);
      hdots(r, da);
      if (two) hdots(r + WPB, db);
    }
  }
  __syncthreads();
  // phase 2: a lane owns 4 consecutive columns of one destination row (a wave = 4 rows x 64 columns)
  const uint32_t cg = lane & 15, rsub = lane >> 4, x0 = xf + 4 * cg;
  for (uint32_t yb = 0; yb < tile_rows; yb += 4 * WPB) {
    const uint32_t yy = yb + wv * 4 + rsub, y = y0 + yy;
    if (yy >= tile_rows || y >= dh || x0 >= dw) continue;
    const uint32_t r0 = WY[yy * 8 + 6];
    int32_t acc[CH][4];
#pragma unroll
    for (int c = 0; c < CH; c++)
#pragma unroll
      for (int i = 0; i < 4; i++) acc[c][i] = (1 << 19) + (1 << 11);
#pragma unroll
    for (int ky = 0; ky < 6; ky++) {
      const uint32_t wq = WY[yy * 8 + ky];
#pragma unroll
      for (int c = 0; c < CH; c++) {
        const u32x4 hv = *reinterpret_cast<const u32x4*>(&H[((r0 + ky) * CH + c) * 64 + 4 * cg]);
#pragma unroll
        for (int i = 0; i < 4; i++) acc[c][i] = dot2(hv[i], wq, acc[c][i]);  // qh z + ql zh
      }
    }
    // pixel-major bytes, four per dword: shift, clamp and pack in six instructions per dword (shift12_sat_pack4, k_resize_common.h)
    auto val = [&](int b) { return (uint32_t)acc[b % CH][b / CH]; };  // byte b of the lane's 4 CH output bytes
    uint32_t ow[CH];
#pragma unroll
    for (int q = 0; q < CH; q++) ow[q] = shift12_sat_pack4(val(4 * q), val(4 * q + 1), val(4 * q + 2), val(4 * q + 3));
    uint8_t* out = dst + (size_t)y * dp + (size_t)CH * x0;
    if (P.vec_ok && x0 + 4 <= dw) {
      if constexpr (CH == 3) {
        stg3<true>(out, ow[0], ow[1], ow[2]);
      } else if constexpr (CH == 2) {
        stg<true, u32x2>(out, u32x2{ow[0], ow[1]});
      } else {
        stg<true, uint32_t>(out, ow[0]);
      }
    } else {
      const uint32_t nv = (dw - x0 < 4 ? dw - x0 : 4) * CH;
      for (uint32_t i = 0; i < nv; i++) out[i] = (uint8_t)(ow[i >> 2] >> (8 * (i & 3)));
    }
  }
}
template <int CH, int WPB>
__global__ __launch_bounds__(64 * WPB) void k_resize_lztile(const uint8_t* __restrict__ src, uint32_t sp, uint32_t sw, uint32_t sh,
                                                            uint8_t* __restrict__ dst, uint32_t dp, uint32_t dw, uint32_t dh,
                                                            float scx, float scy, uint32_t tile_rows, uint32_t nr_cap, uint32_t rowq, uint32_t lshift,
                                                            int vec_ok) {
  LanczosTileTask<CH, WPB>::run(src, sp, dst, dp, PlaneGeom{sw, sh, dw, dh, scx, scy, vec_ok, tile_rows, nr_cap, rowq, lshift}, blockIdx.x, blockIdx.y);
}
template <int CH> struct TileLz4 : LanczosTileTask<CH, 4> {};
template <int CH> struct TileLz8 : LanczosTileTask<CH, 8> {};

// the template-template forms k_planes_mp wants
template <int CH> struct TileBl4 : TileTask<CH, 4> {};
template <int CH> struct TileBl8 : TileTask<CH, 8> {};
template <int CH> struct RowPair1 : RowPairTask<CH, 1> {};
template <int CH> struct RowPair2 : RowPairTask<CH, 2> {};
template <int CH> struct RowPair3 : RowPairTask<CH, 3> {};
template <int CH> struct RowPair4 : RowPairTask<CH, 4> {};
template <int CH> struct RowBand2 : RowBandTask<CH, 2> {};
template <int CH> struct RowBand4 : RowBandTask<CH, 4> {};
template <int CH> struct RowBand8 : RowBandTask<CH, 8> {};
template <int CH> struct RowBand8n : RowBandTask<CH, 8, 1> {};    // narrow strips (<= 1 KiB): 16 slots
template <int CH> struct RowBand16n : RowBandTask<CH, 16, 1> {};
template <int CH> struct RowBand8w : RowBandTask<CH, 8, 1, 8> {};   // ... and 8 pixels per lane on 1-channel planes
template <int CH> struct RowBand16w : RowBandTask<CH, 16, 1, 8> {};
template <int CH> struct RowBand4wm : RowBandTask<CH, 4, 1, 8, true> {};  // the march form: 4-row bands, several per wave (plan_band)

// ------------------------------------------------------------------------------------------
// Exact 2x bilinear down-scale (4K -> 1080p ...): s = 2 d + 0.5 exactly, so every destination pixel is the fx = fy = 0.5
// bilerp of one 2 x 2 block: no tap arithmetic, no LDS, pure streaming.  Lane = 4 destination pixels = 8 source pixels x 2
// rows (CH x 8 contiguous bytes per row, loaded as 8-B units), one CH x 4-B store.  Bit-identical to the general kernels.
// Requires dw % 4 == 0, 8-B aligned source rows, 4-B (8-B for CH == 2) aligned destination rows.
// ------------------------------------------------------------------------------------------
template <int CH>
struct HalfTask {
  static constexpr int kThreads = 256;
  static VPF_DEV void run(const uint8_t* __restrict__ src, uint32_t sp, uint8_t* __restrict__ dst, uint32_t dp, const PlaneGeom& G, uint32_t bx, uint32_t by);
};
template <int CH>
__global__ __launch_bounds__(256) void k_resize_half(const uint8_t* __restrict__ src, uint32_t sp, uint8_t* __restrict__ dst, uint32_t dp,
                                                     uint32_t dw, uint32_t dh) {
  HalfTask<CH>::run(src, sp, dst, dp, PlaneGeom{2 * dw, 2 * dh, dw, dh, 2.f, 2.f, 1, 0, 0, 0, 0}, blockIdx.x, blockIdx.y);
}
template <int CH>
VPF_DEV void HalfTask<CH>::run(const uint8_t* __restrict__ src, uint32_t sp, uint8_t* __restrict__ dst, uint32_t dp, const PlaneGeom& G, uint32_t bx,
                               uint32_t by) {
  const uint32_t dw = G.dw, dh = G.dh;
  const uint32_t gx = bx * 64 + (threadIdx.x & 63), y = by * 4 + (threadIdx.x >> 6);
  const uint32_t x0 = gx * 4;
  if (x0 >= dw || y >= dh) return;
  uint32_t ra[2 * CH], rb[2 * CH];  // 8 source pixels of rows 2y and 2y + 1
  const uint8_t* pa = src + (size_t)(2 * y) * sp + (size_t)CH * 2 * x0;
  const uint8_t* pb = pa + sp;
#pragma unroll
  for (int j = 0; j < CH; j++) {
    const u32x2 a = ldg<true, u32x2>(pa + 8 * j), b = ldg<true, u32x2>(pb + 8 * j);
    ra[2 * j] = a[0]; ra[2 * j + 1] = a[1]; rb[2 * j] = b[0]; rb[2 * j + 1] = b[1];
  }
  float o[4 * CH];
#pragma unroll
  for (int e = 0; e < 4; e++)
#pragma unroll
    for (int c = 0; c < CH; c++) {
      const int i0 = CH * 2 * e + c, i1 = i0 + CH;  // byte index of the two horizontal taps inside the lane's run
      auto byte = [](const uint32_t* d, int i) { return (float)((d[i >> 2] >> (8 * (i & 3))) & 0xffu); };
      o[e * CH + c] = bilerp(byte(ra, i0), byte(ra, i1), byte(rb, i0), byte(rb, i1), 0.5f, 0.5f);
    }
  uint8_t* out = dst + (size_t)y * dp + (size_t)CH * x0;
  if constexpr (CH == 3) {
    { uint32_t d0, d1, d2; pack12_trunc(o, d0, d1, d2); stg3<true>(out, d0, d1, d2); }
  } else if constexpr (CH == 2) {
    stg<true, u32x2>(out, u32x2{pack4_trunc(o[0], o[1], o[2], o[3]), pack4_trunc(o[4], o[5], o[6], o[7])});
  } else {
    stg<true, uint32_t>(out, pack4_trunc(o[0], o[1], o[2], o[3]));
  }
}

// tiled separable launch (Lanczos always; bilinear when up-scaling, where the horizontal lerp is shared by several
// destination rows): needs 16-B aligned source rows and a 64-column span that fits the 2-KiB strip.  Returns false when
// it does not apply.
// Exact 2x down-scale of packed RGB / BGR in the r16 form: a wave turns two source rows x 1024 px into 512 destination
// pixels.  Every global access is a dense 1-KiB wave access (load_run48 on the way in, an LDS-transposed 1 KiB + 512 B on
// the way out; k_resize_half's 8-B lane loads reach ~0.6 of that rate), and the blend is integer: with fx = fy = 0.5 the
// bilinear blend of four 8-bit taps is exactly (p00 + p01 + p10 + p11 + 2) >> 2 (see k_convert_half), taken per channel
// from the de-interleaved dwords with two v_dot4_u32_u8 whose weights (64 on two bytes) pick a horizontal pair of each row.
// Requires sw % 32 == 0 and 16-B aligned source / destination rows.
struct Half3R16Task {
  static constexpr int kThreads = 256;
  static VPF_DEV void run(const uint8_t* __restrict__ src, uint32_t sp, uint8_t* __restrict__ dst, uint32_t dp, const PlaneGeom& G, uint32_t bx, uint32_t by);
};
__global__ __launch_bounds__(256) void k_resize_half3_r16(const uint8_t* __restrict__ src, uint32_t sp, uint8_t* __restrict__ dst, uint32_t dp,
                                                          uint32_t sw, uint32_t chunks_x, uint32_t n_tasks) {
  Half3R16Task::run(src, sp, dst, dp, PlaneGeom{sw, 0, sw >> 1, 0, 2.f, 2.f, 1, chunks_x, n_tasks, 0, 0}, blockIdx.x, 0);
}
VPF_DEV void Half3R16Task::run(const uint8_t* __restrict__ src, uint32_t sp, uint8_t* __restrict__ dst, uint32_t dp, const PlaneGeom& G, uint32_t bx,
                               uint32_t /*by*/) {
  __shared__ u32x4 tile[4 * 192];  // 3 KiB per wave
  const uint32_t sw = G.sw, chunks_x = G.a0, n_tasks = G.a1;
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const uint32_t wt = bx * 4 + wv;
  if (wt >= n_tasks) return;
  const uint32_t y = wt / chunks_x, chunk = wt - y * chunks_x;
  u32x4* t = tile + wv * 192;
  uint32_t top[12], bot[12];
  u32x4 qt[3], qb[3];  // both rows' loads are in flight before the first transpose
  run48_fetch(src + (size_t)(2 * y) * sp, chunk * 3072, 3 * sw, lane, qt);
  run48_fetch(src + (size_t)(2 * y + 1) * sp, chunk * 3072, 3 * sw, lane, qb);
  run48_transpose(t, lane, qt, top);
  wave_sync();  // every lane has read its top bytes before the tile is rewritten
  run48_transpose(t, lane, qb, bot);
  uint32_t v[3][8];  // channel value of destination pixel i in byte 1
#pragma unroll
  for (int g = 0; g < 4; g++) {
    uint32_t tc[3], bc[3];
    deint4(top[3 * g], top[3 * g + 1], top[3 * g + 2], tc[0], tc[1], tc[2]);
    deint4(bot[3 * g], bot[3 * g + 1], bot[3 * g + 2], bc[0], bc[1], bc[2]);
#pragma unroll
    for (int c = 0; c < 3; c++) {
      v[c][2 * g] = __builtin_amdgcn_udot4(tc[c], 0x00004040u, __builtin_amdgcn_udot4(bc[c], 0x00004040u, 128u, false), false);
      v[c][2 * g + 1] = __builtin_amdgcn_udot4(tc[c], 0x40400000u, __builtin_amdgcn_udot4(bc[c], 0x40400000u, 128u, false), false);
    }
  }
  auto gather4 = [](uint32_t v0, uint32_t v1, uint32_t v2, uint32_t v3) {  // byte 1 of four registers -> one dword
    return __builtin_amdgcn_perm(__builtin_amdgcn_perm(v3, v2, 0x0c0c0501u), __builtin_amdgcn_perm(v1, v0, 0x0c0c0501u), 0x05040100u);
  };
  uint32_t* tw = reinterpret_cast<uint32_t*>(t);
  wave_sync();
#pragma unroll
  for (int g = 0; g < 2; g++) {  // 4 px -> 3 dwords, twice
    const int q = 4 * g;
    tw[lane * 6 + 3 * g] = gather4(v[0][q], v[1][q], v[2][q], v[0][q + 1]);
    tw[lane * 6 + 3 * g + 1] = gather4(v[1][q + 1], v[2][q + 1], v[0][q + 2], v[1][q + 2]);
    tw[lane * 6 + 3 * g + 2] = gather4(v[2][q + 2], v[0][q + 3], v[1][q + 3], v[2][q + 3]);
  }
  wave_sync();
  uint8_t* row = dst + (size_t)y * dp;
  const uint32_t row_bytes = 3 * (sw >> 1);
#pragma unroll
  for (int k = 0; k < 2; k++) {  // the wave's 1536 B leave as one dense 1-KiB store and one 512-B store
    const uint32_t idx = k * 64 + lane, off = chunk * 1536 + idx * 16;
    if (idx < 96 && off < row_bytes) stg<true, u32x4>(row + off, t[idx]);
  }
}

// ------------------------------------------------------------------------------------------
// 32-bit float surfaces (RGB_32F: CH = 3 interleaved, RGB_32F_PLANAR: CH = 1 per plane; reference
// NppResizeSurfacePacked32F3C_Impl / NppResizeSurface32FPlanar_Impl, Tasks.cpp:1334-1445): the same taps and operation
// order as the 8-bit kernels on float samples; the result is neither rounded nor clamped.  Lane = one destination pixel
// (CH x 4 B per lane: a wave stores 256-768 contiguous bytes).
// ------------------------------------------------------------------------------------------
template <int CH>
struct FloatPx { float c[CH]; };  // one pixel of an RGB_32F (CH = 3) / planar float (CH = 1) surface: 4-B aligned, loaded as one 4 * CH-byte access
template <int CH, int INTERP>
struct FloatGatherTask {
  static constexpr int kThreads = 256;
  static VPF_DEV void run(const uint8_t* __restrict__ src, uint32_t sp, uint8_t* __restrict__ dst, uint32_t dp, const PlaneGeom& G, uint32_t bx, uint32_t by);
};
template <int CH, int INTERP>
__global__ __launch_bounds__(256) void k_resize_f32(const uint8_t* __restrict__ src, uint32_t sp, uint32_t sw, uint32_t sh,
                                                    uint8_t* __restrict__ dst, uint32_t dp, uint32_t dw, uint32_t dh,
                                                    float scx, float scy) {
  FloatGatherTask<CH, INTERP>::run(src, sp, dst, dp, PlaneGeom{sw, sh, dw, dh, scx, scy, 0, 0, 0, 0, 0}, blockIdx.x, blockIdx.y);
}
template <int CH, int INTERP>
VPF_DEV void FloatGatherTask<CH, INTERP>::run(const uint8_t* __restrict__ src, uint32_t sp, uint8_t* __restrict__ dst, uint32_t dp, const PlaneGeom& G,
                                              uint32_t bx, uint32_t by) {
  const uint32_t sw = G.sw, sh = G.sh, dw = G.dw, dh = G.dh;
  const float scx = G.scx, scy = G.scy;
  const uint32_t x = bx * 64 + (threadIdx.x & 63), y = by * 4 + (threadIdx.x >> 6);
  if (x >= dw || y >= dh) return;
  float* o = reinterpret_cast<float*>(dst + (size_t)y * dp) + (size_t)CH * x;
  if constexpr (INTERP == VPF_INTERP_LANCZOS3) {
    const LTap tx = make_ltap(x, scx), ty = make_ltap(y, scy);
    uint32_t xi[6];
#pragma unroll
    for (int k = 0; k < 6; k++) {
      const int32_t i = tx.i0 + k - 2;
      xi[k] = (uint32_t)(i < 0 ? 0 : (i > (int32_t)sw - 1 ? (int32_t)sw - 1 : i)) * CH;
    }
    float acc[CH];
#pragma unroll
    for (int c = 0; c < CH; c++) acc[c] = 0.f;
#pragma unroll
    for (int ky = 0; ky < 6; ky++) {
      const int32_t j = ty.i0 + ky - 2;
      const float* r = reinterpret_cast<const float*>(src + (size_t)(j < 0 ? 0 : (j > (int32_t)sh - 1 ? (int32_t)sh - 1 : j)) * sp);
      // a row's taps are requested together and only then accumulated: left alone, the compiler sinks each load to its
      // fma and the lane waits out one memory round trip per tap (36 * CH of them)
      // and a pixel's CH floats travel as one 4 * CH-byte load (the kernel is bound by the number of load instructions)
      float v[6][CH];
#pragma unroll
      for (int kx = 0; kx < 6; kx++) {
        const FloatPx<CH> px = *reinterpret_cast<const FloatPx<CH>*>(r + xi[kx]);
#pragma unroll
        for (int c = 0; c < CH; c++) v[kx][c] = px.c[c];
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int c = 0; c < CH; c++) {
        float ra = 0.f;
#pragma unroll
        for (int kx = 0; kx < 6; kx++) ra = __builtin_fmaf(tx.w[kx], v[kx][c], ra);
        acc[c] = __builtin_fmaf(ty.w[ky], ra, acc[c]);
      }
    }
#pragma unroll
    for (int c = 0; c < CH; c++) o[c] = acc[c];
  } else {
    const Tap tx = make_tap<INTERP>(x, scx, sw), ty = make_tap<INTERP>(y, scy, sh);
    const float* r0 = reinterpret_cast<const float*>(src + (size_t)ty.i0 * sp);
    const float* r1 = reinterpret_cast<const float*>(src + (size_t)ty.i1 * sp);
    FloatPx<CH> q00 = *reinterpret_cast<const FloatPx<CH>*>(r0 + CH * tx.i0), q01 = {}, q10 = {}, q11 = {};
    if constexpr (INTERP != VPF_INTERP_NEAREST) {
      q01 = *reinterpret_cast<const FloatPx<CH>*>(r0 + CH * tx.i1);
      q10 = *reinterpret_cast<const FloatPx<CH>*>(r1 + CH * tx.i0); q11 = *reinterpret_cast<const FloatPx<CH>*>(r1 + CH * tx.i1);
    }
#pragma unroll
    for (int c = 0; c < CH; c++) {
      if constexpr (INTERP == VPF_INTERP_NEAREST) {
        o[c] = q00.c[c];
      } else {
        const float p00 = q00.c[c], p01 = q01.c[c], p10 = q10.c[c], p11 = q11.c[c];
        const float top = __builtin_fmaf(tx.f, p01 - p00, p00), bot = __builtin_fmaf(tx.f, p11 - p10, p10);
        o[c] = __builtin_fmaf(ty.f, bot - top, top);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------
// The host side.  WHICH kernels a call takes is resize_plan (vpf_resize_plan.h: a pure function of the shapes, the alignment of the planes
// and the four knobs, tested on the CPU); launch_resize_planned below reduces the alignment bits, asks it once and dispatches on the answer.
// A run-time value becomes a template argument through with_value / with_bool (k_job_launch.h) or through a FORM: one of the named multi-plane
// tasks above (TileBl8, RowPair2, RowBand4wm ...).  k_planes_mp takes the name itself, a plane launched on its own the task the name derives
// from (k_plane_batch<RowBandTask<CH, 4, 1, 8, true>>): the instantiations are the ones there always were.
// ------------------------------------------------------------------------------------------
template <template <int> class MP> struct Form {};
template <int CH, int IT> RowPairTask<CH, IT> form_base(const RowPairTask<CH, IT>&);
template <int CH, int R, int IT, int P1, bool M> RowBandTask<CH, R, IT, P1, M> form_base(const RowBandTask<CH, R, IT, P1, M>&);
template <int CH, int W> TileTask<CH, W> form_base(const TileTask<CH, W>&);
template <int CH, int W> LanczosTileTask<CH, W> form_base(const LanczosTileTask<CH, W>&);
template <template <int> class MP, int CH> using PlaneTaskOf = decltype(form_base(std::declval<MP<CH>>()));

// f(Form<...>): the eight row-band instantiations — the ONE ladder over them, for the launch of all planes, of one plane and (lab builds) the persistent launch
template <class F>
static void with_band_form(const ResizeLaunch& l, F&& f) {
  if (l.multi) f(Form<RowBand4wm>{});
  else if (l.p1 == 8) { if (l.rows == 16) f(Form<RowBand16w>{}); else f(Form<RowBand8w>{}); }
  else if (l.rows == 16) f(Form<RowBand16n>{});
  else if (l.rows == 8) { if (l.narrow) f(Form<RowBand8n>{}); else f(Form<RowBand8>{}); }
  else if (l.rows == 4) f(Form<RowBand4>{});
  else f(Form<RowBand2>{});
}
// f(Form<...>) for a launch of family `fam`: RESIZE_TILE, RESIZE_LZ_TILE, RESIZE_ROWPAIR or RESIZE_BAND
template <class F>
static void with_form(int fam, const ResizeLaunch& l, F&& f) {
  if (fam == RESIZE_TILE) { if (l.wpb == 8) f(Form<TileBl8>{}); else f(Form<TileBl4>{}); }
  else if (fam == RESIZE_LZ_TILE) { if (l.wpb == 8) f(Form<TileLz8>{}); else f(Form<TileLz4>{}); }
  else if (fam == RESIZE_BAND) with_band_form(l, f);
  else if (l.it == 1) f(Form<RowPair1>{});
  else if (l.it == 2) f(Form<RowPair2>{});
  else if (l.it == 3) f(Form<RowPair3>{});
  else f(Form<RowPair4>{});
}
template <class F> static void with_ch(int ch, F&& f) { with_value<1, 2, 3>(ch, f); }     // f(CH): 1, 2, else 3 interleaved channels
template <class F> static void with_ch_f32(int ch, F&& f) { with_value<3, 1>(ch, f); }    // float surfaces: packed (3), else planar (1)

// (the selection log / roctx mark carries __PRETTY_FUNCTION__: it names the task the generic entry was instantiated with)
// (grid.z = the frames of the launch: up to 32 take the small frame table, more the large one — two instantiations of the same kernel)
template <class Task>
static void launch_plane_batch(hipStream_t st, dim3 grid, uint32_t lds, const BatchArgsL& a, int k, const PlaneGeom& g) {
  if (log_level() >= 2 || trace_on()) note_kernel(__PRETTY_FUNCTION__);
  (void)hipGetLastError();
  if (grid.z <= (uint32_t)kSmallBatch) hipLaunchKernelGGL((k_plane_batch<Task, BatchArgs>), grid, dim3(Task::kThreads), lds, st, small_batch(a, grid.z), k, g);
  else hipLaunchKernelGGL((k_plane_batch<Task, BatchArgsL>), grid, dim3(Task::kThreads), lds, st, a, k, g);
}
template <template <int> class TaskCH>
static void launch_planes_mp(hipStream_t st, dim3 grid, uint32_t lds, const BatchArgsL& a, const PlaneTable& t) {
  if (log_level() >= 2 || trace_on()) note_kernel(__PRETTY_FUNCTION__);
  (void)hipGetLastError();
  if (grid.z <= (uint32_t)kSmallBatch) hipLaunchKernelGGL((k_planes_mp<TaskCH, BatchArgs>), grid, dim3(TaskCH<3>::kThreads), lds, st, small_batch(a, grid.z), t);
  else hipLaunchKernelGGL((k_planes_mp<TaskCH, BatchArgsL>), grid, dim3(TaskCH<3>::kThreads), lds, st, a, t);
}
#ifdef VPF_LAB_FORMS
// ---- the persistent form of the same launch (k_resize_common.h: k_planes_mp_persist; vpf_persist.h): the resident set of workgroups pulls
// wave items (frame, plane, wave row, column chunk) from the stream's work counters.  -> false when it does not apply (captured stream, no
// counter slot free, too few items per wave to be worth it): the caller launches the plain grid.
__device__ uint32_t g_persist_ctr[kPersistSlots * 16];  // two sets of eight per slot (vpf_persist.h)
static PersistSlotTable& persist_slots() { static PersistSlotTable t; return t; }
static bool persist_stream_idle(int dev, const void* stream) {
  int cur = -1;
  if (hipGetDevice(&cur) != hipSuccess || cur != dev) { (void)hipGetLastError(); return false; }  // (another device's stream: not asked from here)
  const hipError_t e = hipStreamQuery((hipStream_t)stream);
  if (e != hipSuccess) (void)hipGetLastError();
  return e != hipErrorNotReady;  // drained — or no longer a stream
}
static uint32_t* persist_ctr_base(int dev) {
  static std::atomic<uint32_t*> base[64];
  uint32_t* p = base[dev].load(std::memory_order_acquire);
  if (!p) {
    void* q = nullptr;
    if (hipGetSymbolAddress(&q, HIP_SYMBOL(g_persist_ctr)) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    p = static_cast<uint32_t*>(q);
    base[dev].store(p, std::memory_order_release);
  }
  return p;
}
template <template <int> class TaskCH>
static uint32_t persist_resident_groups(int dev, uint32_t lds) {  // workgroups of this kernel the whole chip holds at `lds` bytes each
  struct Seen { int dev; uint32_t lds, groups; };
  static thread_local Seen seen[4];
  static thread_local unsigned next = 0;
  for (const Seen& e : seen) if (e.groups && e.dev == dev && e.lds == lds) return e.groups;
  int per_cu = 0, cus = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(&k_planes_mp_persist<TaskCH, BatchArgs>), (int)TaskCH<3>::kThreads, lds) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || per_cu < 1 || cus < 1) { (void)hipGetLastError(); return 0; }
  const uint32_t groups = (uint32_t)per_cu * (uint32_t)cus;
  seen[next++ & 3] = Seen{dev, lds, groups};
  return groups;
}
template <template <int> class TaskCH>
static bool launch_planes_mp_persist(hipStream_t st, uint32_t lds, const BatchArgsL& a, const PlaneTable& t, uint32_t n, const uint32_t* nbx, const uint32_t* nbands, uint32_t chunk, uint32_t hops) {
  PersistArgs P{};
  uint32_t per_frame = 0;
  if (!chunk) return false;
  for (uint32_t p = 0; p < t.np; p++) { P.p0[p] = per_frame; P.nbx[p] = nbx[p]; P.nbands[p] = nbands[p]; per_frame += nbx[p] * ((nbands[p] + chunk - 1) / chunk); }
  const uint64_t total = (uint64_t)per_frame * n;
  if (!per_frame || total >= (1u << 22)) return false;
  if (st == hipStreamPerThread) return false;  // one handle, a different stream in every thread: not a key for a slot of counters
  int dev = 0;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev > 63) { (void)hipGetLastError(); return false; }
  const uint32_t resident = persist_resident_groups<TaskCH>(dev, lds), wpg = TaskCH<3>::kThreads / 64u;
  if (!resident) return false;
  if (hipStreamIsCapturing(st, &cs) != hipSuccess) { (void)hipGetLastError(); return false; }
  if (cs != hipStreamCaptureStatusNone) return false;
  uint32_t* const ctr = persist_ctr_base(dev);
  int set = 0;
  const int slot = ctr ? persist_slots().take(dev, (const void*)st, persist_stream_idle, &set) : -1;
  if (slot < 0) return false;
  P.ctr = ctr + 16 * slot + 8 * set;
  P.ctr_other = ctr + 16 * slot + 8 * (set ^ 1);
  P.per_frame = per_frame;
  P.chunk = chunk;
  P.hops = hops > 8 ? 8 : hops;
  persist_shares((uint32_t)total, P.lo);
  if (log_level() >= 2 || trace_on()) note_kernel(__PRETTY_FUNCTION__);
  (void)hipGetLastError();
  const uint32_t groups = (uint32_t)std::max<uint64_t>(8, std::min<uint64_t>(resident, (total + wpg - 1) / wpg));  // >= 8: every XCD's share has a wave that draws from it
  if (n <= (uint32_t)kSmallBatch) hipLaunchKernelGGL((k_planes_mp_persist<TaskCH, BatchArgs>), dim3(groups), dim3(TaskCH<3>::kThreads), lds, st, small_batch(a, n), t, P);
  else hipLaunchKernelGGL((k_planes_mp_persist<TaskCH, BatchArgsL>), dim3(groups), dim3(TaskCH<3>::kThreads), lds, st, a, t, P);
  return true;
}
template <template <int> class MP>
static bool launch_form_persist(Form<MP>, hipStream_t st, uint32_t lds, const BatchArgsL& a, const PlaneTable& t, uint32_t n, const uint32_t* nbx, const uint32_t* nbands, uint32_t chunk, uint32_t hops) {
  return launch_planes_mp_persist<MP>(st, lds, a, t, n, nbx, nbands, chunk, hops);
}
#endif  // VPF_LAB_FORMS
template <template <int> class MP>
static void launch_form_all(Form<MP>, hipStream_t st, dim3 grid, uint32_t lds, const BatchArgsL& a, const PlaneTable& t) { launch_planes_mp<MP>(st, grid, lds, a, t); }
template <template <int> class MP>
static void launch_form_plane(Form<MP>, hipStream_t st, dim3 grid, uint32_t lds, const BatchArgsL& a, const ResizeJob& j, const PlaneGeom& g) {
  with_ch(j.ch, [&](auto C) { launch_plane_batch<PlaneTaskOf<MP, decltype(C)::value>>(st, grid, lds, a, j.k, g); });
}

// one plane of one frame: the scalar-argument kernel entries (kernarg preload, vpf_internal.h)
static hipError_t launch_resize_single(hipStream_t st, const ResizeJob& j, const ResizeLaunch& l, const BatchArgsL& a) {
  const uint8_t* src = a.f[0].s[j.k];
  uint8_t* dst = a.f[0].d[j.k];
  const uint32_t sp = a.f[0].sp[j.k], dp = a.f[0].dp[j.k], sw = j.sw, sh = j.sh, dw = j.dw, dh = j.dh;
  const float scx = l.scx, scy = l.scy;
  const int vec_ok = l.vec_ok;
  const dim3 grid(l.gx, l.gy), block(l.threads);
  int fam = l.family;
  // 8-bit Lanczos: the matrix-core kernel (k_lanczos_mfma.hip) may decline; then the tile shape planned for this plane, or the gather form
  if (fam == RESIZE_LZ_MFMA) fam = launch_lanczos_mfma(st, 1, &j, 1, a) ? RESIZE_NONE : l.fallback;
  switch (fam) {
    case RESIZE_NONE: break;
    case RESIZE_HALF3: VPF_LAUNCH(k_resize_half3_r16, grid, block, 0, st, src, sp, dst, dp, sw, l.a0, l.a1); break;
    case RESIZE_HALF: with_ch(j.ch, [&](auto C) { VPF_LAUNCH_T(k_resize_half, (C), grid, 0, st, src, sp, dst, dp, dw, dh); }); break;
    case RESIZE_TILE:
      with_ch(j.ch, [&](auto C) { with_value<8, 4>(l.wpb, [&](auto W) {
        VPF_LAUNCH_TN(k_resize_tile, (C, W), grid, block, l.lds, st, src, sp, sw, sh, dst, dp, dw, dh, scx, scy, l.a0, l.a1, l.a2, l.a3, vec_ok); }); });
      break;
    case RESIZE_LZ_TILE:
      with_ch(j.ch, [&](auto C) { with_value<8, 4>(l.wpb, [&](auto W) {
        VPF_LAUNCH_TN(k_resize_lztile, (C, W), grid, block, l.lds, st, src, sp, sw, sh, dst, dp, dw, dh, scx, scy, l.a0, l.a1, l.a2, l.a3, vec_ok); }); });
      break;
    case RESIZE_LZ_GATHER: with_ch(j.ch, [&](auto C) { VPF_LAUNCH_T(k_resize_lanczos, (C), grid, 0, st, src, sp, sw, sh, dst, dp, dw, dh, scx, scy); }); break;
    case RESIZE_ROWPAIR:
      with_ch(j.ch, [&](auto C) { with_value<1, 2, 3, 4>(l.it, [&](auto IT) {
        VPF_LAUNCH_T(k_resize_lds, (C, IT), grid, l.lds, st, src, sp, sw, sh, dst, dp, dw, dh, scx, scy, vec_ok, l.a0); }); });
      break;
    case RESIZE_F32_TILE: {  // the float tile task has no scalar-argument entry: the small frame table with this one plane in it
      const PlaneGeom g{sw, sh, dw, dh, scx, scy, vec_ok, l.a0, l.a1, l.a2, l.a3};
      BatchArgs b;
      std::memset(&b, 0, sizeof(b));
      b.f[0].s[0] = src; b.f[0].sp[0] = sp; b.f[0].d[0] = dst; b.f[0].dp[0] = dp;
      with_ch_f32(j.ch, [&](auto C) { with_bool(l.lz, [&](auto LZ) { with_value<8, 4>(l.wpb, [&](auto W) {
        // (the generic kernel over the task: VPF_LAUNCH_TN spells K<targs>, this instantiation is k_plane_batch<TileTaskF32<targs>>)
        if (log_level() >= 2 || trace_on()) note_instantiation("k_plane_batch<TileTaskF32", C, LZ, W);
        (void)hipGetLastError();
        hipLaunchKernelGGL((k_plane_batch<TileTaskF32<decltype(C)::value, decltype(LZ)::value, decltype(W)::value>>), grid, block, l.lds, st, b, 0, g);
      }); }); });
      break;
    }
    case RESIZE_F32_GATHER:
      with_ch_f32(j.ch, [&](auto C) { with_value<VPF_INTERP_LANCZOS3, VPF_INTERP_LINEAR, VPF_INTERP_NEAREST>(l.eff, [&](auto I) {
        VPF_LAUNCH_T(k_resize_f32, (C, I), grid, 0, st, src, sp, sw, sh, dst, dp, dw, dh, scx, scy); }); });
      break;
    default:  // RESIZE_GATHER
      with_ch(j.ch, [&](auto C) { with_value<VPF_INTERP_LINEAR, VPF_INTERP_NEAREST>(l.eff, [&](auto I) {
        VPF_LAUNCH_T(k_resize, (C, I), grid, 0, st, src, sp, sw, sh, dst, dp, dw, dh, scx, scy, vec_ok); }); });
  }
  return hipGetLastError();
}

hipError_t launch_resize_planned(hipStream_t st, bool f32, int interp, int njobs, const ResizeJob* jobs, uint32_t n, const BatchArgsL& a, uint32_t call_n) {
  ResizeShape q{};
  q.f32 = f32; q.interp = interp; q.njobs = njobs; q.n = n; q.call_n = call_n;
  if (njobs >= 1 && njobs <= 3 && n <= (uint32_t)kMaxBatch)
    for (int p = 0; p < njobs; p++) {
      const int k = jobs[p].k;
      q.jobs[p] = jobs[p];
      for (uint32_t i = 0; i < n; i++) {
        q.src_bits[p] |= (uintptr_t)a.f[i].s[k] | a.f[i].sp[k];
        q.dst_bits[p] |= (uintptr_t)a.f[i].d[k] | a.f[i].dp[k];
      }
    }
  q.variant = tuning(VPF_TUNE_NV12_RGB_VARIANT); q.tile = tuning(VPF_TUNE_RESIZE_TILE); q.band = tuning(VPF_TUNE_RESIZE_BAND); q.mfma = tuning(VPF_TUNE_RESIZE_MFMA);
  const ResizePlan P = resize_plan(q);
  if (!P.ok) return hipErrorInvalidValue;
  if (P.single) return launch_resize_single(st, jobs[0], P.plane[0], a);
  auto geom = [&](int p, const ResizeLaunch& l) {
    const ResizeJob& j = jobs[p];
    return PlaneGeom{j.sw, j.sh, j.dw, j.dh, P.plane[p].scx, P.plane[p].scy, P.plane[p].vec_ok, l.a0, l.a1, l.a2, l.a3};
  };
  // ONE launch for every plane of the format
  auto launch_all = [&]() -> hipError_t {
    const ResizeLaunch& m = P.mp;
    PlaneTable t{};
    t.np = (uint32_t)njobs;
    for (int p = 0; p < njobs; p++) { t.g[p] = geom(p, m); t.k[p] = (uint32_t)jobs[p].k; t.ch[p] = (uint32_t)jobs[p].ch; t.by0[p] = P.by0[p]; }
#ifdef VPF_LAB_FORMS
    // the persistent form for the band kernels (lab builds, VPF_TUNE_RESIZE_BAND | 0x10000): chunks of bands instead of a grid
    if (m.family == RESIZE_BAND && ((q.band >> 16) & 1)) {
      // chunks of `chunk` bands (knob bits 8..15; default 2), one counter per XCD; | 0x40000: a wave whose counter has run dry visits the other seven
      uint32_t nbx[3] = {0, 0, 0}, nbands[3] = {0, 0, 0};
      for (int p = 0; p < njobs; p++) {
        const uint32_t wcols = 64u * band_px(jobs[p].ch, m.p1);
        nbx[p] = (jobs[p].dw + wcols - 1) / wcols; nbands[p] = (jobs[p].dh + m.rows - 1) / m.rows;
      }
      const uint32_t chunk = ((q.band >> 8) & 0xff) ? (uint32_t)((q.band >> 8) & 0xff) : 2u;
      const uint32_t hops = ((q.band >> 19) & 1) ? 0u : ((q.band >> 18) & 1) ? 8u : 1u;  // | 0x80000 (measurement): no counters, a wave strides through its XCD's share
      bool done = false;
      with_band_form(m, [&](auto form) { done = launch_form_persist(form, st, m.lds, a, t, n, nbx, nbands, chunk, hops); });
      if (done) return hipGetLastError();
    }
#endif  // VPF_LAB_FORMS
    with_form(m.family, m, [&](auto form) { launch_form_all(form, st, dim3(m.gx, m.gy, m.gz), m.lds, a, t); });
    return hipGetLastError();
  };
  // 8-bit Lanczos: the order resize_plan names.  The matrix-core launcher (k_lanczos_mfma.hip) declines at run time what its windows, its table
  // arena or the device do not allow; a plane it declined takes the fallback planned for it.
  if (P.lz_tile_all_first) return launch_all();
  if (P.lz_mfma_all && launch_lanczos_mfma(st, njobs, jobs, n, a)) return hipGetLastError();
  bool declined[3] = {false, false, false}, all_declined = true;
  for (int p = 0; p < njobs; p++) {
    if (P.plane[p].family == RESIZE_LZ_MFMA) declined[p] = !launch_lanczos_mfma(st, 1, &jobs[p], n, a);
    all_declined = all_declined && declined[p];
  }
  if ((P.lz_tile_all_fallback && all_declined) || P.all) return launch_all();
  // ---- otherwise: one launch per plane over all frames
  for (int p = 0; p < njobs; p++) {
    const ResizeJob& j = jobs[p];
    const ResizeLaunch& l = P.plane[p];
    const int fam = declined[p] ? l.fallback : l.family;
    const PlaneGeom g = geom(p, l);
    const dim3 grid(l.gx, l.gy, l.gz);
    switch (fam) {
      case RESIZE_LZ_MFMA: break;  // launched above
      case RESIZE_F32_TILE:
        with_ch_f32(j.ch, [&](auto C) { with_bool(l.lz, [&](auto LZ) { with_value<8, 4>(l.wpb, [&](auto W) {
          launch_plane_batch<TileTaskF32<decltype(C)::value, decltype(LZ)::value, decltype(W)::value>>(st, grid, l.lds, a, j.k, g); }); }); });
        break;
      case RESIZE_F32_GATHER:
        with_ch_f32(j.ch, [&](auto C) { with_value<VPF_INTERP_LANCZOS3, VPF_INTERP_LINEAR, VPF_INTERP_NEAREST>(l.eff, [&](auto I) {
          launch_plane_batch<FloatGatherTask<decltype(C)::value, decltype(I)::value>>(st, grid, 0, a, j.k, g); }); });
        break;
      case RESIZE_HALF3: launch_plane_batch<Half3R16Task>(st, grid, 0, a, j.k, g); break;
      case RESIZE_HALF: with_ch(j.ch, [&](auto C) { launch_plane_batch<HalfTask<decltype(C)::value>>(st, grid, 0, a, j.k, g); }); break;
      case RESIZE_LZ_GATHER: with_ch(j.ch, [&](auto C) { launch_plane_batch<LanczosGatherTask<decltype(C)::value>>(st, grid, 0, a, j.k, g); }); break;
      case RESIZE_GATHER:
        with_ch(j.ch, [&](auto C) { with_value<VPF_INTERP_LINEAR, VPF_INTERP_NEAREST>(l.eff, [&](auto I) {
          launch_plane_batch<GatherTask<decltype(C)::value, decltype(I)::value>>(st, grid, 0, a, j.k, g); }); });
        break;
      default:  // RESIZE_TILE, RESIZE_LZ_TILE, RESIZE_ROWPAIR, RESIZE_BAND
        with_form(fam, l, [&](auto form) { launch_form_plane(form, st, grid, l.lds, a, j, g); });
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace vpf
VPF_WAVE_TIMES_EXPORT(vpf_lab_wave_times_resize)
