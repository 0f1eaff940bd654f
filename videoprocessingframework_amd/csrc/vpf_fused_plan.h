// vpf_fused_plan.h — the policy of the fused convert + resize launch (k_convert_resize.hip: vpf_convert_resize, vpf_convert_resize_batch,
// vpf_convert_resize_tensor_batch) as ONE pure function: which kernel family, which band height, which frame table, the grid, the dynamic LDS and
// the family's trailing scalar arguments.  No HIP in here: the launcher includes it and only dispatches on the result, and
// tests/test_fused_plan_cpu.py compiles the same header with g++ (tests/c/fused_plan_capi.cpp).  The measured reasons for every limit stand in
// the comments next to it.
#pragma once
#include <stdint.h>

#include "vpf_classes.h"
#include "vpf_hip.h"
#include "vpf_plan_bounds.h"

namespace vpf {

constexpr uint32_t kFusedRowBytes = 2048;  // cap; the launch sizes the strips for its own scale factor (dyn_strip)
constexpr int kStripRows = 8;              // source rows a wave's strip can hold (lab builds: k_convert_strip)

enum FusedFamily : int {
  FUSED_REFUSED = 0,  // hipErrorInvalidValue
  FUSED_HALF,         // k_convert_half(_one)         exact 2x
  FUSED_STRIP_WG,     // k_convert_strip_wg<R>        the workgroup's strip
  FUSED_BAND,         // k_convert_resize_band<IT, 4> the per-tap kernel as a row band
  FUSED_LDS,          // k_convert_resize_lds(_one)<IT>  per-tap, source rows through LDS
  FUSED_GATHER,       // k_convert_resize             per-tap from global memory
  FUSED_STRIP_WAVE,   // k_convert_strip<R>           lab builds only (VPF_LAB_FORMS): the per-wave strips of rounds 2-4
};
enum FusedTable : int {
  FUSED_ONE = 0,  // the single-frame entry with scalar arguments (kernarg preload, vpf_internal.h): 8-bit destinations of k_convert_half and k_convert_resize_lds
  FUSED_SMALL,    // up to kSmallBatch frames: BatchArgs / BatchArgsTE<kSmallBatch>
  FUSED_LARGE,    // BatchArgsL / BatchArgsTE<kMaxBatch>
};

// What the policy looks at.  `src_bits` / `dst_bits`: pointer | pitch OR-ed over the planes the class has (FC_NV12, FC_P16: 2, FC_YUV420: 3;
// FC_PLANAR, FC_TENSOR: 3, else 1) and over the n frames — every alignment test below asks whether ALL of them are multiples of some power of two.
struct FusedShape {
  int src_fc, dst_fc;
  bool has_epilogue;  // tensor destinations: the caller passed a TensorEpi
  uint32_t dtype;     // its VPF_TENSOR_* (tensor destinations only)
  uint32_t sw, sh, dw, dh, n;
  int variant;        // tuning(VPF_TUNE_NV12_RGB_VARIANT), read once by the caller
  uint64_t src_bits, dst_bits;
};
struct FusedPlan {
  int family;                // FusedFamily
  int r;                     // FUSED_STRIP_WG: R = 2 / 4 / 8 / 16 (FUSED_STRIP_WAVE: 2 / 4 / 8); FUSED_BAND, FUSED_LDS: IT = 1 / 2; else 0
  int table;                 // FusedTable
  uint32_t gx, gy, gz;       // the grid, of 256-lane workgroups
  uint32_t lds;              // the kernel's own dynamic LDS, before the staging area of an FC_TENSOR_NHWC launch (nhwc_stage_plan)
  uint32_t stage_npx;        // pixels per lane, for nhwc_stage_plan: 8 for k_convert_half, else 4
  int vec_ok;                // the destination takes the vector stores
  float scx, scy;
  uint32_t chunks, tasks;    // FUSED_HALF
  uint32_t rowq;             // strips and per-tap LDS: 16-B units per strip row (FUSED_STRIP_WAVE: | strip rows per wave << 16)
};

inline FusedPlan fused_plan(const FusedShape& q) {
  const int src_fc = q.src_fc, dst_fc = q.dst_fc, variant = q.variant;
  const uint32_t sw = q.sw, sh = q.sh, dw = q.dw, dh = q.dh, n = q.n;
  FusedPlan p{};
  // FC_TENSOR: the same frame table with the epilogue behind it (BatchArgsTE); entries up to the next multiple of 8 are defined (vpf_abi.hip)
  // FC_TENSOR_NHWC: the same launches with the other destination class: the family is picked exactly as for FC_TENSOR, only the
  // destination alignment test differs — one plane, whose vector stores are 16-B ones whatever the dtype
  const bool nhwc = dst_fc == FC_TENSOR_NHWC, tens = dst_fc == FC_TENSOR || nhwc;
  if (tens && (!q.has_epilogue || n > (uint32_t)kMaxBatch)) return p;
  if (src_fc == FC_P16 ? !tens : src_fc != FC_NV12 && src_fc != FC_YUV420) return p;  // FC_P16: into tensors only; no other source class
  const float scx = (float)sw / (float)dw, scy = (float)sh / (float)dh;
  p.scx = scx; p.scy = scy;
  // up to 32 frames travel in the small frame table, more in the large one: two instantiations of every batch kernel (vpf_internal.h)
  p.table = n <= (uint32_t)kSmallBatch ? FUSED_SMALL : FUSED_LARGE;
  p.stage_npx = 4;
  auto all_aligned = [](uint64_t bits, uint32_t mask) { return (bits & mask) == 0; };
  // destination alignment the vector stores need: 4 px x element size per lane and plane (1-B elements: the 8-bit classes)
  const uint32_t dmask = tens ? vpf_tensor_dmask(nhwc, q.dtype == VPF_TENSOR_F32) : 3u;
  p.vec_ok = all_aligned(q.dst_bits, dmask);
  // strip bytes a wave of the per-tap LDS kernels needs per source row (0 under variant 9, the forced generic form, and for an unaligned
  // source).  The launcher's lds_strip_bytes looked at frame 0's luma plane only; `rowb` is consumed under lds_ok alone —
  // the LDS size and `rowq` of the band and per-tap LDS families, both picked only where lds_ok holds — and lds_ok asks every plane of every
  // frame for the same 16 B, frame 0's luma plane among them.  So the alignment term of lds_strip_bytes is part of src_bits & 15.
  const uint32_t rowb = variant == 9 ? 0u : vpf_bound_strip_bytes(1, sw, dw, kFusedRowBytes, 256);
  const bool lds_ok = rowb != 0 && all_aligned(q.src_bits, 15u);
  auto half = [&] {
    p.family = FUSED_HALF;
    p.chunks = (sw + 1023) / 1024; p.tasks = p.chunks * dh;
    p.gx = (p.tasks + 3) / 4; p.gy = n; p.gz = 1;
    p.stage_npx = 8;
    if (n == 1 && !tens) p.table = FUSED_ONE;
    return p;
  };
  auto gather = [&] {
    p.family = FUSED_GATHER;
    p.gx = ((dw + 3) / 4 + 63) / 64; p.gy = (dh + 3) / 4; p.gz = n;
    return p;
  };
  // 16-bit sources (FC_P16: P10 / P12, into FC_TENSOR only).  Policy: exact 2x -> k_convert_half; the workgroup strip under the wconv rule of
  // the 8-bit sources below; everything else -> the gather form.  The per-tap LDS kernels stage raw bytes and have no 16-bit instantiation
  // (DESIGN 4.10, 8).  VPF_TUNE_NV12_RGB_VARIANT = 9 / 40 / 49 keep the gather form.
  const bool p16_general = variant == 9 || variant == 40 || variant == 49;
  const bool p16_a16 = src_fc == FC_P16 && all_aligned(q.src_bits, 15u);  // 16-B aligned source planes and pitches: what the aligned 16-B loads of the half and strip kernels need
  if (src_fc == FC_P16 && sw == 2 * dw && sh == 2 * dh && sw % 16 == 0 && p16_a16 && !p16_general && all_aligned(q.dst_bits, 15u)) return half();
  // exact 2x from NV12: the quad-structured kernel (no taps, no gathers); tuning 40 / 9 keep the general kernels
  // (packed rows leave as 16-B stores: 3 * dw must be a multiple of 16)
  if ((src_fc == FC_NV12 || src_fc == FC_YUV420) && sw == 2 * dw && sh == 2 * dh && sw % (dst_fc == FC_PLANAR || tens ? 16 : 32) == 0 && lds_ok && variant != 40 &&
      all_aligned(q.dst_bits, dst_fc == FC_PLANAR ? 7u : 15u))  // (FC_TENSOR: 16-B stores whatever the dtype)
    return half();
  // general factors: convert the window once into an LDS RGB strip, blend from bytes (k_convert_strip); odd integer factors on either
  // axis keep the kernels below (their zero-weight shortcuts skip whole rows / taps)
  {
    const bool odd_x = sw % dw == 0 && ((sw / dw) & 1), odd_y = sh % dh == 0 && ((sh / dh) & 1);
    const bool ok8 = (src_fc == FC_NV12 || src_fc == FC_YUV420 || (src_fc == FC_P16 && p16_a16)) && sw % 8 == 0 && !odd_x && !odd_y && variant != 40 &&
                     variant != 9 && variant != 49 && sw < (1u << 22) && sh < (1u << 22) && all_aligned(q.src_bits, 7u);
    if (ok8) {
#ifdef VPF_LAB_FORMS  // the per-wave strips of rounds 2-4 (k_convert_strip): variant 47, and where the workgroup strips do not apply
      const uint32_t rowbytes = vpf_bound_fused_rowbytes(scx);  // a wave's source span + alignment + tap-window slack (vpf_plan_bounds.h)
      int r = 0;
      if (vpf_bound_fused_rows_fit(8, scy, kStripRows)) r = 8;  // rows a wave's R destination rows can touch: <= (R - 1) scy + 3 (+ fp32 slack)
      else if (vpf_bound_fused_rows_fit(4, scy, kStripRows)) r = 4;
      else if (vpf_bound_fused_rows_fit(2, scy, kStripRows)) r = 2;
      if (dh < 64) r = r ? 2 : 0;  // short pictures: more, smaller tasks
      if (r == 8 && (uint64_t)((dw + 255) / 256) * ((dh + 31) / 32) * n < 2048) r = 4;  // keep the chip covered
      // strip rows per wave: what the bands of this shape really touch (a walk with the kernel's tap arithmetic, vpf_plan_bounds.h), not
      // the kStripRows the band height was chosen against — 1080p -> 720p: 6 rows, five workgroups per CU instead of four
      static thread_local struct { int r; uint32_t sh, dh, rows; } seen = {0, 0, 0, 0};
      if (r && !(seen.r == r && seen.sh == sh && seen.dh == dh)) { seen.r = r; seen.sh = sh; seen.dh = dh; seen.rows = vpf_band_rows_exact(r, sh, dh, scy); }
      const uint32_t srows = r ? (seen.rows < (uint32_t)kStripRows ? seen.rows : (uint32_t)kStripRows) : (uint32_t)kStripRows;
      const uint32_t lds1 = 4u * srows * rowbytes;
      // conversions per destination pixel: scx x ((r - 1) scy + 2) / r source pixels against the four taps of the per-tap kernel —
      // measured break-even near 2x (4K -> 1600x900, 2.4x: 9.5 us here vs 5.2 us per-tap; 1080p -> 720p: 2.36 vs 3.21; 1080p -> 4K: 15.0 vs 23.6)
      const double conv_per_px = r ? (double)scx * ((r - 1) * (double)scy + 2.0) / r : 1e9;
#endif  // VPF_LAB_FORMS
      // Round 5: the strip shared by the workgroup (k_convert_strip_wg: the source window of 4 R destination rows converted once, dealt
      // out over all 256 lanes).  Band height: the largest of 16 (up-scales) / 8 / 4 / 2 whose strip leaves four workgroups per CU
      // (<= 40 KiB of the CU's 160: round 6's four-byte pixels make 1080p -> 720p at R = 4 a 39.5-KiB strip) and whose launch still covers the chip.  (Lab builds: VPF_TUNE_NV12_RGB_VARIANT = 47 keeps the per-wave strips.)
#ifdef VPF_LAB_FORMS
      if (variant != 47)
#endif
      {
        static thread_local struct { uint32_t sh, dh, rows[4]; } wseen = {0, 0, {0, 0, 0, 0}};
        if (!(wseen.sh == sh && wseen.dh == dh)) {
          wseen.sh = sh; wseen.dh = dh;
          for (int k = 0; k < 4; k++) wseen.rows[k] = vpf_band_rows_exact(4 * (2 << k), sh, dh, scy);  // the workgroup's 4 R rows: R = 2, 4, 8, 16
        }
        int rw = 0;
        uint32_t wrows = 0;
        const uint32_t rowbytes4 = vpf_bound_fused_rowbytes4(scx);  // the workgroup's strip holds four bytes per pixel (R G B x)
        for (int k = 3; k >= 0; k--) {
          const int cand = 2 << k;
          if (cand == 16 && scy > 1.0f) continue;
          if ((uint64_t)wseen.rows[k] * rowbytes4 > 40u * 1024u) continue;
          if (cand > 2 && (uint64_t)((dw + 255) / 256) * ((dh + 4 * cand - 1) / (4 * cand)) * n < (cand >= 8 ? 2048u : 512u)) continue;  // keep the chip covered
          rw = cand; wrows = wseen.rows[k];
          break;
        }
        // source pixels converted per destination pixel: rows of the strip x its width / (4 R x 256); the per-tap kernel converts four
        auto wconv_of = [&](int cand, uint32_t rows) { return cand ? (double)rows * ((double)scx * 255.0 + 18.0) / (4.0 * cand * 256.0) : 1e9; };
        const double wmax = variant == 48 ? 8.0 : 3.0;
        // Second pass (round 6: the four-byte pixels pushed factors of 1.55-1.9 and small single frames out of the first): 4- or 2-row bands
        // with a strip of up to 53 KiB (three workgroups per CU) however few workgroups the launch has — the shapes the per-wave strips of
        // rounds 2-4 (lab builds: k_convert_strip) used to take, with the rows neighbouring bands share converted once.
        if (!rw || wconv_of(rw, wrows) > wmax) {
          rw = 0;
          for (int k = 1; k >= 0; k--) {
            const int cand = 2 << k;
            if ((uint64_t)wseen.rows[k] * rowbytes4 > 53u * 1024u || (dh < 64 && cand > 2)) continue;
            if (wconv_of(cand, wseen.rows[k]) <= wmax) { rw = cand; wrows = wseen.rows[k]; break; }
          }
        }
        const double wconv = wconv_of(rw, wrows);
        if (rw && wconv <= wmax) {
          p.family = FUSED_STRIP_WG; p.r = rw;
          p.lds = wrows * rowbytes4;
          p.gx = (dw + 255) / 256; p.gy = (dh + 4 * rw - 1) / (4 * rw); p.gz = n;
          p.rowq = rowbytes4 / 16;
          return p;
        }
      }
#ifdef VPF_LAB_FORMS
      if (r && lds1 <= 64u * 1024u && conv_per_px <= 3.0 && !tens) {  // (8-bit destinations only)
        p.family = FUSED_STRIP_WAVE; p.r = r;
        p.lds = lds1;
        p.gx = (dw + 255) / 256; p.gy = (dh + 4 * r - 1) / (4 * r); p.gz = n;
        p.rowq = (rowbytes / 16) | (srows << 16);
        return p;
      }
#endif  // VPF_LAB_FORMS
    }
  }
  if (src_fc == FC_P16) return gather();  // everything else from 16-bit sources: the gather form
  p.lds = 4 * (src_fc == FC_NV12 ? 4 : 6) * rowb;
  p.rowq = rowb / 16;
  p.r = rowb <= 1024 ? 1 : 2;
  // factors beyond ~2x on a launch that covers the chip with four rows per wave: the per-tap kernel as a row band (k_convert_resize_band);
  // odd integer factors keep the row-at-a-time kernel below and its zero-weight shortcuts.  VPF_TUNE_NV12_RGB_VARIANT = 40 / 9 keep it too.
  {
    const bool odd_x = sw % dw == 0 && ((sw / dw) & 1), odd_y = sh % dh == 0 && ((sh / dh) & 1);
    if (lds_ok && !odd_x && !odd_y && variant != 40 && variant != 9 && sw < (1u << 22) && sh < (1u << 22) &&
        ((uint64_t)((dw + 255) / 256) * ((dh + 15) / 16) * n >= 2048u || variant == 49)) {  // 49: whatever the launch size (tests, A/B runs)
      p.family = FUSED_BAND;
      p.gx = (dw + 255) / 256; p.gy = (dh + 15) / 16; p.gz = n;
      return p;
    }
  }
  if (!lds_ok) {
    p.lds = 0; p.rowq = 0; p.r = 0;
    return gather();
  }
  // FC_TENSOR: the frame-table kernels for one frame too (no scalar-argument entry: the epilogue rides behind the table)
  p.family = FUSED_LDS;
  p.gx = ((dw + 3) / 4 + 63) / 64; p.gy = (dh + 3) / 4; p.gz = n;
  if (n == 1 && !tens) p.table = FUSED_ONE;
  return p;
}

}  // namespace vpf
