// vpf_resize_plan.h — the policy of the plain resize launches (k_resize.hip: vpf_resize, vpf_resize_batch) as ONE pure function: which entry (the
// scalar-argument single-plane kernels or the frame-table kernels), whether one launch takes every plane of the format, per launch the kernel
// family, its template selectors, the grid, the dynamic LDS and the PlaneGeom scalars — and for 8-bit Lanczos the ORDER in which the matrix-core
// launcher (k_lanczos_mfma.hip, which may decline at run time) and the kernels here are tried.  No HIP in here: launch_resize_planned includes
// it and only dispatches on the result, and tests/test_resize_plan_cpu.py compiles the same header with g++ (tests/c/resize_plan_capi.cpp).
// The measured reasons for every limit stand in the comments next to it.
#pragma once
#include <stdint.h>

#include <algorithm>

#include "vpf_classes.h"
#include "vpf_hip.h"
#include "vpf_plan_bounds.h"

namespace vpf {

// Kernel families; within a filter all are bit-identical to one another (the header of k_resize.hip describes them)
enum ResizeFamily : int {
  RESIZE_NONE = 0,
  RESIZE_GATHER,      // GatherTask<CH, eff> / k_resize: eff = NEAREST or LINEAR, any size / alignment
  RESIZE_ROWPAIR,     // RowPairTask<CH, it> / k_resize_lds
  RESIZE_BAND,        // RowBandTask<CH, rows, it, p1, multi>
  RESIZE_TILE,        // TileTask<CH, wpb> / k_resize_tile
  RESIZE_HALF,        // HalfTask<CH> / k_resize_half
  RESIZE_HALF3,       // Half3R16Task / k_resize_half3_r16
  RESIZE_LZ_MFMA,     // launch_lanczos_mfma first; where it declines, `fallback` (RESIZE_LZ_TILE or RESIZE_LZ_GATHER) with the shape planned here
  RESIZE_LZ_TILE,     // LanczosTileTask<CH, wpb> / k_resize_lztile
  RESIZE_LZ_GATHER,   // LanczosGatherTask<CH> / k_resize_lanczos
  RESIZE_F32_TILE,    // TileTaskF32<CH, lz, wpb>
  RESIZE_F32_GATHER,  // FloatGatherTask<CH, eff> / k_resize_f32
};

// What the policy looks at.  `src_bits[p]` / `dst_bits[p]`: pointer | pitch of plane jobs[p].k OR-ed over the n frames — every alignment test
// below asks whether ALL frames are multiples of 4, 8 or 16.  The four knobs are read once by the caller.
struct ResizeShape {
  bool f32;
  int interp, njobs;
  uint32_t n;       // frames of this dispatch
  uint32_t call_n;  // frames of the whole C-ABI call (vpf_resize_batch cuts a long one into dispatches): the entry rule looks at it
  ResizeJob jobs[3];
  uint64_t src_bits[3], dst_bits[3];
  int variant, tile, band, mfma;  // tuning(VPF_TUNE_NV12_RGB_VARIANT / _RESIZE_TILE / _RESIZE_BAND / _RESIZE_MFMA)
};
// One launch: of one plane over all frames, or (ResizePlan::mp) of every plane.
struct ResizeLaunch {
  int family, fallback;  // ResizeFamily; fallback: of RESIZE_LZ_MFMA only
  int eff;               // the effective filter after the odd-integer rule
  int it;                // RESIZE_ROWPAIR: 1-KiB staging passes per strip, 1 .. 4; RESIZE_BAND: 1 (the narrow-strip instantiations) or 2
  int rows, p1;          // RESIZE_BAND: destination rows per band 2 / 4 / 8 / 16, pixels per lane on 1-channel planes 4 / 8
  bool narrow, multi;    // RESIZE_BAND: strips of at most 1 KiB; the march form (several bands per wave, a2 of them)
  int wpb;               // tiles: waves per workgroup, 4 or 8
  bool lz;               // RESIZE_F32_TILE: Lanczos-3 (else bilinear)
  uint32_t gx, gy, gz, threads, lds;
  float scx, scy;        // the PlaneGeom scalars
  int vec_ok;
  uint32_t a0, a1, a2, a3;
};
struct ResizePlan {
  bool ok;      // false: refused (hipErrorInvalidValue)
  bool single;  // the scalar-argument single-plane entries (kernarg preload, vpf_internal.h); else the frame-table kernels
  bool all;     // ONE launch `mp` takes every plane: RESIZE_TILE, RESIZE_ROWPAIR or RESIZE_BAND; plane p's workgroup rows start at by0[p]
  // 8-bit Lanczos over several planes, in this order: `mp` (one RESIZE_LZ_TILE launch for all planes) when lz_tile_all_first; one matrix-core
  // launch for all planes when lz_mfma_all; the matrix-core launch plane by plane (plane[p].family == RESIZE_LZ_MFMA); `mp` when
  // lz_tile_all_fallback and EVERY plane's matrix-core launch declined; else each declined plane's own fallback
  bool lz_tile_all_first, lz_mfma_all, lz_tile_all_fallback;
  ResizeLaunch mp;
  uint32_t by0[3];
  ResizeLaunch plane[3];  // per plane: the launch it takes on its own, and always the PlaneGeom scalars scx, scy, vec_ok of its entry in `mp`
};

// Shape of a tiled launch: destination rows per tile (ty) and waves per workgroup (wpb).  A taller tile computes fewer horizontal dots per
// destination pixel ((ty - 1) scy + taps + 2 source rows for ty destination rows) but there are fewer of them to fill the chip with.
// Rule read off rocprofv3 kernel durations over (ty, wpb) for six size pairs (profiles/r02_tile_shape_sweep.txt): 8 waves per workgroup
// always (each wave walks fewer source rows one after the other), and the TALLEST tile that fits LDS and still leaves >= ~900 workgroups
// (about one full round of the chip at 4 workgroups per CU) — e.g. 1080p -> 720p: ty 16 (900 workgroups, 7.5 us; ty 32: 7.7, ty 8: 9.7),
// 720p -> 1080p: ty 32 (7.2 us; ty 64: 9.4), 1080p -> 4K: ty 64 (15.5 us; ty 32: 18.9), batches: the tallest that fits.
// VPF_TUNE_RESIZE_TILE (`forced`) overrides the choice for such sweeps (ty | wpb << 8) — every shape writes the same pixels.
struct TileShape { bool ok; uint32_t ty, nr, lds, rowq, lshift; int wpb; };
inline TileShape plan_tile(int forced, bool lz, int np, const ResizeJob* jobs, uint32_t frames, int elem = 1 /* bytes per sample: 1, or 4 for float surfaces */) {
  TileShape best{false, 0, 0, 0, 0, 0, 4};
  int ch_max = 0;
  uint32_t rowq = 0;  // 16-B units a tile row can span (+ alignment slack), the widest plane decides
  float scy = 0.f;
  for (int p = 0; p < np; p++) {
    const float sx = (float)jobs[p].sw / (float)jobs[p].dw, sy = (float)jobs[p].sh / (float)jobs[p].dh;
    ch_max = jobs[p].ch > ch_max ? jobs[p].ch : ch_max;
    const uint32_t q = vpf_bound_tile_rowq(sx, lz ? 6 : 2, jobs[p].ch, elem);  // (8-bit Lanczos: + pad unit + right margin; vpf_plan_bounds.h)
    rowq = q > rowq ? q : rowq;
    scy = sy > scy ? sy : scy;
  }
  if (rowq > kLzStripQ * (uint32_t)elem || scy > 48.0f) return best;
  uint32_t lshift = 0;
  while ((1u << lshift) < rowq) lshift++;
  uint32_t best_wgs = 0;
  for (int wpb = forced ? 4 : 8; wpb <= 8; wpb += 4)
    for (uint32_t ty = forced ? 4 : 8; ty <= 64; ty += 4) {
      if (forced && ((uint32_t)(forced & 0xff) != ty || (forced >> 8) != wpb)) continue;
      const uint32_t nr = vpf_bound_tile_rows(ty, scy, lz ? 6 : 2);
      const uint32_t lds = nr * rowq * 16 + nr * ch_max * 64 * 4 + ty * 8 * 4 + (lz ? (elem == 4 ? 7 : 4) * 64 * 4 : 0);  // RAW | H | WY | WX (Lanczos)
      if (lds > 64u * 1024u) continue;
      const uint32_t srows = (64u * wpb) >> lshift;  // source rows staged per pass
      if (!srows || (elem == 1 && (nr + srows - 1) / srows > (uint32_t)kTileStagePasses)) continue;  // (the float task stages in rounds)
      double wgs = 0;
      for (int p = 0; p < np; p++) wgs += (double)((jobs[p].dw + 63) / 64) * ((jobs[p].dh + ty - 1) / ty);
      wgs *= frames;
      const uint32_t w = wgs > 4e9 ? 0xffffffffu : (uint32_t)wgs;
      // candidates come in order of growing ty: take a taller tile while it still leaves >= 900 workgroups; below that, the most workgroups win
      if (!best.ok || w >= 900u || w > best_wgs) { best = TileShape{true, ty, nr, lds, rowq, lshift, wpb}; best_wgs = w; }
    }
  return best;
}

// ONE plane of ONE frame per dispatch (what an unmodified PySurfaceResizer.Execute loop issues): the matrix-core Lanczos kernel's waves are
// few and long — operand tables, a ring to fill, two passes — and a lone launch of them is one latency chain of 5-6 us whatever the picture;
// the tile kernel's waves are short and many, so a small single frame leaves it sooner although its throughput is 2.5x lower.  The tile
// kernel's time grows with the DESTINATION (taps per output sample), the matrix-core kernel's with the source: over 63 measured shapes
// (tools/lanczos_single_sweep.py, profiles/r04_lanczos_single_sweep.txt: RGB 1080p -> 720p 6.9 against 8.9 us, Y 4.7 against 6.9) the rule
// "source bytes / 2 + 3 x destination bytes below 25.5 MB (3 channels) / 14 MB (1 channel)" picks the faster kernel but for 1 us summed over
// all of them.  Same bytes either way (both kernels are the integer definition of the filter).  VPF_TUNE_RESIZE_MFMA | 0x40000, or a forced
// launch shape: always the matrix-core kernel.
inline bool lanczos_single_prefers_tile(int mfma_knob, int ch, uint32_t sw, uint32_t sh, uint32_t dw, uint32_t dh) {
  if (mfma_knob & 0xfffff) return false;
  const uint64_t src_b = (uint64_t)sw * sh * (uint32_t)ch, dst_b = (uint64_t)dw * dh * (uint32_t)ch;
  return src_b + 6u * dst_b <= (ch == 1 ? 28000000ull : ch == 2 ? 40000000ull : 51000000ull);
}

// Destination rows per wave for a row-pair launch (RowBandTask) and the strips per wave its LDS is sized for: the largest of 16 / 8 / 4 / 2
// whose bands fit the strip slots (8; 16 when a strip is at most 1 KiB = one staging pass, the 1- and 2-channel planes and the up-scales)
// and 64 KB of LDS (`rb` bytes per strip, at most two 1-KiB staging passes) while the launch keeps at least kBandMinGroups workgroups (a
// single small frame stays at one row per wave: it needs the parallelism more than the shared work).  Vertical factors above 2 skip
// source rows (a contiguous band would read rows nobody blends) and odd integer factors on both axes move bytes (RowPairTask's
// centre-sample shortcut): both keep one row per wave.  VPF_TUNE_RESIZE_BAND (`knob`) forces a value where it applies.
constexpr uint32_t kBandMinGroups = 2048;
struct BandShape { int rows; uint32_t slots; bool narrow; uint32_t rb; };  // rb: strip bytes of the chosen form (16-row bands of packed RGB: four bytes per pixel)
inline uint32_t band_slots(int r, float scy) { return vpf_bound_band_slots(r, scy); }  // (vpf_plan_bounds.h: checked on the CPU against the tap arithmetic)
// The strips a launch ALLOCATES: the rows its bands really touch (vpf_band_rows_exact: a walk over the bands with make_tap's arithmetic),
// never more than the closed-form bound that chose the band height.  1080p -> 720p with 4-row bands: 6 strips instead of 8, five
// workgroups per CU instead of four.  The last shapes are remembered per thread (a launch per frame would walk dh / r taps every time).
inline uint32_t band_slots_exact(int r, int njobs, const ResizeJob* jobs, uint32_t bound) {
  struct Seen { int r; uint32_t sh, dh, rows; };
  static thread_local Seen seen[8];
  static thread_local unsigned next = 0;
  uint32_t most = 1;
  for (int p = 0; p < njobs; p++) {
    const ResizeJob& j = jobs[p];
    uint32_t rows = 0;
    for (const Seen& e : seen)
      if (e.r == r && e.sh == j.sh && e.dh == j.dh && e.rows) rows = e.rows;
    if (!rows) {
      rows = vpf_band_rows_exact(r, j.sh, j.dh, (float)j.sh / (float)j.dh);
      seen[next++ & 7] = Seen{r, j.sh, j.dh, rows};
    }
    most = rows > most ? rows : most;
  }
  return most < bound ? most : bound;
}
// pixels per lane for the 1-channel planes of a band launch: 8 (512 columns per wave) when such chunks fill every 1-channel row to >= 80 %
// (1280 px: 3 chunks, 83 %; the 640-px chroma planes of a 720p YUV420 frame: 2 chunks, 62 % -> 4)
inline int band_p1(int knob, int njobs, const ResizeJob* jobs) {
  bool any = false;
  const bool force8 = (knob >> 17) & 1;  // | 0x20000: 8 pixels per lane on 1-channel planes however well 512-column chunks fill them (measurement knob)
  for (int p = 0; p < njobs; p++) {
    if (jobs[p].ch != 1) continue;
    any = true;
    if (!force8 && (double)jobs[p].dw < 0.8 * 512.0 * ((jobs[p].dw + 511) / 512)) return 4;
  }
  return any ? 8 : 4;
}
// strip bytes of the widest plane for a band launch (RowBandTask: 64 * band_px(ch, p1) columns per wave); 0 when some plane has no LDS path:
// under variant 9 (the forced generic form) or when some frame's source rows are not 16-B aligned (`src_bits` of the planes in `jobs`)
inline uint32_t band_strip_bytes(int variant, int njobs, const ResizeJob* jobs, const uint64_t* src_bits, int p1) {
  uint32_t rbmax = 0;
  for (int p = 0; p < njobs; p++) {
    const ResizeJob& j = jobs[p];
    const uint32_t rb = (src_bits[p] & 15) || variant == 9 ? 0 : vpf_bound_strip_bytes(j.ch, j.sw, j.dw, kResizeRowBytes, 64u * band_px(j.ch, p1));
    if (!rb) return 0;
    rbmax = rb > rbmax ? rb : rbmax;
  }
  return rbmax;
}
inline BandShape band_rows(int knob, int njobs, const ResizeJob* jobs, uint32_t rb, uint32_t n, int p1 = 4) {
  const int forced = knob & 0xff;  // (bits 8..: bands per wave of the march form, plan_band)
  if (forced == 1 || rb == 0 || rb > 2048) return {1, 0, false, rb};
  const uint32_t rb_packed = rb;
  float scy = 0.f;
  for (int p = 0; p < njobs; p++) {
    const ResizeJob& j = jobs[p];
    if (j.sw % j.dw == 0 && j.sh % j.dh == 0 && ((j.sw / j.dw) & 1) && ((j.sh / j.dh) & 1)) return {1, 0, false, rb};
    const float s = (float)j.sh / (float)j.dh;
    scy = s > scy ? s : scy;
  }
  if (scy > 2.0f) return {1, 0, false, rb};
  for (int r = 16; r >= 2; r >>= 1) {
    if (forced && forced != r) continue;
    rb = rb_packed;
    if (r == 16)  // RowBandTask<3, 16, 1>::kPx4: its strips hold packed RGB four bytes per pixel
      for (int p = 0; p < njobs; p++)
        if (jobs[p].ch == 3) {
          const uint32_t rb4 = vpf_bound_strip_bytes_px4(jobs[p].sw, jobs[p].dw, 1024u, 256u);
          rb = !rb4 ? 4096u : rb4 > rb ? rb4 : rb;
        }
    const bool narrow = r >= 8 && rb <= 1024;  // the IT = 1 instantiations (8 and 16 rows)
    if (r == 16 && !narrow) continue;
    const uint32_t slots = band_slots(r, scy);
    if (slots > (uint32_t)(narrow ? 2 * kBandSlots : kBandSlots) || 4u * slots * rb + 16u > 64u * 1024u) continue;
    uint64_t groups = 0;
    for (int p = 0; p < njobs; p++) groups += (uint64_t)((jobs[p].dw + 64u * band_px(jobs[p].ch, p1) - 1) / (64u * band_px(jobs[p].ch, p1))) * ((jobs[p].dh + 4 * r - 1) / (4 * r)) * n;
    if (forced || groups >= kBandMinGroups) return {r, band_slots_exact(r, njobs, jobs, slots), narrow, rb};
  }
  return {1, 0, false, rb_packed};
}
// the whole decision: 8 pixels per lane on the 1-channel planes only with the 16-slot (narrow-strip) instantiations that exist for it.
// Where that form would run 8-row bands on a DOWN-scale (every plane's vertical factor in [1, 2]) the launch takes the MARCH form instead
// (RowBand4wm): bands of 4 rows, nb of them per wave one below the other — the next band's source rows are requested while this band is
// blended, the walk's lerps and the column taps carry over — with half the LDS per wave (four waves per SIMD instead of three) and the
// wave's fixed part paid once per 4 nb rows.  nb = 2 or 3 while the launch keeps kBandMinGroups workgroups.  Measured on the 1- / 2-channel
// planes of Y / NV12 (profiles/r04_bilinear_march.txt: Y 1080p -> 720p 0.85 -> 0.79 us, NV12 1.14 -> 1.06); 3-channel planes and up-scales
// lose with it and keep their forms.  VPF_TUNE_RESIZE_BAND = 4 | nb << 8 forces it where it applies.
struct BandPlan { int rows; uint32_t slots; bool narrow; int p1; uint32_t rb; uint32_t nb; };
inline BandPlan plan_band(int variant, int band_knob, int njobs, const ResizeJob* jobs, const uint64_t* src_bits, uint32_t n) {
  const int p1 = band_p1(band_knob, njobs, jobs), knob = band_knob & 0xffff, forced_nb = (knob & 0xff) == 4 ? knob >> 8 : 0;  // (other row counts: the field is the persistent launch's chunk)
  if (p1 == 8) {
    const uint32_t rb = band_strip_bytes(variant, njobs, jobs, src_bits, 8);
    const BandShape bs = band_rows(band_knob, njobs, jobs, rb, n, 8);
    bool down = rb != 0 && rb <= 1024;
    float scy = 1.f;
    for (int p = 0; p < njobs && down; p++) {
      const float s = (float)jobs[p].sh / (float)jobs[p].dh;
      down = s >= 1.0f && s <= 2.0f;
      scy = s > scy ? s : scy;
    }
    if (down && (forced_nb ? bs.rows == 4 : ((knob & 0xff) == 0 && bs.rows == 8 && bs.narrow))) {
      uint64_t groups = 0;
      for (int p = 0; p < njobs; p++) groups += (uint64_t)((jobs[p].dw + 64u * band_px(jobs[p].ch, 8) - 1) / (64u * band_px(jobs[p].ch, 8))) * ((jobs[p].dh + 15) / 16) * n;
      const uint32_t nb = forced_nb ? (uint32_t)forced_nb : (uint32_t)std::min<uint64_t>(3, groups / kBandMinGroups);
      const uint32_t slots = band_slots_exact(4, njobs, jobs, band_slots(4, scy));
      if (nb >= (forced_nb ? 1u : 2u) && slots <= 9u && 4u * slots * rb + 16u <= 64u * 1024u) return {4, slots, true, 8, rb, nb};
    }
    if (bs.rows >= 8 && bs.narrow) return {bs.rows, bs.slots, true, 8, bs.rb, 0};
  }
  const uint32_t rb = band_strip_bytes(variant, njobs, jobs, src_bits, 4);
  const BandShape bs = band_rows(band_knob, njobs, jobs, rb, n, 4);
  return {bs.rows, bs.slots, bs.narrow, 4, bs.rb, 0};
}

// Every plane of a format over n <= kMaxBatch same-shape frames in as few dispatches as possible.  A 720p plane is 2-3 us of work, the same
// order as a kernel boundary, and an NV12 / YUV420 frame is two or three such planes: one launch per plane per frame leaves the chip idle most
// of the time.  The plane geometry decides the kernel family; when every plane of the format lands in the same (tiled or row-pair) family they
// all go into ONE launch (k_planes_mp), otherwise each plane gets one launch over all frames (k_plane_batch).  One plane of one frame keeps the
// scalar-argument entries, whose family rules differ in two places, marked (single) below.  Same task bodies everywhere -> identical pixels.
inline ResizePlan resize_plan(const ResizeShape& q) {
  ResizePlan P{};
  const int tune = q.variant, njobs = q.njobs, interp = q.interp;
  const uint32_t n = q.n;
  const bool f32 = q.f32;
  if (njobs < 1 || njobs > 3 || !n || n > (uint32_t)kMaxBatch) return P;
  P.ok = true;
  // one plane of one frame: the scalar-argument kernel entries (kernarg preload); measurement runs force the batch kernels on one frame.  (A
  // one-frame tail dispatch of a longer call, 33 frames at 32 per dispatch, keeps the frame-table kernels: the rule asks the CALL for one frame.)
  const bool forced_family = (q.mfma & 0xffff) >= 2 || (q.band & 0xffff) >= 2 || (q.band >> 16);
  const bool single = P.single = n == 1 && q.call_n == 1 && njobs == 1 && !forced_family;
  const ResizeJob* jobs = q.jobs;
  auto aligned = [&](int p, uint64_t src_mask, uint64_t dst_mask) { return !(q.src_bits[p] & src_mask) && !(q.dst_bits[p] & dst_mask); };
  auto set_tile = [&](ResizeLaunch& l, int family, const TileShape& t, uint32_t gx, uint32_t gy) {
    l.family = family; l.wpb = t.wpb; l.threads = 64u * (uint32_t)t.wpb; l.lds = t.lds;
    l.a0 = t.ty; l.a1 = t.nr; l.a2 = t.rowq; l.a3 = t.lshift;
    l.gx = gx; l.gy = gy; l.gz = n;
  };
  auto tile_of_plane = [&](ResizeLaunch& l, int family, const ResizeJob& j, const TileShape& t) { set_tile(l, family, t, (j.dw + 63) / 64, (j.dh + t.ty - 1) / t.ty); };
  // the tiled kernel for every plane in ONE launch: plane p's tiles start at workgroup row by0[p]
  auto tile_all_planes = [&](int family, const TileShape& t) {
    uint32_t gx = 0, gy = 0;
    for (int p = 0; p < njobs; p++) {
      P.by0[p] = gy;
      gx = std::max(gx, (jobs[p].dw + 63) / 64);
      gy += (jobs[p].dh + t.ty - 1) / t.ty;
    }
    set_tile(P.mp, family, t, gx, gy);
  };
  auto gather = [&](ResizeLaunch& l, const ResizeJob& j) {
    l.family = RESIZE_GATHER; l.lds = 0; l.a0 = l.a1 = l.a2 = l.a3 = 0;
    l.gx = ((j.dw + 3) / 4 + 63) / 64; l.gy = (j.dh + 3) / 4; l.gz = n; l.threads = 256;
  };
  // a Lanczos plane's own tile shape, for where the matrix-core launcher declines it — and (single) for one small plane, tried FIRST
  auto lz_fallback_tile = [&](ResizeLaunch& l, const ResizeJob& j, bool ok) {
    const TileShape t1 = ok ? plan_tile(q.tile, true, 1, &j, n) : TileShape{false, 0, 0, 0, 0, 0, 4};
    if (!t1.ok) return;
    tile_of_plane(l, RESIZE_LZ_MFMA, j, t1);
    l.fallback = RESIZE_LZ_TILE;
    if (single && lanczos_single_prefers_tile(q.mfma, j.ch, j.sw, j.sh, j.dw, j.dh)) l.family = RESIZE_LZ_TILE;
  };
  // bilinear up-scales: the tiled kernel for a single frame, the row-band kernel (8 or 4 destination rows per wave, each source row's
  // horizontal lerp evaluated once per band, no barriers) when the launch is large enough for it — 1080p -> 4K batched 11.9 -> 6.9 us / frame
  bool band_up = !single && !f32 && interp == VPF_INTERP_LINEAR && tune != 43 && tune != 9;
  if (band_up) band_up = plan_band(tune, q.band, njobs, jobs, q.src_bits, n).rows >= 4;
  uint32_t rowb[3] = {0, 0, 0};   // RESIZE_ROWPAIR: strip bytes
  bool lz_tile_ok[3] = {false, false, false};  // a Lanczos plane the tiled kernel may take when the matrix-core kernel does not
  TileShape tile1[3] = {};  // RESIZE_TILE: the plane's tile shape when it is launched on its own
  for (int p = 0; p < njobs; p++) {
    const ResizeJob& j = jobs[p];
    ResizeLaunch& l = P.plane[p];
    const float scx = (float)j.sw / (float)j.dw, scy = (float)j.sh / (float)j.dh;
    // Odd integer scale factors on both axes: s = (d + 0.5) k - 0.5 = k d + (k - 1) / 2 exactly, every destination centre is
    // a source pixel centre, so the bilinear fractions are 0 and the Lanczos weights are (0, 0, 1, 0, 0, 0): both filters return
    // that source pixel unchanged, which is also what NEAREST picks (floor((d + 0.5) k) = k d + (k - 1) / 2).  Identical
    // bytes from the cheapest kernel (the tiled kernels were tried with per-tap zero-weight skipping instead: 10 us for
    // Lanczos 4K -> 720p but 30-45 % slower on every other ratio).  8-bit bilinear keeps its row-pair LDS kernel, whose own
    // zero-weight shortcuts make it as fast there (kernel durations 5.1 vs 5.5 us at 4K -> 720p).
    const bool odd_int = j.sw % j.dw == 0 && j.sh % j.dh == 0 && ((j.sw / j.dw) & 1) && ((j.sh / j.dh) & 1) && j.sw < (1u << 22) && j.sh < (1u << 22) &&
                         tune != 40 && tune != 9;
    l.eff = interp;
    l.scx = scx; l.scy = scy;
    l.gz = n; l.threads = 256;
    if (f32) {
      if (interp != VPF_INTERP_NEAREST && odd_int) l.eff = VPF_INTERP_NEAREST;
      // Lanczos: the tiled separable form (16-B aligned source rows; 1080p -> 720p 22.7 -> 15.7 us, 720p -> 1080p 42.7 -> 19.5 us); the
      // gather form otherwise.  Bilinear stays on the gather form: tiled, a 720p -> 1080p up-scale took 17.0 us against 10.1 (four
      // times the bytes of an 8-bit surface go through LDS for little reuse); the bilinear branch of TileTaskF32 is reachable with tuning 43.
      if ((l.eff == VPF_INTERP_LANCZOS3 || (l.eff == VPF_INTERP_LINEAR && scy < 1.0f && tune == 43)) && tune != 9 && tune != 40 && aligned(p, 15, 0)) {
        l.lz = l.eff == VPF_INTERP_LANCZOS3;
        const TileShape t = plan_tile(q.tile, l.lz, 1, &j, n, 4);
        if (t.ok) {
          tile_of_plane(l, RESIZE_F32_TILE, j, t);
          l.vec_ok = aligned(p, 0, 15) ? 1 : 0;
          continue;
        }
      }
      l.family = RESIZE_F32_GATHER;
      l.gx = (j.dw + 63) / 64; l.gy = (j.dh + 3) / 4;
      continue;
    }
    if (interp == VPF_INTERP_LANCZOS3 && odd_int) l.eff = VPF_INTERP_NEAREST;
    l.vec_ok = aligned(p, 0, j.ch == 2 ? 7 : 3) ? 1 : 0;
    const bool src16 = tune != 9 && aligned(p, 15, 0);
    // exact 2x bilinear: the quad-structured streaming kernels
    if (l.eff == VPF_INTERP_LINEAR && j.sw == 2 * j.dw && j.sh == 2 * j.dh && j.dw % 4 == 0 && tune != 40 && tune != 9 && aligned(p, 7, j.ch == 2 ? 7 : 3)) {
      if (j.ch == 3 && j.sw % 32 == 0 && aligned(p, 15, 15)) {
        const uint32_t chunks = (j.sw + 1023) / 1024;
        l.family = RESIZE_HALF3;
        l.a0 = chunks; l.a1 = chunks * j.dh;
        l.gx = (l.a1 + 3) / 4; l.gy = 1;
      } else {
        l.family = RESIZE_HALF;
        l.gx = (j.dw / 4 + 63) / 64; l.gy = (j.dh + 3) / 4;
      }
    } else if (l.eff == VPF_INTERP_LANCZOS3) {
      // the matrix-core kernel (k_lanczos_mfma.hip) wherever its windows fit; the tiled separable form for strong down-scales (beyond those
      // windows) — and, tried FIRST, for one small plane per dispatch (lanczos_single_prefers_tile); the gather form for what is left.
      // (single): the matrix-core launcher is asked whatever the alignment (it declines unaligned rows itself); a batch asks it for 16-B rows only
      lz_tile_ok[p] = src16 && tune != 40;
      l.family = single || src16 ? RESIZE_LZ_MFMA : RESIZE_LZ_GATHER;
      l.fallback = RESIZE_LZ_GATHER;
      l.gx = (j.dw + 63) / 64; l.gy = (j.dh + 3) / 4;
      if (single) lz_fallback_tile(l, j, lz_tile_ok[p]);  // (a batch: below, unless one tile launch takes every plane before anything else)
    } else {
      // up-scaling: several destination rows sit between the same two source rows -> tiled kernel (horizontal lerp once per
      // source row).  Kernel durations (rocprofv3), tiled vs row-pair: 1080p->4K 16.6 vs 20.6 us, 720p->1080p 8.2 vs 9.0;
      // for mild down-scales the row-pair kernel is as fast or faster (1080p->720p 5.9 vs 5.8, 4K->1440p 16.2 vs 12.4,
      // 4K->3000x1688 21.2 vs 14.9), so the tiled kernel is used below 1.0 only
      const bool want_tile = l.eff == VPF_INTERP_LINEAR && (scy < 1.0f || tune == 43) && tune != 40 && src16 && !band_up;
      if (want_tile && single) tile1[p] = plan_tile(q.tile, false, 1, &j, n);  // (a batch: below, where the planes do not all go into one launch)
      // strip bytes a wave of the row-pair kernel needs per source row (vpf_bound_strip_bytes): the row pair is not taken under variant 9 or
      // for an unaligned source — src16 holds both, asked of EVERY frame (the launchers used to ask frame 0 once more) — or when the span is
      // above the cap
      if (want_tile && (tile1[p].ok || !single)) {
        // a batch: decided below, once it is known whether every plane is in this position; (single): a span that does not fit the tile's
        // strip goes on to the row pair
        l.family = RESIZE_TILE;
        if (tile1[p].ok) tile_of_plane(l, RESIZE_TILE, j, tile1[p]);
      } else if (l.eff == VPF_INTERP_LINEAR && src16 && (rowb[p] = vpf_bound_strip_bytes(j.ch, j.sw, j.dw, kResizeRowBytes, 256)) != 0) {
        // (capping residency at 4 / 2 / 1 workgroups per CU to stagger the waves was measured: 8.5 / 8.7 / 11.3 us vs 8.4)
        l.family = RESIZE_ROWPAIR;
        l.it = (int)((rowb[p] + 1023) / 1024); l.lds = 4 * 2 * rowb[p] + 16;  // + 16: a tap window may start in a strip's last dword
        l.a0 = rowb[p] / 16;
        l.gx = ((j.dw + 3) / 4 + 63) / 64; l.gy = (j.dh + 3) / 4;
      } else {
        gather(l, j);
      }
    }
  }
  if (single || f32) return P;
  // ---- every plane Lanczos: one matrix-core launch for the whole format (k_lanczos_mfma.hip); planes it cannot take fall back
  bool all_mfma = true;
  for (int p = 0; p < njobs; p++) all_mfma = all_mfma && P.plane[p].family == RESIZE_LZ_MFMA;
  if (all_mfma) {
    P.lz_mfma_all = true;
    bool tile_ok = true;
    uint64_t dst_b = 0;
    for (int p = 0; p < njobs; p++) { dst_b += (uint64_t)jobs[p].dw * jobs[p].dh * (uint32_t)jobs[p].ch; tile_ok = tile_ok && lz_tile_ok[p]; }
    const TileShape tl = tile_ok ? plan_tile(q.tile, true, njobs, jobs, n) : TileShape{false, 0, 0, 0, 0, 0, 4};
    if (tl.ok) {
      tile_all_planes(RESIZE_LZ_TILE, tl);
      P.mp.eff = VPF_INTERP_LANCZOS3;
      // what the matrix-core kernel does not take (the strongest down-scales): the tiled separable kernel — one launch for the whole format
      // when every plane is in that position, else plane by plane — and the gather kernel for what is left
      P.lz_tile_all_fallback = true;
      // ONE frame of a multi-plane format per dispatch with a small destination (all planes together <= 1 MB: up to ~1100 x 640): a lone launch
      // of the matrix-core kernel is a latency chain of 8-9 us whatever the picture (lanczos_single_prefers_tile above has the single-plane
      // rule), the tile kernel — whose time follows the destination — leaves such a frame after 6-7 (profiles/r04_lanczos_single_multiplane.txt:
      // YUV420 1080p -> 224 x 224 5.9 against 7.9 us, NV12 1080p -> 416 x 416 6.8 against 9.0; 1080p -> 720p stays on the matrix cores, 7.5
      // against 8.3).  Only where ONE tile launch takes every plane (the chroma plane of NV12 at 8 x falls out of its windows).
      P.lz_tile_all_first = n == 1 && njobs > 1 && !(q.mfma & 0xfffff) && dst_b <= 1000000ull;
      if (P.lz_tile_all_first) return P;
    }
  }
  for (int p = 0; p < njobs; p++)
    if (P.plane[p].family == RESIZE_LZ_MFMA) lz_fallback_tile(P.plane[p], jobs[p], lz_tile_ok[p]);
  if (all_mfma) return P;
  // ---- every plane tiled, or every plane on the row pair: one launch for the whole format
  bool all_tile = true, all_rowpair = true;
  for (int p = 0; p < njobs; p++) {
    all_tile = all_tile && P.plane[p].family == RESIZE_TILE && P.plane[p].eff == P.plane[0].eff;
    all_rowpair = all_rowpair && P.plane[p].family == RESIZE_ROWPAIR;
  }
  if (all_tile) {
    const TileShape ts = plan_tile(q.tile, false, njobs, jobs, n);
    if (!ts.ok) {  // the span does not fit a strip: every plane falls back to its gather form
      for (int p = 0; p < njobs; p++) gather(P.plane[p], jobs[p]);
      return P;
    }
    P.all = true;
    tile_all_planes(RESIZE_TILE, ts);
    P.mp.eff = P.plane[0].eff;
    return P;
  }
  for (int p = 0; p < njobs; p++)  // mixed families: a tiled plane is tiled on its own, or falls back to its gather form
    if (P.plane[p].family == RESIZE_TILE) {
      tile1[p] = plan_tile(q.tile, false, 1, &jobs[p], n);
      if (tile1[p].ok) tile_of_plane(P.plane[p], RESIZE_TILE, jobs[p], tile1[p]);
      else gather(P.plane[p], jobs[p]);
    }
  // the band plan of a row-pair plane launched on its own
  auto band_of = [&](ResizeLaunch& l, const BandPlan& bs) {
    l.family = RESIZE_BAND;
    l.rows = bs.rows; l.p1 = bs.p1; l.narrow = bs.narrow; l.multi = bs.rows == 4 && bs.p1 == 8;
    l.it = bs.p1 == 8 || (bs.rows >= 8 && bs.narrow) ? 1 : 2;  // RowBandTask<CH, rows, it, p1, multi>: the eight instantiations (with_band_form, k_resize.hip)
    l.a0 = bs.rb / 16; l.a1 = bs.slots; l.a2 = bs.nb;
    l.lds = 4 * bs.slots * bs.rb + 16;
  };
  if (all_rowpair) {
    P.all = true;
    ResizeLaunch& m = P.mp;
    m.eff = VPF_INTERP_LINEAR; m.threads = 256;
    uint32_t rb = 0;
    for (int p = 0; p < njobs; p++) rb = rowb[p] > rb ? rowb[p] : rb;  // one strip size for the launch (the widest plane's)
    const BandPlan bs = plan_band(tune, q.band, njobs, jobs, q.src_bits, n);
    const uint32_t band = (uint32_t)bs.rows, band_nb = bs.nb ? bs.nb : 1u;  // bands per wave (the march form)
    if (band > 1) {
      band_of(m, bs);
    } else {
      m.family = RESIZE_ROWPAIR;
      m.it = (int)((rb + 1023) / 1024); m.lds = 4 * 2 * rb + 16;
      m.a0 = rb / 16; m.a1 = bs.slots; m.a2 = bs.nb;
    }
    for (int p = 0; p < njobs; p++) {
      const uint32_t wcols = band > 1 ? 64u * band_px(jobs[p].ch, bs.p1) : 256u, bx = (jobs[p].dw + wcols - 1) / wcols;
      P.by0[p] = m.gy;
      m.gx = bx > m.gx ? bx : m.gx;
      m.gy += (jobs[p].dh + 4 * band * band_nb - 1) / (4 * band * band_nb);
    }
    m.gz = n;
    return P;
  }
  // ---- otherwise: one launch per plane over all frames; a row-pair plane takes the band form where its own launch is large enough
  for (int p = 0; p < njobs; p++) {
    ResizeLaunch& l = P.plane[p];
    if (l.family != RESIZE_ROWPAIR) continue;
    const BandPlan bs = plan_band(tune, q.band, 1, &jobs[p], &q.src_bits[p], n);
    if (bs.rows <= 1) continue;
    const uint32_t wcols = 64u * band_px(jobs[p].ch, bs.p1), nbw = bs.nb ? bs.nb : 1u;
    band_of(l, bs);
    l.gx = (jobs[p].dw + wcols - 1) / wcols; l.gy = (jobs[p].dh + 4 * bs.rows * nbw - 1) / (4 * bs.rows * nbw);
  }
  return P;
}

}  // namespace vpf
