// vpf_job_bounds.h — the strip sizing of the two per-job kernel families (k_convert_roi.hip, k_convert_warp.hip), in a header that hipcc (host
// and device) and plain g++ compile as it stands, so that the launchers, the kernels and a CPU property test (tests/test_job_bounds_cpu.py
// through tests/c/job_bounds_capi.cpp) use the SAME code.  The sibling of vpf_plan_bounds.h, for the same reason: a bound that is one byte
// or one row short is silent — k_roi_strip returns without writing, k_warp_strip blends from the wrong texels.
// How the eight launches COMBINE these — which bound decides which job, the caps, the grids, which figure goes to the kernel and which to the launch
// — is job_plan (vpf_job_plan.h, tests/test_job_plan_cpu.py); this header holds what a job or a tile needs.
//   ROI   roi_strip_need: the largest workgroup strip of a job, WALKED with the kernel's own fp32 tap arithmetic, and the policy's two limits
//   letterbox  letterbox_strip_need: the same walk over tiles laid on the destination plane and clipped to the picture (k_convert_letterbox.hip;
//         tests/test_letterbox_bounds_cpu.py through tests/c/letterbox_bounds_capi.cpp)
//         letterbox_fit_ints / letterbox_dev_rect_ok / letterbox_tile_window: the fit (vpf_letterbox_fit's integers), the placement's guard and the
//         per-tile window of the device-table form (k_convert_letterbox_dev.hip; tests/test_letterbox_dev_cpu.py through
//         tests/c/letterbox_dev_bounds_capi.cpp)
//   warp  warp_xy / warp_window / warp_strip: what the kernel computes per tile; warp_need: the launcher's closed-form bound over all tiles;
//         warp_dev_job_ok / warp_dev_lds_bytes: the guard and the LDS bound of the device-table form (k_convert_warp_dev.hip;
//         tests/test_warps_dev_bounds_cpu.py through tests/c/warp_dev_bounds_capi.cpp)
//   persp persp_xy / persp_window / persp_px_in_window / persp_need: the perspective warp's (k_convert_persp.hip); persp_dev_job_ok / persp_step /
//         persp_dev_lds_bytes: the guard, the caller's hint and the LDS bound of its device-table form (k_convert_persp_dev.hip)
//   remap remap_tap / remap_win_none / remap_win_add / remap_win_merge: what ONE pixel of a per-pixel map contributes to its tile's source window and
//         how contributions merge (k_convert_remap.hip; tests/test_remap_tensor_cpu.py through tests/c/remap_bounds_capi.cpp)
#ifndef VPF_JOB_BOUNDS_H_
#define VPF_JOB_BOUNDS_H_
#include <math.h>
#include <stdint.h>

#include "vpf_plan_bounds.h"

#ifdef __HIPCC__
#define VPF_JB_HD __host__ __device__ __forceinline__
#define VPF_JB_HDI __host__ __device__ __forceinline__
#else
#define VPF_JB_HD inline  // (a translation unit may leave any of them unused — vpf_job_plan.h's users do: no warning under -Wall)
#define VPF_JB_HDI inline
#endif

// ------------------------------------------------------------------------------------------
// ROI (k_convert_roi.hip).  A workgroup of the staged form owns 16 destination rows (four waves x kRoiBandRows) x 256 destination columns.
// ------------------------------------------------------------------------------------------
constexpr int kRoiBandRows = 4;  // destination rows per wave of the staged form: a workgroup's strip serves 16 rows x 256 columns
constexpr uint32_t kRoiStripMax = 53u * 1024u;  // three workgroups per CU (160 KiB)
constexpr double kRoiConvMax = 3.0;  // source pixels converted per destination pixel: the measured break-even of the strip against the per-tap kernels
struct RoiStripNeed {
  uint32_t bytes;  // rows x row bytes of the job's largest workgroup strip
  double conv;     // source pixels converted per destination pixel (the gather form converts four)
};
// rectangle (x, .., w, h) of the frame -> dw x dh, scx = (float)w / (float)dw and scy likewise as the entry passes them (the row walk does not
// depend on the rectangle's row offset: the strip's rows are rectangle rows)
static inline RoiStripNeed roi_strip_need(uint32_t x, uint32_t w, uint32_t h, float scx, float scy, uint32_t dw, uint32_t dh) {
  uint32_t rowbytes = 0, rows = 0;
  for (uint32_t xs = 0; xs < dw; xs += 256) {
    const uint32_t xe = xs + 255 < dw - 1 ? xs + 255 : dw - 1;
    const uint32_t i0 = vpf_lin_i0(xe, scx, w);
    const uint32_t first = x + vpf_lin_i0(xs, scx, w), last = x + (i0 + 1 < w ? i0 + 1 : w - 1);
    const uint32_t rb = 32u * (((last - (first & ~1u)) >> 3) + 1u) + 16u;
    rowbytes = rb > rowbytes ? rb : rowbytes;
  }
  for (uint32_t ya = 0; ya < dh; ya += 4 * kRoiBandRows) {
    const uint32_t yb = ya + 4 * kRoiBandRows - 1 < dh - 1 ? ya + 4 * kRoiBandRows - 1 : dh - 1;
    const uint32_t lo = vpf_lin_i0(ya, scy, h), hi0 = vpf_lin_i0(yb, scy, h), hi = hi0 + 1 < h ? hi0 + 1 : h - 1;
    rows = hi - lo + 1 > rows ? hi - lo + 1 : rows;
  }
  const uint32_t cols = dw < 256 ? dw : 256, brows = dh < 4 * kRoiBandRows ? dh : 4 * kRoiBandRows;
  return RoiStripNeed{rows * rowbytes, (double)rows * (rowbytes / 4) / ((double)cols * brows)};
}
// the policy: staged where the window fits a strip that leaves three workgroups per CU and converts at most kRoiConvMax source pixels per
// destination pixel; everything else gathers
static inline bool roi_job_staged(const RoiStripNeed& need) { return need.bytes <= kRoiStripMax && need.conv <= kRoiConvMax; }

// ------------------------------------------------------------------------------------------
// Device-resident boxes (k_convert_roi_dev.hip, vpf_convert_resize_tensor_rois_dev).  The rectangle is read from device memory by the kernel, so what
// the host entry checks before the launch and what its launcher decides per job happen in the kernel: the guard, and staged or per tap PER TILE.
// ------------------------------------------------------------------------------------------
// The guard: the ONLY thing between five untrusted ints and a read outside the frame.  Unsigned compares, no sums: w <= W before W - w, so no
// operation can wrap.  (frame < 0 is a large unsigned number; n_frames <= 128.)
static VPF_JB_HDI bool roi_dev_box_ok(int32_t frame, int32_t x, int32_t y, int32_t w, int32_t h, uint32_t n_frames, uint32_t W, uint32_t H) {
  return (uint32_t)frame < n_frames && w >= 1 && h >= 1 && x >= 0 && y >= 0 && (uint32_t)w <= W && (uint32_t)h <= H && (uint32_t)x <= W - (uint32_t)w &&
         (uint32_t)y <= H - (uint32_t)h;
}
// vpf_lin_i0 (= make_tap<LINEAR>'s i0) for host and device
static VPF_JB_HDI uint32_t roi_lin_i0(uint32_t d, float scale, uint32_t size) {
  float s = fmaf((float)d + 0.5f, scale, -0.5f);
  s = fmaxf(s, 0.f);
  s = fminf(s, (float)(size - 1));
  return (uint32_t)(int32_t)s;
}
// The source window of ONE tile (destination columns xs .. xe, rows Y0 .. Y1) of a job: frame pixels first .. last of every row, rectangle rows
// lo .. hi, and the strip that holds them (whole conversion units from the even pixel at or below `first`: the layout of k_roi_strip) — the
// arithmetic roi_strip_need walks per chunk and per band.
struct RoiTileWin {
  uint32_t first, last, lo, hi;  // frame pixels | rectangle rows
  uint32_t base_px, ng, rowbytes, rows;
};
static VPF_JB_HDI RoiTileWin roi_tile_window(uint32_t x, uint32_t w, uint32_t h, float scx, float scy, uint32_t xs, uint32_t xe, uint32_t Y0, uint32_t Y1) {
  RoiTileWin t;
  const uint32_t i0 = roi_lin_i0(xe, scx, w), hi0 = roi_lin_i0(Y1, scy, h);
  t.first = x + roi_lin_i0(xs, scx, w);
  t.last = x + (i0 + 1 < w ? i0 + 1 : w - 1);
  t.lo = roi_lin_i0(Y0, scy, h);
  t.hi = hi0 + 1 < h ? hi0 + 1 : h - 1;
  t.base_px = t.first & ~1u;
  t.ng = ((t.last - t.base_px) >> 3) + 1u;
  t.rowbytes = 32u * t.ng + 16u;
  t.rows = t.hi - t.lo + 1u;
  return t;
}
// ... and what the policy looks at.  `conv` counts against the pixels a full tile of the job holds (min(dw, 256) x min(dh, 16)), as roi_strip_need's
// does: over all tiles of a job the largest `bytes` is roi_strip_need's bytes and the largest `conv` its conv (rows and row bytes vary independently
// over the grid of tiles; tests/test_rois_dev_bounds_cpu.py).
static VPF_JB_HDI RoiStripNeed roi_tile_need_of(const RoiTileWin& t, uint32_t dw, uint32_t dh) {
  const uint32_t cols = dw < 256 ? dw : 256, brows = dh < 4 * kRoiBandRows ? dh : 4 * kRoiBandRows;
  return RoiStripNeed{t.rows * t.rowbytes, (double)t.rows * (t.rowbytes / 4) / ((double)cols * brows)};
}
static VPF_JB_HDI RoiStripNeed roi_tile_need(uint32_t x, uint32_t w, uint32_t h, float scx, float scy, uint32_t xs, uint32_t xe, uint32_t Y0, uint32_t Y1,
                                            uint32_t dw, uint32_t dh) {
  return roi_tile_need_of(roi_tile_window(x, w, h, scx, scy, xs, xe, Y0, Y1), dw, dh);
}
// A tile is staged when its strip fits the dynamic LDS of the dispatch and converts at most kRoiConvMax source pixels per destination pixel.
// conv <= kRoiConvMax bounds the strip by 12 B x the pixels of a full tile, so a dispatch never needs more LDS than that (roi_dev_lds_bytes): small
// destinations keep their occupancy although no strip is known at the launch.
static VPF_JB_HDI bool roi_tile_staged(const RoiStripNeed& need, uint32_t lds_bytes) { return need.bytes <= lds_bytes && need.conv <= kRoiConvMax; }
static inline uint32_t roi_dev_lds_bytes(uint32_t dw, uint32_t dh) {
  const uint32_t cols = dw < 256 ? dw : 256, brows = dh < 4 * kRoiBandRows ? dh : 4 * kRoiBandRows;
  const uint32_t cap = ((uint32_t)(kRoiConvMax * 4.0) * cols * brows + 15u) & ~15u;
  return cap < kRoiStripMax ? cap : kRoiStripMax;
}

// ------------------------------------------------------------------------------------------
// Letterbox (k_convert_letterbox.hip).  The ROI kernels' workgroup tile (16 rows x 256 columns), laid on the DESTINATION PLANE dw x dh; the picture
// (rectangle -> iw x ih, scx = (float)w / (float)iw and scy likewise) sits at (ix, iy) of the plane.  A tile that meets the picture clips its column
// and row range to it — xs' = max(xs, ix) - ix .. xe' = min(xe, ix + iw - 1) - ix, rows likewise — and its strip holds the taps of that range: a
// clipped chunk does not start at a multiple of 256 picture columns, so this is a walk of its own, with the same fp32 tap arithmetic.  Tiles that
// miss the picture have no strip.  `conv` counts against the picture pixels a tile can hold (min(iw, 256) x min(ih, 16)): with (ix, iy, iw, ih) =
// (0, 0, dw, dh) both members equal roi_strip_need's, and the policy is the ROI one (roi_job_staged).
// ------------------------------------------------------------------------------------------
static inline RoiStripNeed letterbox_strip_need(uint32_t x, uint32_t w, uint32_t h, float scx, float scy, uint32_t ix, uint32_t iy, uint32_t iw,
                                                uint32_t ih, uint32_t dw, uint32_t dh) {
  uint32_t rowbytes = 0, rows = 0;
  for (uint32_t xs = ix & ~255u; xs < dw && xs < ix + iw; xs += 256) {  // (the chunks left of ix & ~255 end before the picture)
    const uint32_t xe = xs + 255 < dw - 1 ? xs + 255 : dw - 1;
    const uint32_t cs = (xs > ix ? xs : ix) - ix, ce = (xe < ix + iw - 1 ? xe : ix + iw - 1) - ix;
    const uint32_t i0 = vpf_lin_i0(ce, scx, w);
    const uint32_t first = x + vpf_lin_i0(cs, scx, w), last = x + (i0 + 1 < w ? i0 + 1 : w - 1);
    const uint32_t rb = 32u * (((last - (first & ~1u)) >> 3) + 1u) + 16u;
    rowbytes = rb > rowbytes ? rb : rowbytes;
  }
  constexpr uint32_t kBand = 4 * kRoiBandRows;
  for (uint32_t ya = iy - iy % kBand; ya < dh && ya < iy + ih; ya += kBand) {
    const uint32_t yb = ya + kBand - 1 < dh - 1 ? ya + kBand - 1 : dh - 1;
    const uint32_t cs = (ya > iy ? ya : iy) - iy, ce = (yb < iy + ih - 1 ? yb : iy + ih - 1) - iy;
    const uint32_t lo = vpf_lin_i0(cs, scy, h), hi0 = vpf_lin_i0(ce, scy, h), hi = hi0 + 1 < h ? hi0 + 1 : h - 1;
    rows = hi - lo + 1 > rows ? hi - lo + 1 : rows;
  }
  const uint32_t cols = iw < 256 ? iw : 256, brows = ih < kBand ? ih : kBand;
  return RoiStripNeed{rows * rowbytes, (double)rows * (rowbytes / 4) / ((double)cols * brows)};
}

// ------------------------------------------------------------------------------------------
// Device-resident boxes for the letterbox (k_convert_letterbox_dev.hip, vpf_convert_letterbox_tensor_dev; tests/test_letterbox_dev_cpu.py through
// tests/c/letterbox_dev_bounds_capi.cpp).  The kernel reads the box — and the placement, where the caller gives one — from device memory, so the
// fit, the placement's guard and staged or per tap PER TILE happen in the kernel.
// ------------------------------------------------------------------------------------------
// The aspect-preserving, centred placement of a w x h picture inside dw x dh (vpf_letterbox_fit, include/vpf_hip.h), integers only: 64-bit
// products and ONE 64-bit division.  With sides <= 65536 the largest intermediate is 2 * 2^16 * 2^16 + 2^16 < 2^34.  Every side >= 1.
struct LetterboxFit { uint32_t ix, iy, iw, ih; };
static VPF_JB_HDI LetterboxFit letterbox_fit_ints(uint32_t w32, uint32_t h32, uint32_t dw32, uint32_t dh32) {
  const uint64_t w = w32, h = h32, dw = dw32, dh = dh32;
  const bool wide = w * dh >= h * dw;  // width-limited
  // the free side: round half up of (short side of the picture x the limiting side of the plane) / the long side of the picture
  const uint64_t num = wide ? 2 * h * dw + w : 2 * w * dh + h, den = wide ? 2 * w : 2 * h, lim = wide ? dh : dw;
  uint64_t q = num / den;
  q = q < 1 ? 1 : (q > lim ? lim : q);
  const uint64_t iw = wide ? dw : q, ih = wide ? q : dh;
  return LetterboxFit{(uint32_t)((dw - iw) / 2), (uint32_t)((dh - ih) / 2), (uint32_t)iw, (uint32_t)ih};
}
// The guard of an explicit placement: four untrusted ints must name a non-empty rectangle inside the dw x dh plane.  As roi_dev_box_ok: unsigned
// compares, no sums — iw <= dw before dw - iw, so no operation can wrap.
static VPF_JB_HDI bool letterbox_dev_rect_ok(int32_t ix, int32_t iy, int32_t iw, int32_t ih, uint32_t dw, uint32_t dh) {
  return iw >= 1 && ih >= 1 && ix >= 0 && iy >= 0 && (uint32_t)iw <= dw && (uint32_t)ih <= dh && (uint32_t)ix <= dw - (uint32_t)iw &&
         (uint32_t)iy <= dh - (uint32_t)ih;
}
// The source window of ONE tile of the PLANE (columns xs .. xe, rows Y0 .. Y1) that MEETS the picture (xs <= ix + iw - 1, xe >= ix, rows likewise;
// the caller tests that): the tile's range clipped to the picture exactly as letterbox_strip_need and k_lb_strip clip it, then roi_tile_window on the
// clipped picture columns and rows.  `cxs .. cye`: the clipped range in picture pixels.
struct LetterboxTileWin {
  RoiTileWin w;
  uint32_t cxs, cxe, cys, cye;
};
static VPF_JB_HDI LetterboxTileWin letterbox_tile_window(uint32_t x, uint32_t w, uint32_t h, float scx, float scy, uint32_t ix, uint32_t iy, uint32_t iw,
                                                         uint32_t ih, uint32_t xs, uint32_t xe, uint32_t Y0, uint32_t Y1) {
  LetterboxTileWin t;
  const uint32_t ixe = ix + iw - 1, iye = iy + ih - 1;
  t.cxs = (xs > ix ? xs : ix) - ix; t.cxe = (xe < ixe ? xe : ixe) - ix;
  t.cys = (Y0 > iy ? Y0 : iy) - iy; t.cye = (Y1 < iye ? Y1 : iye) - iy;
  t.w = roi_tile_window(x, w, h, scx, scy, t.cxs, t.cxe, t.cys, t.cye);
  return t;
}
// ... and what the policy looks at: `conv` counts against the picture pixels a tile can hold (min(iw, 256) x min(ih, 16)), as letterbox_strip_need's
// does, so over the tiles that meet the picture the largest `bytes` and `conv` are the job's.  The tile is staged by roi_tile_staged under the
// dispatch's roi_dev_lds_bytes(dw, dh), which stays a bound: conv <= kRoiConvMax = 3 means rows x (rowbytes / 4) <= 3 x min(iw, 256) x min(ih, 16),
// hence bytes = rows x rowbytes <= 12 B x the picture pixels of a tile <= 12 B x min(dw, 256) x min(dh, 16), the plane pixels of a tile (iw <= dw,
// ih <= dh) — what roi_dev_lds_bytes returns before its cap at kRoiStripMax; above the cap the tile samples per tap, as the host policy has it.
// Were this argument wrong, k_lb_dev's own test rows x rowbytes > lds_bytes -> per tap keeps it from becoming an overrun.
static VPF_JB_HDI RoiStripNeed letterbox_tile_need_of(const RoiTileWin& t, uint32_t iw, uint32_t ih) {
  const uint32_t cols = iw < 256 ? iw : 256, brows = ih < 4 * kRoiBandRows ? ih : 4 * kRoiBandRows;
  return RoiStripNeed{t.rows * t.rowbytes, (double)t.rows * (t.rowbytes / 4) / ((double)cols * brows)};
}

// ------------------------------------------------------------------------------------------
// Warp (k_convert_warp.hip).
// Destination tile of a workgroup: 1024 pixels, four per lane.  Close to square keeps a rotated footprint's bounding box small; 32 x 32 measured
// against 64 x 16 and 16 x 64 (builds with -DVPF_WARP_TILE_W= -DVPF_WARP_TILE_H=, tools/warp_kernel_ab.py).
// ------------------------------------------------------------------------------------------
#ifndef VPF_WARP_TILE_W
#define VPF_WARP_TILE_W 32
#define VPF_WARP_TILE_H 32
#endif
constexpr uint32_t kWarpTileW = VPF_WARP_TILE_W, kWarpTileH = VPF_WARP_TILE_H, kWarpLanesX = kWarpTileW / 4;
static_assert(kWarpTileW * kWarpTileH == 1024 && kWarpTileW % 4 == 0, "a workgroup of 256 lanes x 4 pixels covers one tile");

// Coordinates: host and device run the same separately rounded fp32 operations (the host sizes the strips with them).
struct WarpXY { float sx, sy; };
static VPF_JB_HD WarpXY warp_xy(const float* m, uint32_t dx, uint32_t dy, bool rep, float wmax, float hmax) {
  const float fx = (float)dx, fy = (float)dy;
  float sx = (m[0] * fx + m[1] * fy) + m[2];
  float sy = (m[3] * fx + m[4] * fy) + m[5];
  if (rep) {  // a max, then a min
    sx = fminf(fmaxf(sx, 0.f), wmax);
    sy = fminf(fmaxf(sy, 0.f), hmax);
  }
  return WarpXY{sx, sy};
}
// The source window of a destination tile [xs, xe] x [ys, ye]: rounding is monotonic, so sx and sy are monotonic in dx for fixed dy and in dy
// for fixed dx (clamped or not) and their extremes over the tile lie at its four corners, exactly.  Every in-range pixel of the tile has
// x_lo <= x0, x1 <= x_hi and y_lo <= y0, y1 <= y_hi; `empty`: no pixel of the tile is in range.
struct WarpWin {
  uint32_t x_lo, x_hi, y_lo, y_hi;
  bool empty;
};
static VPF_JB_HD WarpWin warp_window(const float* m, uint32_t xs, uint32_t xe, uint32_t ys, uint32_t ye, bool rep, uint32_t W, uint32_t H) {
  const float wmax = (float)(W - 1), hmax = (float)(H - 1);
  const WarpXY a = warp_xy(m, xs, ys, rep, wmax, hmax), b = warp_xy(m, xe, ys, rep, wmax, hmax), c = warp_xy(m, xs, ye, rep, wmax, hmax),
               d = warp_xy(m, xe, ye, rep, wmax, hmax);
  const float xmin = fminf(fminf(a.sx, b.sx), fminf(c.sx, d.sx)), xmax = fmaxf(fmaxf(a.sx, b.sx), fmaxf(c.sx, d.sx));
  const float ymin = fminf(fminf(a.sy, b.sy), fminf(c.sy, d.sy)), ymax = fmaxf(fmaxf(a.sy, b.sy), fmaxf(c.sy, d.sy));
  WarpWin w{0u, 0u, 0u, 0u, !(xmax >= 0.f && xmin <= wmax && ymax >= 0.f && ymin <= hmax)};
  if (w.empty) return w;
  w.x_lo = (uint32_t)(int)fmaxf(xmin, 0.f);
  w.y_lo = (uint32_t)(int)fmaxf(ymin, 0.f);
  const uint32_t xh = (uint32_t)(int)fminf(xmax, wmax), yh = (uint32_t)(int)fminf(ymax, hmax);
  w.x_hi = xh + 1 < W ? xh + 1 : W - 1;
  w.y_hi = yh + 1 < H ? yh + 1 : H - 1;
  return w;
}
// the strip of a window: whole conversion units from the even pixel at or below x_lo, rows y_lo .. y_hi (the layout of k_roi_strip)
struct WarpStrip { uint32_t base_px, ng, rowbytes, rows, bytes; };
static VPF_JB_HD WarpStrip warp_strip(const WarpWin& w) {
  WarpStrip s;
  s.base_px = w.x_lo & ~1u;
  s.ng = ((w.x_hi - s.base_px) >> 3) + 1;
  s.rowbytes = 32u * s.ng + 16u;  // 16-B unit writes force a pitch of whole four-dword slots; the odd slot keeps rows of ng = 4 k units off one bank
  s.rows = w.y_hi - w.y_lo + 1;
  s.bytes = s.rows * s.rowbytes;
  return s;
}

// The dynamic LDS of a dispatch is an UPPER BOUND of every tile's strip, from the matrix alone, O(1) per job (a walk over every
// tile's corners cost ~10 ns per tile and bounded the whole call).  Along one axis a tile of tw x th pixels spans at most
// |r0| (tw - 1) + |r1| (th - 1) in exact arithmetic; each fp32 coordinate is off by at most 2^-23 (|r0| dx + |r1| dy + |r2|) (three roundings
// of half an ulp of values no larger than that sum), taken four times over here; x_hi - x_lo + 1 <= floor(xmax) - floor(xmin) + 2 <= span + 3;
// a clamp (REPLICATE, the frame) only shrinks a window.  The kernel compares the strip it computes with the bytes it was given and takes the
// per-tap path for a tile that would not fit, so a bound that were ever short costs time, not pixels.
// Policy (measured): the staged form wherever a tile's strip fits kWarpStripMax, the per-tap form otherwise.  Kernel time of the staged
// form is 0.50-0.82 x the per-tap form's in every case whose strip fits, 2.86 x down-scales at 15 degrees (about 12 source pixels converted per
// destination pixel) included: no break-even in converted pixels is reached before the strip outgrows the LDS, so there is none in the policy.
// 64 KiB (two workgroups per CU, the most a launch takes without an attribute) against 53 KiB (three): every case that fits 53 KiB runs the same
// either way, and 2.7 x at 45 degrees (62 KiB) takes 0.585 us per region staged against 0.754 per tap.
#ifndef VPF_WARP_STRIP_MAX_KIB
#define VPF_WARP_STRIP_MAX_KIB 64
#endif
constexpr uint32_t kWarpStripMax = VPF_WARP_STRIP_MAX_KIB * 1024u;
struct WarpNeed {
  uint32_t bytes;  // upper bound of the job's largest tile strip
};
// pixels of a tile's window along one axis, at most (r: the matrix row of that axis, S: the frame's size along it)
static inline uint32_t warp_need_count(const float* r, uint32_t S, double tw, double th, uint32_t dw, uint32_t dh) {
  const double span = fabs((double)r[0]) * (tw - 1) + fabs((double)r[1]) * (th - 1);
  const double err = 4.0 * 0x1p-23 * (fabs((double)r[0]) * dw + fabs((double)r[1]) * dh + fabs((double)r[2]));
  const double n = floor(span + 2.0 * err) + 3.0;
  return n < (double)S ? (uint32_t)n : S;
}
static inline WarpNeed warp_need(const float m[6], uint32_t W, uint32_t H, uint32_t dw, uint32_t dh) {
  const double tw = dw < kWarpTileW ? dw : kWarpTileW, th = dh < kWarpTileH ? dh : kWarpTileH;
  const uint32_t nx = warp_need_count(m, W, tw, th, dw, dh), rows = warp_need_count(m + 3, H, tw, th, dw, dh);
  uint32_t ng = (nx >> 3) + 1;  // the strip starts on the even pixel at or below x_lo
  const uint32_t ng_max = ((W - 1) >> 3) + 1;
  ng = ng < ng_max ? ng : ng_max;
  return WarpNeed{rows * (32u * ng + 16u)};
}

// ------------------------------------------------------------------------------------------
// Device-resident matrices (k_convert_warp_dev.hip, vpf_convert_warp_tensor_dev).  The kernel reads (frame, m[6]) of its job from device memory, so the
// host entry's check of the matrix happens in the kernel, and the launcher sizes the LDS without a matrix.
// ------------------------------------------------------------------------------------------
// The guard: the ONLY thing between untrusted device memory and a read outside a frame.  One unsigned compare (frame < 0 is a large unsigned number;
// n_frames <= 128) and the host entry's six: NaN and the infinities fail `<=`.  With every |m| <= 2^24 and dx, dy <= 65535, sx and sy are finite (at
// most 2^41 in magnitude), the range test and the clamps work on ordinary numbers and every tap lies inside the frame (include/vpf_hip.h).
static VPF_JB_HDI bool warp_dev_job_ok(int32_t frame, const float* m, uint32_t n_frames) {
  bool ok = (uint32_t)frame < n_frames;
  for (int k = 0; k < 6; k++) ok = ok && fabsf(m[k]) <= 0x1p24f;
  return ok;
}
// The dynamic LDS of a dispatch whose matrices nobody has seen, from the caller's hint `max_step` >= |m00| + |m01|, |m10| + |m11| (source pixels per
// destination pixel step) and |m02| <= W, |m12| <= H: warp_need's bound over every such matrix.  warp_need_count is convex in (|r0|, |r1|) before its
// floor, so over the L1 ball of radius max_step it is largest at a vertex: the rows (max_step, 0) and (0, max_step).  Capped at kWarpStripMax, which
// is also the answer without a hint (max_step == 0).  Never a correctness input: a tile whose strip exceeds the LDS it was given samples per tap
// (warp_strip_tile, k_convert_warp_common.h), with identical bits.
static inline uint32_t warp_dev_lds_bytes(float max_step, uint32_t W, uint32_t H, uint32_t dw, uint32_t dh) {
  if (!(max_step > 0.f)) return kWarpStripMax;
  const double tw = dw < kWarpTileW ? dw : kWarpTileW, th = dh < kWarpTileH ? dh : kWarpTileH;
  const float rx[2][3] = {{max_step, 0.f, (float)W}, {0.f, max_step, (float)W}}, ry[2][3] = {{max_step, 0.f, (float)H}, {0.f, max_step, (float)H}};
  const uint32_t nx0 = warp_need_count(rx[0], W, tw, th, dw, dh), nx1 = warp_need_count(rx[1], W, tw, th, dw, dh);
  const uint32_t ny0 = warp_need_count(ry[0], H, tw, th, dw, dh), ny1 = warp_need_count(ry[1], H, tw, th, dw, dh);
  const uint32_t nx = nx0 > nx1 ? nx0 : nx1, rows = ny0 > ny1 ? ny0 : ny1;
  uint32_t ng = (nx >> 3) + 1;
  const uint32_t ng_max = ((W - 1) >> 3) + 1;
  ng = ng < ng_max ? ng : ng_max;
  const uint64_t bytes = (uint64_t)rows * (32u * ng + 16u);
  return bytes < kWarpStripMax ? (uint32_t)bytes : kWarpStripMax;
}

// ------------------------------------------------------------------------------------------
// Perspective warp (k_convert_persp.hip, vpf_convert_persp_tensor): m = (m00 m01 m02; m10 m11 m12; m20 m21 m22), the warp's tile and strip.
// tests/test_persp_bounds_cpu.py through tests/c/persp_bounds_capi.cpp.
// ------------------------------------------------------------------------------------------
// Coordinates (include/vpf_hip.h): three rounded-affine values, two IEEE divisions, no fma.  `front`: w > 0; a pixel behind the plane or on the
// horizon (!(w > 0)) has no coordinate (sx = sy = 0 here, never used) and takes the border in both modes.  With finite coefficients and w > 0 no
// NaN arises; sx, sy = +-inf are legal: out of range under CONSTANT, the edge under REPLICATE (a max, then a min).
struct PerspXY {
  float sx, sy;
  bool front;
};
static VPF_JB_HDI PerspXY persp_xy(const float* m, uint32_t dx, uint32_t dy, bool rep, float wmax, float hmax) {
  const float fx = (float)dx, fy = (float)dy;
  const float nx = (m[0] * fx + m[1] * fy) + m[2];
  const float ny = (m[3] * fx + m[4] * fy) + m[5];
  const float w = (m[6] * fx + m[7] * fy) + m[8];
  if (!(w > 0.f)) return PerspXY{0.f, 0.f, false};
  float sx = nx / w, sy = ny / w;
  if (rep) {
    sx = fminf(fmaxf(sx, 0.f), wmax);
    sy = fminf(fmaxf(sy, 0.f), hmax);
  }
  return PerspXY{sx, sy, true};
}
// What a destination tile [xs, xe] x [ys, ye] does, from its four corners.  w is rounded-affine, hence monotone in dx for fixed dy and in dy for
// fixed dx, so its sign over the tile is decided at the corners:
//   kPerspTileBorder  no corner has w > 0: no pixel has, the tile is the border
//   kPerspTileTap     some corner has, some has not: the horizon crosses or touches the tile, which samples per tap
//   kPerspTileOut     w > 0 everywhere, the corners' bounding box misses the frame (CONSTANT only): nothing is staged
//   kPerspTileStage   w > 0 everywhere: the window is the corners' bounding box, one pixel wider on every side, cut to the frame
// With w > 0 over the tile its exact image is a convex quadrilateral whose bounding box lies at the corners — but fl(fl(nx) / fl(w)) is a quotient
// of two monotone functions and not monotone itself: with cancellation in nx a pixel's coordinate can lie anywhere.  The window is therefore a guess
// that is nearly always right (the extra pixel per side absorbs ordinary rounding), and persp_px_in_window is the per-pixel test that makes the
// kernel correct for every matrix: an in-range pixel that fails it is sampled per tap (kPerspTileOut: every in-range pixel).
enum { kPerspTileBorder = 0, kPerspTileTap = 1, kPerspTileOut = 2, kPerspTileStage = 3 };
struct PerspWin {
  WarpWin w;  // (w.empty: cls != kPerspTileStage)
  uint32_t cls;
};
static VPF_JB_HDI PerspWin persp_window(const float* m, uint32_t xs, uint32_t xe, uint32_t ys, uint32_t ye, bool rep, uint32_t W, uint32_t H) {
  const float wmax = (float)(W - 1), hmax = (float)(H - 1);
  const PerspXY a = persp_xy(m, xs, ys, rep, wmax, hmax), b = persp_xy(m, xe, ys, rep, wmax, hmax), c = persp_xy(m, xs, ye, rep, wmax, hmax),
                d = persp_xy(m, xe, ye, rep, wmax, hmax);
  PerspWin p{WarpWin{0u, 0u, 0u, 0u, true}, kPerspTileBorder};
  const uint32_t nfront = (uint32_t)a.front + (uint32_t)b.front + (uint32_t)c.front + (uint32_t)d.front;
  if (nfront == 0u) return p;
  p.cls = kPerspTileTap;
  if (nfront != 4u) return p;
  const float xmin = fminf(fminf(a.sx, b.sx), fminf(c.sx, d.sx)), xmax = fmaxf(fmaxf(a.sx, b.sx), fmaxf(c.sx, d.sx));
  const float ymin = fminf(fminf(a.sy, b.sy), fminf(c.sy, d.sy)), ymax = fmaxf(fmaxf(a.sy, b.sy), fmaxf(c.sy, d.sy));
  p.cls = kPerspTileOut;
  if (!(xmax >= 0.f && xmin <= wmax && ymax >= 0.f && ymin <= hmax)) return p;
  p.cls = kPerspTileStage;
  p.w.empty = false;
  const uint32_t xl = (uint32_t)(int)fmaxf(xmin, 0.f), yl = (uint32_t)(int)fmaxf(ymin, 0.f);
  const uint32_t xh = (uint32_t)(int)fminf(xmax, wmax), yh = (uint32_t)(int)fminf(ymax, hmax);
  p.w.x_lo = xl ? xl - 1 : 0u;
  p.w.y_lo = yl ? yl - 1 : 0u;
  p.w.x_hi = xh + 2 < W ? xh + 2 : W - 1;
  p.w.y_hi = yh + 2 < H ? yh + 2 : H - 1;
  return p;
}
// The per-pixel test of the staged kernel, on the taps of an IN-RANGE pixel (xa = floor(sx), ya = floor(sy); the second taps are
// min(xa + 1, W - 1), min(ya + 1, H - 1), the frame's clamp): all four lie in the window the tile staged.
static VPF_JB_HDI bool persp_px_in_window(const WarpWin& w, uint32_t xa, uint32_t ya, uint32_t W, uint32_t H) {
  const uint32_t xb = xa + 1 < W ? xa + 1 : W - 1, yb = ya + 1 < H ? ya + 1 : H - 1;
  return xa >= w.x_lo && xb <= w.x_hi && ya >= w.y_lo && yb <= w.y_hi;
}
// The launcher's LDS bound of a job, O(1).  Jobs with w > 0 at the four DESTINATION corners have w > 0 everywhere (w is affine).
// d sx / d dx = (m00 w - nx m20) / w^2, and the numerator does not depend on dx: it is A dy + B with A = m00 m21 - m20 m01, B = m00 m22 - m20 m02.
// For a fixed dy the quotient is largest where w is smallest, at dx = 0 or dw - 1: along either of those two edges it is |B + A t| / (c + d t)^2 in
// t = dy, whose maximum over [0, dh - 1] lies at an end or at its one stationary point (persp_ratio_max).  Likewise d sx / d dy =
// (D - A dx) / w^2 with D = m01 m22 - m21 m02, along the edges dy = 0 and dh - 1.  A tile of tw x th pixels therefore spans at most
// gx (tw - 1) + gy (th - 1) source pixels along x, gx and gy those two maxima over the whole destination (computed in double: the products of floats
// are exact; every w less the rounding the kernel's fp32 w can carry).  The rounding of a coordinate that lies in the frame (nx's and w's three
// roundings each, the division's; a window is cut to the frame, so only such coordinates bound it) and the window's extra pixel per side come on top.
// Jobs the bound does not cover — some destination corner with !(w > 0) — get kWarpStripMax: their tiles decide for themselves.  No corner with
// w > 0: no tile stages, 0 bytes.  As in the affine entry a tile whose strip exceeds the LDS it was given samples per tap: a short bound costs
// time, never pixels.
// max over t in [0, T] of |a + b t| / (c + d t)^2, c + d t > 0 on the interval
static inline double persp_ratio_max(double a, double b, double c, double d, double T) {
  double best = fmax(fabs(a) / (c * c), fabs(a + b * T) / ((c + d * T) * (c + d * T)));
  if (b * d != 0.0) {
    const double t = (b * c - 2.0 * d * a) / (b * d);  // b (c + d t) = 2 d (a + b t)
    if (t > 0.0 && t < T) best = fmax(best, fabs(a + b * t) / ((c + d * t) * (c + d * t)));
  }
  return best;
}
// gx = max |d s / d dx|, gy = max |d s / d dy| of one coordinate row over the whole destination (r: the matrix row of that axis, r2: the last row,
// werr: what is taken off every w): what persp_need_count multiplies by the tile's sides and what persp_step sums
struct PerspGrad { double gx, gy; };
static inline PerspGrad persp_grad(const float* r, const float* r2, uint32_t dw, uint32_t dh, double werr) {
  const double X = (double)(dw - 1), Y = (double)(dh - 1);
  const double A = (double)r[0] * r2[1] - (double)r2[0] * r[1], B = (double)r[0] * r2[2] - (double)r2[0] * r[2], D = (double)r[1] * r2[2] - (double)r2[1] * r[2];
  const double w00 = (double)r2[2] - werr;
  const double gx = fmax(persp_ratio_max(B, A, w00, r2[1], Y), persp_ratio_max(B, A, w00 + (double)r2[0] * X, r2[1], Y));
  const double gy = fmax(persp_ratio_max(D, -A, w00, r2[0], X), persp_ratio_max(D, -A, w00 + (double)r2[1] * Y, r2[0], X));
  return PerspGrad{gx, gy};
}
// pixels of a tile's window along one axis, at most (S: the frame's size along it, wmin: the smallest w of the destination less werr)
static inline uint32_t persp_need_count(const float* r, const float* r2, uint32_t S, double tw, double th, uint32_t dw, uint32_t dh, double werr, double wmin) {
  const double smax = (double)(S - 1);
  const PerspGrad g = persp_grad(r, r2, dw, dh, werr);
  const double span = g.gx * (tw - 1) + g.gy * (th - 1);
  const double nmag = fabs((double)r[0]) * dw + fabs((double)r[1]) * dh + fabs((double)r[2]);
  const double wmag = fabs((double)r2[0]) * dw + fabs((double)r2[1]) * dh + fabs((double)r2[2]);
  const double err = 4.0 * 0x1p-23 * ((nmag + smax * wmag) / wmin + smax);
  const double n = floor(span + 2.0 * err) + 5.0;
  return n < (double)S ? (uint32_t)n : S;
}
// what persp_need looks at before it bounds anything: the fp32 w of the four destination corners.  `bounded`: all four have w > 0 and the smallest,
// less the rounding, is still positive — the jobs whose gradients persp_grad bounds
struct PerspFront {
  uint32_t nfront;
  double werr, wmin;
  bool bounded;
};
static inline PerspFront persp_front(const float m[9], uint32_t dw, uint32_t dh) {
  const uint32_t cx[4] = {0u, dw - 1, 0u, dw - 1}, cy[4] = {0u, 0u, dh - 1, dh - 1};
  PerspFront f{0u, 0.0, 0.0, false};
  for (int k = 0; k < 4; k++) {
    const float w = (m[6] * (float)cx[k] + m[7] * (float)cy[k]) + m[8];
    if (w > 0.f) {
      f.wmin = !f.nfront || (double)w < f.wmin ? (double)w : f.wmin;
      f.nfront++;
    }
  }
  f.werr = 4.0 * 0x1p-23 * (fabs((double)m[6]) * dw + fabs((double)m[7]) * dh + fabs((double)m[8]));
  f.wmin -= 2.0 * f.werr;  // (the exact w of a corner may lie werr below the fp32 one, and werr is taken off every exact w below)
  f.bounded = f.nfront == 4u && f.wmin > 0.0;
  return f;
}
static inline WarpNeed persp_need(const float m[9], uint32_t W, uint32_t H, uint32_t dw, uint32_t dh) {
  const PerspFront f = persp_front(m, dw, dh);
  if (!f.nfront) return WarpNeed{0u};
  if (!f.bounded) return WarpNeed{kWarpStripMax};
  const double tw = dw < kWarpTileW ? dw : kWarpTileW, th = dh < kWarpTileH ? dh : kWarpTileH;
  const uint32_t nx = persp_need_count(m, m + 6, W, tw, th, dw, dh, f.werr, f.wmin), rows = persp_need_count(m + 3, m + 6, H, tw, th, dw, dh, f.werr, f.wmin);
  uint32_t ng = (nx >> 3) + 1;  // the strip starts on the even pixel at or below x_lo
  const uint32_t ng_max = ((W - 1) >> 3) + 1;
  ng = ng < ng_max ? ng : ng_max;
  const uint64_t bytes = (uint64_t)rows * (32u * ng + 16u);
  return WarpNeed{bytes < 0xffffffffull ? (uint32_t)bytes : 0xffffffffu};
}

// ------------------------------------------------------------------------------------------
// Device-resident homographies (k_convert_persp_dev.hip, vpf_convert_persp_tensor_dev; tests/test_persps_dev_bounds_cpu.py through
// tests/c/persp_dev_bounds_capi.cpp).  The kernel reads (frame, m[9]) of its job from device memory, so the host entry's check of the matrix happens
// in the kernel, and the launcher sizes the LDS without a matrix.
// ------------------------------------------------------------------------------------------
// The guard: the ONLY thing between untrusted device memory and a read outside a frame: warp_dev_job_ok over nine floats.  With every |m| <= 2^24
// and dx, dy <= 65535, nx, ny and w are finite; a pixel with !(w > 0) takes the border, every other one divides two finite numbers by a positive
// one: no NaN, and +-inf is out of range (CONSTANT) or clamped to the edge (REPLICATE), so every tap lies inside the frame (include/vpf_hip.h).
static VPF_JB_HDI bool persp_dev_job_ok(int32_t frame, const float* m, uint32_t n_frames) {
  bool ok = (uint32_t)frame < n_frames;
  for (int k = 0; k < 9; k++) ok = ok && fabsf(m[k]) <= 0x1p24f;
  return ok;
}
// The caller's hint for ONE matrix: the bound, over every destination pixel, of |d sx / d dx| + |d sx / d dy| and of |d sy / d dx| + |d sy / d dy|
// (source pixels per destination pixel step) — max(gx + gy) over the two coordinate rows, gx and gy persp_need_count's.  Rounded up to fp32.  A last
// row (0, 0, 1) gives max(|m00| + |m01|, |m10| + |m11|) / (1 - werr)^2: the affine entry's hint.  0, "no hint", where persp_need has no bound
// either: some destination corner with !(w > 0), or the smallest w not positive after its rounding (and where the bound is no fp32 number).
static inline float persp_step(const float m[9], uint32_t dw, uint32_t dh) {
  const PerspFront f = persp_front(m, dw, dh);
  if (!f.bounded) return 0.f;
  const PerspGrad a = persp_grad(m, m + 6, dw, dh, f.werr), b = persp_grad(m + 3, m + 6, dw, dh, f.werr);
  const double s = fmax(a.gx + a.gy, b.gx + b.gy);
  if (!(s < 3.0e38)) return 0.f;  // (not a float: no hint)
  float r = (float)s;
  if ((double)r < s) r = nextafterf(r, INFINITY);
  return r;
}
// The dynamic LDS of a dispatch whose matrices nobody has seen, from the caller's hint `max_step` >= persp_step of every valid job: the strip of a
// window of floor(max_step * max(tw - 1, th - 1) + slack) + 5 pixels per axis, cut to the frame.  gx (tw - 1) + gy (th - 1) <= (gx + gy) max(tw - 1,
// th - 1), persp_need_count's span; the + 5 is its own.  Its rounding term depends on the matrix (2 err, err = 2^-21 ((nmag + smax wmag) / wmin +
// smax)); here it is the `slack` of matrices of moderate condition, kappa = wmag / wmin <= 8, whose coordinates lie in the frame: nmag / wmin is
// then at most kappa (max_step (dw + dh) + S) — a step of max_step per destination pixel away from an offset inside the frame — so
// slack = 2 * 2^-21 (8 max_step (dw + dh) + 17 S): 0.05 pixels for 1080p into 640 x 640 at a step of 3.  A matrix outside that gets a window that
// may be short by the difference, which costs its tile the per-tap form.  Capped at kWarpStripMax, which is also the answer without a hint
// (max_step == 0).  Never a correctness input: a tile whose strip exceeds the LDS it was given samples per tap (persp_strip_tile,
// k_convert_warp_common.h), with identical bits.
static inline uint32_t persp_dev_lds_count(float max_step, uint32_t S, double tw, double th, uint32_t dw, uint32_t dh) {
  const double side = (tw > th ? tw : th) - 1.0;
  const double slack = 0x1p-20 * (8.0 * (double)max_step * ((double)dw + (double)dh) + 17.0 * (double)S);
  const double n = floor((double)max_step * side + slack) + 5.0;
  return n < (double)S ? (uint32_t)n : S;
}
static inline uint32_t persp_dev_lds_bytes(float max_step, uint32_t W, uint32_t H, uint32_t dw, uint32_t dh) {
  if (!(max_step > 0.f)) return kWarpStripMax;
  const double tw = dw < kWarpTileW ? dw : kWarpTileW, th = dh < kWarpTileH ? dh : kWarpTileH;
  const uint32_t nx = persp_dev_lds_count(max_step, W, tw, th, dw, dh), rows = persp_dev_lds_count(max_step, H, tw, th, dw, dh);
  uint32_t ng = (nx >> 3) + 1;
  const uint32_t ng_max = ((W - 1) >> 3) + 1;
  ng = ng < ng_max ? ng : ng_max;
  const uint64_t bytes = (uint64_t)rows * (32u * ng + 16u);
  return bytes < kWarpStripMax ? (uint32_t)bytes : kWarpStripMax;
}

// ------------------------------------------------------------------------------------------
// Per-pixel remap (k_convert_remap.hip, vpf_convert_remap_tensor): the coordinates are DATA — two floats per destination pixel, loaded from device
// memory nobody has checked — so the tile's window is not estimated from corners: it is the exact merge of what every pixel contributes.
// ------------------------------------------------------------------------------------------
// What ONE pixel with the loaded coordinates (sx, sy) does: `in` — it samples the frame — and then its four taps (x0|x1, y0|y1) and the coordinate
// (cx, cy) the blend takes its fractions from; otherwise it takes the border, taps and coordinate are those of pixel (0, 0) and are never blended.
// The ONLY thing between untrusted floats and an index: a NaN in either coordinate is REPLACED BY A SELECT (no min, max or median is asked what
// it does with a NaN) and the pixel is out of range in both modes; REPLICATE's max-then-min puts +-inf on the edge; CONSTANT's test lets -0.0 in
// and +-inf out; a coordinate that failed the test is replaced by 0 — again a select — BEFORE the float -> int conversion.  So the conversion only
// ever sees values in [0, W - 1] x [0, H - 1] (W, H <= 65536: exact floats), and x0 <= x1 <= W - 1, y0 <= y1 <= H - 1 whatever was loaded.
struct RemapTap {
  float cx, cy;
  uint32_t x0, x1, y0, y1;
  bool in;
};
static VPF_JB_HDI RemapTap remap_tap(float sx, float sy, bool rep, uint32_t W, uint32_t H) {
  const float wmax = (float)(W - 1), hmax = (float)(H - 1);
  const bool nan = sx != sx || sy != sy;
  sx = nan ? 0.f : sx;
  sy = nan ? 0.f : sy;
  if (rep) {  // a max, then a min: warp_xy's
    sx = fminf(fmaxf(sx, 0.f), wmax);
    sy = fminf(fmaxf(sy, 0.f), hmax);
  }
  RemapTap t;
  t.in = !nan && sx >= 0.f && sx <= wmax && sy >= 0.f && sy <= hmax;
  t.cx = t.in ? sx : 0.f;
  t.cy = t.in ? sy : 0.f;
  t.x0 = (uint32_t)(int)t.cx;
  t.y0 = (uint32_t)(int)t.cy;
  t.x1 = t.x0 + 1 < W ? t.x0 + 1 : W - 1;
  t.y1 = t.y0 + 1 < H ? t.y0 + 1 : H - 1;
  return t;
}
// The window of a set of pixels: the smallest rectangle that holds the taps of its in-range pixels; `empty`: it has none (x_lo > x_hi then).
static VPF_JB_HDI WarpWin remap_win_none() { return WarpWin{0xffffffffu, 0u, 0xffffffffu, 0u, true}; }
static VPF_JB_HDI void remap_win_add(WarpWin& w, const RemapTap& t) {
  if (!t.in) return;
  w.x_lo = t.x0 < w.x_lo ? t.x0 : w.x_lo; w.x_hi = t.x1 > w.x_hi ? t.x1 : w.x_hi;
  w.y_lo = t.y0 < w.y_lo ? t.y0 : w.y_lo; w.y_hi = t.y1 > w.y_hi ? t.y1 : w.y_hi;
  w.empty = false;
}
static VPF_JB_HDI WarpWin remap_win_merge(const WarpWin& a, const WarpWin& b) {
  return WarpWin{a.x_lo < b.x_lo ? a.x_lo : b.x_lo, a.x_hi > b.x_hi ? a.x_hi : b.x_hi, a.y_lo < b.y_lo ? a.y_lo : b.y_lo, a.y_hi > b.y_hi ? a.y_hi : b.y_hi,
                 a.empty && b.empty};
}
// whether the strip of a window fits `lds_bytes`: rows x row bytes in 64 bits — a window may be the whole of a 65536 x 65536 frame, whose strip's
// bytes do not fit 32
static VPF_JB_HDI bool remap_strip_fits(const WarpStrip& s, uint32_t lds_bytes) { return (uint64_t)s.rows * s.rowbytes <= (uint64_t)lds_bytes; }

#endif  // VPF_JOB_BOUNDS_H_
