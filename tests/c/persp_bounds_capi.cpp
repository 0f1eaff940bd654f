// tests/c/persp_bounds_capi.cpp — the perspective warp's coordinates, tile classes, windows, per-pixel window test and LDS bound
// (csrc/vpf_job_bounds.h: what k_convert_persp.hip includes, on host and device) behind C symbols, for tests/test_persp_bounds_cpu.py.
// Compiled with plain g++: no HIP.
#include <string.h>

#include "vpf_job_bounds.h"

extern "C" {

uint32_t pb_strip_max(void) { return kWarpStripMax; }
uint32_t pb_tile_w(void) { return kWarpTileW; }
uint32_t pb_tile_h(void) { return kWarpTileH; }

// persp_xy of n destination pixels (dxdy: n pairs); front[i] = w > 0
void pb_xy(const float* m, uint32_t n, const uint32_t* dxdy, int rep, float wmax, float hmax, float* sx, float* sy, uint8_t* front) {
  for (uint32_t i = 0; i < n; i++) {
    const PerspXY s = persp_xy(m, dxdy[2 * i], dxdy[2 * i + 1], rep != 0, wmax, hmax);
    sx[i] = s.sx; sy[i] = s.sy; front[i] = s.front ? 1 : 0;
  }
}

uint32_t pb_need(const float* m, uint32_t W, uint32_t H, uint32_t dw, uint32_t dh) { return persp_need(m, W, H, dw, dh).bytes; }

// every tile of a job as the kernel walks them: ten words per tile — xs, ys, xe, ye, class, x_lo, x_hi, y_lo, y_hi, strip bytes (staged class only)
uint32_t pb_tiles(const float* m, int rep, uint32_t W, uint32_t H, uint32_t dw, uint32_t dh, uint32_t* out, uint32_t max_tiles) {
  uint32_t n = 0;
  for (uint32_t ys = 0; ys < dh; ys += kWarpTileH)
    for (uint32_t xs = 0; xs < dw; xs += kWarpTileW) {
      if (n == max_tiles) return n;
      const uint32_t xe = xs + kWarpTileW - 1 < dw - 1 ? xs + kWarpTileW - 1 : dw - 1, ye = ys + kWarpTileH - 1 < dh - 1 ? ys + kWarpTileH - 1 : dh - 1;
      const PerspWin p = persp_window(m, xs, xe, ys, ye, rep != 0, W, H);
      uint32_t* o = out + 10 * n++;
      o[0] = xs; o[1] = ys; o[2] = xe; o[3] = ye; o[4] = p.cls;
      o[5] = p.w.x_lo; o[6] = p.w.x_hi; o[7] = p.w.y_lo; o[8] = p.w.y_hi;
      o[9] = p.cls == kPerspTileStage ? warp_strip(p.w).bytes : 0u;
    }
  return n;
}

// the kernel's per-pixel test on n first taps (xa, ya) against one window
void pb_px_in_window(uint32_t x_lo, uint32_t x_hi, uint32_t y_lo, uint32_t y_hi, const uint32_t* xa, const uint32_t* ya, uint32_t n, uint32_t W, uint32_t H,
                     uint8_t* out) {
  const WarpWin w{x_lo, x_hi, y_lo, y_hi, false};
  for (uint32_t i = 0; i < n; i++) out[i] = persp_px_in_window(w, xa[i], ya[i], W, H) ? 1 : 0;
}

}  // extern "C"
