// tests/c/job_bounds_capi.cpp — the strip sizing of the per-job kernels (csrc/vpf_job_bounds.h: what k_convert_roi.hip and k_convert_warp.hip
// include) behind C symbols, for tests/test_job_bounds_cpu.py.  Compiled with plain g++: no HIP.
#include "vpf_job_bounds.h"

extern "C" {

uint32_t jb_roi_strip_max(void) { return kRoiStripMax; }
double jb_roi_conv_max(void) { return kRoiConvMax; }
uint32_t jb_warp_strip_max(void) { return kWarpStripMax; }
uint32_t jb_warp_tile_w(void) { return kWarpTileW; }
uint32_t jb_warp_tile_h(void) { return kWarpTileH; }

// rectangle (x, .., w, h) -> dw x dh with the entry's scale factors; returns the strip bytes, *conv the converted pixels per destination
// pixel, *staged the policy's decision
uint32_t jb_roi_strip_need(uint32_t x, uint32_t w, uint32_t h, uint32_t dw, uint32_t dh, double* conv, int* staged) {
  const RoiStripNeed n = roi_strip_need(x, w, h, (float)w / (float)dw, (float)h / (float)dh, dw, dh);
  *conv = n.conv;
  *staged = roi_job_staged(n) ? 1 : 0;
  return n.bytes;
}

// out = {x_lo, x_hi, y_lo, y_hi, empty, base_px, ng, rowbytes, rows, bytes} (the last five only where the window is not empty)
void jb_warp_tile(const float* m, uint32_t xs, uint32_t xe, uint32_t ys, uint32_t ye, int rep, uint32_t W, uint32_t H, uint32_t* out) {
  const WarpWin w = warp_window(m, xs, xe, ys, ye, rep != 0, W, H);
  out[0] = w.x_lo; out[1] = w.x_hi; out[2] = w.y_lo; out[3] = w.y_hi; out[4] = w.empty ? 1u : 0u;
  for (int i = 5; i < 10; i++) out[i] = 0u;
  if (w.empty) return;
  const WarpStrip s = warp_strip(w);
  out[5] = s.base_px; out[6] = s.ng; out[7] = s.rowbytes; out[8] = s.rows; out[9] = s.bytes;
}
// every tile of a dw x dh destination, tile-row major: out[10 * tile ..] as jb_warp_tile writes it
void jb_warp_tiles(const float* m, int rep, uint32_t W, uint32_t H, uint32_t dw, uint32_t dh, uint32_t* out) {
  for (uint32_t ys = 0; ys < dh; ys += kWarpTileH)
    for (uint32_t xs = 0; xs < dw; xs += kWarpTileW, out += 10) {
      const uint32_t xe = xs + kWarpTileW - 1 < dw - 1 ? xs + kWarpTileW - 1 : dw - 1, ye = ys + kWarpTileH - 1 < dh - 1 ? ys + kWarpTileH - 1 : dh - 1;
      jb_warp_tile(m, xs, xe, ys, ye, rep, W, H, out);
    }
}
void jb_warp_xy(const float* m, uint32_t dx, uint32_t dy, int rep, uint32_t W, uint32_t H, float* out) {
  const WarpXY s = warp_xy(m, dx, dy, rep != 0, (float)(W - 1), (float)(H - 1));
  out[0] = s.sx; out[1] = s.sy;
}
uint32_t jb_warp_need(const float* m, uint32_t W, uint32_t H, uint32_t dw, uint32_t dh) { return warp_need(m, W, H, dw, dh).bytes; }

}  // extern "C"
