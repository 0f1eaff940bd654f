// tests/c/letterbox_dev_bounds_capi.cpp — what the device-resident letterbox kernel decides for itself (csrc/vpf_job_bounds.h: what
// k_convert_letterbox_dev.hip includes, on host and device) behind C symbols, for tests/test_letterbox_dev_cpu.py.  Compiled with plain g++: no HIP.
#include "vpf_job_bounds.h"

extern "C" {

// the fit vpf_letterbox_fit and the kernel share (every side >= 1)
void ld_fit(uint32_t w, uint32_t h, uint32_t dw, uint32_t dh, uint32_t out[4]) {
  const LetterboxFit f = letterbox_fit_ints(w, h, dw, dh);
  out[0] = f.ix; out[1] = f.iy; out[2] = f.iw; out[3] = f.ih;
}
// the guard of an explicit placement, many at once: rects = n rows of four ints
void ld_rects_ok(const int32_t* rects, uint32_t n, uint32_t dw, uint32_t dh, uint8_t* out) {
  for (uint32_t i = 0; i < n; i++, rects += 4) out[i] = letterbox_dev_rect_ok(rects[0], rects[1], rects[2], rects[3], dw, dh) ? 1 : 0;
}
uint32_t ld_lds_bytes(uint32_t dw, uint32_t dh) { return roi_dev_lds_bytes(dw, dh); }

// the job's need as the host-table entry's launcher computes it (the scale factors are the entry's)
uint32_t ld_job_need(uint32_t x, uint32_t w, uint32_t h, uint32_t ix, uint32_t iy, uint32_t iw, uint32_t ih, uint32_t dw, uint32_t dh, double* conv) {
  const RoiStripNeed n = letterbox_strip_need(x, w, h, (float)w / (float)iw, (float)h / (float)ih, ix, iy, iw, ih, dw, dh);
  *conv = n.conv;
  return n.bytes;
}
// every tile of the PLANE, band-major (16 rows x 256 columns), as k_lb_dev walks them: meets[t] — the tile shows picture —, and for those bytes[t],
// conv[t] and staged[t] under `lds_bytes` of dynamic LDS (the others: 0); returns the tile count
uint32_t ld_tiles(uint32_t x, uint32_t w, uint32_t h, uint32_t ix, uint32_t iy, uint32_t iw, uint32_t ih, uint32_t dw, uint32_t dh, uint32_t lds_bytes,
                  uint32_t* bytes, double* conv, uint8_t* staged, uint8_t* meets) {
  const float scx = (float)w / (float)iw, scy = (float)h / (float)ih;
  const uint32_t ixe = ix + iw - 1, iye = iy + ih - 1;
  uint32_t t = 0;
  for (uint32_t Y0 = 0; Y0 < dh; Y0 += 4 * kRoiBandRows)
    for (uint32_t xs = 0; xs < dw; xs += 256, t++) {
      const uint32_t Y1 = Y0 + 4 * kRoiBandRows - 1 < dh - 1 ? Y0 + 4 * kRoiBandRows - 1 : dh - 1, xe = xs + 255 < dw - 1 ? xs + 255 : dw - 1;
      meets[t] = !(xs > ixe || xe < ix || Y0 > iye || Y1 < iy);
      bytes[t] = 0; conv[t] = 0.0; staged[t] = 0;
      if (!meets[t]) continue;
      const LetterboxTileWin lw = letterbox_tile_window(x, w, h, scx, scy, ix, iy, iw, ih, xs, xe, Y0, Y1);
      const RoiStripNeed n = letterbox_tile_need_of(lw.w, iw, ih);
      bytes[t] = n.bytes; conv[t] = n.conv; staged[t] = roi_tile_staged(n, lds_bytes) ? 1 : 0;
    }
  return t;
}
// ... and for the tiles that meet the picture the four values the staged kernels fill their strip from, win[4 * t ..] = first, last (frame pixels),
// lo, hi (rectangle rows); the others: 0
uint32_t ld_tile_windows(uint32_t x, uint32_t w, uint32_t h, uint32_t ix, uint32_t iy, uint32_t iw, uint32_t ih, uint32_t dw, uint32_t dh, uint32_t* win) {
  const float scx = (float)w / (float)iw, scy = (float)h / (float)ih;
  const uint32_t ixe = ix + iw - 1, iye = iy + ih - 1;
  uint32_t t = 0;
  for (uint32_t Y0 = 0; Y0 < dh; Y0 += 4 * kRoiBandRows)
    for (uint32_t xs = 0; xs < dw; xs += 256, t++) {
      const uint32_t Y1 = Y0 + 4 * kRoiBandRows - 1 < dh - 1 ? Y0 + 4 * kRoiBandRows - 1 : dh - 1, xe = xs + 255 < dw - 1 ? xs + 255 : dw - 1;
      win[4 * t] = win[4 * t + 1] = win[4 * t + 2] = win[4 * t + 3] = 0;
      if (xs > ixe || xe < ix || Y0 > iye || Y1 < iy) continue;
      const RoiTileWin r = letterbox_tile_window(x, w, h, scx, scy, ix, iy, iw, ih, xs, xe, Y0, Y1).w;
      win[4 * t] = r.first; win[4 * t + 1] = r.last; win[4 * t + 2] = r.lo; win[4 * t + 3] = r.hi;
    }
  return t;
}

}  // extern "C"
