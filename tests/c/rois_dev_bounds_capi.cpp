// tests/c/rois_dev_bounds_capi.cpp — what the device-resident ROI kernel decides for itself (csrc/vpf_job_bounds.h: what k_convert_roi_dev.hip
// includes, on host and device) behind C symbols, for tests/test_rois_dev_bounds_cpu.py.  Compiled with plain g++: no HIP.
#include "vpf_job_bounds.h"

extern "C" {

int rd_box_ok(int32_t frame, int32_t x, int32_t y, int32_t w, int32_t h, uint32_t n_frames, uint32_t W, uint32_t H) {
  return roi_dev_box_ok(frame, x, y, w, h, n_frames, W, H) ? 1 : 0;
}
// many boxes at once: boxes = n rows of five ints
void rd_boxes_ok(const int32_t* boxes, uint32_t n, uint32_t n_frames, uint32_t W, uint32_t H, uint8_t* out) {
  for (uint32_t i = 0; i < n; i++, boxes += 5) out[i] = roi_dev_box_ok(boxes[0], boxes[1], boxes[2], boxes[3], boxes[4], n_frames, W, H) ? 1 : 0;
}

uint32_t rd_lds_bytes(uint32_t dw, uint32_t dh) { return roi_dev_lds_bytes(dw, dh); }

// the job's need as the host entry's launcher computes it (the scale factors are the entry's)
uint32_t rd_job_need(uint32_t x, uint32_t w, uint32_t h, uint32_t dw, uint32_t dh, double* conv) {
  const RoiStripNeed n = roi_strip_need(x, w, h, (float)w / (float)dw, (float)h / (float)dh, dw, dh);
  *conv = n.conv;
  return n.bytes;
}
// every tile of the job, band-major (16 rows x 256 columns): bytes[t], conv[t], staged[t] under `lds_bytes` of dynamic LDS; returns the tile count
uint32_t rd_tiles(uint32_t x, uint32_t w, uint32_t h, uint32_t dw, uint32_t dh, uint32_t lds_bytes, uint32_t* bytes, double* conv, uint8_t* staged) {
  const float scx = (float)w / (float)dw, scy = (float)h / (float)dh;
  uint32_t t = 0;
  for (uint32_t Y0 = 0; Y0 < dh; Y0 += 4 * kRoiBandRows)
    for (uint32_t xs = 0; xs < dw; xs += 256, t++) {
      const uint32_t Y1 = Y0 + 4 * kRoiBandRows - 1 < dh - 1 ? Y0 + 4 * kRoiBandRows - 1 : dh - 1, xe = xs + 255 < dw - 1 ? xs + 255 : dw - 1;
      const RoiStripNeed n = roi_tile_need(x, w, h, scx, scy, xs, xe, Y0, Y1, dw, dh);
      bytes[t] = n.bytes; conv[t] = n.conv; staged[t] = roi_tile_staged(n, lds_bytes) ? 1 : 0;
    }
  return t;
}
// ... and the four values the staged kernels fill their strip from, win[4 * t ..] = first, last (frame pixels), lo, hi (rectangle rows)
uint32_t rd_tile_windows(uint32_t x, uint32_t w, uint32_t h, uint32_t dw, uint32_t dh, uint32_t* win) {
  const float scx = (float)w / (float)dw, scy = (float)h / (float)dh;
  uint32_t t = 0;
  for (uint32_t Y0 = 0; Y0 < dh; Y0 += 4 * kRoiBandRows)
    for (uint32_t xs = 0; xs < dw; xs += 256, t++) {
      const uint32_t Y1 = Y0 + 4 * kRoiBandRows - 1 < dh - 1 ? Y0 + 4 * kRoiBandRows - 1 : dh - 1, xe = xs + 255 < dw - 1 ? xs + 255 : dw - 1;
      const RoiTileWin r = roi_tile_window(x, w, h, scx, scy, xs, xe, Y0, Y1);
      win[4 * t] = r.first; win[4 * t + 1] = r.last; win[4 * t + 2] = r.lo; win[4 * t + 3] = r.hi;
    }
  return t;
}

}  // extern "C"
