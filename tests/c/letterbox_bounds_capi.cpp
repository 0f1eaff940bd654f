// tests/c/letterbox_bounds_capi.cpp — the strip sizing of the letterbox kernels (letterbox_strip_need of csrc/vpf_job_bounds.h: what
// k_convert_letterbox.hip includes) behind C symbols, for tests/test_letterbox_bounds_cpu.py.  Compiled with plain g++: no HIP.
#include "vpf_job_bounds.h"

extern "C" {

// rectangle (x, .., w, h) -> the picture (ix, iy, iw, ih) inside dw x dh with the entry's scale factors ((float)w / (float)iw); returns the strip
// bytes, *conv the converted pixels per picture pixel of a tile, *staged the policy's decision
uint32_t lb_strip_need(uint32_t x, uint32_t w, uint32_t h, uint32_t ix, uint32_t iy, uint32_t iw, uint32_t ih, uint32_t dw, uint32_t dh, double* conv,
                       int* staged) {
  const RoiStripNeed n = letterbox_strip_need(x, w, h, (float)w / (float)iw, (float)h / (float)ih, ix, iy, iw, ih, dw, dh);
  *conv = n.conv;
  *staged = roi_job_staged(n) ? 1 : 0;
  return n.bytes;
}
// the ROI kernels' bound for the same rectangle -> dw x dh (the letterbox bound with the picture = the whole destination must equal it)
uint32_t lb_roi_strip_need(uint32_t x, uint32_t w, uint32_t h, uint32_t dw, uint32_t dh, double* conv) {
  const RoiStripNeed n = roi_strip_need(x, w, h, (float)w / (float)dw, (float)h / (float)dh, dw, dh);
  *conv = n.conv;
  return n.bytes;
}

}  // extern "C"
