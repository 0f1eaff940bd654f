// tests/c/persp_dev_bounds_capi.cpp — what the device-resident perspective kernel decides for itself, what its launcher sizes without a matrix and the
// hint a caller computes (csrc/vpf_job_bounds.h: what k_convert_persp_dev.hip includes, on host and device) behind C symbols, for
// tests/test_persps_dev_bounds_cpu.py and the reach test of tests/test_gpu_persps_dev.py.  Compiled with plain g++: no HIP.
#include <string.h>

#include "vpf_job_bounds.h"

extern "C" {

uint32_t pd_strip_max(void) { return kWarpStripMax; }

// many jobs at once: rows = n rows of ten 32-bit words (frame as int32, then the BIT PATTERNS of the nine floats)
void pd_jobs_ok(const uint32_t* rows, uint32_t n, uint32_t n_frames, uint8_t* out) {
  for (uint32_t i = 0; i < n; i++, rows += 10) {
    int32_t frame;
    float m[9];
    memcpy(&frame, rows, 4);
    memcpy(m, rows + 1, 36);
    out[i] = persp_dev_job_ok(frame, m, n_frames) ? 1 : 0;
  }
}

float pd_step(const float* m, uint32_t dw, uint32_t dh) { return persp_step(m, dw, dh); }
uint32_t pd_need(const float* m, uint32_t W, uint32_t H, uint32_t dw, uint32_t dh) { return persp_need(m, W, H, dw, dh).bytes; }
uint32_t pd_lds_bytes(float max_step, uint32_t W, uint32_t H, uint32_t dw, uint32_t dh) { return persp_dev_lds_bytes(max_step, W, H, dw, dh); }
// the rounding slack persp_need_count takes off every w: what persp_step's answer for a last row (0, 0, 1) may exceed the affine hint by
double pd_werr(const float* m, uint32_t dw, uint32_t dh) { return persp_front(m, dw, dh).werr; }

// every tile of a job as the kernel walks it, with the kernel's own per-pixel test: per class (kPerspTileBorder .. kPerspTileStage) the number of
// tiles in counts[0 .. 3]; counts[4]: staged tiles whose strip exceeds lds_bytes; counts[5]: staged tiles (that fit) with an in-range pixel that
// fails persp_px_in_window.  Returns the largest staged strip.
uint32_t pd_walk(const float* m, int rep, uint32_t W, uint32_t H, uint32_t dw, uint32_t dh, uint32_t lds_bytes, uint32_t* counts) {
  uint32_t most = 0;
  const float wmax = (float)(W - 1), hmax = (float)(H - 1);
  for (uint32_t ys = 0; ys < dh; ys += kWarpTileH)
    for (uint32_t xs = 0; xs < dw; xs += kWarpTileW) {
      const uint32_t xe = xs + kWarpTileW - 1 < dw - 1 ? xs + kWarpTileW - 1 : dw - 1, ye = ys + kWarpTileH - 1 < dh - 1 ? ys + kWarpTileH - 1 : dh - 1;
      const PerspWin p = persp_window(m, xs, xe, ys, ye, rep != 0, W, H);
      counts[p.cls]++;
      if (p.cls != kPerspTileStage) continue;
      const uint32_t b = warp_strip(p.w).bytes;
      most = b > most ? b : most;
      if (b > lds_bytes) { counts[4]++; continue; }
      bool flagged = false;
      for (uint32_t y = ys; y <= ye && !flagged; y++)
        for (uint32_t x = xs; x <= xe && !flagged; x++) {
          const PerspXY s = persp_xy(m, x, y, rep != 0, wmax, hmax);
          if (!(s.front && s.sx >= 0.f && s.sx <= wmax && s.sy >= 0.f && s.sy <= hmax)) continue;
          flagged = !persp_px_in_window(p.w, (uint32_t)(int)s.sx, (uint32_t)(int)s.sy, W, H);
        }
      counts[5] += flagged;
    }
  return most;
}

}  // extern "C"
