// tests/c/warp_dev_bounds_capi.cpp — what the device-resident warp kernel decides for itself and what its launcher sizes without a matrix
// (csrc/vpf_job_bounds.h: what k_convert_warp_dev.hip includes, on host and device) behind C symbols, for tests/test_warps_dev_bounds_cpu.py.
// Compiled with plain g++: no HIP.
#include <string.h>

#include "vpf_job_bounds.h"

extern "C" {

uint32_t wd_strip_max(void) { return kWarpStripMax; }

// many jobs at once: rows = n rows of seven 32-bit words (frame as int32, then the BIT PATTERNS of the six floats)
void wd_jobs_ok(const uint32_t* rows, uint32_t n, uint32_t n_frames, uint8_t* out) {
  for (uint32_t i = 0; i < n; i++, rows += 7) {
    int32_t frame;
    float m[6];
    memcpy(&frame, rows, 4);
    memcpy(m, rows + 1, 24);
    out[i] = warp_dev_job_ok(frame, m, n_frames) ? 1 : 0;
  }
}

uint32_t wd_lds_bytes(float max_step, uint32_t W, uint32_t H, uint32_t dw, uint32_t dh) { return warp_dev_lds_bytes(max_step, W, H, dw, dh); }

// the largest strip any tile of the job computes for itself (what the kernel compares with the LDS it was given); 0: every window is empty
uint32_t wd_largest_tile(const float* m, int rep, uint32_t W, uint32_t H, uint32_t dw, uint32_t dh) {
  uint32_t most = 0;
  for (uint32_t ys = 0; ys < dh; ys += kWarpTileH)
    for (uint32_t xs = 0; xs < dw; xs += kWarpTileW) {
      const uint32_t xe = xs + kWarpTileW - 1 < dw - 1 ? xs + kWarpTileW - 1 : dw - 1, ye = ys + kWarpTileH - 1 < dh - 1 ? ys + kWarpTileH - 1 : dh - 1;
      const WarpWin w = warp_window(m, xs, xe, ys, ye, rep != 0, W, H);
      if (w.empty) continue;
      const uint32_t b = warp_strip(w).bytes;
      most = b > most ? b : most;
    }
  return most;
}

}  // extern "C"
