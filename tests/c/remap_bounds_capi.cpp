// tests/c/remap_bounds_capi.cpp — what the per-pixel remap kernel computes from the coordinates it loads and what its launcher decides without
// seeing one (csrc/vpf_job_bounds.h and csrc/vpf_remap_plan.h: what k_convert_remap.hip includes, on host and device) behind C symbols, for
// tests/test_remap_tensor_cpu.py.  Compiled with plain g++: no HIP.
#include <string.h>

#include "vpf_job_bounds.h"
#include "vpf_remap_plan.h"

extern "C" {

// n pixels at once: out[i] = (in, x0, x1, y0, y1) of remap_tap, cxy[i] = (cx, cy)
void rm_taps(const float* sx, const float* sy, uint32_t n, int rep, uint32_t W, uint32_t H, uint32_t* out, float* cxy) {
  for (uint32_t i = 0; i < n; i++) {
    const RemapTap t = remap_tap(sx[i], sy[i], rep != 0, W, H);
    out[5 * i] = t.in ? 1u : 0u;
    out[5 * i + 1] = t.x0; out[5 * i + 2] = t.x1; out[5 * i + 3] = t.y0; out[5 * i + 4] = t.y1;
    cxy[2 * i] = t.cx; cxy[2 * i + 1] = t.cy;
  }
}

// The window of one destination tile [xs, xe] x [ys, ye] of maps with `pitch` floats per row, merged the way the workgroup merges it: every lane's
// four pixels into a window of its own (remap_win_add), the lanes of a wave and then the four waves by remap_win_merge.
// out = (empty, x_lo, x_hi, y_lo, y_hi, strip bytes as 64 bits: low, high)
void rm_tile_window(const float* xmap, const float* ymap, uint32_t pitch, uint32_t dw, uint32_t dh, uint32_t bx, uint32_t by, int rep, uint32_t W, uint32_t H,
                    uint32_t* out) {
  WarpWin wave[4];
  for (uint32_t wv = 0; wv < 4; wv++) {
    wave[wv] = remap_win_none();
    for (uint32_t lane = 0; lane < 64; lane++) {
      const uint32_t tid = 64 * wv + lane;
      const uint32_t x0 = bx * kWarpTileW + (tid % kWarpLanesX) * 4, y = by * kWarpTileH + tid / kWarpLanesX;
      WarpWin lw = remap_win_none();
      if (x0 < dw && y < dh)
        for (uint32_t k = 0; k < 4 && x0 + k < dw; k++)
          remap_win_add(lw, remap_tap(xmap[(size_t)y * pitch + x0 + k], ymap[(size_t)y * pitch + x0 + k], rep != 0, W, H));
      wave[wv] = remap_win_merge(wave[wv], lw);
    }
  }
  const WarpWin w = remap_win_merge(remap_win_merge(wave[0], wave[1]), remap_win_merge(wave[2], wave[3]));
  out[0] = w.empty ? 1u : 0u;
  out[1] = w.x_lo; out[2] = w.x_hi; out[3] = w.y_lo; out[4] = w.y_hi;
  out[5] = out[6] = 0u;
  if (!w.empty) {
    const WarpStrip s = warp_strip(w);
    const uint64_t bytes = (uint64_t)s.rows * s.rowbytes;
    out[5] = (uint32_t)bytes; out[6] = (uint32_t)(bytes >> 32);
  }
}

int rm_strip_fits(uint32_t x_lo, uint32_t x_hi, uint32_t y_lo, uint32_t y_hi, uint32_t lds_bytes) {
  const WarpWin w{x_lo, x_hi, y_lo, y_hi, false};
  return remap_strip_fits(warp_strip(w), lds_bytes) ? 1 : 0;
}

// out = (ok, gx, gy, per, lds, dmask)
void rm_plan(int src_fc, int nhwc, uint32_t dtype, uint32_t W, uint32_t H, uint32_t dw, uint32_t dh, float max_step, int variant, uint32_t* out) {
  const vpf::RemapPlan p = vpf::remap_plan(src_fc, nhwc != 0, dtype, W, H, dw, dh, max_step, variant);
  out[0] = p.ok ? 1u : 0u;
  out[1] = p.gx; out[2] = p.gy; out[3] = p.per; out[4] = p.lds; out[5] = p.dmask;
}

uint32_t rm_warp_dev_lds_bytes(float max_step, uint32_t W, uint32_t H, uint32_t dw, uint32_t dh) { return warp_dev_lds_bytes(max_step, W, H, dw, dh); }

}  // extern "C"
