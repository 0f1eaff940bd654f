// tests/c/aa_ref_capi.cpp — the reference of the antialiased letterbox (vpf_convert_letterbox_tensor_aa) for tests/test_letterbox_aa_cpu.py and
// tests/test_gpu_letterbox_aa.py: the axis, window and weight functions and the plan of csrc/vpf_aa_plan.h — the header the kernels include —
// behind C symbols, and aa_ref, the definition of include/vpf_hip.h on RGB byte planes.  Compiled with g++ -O2 -ffp-contract=off: no HIP, every
// operation rounded on its own, fmaf = std::fmaf.
#include <cmath>
#include <cstring>

#include "vpf_aa_plan.h"

using namespace vpf;

extern "C" {

// out = (s, fs, inv)
void aa_c_axis(uint32_t in, uint32_t out_n, float* out) {
  const AaAxis a = aa_axis(in, out_n);
  out[0] = a.s; out[1] = a.fs; out[2] = a.inv;
}

// per destination index d < out_n: lo[d], hi[d], S[d] (the plain ascending sum of the weights), c[d]; covered[k] = 1 where source index k has a
// positive weight in at least one window
void aa_c_windows(uint32_t in, uint32_t out_n, uint32_t* lo, uint32_t* hi, float* S, float* c, uint8_t* covered) {
  const AaAxis a = aa_axis(in, out_n);
  std::memset(covered, 0, in);
  for (uint32_t d = 0; d < out_n; d++) {
    const AaWindow w = aa_window(a, d);
    lo[d] = w.lo; hi[d] = w.hi; c[d] = w.c;
    float s = 0.0f;
    for (uint32_t k = w.lo; k < w.hi; k++) {
      const float t = aa_weight(a, w.c, k);
      s += t;
      if (t > 0.0f) covered[k] = 1;
    }
    S[d] = s;
  }
}

uint32_t aa_c_window_bound(uint32_t in, uint32_t out_n, uint32_t td) { return aa_window_bound(aa_axis(in, out_n), td, out_n); }
uint32_t aa_c_strip_bytes(uint32_t wx, uint32_t wy) { return aa_strip_bytes(wx, wy); }
// out = (w, h, npx) of tile shape t
void aa_c_tile(uint32_t t, uint32_t* out) { out[0] = aa_tile_w(t); out[1] = aa_tile_h(t); out[2] = aa_tile_npx(t); }
uint32_t aa_c_tiles(void) { return (uint32_t)kAaTiles; }
uint32_t aa_c_cap(void) { return (uint32_t)kLetterboxBatch; }
uint32_t aa_c_strip_max(void) { return kAaStripMax; }

// geom: n x (w, h, iw, ih).  out = (ok, nd, dmask, then per dispatch: form, gx, gy, n, tile, lds); which: n bytes
void aa_c_plan(int src_fc, int nhwc, uint32_t dtype, uint32_t dw, uint32_t dh, int variant, uint32_t n, const uint32_t* geom, uint32_t* out, uint8_t* which) {
  AaShape q;
  std::memset(&q, 0, sizeof(q));
  q.src_fc = src_fc; q.nhwc = nhwc != 0; q.dtype = dtype; q.dw = dw; q.dh = dh; q.variant = variant; q.n = n;
  for (uint32_t i = 0; i < n && i < (uint32_t)kLetterboxBatch; i++) q.g[i] = AaGeom{geom[4 * i], geom[4 * i + 1], geom[4 * i + 2], geom[4 * i + 3]};
  const AaPlan p = aa_plan(q);
  std::memset(out, 0, 15 * sizeof(uint32_t));
  out[0] = p.ok ? 1u : 0u; out[1] = (uint32_t)p.nd; out[2] = p.dmask;
  for (int k = 0; k < p.nd; k++) {
    uint32_t* o = out + 3 + 6 * k;
    o[0] = (uint32_t)p.d[k].form; o[1] = p.d[k].gx; o[2] = p.d[k].gy; o[3] = p.d[k].n; o[4] = p.d[k].tile; o[5] = p.d[k].lds;
  }
  if (p.ok)
    for (uint32_t i = 0; i < n; i++) which[i] = p.which[i];
}

// rgb: three byte planes of a frame, `pitch` bytes per row; the rectangle (x, y, w, h) -> out: three planes of iw x ih bytes, tight
void aa_ref(const uint8_t* r, const uint8_t* g, const uint8_t* b, uint32_t pitch, uint32_t x, uint32_t y, uint32_t w, uint32_t h, uint32_t iw, uint32_t ih,
            uint8_t* out) {
  const AaAxis ax = aa_axis(w, iw), ay = aa_axis(h, ih);
  for (uint32_t dy = 0; dy < ih; dy++)
    for (uint32_t dx = 0; dx < iw; dx++) {
      float v[3];
      aa_pixel(ax, ay, dx, dy, [&](uint32_t i, uint32_t j, float* p) {
        const size_t at = (size_t)(y + j) * pitch + x + i;
        p[0] = (float)r[at]; p[1] = (float)g[at]; p[2] = (float)b[at];
      }, v);
      for (int ch = 0; ch < 3; ch++) out[((size_t)ch * ih + dy) * iw + dx] = (uint8_t)v[ch];
    }
}

}  // extern "C"
