// vpf_aa_plan.h — the antialiased letterbox into a tensor (vpf_convert_letterbox_tensor_aa, launch_convert_letterbox_aa of k_convert_letterbox_aa.hip):
// the arithmetic of the triangle filter, shared VERBATIM by the two kernels and by the test reference (tests/c/aa_ref_capi.cpp), and the launch of a
// job table as one pure function — the refusal, or up to two dispatches (staged, per tap) with grid, tile shape and strip bytes, and which dispatch
// every job goes to.  No HIP in here: the launcher includes it and only dispatches on the result, and tests/test_letterbox_aa_cpu.py compiles the same
// header with g++ -ffp-contract=off.  A sibling of job_plan (vpf_job_plan.h), not a family of it: the window of a tile grows with the scale, so the
// tile shape is part of the decision, which job_plan's families do not have.
//
// The filter (include/vpf_hip.h states it): per axis, `in` source pixels of the rectangle onto `out` pixels of the picture, every operation an
// individually rounded fp32 operation (the library is built with -ffp-contract=off; a division is IEEE-rounded):
//   s = (float)in / (float)out   fs = max(s, 1)   inv = 1 / fs
//   c = ((float)d + 0.5f) * s    lo = max(0, (int)((c - fs) + 0.5f))   hi = min(in, (int)((c + fs) + 0.5f))       taps lo .. hi - 1
//   t_k = max(0, 1 - |((float)k + 0.5f) - c| * inv)              r = 1 / (t_lo + ... + t_(hi-1))   (plain adds, ascending)
// hi > lo and the sum >= 0.5: the pixel nearest c has t >= 0.5.
#pragma once
#include <math.h>
#include <stdint.h>

#include "vpf_classes.h"
#include "vpf_hip.h"
#include "vpf_plan_bounds.h"

#ifdef __HIPCC__
#define VPF_AA_HD __host__ __device__ __forceinline__
#else
#define VPF_AA_HD inline
#endif

namespace vpf {

struct AaAxis {
  float s, fs, inv;
  uint32_t in;
};
struct AaWindow {
  float c;
  uint32_t lo, hi;  // taps lo .. hi - 1 of the rectangle's axis
};
// ... from the scale factor the entry computed, (float)in / (float)out (LetterboxDesc::r.scx / scy)
static VPF_AA_HD AaAxis aa_axis_s(uint32_t in, float s) {
  AaAxis a;
  a.s = s;
  a.fs = s > 1.0f ? s : 1.0f;
  a.inv = 1.0f / a.fs;
  a.in = in;
  return a;
}
static VPF_AA_HD AaAxis aa_axis(uint32_t in, uint32_t out) { return aa_axis_s(in, (float)in / (float)out); }
static VPF_AA_HD AaWindow aa_window(const AaAxis& a, uint32_t d) {
  AaWindow w;
  w.c = ((float)d + 0.5f) * a.s;
  const int lo = (int)((w.c - a.fs) + 0.5f), hi = (int)((w.c + a.fs) + 0.5f);  // (C truncation, then the clamp; c + fs < 2^18)
  w.lo = lo > 0 ? (uint32_t)lo : 0u;
  w.hi = (uint32_t)hi < a.in ? (uint32_t)hi : a.in;
  return w;
}
static VPF_AA_HD float aa_weight(const AaAxis& a, float c, uint32_t k) {
  const float t = 1.0f - fabsf(((float)k + 0.5f) - c) * a.inv;  // (multiply and subtract rounded separately)
  return t > 0.0f ? t : 0.0f;
}
// 1 / the sum of a window's weights
static VPF_AA_HD float aa_norm(const AaAxis& a, const AaWindow& w) {
  float S = 0.0f;
  for (uint32_t k = w.lo; k < w.hi; k++) S += aa_weight(a, w.c, k);
  return 1.0f / S;
}
// One picture pixel (dx, dy): px(i, j, rgb) gives the three bytes of rectangle pixel (i, j) as floats.  Horizontal first, then vertical, no rounding
// to a byte in between; out[ch] = the 8-bit value as a float.
template <class Px>
static VPF_AA_HD void aa_pixel(const AaAxis& ax, const AaAxis& ay, uint32_t dx, uint32_t dy, Px&& px, float out[3]) {
  const AaWindow wx = aa_window(ax, dx), wy = aa_window(ay, dy);
  const float rx = aa_norm(ax, wx), ry = aa_norm(ay, wy);
  float v[3] = {0.0f, 0.0f, 0.0f};
  for (uint32_t j = wy.lo; j < wy.hi; j++) {
    const float ty = aa_weight(ay, wy.c, j);
    float h[3] = {0.0f, 0.0f, 0.0f};
    for (uint32_t i = wx.lo; i < wx.hi; i++) {
      const float tx = aa_weight(ax, wx.c, i);
      float p[3];
      px(i, j, p);
      h[0] = fmaf(tx, p[0], h[0]); h[1] = fmaf(tx, p[1], h[1]); h[2] = fmaf(tx, p[2], h[2]);
    }
    v[0] = fmaf(ty, rx * h[0], v[0]); v[1] = fmaf(ty, rx * h[1], v[1]); v[2] = fmaf(ty, rx * h[2], v[2]);
  }
  for (int ch = 0; ch < 3; ch++) {
    const float u = truncf(ry * v[ch] + 0.5f);
    out[ch] = u < 255.0f ? u : 255.0f;
  }
}

// ------------------------------------------------------------------------------------------
// The launch.  Tile shapes of the staged kernel, of the destination PLANE, 256 lanes each: 64 x 16 with four consecutive pixels of a row per lane,
// 32 x 8 with one.  A tile's source window is at most (TW s_x + 2 fs_x + 2) x (TH s_y + 2 fs_y + 2) pixels, of four bytes each in the strip; the
// strip holds whole conversion units of eight pixels from an even pixel on (strip_fill_window, k_fused_common.h): wy rows of 32 (wx / 8 + 1) bytes.
// A dispatch takes the first shape — the largest — under which the worst window among its jobs fits kAaStripMax; a job whose window fits under
// no shape samples per tap.  64 x 16 reaches about 3.5 x, 32 x 8 about 6.8 x (4K -> 640 x 640 is 6 x); beyond that the window of even one output
// row outgrows the LDS.
// ------------------------------------------------------------------------------------------
constexpr uint32_t kAaStripMax = 64u * 1024u;  // the most a launch may ask for
constexpr int kAaTiles = 2;
static VPF_AA_HD uint32_t aa_tile_w(uint32_t t) { return t == 0 ? 64u : 32u; }
static VPF_AA_HD uint32_t aa_tile_h(uint32_t t) { return t == 0 ? 16u : 8u; }
static VPF_AA_HD uint32_t aa_tile_npx(uint32_t t) { return t == 0 ? 4u : 1u; }  // (tile_w / npx) x tile_h = 256 lanes

// the bound of a tile's window along one axis: `td` picture pixels of the tile (at most the picture's own)
static VPF_AA_HD uint32_t aa_window_bound(const AaAxis& a, uint32_t td, uint32_t out) {
  const uint32_t n = td < out ? td : out;
  const uint32_t b = (uint32_t)((float)n * a.s + 2.0f * a.fs) + 3u;  // (truncation + 1 >= the real bound + 2)
  return b < a.in ? b : a.in;
}
static VPF_AA_HD uint32_t aa_strip_bytes(uint32_t wx, uint32_t wy) { return wy * 32u * (wx / 8u + 1u); }

enum AaForm : int { AA_STRIP = 0, AA_GATHER = 1 };
struct AaGeom {
  uint32_t w, h, iw, ih;  // the rectangle's and the picture's size: the window does not depend on where either lies
};
struct AaShape {
  int src_fc;      // FmtClass of the frames
  bool nhwc;       // FC_TENSOR_NHWC, else FC_TENSOR
  uint32_t dtype;  // TensorEpi::dtype as the caller passes it
  uint32_t dw, dh;
  int variant;     // tuning(VPF_TUNE_NV12_RGB_VARIANT), read once by the caller
  uint32_t n;
  AaGeom g[kLetterboxBatch];  // the first min(n, kLetterboxBatch) are looked at
};
struct AaDispatch {
  int form;         // AaForm
  uint32_t gx, gy;  // the grid, of 256-lane workgroups; z = n
  uint32_t n;       // jobs
  uint32_t tile;    // AA_STRIP: the tile shape
  uint32_t lds;     // AA_STRIP: the strip — the kernel's `lds_bytes` argument and the launch's dynamic LDS; AA_GATHER: 0
};
struct AaPlan {
  bool ok;  // false: refused (hipErrorInvalidValue), nothing is launched
  int nd;   // dispatches in launch order: the staged one first
  AaDispatch d[2];
  uint32_t dmask;                  // destination alignment the vector stores need
  uint8_t which[kLetterboxBatch];  // the dispatch (index into d) of job i; the jobs of a dispatch keep their call order in its table
};

// the strip job g needs under tile shape t
inline uint32_t aa_job_bytes(const AaGeom& g, uint32_t t) {
  const AaAxis ax = aa_axis(g.w, g.iw), ay = aa_axis(g.h, g.ih);
  return aa_strip_bytes(aa_window_bound(ax, aa_tile_w(t), g.iw), aa_window_bound(ay, aa_tile_h(t), g.ih));
}

inline AaPlan aa_plan(const AaShape& q) {
  AaPlan p{};
  if (q.src_fc != FC_NV12 && q.src_fc != FC_YUV420 && q.src_fc != FC_P16) return p;
  if (!q.n || q.n > (uint32_t)kLetterboxBatch || !q.dw || !q.dh || q.dw > 65536u || q.dh > 65536u) return p;
  for (uint32_t i = 0; i < q.n; i++)
    if (!q.g[i].w || !q.g[i].h || !q.g[i].iw || !q.g[i].ih || q.g[i].w > 65536u || q.g[i].h > 65536u || q.g[i].iw > q.dw || q.g[i].ih > q.dh) return p;
  p.ok = true;
  p.dmask = vpf_tensor_dmask(q.nhwc, q.dtype == VPF_TENSOR_F32);
  // VPF_TUNE_NV12_RGB_VARIANT = 9, the any-input generic forms: no strip anywhere, as for the families of job_plan
  const bool all_per_tap = q.variant == 9;
  uint32_t ns = 0, worst[kAaTiles] = {0u, 0u};
  for (uint32_t i = 0; i < q.n; i++) {
    const bool staged = !all_per_tap && aa_job_bytes(q.g[i], kAaTiles - 1) <= kAaStripMax;  // (the smallest shape has the smallest window)
    p.which[i] = !staged;  // (0 = staged for now)
    if (!staged) continue;
    ns++;
    for (int t = 0; t < kAaTiles; t++) {
      const uint32_t b = aa_job_bytes(q.g[i], (uint32_t)t);
      worst[t] = b > worst[t] ? b : worst[t];
    }
  }
  if (ns) {
    uint32_t t = 0;
    while (worst[t] > kAaStripMax) t++;  // (ends: every staged job fits the last shape)
    p.d[p.nd++] = AaDispatch{AA_STRIP, (q.dw + aa_tile_w(t) - 1) / aa_tile_w(t), (q.dh + aa_tile_h(t) - 1) / aa_tile_h(t), ns, t, worst[t]};
  }
  // the per-tap form: k_lb_gather's grid, four rows x 64 lanes x 4 pixels
  if (ns != q.n) p.d[p.nd++] = AaDispatch{AA_GATHER, ((q.dw + 3) / 4 + 63) / 64, (q.dh + 3) / 4, q.n - ns, 0u, 0u};
  if (!ns)  // the per-tap dispatch is the only one: d[0]
    for (uint32_t i = 0; i < q.n; i++) p.which[i] = 0;
  return p;
}

}  // namespace vpf
