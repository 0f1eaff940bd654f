// tests/c/resize_plan_capi.cpp — the policy of the plain resize launches (csrc/vpf_resize_plan.h: what launch_resize_planned of k_resize.hip
// dispatches on) behind C symbols, for tests/test_resize_plan_cpu.py.  Compiled with plain g++: no HIP.  (The plan is the same under
// -DVPF_LAB_FORMS: the lab build's persistent launch decodes its knob bits at its dispatch.)
#include "vpf_lzm_plan.h"
#include "vpf_resize_plan.h"

#include <cstring>

extern "C" {

int rp_small_batch(void) { return vpf::kSmallBatch; }
int rp_max_batch(void) { return vpf::kMaxBatch; }
int rp_launch_words(void) { return 22; }

static uint32_t fbits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
static void put_launch(const vpf::ResizeLaunch& l, uint32_t* o) {
  const uint32_t v[22] = {(uint32_t)l.family, (uint32_t)l.fallback, (uint32_t)l.eff, (uint32_t)l.it, (uint32_t)l.rows, (uint32_t)l.p1, l.narrow, l.multi, (uint32_t)l.wpb, l.lz,
                          l.gx, l.gy, l.gz, l.threads, l.lds, fbits(l.scx), fbits(l.scy), (uint32_t)l.vec_ok, l.a0, l.a1, l.a2, l.a3};
  for (int i = 0; i < 22; i++) o[i] = v[i];
}

// jobs: njobs x {ch, k, sw, sh, dw, dh}; knobs: {variant, tile, band, mfma}
// out = {ok, single, all, lz_tile_all_first, lz_mfma_all, lz_tile_all_fallback, by0[3]} + 22 words each for mp, plane[0..2]
void rp_plan(int f32, int interp, int njobs, uint32_t n, uint32_t call_n, const uint32_t* jobs, const uint64_t* src_bits, const uint64_t* dst_bits, const int* knobs, uint32_t* out) {
  vpf::ResizeShape q{};
  q.f32 = f32 != 0; q.interp = interp; q.njobs = njobs; q.n = n; q.call_n = call_n;
  for (int p = 0; p < njobs && p < 3; p++) {
    q.jobs[p] = vpf::ResizeJob{(int)jobs[6 * p], (int)jobs[6 * p + 1], jobs[6 * p + 2], jobs[6 * p + 3], jobs[6 * p + 4], jobs[6 * p + 5]};
    q.src_bits[p] = src_bits[p]; q.dst_bits[p] = dst_bits[p];
  }
  q.variant = knobs[0]; q.tile = knobs[1]; q.band = knobs[2]; q.mfma = knobs[3];
  const vpf::ResizePlan P = vpf::resize_plan(q);
  const uint32_t head[9] = {P.ok, P.single, P.all, P.lz_tile_all_first, P.lz_mfma_all, P.lz_tile_all_fallback, P.by0[0], P.by0[1], P.by0[2]};
  for (int i = 0; i < 9; i++) out[i] = head[i];
  put_launch(P.mp, out + 9);
  for (int p = 0; p < 3; p++) put_launch(P.plane[p], out + 9 + 22 * (p + 1));
}

// what launch_lanczos_mfma (k_lanczos_mfma.hip) does with `njobs` planes of n frames: lzm_launch of vpf_lzm_plan.h for the product build.  bits, pitches:
// per plane the OR of pointer | pitch on both sides and {source, destination} pitch of the frames (all frames alike) -> the form's name, nullptr = declined
const char* rp_lzm_form(int njobs, const uint32_t* jobs, const uint64_t* bits, const uint32_t* pitches, uint32_t n, int variant, int mfma) {
  vpf::LzmPlaneIn in[3] = {};
  vpf::LzmFramesIn fr[3] = {};
  for (int p = 0; p < njobs && p < 3; p++) {
    in[p] = vpf::LzmPlaneIn{(int)jobs[6 * p], jobs[6 * p + 2], jobs[6 * p + 3], jobs[6 * p + 4], jobs[6 * p + 5]};
    fr[p] = vpf::LzmFramesIn{bits[p], pitches[2 * p], pitches[2 * p + 1]};
  }
  const vpf::LzmLaunch L = vpf::lzm_launch(njobs, in, fr, n, variant, mfma, false);
  return L.ok() ? vpf::kLzmForms[L.form].name : nullptr;
}

// out = {ok, ty, nr, lds, rowq, lshift, wpb}
void rp_plan_tile(int forced, int lz, int np, const uint32_t* jobs, uint32_t frames, int elem, uint32_t* out) {
  vpf::ResizeJob j[3];
  for (int p = 0; p < np && p < 3; p++) j[p] = vpf::ResizeJob{(int)jobs[6 * p], (int)jobs[6 * p + 1], jobs[6 * p + 2], jobs[6 * p + 3], jobs[6 * p + 4], jobs[6 * p + 5]};
  const vpf::TileShape t = vpf::plan_tile(forced, lz != 0, np, j, frames, elem);
  const uint32_t v[7] = {t.ok, t.ty, t.nr, t.lds, t.rowq, t.lshift, (uint32_t)t.wpb};
  for (int i = 0; i < 7; i++) out[i] = v[i];
}

// the bounds the band and row-pair LDS is made of, with the scale factors as the plan forms them
uint32_t rp_band_slots(int r, uint32_t sh, uint32_t dh) { return vpf_bound_band_slots(r, (float)sh / (float)dh); }
uint32_t rp_band_rows_exact(int r, uint32_t sh, uint32_t dh) { return vpf_band_rows_exact(r, sh, dh, (float)sh / (float)dh); }
uint32_t rp_strip_bytes(int ch, uint32_t sw, uint32_t dw, uint32_t cols) { return vpf_bound_strip_bytes(ch, sw, dw, vpf::kResizeRowBytes, cols); }
uint32_t rp_strip_bytes_px4(uint32_t sw, uint32_t dw) { return vpf_bound_strip_bytes_px4(sw, dw, 1024u, 256u); }
int rp_band_px(int ch, int p1) { return vpf::band_px(ch, p1); }

}  // extern "C"
