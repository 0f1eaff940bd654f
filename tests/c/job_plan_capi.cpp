// tests/c/job_plan_capi.cpp — the policy of the eight per-job tensor launches (csrc/vpf_job_plan.h: what launch_convert_resize_rois,
// launch_convert_letterbox, launch_convert_warp, launch_convert_persp and their _dev forms dispatch on) behind C symbols, for
// tests/test_job_plan_cpu.py.  Compiled with plain g++: no HIP.
#include <string.h>

#include "vpf_job_plan.h"

extern "C" {

int jp_forms(void) { return vpf::JOB_FORMS; }
const char* jp_form(int form, const char** args) {
  *args = vpf::kJobForms[form].args;
  return vpf::kJobForms[form].name;
}
// {the four caps, the largest, max_n's limit, n_frames' limit, kRoiStripMax, kWarpStripMax}
void jp_limits(uint32_t* out) {
  for (int f = 0; f < 4; f++) out[f] = vpf::kJobTableCap[f];
  out[4] = vpf::kJobTableMax; out[5] = vpf::kJobDevMax; out[6] = (uint32_t)vpf::kRoiDevFrames; out[7] = kRoiStripMax; out[8] = kWarpStripMax;
}
double jp_roi_conv_max(void) { return kRoiConvMax; }

// the bound functions of vpf_job_bounds.h the sweep compares the plan with
// geom: nine 32-bit words per job — ROI {x, w, h, scx, scy}, letterbox {.., ix, iy, iw, ih}, warp m[6], perspective m[9] (floats as their bits)
static vpf::JobGeom geom_of(int family, const uint32_t* v) {
  vpf::JobGeom g{};
  if (family == vpf::JOB_ROI || family == vpf::JOB_LETTERBOX) {
    g.x = v[0]; g.w = v[1]; g.h = v[2];
    memcpy(&g.scx, v + 3, 4); memcpy(&g.scy, v + 4, 4);
    g.ix = v[5]; g.iy = v[6]; g.iw = v[7]; g.ih = v[8];
  } else {
    memcpy(g.m, v, 36);
  }
  return g;
}
// -> the bytes of the job's strip; *conv: ROI / letterbox converted pixels per pixel (0 for the warps)
uint32_t jp_job_need(int family, const uint32_t* v, uint32_t W, uint32_t H, uint32_t dw, uint32_t dh, double* conv) {
  const vpf::JobGeom g = geom_of(family, v);
  *conv = 0.0;
  if (family == vpf::JOB_ROI || family == vpf::JOB_LETTERBOX) {
    const RoiStripNeed need = family == vpf::JOB_ROI ? roi_strip_need(g.x, g.w, g.h, g.scx, g.scy, dw, dh)
                                                     : letterbox_strip_need(g.x, g.w, g.h, g.scx, g.scy, g.ix, g.iy, g.iw, g.ih, dw, dh);
    *conv = need.conv;
    return need.bytes;
  }
  return family == vpf::JOB_WARP ? warp_need(g.m, W, H, dw, dh).bytes : persp_need(g.m, W, H, dw, dh).bytes;
}
uint32_t jp_dev_bytes(int family, float max_step, uint32_t W, uint32_t H, uint32_t dw, uint32_t dh) {
  if (family == vpf::JOB_ROI || family == vpf::JOB_LETTERBOX) return roi_dev_lds_bytes(dw, dh);
  return family == vpf::JOB_WARP ? warp_dev_lds_bytes(max_step, W, H, dw, dh) : persp_dev_lds_bytes(max_step, W, H, dw, dh);
}
uint32_t jp_tensor_dmask(int nhwc, int f32) { return vpf_tensor_dmask(nhwc, f32); }

// head = {family, dev, src_fc, nhwc, dtype, W, H, dw, dh, variant, n, max_n, n_frames}; geom: 9 words per job (n of them; none for a device table)
// out = {ok, nd, dmask, d[0]: form gx gy n lds stage_npx, d[1]: the same}; which: n bytes
void jp_plan(const uint32_t* head, float max_step, const uint32_t* geom, uint32_t* out, uint8_t* which) {
  static thread_local vpf::JobShape q;
  q.family = (int)head[0]; q.dev = head[1] != 0; q.src_fc = (int)head[2]; q.nhwc = head[3] != 0; q.dtype = head[4];
  q.W = head[5]; q.H = head[6]; q.dw = head[7]; q.dh = head[8]; q.variant = (int)head[9];
  q.n = head[10]; q.max_n = head[11]; q.n_frames = head[12]; q.max_step = max_step;
  if (!q.dev && q.family >= 0 && q.family < vpf::JOB_FAMILIES)
    for (uint32_t i = 0; i < q.n && i < vpf::kJobTableMax; i++) q.g[i] = geom_of(q.family, geom + 9 * i);
  const vpf::JobPlan p = vpf::job_plan(q);
  out[0] = p.ok; out[1] = (uint32_t)p.nd; out[2] = p.dmask;
  for (int k = 0; k < 2; k++) {
    const vpf::JobDispatch& d = p.d[k];
    const uint32_t v[6] = {(uint32_t)d.form, d.gx, d.gy, d.n, d.lds, d.stage_npx};
    for (int i = 0; i < 6; i++) out[3 + 6 * k + i] = v[i];
  }
  for (uint32_t i = 0; i < q.n && i < vpf::kJobTableMax; i++) which[i] = p.which[i];
}

}  // extern "C"
