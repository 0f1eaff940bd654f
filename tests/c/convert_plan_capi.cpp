// tests/c/convert_plan_capi.cpp — the policy of the convert and relayout launches (csrc/vpf_convert_plan.h: what launch_yuv_to_rgb, launch_rgb_to_yuv,
// launch_tensor_to_yuv and launch_relayout dispatch on) behind C symbols, for tests/test_convert_plan_cpu.py.  Compiled with plain g++: no HIP.
#include "vpf_convert_plan.h"

extern "C" {

int cp_forms(void) { return vpf::CONVERT_FORMS; }
int cp_plan_words(void) { return 24; }
// -> the name the selection log prints; out = {has_one}; targs / args: the words of ConvertFormInfo
const char* cp_form(int form, int* has_one, const char** targs, const char** args) {
  const vpf::ConvertFormInfo& f = vpf::kConvertForms[form];
  *has_one = f.has_one; *targs = f.targs; *args = f.args;
  return f.name;
}

// knobs = {variant, dst_reused, dtype, nv12, nhwc}
// out = {ok, form, one, src, dst, nts, ballast, sub, mode, dtype, nv12, nhwc, gx, gy, gz, na, a[6], swap_src02, swap_dst02}
void cp_plan(int kind, int src, int dst, uint32_t w, uint32_t h, uint32_t n, const uint64_t* src_bits, const uint64_t* dst_bits, const int* knobs, uint32_t* out) {
  vpf::ConvertShape q{};
  q.kind = kind; q.src = src; q.dst = dst; q.w = w; q.h = h; q.n = n;
  for (int k = 0; k < 3; k++) { q.src_bits[k] = src_bits[k]; q.dst_bits[k] = dst_bits[k]; }
  q.variant = knobs[0]; q.dst_reused = knobs[1] != 0; q.dtype = (uint32_t)knobs[2]; q.nv12 = knobs[3] != 0; q.nhwc = knobs[4] != 0;
  const vpf::ConvertPlan P = vpf::convert_plan(q);
  const uint32_t v[24] = {P.ok, (uint32_t)P.form, P.one, (uint32_t)P.src, (uint32_t)P.dst, P.nts, (uint32_t)P.ballast, P.sub, (uint32_t)P.mode, P.dtype, P.nv12, P.nhwc,
                          P.gx, P.gy, P.gz, (uint32_t)P.na, P.a[0], P.a[1], P.a[2], P.a[3], P.a[4], P.a[5], P.swap_src02, P.swap_dst02};
  for (int i = 0; i < 24; i++) out[i] = v[i];
}

}  // extern "C"
