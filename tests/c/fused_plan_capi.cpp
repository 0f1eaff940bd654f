// tests/c/fused_plan_capi.cpp — the policy of the whole-frame fused launch (csrc/vpf_fused_plan.h: what launch_convert_resize of
// k_convert_resize.hip dispatches on) behind C symbols, for tests/test_fused_plan_cpu.py.  Compiled with plain g++: no HIP.  Built once more with
// -DVPF_LAB_FORMS for the lab library's extra family.
#include "vpf_fused_plan.h"

extern "C" {

int fp_small_batch(void) { return vpf::kSmallBatch; }
int fp_max_batch(void) { return vpf::kMaxBatch; }

// out = {family, r, table, gx, gy, gz, lds, stage_npx, vec_ok, chunks, tasks, rowq}
void fp_plan(int src_fc, int dst_fc, int has_epilogue, uint32_t dtype, uint32_t sw, uint32_t sh, uint32_t dw, uint32_t dh, uint32_t n, int variant,
             uint64_t src_bits, uint64_t dst_bits, uint32_t* out) {
  const vpf::FusedShape q{src_fc, dst_fc, has_epilogue != 0, dtype, sw, sh, dw, dh, n, variant, src_bits, dst_bits};
  const vpf::FusedPlan p = vpf::fused_plan(q);
  const uint32_t v[12] = {(uint32_t)p.family, (uint32_t)p.r, (uint32_t)p.table, p.gx, p.gy, p.gz, p.lds, p.stage_npx, (uint32_t)p.vec_ok, p.chunks, p.tasks, p.rowq};
  for (int i = 0; i < 12; i++) out[i] = v[i];
}

// the two bounds the strip's LDS is made of, with the scale factors as the launcher forms them
uint32_t fp_band_rows_exact(int r, uint32_t sh, uint32_t dh) { return vpf_band_rows_exact(r, sh, dh, (float)sh / (float)dh); }
uint32_t fp_fused_rowbytes4(uint32_t sw, uint32_t dw) { return vpf_bound_fused_rowbytes4((float)sw / (float)dw); }

}  // extern "C"
