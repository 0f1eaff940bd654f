// k_fused_common.h — what the fused translation units (k_convert_resize.hip, k_convert_roi.hip, k_convert_warp.hip) share: the per-texel conversion,
// the planar-tensor store epilogue, the 8-pixel conversion unit of the workgroup-shared RGB strips and the fill stage of the per-job strips (strip_fill_window).
#ifndef VPF_K_FUSED_COMMON_H_
#define VPF_K_FUSED_COMMON_H_
#include "k_bilinear_blend.h"

namespace vpf {

// loads of any alignment: a rectangle starts at an arbitrary byte of an arbitrarily aligned plane (the backend keeps them one
// global_load_dword / _dwordx2 / _dwordx4: gfx950 global memory takes unaligned addresses)
typedef u32x2 u32x2_any __attribute__((aligned(1)));
typedef uint32_t u32_any __attribute__((aligned(1)));
typedef u32x4 u32x4_any __attribute__((aligned(1)));  // (FC_P16 rows: always 2-B aligned, vpf_abi.hip)

// ------------------------------------------------------------------------------------------
// (Stores: plain here — non-temporal stores measured 1.44 -> 1.61 us per 4K -> 720p frame in the batched fused kernel,
// while the unfused resize kernels gain from them on large outputs: 1080p -> 4K 16.0 -> 13.8 us.)
// fused NV12 / YUV420 -> bilinear -> RGB / BGR / RGB_PLANAR.  Defined as convert-then-resize: each of
// the four source texels is converted to 8-bit RGB with exactly vpf_convert's arithmetic (including
// its rounding), then interpolated — bit-identical to running the two kernels back to back, but the
// 3 B/px intermediate never exists: 12.4 MB read + 2.8 MB written instead of 65 MB for 4K -> 720p.
// ------------------------------------------------------------------------------------------
// FC_P16 (P10 / P12): one 2-B load for Y, one 4-B load for the U V pair (2-B aligned), both narrowed to 8 bits (p16_to_8) — then the same chain.
template <int SRC>
VPF_DEV void texel_rgb(const FrameDesc& f, const Yuv2RgbCoef& c, uint32_t x, uint32_t y, float* rgb) {
  float yf, u, v;
  if constexpr (SRC == FC_P16) {
    yf = (float)p16_to_8(*reinterpret_cast<const uint16_t*>(f.s[0] + (size_t)y * f.sp[0] + 2 * (size_t)x));
    const uint32_t d = *reinterpret_cast<const u32_any*>(f.s[1] + (size_t)(y >> 1) * f.sp[1] + 4 * (size_t)(x >> 1));
    u = (float)p16_to_8((uint16_t)(d & 0xffffu)); v = (float)p16_to_8((uint16_t)(d >> 16));
  } else {
    yf = (float)f.s[0][(size_t)y * f.sp[0] + x];
    if constexpr (SRC == FC_NV12) {
      const uint8_t* p = f.s[1] + (size_t)(y >> 1) * f.sp[1] + 2 * (x >> 1);
      u = p[0]; v = p[1];
    } else {
      u = f.s[1][(size_t)(y >> 1) * f.sp[1] + (x >> 1)]; v = f.s[2][(size_t)(y >> 1) * f.sp[2] + (x >> 1)];
    }
  }
  const Chroma k = chroma_terms(c, u, v);
  rgb[0] = (float)sat_rne(__builtin_fmaf(yf, c.cy, k.rc));
  rgb[1] = (float)sat_rne(__builtin_fmaf(yf, c.cy, k.gc));
  rgb[2] = (float)sat_rne(__builtin_fmaf(yf, c.cy, k.bc));
}

// ------------------------------------------------------------------------------------------
// The planar-tensor destination (FC_TENSOR, vpf_convert_resize_tensor): the store epilogue of every fused family.  Each family hands over
// the 8-bit values FC_PLANAR would store (as floats: the same truncation, rounding or byte extraction that family uses for its bytes);
// here they go through ONE fp32 fma per channel and a round-to-nearest-even conversion (v_cvt_f16_f32 under the default mode / the
// compiler's v_cvt_pk_bf16_f32), then leave as 16 B (f32) or 8 B (f16 / bf16) per lane and channel where the row allows, else one element
// at a time.  The dtype is a kernarg: a wave-uniform branch, one instantiation per family for the three dtypes.
// ------------------------------------------------------------------------------------------
template <int CAP>
VPF_DEV TensorEpi epi_of(const BatchArgsT<CAP>&) { return TensorEpi{}; }  // 8-bit launches: never read
template <int CAP>
VPF_DEV TensorEpi epi_of(const BatchArgsTE<CAP>& a) { return a.e; }
// `vec` of the four-pixel stores below for the per-job kernels: a lane holds four pixels and every plane it stores to (FC_TENSOR_NHWC: the one
// interleaved plane) has base and pitch clear under the launcher's alignment mask (JobPlan::dmask, AaPlan::dmask)
template <int DST>
VPF_DEV bool tensor_vec_ok(const FrameDesc& f, uint32_t nv, uint32_t dmask) {
  bool vec = nv == 4;
#pragma unroll
  for (int ch = 0; ch < (DST == FC_TENSOR_NHWC ? 1 : 3); ch++) vec = vec && ((((uintptr_t)f.d[ch] | f.dp[ch]) & dmask) == 0);
  return vec;
}
// `row` = byte address of row y of channel plane `ch` at column 0; u[] = the 8-bit values of columns x0 .. x0 + 3 (nv of them valid)
template <bool NT>
VPF_DEV void tensor_store4(uint8_t* row, uint32_t x0, const float u[4], const TensorEpi& e, int ch, bool vec, uint32_t nv) {
  float v[4];
#pragma unroll
  for (int k = 0; k < 4; k++) v[k] = __builtin_fmaf(u[k], e.scale[ch], e.bias[ch]);
  if (e.dtype == VPF_TENSOR_F32) {
    float* p = reinterpret_cast<float*>(row) + x0;
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    if (vec) stg<NT, f32x4>(p, f32x4{v[0], v[1], v[2], v[3]});
    else for (uint32_t i = 0; i < nv; i++) p[i] = v[i];
    return;
  }
  uint32_t h[4];
  if (e.dtype == VPF_TENSOR_F16) {
#pragma unroll
    for (int k = 0; k < 4; k++) h[k] = __builtin_bit_cast(uint16_t, (_Float16)v[k]);
  } else {
#pragma unroll
    for (int k = 0; k < 4; k++) h[k] = __builtin_bit_cast(uint16_t, (__bf16)v[k]);
  }
  uint16_t* p = reinterpret_cast<uint16_t*>(row) + x0;
  if (vec) stg<NT, u32x2>(p, u32x2{h[0] | h[1] << 16, h[2] | h[3] << 16});
  else for (uint32_t i = 0; i < nv; i++) p[i] = (uint16_t)h[i];
}
// eight consecutive f16 / bf16 elements per lane (k_convert_half): ONE 16-B store per lane, so a store instruction covers 1 KiB of the row
// without holes (non-temporal, like the 8-bit planes).  (f32 rows go through LDS first: convert_half_task.)
VPF_DEV void tensor_store8(uint8_t* row, uint32_t x0, const float u[8], const TensorEpi& e, int ch) {
  uint32_t h[8];
  if (e.dtype == VPF_TENSOR_F16) {
#pragma unroll
    for (int k = 0; k < 8; k++) h[k] = __builtin_bit_cast(uint16_t, (_Float16)__builtin_fmaf(u[k], e.scale[ch], e.bias[ch]));
  } else {
#pragma unroll
    for (int k = 0; k < 8; k++) h[k] = __builtin_bit_cast(uint16_t, (__bf16)__builtin_fmaf(u[k], e.scale[ch], e.bias[ch]));
  }
  stg<true, u32x4>(reinterpret_cast<uint16_t*>(row) + x0, u32x4{h[0] | h[1] << 16, h[2] | h[3] << 16, h[4] | h[5] << 16, h[6] | h[7] << 16});
}
// the FC_PLANAR store sections' values o[] (+ 0.5 added: truncation gives the byte) of channel ch, pixel k at o[k * stride]
template <bool NT>
VPF_DEV void tensor_store4_trunc(uint8_t* row, uint32_t x0, const float* o, int stride, const TensorEpi& e, int ch, bool vec, uint32_t nv) {
  const float u[4] = {__builtin_truncf(o[0]), __builtin_truncf(o[stride]), __builtin_truncf(o[2 * stride]), __builtin_truncf(o[3 * stride])};
  tensor_store4<NT>(row, x0, u, e, ch, vec, nv);
}

// ------------------------------------------------------------------------------------------
// The channels-last destination (FC_TENSOR_NHWC, VPF_TENSOR_NHWC): the same values in ONE interleaved plane, element (y, x, c) at row y + (3 x + c)
// elements.  A lane holds all three channels of its NPX pixels (4; 8 in k_convert_half), so its 3 NPX elements are one contiguous run: 48 / 96 B of
// f32, 24 / 48 B of f16 / bf16.  The same fma and the same conversions as tensor_store4 / tensor_store8, then one of three store forms:
//   element stores     unaligned planes and row tails (nv < NPX), as tensor_store4 does;
//   per-lane vectors   16-B stores (12-B ones for the 24 B of four 16-bit pixels): every store instruction of a wave writes every third 16 B of its span;
//   dense              the wave's run (64 lanes x 3 NPX elements, one row) goes through wave-private LDS (wave_lds_sync, no workgroup barrier) and
//                      leaves as store instructions that each cover 1 KiB of the row without holes.  The LAUNCHER decides (nhwc_stage_plan,
//                      vpf_internal.h): it appends the staging area to the launch's dynamic LDS and names its place in TensorEpi::dtype; without
//                      one the kernel stores per lane.  Measured: dense wins for f32 in every family and for the half kernel's
//                      16-bit rows; four 16-bit pixels per lane leave faster as two 12-B stores.
// B G R order: the host swapped scale / bias (kernel channel order) and set kEpiSwapRB; kernel channel ch goes to slot 2 - ch (wave-uniform).
// ------------------------------------------------------------------------------------------
typedef uint32_t u32x3_a8 __attribute__((ext_vector_type(3), aligned(8)));
// `row` = byte address of row y of the plane at column 0; u[ch][k] = the 8-bit value of kernel channel ch of column x0 + k (nv of the NPX columns
// valid); `vec`: nv == NPX and a 16-B aligned plane and pitch; `wv`, `lane`: the wave's index in its workgroup and the lane's place in the wave's run
// of the row (x0 = first column of the run + NPX lane); wv = kNoStage: the lanes of a wave are not one run of a row (the warp kernels' tiles).
// Every lane of the wave that is still active calls this together, and the active lanes are lanes 0 .. nact - 1 (lanes right of the row's end
// have left: every family drops them before its epilogue).
constexpr uint32_t kNoStage = ~0u;
template <bool NT, int NPX>
VPF_DEV void tensor_store_nhwc(uint8_t* row, uint32_t x0, const float (&u)[3][NPX], const TensorEpi& e, bool vec, uint32_t nv, uint32_t wv, uint32_t lane) {
  const bool swap = (e.dtype & kEpiSwapRB) != 0;
  const uint32_t dtype = e.dtype & kEpiDtypeMask, stage_q = (e.dtype & kEpiStageMask) >> kEpiStageShift;
  float v[NPX][3];  // slot order
#pragma unroll
  for (int k = 0; k < NPX; k++) {
    const float a = __builtin_fmaf(u[0][k], e.scale[0], e.bias[0]), b = __builtin_fmaf(u[2][k], e.scale[2], e.bias[2]);
    v[k][0] = swap ? b : a;
    v[k][1] = __builtin_fmaf(u[1][k], e.scale[1], e.bias[1]);
    v[k][2] = swap ? a : b;
  }
  constexpr int ND = 3 * NPX;  // dwords of a lane's run: ND of f32, ND / 2 of f16 / bf16
  uint32_t d[ND];
  const bool f32 = dtype == VPF_TENSOR_F32;
  if (f32) {
#pragma unroll
    for (int i = 0; i < ND; i++) d[i] = __float_as_uint(v[i / 3][i % 3]);
  } else {
    uint32_t h[ND];
    if (dtype == VPF_TENSOR_F16) {
#pragma unroll
      for (int i = 0; i < ND; i++) h[i] = __builtin_bit_cast(uint16_t, (_Float16)v[i / 3][i % 3]);
    } else {
#pragma unroll
      for (int i = 0; i < ND; i++) h[i] = __builtin_bit_cast(uint16_t, (__bf16)v[i / 3][i % 3]);
    }
#pragma unroll
    for (int i = 0; i < ND / 2; i++) d[i] = h[2 * i] | h[2 * i + 1] << 16;
#pragma unroll
    for (int i = ND / 2; i < ND; i++) d[i] = 0u;
  }
  const uint32_t elem = f32 ? 4u : 2u;
  uint8_t* const p = row + (size_t)x0 * 3u * elem;
  // dense: every lane of the wave still here takes the vector path (an active lane has all its NPX columns inside the row then)
  if (wv != kNoStage && stage_q != 0 && __builtin_amdgcn_ballot_w64(!vec) == 0) {
    const uint32_t nd = f32 ? (uint32_t)ND : (uint32_t)(ND / 2);  // dwords per lane
    u32x4* const stage = dyn_strip + (stage_q - 1) + wv * (16 * nd);  // 64 lanes x nd dwords per wave, behind the kernel's own dynamic LDS
    uint32_t* const sd = reinterpret_cast<uint32_t*>(stage);
    if (f32) {
#pragma unroll
      for (int j = 0; j < ND / 4; j++) stage[(ND / 4) * lane + j] = u32x4{d[4 * j], d[4 * j + 1], d[4 * j + 2], d[4 * j + 3]};
    } else {
#pragma unroll
      for (int j = 0; j < ND / 4; j++) *reinterpret_cast<u32x2*>(sd + (ND / 2) * lane + 2 * j) = u32x2{d[2 * j], d[2 * j + 1]};
    }
    wave_lds_sync();
    // The nact active lanes wrote the run's first `total` = nact nd dwords (a multiple of 2), all inside the row; the same lanes store them: store
    // k of lane l takes the 16-B unit k nact + l, so every store instruction covers nact x 16 contiguous bytes (1 KiB of a full wave).  Dword
    // 4 idx of the run is 16-B aligned in memory: the run starts at a multiple of 64 NPX columns of a 16-B aligned row.
    const uint32_t nact = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(true)), total = nact * nd;
    uint8_t* const wrow = row + (size_t)(x0 - (uint32_t)NPX * lane) * 3u * elem;
#pragma unroll
    for (int k = 0; k < ND / 4; k++) {
      const uint32_t idx = nact * k + lane;
      if (4 * idx + 4 <= total) stg<NT, u32x4>(wrow + 16 * (size_t)idx, stage[idx]);
      else if (4 * idx + 2 <= total) stg<NT, u32x2>(wrow + 16 * (size_t)idx, *reinterpret_cast<const u32x2*>(sd + 4 * idx));
    }
    wave_lds_sync();  // these LDS reads are done before the wave's next row overwrites the buffer
    return;
  }
  if (vec) {
    if (f32) {
#pragma unroll
      for (int j = 0; j < ND / 4; j++) stg<NT, u32x4>(p + 16 * j, u32x4{d[4 * j], d[4 * j + 1], d[4 * j + 2], d[4 * j + 3]});
    } else if constexpr (NPX % 8 == 0) {
#pragma unroll
      for (int j = 0; j < ND / 8; j++) stg<NT, u32x4>(p + 16 * j, u32x4{d[4 * j], d[4 * j + 1], d[4 * j + 2], d[4 * j + 3]});
    } else {  // 24 B at a multiple of 8: two 12-B stores
#pragma unroll
      for (int j = 0; j < ND / 6; j++) stg<NT, u32x3_a8>(p + 12 * j, u32x3_a8{d[3 * j], d[3 * j + 1], d[3 * j + 2]});
    }
    return;
  }
  if (f32) {
#pragma unroll
    for (int i = 0; i < ND; i++)
      if ((uint32_t)i < 3 * nv) reinterpret_cast<uint32_t*>(p)[i] = d[i];
  } else {
#pragma unroll
    for (int i = 0; i < ND; i++)
      if ((uint32_t)i < 3 * nv) reinterpret_cast<uint16_t*>(p)[i] = (uint16_t)(i & 1 ? d[i >> 1] >> 16 : d[i >> 1]);
  }
}
// the FC_PLANAR store sections' values o[] (+ 0.5 added: truncation gives the byte): channel ch of pixel k at o[ch * cs + k * ps]
template <bool NT>
VPF_DEV void tensor_store4_nhwc_trunc(uint8_t* row, uint32_t x0, const float* o, int cs, int ps, const TensorEpi& e, bool vec, uint32_t nv, uint32_t wv,
                                      uint32_t lane) {
  float u[3][4];
#pragma unroll
  for (int ch = 0; ch < 3; ch++)
#pragma unroll
    for (int k = 0; k < 4; k++) u[ch][k] = __builtin_truncf(o[ch * cs + k * ps]);
  tensor_store_nhwc<NT, 4>(row, x0, u, e, vec, nv, wv, lane);
}

// One conversion unit of the workgroup-shared strips (k_convert_strip_wg, k_roi_strip): 8 pixels x 2 luma rows under one chroma row -> four-byte
// R G B x pixels in LDS.  (FC_P16 sources narrow their samples at the load and come here as FC_NV12.)
template <int SRC>
VPF_DEV void convert_unit8(const FrameDesc& f, const Yuv2RgbCoef& c, uint32_t crow, uint32_t px0, bool row_a, bool row_b, uint8_t* wa /* strip byte of (row 2 crow, px0) */,
                           uint32_t rowbytes, u32x2 ya, u32x2 yb, u32x2 cq, uint32_t vq) {
  (void)f; (void)crow; (void)px0;
  uint32_t uv[2];  // U V U V bytes of pixel pairs 0, 1 | 2, 3
  if constexpr (SRC == FC_NV12) {
    uv[0] = cq[0]; uv[1] = cq[1];
  } else {
    uv[0] = __builtin_amdgcn_perm(vq, cq[0], 0x05010400u); uv[1] = __builtin_amdgcn_perm(vq, cq[0], 0x07030602u);
  }
  Chroma k[4];
#pragma unroll
  for (int j = 0; j < 2; j++) {
    k[2 * j] = chroma_terms(c, ubyte<0>(uv[j]), ubyte<1>(uv[j]));
    k[2 * j + 1] = chroma_terms(c, ubyte<2>(uv[j]), ubyte<3>(uv[j]));
  }
#pragma unroll
  for (int hf = 0; hf < 2; hf++) {
    if (!(hf ? row_b : row_a)) continue;
    const u32x2 yq = hf ? yb : ya;
    uint32_t d[8];  // 8 px -> 8 dwords R G B x (px4 strips, k_bilinear_blend.h), vpf_convert's rounding (v_cvt_pk_u8_f32): three cvt per pixel as for packed bytes
#pragma unroll
    for (int j = 0; j < 2; j++) {  // (the pixel-pair form of convert_strip_task: same IEEE fma per component as convert4 -> same bits)
      const uint32_t yd = yq[j];
      const f32x2 cy2 = {c.cy, c.cy}, ya2 = {ubyte<0>(yd), ubyte<1>(yd)}, yb2 = {ubyte<2>(yd), ubyte<3>(yd)};
      const Chroma &ka = k[2 * j], &kb = k[2 * j + 1];
      const f32x2 ra = __builtin_elementwise_fma(ya2, cy2, f32x2{ka.rc, ka.rc}), ga = __builtin_elementwise_fma(ya2, cy2, f32x2{ka.gc, ka.gc}),
                  ba = __builtin_elementwise_fma(ya2, cy2, f32x2{ka.bc, ka.bc});
      const f32x2 rb = __builtin_elementwise_fma(yb2, cy2, f32x2{kb.rc, kb.rc}), gb = __builtin_elementwise_fma(yb2, cy2, f32x2{kb.gc, kb.gc}),
                  bb = __builtin_elementwise_fma(yb2, cy2, f32x2{kb.bc, kb.bc});
      d[4 * j] = pack3(ra[0], ga[0], ba[0]);
      d[4 * j + 1] = pack3(ra[1], ga[1], ba[1]);
      d[4 * j + 2] = pack3(rb[0], gb[0], bb[0]);
      d[4 * j + 3] = pack3(rb[1], gb[1], bb[1]);
    }
    u32x4* w = reinterpret_cast<u32x4*>(wa + (hf ? rowbytes : 0u));
    w[0] = u32x4{d[0], d[1], d[2], d[3]}; w[1] = u32x4{d[4], d[5], d[6], d[7]};
  }
}

// The fill stage of the staged per-job kernels (k_roi_strip, k_warp_strip): the workgroup's 256 lanes convert the source window of ABSOLUTE frame
// pixels [base_px, base_px + 8 ng) x rows [R_lo, R_hi] into the strip, whole conversion units at a time with loads of any alignment; the unit that
// holds the frame's right edge takes clamped byte loads, so no byte outside the frame's own rows is read.  The caller synchronises afterwards.
// FC_P16: a unit's 8 luma samples and its 4 U V pairs are 16 B each at byte 2 px0 of their rows (px0 even: chroma pair px0 / 2 starts at byte
// 4 (px0 / 2)), loaded at any 2-B alignment and narrowed to the two dwords the 8-bit unit takes.  The whole-unit loads run under the same
// condition px0 + 8 <= W: luma bytes [2 px0, 2 px0 + 16) end at or before 2 W, chroma bytes at 4 (px0 / 2 + 4) <= 4 ceil(W / 2) — inside the
// rows' own samples.  The right-edge unit takes 2-B sample loads with indices clamped to the row's last sample (pair), as the 8-bit code does.
// `base_px` is even; ng = units per row; the window holds the chroma rows (R_lo >> 1) .. (R_hi >> 1); tid = the lane's index in the workgroup.
template <int SRC>
VPF_DEV void strip_fill_window(const FrameDesc& f, const Yuv2RgbCoef& c, uint32_t W, uint8_t* strip, uint32_t base_px, uint32_t R_lo, uint32_t R_hi, uint32_t ng,
                               uint32_t rowbytes, uint32_t tid) {
  const uint32_t c_lo = R_lo >> 1, units = ((R_hi >> 1) - c_lo + 1) * ng;
  const uint32_t cw = (W + 1) >> 1;
  const float rng = 1.0f / (float)ng;
  // unit u -> (chroma row ci = u / ng, group g): (u + 0.5) / ng is at least 0.5 / ng from an integer, far more than the fp32 error for u < 2^14
  struct Unit { bool act = false, ra = false, rb = false; uint8_t* w = nullptr; u32x2 ya = {0u, 0u}, yb = {0u, 0u}, cq = {0u, 0u}; uint32_t vq = 0; };
  auto bytes8 = [&](const uint8_t* row, uint32_t i0, uint32_t n) {  // samples i0 .. i0 + 7 of a row of n, indices clamped to n - 1
    uint32_t d[2] = {0u, 0u};
#pragma unroll
    for (int k = 0; k < 8; k++) {
      const uint32_t i = i0 + k < n ? i0 + k : n - 1;
      d[k >> 2] |= (uint32_t)row[i] << (8 * (k & 3));
    }
    return u32x2{d[0], d[1]};
  };
  auto fetch = [&](uint32_t u, Unit& q) {
    q.act = u < units;
    if (!q.act) return;
    const uint32_t ci = (uint32_t)(((float)u + 0.5f) * rng), g = u - ci * ng;
    const uint32_t crow = c_lo + ci, px0 = base_px + 8 * g, r0 = 2 * crow;
    q.ra = r0 >= R_lo; q.rb = r0 + 1 <= R_hi;  // (r0 <= R_hi and r0 + 1 >= R_lo hold for every chroma row of the window)
    const uint8_t* const y0p = f.s[0] + (size_t)r0 * f.sp[0];
    const uint8_t* const c1p = f.s[1] + (size_t)crow * f.sp[1];
    if constexpr (SRC == FC_P16) {
      (void)bytes8;
      auto words8 = [&](const uint8_t* row, uint32_t i0, uint32_t n) {  // 16-bit samples i0 .. i0 + 7 of a row of n, clamped to n - 1, narrowed
        uint32_t d[2] = {0u, 0u};
#pragma unroll
        for (int k = 0; k < 8; k++) {
          const uint32_t i = i0 + k < n ? i0 + k : n - 1;
          d[k >> 2] |= (uint32_t)p16_to_8(reinterpret_cast<const uint16_t*>(row)[i]) << (8 * (k & 3));
        }
        return u32x2{d[0], d[1]};
      };
      if (px0 + 8 <= W) {
        q.cq = p16x8_to_8(*reinterpret_cast<const u32x4_any*>(c1p + 2 * (size_t)px0));
        if (q.ra) q.ya = p16x8_to_8(*reinterpret_cast<const u32x4_any*>(y0p + 2 * (size_t)px0));
        if (q.rb) q.yb = p16x8_to_8(*reinterpret_cast<const u32x4_any*>(y0p + f.sp[0] + 2 * (size_t)px0));
      } else {  // the unit that holds the frame's right edge
        uint32_t d[2] = {0u, 0u};  // U V pairs of chroma samples (px0 >> 1) .. + 3
#pragma unroll
        for (int k = 0; k < 4; k++) {
          const uint32_t i = (px0 >> 1) + k < cw ? (px0 >> 1) + k : cw - 1;
          const uint16_t* const pc = reinterpret_cast<const uint16_t*>(c1p);
          d[k >> 1] |= ((uint32_t)p16_to_8(pc[2 * i]) | (uint32_t)p16_to_8(pc[2 * i + 1]) << 8) << (16 * (k & 1));
        }
        q.cq = u32x2{d[0], d[1]};
        if (q.ra) q.ya = words8(y0p, px0, W);
        if (q.rb) q.yb = words8(y0p + f.sp[0], px0, W);
      }
    } else if (px0 + 8 <= W) {
      if constexpr (SRC == FC_NV12) {
        q.cq = *reinterpret_cast<const u32x2_any*>(c1p + px0);
      } else {
        q.cq = u32x2{*reinterpret_cast<const u32_any*>(c1p + (px0 >> 1)), 0u};
        q.vq = *reinterpret_cast<const u32_any*>(f.s[2] + (size_t)crow * f.sp[2] + (px0 >> 1));
      }
      if (q.ra) q.ya = *reinterpret_cast<const u32x2_any*>(y0p + px0);
      if (q.rb) q.yb = *reinterpret_cast<const u32x2_any*>(y0p + f.sp[0] + px0);
    } else {  // the unit that holds the frame's right edge
      if constexpr (SRC == FC_NV12) {
        uint32_t d[2] = {0u, 0u};  // U V pairs of chroma samples (px0 >> 1) .. + 3
#pragma unroll
        for (int k = 0; k < 4; k++) {
          const uint32_t i = (px0 >> 1) + k < cw ? (px0 >> 1) + k : cw - 1;
          d[k >> 1] |= ((uint32_t)c1p[2 * i] | (uint32_t)c1p[2 * i + 1] << 8) << (16 * (k & 1));
        }
        q.cq = u32x2{d[0], d[1]};
      } else {
        q.cq = u32x2{bytes8(c1p, px0 >> 1, cw)[0], 0u};
        q.vq = bytes8(f.s[2] + (size_t)crow * f.sp[2], px0 >> 1, cw)[0];
      }
      if (q.ra) q.ya = bytes8(y0p, px0, W);
      if (q.rb) q.yb = bytes8(y0p + f.sp[0], px0, W);
    }
    // strip byte of (row r0, px0); r0 may be R_lo - 1 (that row is not written then: only row r0 + 1 is) — a signed offset
    q.w = strip + ((int32_t)(r0 - R_lo) * (int32_t)rowbytes + (int32_t)(4 * (px0 - base_px)));
  };
  for (uint32_t u0 = tid; u0 < units; u0 += 512) {  // two units per lane in flight
    Unit q0, q1;
    fetch(u0, q0);
    fetch(u0 + 256, q1);
    __builtin_amdgcn_sched_barrier(0);  // both units' loads are requested before the first conversion
    if (q0.act) convert_unit8<(SRC == FC_P16 ? (int)FC_NV12 : SRC)>(f, c, 0u, 0u, q0.ra, q0.rb, q0.w, rowbytes, q0.ya, q0.yb, q0.cq, q0.vq);
    if (q1.act) convert_unit8<(SRC == FC_P16 ? (int)FC_NV12 : SRC)>(f, c, 0u, 0u, q1.ra, q1.rb, q1.w, rowbytes, q1.ya, q1.yb, q1.cq, q1.vq);
  }
}

}  // namespace vpf
#endif  // VPF_K_FUSED_COMMON_H_
