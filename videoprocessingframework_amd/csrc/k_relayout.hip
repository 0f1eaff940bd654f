// k_relayout.hip — pure re-layout converters for gfx950 (no arithmetic on the samples, or a single
// scale): NV12 <-> YUV420 (reference nv12_yuv420 / yuv420_nv12, src/TC/src/TasksColorCvt.cpp:196-240,
// 945-975), RGB <-> RGB_PLANAR (rgb8_deinterleave / rgb8_interleave :1059-1088,1102-1131), RGB <-> BGR
// (rgb_bgr / bgr_rgb :1145-1209), NV12 -> Y (nv12_y :254-279), Y -> YUV444 (y_yuv444 :844-873),
// RGB -> RGB_32F (rbg8_rgb32f :1222-1254), RGB_32F -> RGB_32F_PLANAR (rgb32f_deinterleave :1268-1297),
// P10/P12 -> NV12 (p16_nv12 :990-1045), RGB/BGR -> Y (rbg8_y :293-308).
//
// All of it is 2-24 B/px of pure HBM streaming.  Three tiers per converter, bit-identical: the r16 kernels (a wave = one row x
// 1024 px, every global access a dense non-temporal 1-KiB run, packed sides through a wave-private LDS transpose) for
// 16-px / 16-B regular frames; p4 / p16 kernels (4-16 B per lane, v_perm_b32 shuffles in registers) for 4-B aligned ones;
// a generic per-pixel kernel for everything else.
#include "k_job_launch.h"
#include "vpf_device.h"

namespace vpf {

// ------------------------------------------------------------------------------------------
// NV12 <-> YUV420: one lane = 16 luma px x 2 rows + 8 chroma pairs.
// fast path: w % 16 == 0, h even, Y/UV planes 16-B aligned, U/V planes 8-B aligned.
// ------------------------------------------------------------------------------------------
template <bool TO_PLANAR>
__global__ __launch_bounds__(256) void k_nv12_yuv420_p16(const BatchArgs args, uint32_t w, uint32_t h,
                                                         uint32_t groups_x) {
  const FrameDesc f = args.f[blockIdx.z];
  const uint32_t gx = blockIdx.x * 64 + (threadIdx.x & 63);
  const uint32_t rp = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (gx >= groups_x || rp >= (h >> 1)) return;
  const uint32_t x = gx * 16;
  const u32x4 y0 = ldg<false, u32x4>(f.s[0] + (size_t)(2 * rp) * f.sp[0] + x);
  const u32x4 y1 = ldg<false, u32x4>(f.s[0] + (size_t)(2 * rp + 1) * f.sp[0] + x);
  if constexpr (TO_PLANAR) {
    const u32x4 uv = ldg<false, u32x4>(f.s[1] + (size_t)rp * f.sp[1] + x);
    u32x2 u, v;  // even bytes -> U, odd bytes -> V
    u[0] = __builtin_amdgcn_perm(uv[1], uv[0], 0x06040200u);
    u[1] = __builtin_amdgcn_perm(uv[3], uv[2], 0x06040200u);
    v[0] = __builtin_amdgcn_perm(uv[1], uv[0], 0x07050301u);
    v[1] = __builtin_amdgcn_perm(uv[3], uv[2], 0x07050301u);
    stg<false, u32x2>(f.d[1] + (size_t)rp * f.dp[1] + (x >> 1), u);
    stg<false, u32x2>(f.d[2] + (size_t)rp * f.dp[2] + (x >> 1), v);
  } else {
    const u32x2 u = ldg<false, u32x2>(f.s[1] + (size_t)rp * f.sp[1] + (x >> 1));
    const u32x2 v = ldg<false, u32x2>(f.s[2] + (size_t)rp * f.sp[2] + (x >> 1));
    u32x4 uv;  // interleave: U0 V0 U1 V1 | U2 V2 U3 V3 | ...
    uv[0] = __builtin_amdgcn_perm(v[0], u[0], 0x05010400u);
    uv[1] = __builtin_amdgcn_perm(v[0], u[0], 0x07030602u);
    uv[2] = __builtin_amdgcn_perm(v[1], u[1], 0x05010400u);
    uv[3] = __builtin_amdgcn_perm(v[1], u[1], 0x07030602u);
    stg<false, u32x4>(f.d[1] + (size_t)rp * f.dp[1] + x, uv);
  }
  stg<false, u32x4>(f.d[0] + (size_t)(2 * rp) * f.dp[0] + x, y0);
  stg<false, u32x4>(f.d[0] + (size_t)(2 * rp + 1) * f.dp[0] + x, y1);
}

// ------------------------------------------------------------------------------------------
// packed RGB <-> planar / channel swap: one lane = 4 px = 12 packed bytes.
// fast path: w % 4 == 0, planes 4-B aligned.  MODE 0: packed->planar, 1: planar->packed, 2: swap R/B
// ------------------------------------------------------------------------------------------
template <int MODE>
__global__ __launch_bounds__(256) void k_rgb_relayout_p4(const BatchArgs args, uint32_t w, uint32_t h,
                                                         uint32_t groups_x) {
  const FrameDesc f = args.f[blockIdx.z];
  const uint32_t gx = blockIdx.x * 64 + (threadIdx.x & 63);
  const uint32_t y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (gx >= groups_x || y >= h) return;
  const uint32_t x = gx * 4;
  if constexpr (MODE == 1) {
    const uint32_t r = ldg<false, uint32_t>(f.s[0] + (size_t)y * f.sp[0] + x);
    const uint32_t g = ldg<false, uint32_t>(f.s[1] + (size_t)y * f.sp[1] + x);
    const uint32_t b = ldg<false, uint32_t>(f.s[2] + (size_t)y * f.sp[2] + x);
    uint32_t d0, d1, d2;
    inter4(r, g, b, d0, d1, d2);
    stg3<false>(f.d[0] + (size_t)y * f.dp[0] + 3 * (size_t)x, d0, d1, d2);
  } else {
    const uint8_t* p = f.s[0] + (size_t)y * f.sp[0] + 3 * (size_t)x;
    const uint32_t d0 = ldg<false, uint32_t>(p), d1 = ldg<false, uint32_t>(p + 4), d2 = ldg<false, uint32_t>(p + 8);
    if constexpr (MODE == 0) {
      uint32_t c0, c1, c2;
      deint4(d0, d1, d2, c0, c1, c2);
      stg<false, uint32_t>(f.d[0] + (size_t)y * f.dp[0] + x, c0);
      stg<false, uint32_t>(f.d[1] + (size_t)y * f.dp[1] + x, c1);
      stg<false, uint32_t>(f.d[2] + (size_t)y * f.dp[2] + x, c2);
    } else {
      uint32_t o0, o1, o2;
      swap4(d0, d1, d2, o0, o1, o2);
      stg3<false>(f.d[0] + (size_t)y * f.dp[0] + 3 * (size_t)x, o0, o1, o2);
    }
  }
}

// ------------------------------------------------------------------------------------------
// generic per-pixel re-layout: any size / alignment, byte (or element) accesses.
// ------------------------------------------------------------------------------------------
// (GenericOp — OP_NV12_YUV420 ... : vpf_convert_plan.h, which names the op a launch takes)

template <int OP>
__global__ __launch_bounds__(256) void k_relayout_generic(const BatchArgs args, uint32_t w, uint32_t h) {
  const FrameDesc f = args.f[blockIdx.z];
  const uint32_t x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= w || y >= h) return;
  const uint32_t cw = (w + 1) >> 1, ch = (h + 1) >> 1;
  auto S = [&](int k, uint32_t yy, uint32_t xx) -> uint8_t { return f.s[k][(size_t)yy * f.sp[k] + xx]; };
  auto D = [&](int k, uint32_t yy, uint32_t xx) -> uint8_t& { return f.d[k][(size_t)yy * f.dp[k] + xx]; };
  if constexpr (OP == OP_NV12_YUV420) {
    D(0, y, x) = S(0, y, x);
    if (x < cw && y < ch) { D(1, y, x) = S(1, y, 2 * x); D(2, y, x) = S(1, y, 2 * x + 1); }
  } else if constexpr (OP == OP_YUV420_NV12) {
    D(0, y, x) = S(0, y, x);
    if (x < cw && y < ch) { D(1, y, 2 * x) = S(1, y, x); D(1, y, 2 * x + 1) = S(2, y, x); }
  } else if constexpr (OP == OP_RGB_PLANAR) {
    for (int k = 0; k < 3; k++) D(k, y, x) = S(0, y, 3 * x + k);
  } else if constexpr (OP == OP_PLANAR_RGB) {
    for (int k = 0; k < 3; k++) D(0, y, 3 * x + k) = S(k, y, x);
  } else if constexpr (OP == OP_PLANAR_SWAP) {  // RGB_PLANAR -> BGR packed
    for (int k = 0; k < 3; k++) D(0, y, 3 * x + k) = S(2 - k, y, x);
  } else if constexpr (OP == OP_SWAP_RB) {
    const uint8_t a = S(0, y, 3 * x), b = S(0, y, 3 * x + 1), c = S(0, y, 3 * x + 2);
    D(0, y, 3 * x) = c; D(0, y, 3 * x + 1) = b; D(0, y, 3 * x + 2) = a;
  } else if constexpr (OP == OP_COPY_Y) {
    D(0, y, x) = S(0, y, x);
  } else if constexpr (OP == OP_Y_YUV444) {
    D(0, y, x) = S(0, y, x); D(1, y, x) = 128; D(2, y, x) = 128;
  } else if constexpr (OP == OP_RGB_RGB32F) {
    float* o = reinterpret_cast<float*>(f.d[0] + (size_t)y * f.dp[0]) + 3 * (size_t)x;
    for (int k = 0; k < 3; k++) o[k] = (float)S(0, y, 3 * x + k) / 255.0f;
  } else if constexpr (OP == OP_RGB32F_PLANAR) {
    const float* i = reinterpret_cast<const float*>(f.s[0] + (size_t)y * f.sp[0]) + 3 * (size_t)x;
    for (int k = 0; k < 3; k++) reinterpret_cast<float*>(f.d[k] + (size_t)y * f.dp[k])[x] = i[k];
  } else if constexpr (OP == OP_P16_NV12) {
    D(0, y, x) = p16_to_8(reinterpret_cast<const uint16_t*>(f.s[0] + (size_t)y * f.sp[0])[x]);
    if (x < cw && y < ch) {
      const uint16_t* i = reinterpret_cast<const uint16_t*>(f.s[1] + (size_t)y * f.sp[1]);
      D(1, y, 2 * x) = p16_to_8(i[2 * x]); D(1, y, 2 * x + 1) = p16_to_8(i[2 * x + 1]);
    }
  } else {  // gray: .299R + .587G + .114B, round half up
    float r, g, b;
    if constexpr (OP == OP_PLANAR_GRAY) { r = S(0, y, x); g = S(1, y, x); b = S(2, y, x); }
    else { r = S(0, y, 3 * x + (OP == OP_BGR_GRAY ? 2 : 0)); g = S(0, y, 3 * x + 1); b = S(0, y, 3 * x + (OP == OP_BGR_GRAY ? 0 : 2)); }
    D(0, y, x) = (uint8_t)sat_trunc(__builtin_fmaf(r, 0.299f, __builtin_fmaf(g, 0.587f, __builtin_fmaf(b, 0.114f, 0.5f))));
  }
}

// ------------------------------------------------------------------------------------------
// more fast paths (all: one dense wave access per instruction)
// ------------------------------------------------------------------------------------------
// plane copy, 16 B per lane; FILL: also writes 128 into two more planes (Y -> YUV444, reference y_yuv444 :844-873)
template <bool FILL>
__global__ __launch_bounds__(256) void k_copy_plane_p16(const BatchArgs args, uint32_t wbytes, uint32_t h, uint32_t groups_x) {
  const FrameDesc f = args.f[blockIdx.z];
  const uint32_t gx = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (gx >= groups_x || y >= h) return;
  const uint32_t x = gx * 16;
  stg<true, u32x4>(f.d[0] + (size_t)y * f.dp[0] + x, ldg<false, u32x4>(f.s[0] + (size_t)y * f.sp[0] + x));
  if constexpr (FILL) {
    const u32x4 v = {0x80808080u, 0x80808080u, 0x80808080u, 0x80808080u};
    stg<true, u32x4>(f.d[1] + (size_t)y * f.dp[1] + x, v);
    stg<true, u32x4>(f.d[2] + (size_t)y * f.dp[2] + x, v);
  }
}

// RGB / BGR / RGB_PLANAR -> Y (gray): lane = 4 px.  SRC: 0 RGB, 1 BGR, 2 planar
template <int SRC>
__global__ __launch_bounds__(256) void k_gray_p4(const BatchArgs args, uint32_t w, uint32_t h, uint32_t groups_x) {
  const FrameDesc f = args.f[blockIdx.z];
  const uint32_t gx = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (gx >= groups_x || y >= h) return;
  const uint32_t x = gx * 4;
  float r[4], g[4], b[4];
  if constexpr (SRC == 2) {
    const uint32_t rd = ldg<false, uint32_t>(f.s[0] + (size_t)y * f.sp[0] + x), gd = ldg<false, uint32_t>(f.s[1] + (size_t)y * f.sp[1] + x),
                   bd = ldg<false, uint32_t>(f.s[2] + (size_t)y * f.sp[2] + x);
    r[0] = ubyte<0>(rd); r[1] = ubyte<1>(rd); r[2] = ubyte<2>(rd); r[3] = ubyte<3>(rd);
    g[0] = ubyte<0>(gd); g[1] = ubyte<1>(gd); g[2] = ubyte<2>(gd); g[3] = ubyte<3>(gd);
    b[0] = ubyte<0>(bd); b[1] = ubyte<1>(bd); b[2] = ubyte<2>(bd); b[3] = ubyte<3>(bd);
  } else {
    const uint8_t* p = f.s[0] + (size_t)y * f.sp[0] + 3 * (size_t)x;
    const uint32_t d0 = ldg<false, uint32_t>(p), d1 = ldg<false, uint32_t>(p + 4), d2 = ldg<false, uint32_t>(p + 8);
    float* c0 = (SRC == 1) ? b : r;
    float* c2 = (SRC == 1) ? r : b;
    c0[0] = ubyte<0>(d0); g[0] = ubyte<1>(d0); c2[0] = ubyte<2>(d0);
    c0[1] = ubyte<3>(d0); g[1] = ubyte<0>(d1); c2[1] = ubyte<1>(d1);
    c0[2] = ubyte<2>(d1); g[2] = ubyte<3>(d1); c2[2] = ubyte<0>(d2);
    c0[3] = ubyte<1>(d2); g[3] = ubyte<2>(d2); c2[3] = ubyte<3>(d2);
  }
  float o[4];
#pragma unroll
  for (int k = 0; k < 4; k++) o[k] = __builtin_fmaf(r[k], 0.299f, __builtin_fmaf(g[k], 0.587f, __builtin_fmaf(b[k], 0.114f, 0.5f)));
  stg<false, uint32_t>(f.d[0] + (size_t)y * f.dp[0] + x, pack4_trunc(o[0], o[1], o[2], o[3]));
}

// RGB -> RGB_32F is elementwise over the 3W bytes of a row: lane = 4 bytes in -> 16 B (4 floats) out
__global__ __launch_bounds__(256) void k_u8_to_f32_p4(const BatchArgs args, uint32_t wbytes, uint32_t h, uint32_t groups_x) {
  const FrameDesc f = args.f[blockIdx.z];
  const uint32_t gx = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (gx >= groups_x || y >= h) return;
  const uint32_t d = ldg<false, uint32_t>(f.s[0] + (size_t)y * f.sp[0] + 4 * (size_t)gx);
  typedef float f32x4 __attribute__((ext_vector_type(4)));
  const f32x4 v = {ubyte<0>(d) / 255.0f, ubyte<1>(d) / 255.0f, ubyte<2>(d) / 255.0f, ubyte<3>(d) / 255.0f};
  stg<true, f32x4>(f.d[0] + (size_t)y * f.dp[0] + 16 * (size_t)gx, v);
}

// P10 / P12 -> NV12 is elementwise over 16-bit samples of both planes: lane = 8 samples (16 B) -> 8 B.
// Rows [0, h) are luma, rows [h, h + ceil(h/2)) chroma; both have `wsamples` samples per row.
__global__ __launch_bounds__(256) void k_p16_to_8_p8(const BatchArgs args, uint32_t wsamples, uint32_t h, uint32_t ch, uint32_t groups_x) {
  const FrameDesc f = args.f[blockIdx.z];
  const uint32_t gx = blockIdx.x * 64 + (threadIdx.x & 63), row = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (gx >= groups_x || row >= h + ch) return;
  const int pl = row >= h;
  const uint32_t y = pl ? row - h : row;
  const u32x4 v = ldg<false, u32x4>(f.s[pl] + (size_t)y * f.sp[pl] + 16 * (size_t)gx);
  u32x2 o;
#pragma unroll
  for (int k = 0; k < 2; k++) {
    const uint32_t a = v[2 * k], b = v[2 * k + 1];
    o[k] = (uint32_t)p16_to_8((uint16_t)(a & 0xffffu)) | ((uint32_t)p16_to_8((uint16_t)(a >> 16)) << 8) |
           ((uint32_t)p16_to_8((uint16_t)(b & 0xffffu)) << 16) | ((uint32_t)p16_to_8((uint16_t)(b >> 16)) << 24);
  }
  stg<false, u32x2>(f.d[pl] + (size_t)y * f.dp[pl] + 8 * (size_t)gx, o);
}


// ------------------------------------------------------------------------------------------
// r16 family: one wave = one row x 1024 px, one lane = 16 px; every global access of a wave is a dense 1-KiB
// dwordx4 run, non-temporal (the write-rate law of DESIGN.md §4: few, large, dense stores per wave).  Packed sides go
// through load_run48 / store_run48.  Requires w % 16 == 0 and 16-B aligned planes and pitches.
// MODE 0: packed -> planar, 1: planar -> packed, 2: swap R/B
// ------------------------------------------------------------------------------------------
// RGB_32F -> RGB_32F_PLANAR is the same shape one size up: a 3-KiB run is 256 px of 12 B, a lane owns 4 px and
// de-interleaves whole dwords.  Requires w % 4 == 0, 16-B aligned planes / pitches.
VPF_DEV void rgb32f_planar_r4_task(const FrameDesc& f, uint32_t w, uint32_t h, uint32_t chunks_x, uint32_t n_tasks) {
  __shared__ u32x4 tile[4 * 192];
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const uint32_t wt = blockIdx.x * 4 + wv;
  if (wt >= n_tasks) return;
  const uint32_t y = wt / chunks_x, chunk = wt - y * chunks_x;
  const uint32_t x = chunk * 256 + lane * 4;
  uint32_t d[12];
  load_run48(tile + wv * 192, f.s[0] + (size_t)y * f.sp[0], chunk * 3072, 12 * w, lane, d);
  if (x >= w) return;
#pragma unroll
  for (int k = 0; k < 3; k++) stg<true, u32x4>(f.d[k] + (size_t)y * f.dp[k] + 4 * (size_t)x, u32x4{d[k], d[3 + k], d[6 + k], d[9 + k]});
}
__global__ __launch_bounds__(256) void k_rgb32f_planar_r4(const BatchArgs args, uint32_t w, uint32_t h, uint32_t chunks_x, uint32_t n_tasks) {
  rgb32f_planar_r4_task(args.f[blockIdx.y], w, h, chunks_x, n_tasks);
}
__global__ __launch_bounds__(256) void k_rgb32f_planar_r4_one(VPF_ONE_SRC_PARAMS, uint32_t w, uint32_t h, uint32_t chunks_x, uint32_t n_tasks, VPF_ONE_DST_PARAMS) {  // single-frame entry: scalar arguments
  rgb32f_planar_r4_task(VPF_ONE_FRAME, w, h, chunks_x, n_tasks);
}

template <int MODE>
VPF_DEV void rgb_relayout_r16_task(const FrameDesc& f, uint32_t w, uint32_t h, uint32_t chunks_x, uint32_t n_tasks) {
  __shared__ u32x4 tile[4 * 192];
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const uint32_t wt = blockIdx.x * 4 + wv;
  if (wt >= n_tasks) return;
  const uint32_t y = wt / chunks_x, chunk = wt - y * chunks_x;
  const uint32_t x = chunk * 1024 + lane * 16;
  u32x4* t = tile + wv * 192;
  uint32_t d[12];
  if constexpr (MODE == 0) {
    load_run48(t, f.s[0] + (size_t)y * f.sp[0], chunk * 3072, 3 * w, lane, d);
    if (x >= w) return;
    uint32_t c0[4], c1[4], c2[4];
#pragma unroll
    for (int g = 0; g < 4; g++) deint4(d[3 * g], d[3 * g + 1], d[3 * g + 2], c0[g], c1[g], c2[g]);
    stg<true, u32x4>(f.d[0] + (size_t)y * f.dp[0] + x, u32x4{c0[0], c0[1], c0[2], c0[3]});
    stg<true, u32x4>(f.d[1] + (size_t)y * f.dp[1] + x, u32x4{c1[0], c1[1], c1[2], c1[3]});
    stg<true, u32x4>(f.d[2] + (size_t)y * f.dp[2] + x, u32x4{c2[0], c2[1], c2[2], c2[3]});
  } else if constexpr (MODE == 1) {
    const uint32_t xc = x < w ? x : w - 16;  // clamped lanes compute a duplicate that store_run48 never writes
    const u32x4 c0 = ldg<true, u32x4>(f.s[0] + (size_t)y * f.sp[0] + xc);
    const u32x4 c1 = ldg<true, u32x4>(f.s[1] + (size_t)y * f.sp[1] + xc);
    const u32x4 c2 = ldg<true, u32x4>(f.s[2] + (size_t)y * f.sp[2] + xc);
#pragma unroll
    for (int g = 0; g < 4; g++) inter4(c0[g], c1[g], c2[g], d[3 * g], d[3 * g + 1], d[3 * g + 2]);
    store_run48(t, f.d[0] + (size_t)y * f.dp[0], chunk * 3072, 3 * w, lane, d);
  } else {
    load_run48(t, f.s[0] + (size_t)y * f.sp[0], chunk * 3072, 3 * w, lane, d);
    uint32_t o[12];
#pragma unroll
    for (int g = 0; g < 4; g++) swap4(d[3 * g], d[3 * g + 1], d[3 * g + 2], o[3 * g], o[3 * g + 1], o[3 * g + 2]);
    store_run48(t, f.d[0] + (size_t)y * f.dp[0], chunk * 3072, 3 * w, lane, o);  // each lane rewrites only its own 3 slots
  }
}
template <int MODE>
__global__ __launch_bounds__(256) void k_rgb_relayout_r16(const BatchArgs args, uint32_t w, uint32_t h, uint32_t chunks_x, uint32_t n_tasks) {
  rgb_relayout_r16_task<MODE>(args.f[blockIdx.y], w, h, chunks_x, n_tasks);
}
template <int MODE>  // single-frame entry: scalar arguments (see VPF_ONE_SRC_PARAMS in vpf_internal.h)
__global__ __launch_bounds__(256) void k_rgb_relayout_r16_one(VPF_ONE_SRC_PARAMS, uint32_t w, uint32_t h, uint32_t chunks_x, uint32_t n_tasks,
                                                              VPF_ONE_DST_PARAMS) {
  rgb_relayout_r16_task<MODE>(VPF_ONE_FRAME, w, h, chunks_x, n_tasks);
}

// RGB / BGR / RGB_PLANAR -> Y, 16 px per lane -> one dense 1-KiB store per wave.  SRC: 0 RGB, 1 BGR, 2 planar
template <int SRC>
VPF_DEV void gray_r16_task(const FrameDesc& f, uint32_t w, uint32_t h, uint32_t chunks_x, uint32_t n_tasks) {
  __shared__ u32x4 tile[SRC == 2 ? 1 : 4 * 192];
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const uint32_t wt = blockIdx.x * 4 + wv;
  if (wt >= n_tasks) return;
  const uint32_t y = wt / chunks_x, chunk = wt - y * chunks_x;
  const uint32_t x = chunk * 1024 + lane * 16;
  uint32_t c0[4], c1[4], c2[4];
  if constexpr (SRC == 2) {
    if (x >= w) return;
    const u32x4 q0 = ldg<true, u32x4>(f.s[0] + (size_t)y * f.sp[0] + x);
    const u32x4 q1 = ldg<true, u32x4>(f.s[1] + (size_t)y * f.sp[1] + x);
    const u32x4 q2 = ldg<true, u32x4>(f.s[2] + (size_t)y * f.sp[2] + x);
#pragma unroll
    for (int g = 0; g < 4; g++) { c0[g] = q0[g]; c1[g] = q1[g]; c2[g] = q2[g]; }
  } else {
    uint32_t d[12];
    load_run48(tile + wv * 192, f.s[0] + (size_t)y * f.sp[0], chunk * 3072, 3 * w, lane, d);
    if (x >= w) return;
#pragma unroll
    for (int g = 0; g < 4; g++) deint4(d[3 * g], d[3 * g + 1], d[3 * g + 2], c0[g], c1[g], c2[g]);
  }
  const uint32_t* rr = (SRC == 1) ? c2 : c0;
  const uint32_t* bb = (SRC == 1) ? c0 : c2;
  uint32_t o[4];
#pragma unroll
  for (int g = 0; g < 4; g++) {
    const uint32_t r = rr[g], gg = c1[g], b = bb[g];
    auto gray = [](float R, float G, float B) { return __builtin_fmaf(R, 0.299f, __builtin_fmaf(G, 0.587f, __builtin_fmaf(B, 0.114f, 0.5f))); };
    o[g] = pack4_trunc(gray(ubyte<0>(r), ubyte<0>(gg), ubyte<0>(b)), gray(ubyte<1>(r), ubyte<1>(gg), ubyte<1>(b)),
                       gray(ubyte<2>(r), ubyte<2>(gg), ubyte<2>(b)), gray(ubyte<3>(r), ubyte<3>(gg), ubyte<3>(b)));
  }
  stg<true, u32x4>(f.d[0] + (size_t)y * f.dp[0] + x, u32x4{o[0], o[1], o[2], o[3]});
}
template <int SRC>
__global__ __launch_bounds__(256) void k_gray_r16(const BatchArgs args, uint32_t w, uint32_t h, uint32_t chunks_x, uint32_t n_tasks) {
  gray_r16_task<SRC>(args.f[blockIdx.y], w, h, chunks_x, n_tasks);
}
template <int SRC>
__global__ __launch_bounds__(256) void k_gray_r16_one(VPF_ONE_SRC_PARAMS, uint32_t w, uint32_t h, uint32_t chunks_x, uint32_t n_tasks, VPF_ONE_DST_PARAMS) {  // single-frame entry: scalar arguments
  gray_r16_task<SRC>(VPF_ONE_FRAME, w, h, chunks_x, n_tasks);
}

// NV12 <-> YUV420, rows split by role: a luma wave copies 1 KiB (one load, one store); a chroma wave moves 2 KiB of
// interleaved UV <-> 1 KiB of U + 1 KiB of V.  Requires w % 32 == 0, h even, every plane and pitch 16-B aligned.
// (Numbering the blocks straight through the planes, which is worth 1 % on k_nv12_rgb_p16x, changes nothing here: 0.78 vs 0.79 of 8 TB/s
// at 4K, 0.72 vs 0.72 at 1080p in same-box A/B, round 2.)
template <bool TO_PLANAR>
VPF_DEV void nv12_yuv420_r16_task(const FrameDesc& f, uint32_t w, uint32_t h, uint32_t chunks_y, uint32_t luma_tasks, uint32_t chunks_c, uint32_t n_tasks) {
  __shared__ u32x4 tile[TO_PLANAR ? 1 : 4 * 128];
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const uint32_t wt = blockIdx.x * 4 + wv;
  if (wt >= n_tasks) return;
  if (wt < luma_tasks) {
    const uint32_t y = wt / chunks_y, x = (wt - y * chunks_y) * 1024 + lane * 16;
    if (x < w) stg<true, u32x4>(f.d[0] + (size_t)y * f.dp[0] + x, ldg<true, u32x4>(f.s[0] + (size_t)y * f.sp[0] + x));
    return;
  }
  const uint32_t ct = wt - luma_tasks;
  const uint32_t rp = ct / chunks_c, chunk = ct - rp * chunks_c;
  const uint32_t x = chunk * 2048 + lane * 32;  // byte offset in the interleaved UV row
  if constexpr (TO_PLANAR) {
    if (x >= w) return;
    const uint8_t* p = f.s[1] + (size_t)rp * f.sp[1] + x;
    const u32x4 a = ldg<true, u32x4>(p), b = ldg<true, u32x4>(p + 16);  // the lane's 32 contiguous bytes: both halves of each 128-B line are consumed by this wave
    u32x4 u, v;  // even bytes -> U, odd bytes -> V
    u[0] = __builtin_amdgcn_perm(a[1], a[0], 0x06040200u); u[1] = __builtin_amdgcn_perm(a[3], a[2], 0x06040200u);
    u[2] = __builtin_amdgcn_perm(b[1], b[0], 0x06040200u); u[3] = __builtin_amdgcn_perm(b[3], b[2], 0x06040200u);
    v[0] = __builtin_amdgcn_perm(a[1], a[0], 0x07050301u); v[1] = __builtin_amdgcn_perm(a[3], a[2], 0x07050301u);
    v[2] = __builtin_amdgcn_perm(b[1], b[0], 0x07050301u); v[3] = __builtin_amdgcn_perm(b[3], b[2], 0x07050301u);
    stg<true, u32x4>(f.d[1] + (size_t)rp * f.dp[1] + (x >> 1), u);
    stg<true, u32x4>(f.d[2] + (size_t)rp * f.dp[2] + (x >> 1), v);
  } else {
    const uint32_t xc = x < w ? x : w - 32;
    const u32x4 u = ldg<true, u32x4>(f.s[1] + (size_t)rp * f.sp[1] + (xc >> 1));
    const u32x4 v = ldg<true, u32x4>(f.s[2] + (size_t)rp * f.sp[2] + (xc >> 1));
    u32x4* t = tile + wv * 128;
#pragma unroll
    for (int j = 0; j < 2; j++) {
      u32x4 o;  // interleave: U0 V0 U1 V1 | U2 V2 U3 V3 | ...
      o[0] = __builtin_amdgcn_perm(v[2 * j], u[2 * j], 0x05010400u);
      o[1] = __builtin_amdgcn_perm(v[2 * j], u[2 * j], 0x07030602u);
      o[2] = __builtin_amdgcn_perm(v[2 * j + 1], u[2 * j + 1], 0x05010400u);
      o[3] = __builtin_amdgcn_perm(v[2 * j + 1], u[2 * j + 1], 0x07030602u);
      t[lane * 2 + j] = o;
    }
    wave_sync();
    uint8_t* row = f.d[1] + (size_t)rp * f.dp[1];
#pragma unroll
    for (int k = 0; k < 2; k++) {
      const uint32_t off = chunk * 2048 + (k * 64 + lane) * 16;
      if (off < w) stg<true, u32x4>(row + off, t[k * 64 + lane]);
    }
  }
}
template <bool TO_PLANAR>
__global__ __launch_bounds__(256) void k_nv12_yuv420_r16(const BatchArgs args, uint32_t w, uint32_t h, uint32_t chunks_y, uint32_t luma_tasks, uint32_t chunks_c, uint32_t n_tasks) {
  nv12_yuv420_r16_task<TO_PLANAR>(args.f[blockIdx.y], w, h, chunks_y, luma_tasks, chunks_c, n_tasks);
}
template <bool TO_PLANAR>  // single-frame entry: scalar arguments (see VPF_ONE_SRC_PARAMS in vpf_internal.h)
__global__ __launch_bounds__(256) void k_nv12_yuv420_r16_one(VPF_ONE_SRC_PARAMS, uint32_t w, uint32_t h, uint32_t chunks_y, uint32_t luma_tasks, uint32_t chunks_c, uint32_t n_tasks, VPF_ONE_DST_PARAMS) {
  nv12_yuv420_r16_task<TO_PLANAR>(VPF_ONE_FRAME, w, h, chunks_y, luma_tasks, chunks_c, n_tasks);
}

// RGB -> RGB_32F, elementwise over the 3W bytes of a row: a wave takes 1 KiB of bytes as four dense 256-B dword loads
// (all in flight before the first use) and writes four dense 1-KiB runs of floats.
template <int N>
VPF_DEV void u8_to_f32_x4_task(const FrameDesc& f, uint32_t wdwords, uint32_t h, uint32_t chunks_x, uint32_t n_tasks) {
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const uint32_t wt = blockIdx.x * 4 + wv;
  if (wt >= n_tasks) return;
  const uint32_t y = wt / chunks_x, chunk = wt - y * chunks_x;
  const uint8_t* src = f.s[0] + (size_t)y * f.sp[0];
  uint8_t* dst = f.d[0] + (size_t)y * f.dp[0];
  typedef float f32x4 __attribute__((ext_vector_type(4)));
  uint32_t d[N];
#pragma unroll
  for (int j = 0; j < N; j++) {
    const uint32_t i = chunk * (64 * N) + j * 64 + lane;
    d[j] = ldg<true, uint32_t>(src + 4 * (size_t)(i < wdwords ? i : wdwords - 1));
  }
#pragma unroll
  for (int j = 0; j < N; j++) {
    const uint32_t i = chunk * (64 * N) + j * 64 + lane;
    const f32x4 v = {ubyte<0>(d[j]) / 255.0f, ubyte<1>(d[j]) / 255.0f, ubyte<2>(d[j]) / 255.0f, ubyte<3>(d[j]) / 255.0f};
    if (i < wdwords) stg<true, f32x4>(dst + 16 * (size_t)i, v);
  }
}
template <int N>
__global__ __launch_bounds__(256) void k_u8_to_f32_x4(const BatchArgs args, uint32_t wdwords, uint32_t h, uint32_t chunks_x, uint32_t n_tasks) {
  u8_to_f32_x4_task<N>(args.f[blockIdx.y], wdwords, h, chunks_x, n_tasks);
}
template <int N>
__global__ __launch_bounds__(256) void k_u8_to_f32_x4_one(VPF_ONE_SRC_PARAMS, uint32_t wdwords, uint32_t h, uint32_t chunks_x, uint32_t n_tasks, VPF_ONE_DST_PARAMS) {  // single-frame entry: scalar arguments
  u8_to_f32_x4_task<N>(VPF_ONE_FRAME, wdwords, h, chunks_x, n_tasks);
}

// P10 / P12 -> NV12, 16 samples (32 B) per lane -> one dense 1-KiB store per wave; rows as in k_p16_to_8_p8.
VPF_DEV void p16_to_8_x16_task(const FrameDesc& f, uint32_t wsamples, uint32_t h, uint32_t ch, uint32_t chunks_x, uint32_t n_tasks) {
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const uint32_t wt = blockIdx.x * 4 + wv;
  if (wt >= n_tasks) return;
  const uint32_t row = wt / chunks_x, chunk = wt - row * chunks_x;
  const int pl = row >= h;
  const uint32_t y = pl ? row - h : row;
  const uint32_t xs = chunk * 1024 + lane * 16;  // first sample of the lane
  if (xs >= wsamples) return;
  const uint8_t* p = f.s[pl] + (size_t)y * f.sp[pl] + 2 * (size_t)xs;
  const u32x4 a = ldg<true, u32x4>(p), b = ldg<true, u32x4>(p + 16);
  auto two = [](uint32_t lo, uint32_t hi) {
    return (uint32_t)p16_to_8((uint16_t)(lo & 0xffffu)) | ((uint32_t)p16_to_8((uint16_t)(lo >> 16)) << 8) |
           ((uint32_t)p16_to_8((uint16_t)(hi & 0xffffu)) << 16) | ((uint32_t)p16_to_8((uint16_t)(hi >> 16)) << 24);
  };
  const u32x4 o = {two(a[0], a[1]), two(a[2], a[3]), two(b[0], b[1]), two(b[2], b[3])};
  stg<true, u32x4>(f.d[pl] + (size_t)y * f.dp[pl] + xs, o);
}
__global__ __launch_bounds__(256) void k_p16_to_8_x16(const BatchArgs args, uint32_t wsamples, uint32_t h, uint32_t ch, uint32_t chunks_x, uint32_t n_tasks) {
  p16_to_8_x16_task(args.f[blockIdx.y], wsamples, h, ch, chunks_x, n_tasks);
}
__global__ __launch_bounds__(256) void k_p16_to_8_x16_one(VPF_ONE_SRC_PARAMS, uint32_t wsamples, uint32_t h, uint32_t ch, uint32_t chunks_x, uint32_t n_tasks, VPF_ONE_DST_PARAMS) {  // single-frame entry: scalar arguments
  p16_to_8_x16_task(VPF_ONE_FRAME, wsamples, h, ch, chunks_x, n_tasks);
}

// host side: convert_plan (vpf_convert_plan.h) decides, this launches the instantiation it names
static void dispatch_relayout(hipStream_t st, const ConvertPlan& P, const BatchArgs& a) {
  const dim3 grid(P.gx, P.gy, P.gz);
  const FrameDesc& f0 = a.f[0];
  const uint32_t* s = P.a;
  auto modes = [&](auto&& f) { with_value<0, 1, 2>(P.mode, f); };
  switch (P.form) {
    case CF_NV12_YUV420_R16:
      with_bool(P.mode != 0, [&](auto TO_PLANAR) {
        if (P.one) VPF_LAUNCH_T(k_nv12_yuv420_r16_one, (TO_PLANAR), grid, 0, st, VPF_ONE_SRC_ARGS(f0), s[0], s[1], s[2], s[3], s[4], s[5], VPF_ONE_DST_ARGS(f0));
        else VPF_LAUNCH_T(k_nv12_yuv420_r16, (TO_PLANAR), grid, 0, st, a, s[0], s[1], s[2], s[3], s[4], s[5]);
      });
      break;
    case CF_NV12_YUV420_P16: with_bool(P.mode != 0, [&](auto TO_PLANAR) { VPF_LAUNCH_T(k_nv12_yuv420_p16, (TO_PLANAR), grid, 0, st, a, s[0], s[1], s[2]); }); break;
    case CF_RGB_RELAYOUT_R16:
      modes([&](auto MODE) {
        if (P.one) VPF_LAUNCH_T(k_rgb_relayout_r16_one, (MODE), grid, 0, st, VPF_ONE_SRC_ARGS(f0), s[0], s[1], s[2], s[3], VPF_ONE_DST_ARGS(f0));
        else VPF_LAUNCH_T(k_rgb_relayout_r16, (MODE), grid, 0, st, a, s[0], s[1], s[2], s[3]);
      });
      break;
    case CF_RGB_RELAYOUT_P4: modes([&](auto MODE) { VPF_LAUNCH_T(k_rgb_relayout_p4, (MODE), grid, 0, st, a, s[0], s[1], s[2]); }); break;
    case CF_COPY_PLANE_P16: with_bool(P.mode != 0, [&](auto FILL) { VPF_LAUNCH_T(k_copy_plane_p16, (FILL), grid, 0, st, a, s[0], s[1], s[2]); }); break;
    case CF_U8_TO_F32_X4:
      if (P.one) VPF_LAUNCH(k_u8_to_f32_x4_one<4>, grid, dim3(256), 0, st, VPF_ONE_SRC_ARGS(f0), s[0], s[1], s[2], s[3], VPF_ONE_DST_ARGS(f0));
      else VPF_LAUNCH(k_u8_to_f32_x4<4>, grid, dim3(256), 0, st, a, s[0], s[1], s[2], s[3]);
      break;
    case CF_U8_TO_F32_P4: VPF_LAUNCH(k_u8_to_f32_p4, grid, dim3(256), 0, st, a, s[0], s[1], s[2]); break;
    case CF_RGB32F_PLANAR_R4:
      if (P.one) VPF_LAUNCH(k_rgb32f_planar_r4_one, grid, dim3(256), 0, st, VPF_ONE_SRC_ARGS(f0), s[0], s[1], s[2], s[3], VPF_ONE_DST_ARGS(f0));
      else VPF_LAUNCH(k_rgb32f_planar_r4, grid, dim3(256), 0, st, a, s[0], s[1], s[2], s[3]);
      break;
    case CF_P16_TO_8_X16:
      if (P.one) VPF_LAUNCH(k_p16_to_8_x16_one, grid, dim3(256), 0, st, VPF_ONE_SRC_ARGS(f0), s[0], s[1], s[2], s[3], s[4], VPF_ONE_DST_ARGS(f0));
      else VPF_LAUNCH(k_p16_to_8_x16, grid, dim3(256), 0, st, a, s[0], s[1], s[2], s[3], s[4]);
      break;
    case CF_P16_TO_8_P8: VPF_LAUNCH(k_p16_to_8_p8, grid, dim3(256), 0, st, a, s[0], s[1], s[2], s[3]); break;
    case CF_GRAY_R16:
      modes([&](auto SRC) {
        if (P.one) VPF_LAUNCH_T(k_gray_r16_one, (SRC), grid, 0, st, VPF_ONE_SRC_ARGS(f0), s[0], s[1], s[2], s[3], VPF_ONE_DST_ARGS(f0));
        else VPF_LAUNCH_T(k_gray_r16, (SRC), grid, 0, st, a, s[0], s[1], s[2], s[3]);
      });
      break;
    case CF_GRAY_P4: modes([&](auto SRC) { VPF_LAUNCH_T(k_gray_p4, (SRC), grid, 0, st, a, s[0], s[1], s[2]); }); break;
    default:  // (every op but OP_PLANAR_SWAP, which the plan never names)
      with_value<OP_NV12_YUV420, OP_YUV420_NV12, OP_RGB_PLANAR, OP_PLANAR_RGB, OP_SWAP_RB, OP_COPY_Y, OP_Y_YUV444, OP_RGB_RGB32F, OP_RGB32F_PLANAR, OP_P16_NV12, OP_RGB_GRAY,
                 OP_BGR_GRAY, OP_PLANAR_GRAY>(P.mode, [&](auto OP) { VPF_LAUNCH_T(k_relayout_generic, (OP), grid, 0, st, a, s[0], s[1]); });
  }
}

hipError_t launch_relayout(hipStream_t st, int sf, int df, uint32_t w, uint32_t h, uint32_t n, const BatchArgs& a) {
  const ConvertPlan P = convert_plan(convert_shape(CONVERT_RELAYOUT, sf, df, w, h, n, a, tuning(VPF_TUNE_NV12_RGB_VARIANT)));
  if (!P.ok) return hipErrorInvalidValue;
  if (P.swap_src02 || P.swap_dst02) {  // BGR <-> RGB_PLANAR: the RGB kernel with planes 0 and 2 of the planar side exchanged
    BatchArgs b = a;
    for (uint32_t i = 0; i < n; i++) {
      if (P.swap_src02) { std::swap(b.f[i].s[0], b.f[i].s[2]); std::swap(b.f[i].sp[0], b.f[i].sp[2]); }
      else { std::swap(b.f[i].d[0], b.f[i].d[2]); std::swap(b.f[i].dp[0], b.f[i].dp[2]); }
    }
    dispatch_relayout(st, P, b);
  } else {
    dispatch_relayout(st, P, a);
  }
  return hipGetLastError();
}

}  // namespace vpf
