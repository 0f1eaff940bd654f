// k_yuv2rgb.hip — NV12 / YUV420 / YUV444 -> RGB / BGR / RGB_PLANAR for gfx950 (MI355X).
//
// Replaces the NPP calls behind nv12_rgb / nv12_bgr / yuv420_rgb / yuv420_bgr / yuv444_rgb /
// yuv444_bgr (reference: src/TC/src/TasksColorCvt.cpp:53-108,122-182,322-369,383-430,444-550) and
// fuses nv12_rgb + rgb8_deinterleave (:1059-1088) into one pass for NV12 -> RGB_PLANAR.
//
// This is HBM-bound pointwise work (4.5 B/px: 1.5 read, 3 written), so the design is about memory
// instructions, not math:
//   * a wave owns a strip of one or more ROW PAIRS so each UV sample is read once and serves its
//     2x2 luma quad out of registers (no second trip to memory, no LDS needed for the stencil);
//   * p4 kernels: a lane owns 4 pixels -> 1 dword of Y per row, 1 dword of UV, and writes 12 B per
//     row.  A wave's loads are 256 contiguous bytes, its stores 768 contiguous bytes: every memory
//     instruction is fully coalesced with no cross-lane traffic at all;
//   * p16 kernels: a lane owns 16 pixels -> dwordx4 loads; the 48 B/row it produces are transposed
//     through a wave-private LDS tile so every global store is a dense 1 KiB dwordx4 wave store;
//   * math is fp32 FMA on v_cvt_f32_ubyteN operands, rounded + saturated + byte-packed by
//     v_cvt_pk_u8_f32: 1 cvt + 3 FMA + 3 pack ops per pixel;
//   * `BatchArgs` carries up to 32 frames in the kernarg segment, blockIdx.y selects the frame, so
//     one dispatch streams ~600 MB and the ~2 us kernel boundary is amortised.
#include "k_job_launch.h"
#include "k_yuv2rgb_tasks.h"

namespace vpf {

// batched p4 entry (the 4-B-aligned / irregular-size fast path): 1 row pair per task, cvt_pk pack, non-temporal loads + stores
template <int SRC, int DST>
__global__ __launch_bounds__(256) void k_yuv420_rgb_p4(const BatchArgs args, const Yuv2RgbCoef c, uint32_t w,
                                                       uint32_t h, uint32_t chunks_x, uint32_t n_tasks) {
  yuv420_rgb_p4_task<SRC, DST, 1, 1, true, true, 0>(args.f[blockIdx.y], c, w, h, chunks_x, n_tasks);
}
template <int SRC, int DST>  // single-frame entry of the default p4 form (irregular sizes / alignments): scalar arguments
__global__ __launch_bounds__(256) void k_yuv420_rgb_p4_one(VPF_ONE_SRC_PARAMS, uint32_t w, uint32_t h, uint32_t chunks_x, uint32_t n_tasks,
                                                           VPF_ONE_DST_PARAMS, const Yuv2RgbCoef c) {
  yuv420_rgb_p4_task<SRC, DST, 1, 1, true, true, 0>(VPF_ONE_FRAME, c, w, h, chunks_x, n_tasks);
}

// batched p16 entry: up to 32 frame descriptors by value in the kernarg segment, blockIdx.y = frame.  NTS = non-temporal
// stores (false: allocating stores, VPF_EXEC_DST_REUSED); BALLAST_KB pads the LDS footprint so that 4 instead of 6 workgroups are
// resident per CU (+1-2 % on launches that run long enough, tools/write_probe.hip)
template <int DST, bool NTS, int BALLAST_KB, int SRC>
__global__ __launch_bounds__(256) void k_nv12_rgb_p16(const BatchArgs args, const Yuv2RgbCoef c, uint32_t w,
                                                      uint32_t h, uint32_t chunks_x, uint32_t n_tasks) {
  p16_task<DST, 1, true, NTS, true, 4, BALLAST_KB, false, SRC>(args.f[blockIdx.y], c, w, h, chunks_x, n_tasks);
}
// single-frame entry (one Execute() = one launch): the frame arrives as scalar kernel arguments, source side first, which
// the dispatcher preloads into SGPRs (-amdgpu-kernarg-preload-count): the wave's first loads no longer wait for a
// scalar-cache round trip to the kernarg segment — worth 0.5-0.8 us on a kernel that lasts 6-7 us
template <int DST, bool NTS, int SRC>
__global__ __launch_bounds__(256) void k_nv12_rgb_p16_one(VPF_ONE_SRC_PARAMS, uint32_t w, uint32_t h, uint32_t chunks_x, uint32_t n_tasks,
                                                          VPF_ONE_DST_PARAMS, const Yuv2RgbCoef c) {
  p16_task<DST, 1, true, NTS, true, 4, 0, false, SRC>(VPF_ONE_FRAME, c, w, h, chunks_x, n_tasks);
}

// the same conversion with the blocks numbered straight through the picture (p16x_task): the default for packed outputs of frames at least 1024 px wide
template <int DST, bool NTS, int BALLAST_KB, int SRC>
__global__ __launch_bounds__(256) void k_nv12_rgb_p16x(const BatchArgs args, const Yuv2RgbCoef c, uint32_t bpr, uint32_t n_blocks) {
  p16x_task<DST, NTS, BALLAST_KB, SRC>(args.f[blockIdx.y], c, bpr, n_blocks);
}
template <int DST, bool NTS, int SRC>
__global__ __launch_bounds__(256) void k_nv12_rgb_p16x_one(VPF_ONE_SRC_PARAMS, uint32_t bpr, uint32_t n_blocks, VPF_ONE_DST_PARAMS, const Yuv2RgbCoef c) {
  p16x_task<DST, NTS, 0, SRC>(VPF_ONE_FRAME, c, bpr, n_blocks);
}

template <bool NTS, int SRC = FC_NV12>
__global__ __launch_bounds__(256) void k_nv12_planar_r16(const BatchArgs args, const Yuv2RgbCoef c, uint32_t w, uint32_t h,
                                                         uint32_t chunks_x, uint32_t n_tasks) {
  planar_r16_task<NTS, SRC>(args.f[blockIdx.y], c, w, h, chunks_x, n_tasks);
}
template <bool NTS, int SRC>  // single-frame entry: scalar arguments (see VPF_ONE_SRC_PARAMS)
__global__ __launch_bounds__(256) void k_nv12_planar_r16_one(VPF_ONE_SRC_PARAMS, uint32_t w, uint32_t h, uint32_t chunks_x, uint32_t n_tasks,
                                                             VPF_ONE_DST_PARAMS, const Yuv2RgbCoef c) {
  planar_r16_task<NTS, SRC>(VPF_ONE_FRAME, c, w, h, chunks_x, n_tasks);
}


// ---------------------------------------------------------------------------------------------
// YUV444 (three full planes) -> RGB/BGR/PLANAR, 4 px per lane, one row per task.
// Requires w % 4 == 0 and 4-byte aligned planes.
// ---------------------------------------------------------------------------------------------
template <int DST, int PACK>
__global__ __launch_bounds__(256) void k_yuv444_rgb_p4(const BatchArgs args, const Yuv2RgbCoef c, uint32_t w,
                                                       uint32_t h, uint32_t groups_x) {
  const FrameDesc& f = args.f[blockIdx.z];
  const uint32_t gx = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
  if (gx >= groups_x || y >= h) return;
  const uint32_t x = gx * 4;
  const uint32_t yd = ldg<false, uint32_t>(f.s[0] + (size_t)y * f.sp[0] + x);
  const uint32_t ud = ldg<false, uint32_t>(f.s[1] + (size_t)y * f.sp[1] + x);
  const uint32_t vd = ldg<false, uint32_t>(f.s[2] + (size_t)y * f.sp[2] + x);
  const Chroma k0 = chroma_terms(c, ubyte<0>(ud), ubyte<0>(vd)), k1 = chroma_terms(c, ubyte<1>(ud), ubyte<1>(vd));
  const Chroma k2 = chroma_terms(c, ubyte<2>(ud), ubyte<2>(vd)), k3 = chroma_terms(c, ubyte<3>(ud), ubyte<3>(vd));
  Quad q;
  const float y0 = ubyte<0>(yd), y1 = ubyte<1>(yd), y2 = ubyte<2>(yd), y3 = ubyte<3>(yd);
  q.r[0] = __builtin_fmaf(y0, c.cy, k0.rc); q.g[0] = __builtin_fmaf(y0, c.cy, k0.gc); q.b[0] = __builtin_fmaf(y0, c.cy, k0.bc);
  q.r[1] = __builtin_fmaf(y1, c.cy, k1.rc); q.g[1] = __builtin_fmaf(y1, c.cy, k1.gc); q.b[1] = __builtin_fmaf(y1, c.cy, k1.bc);
  q.r[2] = __builtin_fmaf(y2, c.cy, k2.rc); q.g[2] = __builtin_fmaf(y2, c.cy, k2.gc); q.b[2] = __builtin_fmaf(y2, c.cy, k2.bc);
  q.r[3] = __builtin_fmaf(y3, c.cy, k3.rc); q.g[3] = __builtin_fmaf(y3, c.cy, k3.gc); q.b[3] = __builtin_fmaf(y3, c.cy, k3.bc);
  if constexpr (DST == FC_PLANAR) {
    stg<false, uint32_t>(f.d[0] + (size_t)y * f.dp[0] + x, pack4<PACK>(q.r[0], q.r[1], q.r[2], q.r[3]));
    stg<false, uint32_t>(f.d[1] + (size_t)y * f.dp[1] + x, pack4<PACK>(q.g[0], q.g[1], q.g[2], q.g[3]));
    stg<false, uint32_t>(f.d[2] + (size_t)y * f.dp[2] + x, pack4<PACK>(q.b[0], q.b[1], q.b[2], q.b[3]));
  } else {
    uint32_t d0, d1, d2;
    pack_rgb12<DST, PACK>(q, d0, d1, d2);
    stg3<false>(f.d[0] + (size_t)y * f.dp[0] + 3 * (size_t)x, d0, d1, d2);
  }
}

// YUV444 -> RGB/BGR/PLANAR, r16: one row x 1024 px per wave, three dense 1-KiB plane loads, three dense 1-KiB stores
// (packed outputs through store_run48).  Requires w % 16 == 0 and 16-B aligned planes / pitches.
template <int DST>
VPF_DEV void yuv444_rgb_r16_task(const FrameDesc& f, const Yuv2RgbCoef& c, uint32_t w, uint32_t h, uint32_t chunks_x, uint32_t n_tasks) {
  __shared__ u32x4 tile[DST == FC_PLANAR ? 1 : 4 * 192];
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const uint32_t wt = blockIdx.x * 4 + wv;
  if (wt >= n_tasks) return;
  const uint32_t y = wt / chunks_x, chunk = wt - y * chunks_x;
  const uint32_t x = chunk * 1024 + lane * 16;
  if (DST == FC_PLANAR && x >= w) return;
  const uint32_t xc = x < w ? x : w - 16;  // clamped lanes compute a duplicate that store_run48 never writes
  const u32x4 yq = ldg<true, u32x4>(f.s[0] + (size_t)y * f.sp[0] + xc);
  const u32x4 uq = ldg<true, u32x4>(f.s[1] + (size_t)y * f.sp[1] + xc);
  const u32x4 vq = ldg<true, u32x4>(f.s[2] + (size_t)y * f.sp[2] + xc);
  uint32_t o[12];
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const uint32_t yd = yq[j], ud = uq[j], vd = vq[j];
    const Chroma k0 = chroma_terms(c, ubyte<0>(ud), ubyte<0>(vd)), k1 = chroma_terms(c, ubyte<1>(ud), ubyte<1>(vd));
    const Chroma k2 = chroma_terms(c, ubyte<2>(ud), ubyte<2>(vd)), k3 = chroma_terms(c, ubyte<3>(ud), ubyte<3>(vd));
    Quad q;
    const float y0 = ubyte<0>(yd), y1 = ubyte<1>(yd), y2 = ubyte<2>(yd), y3 = ubyte<3>(yd);
    q.r[0] = __builtin_fmaf(y0, c.cy, k0.rc); q.g[0] = __builtin_fmaf(y0, c.cy, k0.gc); q.b[0] = __builtin_fmaf(y0, c.cy, k0.bc);
    q.r[1] = __builtin_fmaf(y1, c.cy, k1.rc); q.g[1] = __builtin_fmaf(y1, c.cy, k1.gc); q.b[1] = __builtin_fmaf(y1, c.cy, k1.bc);
    q.r[2] = __builtin_fmaf(y2, c.cy, k2.rc); q.g[2] = __builtin_fmaf(y2, c.cy, k2.gc); q.b[2] = __builtin_fmaf(y2, c.cy, k2.bc);
    q.r[3] = __builtin_fmaf(y3, c.cy, k3.rc); q.g[3] = __builtin_fmaf(y3, c.cy, k3.gc); q.b[3] = __builtin_fmaf(y3, c.cy, k3.bc);
    if constexpr (DST == FC_PLANAR) {
      o[j] = pack4<1>(q.r[0], q.r[1], q.r[2], q.r[3]);
      o[4 + j] = pack4<1>(q.g[0], q.g[1], q.g[2], q.g[3]);
      o[8 + j] = pack4<1>(q.b[0], q.b[1], q.b[2], q.b[3]);
    } else {
      pack_rgb12<DST, 1>(q, o[3 * j], o[3 * j + 1], o[3 * j + 2]);
    }
  }
  if constexpr (DST == FC_PLANAR) {
#pragma unroll
    for (int k = 0; k < 3; k++)
      stg<true, u32x4>(f.d[k] + (size_t)y * f.dp[k] + x, u32x4{o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3]});
  } else {
    store_run48(tile + wv * 192, f.d[0] + (size_t)y * f.dp[0], chunk * 3072, 3 * w, lane, o);
  }
}
template <int DST>
__global__ __launch_bounds__(256) void k_yuv444_rgb_r16(const BatchArgs args, const Yuv2RgbCoef c, uint32_t w, uint32_t h, uint32_t chunks_x, uint32_t n_tasks) {
  yuv444_rgb_r16_task<DST>(args.f[blockIdx.y], c, w, h, chunks_x, n_tasks);
}
template <int DST>  // single-frame entry: scalar arguments (see VPF_ONE_SRC_PARAMS in vpf_internal.h)
__global__ __launch_bounds__(256) void k_yuv444_rgb_r16_one(VPF_ONE_SRC_PARAMS, uint32_t w, uint32_t h, uint32_t chunks_x, uint32_t n_tasks, VPF_ONE_DST_PARAMS, const Yuv2RgbCoef c) {
  yuv444_rgb_r16_task<DST>(VPF_ONE_FRAME, c, w, h, chunks_x, n_tasks);
}

// ---------------------------------------------------------------------------------------------
// generic: any size, any alignment.  One thread per 2x2 quad, byte accesses, full bounds checks.
// ---------------------------------------------------------------------------------------------
template <int SRC, int DST>
__global__ __launch_bounds__(256) void k_yuv_rgb_generic(const BatchArgs args, const Yuv2RgbCoef c, uint32_t w,
                                                         uint32_t h) {
  const FrameDesc& f = args.f[blockIdx.z];
  const uint32_t qx = blockIdx.x * 64 + (threadIdx.x & 63), qy = blockIdx.y * 4 + (threadIdx.x >> 6);
  const uint32_t x0 = 2 * qx, y0 = 2 * qy;
  if (x0 >= w || y0 >= h) return;
  float u = 0, v = 0;
  if constexpr (SRC == FC_NV12) {
    const uint8_t* p = f.s[1] + (size_t)qy * f.sp[1] + x0;
    u = p[0]; v = p[1];
  } else if constexpr (SRC == FC_YUV420) {
    u = f.s[1][(size_t)qy * f.sp[1] + qx]; v = f.s[2][(size_t)qy * f.sp[2] + qx];
  }
  Chroma k = chroma_terms(c, u, v);
  for (uint32_t dy = 0; dy < 2; dy++)
    for (uint32_t dx = 0; dx < 2; dx++) {
      const uint32_t x = x0 + dx, y = y0 + dy;
      if (x >= w || y >= h) continue;
      if constexpr (SRC == FC_YUV444) {
        k = chroma_terms(c, (float)f.s[1][(size_t)y * f.sp[1] + x], (float)f.s[2][(size_t)y * f.sp[2] + x]);
      }
      const float yf = (float)f.s[0][(size_t)y * f.sp[0] + x];
      const uint8_t r = (uint8_t)sat_rne(__builtin_fmaf(yf, c.cy, k.rc));
      const uint8_t g = (uint8_t)sat_rne(__builtin_fmaf(yf, c.cy, k.gc));
      const uint8_t b = (uint8_t)sat_rne(__builtin_fmaf(yf, c.cy, k.bc));
      if constexpr (DST == FC_PLANAR) {
        f.d[0][(size_t)y * f.dp[0] + x] = r; f.d[1][(size_t)y * f.dp[1] + x] = g; f.d[2][(size_t)y * f.dp[2] + x] = b;
      } else {
        uint8_t* o = f.d[0] + (size_t)y * f.dp[0] + 3 * (size_t)x;
        o[0] = (DST == FC_BGR) ? b : r; o[1] = g; o[2] = (DST == FC_BGR) ? r : b;
      }
    }
}


// ---------------------------------------------------------------------------------------------
// host side: convert_plan (vpf_convert_plan.h) decides, this launches the instantiation it names
// ---------------------------------------------------------------------------------------------
// f(SRC, DST) as constants: FC_NV12 / FC_YUV420 / FC_YUV444 into FC_RGB / FC_BGR / FC_PLANAR (the plan has refused every other class)
template <class F>
static void with_yuv_src_dst(int src_fc, int dst_fc, F&& f) {
  with_value<FC_NV12, FC_YUV420, FC_YUV444>(src_fc, [&](auto src) { with_value<FC_RGB, FC_BGR, FC_PLANAR>(dst_fc, [&](auto dst) { f(src, dst); }); });
}

hipError_t launch_yuv_to_rgb(hipStream_t st, int src_fc, int dst_fc, const Yuv2RgbCoef& c, uint32_t w, uint32_t h,
                             uint32_t n, const BatchArgs& a, int variant, bool dst_reused) {
  ConvertShape q = convert_shape(CONVERT_YUV2RGB, src_fc, dst_fc, w, h, n, a, variant);
  q.dst_reused = dst_reused;
  const ConvertPlan P = convert_plan(q);
  if (!P.ok) return hipErrorInvalidValue;
  const dim3 grid(P.gx, P.gy, P.gz);
  const FrameDesc& f0 = a.f[0];
  const uint32_t* s = P.a;
  with_yuv_src_dst(P.src, P.dst, [&](auto src, auto dst) {
    constexpr int SRC = decltype(src)::value, DST = decltype(dst)::value;
    // (the guards keep the instantiations to the ones the plan can name: no r16 / p16 / p4 form of a 4:4:4 source, no planar p16x)
    if constexpr (SRC != FC_YUV444) {
      if (P.form == CF_NV12_PLANAR_R16)
        with_bool(P.nts, [&](auto NTS) {
          if (P.one) VPF_LAUNCH_T(k_nv12_planar_r16_one, (NTS, SRC), grid, 0, st, VPF_ONE_SRC_ARGS(f0), s[0], s[1], s[2], s[3], VPF_ONE_DST_ARGS(f0), c);
          else VPF_LAUNCH_T(k_nv12_planar_r16, (NTS, SRC), grid, 0, st, a, c, s[0], s[1], s[2], s[3]);
        });
      if constexpr (DST != FC_PLANAR)
        if (P.form == CF_NV12_RGB_P16X) {
          if (P.one) VPF_LAUNCH_T(k_nv12_rgb_p16x_one, (DST, true, SRC), grid, 0, st, VPF_ONE_SRC_ARGS(f0), s[0], s[1], VPF_ONE_DST_ARGS(f0), c);
          else if (P.ballast) VPF_LAUNCH_T(k_nv12_rgb_p16x, (DST, true, 16, SRC), grid, 0, st, a, c, s[0], s[1]);
          else VPF_LAUNCH_T(k_nv12_rgb_p16x, (DST, true, 0, SRC), grid, 0, st, a, c, s[0], s[1]);
        }
      if (P.form == CF_NV12_RGB_P16) {
        if (P.ballast) VPF_LAUNCH_T(k_nv12_rgb_p16, (DST, true, 16, SRC), grid, 0, st, a, c, s[0], s[1], s[2], s[3]);  // (non-temporal stores only)
        else with_bool(P.nts, [&](auto NTS) {
          if (P.one) VPF_LAUNCH_T(k_nv12_rgb_p16_one, (DST, NTS, SRC), grid, 0, st, VPF_ONE_SRC_ARGS(f0), s[0], s[1], s[2], s[3], VPF_ONE_DST_ARGS(f0), c);
          else VPF_LAUNCH_T(k_nv12_rgb_p16, (DST, NTS, 0, SRC), grid, 0, st, a, c, s[0], s[1], s[2], s[3]);
        });
      }
      if (P.form == CF_YUV420_RGB_P4) {
        if (P.one) VPF_LAUNCH_T(k_yuv420_rgb_p4_one, (SRC, DST), grid, 0, st, VPF_ONE_SRC_ARGS(f0), s[0], s[1], s[2], s[3], VPF_ONE_DST_ARGS(f0), c);
        else VPF_LAUNCH_T(k_yuv420_rgb_p4, (SRC, DST), grid, 0, st, a, c, s[0], s[1], s[2], s[3]);
      }
    } else {
      if (P.form == CF_YUV444_RGB_R16) {
        if (P.one) VPF_LAUNCH_T(k_yuv444_rgb_r16_one, (DST), grid, 0, st, VPF_ONE_SRC_ARGS(f0), s[0], s[1], s[2], s[3], VPF_ONE_DST_ARGS(f0), c);
        else VPF_LAUNCH_T(k_yuv444_rgb_r16, (DST), grid, 0, st, a, c, s[0], s[1], s[2], s[3]);
      }
      if (P.form == CF_YUV444_RGB_P4) VPF_LAUNCH_T(k_yuv444_rgb_p4, (DST, 1), grid, 0, st, a, c, s[0], s[1], s[2]);
    }
    if (P.form == CF_YUV_RGB_GENERIC) VPF_LAUNCH_T(k_yuv_rgb_generic, (SRC, DST), grid, 0, st, a, c, s[0], s[1]);
  });
  return hipGetLastError();
}

}  // namespace vpf
