// k_job_launch.h — the host side the fused tensor launchers share (k_convert_roi.hip, k_convert_letterbox.hip, k_convert_warp.hip, k_convert_persp.hip,
// their device-table forms, the convert and relayout launchers of k_yuv2rgb.hip, k_rgb2yuv.hip and k_relayout.hip, the whole-frame launch_convert_resize and the
// plain launch_resize_planned): the frame table's alignment bits, the run-time -> template-argument dispatch, the launch of the instantiation it picked
// and, for the eight per-job launchers, what they share around job_plan (vpf_job_plan.h, where the policy stands: caps, staged or per tap, grids, LDS,
// the alignment mask): filling the shape, filling the two zeroed job tables from the plan's per-job assignment, and the channels-last staging of a
// dispatch.  Inline functions, function templates over callables and two launch macros: nothing is type-erased and nothing allocates.
#ifndef VPF_K_JOB_LAUNCH_H_
#define VPF_K_JOB_LAUNCH_H_
#include <cstdio>
#include <cstring>
#include <type_traits>

#include "vpf_convert_plan.h"
#include "vpf_internal.h"
#include "vpf_job_plan.h"

namespace vpf {

// f(SRC, DST): the source class and the destination layout as std::integral_constant<int, ...>, usable as template arguments
template <class F>
inline void with_src_dst(int src_fc, bool nhwc, F&& f) {
  auto layout = [&](auto src) {
    if (nhwc) f(src, std::integral_constant<int, FC_TENSOR_NHWC>{});
    else f(src, std::integral_constant<int, FC_TENSOR>{});
  };
  if (src_fc == FC_NV12) layout(std::integral_constant<int, FC_NV12>{});
  else if (src_fc == FC_P16) layout(std::integral_constant<int, FC_P16>{});
  else layout(std::integral_constant<int, FC_YUV420>{});
}
// f(std::true_type / std::false_type)
template <class F>
inline void with_bool(bool b, F&& f) {
  if (b) f(std::true_type{});
  else f(std::false_type{});
}

// f(DT): the tensor dtype as std::integral_constant<int, VPF_TENSOR_*>; false, and f not called, for any other value
template <class F>
inline bool with_tensor_dtype(uint32_t dtype, F&& f) {
  switch (dtype) {
    case VPF_TENSOR_F32: f(std::integral_constant<int, VPF_TENSOR_F32>{}); return true;
    case VPF_TENSOR_F16: f(std::integral_constant<int, VPF_TENSOR_F16>{}); return true;
    case VPF_TENSOR_BF16: f(std::integral_constant<int, VPF_TENSOR_BF16>{}); return true;
    default: return false;
  }
}

// VPF_LAUNCH for the 256-lane instantiation K<TARGS> a dispatcher above picked: VPF_LAUNCH_T(k_roi_strip, (S, D), grid, lds, st, args...).  The
// selection log (VPF_HIP_LOG=2, roctx markers) gets the template-id the code object and a profiler show — "(k_roi_strip<7, 8>)": FC_NV12 = 0,
// FC_YUV420 = 1, FC_YUV444 = 2, FC_RGB = 3, FC_BGR = 4, FC_PLANAR = 5, FC_P16 = 7, FC_TENSOR = 6, FC_TENSOR_NHWC = 8; bools as true / false —
// written from the same K and TARGS tokens the launch is.
inline int put_targ(char* p, size_t n, int v) { return std::snprintf(p, n, "%d, ", v); }
inline int put_targ(char* p, size_t n, bool v) { return std::snprintf(p, n, "%s, ", v ? "true" : "false"); }
template <class T> struct TableName {};  // a frame table as a template argument: "BatchArgsT<32>", "BatchArgsTE<128>"
template <int CAP> inline int put_targ(char* p, size_t n, TableName<BatchArgsT<CAP>>) { return std::snprintf(p, n, "BatchArgsT<%d>, ", CAP); }
template <int CAP> inline int put_targ(char* p, size_t n, TableName<BatchArgsTE<CAP>>) { return std::snprintf(p, n, "BatchArgsTE<%d>, ", CAP); }
template <class T, T V> inline int put_targ(char* p, size_t n, std::integral_constant<T, V>) { return put_targ(p, n, V); }
// (`family` may open a template-id of its own, the task a generic kernel runs — "k_plane_batch<TileTaskF32": every bracket it opens is closed behind the arguments)
template <class... T>  // T: std::integral_constant<int or bool, ...>, TableName<...>
inline void note_instantiation(const char* family, T... targs) {
  char label[96];
  size_t o = (size_t)std::snprintf(label, sizeof(label), "(%s<", family);
  ((o += (size_t)put_targ(label + o, sizeof(label) - o, targs)), ...);
  o -= 2;  // (over the last ", ")
  for (const char* c = family; *c && o + 3 < sizeof(label); c++)
    if (*c == '<') label[o++] = '>';
  std::snprintf(label + o, sizeof(label) - o, ">)");
  note_kernel(label);
}
#define VPF_TARGS(...) __VA_ARGS__
#define VPF_LAUNCH_T(K, TARGS, GRID, LDS, ST, ...) VPF_LAUNCH_TN(K, TARGS, GRID, dim3(256), LDS, ST, __VA_ARGS__)
// ... with the workgroup size as an argument (the tiled resize kernels: 64 lanes x waves per workgroup)
#define VPF_LAUNCH_TN(K, TARGS, GRID, BLOCK, LDS, ST, ...)                                                 \
  do {                                                                                                     \
    if (vpf::log_level() >= 2 || vpf::trace_on()) vpf::note_instantiation(#K, VPF_TARGS TARGS);            \
    (void)hipGetLastError(); /* (sticky per thread: see VPF_LAUNCH) */                                     \
    hipLaunchKernelGGL((K<VPF_TARGS TARGS>), GRID, BLOCK, LDS, ST, __VA_ARGS__);                           \
  } while (0)
// ... for the kernels whose LAST template argument is the type of their first argument, the frame table (with_frame_table below):
// VPF_LAUNCH_TB(k_convert_strip_wg, (S, D, R), table, grid, lds, st, c, ...) launches and logs "(k_convert_strip_wg<0, 8, 2, BatchArgsTE<32>>)"
#define VPF_LAUNCH_TB(K, TARGS, TABLE, GRID, LDS, ST, ...)                                                                             \
  do {                                                                                                                                 \
    using Table_ = std::decay_t<decltype(TABLE)>;                                                                                      \
    if (vpf::log_level() >= 2 || vpf::trace_on()) vpf::note_instantiation(#K, VPF_TARGS TARGS, vpf::TableName<Table_>{});              \
    (void)hipGetLastError();                                                                                                           \
    hipLaunchKernelGGL((K<VPF_TARGS TARGS, Table_>), GRID, dim3(256), LDS, ST, TABLE, __VA_ARGS__);                                     \
  } while (0)

// ---- the whole-frame fused launch (k_convert_resize.hip)
// f(SRC, DST) for the legal pairs: FC_NV12 / FC_YUV420 into the five destination classes (any class but the four named ones counts as
// FC_PLANAR), FC_P16 into the two tensor classes; f is not called for anything else
template <class F>
inline void with_fused_src_dst(int src_fc, int dst_fc, F&& f) {
  auto dst = [&](auto src) {
    if (dst_fc == FC_TENSOR_NHWC) f(src, std::integral_constant<int, FC_TENSOR_NHWC>{});
    else if (dst_fc == FC_TENSOR) f(src, std::integral_constant<int, FC_TENSOR>{});
    else if constexpr (decltype(src)::value != FC_P16) {
      if (dst_fc == FC_RGB) f(src, std::integral_constant<int, FC_RGB>{});
      else if (dst_fc == FC_BGR) f(src, std::integral_constant<int, FC_BGR>{});
      else f(src, std::integral_constant<int, FC_PLANAR>{});
    }
  };
  if (src_fc == FC_NV12) dst(std::integral_constant<int, FC_NV12>{});
  else if (src_fc == FC_YUV420) dst(std::integral_constant<int, FC_YUV420>{});
  else if (src_fc == FC_P16) dst(std::integral_constant<int, FC_P16>{});
}
// f(R): a band height out of the descending list RS..., the last one for any other value — with_rows<16, 8, 4, 2>(r, f), with_rows<1, 2>(it, f)
template <int R0, int... RS, class F>
inline void with_rows(int r, F&& f) {
  if constexpr (sizeof...(RS) == 0) f(std::integral_constant<int, R0>{});
  else if (r == R0) f(std::integral_constant<int, R0>{});
  else with_rows<RS...>(r, f);
}
// ... under a neutral name for values that are no band heights: the plain resize dispatch (k_resize.hip) picks channel counts, staging passes,
// waves per workgroup and filters with it — with_value<1, 2, 3>(ch, f), with_value<8, 4>(wpb, f); f(V), the last one for any other value
template <int... VS, class F>
inline void with_value(int v, F&& f) { with_rows<VS...>(v, f); }
// f(table, lds): the frame table a batch kernel of destination class DST takes for the first n frames of `a` — BatchArgs / BatchArgsL for the
// 8-bit classes, for the tensor classes BatchArgsTE<32> / <128> (entries up to the next multiple of 8 are defined, vpf_abi.hip) with the
// epilogue behind it — and the dynamic LDS to ask for: the kernel's own `lds`, plus where an FC_TENSOR_NHWC launch has room the staging area
// of the waves' interleaved rows, named in the epilogue (nhwc_stage_plan, vpf_internal.h; npx = pixels per lane of the kernel)
template <int DST, class F>
inline void with_frame_table(const BatchArgsL& a, uint32_t n, bool small, const TensorEpi* te, uint32_t lds, uint32_t npx, F&& f) {
  if constexpr (DST == FC_TENSOR || DST == FC_TENSOR_NHWC) {
    const uint32_t ncopy = ((n + 7u) & ~7u) < (uint32_t)kMaxBatch ? ((n + 7u) & ~7u) : (uint32_t)kMaxBatch;
    auto fill = [&](auto& t, uint32_t cap) {
      std::memcpy(t.f, a.f, (ncopy < cap ? ncopy : cap) * sizeof(FrameDesc));
      const uint32_t l = DST == FC_TENSOR_NHWC ? nhwc_stage_plan(*te, lds, npx, &t.e) : (t.e = *te, lds);
      f(t, l);
    };
    if (small) { BatchArgsTE<kSmallBatch> t; fill(t, (uint32_t)kSmallBatch); }
    else { BatchArgsTE<kMaxBatch> t; fill(t, (uint32_t)kMaxBatch); }
  } else if (small) {
    const BatchArgs t = small_batch(a, n);
    f(t, lds);
  } else {
    f(a, lds);
  }
}

// ---- the convert and relayout launches (k_yuv2rgb.hip, k_rgb2yuv.hip, k_relayout.hip)
// What convert_plan (vpf_convert_plan.h) looks at: the bits of every plane formed in ONE pass over the n frames of the dispatch (planes a format
// does not have are zero in the table, and the plan does not ask for them)
inline ConvertShape convert_shape(int kind, int src, int dst, uint32_t w, uint32_t h, uint32_t n, const BatchArgs& a, int variant) {
  ConvertShape q{};
  q.kind = kind; q.src = src; q.dst = dst; q.w = w; q.h = h; q.n = n; q.variant = variant;
  for (uint32_t i = 0; i < n; i++)
    for (int k = 0; k < 3; k++) {
      q.src_bits[k] |= (uintptr_t)a.f[i].s[k] | a.f[i].sp[k];
      q.dst_bits[k] |= (uintptr_t)a.f[i].d[k] | a.f[i].dp[k];
    }
  return q;
}

// ---- the per-job tensor launches (k_convert_roi.hip, k_convert_letterbox.hip, k_convert_warp.hip, k_convert_persp.hip and their _dev forms)
// What job_plan (vpf_job_plan.h) looks at, less the jobs: the knob is read HERE, once per launcher call
inline void job_shape(JobShape& q, int family, bool dev, int src_fc, bool nhwc, const TensorEpi& te, uint32_t W, uint32_t H, uint32_t dw, uint32_t dh) {
  q.family = family; q.dev = dev; q.src_fc = src_fc; q.nhwc = nhwc; q.dtype = te.dtype;
  q.W = W; q.H = H; q.dw = dw; q.dh = dh;
  q.variant = tuning(VPF_TUNE_NV12_RGB_VARIANT);
  q.n = q.max_n = q.n_frames = 0u; q.max_step = 0.f;
}
// ... a host table's jobs: geom(JobGeom&, const Desc&) copies the members the family's policy reads (a table beyond the largest cap is refused by
// the plan, which then looks at no job)
template <class Desc, class F>
inline void job_shape_jobs(JobShape& q, const Desc* jobs, uint32_t n, F&& geom) {
  q.n = n;
  for (uint32_t i = 0; i < n && i < kJobTableMax; i++) geom(q.g[i], jobs[i]);
}
// ... a device table's counts and, for the two warps, the caller's hint
inline void job_shape_dev(JobShape& q, uint32_t max_n, uint32_t n_frames, float max_step = 0.f) { q.max_n = max_n; q.n_frames = n_frames; q.max_step = max_step; }
// The two zeroed tables of a host-table call, t[k] for dispatch k of the plan: every job goes behind the earlier jobs of its dispatch.  Entries
// beyond a table's jobs are never read: blockIdx.z runs over its jobs.
template <class Args, class Desc>
inline void fill_job_tables(const JobPlan& p, const Desc* jobs, uint32_t n, const TensorEpi& te, Args (&t)[2]) {
  std::memset(t, 0, sizeof(t));
  t[0].e = t[1].e = te;
  uint32_t cnt[2] = {0u, 0u};
  for (uint32_t i = 0; i < n; i++) t[p.which[i]].j[cnt[p.which[i]]++] = jobs[i];
}
// The epilogue a dispatch passes (args.e) and the dynamic LDS it asks for: the strip, then — where the plan names a pixel count and both fit — the
// waves' channels-last staging area (nhwc_stage_plan, vpf_internal.h)
template <class Args>
inline uint32_t job_launch_lds(const JobDispatch& d, const TensorEpi& te, Args& args) {
  args.e = te;
  return d.stage_npx ? nhwc_stage_plan(te, d.lds, d.stage_npx, &args.e) : d.lds;
}

}  // namespace vpf
#endif  // VPF_K_JOB_LAUNCH_H_
