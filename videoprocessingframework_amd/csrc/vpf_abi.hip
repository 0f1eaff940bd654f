// vpf_abi.hip — the C ABI of libvpfhip (include/vpf_hip.h): argument validation, format dispatch,
// kernarg packing.  No CPU fallback of any kind: every success path ends in a HIP kernel launch.
#include <atomic>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>

#include <dlfcn.h>

#include "vpf_coef.h"
#include "vpf_internal.h"
#include "vpf_job_bounds.h"

namespace vpf {

bool make_yuv2rgb(int cs, int cr, Yuv2RgbCoef* o) { return coef_yuv2rgb(cs, cr, o); }

struct Rgb2YuvDec {
  int64_t m[3][3];
  int d[3];
};
static const Rgb2YuvDec kRgb2Yuv[2] = {
    {{{257000, 504000, 98000}, {-148000, -291000, 439000}, {439000, -368000, -71000}}, {16, 128, 128}},   // MPEG "YCbCr"
    {{{299000, 587000, 114000}, {-147108, -288804, 435912}, {614777, -514799, -99978}}, {0, 128, 128}}};  // JPEG "YUV"

bool make_rgb2yuv(int cr, Rgb2YuvCoef* o) {
  if (cr != VPF_MPEG && cr != VPF_JPEG) return false;
  const Rgb2YuvDec& m = kRgb2Yuv[cr];
  for (int k = 0; k < 3; k++) {
    for (int j = 0; j < 3; j++) o->m[k][j] = q6(m.m[k][j]);
    o->d[k] = q6((int64_t)m.d[k] * 1000000 + 500000);
  }
  return true;
}

// ------------------------------------------------------------------------------------------
// diagnostics: VPF_HIP_LOG / VPF_HIP_ROCTX (vpf_internal.h)
// ------------------------------------------------------------------------------------------
static std::atomic<int> g_log_level{-1}, g_trace{-1};
static int (*g_roctx_push)(const char*) = nullptr;
static int (*g_roctx_pop)() = nullptr;
static void (*g_roctx_mark)(const char*) = nullptr;
int log_level() {
  int v = g_log_level.load(std::memory_order_relaxed);
  if (v < 0) {
    const char* e = std::getenv("VPF_HIP_LOG");
    v = e ? (std::atoi(e) > 0 ? std::atoi(e) : 1) : 0;
    g_log_level.store(v, std::memory_order_relaxed);
  }
  return v;
}
bool trace_on() {
  int v = g_trace.load(std::memory_order_acquire);
  if (v < 0) {
    static std::mutex m;
    std::lock_guard<std::mutex> lock(m);
    v = g_trace.load(std::memory_order_acquire);
    if (v < 0) {
      v = 0;
      const char* e = std::getenv("VPF_HIP_ROCTX");
      if (e && std::atoi(e) > 0) {
        void* h = dlopen("librocprofiler-sdk-roctx.so", RTLD_NOW | RTLD_GLOBAL);
        if (!h) h = dlopen("librocprofiler-sdk-roctx.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!h) h = dlopen("libroctx64.so", RTLD_NOW | RTLD_GLOBAL);
        if (h) {
          g_roctx_push = reinterpret_cast<int (*)(const char*)>(dlsym(h, "roctxRangePushA"));
          g_roctx_pop = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
          g_roctx_mark = reinterpret_cast<void (*)(const char*)>(dlsym(h, "roctxMarkA"));
        }
        if (g_roctx_push && g_roctx_pop) v = 1;
        else std::fprintf(stderr, "libvpfhip: VPF_HIP_ROCTX is set but no roctx library could be loaded; tracing stays off\n");
      }
      g_trace.store(v, std::memory_order_release);
    }
  }
  return v > 0;
}
void trace_push(const char* name) { if (g_roctx_push) g_roctx_push(name); }
void trace_pop() { if (g_roctx_pop) g_roctx_pop(); }
void note_kernel(const char* k) {
  if (log_level() >= 2) std::fprintf(stderr, "libvpfhip: launch %s\n", k);
  if (trace_on() && g_roctx_mark) g_roctx_mark(k);
}

static std::atomic<int> g_tune_variant{0}, g_tune_tile{0}, g_tune_band{0}, g_tune_mfma{0};
int tuning(int key) {
  return key == VPF_TUNE_NV12_RGB_VARIANT ? g_tune_variant.load() : key == VPF_TUNE_RESIZE_TILE ? g_tune_tile.load() : key == VPF_TUNE_RESIZE_BAND ? g_tune_band.load() : key == VPF_TUNE_RESIZE_MFMA ? g_tune_mfma.load() : 0;
}

// ------------------------------------------------------------------------------------------
// format helpers
// ------------------------------------------------------------------------------------------
static int num_planes(int f) {
  switch (f) {
    case VPF_FMT_Y: case VPF_FMT_RGB: case VPF_FMT_BGR: case VPF_FMT_RGB_32F: return 1;
    case VPF_FMT_NV12: case VPF_FMT_P10: case VPF_FMT_P12: return 2;
    case VPF_FMT_YUV420: case VPF_FMT_YCBCR: case VPF_FMT_YUV444: case VPF_FMT_RGB_PLANAR:
    case VPF_FMT_RGB_32F_PLANAR: return 3;
    default: return 0;
  }
}
static uint32_t row_bytes(int f, int k, uint32_t w) {
  const uint32_t cw = (w + 1) / 2;
  switch (f) {
    case VPF_FMT_Y: return w;
    case VPF_FMT_RGB: case VPF_FMT_BGR: return 3 * w;
    case VPF_FMT_NV12: return k == 0 ? w : 2 * cw;
    case VPF_FMT_YUV420: case VPF_FMT_YCBCR: return k == 0 ? w : cw;
    case VPF_FMT_YUV444: case VPF_FMT_RGB_PLANAR: return w;
    case VPF_FMT_RGB_32F: return 12 * w;
    case VPF_FMT_RGB_32F_PLANAR: return 4 * w;
    case VPF_FMT_P10: case VPF_FMT_P12: return k == 0 ? 2 * w : 4 * cw;
    default: return 0;
  }
}
// Frames per dispatch of the resize / fused batch entries (round 5).  A dispatch costs ~3 us between its last wave and the next one's first
// plus a tail of partly empty CUs of about one wave life: for SMALL planes (a 32-frame dispatch of Y 1080p -> 720p is 24 us of kernel) four
// times the frames per dispatch are worth 8-18 %; for larger ones they are level or a loss (RGB 1080p -> 720p Lanczos 2.04 -> 2.31 us per
// frame, RGB 720p -> 1080p bilinear 1.82 -> 2.14: dispatches of 60 us and more had little tail to amortise, and the launch planners are fitted
// at 32 and at 128 frames only).  Measured over seven shapes x 32 / 64 / 96 / 128 frames (profiles/r05_frames_per_dispatch_curve.txt): the
// gain sits with the shapes that move up to ~7 MB per frame (source + destination).
// Round 6: between the two, bilinear / nearest frames of 7-10 MB (packed RGB 1080p <-> 720p) go 64 to a dispatch: the r05 curve has them at 1.72 -> 1.60 us
// per frame (1080p -> 720p) and 1.82 -> 1.74 (720p -> 1080p) at 64 and losing again at 128; the Lanczos kernel is level at 64 and keeps 32.
static uint32_t frames_per_dispatch(uint64_t bytes_per_frame, bool mid_ok = false) {
  static const bool mid_on = [] { const char* e = std::getenv("VPF_HIP_MID_BATCH"); return !(e && e[0] == '0'); }();  // (A/B: VPF_HIP_MID_BATCH=0 keeps 32)
  mid_ok = mid_ok && mid_on;
  return bytes_per_frame <= 7000000ull ? (uint32_t)kMaxBatch : (mid_ok && bytes_per_frame <= 10000000ull) ? 64u : (uint32_t)kSmallBatch;
}
static uint64_t frame_bytes(int f, vpf_size s) {
  uint64_t b = 0;
  for (int k = 0; k < num_planes(f); k++) {
    const bool half = k > 0 && (f == VPF_FMT_NV12 || f == VPF_FMT_YUV420 || f == VPF_FMT_YCBCR || f == VPF_FMT_P10 || f == VPF_FMT_P12);
    b += (uint64_t)row_bytes(f, k, s.width) * (half ? (s.height + 1) / 2 : s.height);
  }
  return b;
}
// Pictures larger than 65536 in either dimension are refused: beyond that 12 * width (RGB_32F row bytes) and the kernels'
// 32-bit in-row offsets could wrap, and no video surface is that large.
static bool dims_ok(vpf_size s) { return s.width && s.height && s.width <= 65536u && s.height <= 65536u; }
static bool planes_ok(int f, uint32_t w, const vpf_plane* p) {
  const int n = num_planes(f);
  if (!n || !p) return false;
  for (int k = 0; k < n; k++)
    if (!p[k].ptr || p[k].pitch < row_bytes(f, k, w)) return false;
  return true;
}
static int yuv_src_class(int f) {
  switch (f) {
    case VPF_FMT_NV12: return FC_NV12;
    case VPF_FMT_YUV420: return FC_YUV420;
    case VPF_FMT_YUV444: return FC_YUV444;
    default: return -1;
  }
}
// The sources of the fused TENSOR entries (vpf_convert_resize_tensor(_batch), _rois, vpf_convert_warp_tensor): the 8-bit 4:2:0 formats and
// P10 / P12, whose 16-bit samples the kernels narrow at the load.  A mapping of its own: classify() and the 8-bit fused entries keep
// yuv_src_class(), so vpf_convert_supported(P10, RGB ..) and vpf_convert_resize(P10 ..) answer as before.
static int tensor_src_class(int f) {
  switch (f) {
    case VPF_FMT_NV12: return FC_NV12;
    case VPF_FMT_YUV420: return FC_YUV420;
    case VPF_FMT_P10: case VPF_FMT_P12: return FC_P16;
    default: return -1;
  }
}
// planes_ok, for the 16-bit formats 2-B aligned pointers and pitches, and where the entry says so (the warp entries) zero `reserved` fields
static bool tensor_src_ok(int f, uint32_t w, const vpf_plane* p, bool reserved_zero = false) {
  if (!planes_ok(f, w, p)) return false;
  if (reserved_zero)
    for (int k = 0; k < num_planes(f); k++)
      if (p[k].reserved) return false;
  if (f == VPF_FMT_P10 || f == VPF_FMT_P12)
    for (int k = 0; k < 2; k++)
      if (((uintptr_t)p[k].ptr | p[k].pitch) & 1) return false;
  return true;
}
static int rgb_class(int f) {
  switch (f) {
    case VPF_FMT_RGB: return FC_RGB;
    case VPF_FMT_BGR: return FC_BGR;
    case VPF_FMT_RGB_PLANAR: return FC_PLANAR;
    default: return -1;
  }
}
static bool cscr_ok(int cs, int cr) {
  return (cs == VPF_BT_601 || cs == VPF_BT_709) && (cr == VPF_MPEG || cr == VPF_JPEG);
}

enum Family { FAM_NONE, FAM_YUV2RGB, FAM_RGB2YUV, FAM_RELAYOUT };
static Family classify(int sf, int df, int cs, int cr) {
  if (yuv_src_class(sf) >= 0 && rgb_class(df) >= 0) return cscr_ok(cs, cr) ? FAM_YUV2RGB : FAM_NONE;
  if (rgb_class(sf) >= 0 && (df == VPF_FMT_YUV444 || df == VPF_FMT_YUV420 || df == VPF_FMT_YCBCR))
    return (cs == VPF_BT_601 && (cr == VPF_MPEG || cr == VPF_JPEG)) ? FAM_RGB2YUV : FAM_NONE;
  if (sf == VPF_FMT_NV12 && (df == VPF_FMT_YUV420 || df == VPF_FMT_Y)) return FAM_RELAYOUT;
  if (sf == VPF_FMT_YUV420 && df == VPF_FMT_NV12) return FAM_RELAYOUT;
  if (rgb_class(sf) >= 0 && rgb_class(df) >= 0 && sf != df) return FAM_RELAYOUT;
  if (sf == VPF_FMT_Y && df == VPF_FMT_YUV444) return FAM_RELAYOUT;
  if (rgb_class(sf) >= 0 && df == VPF_FMT_Y) return FAM_RELAYOUT;
  if (sf == VPF_FMT_RGB && df == VPF_FMT_RGB_32F) return FAM_RELAYOUT;
  if (sf == VPF_FMT_RGB_32F && df == VPF_FMT_RGB_32F_PLANAR) return FAM_RELAYOUT;
  if ((sf == VPF_FMT_P10 || sf == VPF_FMT_P12) && df == VPF_FMT_NV12) return FAM_RELAYOUT;
  return FAM_NONE;
}

// RAII device guard: the ABI never leaves the caller's current device changed
struct DeviceGuard {
  int prev = -1;
  bool switched = false;
  hipError_t err = hipSuccess;
  explicit DeviceGuard(int dev) {
    if (dev < 0) return;
    err = hipGetDevice(&prev);
    if (err == hipSuccess && prev != dev) {
      err = hipSetDevice(dev);
      switched = (err == hipSuccess);
    }
  }
  ~DeviceGuard() {
    if (switched) (void)hipSetDevice(prev);
  }
};

static void fill_desc(FrameDesc& d, const vpf_plane* s, int ns, const vpf_plane* o, int nd) {
  std::memset(&d, 0, sizeof(d));
  for (int k = 0; k < ns; k++) { d.s[k] = static_cast<const uint8_t*>(s[k].ptr); d.sp[k] = s[k].pitch; }
  for (int k = 0; k < nd; k++) { d.d[k] = static_cast<uint8_t*>(o[k].ptr); d.dp[k] = o[k].pitch; }
}

static vpf_status status_of(hipError_t e) {
  if (e == hipSuccess) return VPF_OK;
  if (log_level() >= 1) std::fprintf(stderr, "libvpfhip: %s (%s)\n", hipGetErrorName(e), hipGetErrorString(e));
  if (e == hipErrorNoDevice || e == hipErrorInvalidDevice || e == hipErrorInsufficientDriver) return VPF_ERR_NO_DEVICE;
  return VPF_ERR_LAUNCH;
}

// one frame's planes as the batch entries take them: the single-frame entries are their batch entry with n = 1
static vpf_frame_io single_frame(const vpf_plane* src, int ns, const vpf_plane* dst, int nd) {
  vpf_frame_io io;
  std::memset(&io, 0, sizeof(io));
  for (int k = 0; k < ns; k++) io.src[k] = src[k];
  for (int k = 0; k < nd; k++) io.dst[k] = dst[k];
  return io;
}
// a non-empty rectangle inside a picture of `size` (64-bit sums: x + width may pass 2^32); nothing is clipped silently
static bool rect_inside(const vpf_rect& r, vpf_size size) {
  return r.width && r.height && (uint64_t)r.x + r.width <= size.width && (uint64_t)r.y + r.height <= size.height;
}

// ------------------------------------------------------------------------------------------
// the tensor entries' host path: what every entry asks of its vpf_tensor_norm, and what the kernels get of it
// ------------------------------------------------------------------------------------------
// The refusals that come between the source format's and the pointers', in the order the entries have always had: no norm, an unknown dtype or
// flag, then what the entry's own options refuse (unsupported before bad), and only then a non-finite scale or bias — options BEFORE finiteness.
static vpf_status norm_status(const vpf_tensor_norm* norm, bool opts_unsupported = false, bool opts_bad = false) {
  if (!norm) return VPF_ERR_BAD_ARG;
  if (norm->dtype > VPF_TENSOR_BF16 || (norm->flags & ~(VPF_TENSOR_BGR | VPF_TENSOR_NHWC))) return VPF_ERR_UNSUPPORTED;
  if (opts_unsupported) return VPF_ERR_UNSUPPORTED;
  if (opts_bad) return VPF_ERR_BAD_ARG;
  for (int c = 0; c < 3; c++)
    if (!std::isfinite(norm->scale[c]) || !std::isfinite(norm->bias[c])) return VPF_ERR_BAD_ARG;
  return VPF_OK;
}
struct TensorLayout {
  uint32_t elem;  // bytes per element
  bool nhwc, bgr;
};
static TensorLayout layout_of(const vpf_tensor_norm& norm) {
  return TensorLayout{norm.dtype == VPF_TENSOR_F32 ? 4u : 2u, (norm.flags & VPF_TENSOR_NHWC) != 0, (norm.flags & VPF_TENSOR_BGR) != 0};
}
// the kernels give channel k (R G B) parameter k: B G R order swaps the parameters of channels 0 and 2 (and tensor_planes() their planes)
static void kernel_scale_bias(const vpf_tensor_norm& norm, float scale[3], float bias[3]) {
  const bool bgr = layout_of(norm).bgr;
  for (int k = 0; k < 3; k++) { scale[k] = norm.scale[bgr ? 2 - k : k]; bias[k] = norm.bias[bgr ? 2 - k : k]; }
}
// The planes of a tensor frame or job: three of `width` elements per row, or with VPF_TENSOR_NHWC the ONE interleaved plane p[0] of 3 x width
// elements per row (p[1], p[2] are not looked at).  Pointers and pitches are multiples of the element size.
static bool tensor_planes_ok(const vpf_plane* p, const TensorLayout& l, uint32_t width, bool reserved_zero = false) {
  for (int k = 0; k < (l.nhwc ? 1 : 3); k++) {
    if (!p[k].ptr || (reserved_zero && p[k].reserved) || (uint64_t)p[k].pitch < (uint64_t)width * l.elem * (l.nhwc ? 3u : 1u) ||
        (((uintptr_t)p[k].ptr | p[k].pitch) & (l.elem - 1)))
      return false;
  }
  return true;
}
// the planes the kernels take: kernel channel k (R G B) -> plane k, B G R order swaps planes 0 and 2; NHWC: the one plane (the kernel swaps slots)
static int tensor_planes(const vpf_plane* p, const TensorLayout& l, vpf_plane out[3]) {
  if (l.nhwc) { out[0] = p[0]; return 1; }
  for (int k = 0; k < 3; k++) out[k] = p[l.bgr ? 2 - k : k];
  return 3;
}
// the device-table entries (vpf_*_dev): the whole frames the jobs sample, and job 0's destination planes in kernel channel order
static void fill_frame_srcs(FrameSrcDesc* f, const vpf_frame_src* frames, uint32_t n_frames, int ns) {
  for (uint32_t i = 0; i < n_frames; i++)
    for (int k = 0; k < ns; k++) { f[i].s[k] = static_cast<const uint8_t*>(frames[i].src[k].ptr); f[i].sp[k] = frames[i].src[k].pitch; }
}
static void fill_job0_dst(uint8_t* d[3], uint32_t dp[3], const vpf_plane* dst, const TensorLayout& l) {
  vpf_plane p[3];
  const int nd = tensor_planes(dst, l, p);
  for (int k = 0; k < nd; k++) { d[k] = static_cast<uint8_t*>(p[k].ptr); dp[k] = p[k].pitch; }
}
// The entries whose boxes lie in DEVICE memory (vpf_convert_resize_tensor_rois_dev, vpf_convert_letterbox_tensor_dev): everything they can check without
// a box — the pointers, the sizes, 1 .. 128 frames, 1 .. 65535 jobs, the box table's alignment and stride, the job stride, every frame's planes and
// job 0's planes.  The host never dereferences `boxes` or `count`.
static bool dev_boxes_ok(const vpf_exec* exec, int sf, vpf_size ss, vpf_size ds, uint32_t n_frames, const vpf_frame_src* frames, const vpf_roi_dev* boxes,
                         const int32_t* count, uint32_t box_stride, uint32_t max_n, const vpf_plane* dst, uint64_t dst_job_stride, const TensorLayout& l) {
  if (!exec || !frames || !dims_ok(ss) || !dims_ok(ds)) return false;
  if (!n_frames || n_frames > (uint32_t)kRoiDevFrames || !max_n || max_n > 65535u) return false;
  if (!boxes || (((uintptr_t)boxes | (uintptr_t)count) & 3u) || box_stride < sizeof(vpf_roi_dev) || (box_stride & 3u) || (dst_job_stride & (l.elem - 1)))
    return false;
  for (uint32_t i = 0; i < n_frames; i++)
    if (!tensor_src_ok(sf, ss.width, frames[i].src)) return false;
  return tensor_planes_ok(dst, l, ds.width);
}
// ... and what their kernels get of it (RoiDevArgs, LetterboxDevArgs: the same members)
template <class Args>
static void fill_dev_boxes(Args& a, const vpf_frame_src* frames, uint32_t n_frames, int ns, const vpf_roi_dev* boxes, const int32_t* count, uint32_t box_stride,
                           uint32_t max_n, const vpf_plane* dst, uint64_t dst_job_stride, const TensorLayout& l) {
  std::memset(&a, 0, sizeof(a));
  fill_frame_srcs(a.f, frames, n_frames, ns);
  fill_job0_dst(a.d, a.dp, dst, l);
  a.boxes = reinterpret_cast<const int32_t*>(boxes);
  a.count = count;
  a.job_stride = dst_job_stride;
  a.box_stride = box_stride; a.max_n = max_n; a.n_frames = n_frames;
}
// The epilogue of a tensor launch.  `fill`: the three pad (letterbox) or border (warp) bytes per OUTPUT channel, swapped like the parameters, or
// null for zeros; `mode`: the warp's border mode, bits 24 .. 31 of TensorEpi::pad.
static TensorEpi make_epi(const vpf_tensor_norm& norm, const uint8_t* fill = nullptr, uint32_t mode = 0u) {
  const TensorLayout l = layout_of(norm);
  TensorEpi te;
  std::memset(&te, 0, sizeof(te));
  kernel_scale_bias(norm, te.scale, te.bias);
  te.dtype = norm.dtype | (l.nhwc && l.bgr ? kEpiSwapRB : 0u);
  if (fill)
    for (int k = 0; k < 3; k++) te.pad |= (uint32_t)fill[l.bgr ? 2 - k : k] << (8 * k);
  te.pad |= mode << 24;
  return te;
}

// The two warps with the matrices, their frame indices and the count in DEVICE memory (include/vpf_hip.h): every check that needs no matrix happens
// here, once for both entries, the matrix check in the kernel; one dispatch.  `Table`: vpf_warps_dev (kCoefs = 6, k_convert_warp_dev.hip) or
// vpf_persps_dev (kCoefs = 9, k_convert_persp_dev.hip), the same 96 bytes.
static_assert(sizeof(vpf_persps_dev) == 96 && sizeof(vpf_warps_dev) == 96 && offsetof(vpf_persps_dev, matrix_stride) == offsetof(vpf_warps_dev, matrix_stride) &&
                  offsetof(vpf_persps_dev, max_step) == 36 && offsetof(vpf_persps_dev, dst) == 40 && offsetof(vpf_persps_dev, dst_job_stride) == 88,
              "vpf_persps_dev has the layout of vpf_warps_dev, no implicit padding");
template <uint32_t kCoefs, typename Table, typename Launch>
static vpf_status matrices_dev_entry(const vpf_exec* exec, int sf, int cs, int cr, vpf_size ss, vpf_size ds, uint32_t n_frames, const vpf_frame_src* frames,
                                     const Table* table, const vpf_tensor_norm* norm, const vpf_warp_opts* opts, Launch launch) {
  if (tensor_src_class(sf) < 0 || !cscr_ok(cs, cr)) return VPF_ERR_UNSUPPORTED;
  if (const vpf_status refused = norm_status(norm, opts && opts->border_mode > VPF_WARP_REPLICATE, opts && opts->reserved)) return refused;
  if (!exec || !frames || !table || !dims_ok(ss) || !dims_ok(ds)) return VPF_ERR_BAD_ARG;
  if (!n_frames || n_frames > (uint32_t)kRoiDevFrames || !table->max_n || table->max_n > 65535u) return VPF_ERR_BAD_ARG;
  const TensorLayout l = layout_of(*norm);
  if (!table->matrices || (((uintptr_t)table->matrices | (uintptr_t)table->frame_index | (uintptr_t)table->count) & 3u) || table->matrix_stride < 4u * kCoefs ||
      (table->matrix_stride & 3u) || (table->frame_index && (table->frame_stride < 4u || (table->frame_stride & 3u))) ||
      (table->dst_job_stride & (l.elem - 1)) || !(table->max_step >= 0.f) || !std::isfinite(table->max_step))
    return VPF_ERR_BAD_ARG;
  for (uint32_t i = 0; i < n_frames; i++)
    if (!tensor_src_ok(sf, ss.width, frames[i].src, true)) return VPF_ERR_BAD_ARG;
  if (!tensor_planes_ok(table->dst, l, ds.width, true)) return VPF_ERR_BAD_ARG;
  DeviceGuard guard(exec->device);
  if (guard.err != hipSuccess) return status_of(guard.err);
  Yuv2RgbCoef c;
  make_yuv2rgb(cs, cr, &c);
  const TensorEpi te = make_epi(*norm, opts ? opts->border : nullptr, opts ? opts->border_mode : 0u);
  WarpDevArgs a;
  std::memset(&a, 0, sizeof(a));
  fill_frame_srcs(a.f, frames, n_frames, num_planes(sf));
  fill_job0_dst(a.d, a.dp, table->dst, l);
  a.matrices = table->matrices;
  a.frame_index = table->frame_index;
  a.count = table->count;
  a.job_stride = table->dst_job_stride;
  a.matrix_stride = table->matrix_stride; a.frame_stride = table->frame_index ? table->frame_stride : 0u; a.max_n = table->max_n; a.n_frames = n_frames;
  return status_of(launch(static_cast<hipStream_t>(exec->stream), tensor_src_class(sf), c, ss.width, ss.height, a, ds.width, ds.height, table->max_step, te, l.nhwc));
}

}  // namespace vpf

using namespace vpf;

extern "C" {

int vpf_convert_supported(int sf, int df, int cs, int cr) { return classify(sf, df, cs, cr) != FAM_NONE; }

vpf_status vpf_convert_batch(const vpf_exec* exec, int sf, int df, int cs, int cr, vpf_size size, uint32_t n,
                             const vpf_frame_io* frames) {
  const Mark mark("vpf_convert_batch");
  const Family fam = classify(sf, df, cs, cr);
  if (fam == FAM_NONE) return VPF_ERR_UNSUPPORTED;
  if (!exec || !frames || !n || !dims_ok(size)) return VPF_ERR_BAD_ARG;
  for (uint32_t i = 0; i < n; i++)
    if (!planes_ok(sf, size.width, frames[i].src) || !planes_ok(df, size.width, frames[i].dst)) return VPF_ERR_BAD_ARG;
  DeviceGuard guard(exec->device);
  if (guard.err != hipSuccess) return status_of(guard.err);
  hipStream_t st = static_cast<hipStream_t>(exec->stream);
  const int ns = num_planes(sf), nd = num_planes(df);
  Yuv2RgbCoef yc;
  Rgb2YuvCoef rc;
  if (fam == FAM_YUV2RGB) make_yuv2rgb(cs, cr, &yc);
  if (fam == FAM_RGB2YUV) make_rgb2yuv(cr, &rc);
  for (uint32_t base = 0; base < n; base += kSmallBatch) {
    const uint32_t m = (n - base < (uint32_t)kSmallBatch) ? n - base : (uint32_t)kSmallBatch;
    BatchArgs a;
    for (uint32_t i = 0; i < m; i++) fill_desc(a.f[i], frames[base + i].src, ns, frames[base + i].dst, nd);
    for (uint32_t i = m; i < (uint32_t)kSmallBatch; i++) a.f[i] = a.f[0];
    hipError_t e;
    switch (fam) {
      case FAM_YUV2RGB:
        e = launch_yuv_to_rgb(st, yuv_src_class(sf), rgb_class(df), yc, size.width, size.height, m, a,
                              tuning(VPF_TUNE_NV12_RGB_VARIANT), (exec->flags & VPF_EXEC_DST_REUSED) != 0);
        break;
      case FAM_RGB2YUV:
        e = launch_rgb_to_yuv(st, rgb_class(sf), df == VPF_FMT_YUV444 ? FC_YUV444 : FC_YUV420, rc, size.width,
                              size.height, m, a);
        break;
      default: e = launch_relayout(st, sf, df, size.width, size.height, m, a);
    }
    if (e != hipSuccess) return status_of(e);
  }
  return VPF_OK;
}

vpf_status vpf_convert(const vpf_exec* exec, int sf, int df, int cs, int cr, vpf_size size, const vpf_plane src[3],
                       const vpf_plane dst[3]) {
  if (classify(sf, df, cs, cr) == FAM_NONE) return VPF_ERR_UNSUPPORTED;
  if (!src || !dst) return VPF_ERR_BAD_ARG;
  const vpf_frame_io io = single_frame(src, num_planes(sf), dst, num_planes(df));
  return vpf_convert_batch(exec, sf, df, cs, cr, size, 1, &io);
}

// planes of `fmt` as resize jobs: (interleaved channels, plane index, plane size in pixels)
static int resize_jobs(int fmt, vpf_size ss, vpf_size ds, ResizeJob jobs[3], bool* f32) {
  const uint32_t scw = (ss.width + 1) / 2, sch = (ss.height + 1) / 2, dcw = (ds.width + 1) / 2, dch = (ds.height + 1) / 2;
  *f32 = fmt == VPF_FMT_RGB_32F || fmt == VPF_FMT_RGB_32F_PLANAR;
  const ResizeJob full1 = {1, 0, ss.width, ss.height, ds.width, ds.height};
  switch (fmt) {
    case VPF_FMT_RGB: case VPF_FMT_BGR: case VPF_FMT_RGB_32F: jobs[0] = ResizeJob{3, 0, ss.width, ss.height, ds.width, ds.height}; return 1;
    case VPF_FMT_Y: jobs[0] = full1; return 1;
    case VPF_FMT_YUV444: case VPF_FMT_RGB_PLANAR: case VPF_FMT_RGB_32F_PLANAR:
      for (int k = 0; k < 3; k++) { jobs[k] = full1; jobs[k].k = k; }
      return 3;
    case VPF_FMT_YUV420: case VPF_FMT_YCBCR:
      jobs[0] = full1;
      for (int k = 1; k < 3; k++) jobs[k] = ResizeJob{1, k, scw, sch, dcw, dch};
      return 3;
    case VPF_FMT_NV12:  // luma plane + the UV plane as a 2-channel image (== C3 -> R2 -> C4 of Tasks.cpp:1303-1318)
      jobs[0] = full1;
      jobs[1] = ResizeJob{2, 1, scw, sch, dcw, dch};
      return 2;
    default: return 0;
  }
}

vpf_status vpf_resize_batch(const vpf_exec* exec, int fmt, int interp, vpf_size ss, vpf_size ds, uint32_t n, const vpf_frame_io* frames) {
  const Mark mark("vpf_resize_batch");
  if (interp != VPF_INTERP_NEAREST && interp != VPF_INTERP_LINEAR && interp != VPF_INTERP_LANCZOS3) return VPF_ERR_UNSUPPORTED;
  ResizeJob jobs[3];
  bool f32 = false;
  const int nj = resize_jobs(fmt, ss, ds, jobs, &f32);
  if (!nj) return VPF_ERR_UNSUPPORTED;
  if (!exec || !frames || !n || !dims_ok(ss) || !dims_ok(ds)) return VPF_ERR_BAD_ARG;
  for (uint32_t i = 0; i < n; i++) {
    if (!planes_ok(fmt, ss.width, frames[i].src) || !planes_ok(fmt, ds.width, frames[i].dst)) return VPF_ERR_BAD_ARG;
    if (f32)  // float samples: rows must be 4-B aligned
      for (int k = 0; k < num_planes(fmt); k++)
        if ((((uintptr_t)frames[i].src[k].ptr | frames[i].src[k].pitch | (uintptr_t)frames[i].dst[k].ptr | frames[i].dst[k].pitch) & 3)) return VPF_ERR_BAD_ARG;
  }
  DeviceGuard guard(exec->device);
  if (guard.err != hipSuccess) return status_of(guard.err);
  hipStream_t st = static_cast<hipStream_t>(exec->stream);
  const int np = num_planes(fmt);
  const uint32_t per = frames_per_dispatch(frame_bytes(fmt, ss) + frame_bytes(fmt, ds), interp != VPF_INTERP_LANCZOS3);  // 128 for small planes, 64 for mid-sized bilinear ones, else 32 (the launchers take the small frame table for up to 32)
  for (uint32_t base = 0; base < n; base += per) {
    const uint32_t m = (n - base < per) ? n - base : per;
    BatchArgsL a;
    for (uint32_t i = 0; i < m; i++) fill_desc(a.f[i], frames[base + i].src, np, frames[base + i].dst, np);
    for (uint32_t i = m; i < ((m + 7u) & ~7u); i++) a.f[i] = a.f[0];  // (entries beyond the batch are never read: blockIdx runs over m frames; a few copies keep the tail of the last cache line defined)
    const hipError_t e = launch_resize_planned(st, f32, interp, nj, jobs, m, a, n);  // (one plane of one frame: the scalar-argument entries, resize_plan)
    if (e != hipSuccess) return status_of(e);
  }
  return VPF_OK;
}

vpf_status vpf_resize(const vpf_exec* exec, int fmt, int interp, vpf_size ss, const vpf_plane src[3], vpf_size ds,
                      const vpf_plane dst[3]) {
  if (interp != VPF_INTERP_NEAREST && interp != VPF_INTERP_LINEAR && interp != VPF_INTERP_LANCZOS3) return VPF_ERR_UNSUPPORTED;
  ResizeJob probe[3];
  bool f32 = false;
  if (!resize_jobs(fmt, vpf_size{2, 2}, vpf_size{2, 2}, probe, &f32)) return VPF_ERR_UNSUPPORTED;
  if (!src || !dst) return VPF_ERR_BAD_ARG;
  const vpf_frame_io io = single_frame(src, num_planes(fmt), dst, num_planes(fmt));
  return vpf_resize_batch(exec, fmt, interp, ss, ds, 1, &io);
}

// the workspace forms: the same calls with the caller's table region made known to the Lanczos launcher for their duration
struct WorkspaceScope {
  explicit WorkspaceScope(vpf_workspace* ws) { set_lanczos_workspace(ws); }
  ~WorkspaceScope() { set_lanczos_workspace(nullptr); }
};
vpf_status vpf_resize_batch_ws(const vpf_exec* exec, int fmt, int interp, vpf_size ss, vpf_size ds, uint32_t n, const vpf_frame_io* frames, vpf_workspace* ws) {
  const WorkspaceScope scope(ws);
  return vpf_resize_batch(exec, fmt, interp, ss, ds, n, frames);
}
vpf_status vpf_resize_ws(const vpf_exec* exec, int fmt, int interp, vpf_size ss, const vpf_plane src[3], vpf_size ds, const vpf_plane dst[3], vpf_workspace* ws) {
  const WorkspaceScope scope(ws);
  return vpf_resize(exec, fmt, interp, ss, src, ds, dst);
}
uint64_t vpf_resize_workspace_bytes(int fmt, int interp, vpf_size ss, vpf_size ds) {
  ResizeJob jobs[3];
  bool f32 = false;
  if (interp != VPF_INTERP_LANCZOS3 || !dims_ok(ss) || !dims_ok(ds)) return 0;
  const int nj = resize_jobs(fmt, ss, ds, jobs, &f32);
  if (!nj || f32) return 0;
  uint64_t total = 256;  // (offset 0 of a region means "no table": its first 256 bytes stay unused)
  for (int p = 0; p < nj; p++) total += lanczos_table_bytes_bound(jobs[p].ch, jobs[p].dw, jobs[p].dh);
  return total;
}

vpf_status vpf_remap_batch(const vpf_exec* exec, int fmt, vpf_size ss, const float* xmap, uint32_t xp, const float* ymap, uint32_t yp, vpf_size ds,
                           uint32_t n, const vpf_frame_io* frames) {
  const Mark mark("vpf_remap_batch");
  if (fmt != VPF_FMT_RGB && fmt != VPF_FMT_BGR) return VPF_ERR_UNSUPPORTED;
  if (!exec || !frames || !n || !dims_ok(ss) || !dims_ok(ds) || !xmap || !ymap || xp < 4 * ds.width || yp < 4 * ds.width || (xp & 3) || (yp & 3) ||
      ((uintptr_t)xmap & 3) || ((uintptr_t)ymap & 3))
    return VPF_ERR_BAD_ARG;
  for (uint32_t i = 0; i < n; i++)
    if (!planes_ok(fmt, ss.width, frames[i].src) || !planes_ok(fmt, ds.width, frames[i].dst)) return VPF_ERR_BAD_ARG;
  DeviceGuard guard(exec->device);
  if (guard.err != hipSuccess) return status_of(guard.err);
  for (uint32_t base = 0; base < n; base += kSmallBatch) {
    const uint32_t m = (n - base < (uint32_t)kSmallBatch) ? n - base : (uint32_t)kSmallBatch;
    BatchArgs a;
    for (uint32_t i = 0; i < m; i++) fill_desc(a.f[i], frames[base + i].src, 1, frames[base + i].dst, 1);
    for (uint32_t i = m; i < (uint32_t)kSmallBatch; i++) a.f[i] = a.f[0];
    const hipError_t e = launch_remap_batch(static_cast<hipStream_t>(exec->stream), ss.width, ss.height, xmap, xp, ymap, yp, ds.width, ds.height, m, a);
    if (e != hipSuccess) return status_of(e);
  }
  return VPF_OK;
}

vpf_status vpf_remap(const vpf_exec* exec, int fmt, vpf_size ss, const vpf_plane* src, const float* xmap, uint32_t xp,
                     const float* ymap, uint32_t yp, vpf_size ds, const vpf_plane* dst) {
  const Mark mark("vpf_remap");
  if (fmt != VPF_FMT_RGB && fmt != VPF_FMT_BGR) return VPF_ERR_UNSUPPORTED;
  if (!exec || !dims_ok(ss) || !dims_ok(ds) || !xmap || !ymap || !planes_ok(fmt, ss.width, src) ||
      !planes_ok(fmt, ds.width, dst) || xp < 4 * ds.width || yp < 4 * ds.width || (xp & 3) || (yp & 3) ||
      ((uintptr_t)xmap & 3) || ((uintptr_t)ymap & 3))
    return VPF_ERR_BAD_ARG;
  DeviceGuard guard(exec->device);
  if (guard.err != hipSuccess) return status_of(guard.err);
  return status_of(launch_remap(static_cast<hipStream_t>(exec->stream), ss.width, ss.height,
                                static_cast<const uint8_t*>(src->ptr), src->pitch, xmap, xp, ymap, yp, ds.width,
                                ds.height, static_cast<uint8_t*>(dst->ptr), dst->pitch));
}

vpf_status vpf_convert_resize_batch(const vpf_exec* exec, int sf, int df, int cs, int cr, vpf_size ss, vpf_size ds,
                                    uint32_t n, const vpf_frame_io* frames) {
  const Mark mark("vpf_convert_resize_batch");
  if (!(sf == VPF_FMT_NV12 || sf == VPF_FMT_YUV420) || rgb_class(df) < 0 || !cscr_ok(cs, cr)) return VPF_ERR_UNSUPPORTED;
  if (!exec || !frames || !n || !dims_ok(ss) || !dims_ok(ds)) return VPF_ERR_BAD_ARG;
  for (uint32_t i = 0; i < n; i++)
    if (!planes_ok(sf, ss.width, frames[i].src) || !planes_ok(df, ds.width, frames[i].dst)) return VPF_ERR_BAD_ARG;
  DeviceGuard guard(exec->device);
  if (guard.err != hipSuccess) return status_of(guard.err);
  Yuv2RgbCoef c;
  make_yuv2rgb(cs, cr, &c);
  const uint32_t per = frames_per_dispatch(frame_bytes(sf, ss) + frame_bytes(df, ds), true);  // 128 for small frames (1080p -> 720p and smaller), 64 for 7-10 MB ones (720p -> 1080p), else 32
  for (uint32_t base = 0; base < n; base += per) {
    const uint32_t m = (n - base < per) ? n - base : per;
    BatchArgsL a;
    for (uint32_t i = 0; i < m; i++) fill_desc(a.f[i], frames[base + i].src, num_planes(sf), frames[base + i].dst, num_planes(df));
    for (uint32_t i = m; i < ((m + 7u) & ~7u); i++) a.f[i] = a.f[0];  // (entries beyond the batch are never read: blockIdx runs over m frames; a few copies keep the tail of the last cache line defined)
    const hipError_t e = launch_convert_resize(static_cast<hipStream_t>(exec->stream), yuv_src_class(sf), rgb_class(df), c,
                                               ss.width, ss.height, m, a, ds.width, ds.height);
    if (e != hipSuccess) return status_of(e);
  }
  return VPF_OK;
}

vpf_status vpf_convert_resize(const vpf_exec* exec, int sf, int df, int cs, int cr, vpf_size ss, const vpf_plane src[3],
                              vpf_size ds, const vpf_plane dst[3]) {
  if (!(sf == VPF_FMT_NV12 || sf == VPF_FMT_YUV420) || rgb_class(df) < 0 || !cscr_ok(cs, cr)) return VPF_ERR_UNSUPPORTED;
  if (!src || !dst) return VPF_ERR_BAD_ARG;
  const vpf_frame_io io = single_frame(src, num_planes(sf), dst, num_planes(df));
  return vpf_convert_resize_batch(exec, sf, df, cs, cr, ss, ds, 1, &io);
}

// The planar-tensor form of the fused path (include/vpf_hip.h): the RGB_PLANAR bytes through one fp32 fma per channel, stored as f32 / f16 / bf16.
vpf_status vpf_convert_resize_tensor_batch(const vpf_exec* exec, int sf, int cs, int cr, vpf_size ss, vpf_size ds, uint32_t n,
                                           const vpf_frame_io* frames, const vpf_tensor_norm* norm) {
  const Mark mark("vpf_convert_resize_tensor_batch");
  if (tensor_src_class(sf) < 0 || !cscr_ok(cs, cr)) return VPF_ERR_UNSUPPORTED;
  if (const vpf_status refused = norm_status(norm)) return refused;
  if (!exec || !frames || !n || !dims_ok(ss) || !dims_ok(ds)) return VPF_ERR_BAD_ARG;
  const TensorLayout l = layout_of(*norm);
  for (uint32_t i = 0; i < n; i++) {
    if (!tensor_src_ok(sf, ss.width, frames[i].src)) return VPF_ERR_BAD_ARG;
    if (!tensor_planes_ok(frames[i].dst, l, ds.width)) return VPF_ERR_BAD_ARG;
  }
  DeviceGuard guard(exec->device);
  if (guard.err != hipSuccess) return status_of(guard.err);
  Yuv2RgbCoef c;
  make_yuv2rgb(cs, cr, &c);
  const TensorEpi te = make_epi(*norm);
  const uint32_t per = frames_per_dispatch(frame_bytes(sf, ss) + 3ull * ds.width * ds.height * l.elem, true);  // the tensor's real bytes: 4x the 8-bit planes for f32
  for (uint32_t base = 0; base < n; base += per) {
    const uint32_t m = (n - base < per) ? n - base : per;
    BatchArgsL a;
    for (uint32_t i = 0; i < m; i++) {
      vpf_plane d[3];
      const int nd = tensor_planes(frames[base + i].dst, l, d);
      fill_desc(a.f[i], frames[base + i].src, num_planes(sf), d, nd);
    }
    for (uint32_t i = m; i < ((m + 7u) & ~7u); i++) a.f[i] = a.f[0];
    const hipError_t e = launch_convert_resize(static_cast<hipStream_t>(exec->stream), tensor_src_class(sf), l.nhwc ? FC_TENSOR_NHWC : FC_TENSOR, c, ss.width, ss.height, m, a,
                                               ds.width, ds.height, &te);
    if (e != hipSuccess) return status_of(e);
  }
  return VPF_OK;
}

vpf_status vpf_convert_resize_tensor(const vpf_exec* exec, int sf, int cs, int cr, vpf_size ss, const vpf_plane src[3], vpf_size ds,
                                     const vpf_plane dst[3], const vpf_tensor_norm* norm) {
  if (tensor_src_class(sf) < 0 || !cscr_ok(cs, cr)) return VPF_ERR_UNSUPPORTED;
  if (!src || !dst) return VPF_ERR_BAD_ARG;
  const vpf_frame_io io = single_frame(src, num_planes(sf), dst, 3);
  return vpf_convert_resize_tensor_batch(exec, sf, cs, cr, ss, ds, 1, &io, norm);
}

// Many rectangles of decoded frames -> one batch of normalised planes (include/vpf_hip.h): per-job geometry, kRoiBatch jobs per job table,
// each table at most two dispatches (k_convert_roi.hip).
vpf_status vpf_convert_resize_tensor_rois(const vpf_exec* exec, int sf, int cs, int cr, vpf_size ss, vpf_size ds, uint32_t n,
                                          const vpf_roi_io* rois, const vpf_tensor_norm* norm) {
  const Mark mark("vpf_convert_resize_tensor_rois");
  if (tensor_src_class(sf) < 0 || !cscr_ok(cs, cr)) return VPF_ERR_UNSUPPORTED;
  if (const vpf_status refused = norm_status(norm)) return refused;
  if (!exec || !rois || !n || !dims_ok(ss) || !dims_ok(ds)) return VPF_ERR_BAD_ARG;
  const TensorLayout l = layout_of(*norm);
  for (uint32_t i = 0; i < n; i++) {
    if (!rect_inside(rois[i].rect, ss)) return VPF_ERR_BAD_ARG;
    if (!tensor_src_ok(sf, ss.width, rois[i].src)) return VPF_ERR_BAD_ARG;
    if (!tensor_planes_ok(rois[i].dst, l, ds.width)) return VPF_ERR_BAD_ARG;
  }
  DeviceGuard guard(exec->device);
  if (guard.err != hipSuccess) return status_of(guard.err);
  Yuv2RgbCoef c;
  make_yuv2rgb(cs, cr, &c);
  const TensorEpi te = make_epi(*norm);
  RoiDesc jobs[kRoiBatch];
  for (uint32_t base = 0; base < n; base += kRoiBatch) {
    const uint32_t m = (n - base < (uint32_t)kRoiBatch) ? n - base : (uint32_t)kRoiBatch;
    for (uint32_t i = 0; i < m; i++) {
      const vpf_roi_io& io = rois[base + i];
      vpf_plane d[3];
      const int nd = tensor_planes(io.dst, l, d);
      RoiDesc& j = jobs[i];
      fill_desc(j.f, io.src, num_planes(sf), d, nd);
      j.x = io.rect.x; j.y = io.rect.y; j.w = io.rect.width; j.h = io.rect.height;
      j.scx = (float)j.w / (float)ds.width; j.scy = (float)j.h / (float)ds.height;
    }
    const hipError_t e = launch_convert_resize_rois(static_cast<hipStream_t>(exec->stream), tensor_src_class(sf), c, ss.width, m, jobs, ds.width, ds.height, te, l.nhwc);
    if (e != hipSuccess) return status_of(e);
  }
  return VPF_OK;
}

// The same with the rectangles and their count in DEVICE memory (include/vpf_hip.h): every check that needs no box happens here, the rest in the
// kernel (k_convert_roi_dev.hip); one dispatch.
vpf_status vpf_convert_resize_tensor_rois_dev(const vpf_exec* exec, int sf, int cs, int cr, vpf_size ss, vpf_size ds, uint32_t n_frames,
                                              const vpf_frame_src* frames, const vpf_rois_dev* table, const vpf_tensor_norm* norm) {
  const Mark mark("vpf_convert_resize_tensor_rois_dev");
  if (tensor_src_class(sf) < 0 || !cscr_ok(cs, cr)) return VPF_ERR_UNSUPPORTED;
  if (const vpf_status refused = norm_status(norm)) return refused;
  const TensorLayout l = layout_of(*norm);
  if (!table || !dev_boxes_ok(exec, sf, ss, ds, n_frames, frames, table->boxes, table->count, table->box_stride, table->max_n, table->dst, table->dst_job_stride, l))
    return VPF_ERR_BAD_ARG;
  DeviceGuard guard(exec->device);
  if (guard.err != hipSuccess) return status_of(guard.err);
  Yuv2RgbCoef c;
  make_yuv2rgb(cs, cr, &c);
  const TensorEpi te = make_epi(*norm);
  RoiDevArgs a;
  fill_dev_boxes(a, frames, n_frames, num_planes(sf), table->boxes, table->count, table->box_stride, table->max_n, table->dst, table->dst_job_stride, l);
  return status_of(launch_convert_resize_rois_dev(static_cast<hipStream_t>(exec->stream), tensor_src_class(sf), c, ss.width, ss.height, a, ds.width, ds.height, te, l.nhwc));
}

// The aspect-preserving placement of a w x h picture inside dw x dh (include/vpf_hip.h): integers only, 64-bit products.
vpf_rect vpf_letterbox_fit(vpf_size src, vpf_size dst) {
  vpf_rect r = {0u, 0u, 0u, 0u};
  if (!src.width || !src.height || !dst.width || !dst.height) return r;
  const LetterboxFit f = letterbox_fit_ints(src.width, src.height, dst.width, dst.height);  // (vpf_job_bounds.h: the device-table kernel runs it too)
  r.x = f.ix; r.y = f.iy; r.width = f.iw; r.height = f.ih;
  return r;
}

// Many rectangles of decoded frames, each resized into a rectangle of its own inside its destination planes, the rest padded (include/vpf_hip.h):
// the ROI entry's checks and colour rules, kLetterboxBatch jobs per job table, each table at most two dispatches (k_convert_letterbox.hip).
// (`aa`: the antialiased entry, which shares every check, the colour rules, the cut into job tables and the job descriptors: only the launcher differs)
static vpf_status letterbox_tensor_call(const vpf_exec* exec, int sf, int cs, int cr, vpf_size ss, vpf_size ds, uint32_t n, const vpf_letterbox_io* jobs,
                                        const vpf_tensor_norm* norm, const vpf_letterbox_opts* opts, bool aa) {
  if (tensor_src_class(sf) < 0 || !cscr_ok(cs, cr)) return VPF_ERR_UNSUPPORTED;
  if (const vpf_status refused = norm_status(norm, false, opts && opts->reserved)) return refused;
  if (!exec || !jobs || !n || !dims_ok(ss) || !dims_ok(ds)) return VPF_ERR_BAD_ARG;
  const TensorLayout l = layout_of(*norm);
  for (uint32_t i = 0; i < n; i++) {
    if (!rect_inside(jobs[i].rect, ss) || !rect_inside(jobs[i].dst_rect, ds)) return VPF_ERR_BAD_ARG;
    if (!tensor_src_ok(sf, ss.width, jobs[i].src)) return VPF_ERR_BAD_ARG;
    if (!tensor_planes_ok(jobs[i].dst, l, ds.width)) return VPF_ERR_BAD_ARG;
  }
  DeviceGuard guard(exec->device);
  if (guard.err != hipSuccess) return status_of(guard.err);
  Yuv2RgbCoef c;
  make_yuv2rgb(cs, cr, &c);
  const TensorEpi te = make_epi(*norm, opts ? opts->pad : nullptr);
  LetterboxDesc table[kLetterboxBatch];
  for (uint32_t base = 0; base < n; base += kLetterboxBatch) {
    const uint32_t m = (n - base < (uint32_t)kLetterboxBatch) ? n - base : (uint32_t)kLetterboxBatch;
    for (uint32_t i = 0; i < m; i++) {
      const vpf_letterbox_io& io = jobs[base + i];
      vpf_plane d[3];
      const int nd = tensor_planes(io.dst, l, d);
      LetterboxDesc& j = table[i];
      fill_desc(j.r.f, io.src, num_planes(sf), d, nd);
      j.r.x = io.rect.x; j.r.y = io.rect.y; j.r.w = io.rect.width; j.r.h = io.rect.height;
      j.ix = io.dst_rect.x; j.iy = io.dst_rect.y; j.iw = io.dst_rect.width; j.ih = io.dst_rect.height;
      j.r.scx = (float)j.r.w / (float)j.iw; j.r.scy = (float)j.r.h / (float)j.ih;
    }
    const hipStream_t st = static_cast<hipStream_t>(exec->stream);
    const hipError_t e = aa ? launch_convert_letterbox_aa(st, tensor_src_class(sf), c, ss.width, m, table, ds.width, ds.height, te, l.nhwc)
                            : launch_convert_letterbox(st, tensor_src_class(sf), c, ss.width, m, table, ds.width, ds.height, te, l.nhwc);
    if (e != hipSuccess) return status_of(e);
  }
  return VPF_OK;
}
vpf_status vpf_convert_letterbox_tensor(const vpf_exec* exec, int sf, int cs, int cr, vpf_size ss, vpf_size ds, uint32_t n,
                                        const vpf_letterbox_io* jobs, const vpf_tensor_norm* norm, const vpf_letterbox_opts* opts) {
  const Mark mark("vpf_convert_letterbox_tensor");
  return letterbox_tensor_call(exec, sf, cs, cr, ss, ds, n, jobs, norm, opts, false);
}
// The same jobs through the triangle filter of PIL and of torch's antialias=True (include/vpf_hip.h; k_convert_letterbox_aa.hip).
vpf_status vpf_convert_letterbox_tensor_aa(const vpf_exec* exec, int sf, int cs, int cr, vpf_size ss, vpf_size ds, uint32_t n,
                                           const vpf_letterbox_io* jobs, const vpf_tensor_norm* norm, const vpf_letterbox_opts* opts) {
  const Mark mark("vpf_convert_letterbox_tensor_aa");
  return letterbox_tensor_call(exec, sf, cs, cr, ss, ds, n, jobs, norm, opts, true);
}

// The same with the boxes, the optional placements and the count in DEVICE memory (include/vpf_hip.h): every check that needs no box happens here
// (dev_boxes_ok: the device-ROI entry's list), the guards and the fit in the kernel (k_convert_letterbox_dev.hip); one dispatch.
static_assert(sizeof(vpf_letterbox_dev) == 96 && offsetof(vpf_letterbox_dev, box_stride) == 24 && offsetof(vpf_letterbox_dev, dst) == 40 &&
                  offsetof(vpf_letterbox_dev, dst_job_stride) == 88,
              "vpf_letterbox_dev has no implicit padding");
vpf_status vpf_convert_letterbox_tensor_dev(const vpf_exec* exec, int sf, int cs, int cr, vpf_size ss, vpf_size ds, uint32_t n_frames,
                                            const vpf_frame_src* frames, const vpf_letterbox_dev* table, const vpf_tensor_norm* norm,
                                            const vpf_letterbox_opts* opts) {
  const Mark mark("vpf_convert_letterbox_tensor_dev");
  if (tensor_src_class(sf) < 0 || !cscr_ok(cs, cr)) return VPF_ERR_UNSUPPORTED;
  if (const vpf_status refused = norm_status(norm, false, opts && opts->reserved)) return refused;
  const TensorLayout l = layout_of(*norm);
  if (!table || !dev_boxes_ok(exec, sf, ss, ds, n_frames, frames, table->boxes, table->count, table->box_stride, table->max_n, table->dst, table->dst_job_stride, l))
    return VPF_ERR_BAD_ARG;
  if (((uintptr_t)table->dst_rects & 3u) || (table->dst_rects && (table->rect_stride < 16u || (table->rect_stride & 3u))) || table->reserved) return VPF_ERR_BAD_ARG;
  DeviceGuard guard(exec->device);
  if (guard.err != hipSuccess) return status_of(guard.err);
  Yuv2RgbCoef c;
  make_yuv2rgb(cs, cr, &c);
  const TensorEpi te = make_epi(*norm, opts ? opts->pad : nullptr);
  LetterboxDevArgs a;
  fill_dev_boxes(a, frames, n_frames, num_planes(sf), table->boxes, table->count, table->box_stride, table->max_n, table->dst, table->dst_job_stride, l);
  a.rects = table->dst_rects;
  a.rect_stride = table->dst_rects ? table->rect_stride : 0u;
  return status_of(launch_convert_letterbox_dev(static_cast<hipStream_t>(exec->stream), tensor_src_class(sf), c, ss.width, ss.height, a, ds.width, ds.height, te, l.nhwc));
}

// Many affine warps of decoded frames -> one batch of normalised planes (include/vpf_hip.h): per-job matrices, kWarpBatch jobs per job table,
// each table at most two dispatches (k_convert_warp.hip).
vpf_status vpf_convert_warp_tensor(const vpf_exec* exec, int sf, int cs, int cr, vpf_size ss, vpf_size ds, uint32_t n, const vpf_warp_io* jobs,
                                   const vpf_tensor_norm* norm, const vpf_warp_opts* opts) {
  const Mark mark("vpf_convert_warp_tensor");
  if (tensor_src_class(sf) < 0 || !cscr_ok(cs, cr)) return VPF_ERR_UNSUPPORTED;
  if (const vpf_status refused = norm_status(norm, opts && opts->border_mode > VPF_WARP_REPLICATE, opts && opts->reserved)) return refused;
  if (!exec || !jobs || !n || !dims_ok(ss) || !dims_ok(ds)) return VPF_ERR_BAD_ARG;
  const TensorLayout l = layout_of(*norm);
  for (uint32_t i = 0; i < n; i++) {
    for (int k = 0; k < 6; k++)
      if (!(std::fabs(jobs[i].m[k]) <= 16777216.0f)) return VPF_ERR_BAD_ARG;  // NaN and infinities fail the comparison too
    if (!tensor_src_ok(sf, ss.width, jobs[i].src, true)) return VPF_ERR_BAD_ARG;
    if (!tensor_planes_ok(jobs[i].dst, l, ds.width, true)) return VPF_ERR_BAD_ARG;
  }
  DeviceGuard guard(exec->device);
  if (guard.err != hipSuccess) return status_of(guard.err);
  Yuv2RgbCoef c;
  make_yuv2rgb(cs, cr, &c);
  const TensorEpi te = make_epi(*norm, opts ? opts->border : nullptr, opts ? opts->border_mode : 0u);
  WarpDesc table[kWarpBatch];
  for (uint32_t base = 0; base < n; base += kWarpBatch) {
    const uint32_t m = (n - base < (uint32_t)kWarpBatch) ? n - base : (uint32_t)kWarpBatch;
    for (uint32_t i = 0; i < m; i++) {
      const vpf_warp_io& io = jobs[base + i];
      vpf_plane d[3];
      const int nd = tensor_planes(io.dst, l, d);
      fill_desc(table[i].f, io.src, num_planes(sf), d, nd);
      for (int k = 0; k < 6; k++) table[i].m[k] = io.m[k];
    }
    const hipError_t e = launch_convert_warp(static_cast<hipStream_t>(exec->stream), tensor_src_class(sf), c, ss.width, ss.height, m, table, ds.width,
                                             ds.height, te, l.nhwc);
    if (e != hipSuccess) return status_of(e);
  }
  return VPF_OK;
}

// Many perspective warps of decoded frames -> one batch of normalised planes (include/vpf_hip.h): the warp entry's checks on nine coefficients,
// kPerspBatch jobs per job table, each table at most two dispatches (k_convert_persp.hip).
vpf_status vpf_convert_persp_tensor(const vpf_exec* exec, int sf, int cs, int cr, vpf_size ss, vpf_size ds, uint32_t n, const vpf_persp_io* jobs,
                                    const vpf_tensor_norm* norm, const vpf_warp_opts* opts) {
  const Mark mark("vpf_convert_persp_tensor");
  if (tensor_src_class(sf) < 0 || !cscr_ok(cs, cr)) return VPF_ERR_UNSUPPORTED;
  if (const vpf_status refused = norm_status(norm, opts && opts->border_mode > VPF_WARP_REPLICATE, opts && opts->reserved)) return refused;
  if (!exec || !jobs || !n || !dims_ok(ss) || !dims_ok(ds)) return VPF_ERR_BAD_ARG;
  const TensorLayout l = layout_of(*norm);
  for (uint32_t i = 0; i < n; i++) {
    for (int k = 0; k < 9; k++)
      if (!(std::fabs(jobs[i].m[k]) <= 16777216.0f)) return VPF_ERR_BAD_ARG;  // NaN and infinities fail the comparison too
    if (jobs[i].reserved) return VPF_ERR_BAD_ARG;
    if (!tensor_src_ok(sf, ss.width, jobs[i].src, true)) return VPF_ERR_BAD_ARG;
    if (!tensor_planes_ok(jobs[i].dst, l, ds.width, true)) return VPF_ERR_BAD_ARG;
  }
  DeviceGuard guard(exec->device);
  if (guard.err != hipSuccess) return status_of(guard.err);
  Yuv2RgbCoef c;
  make_yuv2rgb(cs, cr, &c);
  const TensorEpi te = make_epi(*norm, opts ? opts->border : nullptr, opts ? opts->border_mode : 0u);
  PerspDesc table[kPerspBatch];
  for (uint32_t base = 0; base < n; base += kPerspBatch) {
    const uint32_t m = (n - base < (uint32_t)kPerspBatch) ? n - base : (uint32_t)kPerspBatch;
    for (uint32_t i = 0; i < m; i++) {
      const vpf_persp_io& io = jobs[base + i];
      vpf_plane d[3];
      const int nd = tensor_planes(io.dst, l, d);
      fill_desc(table[i].f, io.src, num_planes(sf), d, nd);
      for (int k = 0; k < 9; k++) table[i].m[k] = io.m[k];
    }
    const hipError_t e = launch_convert_persp(static_cast<hipStream_t>(exec->stream), tensor_src_class(sf), c, ss.width, ss.height, m, table, ds.width,
                                              ds.height, te, l.nhwc);
    if (e != hipSuccess) return status_of(e);
  }
  return VPF_OK;
}

// The two warps with the matrices in DEVICE memory (include/vpf_hip.h) through their one host path (matrices_dev_entry); one dispatch each.
vpf_status vpf_convert_warp_tensor_dev(const vpf_exec* exec, int sf, int cs, int cr, vpf_size ss, vpf_size ds, uint32_t n_frames, const vpf_frame_src* frames,
                                       const vpf_warps_dev* table, const vpf_tensor_norm* norm, const vpf_warp_opts* opts) {
  const Mark mark("vpf_convert_warp_tensor_dev");
  return matrices_dev_entry<6>(exec, sf, cs, cr, ss, ds, n_frames, frames, table, norm, opts, launch_convert_warp_dev);
}
vpf_status vpf_convert_persp_tensor_dev(const vpf_exec* exec, int sf, int cs, int cr, vpf_size ss, vpf_size ds, uint32_t n_frames, const vpf_frame_src* frames,
                                        const vpf_persps_dev* table, const vpf_tensor_norm* norm, const vpf_warp_opts* opts) {
  const Mark mark("vpf_convert_persp_tensor_dev");
  return matrices_dev_entry<9>(exec, sf, cs, cr, ss, ds, n_frames, frames, table, norm, opts, launch_convert_persp_dev);
}
// The caller's LDS hint for one homography (include/vpf_hip.h): persp_step, vpf_job_bounds.h.  0: no bound.
float vpf_persp_max_step(const float m[9], vpf_size dst) {
  if (!m || !dims_ok(dst)) return 0.f;
  for (int k = 0; k < 9; k++)
    if (!(std::fabs(m[k]) <= 16777216.0f)) return 0.f;
  return persp_step(m, dst.width, dst.height);
}

// Many per-pixel remaps of decoded frames -> one batch of normalised planes (include/vpf_hip.h): the warp entry's checks, then the maps' — their
// pointers and pitches only: the maps are device data the host never reads —, kRemapBatch jobs per job table, one dispatch each (k_convert_remap.hip).
static_assert(sizeof(vpf_remap_io) == 120 && offsetof(vpf_remap_io, dst) == 48 && offsetof(vpf_remap_io, xmap) == 96 && offsetof(vpf_remap_io, ymap) == 104 &&
                  offsetof(vpf_remap_io, xmap_pitch) == 112 && offsetof(vpf_remap_io, ymap_pitch) == 116 && sizeof(vpf_remap_opts) == 16,
              "vpf_remap_io and vpf_remap_opts have no implicit padding");
vpf_status vpf_convert_remap_tensor(const vpf_exec* exec, int sf, int cs, int cr, vpf_size ss, vpf_size ds, uint32_t n, const vpf_remap_io* jobs,
                                    const vpf_tensor_norm* norm, const vpf_remap_opts* opts) {
  const Mark mark("vpf_convert_remap_tensor");
  if (tensor_src_class(sf) < 0 || !cscr_ok(cs, cr)) return VPF_ERR_UNSUPPORTED;
  if (const vpf_status refused = norm_status(norm, opts && opts->border_mode > VPF_WARP_REPLICATE,
                                             opts && (opts->reserved || opts->reserved2 || !(opts->max_step >= 0.f) || !std::isfinite(opts->max_step))))
    return refused;
  if (!exec || !jobs || !n || !dims_ok(ss) || !dims_ok(ds)) return VPF_ERR_BAD_ARG;
  const TensorLayout l = layout_of(*norm);
  for (uint32_t i = 0; i < n; i++) {
    const vpf_remap_io& io = jobs[i];
    if (!io.xmap || !io.ymap || (((uintptr_t)io.xmap | (uintptr_t)io.ymap | io.xmap_pitch | io.ymap_pitch) & 3u) || (uint64_t)io.xmap_pitch < 4ull * ds.width ||
        (uint64_t)io.ymap_pitch < 4ull * ds.width)
      return VPF_ERR_BAD_ARG;
    if (!tensor_src_ok(sf, ss.width, io.src, true)) return VPF_ERR_BAD_ARG;
    if (!tensor_planes_ok(io.dst, l, ds.width, true)) return VPF_ERR_BAD_ARG;
  }
  DeviceGuard guard(exec->device);
  if (guard.err != hipSuccess) return status_of(guard.err);
  Yuv2RgbCoef c;
  make_yuv2rgb(cs, cr, &c);
  const TensorEpi te = make_epi(*norm, opts ? opts->border : nullptr, opts ? opts->border_mode : 0u);
  RemapDesc table[kRemapBatch];
  for (uint32_t base = 0; base < n; base += kRemapBatch) {
    const uint32_t m = (n - base < (uint32_t)kRemapBatch) ? n - base : (uint32_t)kRemapBatch;
    for (uint32_t i = 0; i < m; i++) {
      const vpf_remap_io& io = jobs[base + i];
      vpf_plane d[3];
      const int nd = tensor_planes(io.dst, l, d);
      fill_desc(table[i].f, io.src, num_planes(sf), d, nd);
      table[i].xm = io.xmap; table[i].ym = io.ymap; table[i].xp = io.xmap_pitch; table[i].yp = io.ymap_pitch;
    }
    const hipError_t e = launch_convert_remap(static_cast<hipStream_t>(exec->stream), tensor_src_class(sf), c, ss.width, ss.height, m, table, ds.width, ds.height,
                                              opts ? opts->max_step : 0.f, te, l.nhwc);
    if (e != hipSuccess) return status_of(e);
  }
  return VPF_OK;
}

// Planar float tensor -> NV12 / YUV420 (include/vpf_hip.h): quantise, BT.601 RGB -> YUV and the 4:2:0 mean in one kernel.
int vpf_tensor_convert_supported(int df, int cs, int cr) {
  return (df == VPF_FMT_NV12 || df == VPF_FMT_YUV420) && classify(VPF_FMT_RGB_PLANAR, VPF_FMT_YUV420, cs, cr) == FAM_RGB2YUV;
}

vpf_status vpf_tensor_convert_batch(const vpf_exec* exec, int df, int cs, int cr, vpf_size size, uint32_t n, const vpf_frame_io* frames,
                                    const vpf_tensor_norm* denorm) {
  const Mark mark("vpf_tensor_convert_batch");
  if (!vpf_tensor_convert_supported(df, cs, cr)) return VPF_ERR_UNSUPPORTED;
  if (const vpf_status refused = norm_status(denorm)) return refused;
  if (!exec || !frames || !n || !dims_ok(size)) return VPF_ERR_BAD_ARG;
  const TensorLayout l = layout_of(*denorm);
  for (uint32_t i = 0; i < n; i++) {
    if (!tensor_planes_ok(frames[i].src, l, size.width)) return VPF_ERR_BAD_ARG;
    if (!planes_ok(df, size.width, frames[i].dst)) return VPF_ERR_BAD_ARG;
  }
  DeviceGuard guard(exec->device);
  if (guard.err != hipSuccess) return status_of(guard.err);
  Rgb2YuvCoef rc;
  make_rgb2yuv(cr, &rc);
  // the kernels read channel k (R G B) from plane k with parameter k; B G R order swaps planes 0 and 2 and their parameters here
  TensorPro tp;
  std::memset(&tp, 0, sizeof(tp));
  kernel_scale_bias(*denorm, tp.scale, tp.bias);
  tp.dtype = denorm->dtype;
  tp.pad = l.nhwc && l.bgr ? 1u : 0u;
  const int nd = num_planes(df);
  for (uint32_t base = 0; base < n; base += kSmallBatch) {
    const uint32_t m = (n - base < (uint32_t)kSmallBatch) ? n - base : (uint32_t)kSmallBatch;
    BatchArgs a;
    for (uint32_t i = 0; i < m; i++) {
      vpf_plane s[3];
      const int ns = tensor_planes(frames[base + i].src, l, s);
      fill_desc(a.f[i], s, ns, frames[base + i].dst, nd);
    }
    for (uint32_t i = m; i < (uint32_t)kSmallBatch; i++) a.f[i] = a.f[0];
    const hipError_t e = launch_tensor_to_yuv(static_cast<hipStream_t>(exec->stream), df == VPF_FMT_NV12, rc, tp, size.width, size.height, m, a, l.nhwc);
    if (e != hipSuccess) return status_of(e);
  }
  return VPF_OK;
}

vpf_status vpf_tensor_convert(const vpf_exec* exec, int df, int cs, int cr, vpf_size size, const vpf_plane src[3], const vpf_plane dst[3],
                              const vpf_tensor_norm* denorm) {
  if (!vpf_tensor_convert_supported(df, cs, cr)) return VPF_ERR_UNSUPPORTED;
  if (!src || !dst) return VPF_ERR_BAD_ARG;
  const vpf_frame_io io = single_frame(src, 3, dst, num_planes(df));
  return vpf_tensor_convert_batch(exec, df, cs, cr, size, 1, &io, denorm);
}

const char* vpf_status_string(int s) {
  switch (s) {
    case VPF_OK: return "ok";
    case VPF_ERR_UNSUPPORTED: return "unsupported format / colour-space combination";
    case VPF_ERR_BAD_ARG: return "bad argument";
    case VPF_ERR_LAUNCH: return "HIP launch failed";
    case VPF_ERR_NO_DEVICE: return "no usable HIP device";
    default: return "unknown status";
  }
}
const char* vpf_version(void) { return "vpf-hip 0.1 (gfx950)"; }
int vpf_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}
/* Additive, for the Task layer's marks (the reference brackets every Task::Run with an NvtxMark): a roctx range when VPF_HIP_ROCTX=1,
 * nothing otherwise.  vpf_trace_push returns 1 if a range was opened (pass that to vpf_trace_pop). */
int vpf_trace_push(const char* name) {
  if (!trace_on()) return 0;
  trace_push(name);
  return 1;
}
void vpf_trace_pop(int opened) { if (opened) trace_pop(); }

int vpf_set_tuning(int key, int value) {
  if (key == VPF_TUNE_RESIZE_TILE) {
    const int ty = value & 0xff, wpb = value >> 8;
    if (value != 0 && (ty < 4 || ty > 64 || (ty & 3) || (wpb != 4 && wpb != 8))) return -1;
    return g_tune_tile.exchange(value);
  }
  if (key == VPF_TUNE_RESIZE_MFMA) {
    const int shape = value & 0xffff, nt = shape >> 8, tiles = shape & 0xff;  // | 0x10000: no weight tables; | 0x20000: the two-role kernel form; | 0x40000: small single planes too; | 0x80000: no ring of two
    if (value < 0 || (value & ~0xfffff)) return -1;
#ifndef VPF_LAB_FORMS
    if (value & 0x20000) return -1;  // the two-role form lives in the lab build (tools/lab/libvpfhip_forms.so)
#endif
    if (shape != 0 && shape != 1 && ((nt != 0 && nt != 4 && nt != 8) || tiles > 64 || (nt == 0 && tiles < 2))) return -1;
    return g_tune_mfma.exchange(value);
  }
  if (key == VPF_TUNE_RESIZE_BAND) {
    const int rows = value & 0xff, nb = (value >> 8) & 0xff, form = value >> 16;  // nb: bands per wave of the march form (4-row bands only) / bands per chunk of the persistent launch
    // form: | 1 the persistent launch, | 2 eight pixels per lane on every 1-channel plane, | 4 persistent waves visit every XCD's counter
    const bool ok = value >= 0 && (rows == 0 || rows == 1 || rows == 2 || rows == 4 || rows == 8 || rows == 16) && nb <= 8 && (nb == 0 || rows == 4 || (form & 1)) && form <= 15 && (!(form & 12) || (form & 1));  // | 8 (measurement) persistent waves stride through their share, no counters
#ifndef VPF_LAB_FORMS
    if (form & 13) return -1;  // the persistent launch and its knobs live in the lab build (tools/lab/libvpfhip_forms.so)
#endif
    return ok ? g_tune_band.exchange(value) : -1;
  }
  if (key != VPF_TUNE_NV12_RGB_VARIANT) return -1;
  switch (value) {  // the kernels libvpfhip contains: every one writes the same pixels (include/vpf_hip.h)
#ifdef VPF_LAB_FORMS
    case 47:  // the per-wave strips of the fused kernel (rounds 2-4): lab build only
#endif
    case 0: case 4: case 8: case 9: case 12: case 30: case 37: case 40: case 43: case 44: case 45: case 46: case 48: case 49: return g_tune_variant.exchange(value);
    default: return -1;  // unknown value: nothing changes
  }
}

}  // extern "C"
