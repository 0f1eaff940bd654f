// vpf_convert_plan.h — the policy of the convert and relayout launches (vpf_convert, vpf_convert_batch, vpf_tensor_convert: launch_yuv_to_rgb of
// k_yuv2rgb.hip, launch_rgb_to_yuv and launch_tensor_to_yuv of k_rgb2yuv.hip, launch_relayout of k_relayout.hip) as ONE pure function: the
// refusal, or the kernel family (a row of kConvertForms), its template selectors, whether the scalar-argument single-frame entry is taken, the
// grid and the scalar kernel arguments.  Every launch is 256 lanes and no dynamic LDS.  No HIP in here: the four launchers include it and only
// dispatch on the result, and tests/test_convert_plan_cpu.py compiles the same header with g++ (tests/c/convert_plan_capi.cpp).  The measured
// reasons for every rule stand in the comments next to it.  Every form of a (source, destination) pair writes the same bytes.
#pragma once
#include <stdint.h>

#include "vpf_classes.h"
#include "vpf_hip.h"

namespace vpf {

enum ConvertLaunchKind : int {
  CONVERT_YUV2RGB = 0,  // launch_yuv_to_rgb: src = FC_NV12 / FC_YUV420 / FC_YUV444, dst = FC_RGB / FC_BGR / FC_PLANAR
  CONVERT_RGB2YUV,      // launch_rgb_to_yuv: src = FC_RGB / FC_BGR / FC_PLANAR, dst = FC_YUV444 / FC_YUV420
  CONVERT_TENSOR2YUV,   // launch_tensor_to_yuv: dtype, nv12, nhwc
  CONVERT_RELAYOUT,     // launch_relayout: src, dst = VPF_FMT_*
};

// What k_relayout_generic<OP> does (k_relayout.hip); OP_PLANAR_SWAP has no instantiation: RGB_PLANAR -> BGR is OP_PLANAR_RGB on exchanged planes
enum GenericOp : int {
  OP_NV12_YUV420, OP_YUV420_NV12, OP_RGB_PLANAR, OP_PLANAR_RGB, OP_SWAP_RB, OP_COPY_Y, OP_Y_YUV444,
  OP_RGB_RGB32F, OP_RGB32F_PLANAR, OP_P16_NV12, OP_RGB_GRAY, OP_BGR_GRAY, OP_PLANAR_GRAY, OP_PLANAR_SWAP
};

// Kernel families, one row of kConvertForms each.  Three tiers per converter: the r16 / p16 / x16 / r4 kernels (a wave = one row or row pair x
// 1024 px, every global access a dense 1-KiB run) for 16-px / 16-B regular frames, the p4 / p8 / p16 lane-group kernels for 4-B aligned ones, a
// generic per-pixel kernel for everything else.
enum ConvertForm : int {
  CF_NV12_PLANAR_R16 = 0, CF_NV12_RGB_P16X, CF_NV12_RGB_P16, CF_YUV420_RGB_P4, CF_YUV_RGB_GENERIC, CF_YUV444_RGB_R16, CF_YUV444_RGB_P4,
  CF_RGB_YUV_R16, CF_RGB_YUV_P4, CF_RGB_YUV_QUAD,
  CF_TENSOR_YUV_R, CF_TENSOR_YUV_QUAD,
  CF_NV12_YUV420_R16, CF_NV12_YUV420_P16, CF_RGB_RELAYOUT_R16, CF_RGB_RELAYOUT_P4, CF_COPY_PLANE_P16, CF_U8_TO_F32_X4, CF_U8_TO_F32_P4,
  CF_RGB32F_PLANAR_R4, CF_P16_TO_8_X16, CF_P16_TO_8_P8, CF_GRAY_R16, CF_GRAY_P4, CF_RELAYOUT_GENERIC,
  CONVERT_FORMS
};
// name: what the selection log prints in front of the template arguments (the single-frame entry: name + "_one"); targs: the fields of
// ConvertPlan the template-id is made of, in its order ("1", "4": a constant; to_planar, fill: `mode` as a bool; the single-frame entries of the
// p16 / p16x forms have no ballast argument; the kernels without a field in it are launched by name and logged without brackets); args: the
// scalar kernel arguments ConvertPlan::a holds, in the kernel's order
struct ConvertFormInfo { const char* name; bool has_one; const char* targs; const char* args; };
constexpr ConvertFormInfo kConvertForms[CONVERT_FORMS] = {
    {"k_nv12_planar_r16", true, "nts src", "w h chunks tasks"},           // NV12 / YUV420 -> planar: one row x 1024 px per wave, three 1-KiB plane stores
    {"k_nv12_rgb_p16x", true, "dst nts ballast src", "bpr nb"},           // ... -> packed, blocks numbered straight through the picture
    {"k_nv12_rgb_p16", true, "dst nts ballast src", "w h chunks tasks"},  // ... -> any, one row pair x 1024 px per wave, LDS transpose for the stores
    {"k_yuv420_rgb_p4", true, "src dst", "w h chunks tasks"},             // ... 4 px per lane, 4-B aligned planes, any size
    {"k_yuv_rgb_generic", false, "src dst", "w h"},                       // one lane per 2x2 quad, byte accesses (YUV444 too)
    {"k_yuv444_rgb_r16", true, "dst", "w h chunks tasks"},
    {"k_yuv444_rgb_p4", false, "dst 1", "w h groups"},
    {"k_rgb_yuv_r16", true, "src sub", "w h chunks tasks"},
    {"k_rgb_yuv_p4", false, "src sub", "w h groups"},
    {"k_rgb_yuv_quad", false, "src sub", "w h"},
    {"k_tensor_yuv_r", false, "dtype nv12 nhwc", "w h chunks tasks"},
    {"k_tensor_yuv_quad", false, "nv12 nhwc", "w h"},
    {"k_nv12_yuv420_r16", true, "to_planar", "w h cx luma cc total"},     // to_planar = (mode != 0): NV12 -> YUV420; else YUV420 -> NV12
    {"k_nv12_yuv420_p16", false, "to_planar", "w h groups"},
    {"k_rgb_relayout_r16", true, "mode", "w h chunks tasks"},             // mode: 0 = packed -> planar, 1 = planar -> packed, 2 = R <-> B
    {"k_rgb_relayout_p4", false, "mode", "w h groups"},
    {"k_copy_plane_p16", false, "fill", "w h groups"},                    // fill = (mode != 0): also fills two more planes with 128 (Y -> YUV444)
    {"k_u8_to_f32_x4", true, "4", "wd h chunks tasks"},                   // wd: dwords of a packed row, 3 w / 4
    {"k_u8_to_f32_p4", false, "", "wbytes h groups"},
    {"k_rgb32f_planar_r4", true, "", "w h chunks tasks"},
    {"k_p16_to_8_x16", true, "", "w h ch chunks tasks"},                  // ch: chroma rows, (h + 1) / 2
    {"k_p16_to_8_p8", false, "", "w h ch groups"},
    {"k_gray_r16", true, "mode", "w h chunks tasks"},                     // mode: source 0 = RGB, 1 = BGR, 2 = RGB_PLANAR
    {"k_gray_p4", false, "mode", "w h groups"},
    {"k_relayout_generic", false, "mode", "w h"},                         // mode: GenericOp
};

// What the policy looks at.  `src_bits[k]` / `dst_bits[k]`: pointer | pitch of plane k OR-ed over the n frames of the dispatch (convert_shape,
// k_job_launch.h: one pass over the frame table) — every alignment test below asks whether ALL frames are multiples of 2, 4, 8 or 16.
struct ConvertShape {
  int kind;      // ConvertLaunchKind
  int src, dst;  // FmtClass (CONVERT_YUV2RGB, CONVERT_RGB2YUV) or VPF_FMT_* (CONVERT_RELAYOUT)
  uint32_t w, h, n;
  uint64_t src_bits[3], dst_bits[3];
  int variant;      // tuning(VPF_TUNE_NV12_RGB_VARIANT), read once by the caller
  bool dst_reused;  // VPF_EXEC_DST_REUSED (CONVERT_YUV2RGB)
  uint32_t dtype;   // CONVERT_TENSOR2YUV: VPF_TENSOR_*
  bool nv12, nhwc;  // CONVERT_TENSOR2YUV: NV12 (else YUV420) out; one interleaved source plane
};
struct ConvertPlan {
  bool ok;   // false: refused (hipErrorInvalidValue), nothing is launched
  int form;  // ConvertForm
  // the scalar-argument single-frame entry (kernarg preload, vpf_internal.h): exactly when the DISPATCH has one frame and the form has such an
  // entry.  vpf_convert_batch cuts a call into dispatches of 32: a call of 33 frames ends in a dispatch of one, which takes this entry — unlike
  // the plain resize, whose entry rule asks the call (ResizeShape::call_n).
  bool one;
  // template selectors (ConvertFormInfo::targs says which of them a form has)
  int src, dst;    // FmtClass
  bool nts;        // non-temporal stores (false: allocating stores, VPF_EXEC_DST_REUSED)
  int ballast;     // KiB of LDS ballast: 16 -> 40 KiB per workgroup, 4 instead of 6 workgroups per CU; 0 in the single-frame entries
  bool sub;        // 4:2:0 output of the RGB -> YUV kernels
  int mode;        // the relayout kernels' one selector (kConvertForms)
  uint32_t dtype;  // CF_TENSOR_YUV_R
  bool nv12, nhwc;
  uint32_t gx, gy, gz;  // the task kernels (chunks / tasks arguments) take the frame from blockIdx.y: gy = n, gz = 1; the others from blockIdx.z
  int na;
  uint32_t a[6];  // ConvertFormInfo::args
  // BGR <-> RGB_PLANAR is the RGB kernel on a copy of the frame table with planes 0 and 2 of the planar side exchanged
  bool swap_src02, swap_dst02;
};

// every frame's source plane k < ns is a multiple of (k ? s12 : s0), its destination plane k < nd of (k ? d12 : d0) — powers of two
inline bool convert_aligned(const ConvertShape& q, int ns, int nd, uint32_t s0, uint32_t s12, uint32_t d0, uint32_t d12) {
  for (int k = 0; k < ns; k++)
    if (q.src_bits[k] & ((k ? s12 : s0) - 1)) return false;
  for (int k = 0; k < nd; k++)
    if (q.dst_bits[k] & ((k ? d12 : d0) - 1)) return false;
  return true;
}

namespace convert_detail {
inline void set_args(ConvertPlan& P, uint32_t a0, uint32_t a1, uint32_t a2 = 0, uint32_t a3 = 0, uint32_t a4 = 0, uint32_t a5 = 0, int na = 2) {
  P.na = na;
  P.a[0] = a0; P.a[1] = a1; P.a[2] = a2; P.a[3] = a3; P.a[4] = a4; P.a[5] = a5;
}
// a task kernel: a wave takes task blockIdx.x * 4 + wave of `chunks` x rows of them, blockIdx.y is the frame; args (w, h, chunks, tasks)
inline void task_form(ConvertPlan& P, const ConvertShape& q, int form, uint32_t w_arg, uint32_t chunks, uint32_t rows) {
  P.form = form;
  P.one = q.n == 1 && kConvertForms[form].has_one;
  P.gx = (chunks * rows + 3) / 4; P.gy = q.n; P.gz = 1;
  set_args(P, w_arg, q.h, chunks, chunks * rows, 0, 0, 4);
}
// a lane-group kernel: a lane takes group blockIdx.x * 64 + lane of `groups` in row (pair) blockIdx.y * 4 + wave; args (w, h, groups)
inline void group_form(ConvertPlan& P, const ConvertShape& q, int form, uint32_t w_arg, uint32_t groups, uint32_t rows) {
  P.form = form;
  P.gx = (groups + 63) / 64; P.gy = (rows + 3) / 4; P.gz = q.n;
  set_args(P, w_arg, q.h, groups, 0, 0, 0, 3);
}
// one lane per 2x2 quad: args (w, h)
inline void quad_form(ConvertPlan& P, const ConvertShape& q, int form) {
  P.form = form;
  P.gx = ((q.w + 1) / 2 + 63) / 64; P.gy = ((q.h + 1) / 2 + 3) / 4; P.gz = q.n;
  set_args(P, q.w, q.h);
}

// Kernel selection for 4:2:0 sources.  `variant` is the tuning hint (include/vpf_hip.h): 0 = policy below; a named kernel
// (4 / 8 / 12 / 30 / 37 / 44 / 45 / 46) is honoured where it applies and falls back down the same chain where it does not; 40 = the
// narrower p4 path, 9 = the any-input generic kernel.
//   p16x (45 | 46: 4 workgroups / CU)                                               packed outputs, w >= 1024: blocks numbered straight through the picture
//   p16  (8: non-temporal stores | 12: allocating stores | 30: 4 workgroups / CU)   packed outputs; w % 16 == 0, h even, 16-B aligned
//   r16  (37: non-temporal | 44: allocating stores)                                 planar outputs; same conditions
//        (the straight numbering applied to r16 measured 1 % SLOWER on the 1080p planar batch, 0.779 vs 0.787 in same-box A/B: not kept)
//   p4   (4)                                                                        4-B aligned planes, any size
//   generic (9)                                                                     anything
inline void plan_420(ConvertPlan& P, const ConvertShape& q) {
  const uint32_t w = q.w, h = q.h, n = q.n;
  const bool nv12 = q.src == FC_NV12, planar = q.dst == FC_PLANAR;
  const int nsrc = nv12 ? 2 : 3, ndst = planar ? 3 : 1;
  int variant = q.variant;
  // VPF_EXEC_DST_REUSED: single-frame launches keep their output in the Infinity Cache (allocating stores) for the next
  // kernel of the chain: variant 12 = p16 with non-temporal loads only, 44 = planar r16 with plain stores
  if (variant == 0 && q.dst_reused && n < 4) variant = planar ? 44 : 12;
  const bool even = (w % 4 == 0) && (h % 2 == 0);
  const bool p16_ok = even && (w % 16 == 0) && convert_aligned(q, nsrc, ndst, 16, nv12 ? 16 : 8, 16, 16);
  const bool p4_ok = convert_aligned(q, nsrc, ndst, 4, nv12 ? 4 : 2, 4, 4);
  const bool big_single = n < 4 && (uint64_t)w * h >= (uint64_t)3 << 20;
  // (the kernel numbers its blocks in 32 bits, (blockIdx.x * 4 + wave) * 64 + lane: fewer than 2^30 of them.  A guard only: the C ABI stops at
  // 65536 x 65536 pixels, 2^27 blocks)
  const bool p16x_ok = p16_ok && !planar && w >= 1024 && (uint64_t)(w / 16) * (h / 2) < (1u << 30);
  // values of the shared tuning key that name no NV12 / YUV420 -> RGB kernel (43 = a resize-only hint, anything unknown) mean the default policy
  if (variant != 4 && variant != 8 && variant != 9 && variant != 12 && variant != 30 && variant != 37 && variant != 40 && variant != 44 && variant != 45 && variant != 46) variant = 0;
  // Policy (profiles/r01_bench_sweep.log, r02_bench_sweep.log, tools/lab): packed -> p16x (p16 below 1024 px), with the 4-workgroup cap when the
  // launch is a batch (>= 4 frames: a narrower chip-wide write frontier is worth 1-2 %; short single-frame launches want all the waves they can
  // get; single frames: p16x measured level with p16, 0.710 vs 0.717); planar -> r16 (three 1-KiB plane stores per wave), except a lone frame of
  // >= 3 Mpx where the row-pair p16 form wins (kernel 7.3 vs 7.9 us at 4K, but 4.3 vs 3.6 at 1080p: tools/gpu_planar_single.sh).  The
  // alternatives that were measured and dropped (more row pairs per task, one-store-per-wave forms, XCD swizzles, other occupancy caps,
  // byte-stream stores) live in tools/lab/k_lab.hip.
  if (variant == 0) variant = p16_ok ? (planar ? (big_single ? 8 : 37) : (n >= 4 ? (p16x_ok ? 46 : 30) : 8)) : 4;
  if ((variant == 45 || variant == 46) && !p16x_ok) variant = variant == 46 ? 30 : 8;  // narrow frames / planar outputs: the chunk-per-row form
  const bool is_p16 = variant == 8 || variant == 12 || variant == 30, is_r16 = variant == 37 || variant == 44;
  if ((is_p16 || is_r16) && !p16_ok) variant = 4;
  if (is_r16 && !planar) variant = 4;  // r16 has no packed form
  if (variant != 9 && !p4_ok) variant = 9;  // p16_ok implies p4_ok
  const uint32_t chunks = (w + 1023) / 1024;
  if (variant == 37 || variant == 44) {
    task_form(P, q, CF_NV12_PLANAR_R16, w, chunks, h);  // one task per row per chunk (h even)
    P.nts = variant == 37;
  } else if (variant == 45 || variant == 46) {
    const uint32_t bpr = w / 16, nb = bpr * (h / 2);
    P.form = CF_NV12_RGB_P16X;
    P.one = n == 1;
    P.nts = true;
    P.ballast = (variant == 46 && !P.one) ? 16 : 0;
    P.gx = (nb + 255) / 256; P.gy = n; P.gz = 1;
    set_args(P, bpr, nb);
  } else if (variant == 8 || variant == 12 || variant == 30) {
    task_form(P, q, CF_NV12_RGB_P16, w, chunks, h / 2);
    P.nts = variant != 12;
    P.ballast = (variant == 30 && !P.one) ? 16 : 0;
  } else if (variant != 9) {  // 4, 40 and every fallback
    task_form(P, q, CF_YUV420_RGB_P4, w, ((w + 3) / 4 + 63) / 64, (h + 1) / 2);
  } else {
    quad_form(P, q, CF_YUV_RGB_GENERIC);
  }
}

// 4:4:4 sources: r16 (16-px widths, 16-B aligned; not under knob 9 or 40), p4 (4-px widths, 4-B aligned; not under knob 9 — and blockIdx.y is
// the row: h <= 65535), generic
inline void plan_444(ConvertPlan& P, const ConvertShape& q) {
  const uint32_t w = q.w, h = q.h;
  const int ndst = q.dst == FC_PLANAR ? 3 : 1, variant = q.variant;
  if (variant != 9 && variant != 40 && w % 16 == 0 && convert_aligned(q, 3, ndst, 16, 16, 16, 16)) {
    task_form(P, q, CF_YUV444_RGB_R16, w, (w + 1023) / 1024, h);
  } else if (variant != 9 && w % 4 == 0 && convert_aligned(q, 3, ndst, 4, 4, 4, 4) && h <= 65535) {
    P.form = CF_YUV444_RGB_P4;
    P.gx = (w / 4 + 255) / 256; P.gy = h; P.gz = q.n;
    set_args(P, w, h, w / 4, 0, 0, 0, 3);
  } else {
    quad_form(P, q, CF_YUV_RGB_GENERIC);
  }
}

// RGB / BGR / RGB_PLANAR -> YUV444 / YUV420: r16 not under knob 9 or 40, p4 not under knob 9 (and h even for 4:4:4 too: a lane owns two rows).
// (a lone 4K frame used to take the narrower p4 kernel — a row-pair wave halves the wave count, and p4 won by 8 %; with the scalar-argument
// single-frame entry r16 is the faster one again: 0.51 vs 0.47 of 8 TB/s)
inline void plan_rgb2yuv(ConvertPlan& P, const ConvertShape& q) {
  const uint32_t w = q.w, h = q.h;
  const bool sub = P.sub = q.dst == FC_YUV420;
  const int ns = q.src == FC_PLANAR ? 3 : 1, tv = q.variant;
  if (tv != 9 && tv != 40 && !(w & 15) && !(sub && (h & 1)) && convert_aligned(q, ns, 3, 16, 16, 16, sub ? 8 : 16))
    task_form(P, q, CF_RGB_YUV_R16, w, (w + 1023) / 1024, sub ? h / 2 : h);
  else if (tv != 9 && !(w & 3) && !(h & 1) && convert_aligned(q, ns, 3, 4, 4, 4, sub ? 2 : 4))
    group_form(P, q, CF_RGB_YUV_P4, w, w / 4, h / 2);
  else
    quad_form(P, q, CF_RGB_YUV_QUAD);
}

// float tensor -> NV12 / YUV420: the row-pair kernel (a lane: 8 f32 or 16 f16 / bf16 pixels) for 16-px widths, even heights, 16-B aligned
// source planes, luma and NV12 chroma, 8-B aligned YUV420 chroma; not under knob 9.  Only THIS path has the dtype as a template argument and
// refuses a value that is none of the three; the quad kernel branches on it at run time and is launched whatever it is (the C ABI has
// refused such a call before, norm_status of vpf_abi.hip).
inline void plan_tensor2yuv(ConvertPlan& P, const ConvertShape& q) {
  const uint32_t w = q.w, h = q.h;
  P.nv12 = q.nv12; P.nhwc = q.nhwc; P.dtype = q.dtype;
  if (q.variant != 9 && !(w & 15) && !(h & 1) && convert_aligned(q, q.nhwc ? 1 : 3, q.nv12 ? 2 : 3, 16, 16, 16, q.nv12 ? 16 : 8)) {
    if (q.dtype != VPF_TENSOR_F32 && q.dtype != VPF_TENSOR_F16 && q.dtype != VPF_TENSOR_BF16) { P.ok = false; return; }
    const uint32_t px = q.dtype == VPF_TENSOR_F32 ? 8 : 16;
    task_form(P, q, CF_TENSOR_YUV_R, w, (w + 64 * px - 1) / (64 * px), h / 2);
  } else {
    quad_form(P, q, CF_TENSOR_YUV_QUAD);
  }
}

// One relayout pair: its dense tier (knob 9 and knob 40 switch it off: 40 keeps the narrower fast paths for A/B measurements, and so the tests
// still cover them on regular frames), its lane-group tier (knob 9 switches it off) and the op of the generic kernel.  A tier: form 0 = none,
// its mode, the width modulus, whether h must be even, and the alignments convert_aligned asks.
struct RelayoutTier { int form, mode; uint32_t wmod; bool heven; uint32_t s0, s12, d0, d12; };
struct RelayoutRule { int ns, nd; RelayoutTier dense, group; int op; };
constexpr RelayoutTier kNoTier = {-1, 0, 1, false, 1, 1, 1, 1};
inline bool relayout_rule(int sf, int df, RelayoutRule& r) {
  const bool packed_s = sf == VPF_FMT_RGB || sf == VPF_FMT_BGR, packed_d = df == VPF_FMT_RGB || df == VPF_FMT_BGR;
  // the r16 form moves luma in 1024-px and chroma in 2048-px chunks of whole 16-B runs per plane: w % 32 (16 chroma samples per run)
  if (sf == VPF_FMT_NV12 && df == VPF_FMT_YUV420)
    r = {2, 3, {CF_NV12_YUV420_R16, 1, 32, true, 16, 16, 16, 16}, {CF_NV12_YUV420_P16, 1, 16, true, 16, 16, 16, 8}, OP_NV12_YUV420};
  else if (sf == VPF_FMT_YUV420 && df == VPF_FMT_NV12)
    r = {3, 2, {CF_NV12_YUV420_R16, 0, 32, true, 16, 16, 16, 16}, {CF_NV12_YUV420_P16, 0, 16, true, 16, 8, 16, 16}, OP_YUV420_NV12};
  else if (packed_s && df == VPF_FMT_RGB_PLANAR)  // (BGR: the destination's planes 0 and 2 exchanged)
    r = {1, 3, {CF_RGB_RELAYOUT_R16, 0, 16, false, 16, 16, 16, 16}, {CF_RGB_RELAYOUT_P4, 0, 4, false, 4, 4, 4, 4}, OP_RGB_PLANAR};
  else if (sf == VPF_FMT_RGB_PLANAR && packed_d)  // (BGR: the source's planes 0 and 2 exchanged)
    r = {3, 1, {CF_RGB_RELAYOUT_R16, 1, 16, false, 16, 16, 16, 16}, {CF_RGB_RELAYOUT_P4, 1, 4, false, 4, 4, 4, 4}, OP_PLANAR_RGB};
  else if (packed_s && packed_d && sf != df)
    r = {1, 1, {CF_RGB_RELAYOUT_R16, 2, 16, false, 16, 16, 16, 16}, {CF_RGB_RELAYOUT_P4, 2, 4, false, 4, 4, 4, 4}, OP_SWAP_RB};
  else if (sf == VPF_FMT_NV12 && df == VPF_FMT_Y)  // plane copies have no denser form than 16 B per lane
    r = {1, 1, kNoTier, {CF_COPY_PLANE_P16, 0, 16, false, 16, 16, 16, 16}, OP_COPY_Y};
  else if (sf == VPF_FMT_Y && df == VPF_FMT_YUV444)
    r = {1, 3, kNoTier, {CF_COPY_PLANE_P16, 1, 16, false, 16, 16, 16, 16}, OP_Y_YUV444};
  else if (sf == VPF_FMT_RGB && df == VPF_FMT_RGB_32F)  // a lane reads one dword: 4-B aligned sources in both tiers
    r = {1, 1, {CF_U8_TO_F32_X4, 4, 16, false, 4, 4, 16, 16}, {CF_U8_TO_F32_P4, 0, 4, false, 4, 4, 16, 16}, OP_RGB_RGB32F};
  else if (sf == VPF_FMT_RGB_32F && df == VPF_FMT_RGB_32F_PLANAR)  // a lane takes 4 pixels = 48 B: w % 4, not w % 16
    r = {1, 3, {CF_RGB32F_PLANAR_R4, 0, 4, false, 16, 16, 16, 16}, kNoTier, OP_RGB32F_PLANAR};
  else if ((sf == VPF_FMT_P10 || sf == VPF_FMT_P12) && df == VPF_FMT_NV12)  // luma and chroma rows both hold w 16-bit samples
    r = {2, 2, {CF_P16_TO_8_X16, 0, 16, false, 16, 16, 16, 16}, {CF_P16_TO_8_P8, 0, 8, false, 16, 16, 8, 8}, OP_P16_NV12};
  else if (df == VPF_FMT_Y && (packed_s || sf == VPF_FMT_RGB_PLANAR)) {
    const int s = sf == VPF_FMT_RGB ? 0 : sf == VPF_FMT_BGR ? 1 : 2;
    r = {s == 2 ? 3 : 1, 1, {CF_GRAY_R16, s, 16, false, 16, 16, 16, 16}, {CF_GRAY_P4, s, 4, false, 4, 4, 4, 4}, OP_RGB_GRAY + s};
  } else
    return false;
  return true;
}
inline void plan_relayout(ConvertPlan& P, const ConvertShape& q) {
  const uint32_t w = q.w, h = q.h;
  RelayoutRule r{};
  if (!relayout_rule(q.src, q.dst, r)) { P.ok = false; return; }
  // (the exchanged planes face the same alignment in every form that has them: the choice does not depend on the exchange)
  P.swap_dst02 = q.src == VPF_FMT_BGR && q.dst == VPF_FMT_RGB_PLANAR;
  P.swap_src02 = q.src == VPF_FMT_RGB_PLANAR && q.dst == VPF_FMT_BGR;
  auto takes = [&](const RelayoutTier& t) { return t.form >= 0 && w % t.wmod == 0 && !(t.heven && (h & 1)) && convert_aligned(q, r.ns, r.nd, t.s0, t.s12, t.d0, t.d12); };
  const RelayoutTier* t = nullptr;
  if (q.variant != 9 && q.variant != 40 && takes(r.dense)) t = &r.dense;
  else if (q.variant != 9 && takes(r.group)) t = &r.group;
  P.mode = t ? t->mode : r.op;
  const uint32_t cx = (w + 1023) / 1024, ch = (h + 1) / 2;
  switch (t ? t->form : (int)CF_RELAYOUT_GENERIC) {
    case CF_NV12_YUV420_R16: {  // luma rows in 1024-px chunks, then chroma rows in 2048-px chunks
      const uint32_t cc = (w + 2047) / 2048, luma = cx * h, total = luma + cc * (h / 2);
      P.form = CF_NV12_YUV420_R16;
      P.one = q.n == 1;
      P.gx = (total + 3) / 4; P.gy = q.n; P.gz = 1;
      set_args(P, w, h, cx, luma, cc, total, 6);
      break;
    }
    case CF_NV12_YUV420_P16: group_form(P, q, t->form, w, w / 16, h / 2); break;
    case CF_RGB_RELAYOUT_R16: case CF_GRAY_R16: task_form(P, q, t->form, w, cx, h); break;
    case CF_RGB_RELAYOUT_P4: case CF_GRAY_P4: group_form(P, q, t->form, w, w / 4, h); break;
    case CF_COPY_PLANE_P16: group_form(P, q, t->form, w, w / 16, h); break;
    case CF_U8_TO_F32_X4: {  // 4 loads + 4 stores per wave: measured 0.74 (2: 0.69, 8: 0.72)
      const uint32_t wd = 3 * w / 4;
      task_form(P, q, t->form, wd, (wd + 255) / 256, h);
      break;
    }
    case CF_U8_TO_F32_P4: group_form(P, q, t->form, 3 * w, 3 * w / 4, h); break;
    case CF_RGB32F_PLANAR_R4: task_form(P, q, t->form, w, (w + 255) / 256, h); break;
    case CF_P16_TO_8_X16:  // luma rows, then the chroma rows
      task_form(P, q, t->form, w, cx, h + ch);
      set_args(P, w, h, ch, cx, cx * (h + ch), 0, 5);
      break;
    case CF_P16_TO_8_P8:
      group_form(P, q, t->form, w, w / 8, h + ch);
      set_args(P, w, h, ch, w / 8, 0, 0, 4);
      break;
    default:  // one lane per pixel
      P.form = CF_RELAYOUT_GENERIC;
      P.gx = (w + 63) / 64; P.gy = (h + 3) / 4; P.gz = q.n;
      set_args(P, w, h);
  }
}
}  // namespace convert_detail

inline ConvertPlan convert_plan(const ConvertShape& q) {
  ConvertPlan P{};
  P.ok = true;
  P.src = q.src; P.dst = q.dst;
  switch (q.kind) {
    case CONVERT_YUV2RGB:
      if (q.dst != FC_RGB && q.dst != FC_BGR && q.dst != FC_PLANAR) P.ok = false;
      else if (q.src == FC_NV12 || q.src == FC_YUV420) convert_detail::plan_420(P, q);
      else if (q.src == FC_YUV444) convert_detail::plan_444(P, q);
      else P.ok = false;
      break;
    case CONVERT_RGB2YUV:
      if (q.src != FC_RGB && q.src != FC_BGR && q.src != FC_PLANAR) P.ok = false;
      else convert_detail::plan_rgb2yuv(P, q);
      break;
    case CONVERT_TENSOR2YUV: convert_detail::plan_tensor2yuv(P, q); break;
    case CONVERT_RELAYOUT: convert_detail::plan_relayout(P, q); break;
    default: P.ok = false;
  }
  return P;
}

}  // namespace vpf
