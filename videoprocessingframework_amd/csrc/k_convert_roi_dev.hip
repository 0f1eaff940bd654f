// k_convert_roi_dev.hip — the multi-ROI crop + bilinear resize of k_convert_roi.hip with the rectangles in DEVICE memory (gfx950):
// vpf_convert_resize_tensor_rois_dev.  A detector and its NMS leave their boxes on the GPU; this kernel reads (frame, x, y, w, h) of job blockIdx.z and
// the job count WHEN IT RUNS, so the call needs no sync and no copy to the host, and a captured graph replays with the boxes of replay time.
//   k_roi_dev      ONE dispatch over (tiles of 16 destination rows x 256 columns, max_n jobs).  A workgroup loads the count (jobs at or
//                  behind it write nothing), loads its box, runs the guard (roi_dev_box_ok: an invalid box reads no frame and writes the epilogue
//                  of byte 0), computes the job's scale factors — the correctly rounded fp32 quotients the host entry computes: no fast-math, no
//                  contraction in this translation unit — and then decides for ITS TILE (roi_tile_need, vpf_job_bounds.h): the staged form of
//                  k_roi_strip where the tile's strip fits the dispatch's LDS and converts at most kRoiConvMax source pixels per destination
//                  pixel, k_roi_gather's per-tap pixel otherwise.  A workgroup-uniform branch, as in k_warp_strip.
// The staged form is the function k_roi_strip runs (roi_strip_tile, k_convert_roi_common.h); the per-tap form runs k_roi_gather's fp32 operations
// in its order: identical bits to vpf_convert_resize_tensor_rois on the same rectangles, whichever form either entry picks.
#include "k_convert_roi_common.h"
#include "k_dev_table.h"
#include "k_job_launch.h"
#include "vpf_job_bounds.h"  // roi_dev_box_ok, roi_tile_window, roi_tile_need_of, roi_tile_staged: shared with the CPU tests

namespace vpf {

// The per-tap form: destination row y's four pixels of a lane, column taps tx[k] and row tap ty on the rectangle at (rx, ry) — k_roi_gather's pixel:
// texel_rgb at absolute frame coordinates, bilerp, truncation, the tensor epilogue, in its order.  A function of this unit and not one shared with
// k_roi_gather: called from there, that kernel ran 5 % slower.
template <int SRC, int DST>
VPF_DEV void roi_dev_gather4(const FrameDesc& f, const Yuv2RgbCoef& c, uint32_t rx, uint32_t ry, const Tap (&tx)[4], const Tap& ty, uint32_t x0, uint32_t y,
                         const TensorEpi& te, bool vec, uint32_t nv, uint32_t wv, uint32_t lane) {
  float o[3][4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    float p00[3], p01[3], p10[3], p11[3];
    texel_rgb<SRC>(f, c, rx + tx[k].i0, ry + ty.i0, p00);
    texel_rgb<SRC>(f, c, rx + tx[k].i1, ry + ty.i0, p01);
    texel_rgb<SRC>(f, c, rx + tx[k].i0, ry + ty.i1, p10);
    texel_rgb<SRC>(f, c, rx + tx[k].i1, ry + ty.i1, p11);
#pragma unroll
    for (int ch = 0; ch < 3; ch++) o[ch][k] = bilerp(p00[ch], p01[ch], p10[ch], p11[ch], tx[k].f, ty.f);
  }
  if constexpr (DST == FC_TENSOR_NHWC) {
    tensor_store4_nhwc_trunc<false>(f.d[0] + (size_t)y * f.dp[0], x0, &o[0][0], 4, 1, te, vec, nv, wv, lane);
  } else {
#pragma unroll
    for (int ch = 0; ch < 3; ch++) tensor_store4_trunc<false>(f.d[ch] + (size_t)y * f.dp[ch], x0, o[ch], 1, te, ch, vec, nv);
  }
}

template <int SRC, int DST>  // DST = FC_TENSOR: three planes per job; FC_TENSOR_NHWC: one interleaved plane
__global__ __launch_bounds__(256) void k_roi_dev(const RoiDevArgs args, const Yuv2RgbCoef c, uint32_t W, uint32_t H, uint32_t dw, uint32_t dh, uint32_t dmask,
                                                 uint32_t lds_bytes) {
  constexpr int R = kRoiBandRows;
  const uint32_t job = blockIdx.z;
  // 1. the count: jobs at or behind it write nothing
  if (job >= dev_job_count(args.count, args.max_n)) return;
  // 2. the five ints of this job, wave-uniform
  const DevBox5 b = dev_box5(args.boxes, args.box_stride, job);
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63, tid = threadIdx.x;
  const uint32_t Y0 = blockIdx.y * (4 * R), xs = blockIdx.x * 256;  // the grid covers the destination exactly: Y0 < dh, xs < dw
  const uint32_t Y1 = (Y0 + 4 * R - 1 < dh - 1) ? Y0 + 4 * R - 1 : dh - 1, xe = (xs + 255 < dw - 1) ? xs + 255 : dw - 1;
  const TensorEpi te = args.e;
  FrameDesc f;
  dev_dst_planes<DST>(args, job, f);
  const uint32_t ya = Y0 + wv * R, yb = (ya + R - 1 < Y1) ? ya + R - 1 : Y1;  // this wave's rows (none when ya > Y1)
  const uint32_t x0 = xs + lane * 4;                                        // this lane's four columns (none when x0 >= dw)
  const uint32_t nv = x0 < dw ? (dw - x0 < 4 ? dw - x0 : 4) : 0;
  const bool vec = tensor_vec_ok<DST>(f, nv, dmask);
  // 3. the guard (vpf_job_bounds.h): an invalid box reads no frame; its tile takes the epilogue of byte 0
  if (!roi_dev_box_ok(b.f, b.x, b.y, b.w, b.h, args.n_frames, W, H)) {
    if (ya > Y1 || !nv) return;
    for (uint32_t y = ya; y <= yb; y++) {
      if constexpr (DST == FC_TENSOR_NHWC) {
        const float u[3][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
        tensor_store_nhwc<false, 4>(f.d[0] + (size_t)y * f.dp[0], x0, u, te, vec, nv, kNoStage, 0u);
      } else {
        const float u[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ch = 0; ch < 3; ch++) tensor_store4<false>(f.d[ch] + (size_t)y * f.dp[ch], x0, u, te, ch, vec, nv);
      }
    }
    return;
  }
  const FrameSrcDesc& fs = args.f[b.f];
#pragma unroll
  for (int ch = 0; ch < 3; ch++) { f.s[ch] = fs.s[ch]; f.sp[ch] = fs.sp[ch]; }
  const uint32_t rx = (uint32_t)b.x, ry = (uint32_t)b.y, rw = (uint32_t)b.w, rh = (uint32_t)b.h;
  // 4. the scale factors: the correctly rounded fp32 quotients the host entry computes
  const float scx = (float)rw / (float)dw, scy = (float)rh / (float)dh;
  // staged or per tap: this tile's own window
  RoiTileWin win = roi_tile_window(rx, rw, rh, scx, scy, xs, xe, Y0, Y1);
  tile_window_uniform(win);
  if (roi_tile_staged(roi_tile_need_of(win, dw, dh), lds_bytes)) {
    roi_strip_tile<SRC, DST>(f, c, W, rx, ry, rw, rh, scx, scy, win, dw, ya, yb, x0, nv, vec, wv, lane, tid, te);
    return;
  }
  // per tap: this wave's rows one after the other
  if (ya > Y1 || !nv) return;
  Tap tx[4];
#pragma unroll
  for (int k = 0; k < 4; k++) tx[k] = make_tap<VPF_INTERP_LINEAR>((x0 + k < dw) ? x0 + k : dw - 1, scx, rw);
  for (uint32_t y = ya; y <= yb; y++) roi_dev_gather4<SRC, DST>(f, c, rx, ry, tx, make_tap<VPF_INTERP_LINEAR>(y, scy, rh), x0, y, te, vec, nv, wv, lane);
}

// ------------------------------------------------------------------------------------------
// Host side.  No rectangle is known here: job_plan (vpf_job_plan.h) gives the ONE dispatch the most a staged tile of this destination size can need
// (roi_dev_lds_bytes, vpf_job_bounds.h), nothing under VPF_TUNE_NV12_RGB_VARIANT = 9 — no strip fits then, every tile samples per tap.
// ------------------------------------------------------------------------------------------
hipError_t launch_convert_resize_rois_dev(hipStream_t st, int src_fc, const Yuv2RgbCoef& c, uint32_t W, uint32_t H, RoiDevArgs& a, uint32_t dw, uint32_t dh,
                                          const TensorEpi& te, bool nhwc) {
  JobShape q;
  job_shape(q, JOB_ROI, true, src_fc, nhwc, te, W, H, dw, dh);
  job_shape_dev(q, a.max_n, a.n_frames);
  const JobPlan p = job_plan(q);
  if (!p.ok) return hipErrorInvalidValue;
  const JobDispatch& d = p.d[0];
  const dim3 grid(d.gx, d.gy, d.n);
  const uint32_t lds_all = job_launch_lds(d, te, a);  // (sets a.e)
  hipError_t e = hipSuccess;
  with_src_dst(src_fc, nhwc, [&](auto S, auto D) { VPF_LAUNCH_T(k_roi_dev, (S, D), grid, lds_all, st, a, c, W, H, dw, dh, p.dmask, d.lds); e = hipGetLastError(); });
  return e;
}

}  // namespace vpf
