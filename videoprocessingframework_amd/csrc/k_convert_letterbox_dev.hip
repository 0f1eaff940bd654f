// k_convert_letterbox_dev.hip — the letterbox of k_convert_letterbox.hip with the boxes in DEVICE memory (gfx950): vpf_convert_letterbox_tensor_dev.
// A detector and its NMS leave their boxes on the GPU; a second-stage network (ReID, face, OCR) wants them as aspect-preserving padded crops.  This
// kernel reads (frame, x, y, w, h) of job blockIdx.z, the optional placement (ix, iy, iw, ih) and the job count WHEN IT RUNS: no sync, no copy to
// the host, and a captured graph replays with the tables of replay time.
//   k_lb_dev       ONE dispatch over (tiles of 16 rows x 256 columns of the destination PLANE, max_n jobs).  A workgroup loads the count (jobs at or
//                  behind it write nothing), its box and its placement, runs the guards (roi_dev_box_ok, letterbox_dev_rect_ok: an invalid job
//                  reads no frame and writes the pad's epilogue), computes the fit where no placement was given (letterbox_fit_ints: the integers of
//                  vpf_letterbox_fit) and the scale factors — correctly rounded fp32 quotients: no fast-math, no contraction in this translation
//                  unit —, pads and leaves when its tile misses the picture, and otherwise decides for ITS TILE (letterbox_tile_window,
//                  vpf_job_bounds.h): k_lb_strip's staged form where the tile's strip fits the dispatch's LDS and converts at most kRoiConvMax
//                  source pixels per picture pixel, k_lb_gather's per-tap pixel otherwise.  Every branch before the barrier is workgroup-uniform.
// The per-tap form is the function k_lb_gather runs (lb_gather4, k_letterbox_common.h); the staged form runs k_lb_strip's fp32 operations in its
// order: identical bits to vpf_convert_letterbox_tensor on the same rectangles and placements, whichever form either entry picks.
#include "k_dev_table.h"
#include "k_job_launch.h"
#include "k_letterbox_common.h"
#include "vpf_job_bounds.h"  // roi_dev_box_ok, letterbox_dev_rect_ok, letterbox_fit_ints, letterbox_tile_window, roi_tile_staged: shared with the CPU tests

namespace vpf {

// a wave-uniform value held per lane: the per-tap loop's scalar registers are short, its vector registers are not
VPF_DEV uint32_t lane_copy(uint32_t s) {
  uint32_t v;
  asm("v_mov_b32 %0, %1" : "=v"(v) : "s"(s));
  return v;
}

// The staged form of a tile that meets the picture: k_lb_strip from its fill stage on — its strip, its clipped column taps, its row taps, its pad rows
// and its choice between blend and pad, in its order.  f: the job's planes; (rx, ry, rw, rh), scx, scy: its rectangle and scale factors; ix, iy, ixe,
// iye: the picture on the plane; lw: the tile's window; ya .. yb: the wave's rows (none: ya > yb); x0, nv: the lane's columns (none: nv = 0).  Every
// lane of the workgroup calls this (one barrier inside).  A function of this unit and not one shared with k_lb_strip: called from there, that
// kernel ran up to 6 % slower.
template <int SRC, int DST>
VPF_DEV void lb_dev_strip_tile(const FrameDesc& f, const Yuv2RgbCoef& c, uint32_t W, uint32_t rx, uint32_t ry, uint32_t rw, uint32_t rh, float scx, float scy,
                           uint32_t ix, uint32_t iy, uint32_t ixe, uint32_t iye, const LetterboxTileWin& lw, uint32_t ya, uint32_t yb, uint32_t x0,
                           uint32_t nv, bool vec, uint32_t wv, uint32_t lane, uint32_t tid, const TensorEpi& te) {
  const RoiTileWin& win = lw.w;
  // Column taps, as make_col_taps_x gives them for picture column x0 + k - ix; a column outside the picture takes the taps of the tile's nearest
  // picture column — inside the strip — and its blend is dropped for the pad below.  Computed BEFORE the fill: they need no strip, and the
  // placement's scalars need not outlive it.
  ColTapsX T;
  bool in[4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const uint32_t x = x0 + k;
    in[k] = x >= ix && x <= ixe;
    const uint32_t px = x < ix + lw.cxs ? lw.cxs : (x > ix + lw.cxe ? lw.cxe : x - ix);
    const Tap t = make_tap<VPF_INTERP_LINEAR>(px, scx, rw);
    T.a[k] = 4u * (t.i0 - (win.base_px - rx));  // (frame pixel base_px = rectangle pixel base_px - rx, modulo 2^32)
    T.f[k] = t.f;
  }
  uint8_t* const strip = reinterpret_cast<uint8_t*>(dyn_strip);
  strip_fill_window<SRC>(f, c, W, strip, win.base_px, ry + win.lo, ry + win.hi, win.ng, win.rowbytes, tid);  // (k_fused_common.h)
  __syncthreads();
  if (ya > yb) return;
  const uint32_t ra = ya > iy ? ya : iy, rb = yb < iye ? yb : iye;  // the wave's rows inside the picture (none: ra > rb)
  const bool rows_in = ra <= rb;
  const Tap row_taps = band_row_taps(rows_in ? ra - iy : lw.cys, rows_in ? rb - iy : lw.cys, scy, rh);  // every lane of the wave still active here
  if (!nv) return;
  lb_pad_rows<DST>(f, x0, ya, yb, ra, rb, te, vec, nv, wv, lane);
  if (!rows_in) return;
  const float pad[3] = {lb_pad(te, 0), lb_pad(te, 1), lb_pad(te, 2)};
  band_blend_rows<3, kRoiBandRows>(strip, win.rowbytes, win.lo, ra - iy, rb - iy, row_taps, T, [&](uint32_t y, const float* o) {  // o: pixel-major R G B, + 0.5 added
    float u[3][4];
#pragma unroll
    for (int ch = 0; ch < 3; ch++)
#pragma unroll
      for (int k = 0; k < 4; k++) u[ch][k] = in[k] ? __builtin_truncf(o[3 * k + ch]) : pad[ch];
    lb_store4<DST>(f, x0, y + iy, u, te, vec, nv, wv, lane);
  });
}

template <int SRC, int DST>  // DST = FC_TENSOR: three planes per job; FC_TENSOR_NHWC: one interleaved plane
__global__ __launch_bounds__(256) void k_lb_dev(const LetterboxDevArgs args, const Yuv2RgbCoef c, uint32_t W, uint32_t H, uint32_t dw, uint32_t dh,
                                                uint32_t dmask, uint32_t lds_bytes) {
  constexpr int R = kRoiBandRows;
  const uint32_t job = blockIdx.z;
  // 1. the count: jobs at or behind it write nothing and read neither box nor placement
  if (job >= dev_job_count(args.count, args.max_n)) return;
  // 2. the five ints of this job's box, then the four of its placement, wave-uniform
  const DevBox5 b = dev_box5(args.boxes, args.box_stride, job);
  int32_t r_x = 0, r_y = 0, r_w = 1, r_h = 1;
  if (args.rects) {
    const int32_t* const rp = reinterpret_cast<const int32_t*>(reinterpret_cast<const uint8_t*>(args.rects) + (size_t)job * args.rect_stride);
    r_x = __builtin_amdgcn_readfirstlane(rp[0]); r_y = __builtin_amdgcn_readfirstlane(rp[1]);
    r_w = __builtin_amdgcn_readfirstlane(rp[2]); r_h = __builtin_amdgcn_readfirstlane(rp[3]);
  }
  // 3. the guards (vpf_job_bounds.h): an invalid job reads no frame; its tile takes the pad
  const bool ok = roi_dev_box_ok(b.f, b.x, b.y, b.w, b.h, args.n_frames, W, H) && letterbox_dev_rect_ok(r_x, r_y, r_w, r_h, dw, dh);
  // 4. the placement: the caller's, or the fit of the box into the plane, once per workgroup on wave-uniform values
  uint32_t ix = (uint32_t)r_x, iy = (uint32_t)r_y, iw = (uint32_t)r_w, ih = (uint32_t)r_h;
  if (ok && !args.rects) {
    const LetterboxFit fit = letterbox_fit_ints((uint32_t)b.w, (uint32_t)b.h, dw, dh);
    ix = __builtin_amdgcn_readfirstlane(fit.ix); iy = __builtin_amdgcn_readfirstlane(fit.iy);
    iw = __builtin_amdgcn_readfirstlane(fit.iw); ih = __builtin_amdgcn_readfirstlane(fit.ih);
  }
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63, tid = threadIdx.x;
  const uint32_t Y0 = blockIdx.y * (4 * R), xs = blockIdx.x * 256;  // the grid covers the destination plane exactly: Y0 < dh, xs < dw
  const uint32_t Y1 = (Y0 + 4 * R - 1 < dh - 1) ? Y0 + 4 * R - 1 : dh - 1, xe = (xs + 255 < dw - 1) ? xs + 255 : dw - 1;
  const TensorEpi te = args.e;
  FrameDesc f;
  dev_dst_planes<DST>(args, job, f);
  const uint32_t ya = Y0 + wv * R, yb = (ya + R - 1 < Y1) ? ya + R - 1 : Y1;  // this wave's rows of the plane (none when ya > Y1)
  const uint32_t x0 = xs + lane * 4;                                        // this lane's four columns of the plane (none when x0 >= dw)
  const uint32_t nv = x0 < dw ? (dw - x0 < 4 ? dw - x0 : 4) : 0;
  const bool vec = tensor_vec_ok<DST>(f, nv, dmask);
  const uint32_t ixe = ix + iw - 1, iye = iy + ih - 1;  // the picture's last column and row on the plane
  // 5. an invalid job, or a tile that misses the picture: pad, nothing converted, no barrier
  if (!ok || xs > ixe || xe < ix || Y0 > iye || Y1 < iy) {
    if (ya > Y1 || !nv) return;
    lb_pad_rows<DST>(f, x0, ya, yb, 1u, 0u, te, vec, nv, wv, lane);
    return;
  }
  const FrameSrcDesc& fs = args.f[b.f];
#pragma unroll
  for (int ch = 0; ch < 3; ch++) { f.s[ch] = fs.s[ch]; f.sp[ch] = fs.sp[ch]; }
  const uint32_t rx = (uint32_t)b.x, ry = (uint32_t)b.y, rw = (uint32_t)b.w, rh = (uint32_t)b.h;
  // the scale factors: the correctly rounded fp32 quotients the host entry computes
  const float scx = (float)rw / (float)iw, scy = (float)rh / (float)ih;
  // 6. staged or per tap: this tile's own window, clipped to the picture
  LetterboxTileWin lw = letterbox_tile_window(rx, rw, rh, scx, scy, ix, iy, iw, ih, xs, xe, Y0, Y1);
  RoiTileWin& win = lw.w;
  tile_window_uniform(win);
  if (!roi_tile_staged(letterbox_tile_need_of(win, iw, ih), lds_bytes)) {
    // 7a. per tap: this wave's rows one after the other through lb_gather4 (a row outside the picture: its tap is not used).  What the loop uses
    // in per-lane arithmetic only moves to vector registers (lane_copy): the kernel is short of scalar registers here, not of those.
    if (ya > Y1 || !nv) return;
    const uint32_t ra = ya > iy ? ya : iy, rb = yb < iye ? yb : iye;  // the wave's rows inside the picture (none: ra > rb)
    const bool cols_in = x0 + 3 >= ix && x0 <= ixe;
    Tap tx[4];
    bool in[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const uint32_t x = x0 + k;  // (a column right of the plane is right of the picture: pad, not stored)
      in[k] = x >= ix && x <= ixe;
      tx[k] = make_tap<VPF_INTERP_LINEAR>(x < ix ? 0u : (x > ixe ? ixe - ix : x - ix), scx, rw);
    }
    const uint32_t vrx = lane_copy(rx), vry = lane_copy(ry), viy = lane_copy(iy), vrh = lane_copy(rh);
    const float vscy = __uint_as_float(lane_copy(__float_as_uint(scy)));
    TensorEpi tv = te;
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
      f.sp[ch] = lane_copy(f.sp[ch]); f.dp[ch] = lane_copy(f.dp[ch]);
      tv.scale[ch] = __uint_as_float(lane_copy(__float_as_uint(te.scale[ch])));
      tv.bias[ch] = __uint_as_float(lane_copy(__float_as_uint(te.bias[ch])));
    }
    for (uint32_t y = ya; y <= yb; y++)
      lb_gather4<SRC, DST>(f, c, vrx, vry, tx, in, make_tap<VPF_INTERP_LINEAR>(y - viy, vscy, vrh), cols_in && y >= ra && y <= rb, x0, y, tv, vec, nv, wv, lane);
    return;
  }
  // 7b. the staged form
  lb_dev_strip_tile<SRC, DST>(f, c, W, rx, ry, rw, rh, scx, scy, ix, iy, ixe, iye, lw, ya, yb, x0, nv, vec, wv, lane, tid, te);
}

// ------------------------------------------------------------------------------------------
// Host side.  Neither box nor placement is known here: job_plan (vpf_job_plan.h) gives the ONE dispatch the ROI device form's LDS (roi_dev_lds_bytes
// stays a bound for a picture inside the plane: letterbox_tile_need_of, vpf_job_bounds.h), nothing under VPF_TUNE_NV12_RGB_VARIANT = 9.
// ------------------------------------------------------------------------------------------
hipError_t launch_convert_letterbox_dev(hipStream_t st, int src_fc, const Yuv2RgbCoef& c, uint32_t W, uint32_t H, LetterboxDevArgs& a, uint32_t dw, uint32_t dh,
                                        const TensorEpi& te, bool nhwc) {
  JobShape q;
  job_shape(q, JOB_LETTERBOX, true, src_fc, nhwc, te, W, H, dw, dh);
  job_shape_dev(q, a.max_n, a.n_frames);
  const JobPlan p = job_plan(q);
  if (!p.ok) return hipErrorInvalidValue;
  const JobDispatch& d = p.d[0];
  const dim3 grid(d.gx, d.gy, d.n);
  const uint32_t lds_all = job_launch_lds(d, te, a);  // (sets a.e)
  hipError_t e = hipSuccess;
  with_src_dst(src_fc, nhwc, [&](auto S, auto D) { VPF_LAUNCH_T(k_lb_dev, (S, D), grid, lds_all, st, a, c, W, H, dw, dh, p.dmask, d.lds); e = hipGetLastError(); });
  return e;
}

}  // namespace vpf
