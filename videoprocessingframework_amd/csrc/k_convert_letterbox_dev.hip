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
// Both forms run k_convert_letterbox.hip's fp32 operations in its order (strip_fill_window, band_row_taps, band_blend_rows, texel_rgb, bilerp,
// lb_store4, lb_pad_rows): identical bits to vpf_convert_letterbox_tensor on the same rectangles and placements, whichever form either entry picks.
#include "k_bilinear_blend.h"
#include "k_fused_common.h"
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

template <int SRC, int DST>  // DST = FC_TENSOR: three planes per job; FC_TENSOR_NHWC: one interleaved plane
__global__ __launch_bounds__(256) void k_lb_dev(const LetterboxDevArgs args, const Yuv2RgbCoef c, uint32_t W, uint32_t H, uint32_t dw, uint32_t dh,
                                                uint32_t dmask, uint32_t lds_bytes) {
  constexpr int R = kRoiBandRows;
  const uint32_t job = blockIdx.z;
  // 1. the count: jobs at or behind it write nothing and read neither box nor placement
  uint32_t cnt = args.max_n;
  if (args.count) {
    const int32_t v = __builtin_amdgcn_readfirstlane(*args.count);
    cnt = v < 0 ? 0u : ((uint32_t)v < args.max_n ? (uint32_t)v : args.max_n);
  }
  if (job >= cnt) return;
  // 2. the five ints of this job's box, then the four of its placement, wave-uniform
  const int32_t* const bp = reinterpret_cast<const int32_t*>(reinterpret_cast<const uint8_t*>(args.boxes) + (size_t)job * args.box_stride);
  const int32_t b_f = __builtin_amdgcn_readfirstlane(bp[0]), b_x = __builtin_amdgcn_readfirstlane(bp[1]), b_y = __builtin_amdgcn_readfirstlane(bp[2]),
                b_w = __builtin_amdgcn_readfirstlane(bp[3]), b_h = __builtin_amdgcn_readfirstlane(bp[4]);
  int32_t r_x = 0, r_y = 0, r_w = 1, r_h = 1;
  if (args.rects) {
    const int32_t* const rp = reinterpret_cast<const int32_t*>(reinterpret_cast<const uint8_t*>(args.rects) + (size_t)job * args.rect_stride);
    r_x = __builtin_amdgcn_readfirstlane(rp[0]); r_y = __builtin_amdgcn_readfirstlane(rp[1]);
    r_w = __builtin_amdgcn_readfirstlane(rp[2]); r_h = __builtin_amdgcn_readfirstlane(rp[3]);
  }
  // 3. the guards (vpf_job_bounds.h): an invalid job reads no frame; its tile takes the pad
  const bool ok = roi_dev_box_ok(b_f, b_x, b_y, b_w, b_h, args.n_frames, W, H) && letterbox_dev_rect_ok(r_x, r_y, r_w, r_h, dw, dh);
  // 4. the placement: the caller's, or the fit of the box into the plane, once per workgroup on wave-uniform values
  uint32_t ix = (uint32_t)r_x, iy = (uint32_t)r_y, iw = (uint32_t)r_w, ih = (uint32_t)r_h;
  if (ok && !args.rects) {
    const LetterboxFit fit = letterbox_fit_ints((uint32_t)b_w, (uint32_t)b_h, dw, dh);
    ix = __builtin_amdgcn_readfirstlane(fit.ix); iy = __builtin_amdgcn_readfirstlane(fit.iy);
    iw = __builtin_amdgcn_readfirstlane(fit.iw); ih = __builtin_amdgcn_readfirstlane(fit.ih);
  }
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63, tid = threadIdx.x;
  const uint32_t Y0 = blockIdx.y * (4 * R), xs = blockIdx.x * 256;  // the grid covers the destination plane exactly: Y0 < dh, xs < dw
  const uint32_t Y1 = (Y0 + 4 * R - 1 < dh - 1) ? Y0 + 4 * R - 1 : dh - 1, xe = (xs + 255 < dw - 1) ? xs + 255 : dw - 1;
  const TensorEpi te = args.e;
  FrameDesc f;
#pragma unroll
  for (int ch = 0; ch < 3; ch++) {
    f.d[ch] = (DST == FC_TENSOR_NHWC && ch) ? nullptr : args.d[ch] + (size_t)job * args.job_stride;
    f.dp[ch] = args.dp[ch];
  }
  const uint32_t ya = Y0 + wv * R, yb = (ya + R - 1 < Y1) ? ya + R - 1 : Y1;  // this wave's rows of the plane (none when ya > Y1)
  const uint32_t x0 = xs + lane * 4;                                        // this lane's four columns of the plane (none when x0 >= dw)
  const uint32_t nv = x0 < dw ? (dw - x0 < 4 ? dw - x0 : 4) : 0;
  bool vec = nv == 4;
#pragma unroll
  for (int ch = 0; ch < (DST == FC_TENSOR_NHWC ? 1 : 3); ch++) vec = vec && ((((uintptr_t)f.d[ch] | f.dp[ch]) & dmask) == 0);
  const uint32_t ixe = ix + iw - 1, iye = iy + ih - 1;  // the picture's last column and row on the plane
  // 5. an invalid job, or a tile that misses the picture: pad, nothing converted, no barrier
  if (!ok || xs > ixe || xe < ix || Y0 > iye || Y1 < iy) {
    if (ya > Y1 || !nv) return;
    lb_pad_rows<DST>(f, x0, ya, yb, 1u, 0u, te, vec, nv, wv, lane);
    return;
  }
  const FrameSrcDesc& fs = args.f[b_f];
#pragma unroll
  for (int ch = 0; ch < 3; ch++) { f.s[ch] = fs.s[ch]; f.sp[ch] = fs.sp[ch]; }
  const uint32_t rx = (uint32_t)b_x, ry = (uint32_t)b_y, rw = (uint32_t)b_w, rh = (uint32_t)b_h;
  // the scale factors: the correctly rounded fp32 quotients the host entry computes
  const float scx = (float)rw / (float)iw, scy = (float)rh / (float)ih;
  // 6. staged or per tap: this tile's own window, clipped to the picture
  LetterboxTileWin lw = letterbox_tile_window(rx, rw, rh, scx, scy, ix, iy, iw, ih, xs, xe, Y0, Y1);
  RoiTileWin& win = lw.w;
  win.first = __builtin_amdgcn_readfirstlane(win.first); win.last = __builtin_amdgcn_readfirstlane(win.last);
  win.lo = __builtin_amdgcn_readfirstlane(win.lo); win.hi = __builtin_amdgcn_readfirstlane(win.hi);
  win.base_px = win.first & ~1u; win.ng = ((win.last - win.base_px) >> 3) + 1u; win.rowbytes = 32u * win.ng + 16u; win.rows = win.hi - win.lo + 1u;
  const uint32_t cxs = lw.cxs, cxe = lw.cxe, cys = lw.cys;
  if (!roi_tile_staged(letterbox_tile_need_of(win, iw, ih), lds_bytes)) {
    // 7a. per tap: k_lb_gather's pixel, this wave's rows one after the other.  A lane whose four columns miss the picture loads nothing.  What the
    // loop uses in per-lane arithmetic only moves to vector registers (lane_copy): the kernel is short of scalar registers here, not of those.
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
    const float pad[3] = {lb_pad(te, 0), lb_pad(te, 1), lb_pad(te, 2)};
    const uint32_t vrx = lane_copy(rx), vry = lane_copy(ry), viy = lane_copy(iy), vrh = lane_copy(rh);
    const float vscy = __uint_as_float(lane_copy(__float_as_uint(scy)));
    TensorEpi tv = te;
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
      f.sp[ch] = lane_copy(f.sp[ch]); f.dp[ch] = lane_copy(f.dp[ch]);
      tv.scale[ch] = __uint_as_float(lane_copy(__float_as_uint(te.scale[ch])));
      tv.bias[ch] = __uint_as_float(lane_copy(__float_as_uint(te.bias[ch])));
    }
    for (uint32_t y = ya; y <= yb; y++) {
      float u[3][4];
#pragma unroll
      for (int ch = 0; ch < 3; ch++)
#pragma unroll
        for (int k = 0; k < 4; k++) u[ch][k] = pad[ch];
      if (cols_in && y >= ra && y <= rb) {
        const Tap ty = make_tap<VPF_INTERP_LINEAR>(y - viy, vscy, vrh);
#pragma unroll
        for (int k = 0; k < 4; k++) {
          float p00[3], p01[3], p10[3], p11[3];
          texel_rgb<SRC>(f, c, vrx + tx[k].i0, vry + ty.i0, p00);
          texel_rgb<SRC>(f, c, vrx + tx[k].i1, vry + ty.i0, p01);
          texel_rgb<SRC>(f, c, vrx + tx[k].i0, vry + ty.i1, p10);
          texel_rgb<SRC>(f, c, vrx + tx[k].i1, vry + ty.i1, p11);
#pragma unroll
          for (int ch = 0; ch < 3; ch++) {
            const float v = __builtin_truncf(bilerp(p00[ch], p01[ch], p10[ch], p11[ch], tx[k].f, ty.f));
            u[ch][k] = in[k] ? v : u[ch][k];
          }
        }
      }
      lb_store4<DST>(f, x0, y, u, tv, vec, nv, wv, lane);
    }
    return;
  }
  // 7b. the staged form: k_lb_strip from its fill stage on
  const uint32_t base_px = win.base_px, R_lo_rel = win.lo, R_lo = ry + win.lo, R_hi = ry + win.hi;  // frame rows
  // column taps as k_lb_strip has them: a column outside the picture takes the taps of the tile's nearest picture column — inside the strip —
  // and its blend is dropped for the pad below.  Computed BEFORE the fill: they need no strip, and the placement's scalars need not outlive it.
  ColTapsX T;
  bool in[4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const uint32_t x = x0 + k;
    in[k] = x >= ix && x <= ixe;
    const uint32_t px = x < ix + cxs ? cxs : (x > ix + cxe ? cxe : x - ix);
    const Tap t = make_tap<VPF_INTERP_LINEAR>(px, scx, rw);
    T.a[k] = 4u * (t.i0 - (base_px - rx));  // (frame pixel base_px = rectangle pixel base_px - rx, modulo 2^32)
    T.f[k] = t.f;
  }
  uint8_t* const strip = reinterpret_cast<uint8_t*>(dyn_strip);
  const uint32_t rowbytes = win.rowbytes;
  strip_fill_window<SRC>(f, c, W, strip, base_px, R_lo, R_hi, win.ng, rowbytes, tid);  // (k_fused_common.h)
  __syncthreads();
  if (ya > Y1) return;
  const uint32_t ra = ya > iy ? ya : iy, rb = yb < iye ? yb : iye;  // the wave's rows inside the picture (none: ra > rb)
  const bool rows_in = ra <= rb;
  const Tap row_taps = band_row_taps(rows_in ? ra - iy : cys, rows_in ? rb - iy : cys, scy, rh);  // every lane of the wave still active here
  if (!nv) return;
  lb_pad_rows<DST>(f, x0, ya, yb, ra, rb, te, vec, nv, wv, lane);
  if (!rows_in) return;
  const float pad[3] = {lb_pad(te, 0), lb_pad(te, 1), lb_pad(te, 2)};
  band_blend_rows<3, R>(strip, rowbytes, R_lo_rel, ra - iy, rb - iy, row_taps, T, [&](uint32_t y, const float* o) {  // o: pixel-major R G B, + 0.5 added
    float u[3][4];
#pragma unroll
    for (int ch = 0; ch < 3; ch++)
#pragma unroll
      for (int k = 0; k < 4; k++) u[ch][k] = in[k] ? __builtin_truncf(o[3 * k + ch]) : pad[ch];
    lb_store4<DST>(f, x0, y + iy, u, te, vec, nv, wv, lane);
  });
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
