// k_convert_letterbox.hip — fused multi-ROI crop + bilinear resize of NV12 / YUV420 (P10 / P12) with PLACEMENT and PADDING into a normalised tensor
// (gfx950): vpf_convert_letterbox_tensor.  The ROI entry (k_convert_roi.hip) with a destination rectangle per job: the rectangle of the frame is
// resized to iw x ih and lands at (ix, iy) of the job's dw x dh planes, every other element of the planes takes the pad value (LetterboxDesc,
// vpf_internal.h).  One dispatch serves many jobs with rectangles, pictures and placements of their own.  Grid z = job.
//   k_lb_strip    the staged form: a workgroup owns (job, 16 rows, 256 columns) of the destination PLANE — not of the picture: a lane's four
//                 pixels start at a multiple of four columns of the plane, so an aligned tensor keeps its 16-B / 8-B stores whatever ix is.
//                 A tile that misses the picture stores the pad and leaves (no load, no strip, no barrier); a tile that meets it clips its
//                 column and row range to the picture, converts the taps' source window once into an LDS strip of four-byte RGB pixels
//                 (strip_fill_window, the fill stage of k_roi_strip) and blends from bytes, choosing per pixel between blend and pad
//   k_lb_gather   per-tap texel_rgb: jobs whose window does not pay or does not fit (large down-scales), VPF_TUNE_NV12_RGB_VARIANT = 9
// Definition (include/vpf_hip.h): inside the picture the byte vpf_convert_resize_tensor_rois defines for rect -> (iw, ih) at (dx - ix, dy - iy) —
// make_tap<LINEAR> on the rectangle with scale (float)w / (float)iw, frame texels at absolute coordinates, bilerp, truncation —, outside pad[c];
// then the tensor epilogue.  Both kernels run exactly the ROI kernels' fp32 operations in their order on the picture: identical bits.  The per-tap
// body is lb_gather4 (k_letterbox_common.h), which k_lb_dev runs as well; the staged tile is typed here and in k_lb_dev.
#include "k_job_launch.h"
#include "k_letterbox_common.h"  // lb_pad, lb_store4, lb_pad_rows, lb_gather4: shared with k_convert_letterbox_dev.hip
#include "vpf_job_bounds.h"  // kRoiBandRows: shared with the launch policy (vpf_job_plan.h) and the CPU property tests

namespace vpf {

// ------------------------------------------------------------------------------------------
// The staged form: k_roi_strip's strip (ABSOLUTE frame pixels [base_px, ..) x rows [y + R_lo, y + R_hi], whole conversion units, the frame's
// right-edge unit through clamped byte loads) for the part of the picture that the tile holds.  Tile, clip and the tile's miss are functions of the
// block indices and the job alone: workgroup-uniform, decided before the barrier.
// ------------------------------------------------------------------------------------------
template <int SRC, int DST>  // DST = FC_TENSOR: three planes per job; FC_TENSOR_NHWC: one interleaved plane
__global__ __launch_bounds__(256) void k_lb_strip(const LetterboxArgs args, const Yuv2RgbCoef c, uint32_t W, uint32_t dw, uint32_t dh, uint32_t dmask,
                                                  uint32_t lds_bytes) {
  constexpr int R = kRoiBandRows;
  const LetterboxDesc& L = args.j[blockIdx.z];
  const RoiDesc& J = L.r;
  const FrameDesc& f = J.f;
  const uint32_t rx = J.x, ry = J.y, rw = J.w, rh = J.h;
  const float scx = J.scx, scy = J.scy;
  const uint32_t ix = L.ix, iy = L.iy, ixe = ix + L.iw - 1, iye = iy + L.ih - 1;  // the picture's first and last column and row on the plane
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63, tid = threadIdx.x;
  const uint32_t Y0 = blockIdx.y * (4 * R), xs = blockIdx.x * 256;  // the grid covers the destination plane exactly: Y0 < dh, xs < dw
  const uint32_t Y1 = (Y0 + 4 * R - 1 < dh - 1) ? Y0 + 4 * R - 1 : dh - 1, xe = (xs + 255 < dw - 1) ? xs + 255 : dw - 1;
  const TensorEpi te = args.e;
  const uint32_t ya = Y0 + wv * R, yb = (ya + R - 1 < Y1) ? ya + R - 1 : Y1;  // the wave's rows of the plane
  const uint32_t x0 = xs + lane * 4;                                           // the lane's columns of the plane: a multiple of four
  const uint32_t nv = dw - x0 < 4 ? dw - x0 : 4;                               // (x0 < dw where it is used)
  bool vec = nv == 4;
#pragma unroll
  for (int ch = 0; ch < (DST == FC_TENSOR_NHWC ? 1 : 3); ch++) vec = vec && ((((uintptr_t)f.d[ch] | f.dp[ch]) & dmask) == 0);
  if (xs > ixe || xe < ix || Y0 > iye || Y1 < iy) {  // the tile misses the picture: pad, nothing converted
    if (ya > Y1 || x0 >= dw) return;
    lb_pad_rows<DST>(f, x0, ya, yb, 1u, 0u, te, vec, nv, wv, lane);
    return;
  }
  // the tile's columns and rows of the PICTURE
  const uint32_t cxs = (xs > ix ? xs : ix) - ix, cxe = (xe < ixe ? xe : ixe) - ix, cys = (Y0 > iy ? Y0 : iy) - iy, cye = (Y1 < iye ? Y1 : iye) - iy;
  const uint32_t first = rx + make_tap<VPF_INTERP_LINEAR>(cxs, scx, rw).i0, last = rx + make_tap<VPF_INTERP_LINEAR>(cxe, scx, rw).i1;  // frame pixels
  const uint32_t base_px = first & ~1u;
  const uint32_t R_lo_rel = __builtin_amdgcn_readfirstlane(make_tap<VPF_INTERP_LINEAR>(cys, scy, rh).i0);
  const uint32_t R_lo = ry + R_lo_rel, R_hi = ry + __builtin_amdgcn_readfirstlane(make_tap<VPF_INTERP_LINEAR>(cye, scy, rh).i1);  // frame rows
  uint8_t* const strip = reinterpret_cast<uint8_t*>(dyn_strip);
  const uint32_t ng = ((last - base_px) >> 3) + 1;
  const uint32_t rowbytes = 32u * ng + 16u;  // whole units + the second tap's dword behind the last pixel (weight 0 there)
  if ((R_hi - R_lo + 1) * rowbytes > lds_bytes) return;  // (never: the launcher sized the strip with this arithmetic, letterbox_strip_need)
  strip_fill_window<SRC>(f, c, W, strip, base_px, R_lo, R_hi, ng, rowbytes, tid);  // (k_fused_common.h: shared with k_roi_strip and k_warp_strip)
  __syncthreads();
  if (ya > Y1) return;
  const uint32_t ra = ya > iy ? ya : iy, rb = yb < iye ? yb : iye;  // the wave's rows inside the picture (none: ra > rb)
  const bool rows_in = ra <= rb;
  const Tap row_taps = band_row_taps(rows_in ? ra - iy : cys, rows_in ? rb - iy : cys, scy, rh);  // every lane of the wave still active here
  if (x0 >= dw) return;
  lb_pad_rows<DST>(f, x0, ya, yb, ra, rb, te, vec, nv, wv, lane);
  if (!rows_in) return;
  // Column taps, as make_col_taps_x gives them for picture column x0 + k - ix; a column outside the picture takes the taps of the tile's nearest
  // picture column — inside the strip — and its blend is dropped for the pad below.
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
// The gather form: k_roi_gather on the plane (four rows x 64 lanes x 4 pixels per workgroup, a wave = one row through lb_gather4,
// k_letterbox_common.h).  A lane whose four columns miss the picture loads nothing; a wave whose row or columns miss it branches over the conversion
// as a whole.
// ------------------------------------------------------------------------------------------
template <int SRC, int DST>  // (FC_TENSOR_NHWC: four waves per SIMD asked for, as k_roi_gather)
__global__ __launch_bounds__(256, (DST == FC_TENSOR_NHWC ? 4 : 1)) void k_lb_gather(const LetterboxArgs args, const Yuv2RgbCoef c, uint32_t dw,
                                                                                    uint32_t dh, uint32_t dmask) {
  const LetterboxDesc& L = args.j[blockIdx.z];
  const RoiDesc& J = L.r;
  const FrameDesc& f = J.f;
  const uint32_t x0 = (blockIdx.x * 64 + (threadIdx.x & 63)) * 4;
  const uint32_t y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x0 >= dw || y >= dh) return;
  const uint32_t ix = L.ix, iy = L.iy, ixe = ix + L.iw - 1, iye = iy + L.ih - 1;
  const bool row_in = y >= iy && y <= iye;
  Tap tx[4];
  bool in[4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const uint32_t x = x0 + k;  // (a column right of the plane is right of the picture: pad, not stored)
    in[k] = x >= ix && x <= ixe;
    tx[k] = make_tap<VPF_INTERP_LINEAR>(x < ix ? 0u : (x > ixe ? ixe - ix : x - ix), J.scx, J.w);
  }
  const uint32_t nv = dw - x0 < 4 ? dw - x0 : 4;
  lb_gather4<SRC, DST>(f, c, J.x, J.y, tx, in, make_tap<VPF_INTERP_LINEAR>(row_in ? y - iy : 0u, J.scy, J.h), row_in && x0 + 3 >= ix && x0 <= ixe, x0, y,
                       args.e, tensor_vec_ok<DST>(f, nv, dmask), nv, __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), threadIdx.x & 63);
}

// ------------------------------------------------------------------------------------------
// Host side: launch_convert_resize_rois with the letterbox family of job_plan (vpf_job_plan.h): the walk is laid on the plane and clipped to the
// picture (letterbox_strip_need, vpf_job_bounds.h), the policy is the ROI kernels'.
// ------------------------------------------------------------------------------------------
hipError_t launch_convert_letterbox(hipStream_t st, int src_fc, const Yuv2RgbCoef& c, uint32_t W, uint32_t n, const LetterboxDesc* jobs, uint32_t dw,
                                    uint32_t dh, const TensorEpi& te, bool nhwc) {
  JobShape q;
  job_shape(q, JOB_LETTERBOX, false, src_fc, nhwc, te, W, 0u, dw, dh);
  job_shape_jobs(q, jobs, n, [](JobGeom& g, const LetterboxDesc& j) { g.x = j.r.x; g.w = j.r.w; g.h = j.r.h; g.scx = j.r.scx; g.scy = j.r.scy; g.ix = j.ix; g.iy = j.iy; g.iw = j.iw; g.ih = j.ih; });
  const JobPlan p = job_plan(q);
  if (!p.ok) return hipErrorInvalidValue;
  LetterboxArgs t[2];
  fill_job_tables(p, jobs, n, te, t);
  hipError_t e = hipSuccess;
  for (int k = 0; k < p.nd && e == hipSuccess; k++) {  // staged first; its error returns before the per-tap launch
    const JobDispatch& d = p.d[k];
    const dim3 grid(d.gx, d.gy, d.n);
    const uint32_t lds_all = job_launch_lds(d, te, t[k]);
    with_src_dst(src_fc, nhwc, [&](auto S, auto D) {
      if (d.form == JF_LB_STRIP) VPF_LAUNCH_T(k_lb_strip, (S, D), grid, lds_all, st, t[k], c, W, dw, dh, p.dmask, d.lds);
      else VPF_LAUNCH_T(k_lb_gather, (S, D), grid, lds_all, st, t[k], c, dw, dh, p.dmask);
      e = hipGetLastError();
    });
  }
  return e;
}

}  // namespace vpf
