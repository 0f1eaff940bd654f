// k_convert_letterbox_aa.hip — the ANTIALIASED letterbox of NV12 / YUV420 (P10 / P12) into a normalised tensor (gfx950):
// vpf_convert_letterbox_tensor_aa.  The job table, the plane rules, the pad and the epilogue of k_convert_letterbox.hip; inside the picture the bare
// bilinear pair is replaced by the triangle filter of PIL and of torch's antialias=True, whose support grows with the scale: at 6 x a picture pixel
// is a fold over 12 x 12 source pixels instead of 2 x 2 out of 36.  One dispatch serves many jobs.  Grid z = job.
//   k_lbaa_strip   the staged form: a workgroup owns a tile of the destination PLANE (64 x 16 or 32 x 8, aa_plan picks per dispatch).  A tile that
//                  misses the picture stores the pad and leaves (no load, no strip, no barrier); a tile that meets it converts the exact source
//                  window of its picture pixels ONCE into an LDS strip of four-byte RGB pixels (strip_fill_window, the fill stage of k_lb_strip)
//                  and, after one barrier, evaluates every pixel's folds from LDS: a tap is one ds_read_b32 and three byte conversions instead
//                  of three global loads and the YUV -> RGB chain
//   k_lbaa_gather  per tap through texel_rgb: jobs whose window fits under no tile shape (beyond about 6.8 x), VPF_TUNE_NV12_RGB_VARIANT = 9
// Definition (include/vpf_hip.h, csrc/vpf_aa_plan.h): aa_pixel — rows outer, columns inner, horizontal fold, normalise, vertical fold, normalise,
// round half up — on the bytes vpf_convert gives the frame's pixels.  Both kernels run aa_pixel itself, on the same bytes: identical bits.  Weights
// are recomputed per tap from the centre (a handful of VALU operations); nothing per tap is kept in a per-lane array.
#include "k_bilinear_blend.h"
#include "k_fused_common.h"
#include "k_job_launch.h"
#include "k_letterbox_common.h"  // lb_fill_pad, lb_store4
#include "vpf_aa_plan.h"

namespace vpf {

// u[ch][k] = v[ch] for a k the compiler does not know: twelve selects, no indexed array
VPF_DEV void lbaa_put(float (&u)[3][4], uint32_t k, const float (&v)[3]) {
#pragma unroll
  for (int kk = 0; kk < 4; kk++)
#pragma unroll
    for (int ch = 0; ch < 3; ch++) u[ch][kk] = (uint32_t)kk == k ? v[ch] : u[ch][kk];
}

// ------------------------------------------------------------------------------------------
// The staged form.  Tile, clip and the tile's miss are functions of the block indices and the job alone: workgroup-uniform, decided before the
// barrier.  The strip holds ABSOLUTE frame pixels [base_px, base_px + 8 ng) x rows [R_lo, R_hi]: the windows of the tile's first and last picture
// column and row (lo and hi do not decrease with the pixel).  A lane's pixels are consecutive in a row, so the four-pixel shape keeps the 16-B / 8-B
// stores of an aligned tensor; a wave's lanes span several rows of the tile, so channels-last rows are stored per lane (kNoStage).
// ------------------------------------------------------------------------------------------
template <int SRC, int DST>
__global__ __launch_bounds__(256) void k_lbaa_strip(const LetterboxArgs args, const Yuv2RgbCoef c, uint32_t W, uint32_t dw, uint32_t dh, uint32_t dmask,
                                                    uint32_t lds_bytes, uint32_t tile) {
  const LetterboxDesc& L = args.j[blockIdx.z];
  const RoiDesc& J = L.r;
  const FrameDesc& f = J.f;
  const TensorEpi te = args.e;
  const uint32_t ix = L.ix, iy = L.iy, ixe = ix + L.iw - 1, iye = iy + L.ih - 1;  // the picture's first and last column and row on the plane
  const uint32_t tw = aa_tile_w(tile), th = aa_tile_h(tile), npx = aa_tile_npx(tile), lpr = tw / npx;  // lanes per row of the tile: 16 or 32
  const uint32_t tid = threadIdx.x;
  const uint32_t xs = blockIdx.x * tw, Y0 = blockIdx.y * th;  // the grid covers the plane exactly: xs < dw, Y0 < dh
  const uint32_t xe = (xs + tw - 1 < dw - 1) ? xs + tw - 1 : dw - 1, Y1 = (Y0 + th - 1 < dh - 1) ? Y0 + th - 1 : dh - 1;
  const uint32_t x0 = xs + (tid & (lpr - 1)) * npx, y = Y0 + tid / lpr;
  const bool live = x0 <= xe && y <= Y1;
  const uint32_t nv = live ? (xe - x0 + 1 < npx ? xe - x0 + 1 : npx) : 0u;
  const bool vec = tensor_vec_ok<DST>(f, nv, dmask);
  float u[3][4];
  lb_fill_pad(u, te);
  if (xs > ixe || xe < ix || Y0 > iye || Y1 < iy) {  // the tile misses the picture: pad, nothing converted
    if (live) lb_store4<DST>(f, x0, y, u, te, vec, nv, kNoStage, tid & 63);
    return;
  }
  const AaAxis ax = aa_axis_s(J.w, J.scx), ay = aa_axis_s(J.h, J.scy);
  // the tile's columns and rows of the PICTURE, and their source window
  const uint32_t cxs = (xs > ix ? xs : ix) - ix, cxe = (xe < ixe ? xe : ixe) - ix, cys = (Y0 > iy ? Y0 : iy) - iy, cye = (Y1 < iye ? Y1 : iye) - iy;
  const uint32_t first = J.x + aa_window(ax, cxs).lo, last = J.x + aa_window(ax, cxe).hi - 1;  // frame pixels
  const uint32_t base_px = first & ~1u;
  const uint32_t R_lo = J.y + aa_window(ay, cys).lo, R_hi = J.y + aa_window(ay, cye).hi - 1;   // frame rows
  uint8_t* const strip = reinterpret_cast<uint8_t*>(dyn_strip);
  const uint32_t ng = ((last - base_px) >> 3) + 1;
  const uint32_t rowbytes = 32u * ng;
  if ((R_hi - R_lo + 1) * rowbytes > lds_bytes) return;  // (never: the plan sized the strip with a bound of this arithmetic, aa_job_bytes)
  strip_fill_window<SRC>(f, c, W, strip, base_px, R_lo, R_hi, ng, rowbytes, tid);  // (k_fused_common.h: shared with k_roi_strip, k_lb_strip, k_warp_strip)
  __syncthreads();
  if (!live) return;
  if (y >= iy && y <= iye) {
    // strip byte of rectangle pixel (0, 0): a signed offset, the window starts at or right of it
    const int32_t org = (int32_t)(J.y - R_lo) * (int32_t)rowbytes + 4 * (int32_t)(J.x - base_px);
#pragma nounroll
    for (uint32_t k = 0; k < nv; k++) {
      const uint32_t x = x0 + k;
      if (x < ix || x > ixe) continue;
      float v[3];
      aa_pixel(ax, ay, x - ix, y - iy, [&](uint32_t i, uint32_t j, float* p) {
        const uint32_t d = *reinterpret_cast<const uint32_t*>(strip + (org + (int32_t)(j * rowbytes + 4u * i)));
        p[0] = ubyte<0>(d); p[1] = ubyte<1>(d); p[2] = ubyte<2>(d);
      }, v);
      lbaa_put(u, k, v);
    }
  }
  lb_store4<DST>(f, x0, y, u, te, vec, nv, kNoStage, tid & 63);
}

// ------------------------------------------------------------------------------------------
// The per-tap form: k_lb_gather's shape (four rows x 64 lanes x 4 pixels per workgroup, a wave = one row).  A lane whose four columns miss the
// picture loads nothing.
// ------------------------------------------------------------------------------------------
template <int SRC, int DST>
__global__ __launch_bounds__(256) void k_lbaa_gather(const LetterboxArgs args, const Yuv2RgbCoef c, uint32_t dw, uint32_t dh, uint32_t dmask) {
  const LetterboxDesc& L = args.j[blockIdx.z];
  const RoiDesc& J = L.r;
  const FrameDesc& f = J.f;
  const uint32_t x0 = (blockIdx.x * 64 + (threadIdx.x & 63)) * 4;
  const uint32_t y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x0 >= dw || y >= dh) return;
  const uint32_t ix = L.ix, iy = L.iy, ixe = ix + L.iw - 1, iye = iy + L.ih - 1;
  const uint32_t nv = dw - x0 < 4 ? dw - x0 : 4;
  float u[3][4];
  lb_fill_pad(u, args.e);
  if (y >= iy && y <= iye && x0 + 3 >= ix && x0 <= ixe) {  // the lane holds picture
    const AaAxis ax = aa_axis_s(J.w, J.scx), ay = aa_axis_s(J.h, J.scy);
#pragma nounroll
    for (uint32_t k = 0; k < nv; k++) {
      const uint32_t x = x0 + k;
      if (x < ix || x > ixe) continue;
      float v[3];
      aa_pixel(ax, ay, x - ix, y - iy, [&](uint32_t i, uint32_t j, float* p) { texel_rgb<SRC>(f, c, J.x + i, J.y + j, p); }, v);
      lbaa_put(u, k, v);
    }
  }
  lb_store4<DST>(f, x0, y, u, args.e, tensor_vec_ok<DST>(f, nv, dmask), nv, kNoStage, threadIdx.x & 63);
}

// ------------------------------------------------------------------------------------------
// Host side: aa_plan (vpf_aa_plan.h) decides, this dispatches: the staged jobs first, its error returns before the per-tap launch.
// ------------------------------------------------------------------------------------------
hipError_t launch_convert_letterbox_aa(hipStream_t st, int src_fc, const Yuv2RgbCoef& c, uint32_t W, uint32_t n, const LetterboxDesc* jobs, uint32_t dw,
                                       uint32_t dh, const TensorEpi& te, bool nhwc) {
  AaShape q;
  q.src_fc = src_fc; q.nhwc = nhwc; q.dtype = te.dtype; q.dw = dw; q.dh = dh; q.n = n;
  q.variant = tuning(VPF_TUNE_NV12_RGB_VARIANT);
  for (uint32_t i = 0; i < n && i < (uint32_t)kLetterboxBatch; i++) q.g[i] = AaGeom{jobs[i].r.w, jobs[i].r.h, jobs[i].iw, jobs[i].ih};
  const AaPlan p = aa_plan(q);
  if (!p.ok) return hipErrorInvalidValue;
  LetterboxArgs t[2];
  std::memset(t, 0, sizeof(t));
  t[0].e = t[1].e = te;
  uint32_t cnt[2] = {0u, 0u};
  for (uint32_t i = 0; i < n; i++) t[p.which[i]].j[cnt[p.which[i]]++] = jobs[i];
  hipError_t e = hipSuccess;
  for (int k = 0; k < p.nd && e == hipSuccess; k++) {
    const AaDispatch& d = p.d[k];
    const dim3 grid(d.gx, d.gy, d.n);
    with_src_dst(src_fc, nhwc, [&](auto S, auto D) {
      if (d.form == AA_STRIP) VPF_LAUNCH_T(k_lbaa_strip, (S, D), grid, d.lds, st, t[k], c, W, dw, dh, p.dmask, d.lds, d.tile);
      else VPF_LAUNCH_T(k_lbaa_gather, (S, D), grid, 0, st, t[k], c, dw, dh, p.dmask);
      e = hipGetLastError();
    });
  }
  return e;
}

}  // namespace vpf
