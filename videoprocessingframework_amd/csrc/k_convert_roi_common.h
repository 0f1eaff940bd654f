// k_convert_roi_common.h — the device body the two ROI translation units share (k_convert_roi.hip: the host-table kernels; k_convert_roi_dev.hip: the
// device-table kernel), as k_convert_warp_common.h holds the warps': roi_strip_tile, the staged form of a workgroup's tile from its window on (the
// whole of k_roi_strip behind its job load, the staged branch of k_roi_dev).  One text: a staged tile of the device-table entry gives the bits of
// its host-table twin because both run this function.  Every value comes in as a parameter; forced inline everywhere.  The
// per-tap pixel is typed in both units: shared, k_roi_gather ran 5 % slower.
#ifndef VPF_K_CONVERT_ROI_COMMON_H_
#define VPF_K_CONVERT_ROI_COMMON_H_
#include "k_bilinear_blend.h"
#include "k_fused_common.h"
#include "vpf_job_bounds.h"

namespace vpf {

// ------------------------------------------------------------------------------------------
// The staged form.  convert_strip_wg_task (k_convert_resize.hip) with per-job geometry: the strip's pixels are ABSOLUTE frame pixels
// [base_px, ..) x rows [ry + lo, ry + hi], base_px = the even pixel at or below the first tap (a conversion unit = 8 pixels x 2 luma
// rows under ONE chroma row, so units start on chroma pairs of the frame, whatever the parity of the rectangle's corner); the blend
// addresses them through rectangle-relative taps.  A unit that would read past the frame's right edge takes byte loads clamped to the
// row's last sample instead of the 8-byte ones (its surplus pixels are converted and never blended): no byte outside the frame's own
// rows is read.  Rows need no clamp: every row of the window lies in the rectangle, every chroma row under it in the frame.
// f: the job's planes; (rx, ry, rw, rh), scx, scy: its rectangle and scale factors; win: the tile's window (roi_tile_window, tile_window_uniform),
// whose strip fits the dynamic LDS; ya .. yb: the wave's destination rows (none: ya > yb); x0, nv: the lane's columns (none: nv = 0).  Every lane
// of the workgroup calls this (one barrier inside).
// ------------------------------------------------------------------------------------------
template <int SRC, int DST>
VPF_DEV void roi_strip_tile(const FrameDesc& f, const Yuv2RgbCoef& c, uint32_t W, uint32_t rx, uint32_t ry, uint32_t rw, uint32_t rh, float scx, float scy,
                            const RoiTileWin& win, uint32_t dw, uint32_t ya, uint32_t yb, uint32_t x0, uint32_t nv, bool vec, uint32_t wv, uint32_t lane,
                            uint32_t tid, const TensorEpi& te) {
  uint8_t* const strip = reinterpret_cast<uint8_t*>(dyn_strip);
  strip_fill_window<SRC>(f, c, W, strip, win.base_px, ry + win.lo, ry + win.hi, win.ng, win.rowbytes, tid);  // (k_fused_common.h: shared with the warps)
  __syncthreads();
  if (ya > yb) return;
  const Tap row_taps = band_row_taps(ya, yb, scy, rh);  // every lane of the wave still active here
  if (!nv) return;
  const ColTapsX T = make_col_taps_x(win.base_px - rx, x0, dw, rw, scx);  // tap offsets from the strip's first pixel (frame pixel base_px = rectangle pixel base_px - rx, modulo 2^32)
  band_blend_rows<3, kRoiBandRows>(strip, win.rowbytes, win.lo, ya, yb, row_taps, T, [&](uint32_t y, const float* o) {  // o: pixel-major R G B, + 0.5 added
    if constexpr (DST == FC_TENSOR_NHWC) {
      tensor_store4_nhwc_trunc<false>(f.d[0] + (size_t)y * f.dp[0], x0, o, 1, 3, te, vec, nv, wv, lane);
    } else {
#pragma unroll
      for (int ch = 0; ch < 3; ch++) tensor_store4_trunc<false>(f.d[ch] + (size_t)y * f.dp[ch], x0, o + ch, 3, te, ch, vec, nv);
    }
  });
}

}  // namespace vpf
#endif  // VPF_K_CONVERT_ROI_COMMON_H_
