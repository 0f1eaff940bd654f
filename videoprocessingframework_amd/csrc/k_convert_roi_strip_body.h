// The body of k_roi_strip / k_roi_strip_nhwc (k_convert_roi.hip), included into both with DST = FC_TENSOR / FC_TENSOR_NHWC in scope: the text stands in
// the kernel itself, so the planar kernel's code object is what it was before the second destination class existed.
  constexpr int R = kRoiBandRows;
  const RoiDesc& J = args.j[blockIdx.z];
  const FrameDesc& f = J.f;
  const uint32_t rx = J.x, ry = J.y, rw = J.w, rh = J.h;
  const float scx = J.scx, scy = J.scy;
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63, tid = threadIdx.x;
  const uint32_t Y0 = blockIdx.y * (4 * R), xs = blockIdx.x * 256;  // the grid covers the destination exactly: Y0 < dh, xs < dw
  const uint32_t Y1 = (Y0 + 4 * R - 1 < dh - 1) ? Y0 + 4 * R - 1 : dh - 1, xe = (xs + 255 < dw - 1) ? xs + 255 : dw - 1;
  const uint32_t first = rx + make_tap<VPF_INTERP_LINEAR>(xs, scx, rw).i0, last = rx + make_tap<VPF_INTERP_LINEAR>(xe, scx, rw).i1;  // frame pixels
  const uint32_t base_px = first & ~1u;
  const uint32_t R_lo_rel = __builtin_amdgcn_readfirstlane(make_tap<VPF_INTERP_LINEAR>(Y0, scy, rh).i0);
  const uint32_t R_lo = ry + R_lo_rel, R_hi = ry + __builtin_amdgcn_readfirstlane(make_tap<VPF_INTERP_LINEAR>(Y1, scy, rh).i1);  // frame rows
  uint8_t* const strip = reinterpret_cast<uint8_t*>(dyn_strip);
  const uint32_t c_lo = R_lo >> 1, ncr = (R_hi >> 1) - c_lo + 1, ng = ((last - base_px) >> 3) + 1, units = ncr * ng;
  const uint32_t rowbytes = 32u * ng + 16u;  // whole units + the second tap's dword behind the last pixel (weight 0 there)
  if ((R_hi - R_lo + 1) * rowbytes > lds_bytes) return;  // (never: the launcher sized the strip with this arithmetic, launch_convert_resize_rois)
  VPF_STRIP_FILL_WINDOW  // (k_fused_common.h: shared with k_warp_strip)
  __syncthreads();
  const uint32_t ya = Y0 + wv * R;
  if (ya > Y1) return;
  const uint32_t yb = (ya + R - 1 < Y1) ? ya + R - 1 : Y1;
  const Tap row_taps = band_row_taps(ya, yb, scy, rh);  // every lane of the wave still active here
  const uint32_t x0 = xs + lane * 4;
  if (x0 >= dw) return;
  const uint32_t nv = dw - x0 < 4 ? dw - x0 : 4;
  bool vec = nv == 4;
#pragma unroll
  for (int ch = 0; ch < (DST == FC_TENSOR_NHWC ? 1 : 3); ch++) vec = vec && ((((uintptr_t)f.d[ch] | f.dp[ch]) & dmask) == 0);
  const ColTapsX T = make_col_taps_x(base_px - rx, x0, dw, rw, scx);  // tap offsets from the strip's first pixel (frame pixel base_px = rectangle pixel base_px - x, modulo 2^32)
  const TensorEpi te = args.e;
  band_blend_rows<3, R>(strip, rowbytes, R_lo_rel, ya, yb, row_taps, T, [&](uint32_t y, const float* o) {  // o: pixel-major R G B, + 0.5 added
    if constexpr (DST == FC_TENSOR_NHWC) {
      tensor_store4_nhwc_trunc<false>(f.d[0] + (size_t)y * f.dp[0], x0, o, 1, 3, te, vec, nv, wv, lane);
    } else {
#pragma unroll
      for (int ch = 0; ch < 3; ch++) tensor_store4_trunc<false>(f.d[ch] + (size_t)y * f.dp[ch], x0, o + ch, 3, te, ch, vec, nv);
    }
  });
