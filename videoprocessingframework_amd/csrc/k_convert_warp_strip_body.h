// The body of k_warp_strip / k_warp_strip_nhwc (k_convert_warp.hip), included into both with DST = FC_TENSOR / FC_TENSOR_NHWC in scope: the text
// stands in the kernel itself, so the planar kernel's code object is what it was before the second destination class existed.
// Also the body of k_warp_dev / k_warp_dev_nhwc (k_convert_warp_dev.hip) behind their prologue.  In scope: J (the job: a WarpDesc), args.e, c, W, H, dw,
// dh, dmask, lds_bytes.
  const FrameDesc& f = J.f;
  const TensorEpi te = args.e;
  const bool rep = warp_rep(te);
  const uint32_t tid = threadIdx.x;
  const uint32_t xs = blockIdx.x * kWarpTileW, ys = blockIdx.y * kWarpTileH;  // the grid covers the destination exactly: xs < dw, ys < dh
  const uint32_t xe = (xs + kWarpTileW - 1 < dw - 1) ? xs + kWarpTileW - 1 : dw - 1, ye = (ys + kWarpTileH - 1 < dh - 1) ? ys + kWarpTileH - 1 : dh - 1;
  const uint32_t x0 = xs + (tid % kWarpLanesX) * 4, y = ys + tid / kWarpLanesX;
  const bool mine = x0 < dw && y < dh;
  WarpWin w = warp_window(J.m, xs, xe, ys, ye, rep, W, H);
  w.x_lo = __builtin_amdgcn_readfirstlane(w.x_lo); w.x_hi = __builtin_amdgcn_readfirstlane(w.x_hi);
  w.y_lo = __builtin_amdgcn_readfirstlane(w.y_lo); w.y_hi = __builtin_amdgcn_readfirstlane(w.y_hi);
  const uint32_t nv = dw - x0 < 4 ? dw - x0 : 4;
  bool vec = nv == 4;
#pragma unroll
  for (int ch = 0; ch < (DST == FC_TENSOR_NHWC ? 1 : 3); ch++) vec = vec && ((((uintptr_t)f.d[ch] | f.dp[ch]) & dmask) == 0);
  if (w.empty) {  // (CONSTANT only: a clamped coordinate is always in range)
    if (!mine) return;
    if constexpr (DST == FC_TENSOR_NHWC) {
      float u[3][4];
#pragma unroll
      for (int ch = 0; ch < 3; ch++)
#pragma unroll
        for (int k = 0; k < 4; k++) u[ch][k] = warp_border(te, ch);
      warp_store4<DST>(f, x0, y, u, te, vec, nv);
    } else {
#pragma unroll
      for (int ch = 0; ch < 3; ch++) {
        const float b = warp_border(te, ch), u[4] = {b, b, b, b};
        tensor_store4<false>(f.d[ch] + (size_t)y * f.dp[ch], x0, u, te, ch, vec, nv);
      }
    }
    return;
  }
  const WarpStrip S = warp_strip(w);
  if (S.bytes > lds_bytes) {
    if (mine) warp_gather4<SRC, DST>(J, c, te, W, H, dw, dmask, x0, y);
    return;
  }
  uint8_t* const strip = reinterpret_cast<uint8_t*>(dyn_strip);
  {  // the names VPF_STRIP_FILL_WINDOW takes from its scope
    const uint32_t base_px = S.base_px, R_lo = w.y_lo, R_hi = w.y_hi, c_lo = R_lo >> 1, ng = S.ng, units = ((R_hi >> 1) - c_lo + 1) * ng, rowbytes = S.rowbytes;
    VPF_STRIP_FILL_WINDOW
  }
  __syncthreads();
  if (!mine) return;
  const float wmax = (float)(W - 1), hmax = (float)(H - 1);
  const float xlf = (float)w.x_lo, xhf = (float)w.x_hi, ylf = (float)w.y_lo, yhf = (float)w.y_hi;
  float u[3][4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const WarpXY s = warp_xy(J.m, (x0 + k < dw) ? x0 + k : dw - 1, y, rep, wmax, hmax);
    const bool in = s.sx >= 0.f && s.sx <= wmax && s.sy >= 0.f && s.sy <= hmax;
    // an in-range coordinate lies inside the window, so pulling it to the window leaves it unchanged; every other one reads some pixel of
    // the strip and is replaced by the border.  x1 = min(x0 + 1, x_hi) is min(x0 + 1, W - 1) for an in-range pixel (x_hi = min(floor + 1, W - 1)).
    const float cx = __builtin_amdgcn_fmed3f(s.sx, xlf, xhf), cy = __builtin_amdgcn_fmed3f(s.sy, ylf, yhf);
    const uint32_t xa = (uint32_t)(int)cx, ya = (uint32_t)(int)cy;
    const uint32_t xb = xa + 1 < w.x_hi ? xa + 1 : w.x_hi, yb = ya + 1 < w.y_hi ? ya + 1 : w.y_hi;
    const float fx = cx - (float)xa, fy = cy - (float)ya;
    const uint8_t* const ra = strip + (ya - w.y_lo) * S.rowbytes, * const rb = strip + (yb - w.y_lo) * S.rowbytes;
    const uint32_t oa = 4 * (xa - S.base_px), ob = 4 * (xb - S.base_px);
    const uint32_t q00 = *reinterpret_cast<const uint32_t*>(ra + oa), q01 = *reinterpret_cast<const uint32_t*>(ra + ob);
    const uint32_t q10 = *reinterpret_cast<const uint32_t*>(rb + oa), q11 = *reinterpret_cast<const uint32_t*>(rb + ob);
    const float v[3] = {__builtin_truncf(bilerp(ubyte<0>(q00), ubyte<0>(q01), ubyte<0>(q10), ubyte<0>(q11), fx, fy)),
                        __builtin_truncf(bilerp(ubyte<1>(q00), ubyte<1>(q01), ubyte<1>(q10), ubyte<1>(q11), fx, fy)),
                        __builtin_truncf(bilerp(ubyte<2>(q00), ubyte<2>(q01), ubyte<2>(q10), ubyte<2>(q11), fx, fy))};
#pragma unroll
    for (int ch = 0; ch < 3; ch++) u[ch][k] = in ? v[ch] : warp_border(te, ch);
  }
  if constexpr (DST == FC_TENSOR_NHWC) warp_store4<DST>(f, x0, y, u, te, vec, nv);
  else for (int ch = 0; ch < 3; ch++) tensor_store4<false>(f.d[ch] + (size_t)y * f.dp[ch], x0, u[ch], te, ch, vec, nv);
