// The body of k_persp_strip / k_persp_strip_nhwc (k_convert_persp.hip), included into both with DST = FC_TENSOR / FC_TENSOR_NHWC in scope, as
// k_convert_warp_strip_body.h is into the affine kernels.  In scope: J (the job: a PerspDesc), args.e, c, W, H, dw, dh, dmask, lds_bytes.
// What differs from the affine body: the tile's class (persp_window: border, per tap, nothing staged, staged), and the per-pixel test of an in-range
// pixel's taps against the window the tile staged (persp_px_in_window) — the affine body's "an in-range coordinate lies inside the window" does not
// hold for a rounded quotient, so a pixel that fails the test is sampled per tap instead of being pulled into the window.
  const FrameDesc& f = J.f;
  const TensorEpi te = args.e;
  const bool rep = warp_rep(te);
  const uint32_t tid = threadIdx.x;
  const uint32_t xs = blockIdx.x * kWarpTileW, ys = blockIdx.y * kWarpTileH;  // the grid covers the destination exactly: xs < dw, ys < dh
  const uint32_t xe = (xs + kWarpTileW - 1 < dw - 1) ? xs + kWarpTileW - 1 : dw - 1, ye = (ys + kWarpTileH - 1 < dh - 1) ? ys + kWarpTileH - 1 : dh - 1;
  const uint32_t x0 = xs + (tid % kWarpLanesX) * 4, y = ys + tid / kWarpLanesX;
  const bool mine = x0 < dw && y < dh;
  PerspWin pw = persp_window(J.m, xs, xe, ys, ye, rep, W, H);
  pw.cls = __builtin_amdgcn_readfirstlane(pw.cls);
  WarpWin& w = pw.w;
  w.x_lo = __builtin_amdgcn_readfirstlane(w.x_lo); w.x_hi = __builtin_amdgcn_readfirstlane(w.x_hi);
  w.y_lo = __builtin_amdgcn_readfirstlane(w.y_lo); w.y_hi = __builtin_amdgcn_readfirstlane(w.y_hi);
  const uint32_t nv = dw - x0 < 4 ? dw - x0 : 4;
  bool vec = nv == 4;
#pragma unroll
  for (int ch = 0; ch < (DST == FC_TENSOR_NHWC ? 1 : 3); ch++) vec = vec && ((((uintptr_t)f.d[ch] | f.dp[ch]) & dmask) == 0);
  if (pw.cls == kPerspTileBorder) {  // behind the plane: both modes
    if (!mine) return;
    float u[3][4];
#pragma unroll
    for (int ch = 0; ch < 3; ch++)
#pragma unroll
      for (int k = 0; k < 4; k++) u[ch][k] = warp_border(te, ch);
    warp_store4<DST>(f, x0, y, u, te, vec, nv);
    return;
  }
  const bool staged = pw.cls == kPerspTileStage;
  const WarpStrip S = warp_strip(w);  // (not staged: the window is 0 .. 0, never read)
  if (pw.cls == kPerspTileTap || (staged && S.bytes > lds_bytes)) {  // the horizon in the tile, or a strip the dispatch has no room for
    if (mine) persp_gather4<SRC, DST>(J, c, te, W, H, dw, dmask, x0, y);
    return;
  }
  uint8_t* const strip = reinterpret_cast<uint8_t*>(dyn_strip);
  if (staged) {  // the names VPF_STRIP_FILL_WINDOW takes from its scope
    const uint32_t base_px = S.base_px, R_lo = w.y_lo, R_hi = w.y_hi, c_lo = R_lo >> 1, ng = S.ng, units = ((R_hi >> 1) - c_lo + 1) * ng, rowbytes = S.rowbytes;
    VPF_STRIP_FILL_WINDOW
    __syncthreads();
  }
  if (!mine) return;
  const float wmax = (float)(W - 1), hmax = (float)(H - 1);
  float u[3][4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const PerspXY s = persp_xy(J.m, (x0 + k < dw) ? x0 + k : dw - 1, y, rep, wmax, hmax);  // (front: w > 0 on every pixel of this tile)
    const bool in = s.front && s.sx >= 0.f && s.sx <= wmax && s.sy >= 0.f && s.sy <= hmax;
    const float cx = __builtin_amdgcn_fmed3f(s.sx, 0.f, wmax), cy = __builtin_amdgcn_fmed3f(s.sy, 0.f, hmax);  // == sx, sy when in range
    const uint32_t xa0 = (uint32_t)(int)cx, ya0 = (uint32_t)(int)cy;
    const bool inwin = staged && persp_px_in_window(w, xa0, ya0, W, H);
    float v[3] = {0.f, 0.f, 0.f};
    if (staged) {
      // a pixel inside the window keeps its taps (xb = min(xa + 1, W - 1) <= x_hi was tested); every other one reads some pixel of the strip and is
      // replaced below
      const uint32_t xa = xa0 < w.x_lo ? w.x_lo : (xa0 < w.x_hi ? xa0 : w.x_hi), ya = ya0 < w.y_lo ? w.y_lo : (ya0 < w.y_hi ? ya0 : w.y_hi);
      const uint32_t xb = xa + 1 < w.x_hi ? xa + 1 : w.x_hi, yb = ya + 1 < w.y_hi ? ya + 1 : w.y_hi;
      const float fx = cx - (float)xa0, fy = cy - (float)ya0;
      const uint8_t* const ra = strip + (ya - w.y_lo) * S.rowbytes, * const rb = strip + (yb - w.y_lo) * S.rowbytes;
      const uint32_t oa = 4 * (xa - S.base_px), ob = 4 * (xb - S.base_px);
      const uint32_t q00 = *reinterpret_cast<const uint32_t*>(ra + oa), q01 = *reinterpret_cast<const uint32_t*>(ra + ob);
      const uint32_t q10 = *reinterpret_cast<const uint32_t*>(rb + oa), q11 = *reinterpret_cast<const uint32_t*>(rb + ob);
      v[0] = __builtin_truncf(bilerp(ubyte<0>(q00), ubyte<0>(q01), ubyte<0>(q10), ubyte<0>(q11), fx, fy));
      v[1] = __builtin_truncf(bilerp(ubyte<1>(q00), ubyte<1>(q01), ubyte<1>(q10), ubyte<1>(q11), fx, fy));
      v[2] = __builtin_truncf(bilerp(ubyte<2>(q00), ubyte<2>(q01), ubyte<2>(q10), ubyte<2>(q11), fx, fy));
    }
    if (in && !inwin) persp_tap<SRC>(f, c, cx, cy, W, H, v);  // cold: the corner box missed this pixel (or nothing was staged)
#pragma unroll
    for (int ch = 0; ch < 3; ch++) u[ch][k] = in ? v[ch] : warp_border(te, ch);
  }
  warp_store4<DST>(f, x0, y, u, te, vec, nv);
