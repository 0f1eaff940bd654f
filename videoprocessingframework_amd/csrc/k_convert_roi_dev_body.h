// The body of k_roi_dev / k_roi_dev_nhwc (k_convert_roi_dev.hip), included into both with DST = FC_TENSOR / FC_TENSOR_NHWC in scope.
  constexpr int R = kRoiBandRows;
  const uint32_t job = blockIdx.z;
  // 1. the count: jobs at or behind it write nothing
  uint32_t cnt = args.max_n;
  if (args.count) {
    const int32_t v = __builtin_amdgcn_readfirstlane(*args.count);
    cnt = v < 0 ? 0u : ((uint32_t)v < args.max_n ? (uint32_t)v : args.max_n);
  }
  if (job >= cnt) return;
  // 2. the five ints of this job, wave-uniform
  const int32_t* const bp = reinterpret_cast<const int32_t*>(reinterpret_cast<const uint8_t*>(args.boxes) + (size_t)job * args.box_stride);
  const int32_t b_f = __builtin_amdgcn_readfirstlane(bp[0]), b_x = __builtin_amdgcn_readfirstlane(bp[1]), b_y = __builtin_amdgcn_readfirstlane(bp[2]),
                b_w = __builtin_amdgcn_readfirstlane(bp[3]), b_h = __builtin_amdgcn_readfirstlane(bp[4]);
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63, tid = threadIdx.x;
  const uint32_t Y0 = blockIdx.y * (4 * R), xs = blockIdx.x * 256;  // the grid covers the destination exactly: Y0 < dh, xs < dw
  const uint32_t Y1 = (Y0 + 4 * R - 1 < dh - 1) ? Y0 + 4 * R - 1 : dh - 1, xe = (xs + 255 < dw - 1) ? xs + 255 : dw - 1;
  const TensorEpi te = args.e;
  FrameDesc f;
#pragma unroll
  for (int ch = 0; ch < 3; ch++) {
    f.d[ch] = (DST == FC_TENSOR_NHWC && ch) ? nullptr : args.d[ch] + (size_t)job * args.job_stride;
    f.dp[ch] = args.dp[ch];
  }
  const uint32_t ya = Y0 + wv * R, yb = (ya + R - 1 < Y1) ? ya + R - 1 : Y1;  // this wave's rows (none when ya > Y1)
  const uint32_t x0 = xs + lane * 4;                                        // this lane's four columns (none when x0 >= dw)
  const uint32_t nv = x0 < dw ? (dw - x0 < 4 ? dw - x0 : 4) : 0;
  bool vec = nv == 4;
#pragma unroll
  for (int ch = 0; ch < (DST == FC_TENSOR_NHWC ? 1 : 3); ch++) vec = vec && ((((uintptr_t)f.d[ch] | f.dp[ch]) & dmask) == 0);
  // 3. the guard (vpf_job_bounds.h): an invalid box reads no frame; its tile takes the epilogue of byte 0
  if (!roi_dev_box_ok(b_f, b_x, b_y, b_w, b_h, args.n_frames, W, H)) {
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
  const FrameSrcDesc& fs = args.f[b_f];
#pragma unroll
  for (int ch = 0; ch < 3; ch++) { f.s[ch] = fs.s[ch]; f.sp[ch] = fs.sp[ch]; }
  const uint32_t rx = (uint32_t)b_x, ry = (uint32_t)b_y, rw = (uint32_t)b_w, rh = (uint32_t)b_h;
  // 4. the scale factors: the correctly rounded fp32 quotients the host entry computes
  const float scx = (float)rw / (float)dw, scy = (float)rh / (float)dh;
  // staged or per tap: this tile's own window
  RoiTileWin win = roi_tile_window(rx, rw, rh, scx, scy, xs, xe, Y0, Y1);
  win.first = __builtin_amdgcn_readfirstlane(win.first); win.last = __builtin_amdgcn_readfirstlane(win.last);
  win.lo = __builtin_amdgcn_readfirstlane(win.lo); win.hi = __builtin_amdgcn_readfirstlane(win.hi);
  win.base_px = win.first & ~1u; win.ng = ((win.last - win.base_px) >> 3) + 1u; win.rowbytes = 32u * win.ng + 16u; win.rows = win.hi - win.lo + 1u;
  if (roi_tile_staged(roi_tile_need_of(win, dw, dh), lds_bytes)) {
    // the staged form: k_roi_strip from its fill stage on
    const uint32_t base_px = win.base_px, R_lo_rel = win.lo, R_lo = ry + win.lo, R_hi = ry + win.hi;  // frame rows
    uint8_t* const strip = reinterpret_cast<uint8_t*>(dyn_strip);
    const uint32_t c_lo = R_lo >> 1, ncr = (R_hi >> 1) - c_lo + 1, ng = win.ng, units = ncr * ng;
    const uint32_t rowbytes = win.rowbytes;
    VPF_STRIP_FILL_WINDOW  // (k_fused_common.h)
    __syncthreads();
    if (ya > Y1) return;
    const Tap row_taps = band_row_taps(ya, yb, scy, rh);  // every lane of the wave still active here
    if (!nv) return;
    const ColTapsX T = make_col_taps_x(base_px - rx, x0, dw, rw, scx);
    band_blend_rows<3, R>(strip, rowbytes, R_lo_rel, ya, yb, row_taps, T, [&](uint32_t y, const float* o) {  // o: pixel-major R G B, + 0.5 added
      if constexpr (DST == FC_TENSOR_NHWC) {
        tensor_store4_nhwc_trunc<false>(f.d[0] + (size_t)y * f.dp[0], x0, o, 1, 3, te, vec, nv, wv, lane);
      } else {
#pragma unroll
        for (int ch = 0; ch < 3; ch++) tensor_store4_trunc<false>(f.d[ch] + (size_t)y * f.dp[ch], x0, o + ch, 3, te, ch, vec, nv);
      }
    });
    return;
  }
  // per tap: k_roi_gather's pixel, this wave's rows one after the other
  if (ya > Y1 || !nv) return;
  Tap tx[4];
#pragma unroll
  for (int k = 0; k < 4; k++) tx[k] = make_tap<VPF_INTERP_LINEAR>((x0 + k < dw) ? x0 + k : dw - 1, scx, rw);
  for (uint32_t y = ya; y <= yb; y++) {
    const Tap ty = make_tap<VPF_INTERP_LINEAR>(y, scy, rh);
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
