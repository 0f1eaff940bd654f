// The body of k_tensor_yuv_r / k_tensor_yuv_r_nhwc (k_rgb2yuv.hip), included into both with NHWC = false / true in scope.
  constexpr int EL = (DT == VPF_TENSOR_F32) ? 4 : 2, PX = 32 / EL, NG = PX / 4;
  const FrameDesc f = args.f[blockIdx.y];
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const uint32_t wt = blockIdx.x * 4 + wv;
  if (wt >= n_tasks) return;
  const uint32_t rg = wt / chunks_x, chunk = wt - rg * chunks_x;
  const uint32_t y0 = 2 * rg, x = (chunk * 64 + lane) * PX;
  if (x >= w) return;  // (w % 16 == 0 and PX divides 16: a lane's pixels are all inside or all outside)
  u32x4 in[2][3][2];  // NHWC: in[r][0..2][0..1] = the six 16-B units of row r in order
#pragma unroll
  for (int r = 0; r < 2; r++)
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
      for (int j = 0; j < 2; j++) {
        if constexpr (NHWC) in[r][k][j] = ldg<false, u32x4>(f.s[0] + (size_t)(y0 + r) * f.sp[0] + (size_t)x * 3 * EL + 16 * (2 * k + j));
        else in[r][k][j] = ldg<false, u32x4>(f.s[k] + (size_t)(y0 + r) * f.sp[k] + (size_t)x * EL + 16 * j);
      }
  const bool swap_rb = NHWC && t.pad != 0;
  uint32_t yo[2][NG], uv[NG], uo[NG / 2], vo[NG / 2];
#pragma unroll
  for (int g = 0; g < NG / 2; g++) uo[g] = vo[g] = 0;
#pragma unroll
  for (int g = 0; g < NG; g++) {
    float q[2][3][4];
#pragma unroll
    for (int r = 0; r < 2; r++) {
      if constexpr (NHWC) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
          float e[3];  // slots 0 1 2 of pixel 4 g + i
#pragma unroll
          for (int sl = 0; sl < 3; sl++) {
            const int el = 3 * (4 * g + i) + sl;  // element of the lane's run
            if constexpr (DT == VPF_TENSOR_F32) e[sl] = __uint_as_float(in[r][el / 8][(el / 4) & 1][el & 3]);
            else e[sl] = tin_widen16<DT>(in[r][el / 16][(el / 8) & 1][(el / 2) & 3], el & 1);
          }
          q[r][0][i] = tin_quant(swap_rb ? e[2] : e[0], t.scale[0], t.bias[0]);
          q[r][1][i] = tin_quant(e[1], t.scale[1], t.bias[1]);
          q[r][2][i] = tin_quant(swap_rb ? e[0] : e[2], t.scale[2], t.bias[2]);
        }
      } else {
#pragma unroll
      for (int k = 0; k < 3; k++)
#pragma unroll
        for (int i = 0; i < 4; i++) {
          float e;
          if constexpr (DT == VPF_TENSOR_F32) e = __uint_as_float(in[r][k][g][i]);
          else e = tin_widen16<DT>(in[r][k][g >> 1][2 * (g & 1) + (i >> 1)], i & 1);
          q[r][k][i] = tin_quant(e, t.scale[k], t.bias[k]);
        }
      }
    }
#pragma unroll
    for (int r = 0; r < 2; r++)
      yo[r][g] = pack4_trunc(mrow(c, 0, q[r][0][0], q[r][1][0], q[r][2][0]), mrow(c, 0, q[r][0][1], q[r][1][1], q[r][2][1]),
                             mrow(c, 0, q[r][0][2], q[r][1][2], q[r][2][2]), mrow(c, 0, q[r][0][3], q[r][1][3], q[r][2][3]));
    // two quads: px {0,1} and {2,3} of both rows; sums of small integers are exact in fp32, as is the 0.25 scale
    uint32_t cu[2], cv[2];
#pragma unroll
    for (int p = 0; p < 2; p++) {
      const float qr = 0.25f * (q[0][0][2 * p] + q[0][0][2 * p + 1] + q[1][0][2 * p] + q[1][0][2 * p + 1]);
      const float qg = 0.25f * (q[0][1][2 * p] + q[0][1][2 * p + 1] + q[1][1][2 * p] + q[1][1][2 * p + 1]);
      const float qb = 0.25f * (q[0][2][2 * p] + q[0][2][2 * p + 1] + q[1][2][2 * p] + q[1][2][2 * p + 1]);
      cu[p] = sat_trunc(mrow(c, 1, qr, qg, qb));
      cv[p] = sat_trunc(mrow(c, 2, qr, qg, qb));
    }
    if constexpr (NV12) uv[g] = cu[0] | (cv[0] << 8) | (cu[1] << 16) | (cv[1] << 24);
    else {
      uo[g >> 1] |= (cu[0] | (cu[1] << 8)) << (16 * (g & 1));
      vo[g >> 1] |= (cv[0] | (cv[1] << 8)) << (16 * (g & 1));
    }
  }
#pragma unroll
  for (int r = 0; r < 2; r++) tin_store<NG>(f.d[0] + (size_t)(y0 + r) * f.dp[0] + x, yo[r]);
  if constexpr (NV12) tin_store<NG>(f.d[1] + (size_t)rg * f.dp[1] + x, uv);
  else {
    tin_store<NG / 2>(f.d[1] + (size_t)rg * f.dp[1] + (x >> 1), uo);
    tin_store<NG / 2>(f.d[2] + (size_t)rg * f.dp[2] + (x >> 1), vo);
  }
