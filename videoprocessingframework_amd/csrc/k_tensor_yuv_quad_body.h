// The body of k_tensor_yuv_quad / k_tensor_yuv_quad_nhwc (k_rgb2yuv.hip), included into both with NHWC = false / true in scope.
  const FrameDesc f = args.f[blockIdx.z];
  const uint32_t qx = blockIdx.x * 64 + (threadIdx.x & 63), qy = blockIdx.y * 4 + (threadIdx.x >> 6);
  const uint32_t x0 = 2 * qx, y0 = 2 * qy;
  if (x0 >= w || y0 >= h) return;
  const uint32_t x1 = (x0 + 1 < w) ? x0 + 1 : x0, y1 = (y0 + 1 < h) ? y0 + 1 : y0;  // edge quads replicate
  const uint32_t xs[4] = {x0, x1, x0, x1}, ys[4] = {y0, y0, y1, y1};
  const uint32_t dtype = t.dtype;
  auto load = [&](int k, uint32_t y, uint32_t x) -> float {
    const uint8_t* row = f.s[NHWC ? 0 : k] + (size_t)y * f.sp[NHWC ? 0 : k];
    if constexpr (NHWC) x = 3 * x + (t.pad ? 2 - k : k);
    if (dtype == VPF_TENSOR_F32) return reinterpret_cast<const float*>(row)[x];
    const uint32_t d = reinterpret_cast<const uint16_t*>(row)[x];
    return dtype == VPF_TENSOR_F16 ? tin_widen16<VPF_TENSOR_F16>(d, 0) : tin_widen16<VPF_TENSOR_BF16>(d, 0);
  };
  float rs = 0.f, gs = 0.f, bs = 0.f;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const uint32_t x = xs[i], y = ys[i];
    const float r = tin_quant(load(0, y, x), t.scale[0], t.bias[0]), g = tin_quant(load(1, y, x), t.scale[1], t.bias[1]),
                b = tin_quant(load(2, y, x), t.scale[2], t.bias[2]);
    rs += r; gs += g; bs += b;  // exact: small integers
    const bool dup = (i == 1 && x1 == x0) || (i == 2 && y1 == y0) || (i == 3 && (x1 == x0 || y1 == y0));
    if (!dup) f.d[0][(size_t)y * f.dp[0] + x] = (uint8_t)sat_trunc(mrow(c, 0, r, g, b));
  }
  rs *= 0.25f; gs *= 0.25f; bs *= 0.25f;  // exact in fp32
  const uint8_t u = (uint8_t)sat_trunc(mrow(c, 1, rs, gs, bs)), v = (uint8_t)sat_trunc(mrow(c, 2, rs, gs, bs));
  if constexpr (NV12) {
    uint8_t* p = f.d[1] + (size_t)qy * f.dp[1] + 2 * (size_t)qx;
    p[0] = u; p[1] = v;
  } else {
    f.d[1][(size_t)qy * f.dp[1] + qx] = u;
    f.d[2][(size_t)qy * f.dp[2] + qx] = v;
  }
