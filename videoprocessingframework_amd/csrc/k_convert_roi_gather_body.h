// The body of k_roi_gather / k_roi_gather_nhwc (k_convert_roi.hip), included into both with DST = FC_TENSOR / FC_TENSOR_NHWC in scope.
  const RoiDesc& J = args.j[blockIdx.z];
  const FrameDesc& f = J.f;
  const uint32_t x0 = (blockIdx.x * 64 + (threadIdx.x & 63)) * 4;
  const uint32_t y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x0 >= dw || y >= dh) return;
  const Tap ty = make_tap<VPF_INTERP_LINEAR>(y, J.scy, J.h);
  float o[3][4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const Tap tx = make_tap<VPF_INTERP_LINEAR>((x0 + k < dw) ? x0 + k : dw - 1, J.scx, J.w);
    float p00[3], p01[3], p10[3], p11[3];
    texel_rgb<SRC>(f, c, J.x + tx.i0, J.y + ty.i0, p00);
    texel_rgb<SRC>(f, c, J.x + tx.i1, J.y + ty.i0, p01);
    texel_rgb<SRC>(f, c, J.x + tx.i0, J.y + ty.i1, p10);
    texel_rgb<SRC>(f, c, J.x + tx.i1, J.y + ty.i1, p11);
#pragma unroll
    for (int ch = 0; ch < 3; ch++) o[ch][k] = bilerp(p00[ch], p01[ch], p10[ch], p11[ch], tx.f, ty.f);
  }
  const uint32_t nv = dw - x0 < 4 ? dw - x0 : 4;
  bool vec = nv == 4;
#pragma unroll
  for (int ch = 0; ch < (DST == FC_TENSOR_NHWC ? 1 : 3); ch++) vec = vec && ((((uintptr_t)f.d[ch] | f.dp[ch]) & dmask) == 0);
  if constexpr (DST == FC_TENSOR_NHWC) {
    tensor_store4_nhwc_trunc<false>(f.d[0] + (size_t)y * f.dp[0], x0, &o[0][0], 4, 1, args.e, vec, nv,
                                    __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), threadIdx.x & 63);
  } else {
    for (int ch = 0; ch < 3; ch++) tensor_store4_trunc<false>(f.d[ch] + (size_t)y * f.dp[ch], x0, o[ch], 1, args.e, ch, vec, nv);
  }
