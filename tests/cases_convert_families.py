"""The case table of the convert and relayout families (csrc/vpf_convert_plan.h: kConvertForms), shared by tests/test_convert_plan_cpu.py (the plan
names each row's launches) and tests/test_gpu_convert_families.py (the library's selection log names them and the bytes equal the oracle's).  Every
row is a legal call at the smallest shape that still selects its form: 16 x 2 for the r16 / p16 forms (32 x 2 for NV12 <-> YUV420 r16, 4 x 2 for the
float r4 form), 1024 x 2 for p16x, 4 x 2 (8 x 2: P10) for the lane-group forms, 3 x 3 for the generic kernels; the two 3-Mpx rows sit just below
and just at the size where one planar frame leaves r16 for p16.  Every row of kConvertForms is reached.

A row: (name, entry, source, destination, w, h, frames, VPF_TUNE_NV12_RGB_VARIANT, VPF_EXEC_DST_REUSED, source offset, destination offset, the
selection labels in launch order).  entry "convert": vpf_convert (one frame) / vpf_convert_batch on VPF_FMT_* formats; the offsets move the base of
every plane of every frame off its 256-B alignment, in bytes.  entry "tensor": vpf_tensor_convert / _batch, source = (dtype, nhwc, bgr); its offset is
in elements.  Pitches are the row bytes rounded up to 256."""
Y, RGB, NV12, YUV420, RGB_PLANAR, BGR, YCBCR, YUV444, RGB_32F, RGB_32F_PLANAR, P10, P12 = 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 13   # VPF_FMT_* (include/vpf_hip.h)
F32, F16, BF16 = 0, 1, 2
# the numbers in the labels are FmtClass values (csrc/vpf_classes.h): FC_NV12 0, FC_YUV420 1, FC_YUV444 2, FC_RGB 3, FC_BGR 4, FC_PLANAR 5


def C(name, src, dst, w, h, n, labels, knob=0, reused=0, soff=0, doff=0):
    return (name, "convert", src, dst, w, h, n, knob, reused, soff, doff, labels)


def T(name, dtype, nhwc, bgr, dst, w, h, n, labels, knob=0, soff=0, doff=0):
    return (name, "tensor", (dtype, nhwc, bgr), dst, w, h, n, knob, 0, soff, doff, labels)


CASES = [
    # ---- NV12 / YUV420 -> RGB / BGR / RGB_PLANAR
    C("p16 single", NV12, RGB, 16, 2, 1, ["(k_nv12_rgb_p16_one<3, true, 0>)"]),
    C("p16 batch of 2", YUV420, BGR, 16, 2, 2, ["(k_nv12_rgb_p16<4, true, 0, 1>)"]),
    C("p16 batch of 4: ballast", NV12, RGB, 16, 2, 4, ["(k_nv12_rgb_p16<3, true, 16, 0>)"]),
    C("planar r16 single", NV12, RGB_PLANAR, 16, 2, 1, ["(k_nv12_planar_r16_one<true, 0>)"]),
    C("planar r16 batch", YUV420, RGB_PLANAR, 16, 2, 2, ["(k_nv12_planar_r16<true, 1>)"]),
    C("p16x batch of 4: ballast", NV12, RGB, 1024, 2, 4, ["(k_nv12_rgb_p16x<3, true, 16, 0>)"]),
    C("p16x single entry (knob 46)", NV12, RGB, 1024, 2, 1, ["(k_nv12_rgb_p16x_one<3, true, 0>)"], knob=46),
    C("p16x without ballast (knob 45)", YUV420, BGR, 1024, 2, 2, ["(k_nv12_rgb_p16x<4, true, 0, 1>)"], knob=45),
    C("1024 px single: p16 by policy", NV12, BGR, 1024, 2, 1, ["(k_nv12_rgb_p16_one<4, true, 0>)"]),
    C("p16x asked of a planar output: p16", NV12, RGB_PLANAR, 1024, 2, 2, ["(k_nv12_rgb_p16<5, true, 16, 0>)"], knob=46),
    C("reused destination: allocating p16 (knob 12)", NV12, RGB, 16, 2, 1, ["(k_nv12_rgb_p16_one<3, false, 0>)"], reused=1),
    C("reused destination, 2 frames", NV12, RGB, 16, 2, 2, ["(k_nv12_rgb_p16<3, false, 0, 0>)"], reused=1),
    C("reused planar destination: allocating r16 (knob 44)", NV12, RGB_PLANAR, 16, 2, 1, ["(k_nv12_planar_r16_one<false, 0>)"], reused=1),
    C("reused planar destination, 2 frames", YUV420, RGB_PLANAR, 16, 2, 2, ["(k_nv12_planar_r16<false, 1>)"], reused=1),
    C("reused destination, 4 frames: the batch policy", NV12, RGB, 16, 2, 4, ["(k_nv12_rgb_p16<3, true, 16, 0>)"], reused=1),
    C("one planar frame just below 3 Mpx: r16", NV12, RGB_PLANAR, 2048, 1534, 1, ["(k_nv12_planar_r16_one<true, 0>)"]),
    C("one planar frame at 3 Mpx: p16", NV12, RGB_PLANAR, 2048, 1536, 1, ["(k_nv12_rgb_p16_one<5, true, 0>)"]),
    C("33 frames: 32 + a single-frame dispatch", NV12, RGB, 16, 2, 33, ["(k_nv12_rgb_p16<3, true, 16, 0>)", "(k_nv12_rgb_p16_one<3, true, 0>)"]),
    C("p4 single: bases 4 B off", NV12, RGB, 4, 2, 1, ["(k_yuv420_rgb_p4_one<0, 3>)"], soff=4, doff=4),
    C("p4 batch", YUV420, RGB_PLANAR, 4, 2, 2, ["(k_yuv420_rgb_p4<1, 5>)"], soff=4, doff=4),
    C("knob 40 on a regular frame: p4", NV12, RGB, 16, 2, 1, ["(k_yuv420_rgb_p4_one<0, 3>)"], knob=40),
    C("r16 asked of a packed output (knob 37): p4", NV12, RGB, 16, 2, 1, ["(k_yuv420_rgb_p4_one<0, 3>)"], knob=37),
    C("generic: source 1 B off", NV12, RGB, 3, 3, 1, ["(k_yuv_rgb_generic<0, 3>)"], soff=1),
    C("generic: knob 9 on a regular frame", YUV420, BGR, 16, 2, 2, ["(k_yuv_rgb_generic<1, 4>)"], knob=9),
    # ---- YUV444 -> RGB / BGR / RGB_PLANAR
    C("444 r16 single", YUV444, RGB, 16, 2, 1, ["(k_yuv444_rgb_r16_one<3>)"]),
    C("444 r16 batch", YUV444, RGB_PLANAR, 16, 2, 2, ["(k_yuv444_rgb_r16<5>)"]),
    C("444 p4", YUV444, RGB, 4, 2, 1, ["(k_yuv444_rgb_p4<3, 1>)"], soff=4, doff=4),
    C("444 knob 40: p4", YUV444, BGR, 16, 2, 1, ["(k_yuv444_rgb_p4<4, 1>)"], knob=40),
    C("444 generic", YUV444, BGR, 3, 3, 1, ["(k_yuv_rgb_generic<2, 4>)"], soff=1),
    # ---- RGB / BGR / RGB_PLANAR -> YUV444 / YUV420 / YCBCR
    C("rgb2yuv r16 single, 4:2:0", RGB, YUV420, 16, 2, 1, ["(k_rgb_yuv_r16_one<3, true>)"]),
    C("rgb2yuv r16 batch, 4:4:4", BGR, YUV444, 16, 2, 2, ["(k_rgb_yuv_r16<4, false>)"]),
    C("rgb2yuv r16 planar source, YCBCR", RGB_PLANAR, YCBCR, 16, 2, 1, ["(k_rgb_yuv_r16_one<5, true>)"]),
    C("rgb2yuv p4", RGB, YUV420, 4, 2, 1, ["(k_rgb_yuv_p4<3, true>)"], soff=4, doff=4),
    C("rgb2yuv knob 40: p4", RGB_PLANAR, YUV444, 16, 2, 2, ["(k_rgb_yuv_p4<5, false>)"], knob=40),
    C("rgb2yuv quad", RGB, YUV420, 3, 3, 1, ["(k_rgb_yuv_quad<3, true>)"], soff=1),
    C("rgb2yuv quad: odd height of a 4:4:4 frame", BGR, YUV444, 4, 3, 1, ["(k_rgb_yuv_quad<4, false>)"]),
    # ---- float tensor -> NV12 / YUV420
    T("tensor r f32 nv12", F32, False, False, NV12, 16, 2, 1, ["(k_tensor_yuv_r<0, true, false>)"]),
    T("tensor r f16 yuv420 nhwc", F16, True, True, YUV420, 16, 2, 2, ["(k_tensor_yuv_r<1, false, true>)"]),
    T("tensor r bf16 nv12 nhwc", BF16, True, False, NV12, 16, 2, 1, ["(k_tensor_yuv_r<2, true, true>)"]),
    T("tensor r bf16 yuv420", BF16, False, True, YUV420, 16, 2, 2, ["(k_tensor_yuv_r<2, false, false>)"]),
    T("tensor quad nv12", F32, False, False, NV12, 3, 3, 1, ["(k_tensor_yuv_quad<true, false>)"]),
    T("tensor quad yuv420 nhwc: source one element off", F16, True, False, YUV420, 16, 2, 2, ["(k_tensor_yuv_quad<false, true>)"], soff=1),
    T("tensor quad nv12 nhwc", BF16, True, True, NV12, 3, 3, 1, ["(k_tensor_yuv_quad<true, true>)"]),
    T("tensor quad yuv420: knob 9", F32, False, True, YUV420, 16, 2, 1, ["(k_tensor_yuv_quad<false, false>)"], knob=9),
    # ---- relayouts
    C("nv12 -> yuv420 r16 single", NV12, YUV420, 32, 2, 1, ["(k_nv12_yuv420_r16_one<true>)"]),
    C("yuv420 -> nv12 r16 batch", YUV420, NV12, 32, 2, 2, ["(k_nv12_yuv420_r16<false>)"]),
    C("nv12 -> yuv420 p16: w % 32 != 0", NV12, YUV420, 16, 2, 1, ["(k_nv12_yuv420_p16<true>)"]),
    C("yuv420 -> nv12 p16: knob 40", YUV420, NV12, 32, 2, 2, ["(k_nv12_yuv420_p16<false>)"], knob=40),
    C("rgb -> planar r16 single", RGB, RGB_PLANAR, 16, 2, 1, ["(k_rgb_relayout_r16_one<0>)"]),
    C("bgr -> planar r16: planes exchanged", BGR, RGB_PLANAR, 16, 2, 2, ["(k_rgb_relayout_r16<0>)"]),
    C("planar -> bgr r16: planes exchanged", RGB_PLANAR, BGR, 16, 2, 1, ["(k_rgb_relayout_r16_one<1>)"]),
    C("rgb -> bgr r16", RGB, BGR, 16, 2, 2, ["(k_rgb_relayout_r16<2>)"]),
    C("bgr -> planar p4: planes exchanged", BGR, RGB_PLANAR, 4, 2, 1, ["(k_rgb_relayout_p4<0>)"], soff=4, doff=4),
    C("planar -> rgb p4", RGB_PLANAR, RGB, 4, 2, 2, ["(k_rgb_relayout_p4<1>)"], soff=4, doff=4),
    C("bgr -> rgb p4", BGR, RGB, 4, 2, 1, ["(k_rgb_relayout_p4<2>)"], soff=4, doff=4),
    C("nv12 -> y copy", NV12, Y, 16, 2, 1, ["(k_copy_plane_p16<false>)"]),
    C("y -> yuv444 copy and fill", Y, YUV444, 16, 2, 2, ["(k_copy_plane_p16<true>)"]),
    C("rgb -> rgb_32f x4 single", RGB, RGB_32F, 16, 2, 1, ["k_u8_to_f32_x4_one<4>"]),
    C("rgb -> rgb_32f x4 batch", RGB, RGB_32F, 16, 2, 2, ["k_u8_to_f32_x4<4>"]),
    C("rgb -> rgb_32f p4", RGB, RGB_32F, 4, 2, 1, ["k_u8_to_f32_p4"], soff=4),
    C("rgb_32f -> planar r4 single: w % 4", RGB_32F, RGB_32F_PLANAR, 4, 2, 1, ["k_rgb32f_planar_r4_one"]),
    C("rgb_32f -> planar r4 batch", RGB_32F, RGB_32F_PLANAR, 4, 2, 2, ["k_rgb32f_planar_r4"]),
    C("p10 -> nv12 x16 single", P10, NV12, 16, 2, 1, ["k_p16_to_8_x16_one"]),
    C("p12 -> nv12 x16 batch", P12, NV12, 16, 2, 2, ["k_p16_to_8_x16"]),
    C("p10 -> nv12 p8", P10, NV12, 8, 2, 1, ["k_p16_to_8_p8"], doff=8),
    C("rgb -> y r16 single", RGB, Y, 16, 2, 1, ["(k_gray_r16_one<0>)"]),
    C("bgr -> y r16 batch", BGR, Y, 16, 2, 2, ["(k_gray_r16<1>)"]),
    C("planar -> y r16 single", RGB_PLANAR, Y, 16, 2, 1, ["(k_gray_r16_one<2>)"]),
    C("rgb -> y p4", RGB, Y, 4, 2, 1, ["(k_gray_p4<0>)"], soff=4, doff=4),
    C("bgr -> y p4", BGR, Y, 4, 2, 2, ["(k_gray_p4<1>)"], soff=4, doff=4),
    C("planar -> y p4: knob 40", RGB_PLANAR, Y, 16, 2, 1, ["(k_gray_p4<2>)"], knob=40),
    # the generic kernel, every op it is instantiated for (OP_NV12_YUV420 = 0 ... OP_PLANAR_GRAY = 12)
    C("generic nv12 -> yuv420", NV12, YUV420, 3, 3, 1, ["(k_relayout_generic<0>)"], soff=1),
    C("generic yuv420 -> nv12", YUV420, NV12, 3, 3, 2, ["(k_relayout_generic<1>)"], soff=1),
    C("generic bgr -> planar: planes exchanged", BGR, RGB_PLANAR, 3, 3, 1, ["(k_relayout_generic<2>)"], soff=1),
    C("generic planar -> bgr: planes exchanged", RGB_PLANAR, BGR, 3, 3, 1, ["(k_relayout_generic<3>)"], soff=1),
    C("generic rgb -> bgr", RGB, BGR, 3, 3, 1, ["(k_relayout_generic<4>)"], soff=1),
    C("generic nv12 -> y", NV12, Y, 3, 3, 1, ["(k_relayout_generic<5>)"], soff=1),
    C("generic y -> yuv444", Y, YUV444, 3, 3, 1, ["(k_relayout_generic<6>)"], soff=1),
    C("generic rgb -> rgb_32f", RGB, RGB_32F, 3, 3, 1, ["(k_relayout_generic<7>)"], soff=1),
    C("generic rgb_32f -> planar: knob 40 takes the r4 form away", RGB_32F, RGB_32F_PLANAR, 4, 2, 1, ["(k_relayout_generic<8>)"], knob=40),
    C("generic p10 -> nv12", P10, NV12, 3, 3, 1, ["(k_relayout_generic<9>)"]),
    C("generic rgb -> y", RGB, Y, 3, 3, 1, ["(k_relayout_generic<10>)"], soff=1),
    C("generic bgr -> y", BGR, Y, 3, 3, 1, ["(k_relayout_generic<11>)"], soff=1),
    C("generic planar -> y", RGB_PLANAR, Y, 3, 3, 1, ["(k_relayout_generic<12>)"], soff=1),
]
