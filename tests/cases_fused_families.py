"""The case tables of the whole-frame fused tensor tests (tests/test_gpu_tensor_out.py, tests/test_gpu_tensor_nhwc.py, tests/test_gpu_p16_tensor.py):
the smallest shapes at which each kernel family of launch_convert_resize (csrc/k_convert_resize.hip) and each band height is reached, and what the
selection log (VPF_HIP_LOG=2) must say for them.  A module of its own so that the CPU test of the policy (tests/test_fused_plan_cpu.py: the plan
function of csrc/vpf_fused_plan.h names the same family for every row) imports it without a GPU.

The log carries the template-id the code object holds: "(k_convert_strip_wg<0, 8, 2, BatchArgsTE<32>>)" — source class, destination class, the
family's own argument, the frame table.  `label` below is the one place that spelling is written down."""

NV12, YUV420, P16 = 0, 1, 7                      # FmtClass (csrc/vpf_classes.h): the source classes ...
RGB, BGR, PLANAR, TENSOR, TENSOR_NHWC = 3, 4, 5, 6, 8   # ... and the destination classes
SMALL_BATCH = 32                                 # frames of the small frame table (kSmallBatch); more travel in the table of 128

HALF, STRIP, BAND, LDS, GATHER = "k_convert_half", "k_convert_strip_wg", "k_convert_resize_band", "k_convert_resize_lds", "k_convert_resize"
FAMILIES = (HALF, STRIP, BAND, LDS, GATHER)


def label(family, r, src, dst, n):
    """the selection-log label of a frame-table launch: r = the band height R of STRIP (2 / 4 / 8 / 16), the strip passes IT of BAND and LDS (1 / 2),
    None for HALF and GATHER; tensor destinations carry the epilogue behind the table (BatchArgsTE), 8-bit ones do not (BatchArgsT)"""
    targs = [src, dst] + ([r] if r is not None else []) + ([4] if family == BAND else [])   # (k_convert_resize_band<SRC, DST, IT, 4 rows per wave>)
    table = f"{'BatchArgsTE' if dst in (TENSOR, TENSOR_NHWC) else 'BatchArgsT'}<{SMALL_BATCH if n <= SMALL_BATCH else 128}>"
    return f"({family}<{', '.join(str(t) for t in targs)}, {table}>)"


def label_one(family, r, src, dst):
    """... of the single-frame scalar-argument entries (8-bit destinations of HALF and LDS, one frame)"""
    return f"({family}_one<{', '.join(str(t) for t in [src, dst] + ([r] if r is not None else []))}>)"


# tests/test_gpu_tensor_out.py — planar f32 tensors from NV12:
# (name, sw, sh, dw, dh, frames, VPF_TUNE_NV12_RGB_VARIANT, source offset, the label the selection log must carry)
TENSOR_OUT_CASES = [
    ("half", 3840, 2160, 1920, 1080, 1, 0, 0, label(HALF, None, NV12, TENSOR, 1)),
    ("strip_down", 1920, 1080, 1280, 720, 1, 0, 0, label(STRIP, 2, NV12, TENSOR, 1)),
    ("strip_up", 1280, 720, 1920, 1080, 1, 0, 0, label(STRIP, 4, NV12, TENSOR, 1)),
    ("band", 3840, 2160, 1600, 900, 32, 0, 0, label(BAND, 1, NV12, TENSOR, 32)),
    ("odd3x", 1920, 1080, 640, 360, 1, 0, 0, label(LDS, 1, NV12, TENSOR, 1)),
    ("resnet", 1920, 1080, 224, 224, 1, 0, 0, label(GATHER, None, NV12, TENSOR, 1)),   # the network input: its source span exceeds the LDS strips
    ("gather", 1917, 1079, 223, 225, 1, 0, 1, label(GATHER, None, NV12, TENSOR, 1)),   # source base 1 byte off: no LDS path
    ("lds_forced", 1920, 1080, 1280, 720, 2, 40, 0, label(LDS, 1, NV12, TENSOR, 2)),
    ("band_forced", 1920, 1080, 800, 450, 3, 49, 0, label(BAND, 1, NV12, TENSOR, 3)),  # (1080p -> 224 x 224 spans too many source columns for LDS)
    ("gather_forced", 1280, 720, 1920, 1080, 1, 9, 0, label(GATHER, None, NV12, TENSOR, 1)),
]

# tests/test_gpu_tensor_nhwc.py — channels-last tensors; the source class varies inside the test (NV12, YUV420, and P10 where the family has a 16-bit
# instantiation), so a row names (family, r) and the test builds the label:
# (name, sw, sh, dw, dh, frames, VPF_TUNE_NV12_RGB_VARIANT, source offset in samples, (family, r), 16-bit instantiation too)
TENSOR_NHWC_CASES = [
    # two full 512-pixel wave chunks and a third with ONE active lane: the LDS hand-off with inactive lanes
    ("half", 2080, 8, 1040, 4, 1, 0, 0, (HALF, None), True),
    ("strip_r2_down", 192, 48, 128, 32, 1, 0, 0, (STRIP, 2), True),   # 3 : 2 down
    ("strip_r2_up", 128, 32, 192, 48, 1, 0, 0, (STRIP, 2), True),     # 3 : 2 up
    # the 4-, 8- and 16-row bands need 512 / 2048 workgroups in the launch: the tall narrow pictures of tests/test_gpu_p16_tensor.py
    ("strip_r4", 8, 2560, 16, 2048, 8, 0, 0, (STRIP, 4), True),
    ("strip_r8", 8, 2560, 16, 2048, 32, 0, 0, (STRIP, 8), True),
    ("strip_r16", 8, 1024, 16, 2048, 64, 0, 0, (STRIP, 16), True),
    ("odd3x", 768, 48, 256, 16, 1, 0, 0, (LDS, 1), False),
    ("lds_forced", 192, 48, 128, 32, 1, 40, 0, (LDS, 1), False),
    ("band_forced", 640, 90, 256, 36, 3, 49, 0, (BAND, 1), False),
    ("gather", 61, 35, 13, 9, 1, 0, 1, (GATHER, None), True),           # dw % 4 != 0: the nv < 4 tail; source base one sample off
    ("gather_forced", 128, 32, 192, 48, 1, 9, 0, (GATHER, None), True),
]

# tests/test_gpu_p16_tensor.py — P10 / P12 whole frames into planar tensors:
# (name, sw, sh, dw, dh, frames, VPF_TUNE_NV12_RGB_VARIANT, (row alignment, extra pitch bytes), the label the selection log must carry)
P16_WHOLE_CASES = [
    ("half_across_chunks", 1056, 36, 528, 18, 1, 0, (256, 0), label(HALF, None, P16, TENSOR, 1)),       # exact 2x, a wave's 1024-px chunk boundary inside the row
    ("strip_down_1_25", 160, 96, 128, 80, 1, 0, (256, 0), label(STRIP, 2, P16, TENSOR, 1)),
    ("strip_up_2", 64, 40, 128, 80, 1, 0, (256, 0), label(STRIP, 2, P16, TENSOR, 1)),
    ("odd_3x", 192, 96, 64, 32, 1, 0, (256, 0), label(GATHER, None, P16, TENSOR, 1)),                    # odd integer factor: no strip; no 16-bit per-tap LDS form: gather
    ("odd_sizes_pitch_plus_2", 131, 79, 61, 35, 1, 0, (64, 2), label(GATHER, None, P16, TENSOR, 1)),     # rows start at addresses that are only 2-B aligned
    ("gather_forced", 160, 96, 128, 80, 1, 9, (256, 0), label(GATHER, None, P16, TENSOR, 1)),
    ("batch_3", 64, 40, 128, 80, 3, 0, (256, 0), label(STRIP, 2, P16, TENSOR, 3)),
    ("batch_33_large_table", 64, 40, 32, 20, 33, 0, (256, 0), label(HALF, None, P16, TENSOR, 33)),       # > 32 frames: the BatchArgsTE<128> instantiation
    # the 4-, 8- and 16-row bands of the workgroup strip need 512 / 2048 workgroups in the launch: tall, narrow pictures reach them with few bytes
    ("strip_r4", 8, 2560, 16, 2048, 8, 0, (256, 0), label(STRIP, 4, P16, TENSOR, 8)),
    ("strip_r8", 8, 2560, 16, 2048, 32, 0, (256, 0), label(STRIP, 8, P16, TENSOR, 32)),
    ("strip_r16_large_table", 8, 1024, 16, 2048, 64, 0, (256, 0), label(STRIP, 16, P16, TENSOR, 64)),
]
