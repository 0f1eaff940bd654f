"""The case table of the plain resize families (csrc/vpf_resize_plan.h), shared by tests/test_resize_plan_cpu.py (the plan names each row's
launches) and tests/test_gpu_resize_families.py (the library's selection log names them and the bytes equal the oracle's).  Every row is a legal
call at the smallest shape that still reaches its family (the two large Lanczos rows sit just above the byte limits that send one frame to the
matrix cores).

A row: (name, format, filter, sw, sh, dw, dh, frames, (VPF_TUNE_NV12_RGB_VARIANT, _RESIZE_TILE, _RESIZE_BAND, _RESIZE_MFMA), bytes the
source base of every plane is moved off its 256-B alignment, the selection labels in launch order)."""
Y, RGB, NV12, YUV420, RGB_PLANAR, BGR, YCBCR, YUV444, RGB_32F, RGB_32F_PLANAR = 1, 2, 3, 4, 5, 6, 7, 8, 9, 10   # VPF_FMT_* (include/vpf_hip.h)
NEAREST, LINEAR, LANCZOS3 = 0, 1, 2

_PB = "void vpf::launch_plane_batch(hipStream_t, dim3, uint32_t, const BatchArgsL &, int, const PlaneGeom &) [Task = vpf::%s]"
_MP = "void vpf::launch_planes_mp(hipStream_t, dim3, uint32_t, const BatchArgsL &, const PlaneTable &) [TaskCH = vpf::%s]"


def PB(task):
    """one plane over all frames of the dispatch: k_plane_batch<Task>"""
    return _PB % task


def MP(form):
    """every plane of the format in one launch: k_planes_mp<Form>"""
    return _MP % form


def MFMA(kernel):
    """the matrix-core Lanczos launch (k_lanczos_mfma.hip)"""
    return "k_lanczos_mfma<%s>" % kernel


def planes_of(fmt, w, h):
    """[(interleaved channels, bytes per sample, plane width, plane height)] of a w x h frame: resize_jobs of csrc/vpf_abi.hip"""
    cw, ch = (w + 1) // 2, (h + 1) // 2
    return {Y: [(1, 1, w, h)], RGB: [(3, 1, w, h)], BGR: [(3, 1, w, h)], NV12: [(1, 1, w, h), (2, 1, cw, ch)], YUV420: [(1, 1, w, h), (1, 1, cw, ch), (1, 1, cw, ch)],
            YCBCR: [(1, 1, w, h), (1, 1, cw, ch), (1, 1, cw, ch)], YUV444: [(1, 1, w, h)] * 3, RGB_PLANAR: [(1, 1, w, h)] * 3, RGB_32F: [(3, 4, w, h)],
            RGB_32F_PLANAR: [(1, 4, w, h)] * 3}[fmt]


CASES = [
    # exact 2x: the quad-structured streaming kernels
    ("half3 rgb", RGB, LINEAR, 64, 32, 32, 16, 1, (0, 0, 0, 0), 0, ["k_resize_half3_r16"]),
    ("half y", Y, LINEAR, 64, 32, 32, 16, 1, (0, 0, 0, 0), 0, ["(k_resize_half<1>)"]),
    ("half nv12: 1- and 2-channel planes", NV12, LINEAR, 64, 32, 32, 16, 1, (0, 0, 0, 0), 0, [PB("HalfTask<1>"), PB("HalfTask<2>")]),
    ("half3 rgb x3", RGB, LINEAR, 64, 32, 32, 16, 3, (0, 0, 0, 0), 0, [PB("Half3R16Task")]),
    # an up-scale: tiled; a mild down-scale: the row pair
    ("tile y up", Y, LINEAR, 48, 20, 96, 40, 1, (0, 0, 0, 0), 0, ["(k_resize_tile<1, 8>)"]),
    ("tile rgb up", RGB, LINEAR, 48, 20, 96, 40, 1, (0, 0, 0, 0), 0, ["(k_resize_tile<3, 8>)"]),
    ("tile yuv420 up: one launch", YUV420, LINEAR, 48, 20, 96, 40, 1, (0, 0, 0, 0), 0, [MP("TileBl8")]),
    ("tile forced 16 x 4 waves", Y, LINEAR, 48, 20, 96, 40, 2, (0, 16 | (4 << 8), 0, 0), 0, [MP("TileBl4")]),
    ("row pair y", Y, LINEAR, 96, 64, 64, 40, 1, (0, 0, 0, 0), 0, ["(k_resize_lds<1, 1>)"]),
    ("row pair rgb", RGB, LINEAR, 96, 64, 64, 40, 1, (0, 0, 0, 0), 0, ["(k_resize_lds<3, 2>)"]),
    ("row pair nv12: one launch", NV12, LINEAR, 96, 64, 64, 40, 2, (0, 0, 0, 0), 0, [MP("RowPair1")]),
    ("gather: source off by one", Y, LINEAR, 96, 64, 64, 40, 1, (0, 0, 0, 0), 1, ["(k_resize<1, 1>)"]),
    ("nearest", RGB, NEAREST, 96, 64, 64, 40, 1, (0, 0, 0, 0), 0, ["(k_resize<3, 0>)"]),
    # odd integer factors: every filter returns the centre sample
    ("3x bilinear keeps the row pair", Y, LINEAR, 96, 60, 32, 20, 1, (0, 0, 0, 0), 0, ["(k_resize_lds<1, 1>)"]),
    ("3x lanczos -> nearest", Y, LANCZOS3, 96, 60, 32, 20, 1, (0, 0, 0, 0), 0, ["(k_resize<1, 0>)"]),
    ("3x float bilinear -> nearest", RGB_32F, LINEAR, 96, 60, 32, 20, 1, (0, 0, 0, 0), 0, ["(k_resize_f32<3, 0>)"]),
    # the band heights, the narrow form, P1 = 8 and the march form, forced on batches of 2 - 3 frames
    ("band 2", Y, LINEAR, 96, 64, 64, 40, 2, (0, 0, 2, 0), 0, [MP("RowBand2")]),
    ("band 4", Y, LINEAR, 96, 64, 64, 40, 3, (0, 0, 4, 0), 0, [MP("RowBand4")]),
    ("band 8 narrow", Y, LINEAR, 96, 64, 64, 40, 2, (0, 0, 8, 0), 0, [MP("RowBand8n")]),
    ("band 8 wide strips", RGB, LINEAR, 600, 20, 400, 40, 2, (0, 0, 8, 0), 0, [MP("RowBand8")]),
    ("band 16", Y, LINEAR, 48, 20, 96, 40, 2, (0, 0, 16, 0), 0, [MP("RowBand16n")]),
    ("band 8, 8 px per lane", Y, LINEAR, 96, 64, 64, 40, 2, (0, 0, 8 | 0x20000, 0), 0, [MP("RowBand8w")]),
    ("band 16, 8 px per lane", Y, LINEAR, 48, 20, 96, 40, 2, (0, 0, 16 | 0x20000, 0), 0, [MP("RowBand16w")]),
    ("march, 2 bands per wave", Y, LINEAR, 96, 64, 64, 40, 3, (0, 0, 4 | (2 << 8) | 0x20000, 0), 0, [MP("RowBand4wm")]),
    # planes in different families: one launch per plane
    ("nv12, chroma source off by one", NV12, LINEAR, 96, 64, 64, 40, 2, (0, 0, 0, 0), (0, 1), [PB("RowPairTask<1, 1>"), PB("GatherTask<2, 1>")]),
    ("yuv420 band 4, one chroma plane off", YUV420, LINEAR, 96, 64, 64, 40, 2, (0, 0, 4, 0), (0, 0, 1), [PB("RowBandTask<1, 4>"), PB("RowBandTask<1, 4>"), PB("GatherTask<1, 1>")]),
    ("yuv420 up, luma off: tile per plane", YUV420, LINEAR, 48, 20, 96, 40, 2, (0, 0, 0, 0), (1, 0, 0), [PB("GatherTask<1, 1>"), PB("TileTask<1, 8>"), PB("TileTask<1, 8>")]),
    # the large frame table
    ("33 frames", Y, LINEAR, 24, 16, 16, 10, 33, (0, 0, 0, 0), 0, [MP("RowPair1")]),   # (planes this small: up to 128 frames per dispatch)
    # Lanczos: one small plane (tile first), a small batch (matrix cores), matrix cores off (tile, then gather), source off by one (gather)
    ("lanczos one plane", Y, LANCZOS3, 96, 64, 64, 40, 1, (0, 0, 0, 0), 0, ["(k_resize_lztile<1, 8>)"]),
    ("lanczos batch", Y, LANCZOS3, 96, 64, 64, 40, 3, (0, 0, 0, 0), 0, [MFMA("LzMfma4n")]),
    ("lanczos one large plane: matrix cores (28.3 MB against the 28-MB rule)", Y, LANCZOS3, 4096, 4096, 1600, 1200, 1, (0, 0, 0, 0), 0, [MFMA("LzMfma4")]),
    ("lanczos nv12 one frame above 1 MB: matrix cores", NV12, LANCZOS3, 1920, 1080, 1280, 720, 1, (0, 0, 0, 0), 0, [MFMA("LzMfma4")]),
    ("lanczos nv12 one frame: tile for all planes", NV12, LANCZOS3, 96, 64, 64, 40, 1, (0, 0, 0, 0), 0, [MP("TileLz8")]),
    ("lanczos, matrix cores off", RGB, LANCZOS3, 96, 64, 64, 40, 3, (0, 0, 0, 1), 0, [MP("TileLz8")]),
    ("lanczos, matrix cores off, variant 40", RGB, LANCZOS3, 96, 64, 64, 40, 3, (40, 0, 0, 1), 0, [PB("LanczosGatherTask<3>")]),
    ("lanczos nv12, chroma off, matrix cores off", NV12, LANCZOS3, 96, 64, 64, 40, 2, (0, 0, 0, 1), (0, 1), [PB("LanczosTileTask<1, 8>"), PB("LanczosGatherTask<2>")]),
    ("lanczos source off by one", Y, LANCZOS3, 96, 64, 64, 40, 1, (0, 0, 0, 0), 1, ["(k_resize_lanczos<1>)"]),
    # the forms of the matrix-core launch (csrc/vpf_lzm_plan.h: kLzmForms) at two frames: the ring of two, the 8-tile strips (forced: the planner takes
    # 4-tile strips on planes this small), the two- and three-chunk windows of strong horizontal down-scales, half tiles
    ("lanczos up: ring of two, 4-tile strips", Y, LANCZOS3, 16, 32, 16, 64, 2, (0, 0, 0, 0), 0, [MFMA("LzMfma4u")]),
    ("lanczos up: ring of two, 8-tile strips", Y, LANCZOS3, 16, 32, 16, 64, 2, (0, 0, 0, 0x800), 0, [MFMA("LzMfma8u")]),
    ("lanczos 8-tile strips, narrow", Y, LANCZOS3, 16, 64, 16, 40, 2, (0, 0, 0, 0x800), 0, [MFMA("LzMfma8n")]),
    ("lanczos 8-tile strips", RGB, LANCZOS3, 48, 32, 24, 64, 2, (0, 0, 0, 0x800), 0, [MFMA("LzMfma8")]),
    ("lanczos 8-tile strips, wide", RGB, LANCZOS3, 96, 32, 48, 64, 2, (0, 0, 0, 0x800), 0, [MFMA("LzMfma8w")]),
    ("lanczos two-chunk windows, 256-B rows", RGB, LANCZOS3, 48, 32, 16, 64, 2, (0, 0, 0, 0), 0, [MFMA("LzMfma4k4")]),
    ("lanczos two-chunk windows, 384-B rows", RGB, LANCZOS3, 96, 32, 16, 64, 2, (0, 0, 0, 0), 0, [MFMA("LzMfma4k6")]),
    ("lanczos two-chunk windows, 512-B rows", RGB, LANCZOS3, 160, 32, 24, 64, 2, (0, 0, 0, 0), 0, [MFMA("LzMfma4k8")]),
    ("lanczos three-chunk windows, 2-tile strips", Y, LANCZOS3, 160, 32, 16, 64, 2, (0, 0, 0, 0), 0, [MFMA("LzMfma2k6")]),
    ("lanczos half tiles (8 destination rows per tile)", Y, LANCZOS3, 128, 128, 40, 16, 2, (0, 0, 0, 0), 0, [MFMA("LzMfma4")]),
    # float surfaces
    ("float lanczos tiled, packed", RGB_32F, LANCZOS3, 96, 64, 64, 40, 1, (0, 0, 0, 0), 0, ["(k_plane_batch<TileTaskF32<3, true, 8>>)"]),
    ("float lanczos tiled, planar", RGB_32F_PLANAR, LANCZOS3, 96, 64, 64, 40, 2, (0, 0, 0, 0), 0, [PB("TileTaskF32<1, true, 8>")] * 3),
    ("float bilinear gather, packed", RGB_32F, LINEAR, 96, 64, 64, 40, 1, (0, 0, 0, 0), 0, ["(k_resize_f32<3, 1>)"]),
    ("float bilinear gather, planar", RGB_32F_PLANAR, LINEAR, 96, 64, 64, 40, 2, (0, 0, 0, 0), 0, [PB("FloatGatherTask<1, 1>")] * 3),
    ("float lanczos gather, source off by four", RGB_32F, LANCZOS3, 96, 64, 64, 40, 1, (0, 0, 0, 0), 4, ["(k_resize_f32<3, 2>)"]),
]
