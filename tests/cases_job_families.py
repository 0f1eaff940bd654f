"""The case table of tests/test_gpu_job_families.py: the eight per-job tensor entries at the smallest shapes at which the launch policy
(csrc/vpf_job_plan.h) still has something to decide.  For each of the four families and each of the six (source format, layout) pairs: ONE host call
of three jobs ordered staged, per tap, staged — each job into a destination of its own, so a slot mix-up between the two job tables moves pixels
between jobs — and ONE device-table call; dtypes rotate over the rows.  Beside them: the perspective job whose horizon crosses the destination
(staged, with the full 64 KiB), device rows with and without the hint and one under the tuning knob, and one ROI call of 97 and one letterbox call
of 83 jobs, whose second table holds one job.  tests/test_job_plan_cpu.py checks without a device that every row selects what it claims and derives
the labels the GPU test reads off the selection log from the plan alone.

A row: dict(name, family, dev, sf, nhwc, dtype, W, H, dw, dh, knob, jobs, want) —
  jobs   ROI: rectangles (x, y, w, h); letterbox: (rectangle, placement (ix, iy, iw, ih)); warp: six floats; perspective: nine;
         a device row's jobs are the contents of its device table (letterbox: rectangles only, the kernel fits them)
  want   host rows: 'S' (staged) or 'T' (per tap) per job, in call order; device rows: None
  max_step  device warps: the hint (0: none)"""

ROI, LETTERBOX, WARP, PERSP = range(4)
FAMILY_NAMES = ("roi", "letterbox", "warp", "persp")
SOURCES = ("NV12", "YUV420", "P10")
SRC_FC = {"NV12": 0, "YUV420": 1, "P10": 7}      # FmtClass (csrc/vpf_classes.h)
PAIRS = [(sf, nhwc) for sf in SOURCES for nhwc in (False, True)]
CAPS = (96, 82, 96, 82)

# ROI: frames of 72 x 40.  Host call into 8 x 4 — a 72 x 40 frame holds no rectangle that an 64 x 32 destination would sample per tap.
ROI_FRAME = (72, 40)
ROI_HOST_DST = (8, 4)
ROI_HOST = [(2, 0, 8, 4), (3, 0, 60, 30), (4, 3, 8, 4)]                 # staged (1.5 px per px), per tap (45 px per px), staged
ROI_DEV_DST = (64, 32)
ROI_DEV = [(2, 0, 64, 32), (0, 0, 72, 40), (3, 1, 33, 17)]              # 4 624 B at 1.13 px per px; the whole frame; an up-scale at odd offsets
# letterbox: planes of 72 x 40
LB_DST = (72, 40)
LB_HOST = [((2, 0, 64, 32), (4, 4, 64, 32)), ((3, 0, 60, 30), (4, 6, 8, 4)), ((2, 0, 64, 32), (4, 6, 64, 24))]   # placed; per tap; picture shorter than the plane
# the warps: a host call 160 x 160 -> 32 x 32 (a 5 x down-scale needs 103 648 / 104 960 B against 65 536), device calls 64 x 32 -> 16 x 8
WARP_HOST_FRAME, WARP_HOST_DST = (160, 160), (32, 32)
WARP_HOST = [(1.0, 0.0, 3.0, 0.0, 1.0, 2.0), (5.0, 0.0, 0.0, 0.0, 5.0, 0.0), (1.0, 0.0, 40.5, 0.0, 1.0, 7.25)]
PERSP_HOST = [WARP_HOST[0] + (0.0, 0.0, 1.0), WARP_HOST[1] + (0.0, 0.0, 1.0), WARP_HOST[2] + (1e-4, 2e-4, 1.0)]
WARP_DEV_FRAME, WARP_DEV_DST = (64, 32), (16, 8)
WARP_DEV = [(1.0, 0.0, 3.0, 0.0, 1.0, 2.0), (2.0, 0.0, 1.5, 0.0, 2.0, 0.5), (0.0, -1.0, 20.0, 1.0, 0.0, 4.0)]   # identity with an offset (1 120 / 1 344 B), 2 x, a right angle
PERSP_DEV = [WARP_DEV[0] + (0.0, 0.0, 1.0), WARP_DEV[1] + (1e-3, 0.0, 1.0), WARP_DEV[2] + (0.0, 0.0, 1.0)]
HORIZON = (1.0, 0.0, 2.0, 0.0, 1.0, 1.0, 0.0, -0.1, 1.0)                # w = 1 - 0.1 dy: not positive from row 10 on


def _row(name, family, dev, sf, nhwc, dtype, frame, dst, jobs, want=None, knob=0, max_step=0.0):
    return dict(name=name, family=family, dev=dev, sf=sf, nhwc=nhwc, dtype=dtype, W=frame[0], H=frame[1], dw=dst[0], dh=dst[1], knob=knob, jobs=list(jobs),
                want=want, max_step=max_step)


def _cases():
    out, k = [], 0
    for family in range(4):
        for sf, nhwc in PAIRS:
            tag = f"{FAMILY_NAMES[family]}_{sf}_{'nhwc' if nhwc else 'nchw'}"
            if family == ROI:
                host, dev = (ROI_FRAME, ROI_HOST_DST, ROI_HOST), (ROI_FRAME, ROI_DEV_DST, ROI_DEV)
            elif family == LETTERBOX:
                host, dev = (ROI_FRAME, LB_DST, LB_HOST), (ROI_FRAME, LB_DST, ROI_DEV)
            elif family == WARP:
                host, dev = (WARP_HOST_FRAME, WARP_HOST_DST, WARP_HOST), (WARP_DEV_FRAME, WARP_DEV_DST, WARP_DEV)
            else:
                host, dev = (WARP_HOST_FRAME, WARP_HOST_DST, PERSP_HOST), (WARP_DEV_FRAME, WARP_DEV_DST, PERSP_DEV)
            out.append(_row(tag + "_host", family, False, sf, nhwc, k % 3, *host, want="STS"))
            # device rows: the hint (the two warps) on every second pair, the knob on the channels-last P10 pair
            out.append(_row(tag + "_dev", family, True, sf, nhwc, (k + 1) % 3, *dev, knob=9 if (sf, nhwc) == ("P10", True) else 0,
                            max_step=2.0 if family >= WARP and not nhwc else 0.0))
            k += 1
    out.append(_row("persp_horizon", PERSP, False, "NV12", False, 0, (64, 32), (16, 16), [HORIZON], want="S"))
    out.append(_row("persp_horizon_nhwc", PERSP, False, "YUV420", True, 1, (64, 32), (16, 16), [HORIZON], want="S"))
    out.append(_row("roi_host_64x32", ROI, False, "NV12", True, 0, ROI_FRAME, ROI_DEV_DST, ROI_DEV, want="SSS"))
    out.append(_row("roi_knob9_host", ROI, False, "NV12", False, 2, ROI_FRAME, ROI_HOST_DST, ROI_HOST, want="TTT", knob=9))
    # one job more than a table holds: the second table of ONE job is seen (vpf_abi.hip cuts the call)
    out.append(_row("roi_97", ROI, False, "NV12", False, 0, ROI_FRAME, ROI_HOST_DST, [ROI_HOST[i % 3] for i in range(97)], want="".join("STS"[i % 3] for i in range(97))))
    out.append(_row("letterbox_83", LETTERBOX, False, "NV12", False, 0, ROI_FRAME, LB_DST, [LB_HOST[(i + 1) % 3] for i in range(83)],
                    want="".join("STS"[(i + 1) % 3] for i in range(83))))
    return out


def labels(row):
    """the labels the selection log shows for a row, in launch order, as the row CLAIMS them (tests/test_job_plan_cpu.py holds them against the plan):
    per job table of the family's cap the staged dispatch, then the per-tap one; a device row: its one dispatch"""
    stem = ("k_roi", "k_lb", "k_warp", "k_persp")[row["family"]]
    targs = "<%d, %d>" % (SRC_FC[row["sf"]], 8 if row["nhwc"] else 6)
    if row["dev"]:
        return ["(%s_dev%s)" % (stem, targs)]
    cap, out = CAPS[row["family"]], []
    for b in range(0, len(row["want"]), cap):
        table = row["want"][b:b + cap]
        out += ["(%s_%s%s)" % (stem, form, targs) for form, c in (("strip", "S"), ("gather", "T")) if c in table]
    return out


CASES = _cases()
