"""The case generator of the seeded differential fuzz of the fused tensor entries (tests/test_gpu_tensor_fuzz.py), importable without a GPU:
tests/test_tensor_fuzz_cases_cpu.py checks, on the CPU, that it is deterministic, emits only calls the library accepts, reaches both kernel forms
of every entry that has two, and that the composed FP32 ground truth stays within 2 codes of the same composition in the oracle's EXACT mode.

One function per entry family.  Each takes np.random.default_rng(BASE[family] + seed) and returns the plain description of ONE call — a dict of
ints, floats, strings and lists, printable in one line, reproducible from (seed, case index) alone: cases(family, seed) draws the
CASES_PER_SEED[family] calls of a seed one after the other from the same generator.

What is drawn PER JOB and not per call: the frame the job reads, its geometry, and the layout of its destination planes (LAYOUT_KINDS) — all jobs of
a host-table call sit in one canary-filled buffer at differing row pitches and base alignments (job_geo / pack).  The device-table entries have one
destination and a job stride, so their stride and base are drawn instead (dev_geo).

Ten families: whole, rois, rois_dev, letterbox, warp, warp_dev, encode, persp, and the two youngest entries — letterbox_aa
(vpf_convert_letterbox_tensor_aa: the letterbox family's draws under a per-call class, so that the 64 x 16 tile, the 32 x 8 tile and the per-tap
dispatch of csrc/vpf_aa_plan.h all occur) and remap (vpf_convert_remap_tensor: a job names its map pair by kind, parameters and seed, and maps_of
builds the coordinates on the host).  A family has a BASE of its own and shares no generator state with another: adding one changes no case of
the others."""
import math

import numpy as np

from test_letterbox_tensor_cpu import fit_reference
from test_persp_tensor_cpu import NAMED

F = np.float32
FAMILIES = ("whole", "rois", "rois_dev", "letterbox", "warp", "warp_dev", "encode", "persp", "letterbox_aa", "remap")
BASE = {"whole": 21000, "rois": 23000, "rois_dev": 25000, "letterbox": 27000, "warp": 29000, "warp_dev": 31000, "encode": 33000, "persp": 35000,
        "letterbox_aa": 37000, "remap": 39000}
CASES_PER_SEED = {"whole": 4, "rois": 5, "rois_dev": 5, "letterbox": 5, "warp": 5, "warp_dev": 5, "encode": 6, "persp": 5, "letterbox_aa": 5, "remap": 5}
# jobs per job table (kRoiBatch, kWarpBatch, kLetterboxBatch, kPerspBatch, kRemapBatch of csrc/vpf_internal.h and csrc/vpf_classes.h)
TABLE = {"rois": 96, "warp": 96, "letterbox": 82, "persp": 82, "letterbox_aa": 82, "remap": 96}
OVER_TABLE = {"rois": (97, 110), "warp": (97, 110), "letterbox": (83, 90), "persp": (83, 90), "letterbox_aa": (83, 90), "remap": (97, 110)}
LIMIT = 16777216.0  # |matrix coefficient| limit of the warp entries (include/vpf_hip.h)
SOURCES = ("NV12", "YUV420", "P10", "P12")
PARAM_NAMES = ("imagenet", "unit", "symmetric")
ELEM = {0: 4, 1: 2, 2: 2}
LAYOUT_KINDS = ("contiguous", "off_by_one_element", "padded", "padded64")
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


def cases(family, seed):
    """the calls of one seed, in the order the GPU test runs them"""
    rng = np.random.default_rng(BASE[family] + seed)
    return [GENERATORS[family](rng) for _ in range(CASES_PER_SEED[family])]


def describe(call):
    """one line that names the whole call"""
    return repr(call)


def _i(rng, lo, hi):
    """an int in lo .. hi, both included"""
    return int(rng.integers(lo, hi + 1))


def _pick(rng, seq):
    return seq[int(rng.integers(len(seq)))]


# ------------------------------------------------------------------------------------------------ what every decode-side call draws
def draw_frame_size(rng):
    """W x H: anything from 2 x 2 to 420 x 300; wide and flat (several 256-column chunks, a unit against the right edge at every W mod 8); narrow
    and tall — every frame stays far below 1 MB"""
    k = int(rng.integers(5))
    if k == 0:
        return _i(rng, 900, 2100), _i(rng, 2, 40)
    if k == 1:
        return _i(rng, 2, 24), _i(rng, 150, 500)
    return _i(rng, 2, 420), _i(rng, 2, 300)


def draw_dst_size(rng):
    """dw x dh: small; a second and third 256-column chunk; multiples of 4 wide with band edges at 16 rows; scalar tails only"""
    k = int(rng.integers(6))
    if k == 0:
        return _i(rng, 250, 530), _i(rng, 1, 24)
    if k == 1:
        return 4 * _i(rng, 1, 30), _i(rng, 15, 50)
    if k == 2:
        return _i(rng, 1, 5), _i(rng, 1, 70)
    return _i(rng, 1, 90), _i(rng, 1, 70)


def draw_common(rng, entry):
    sf = _pick(rng, SOURCES)
    W, H = draw_frame_size(rng)
    call = dict(entry=entry, sf=sf, cs=_i(rng, 0, 1), cr=_i(rng, 0, 1), W=W, H=H, dtype=_i(rng, 0, 2), bgr=bool(rng.integers(2)), nhwc=bool(rng.integers(2)),
                params=_pick(rng, PARAM_NAMES), tune=0 if rng.integers(5) else 9)
    # source pitches: rows padded to 64 B plus an odd remainder (rows start at every alignment; 16-bit samples: 2-B aligned) or unpadded
    call["frames"] = [dict(seed=_i(rng, 0, (1 << 30) - 1), align=64, extra=2 if sf in ("P10", "P12") else 3) if rng.integers(2) else
                      dict(seed=_i(rng, 0, (1 << 30) - 1), align=1, extra=0) for _ in range(_i(rng, 2, 3))]
    return call


def settle_sources(call):
    """once W x H is final: the planted 16-bit frames (tests/test_p16_tensor_cpu.py::plant) need seven luma samples and seven chroma pairs, so a
    smaller frame takes the 8-bit format instead; padded 16-bit rows stay 2-B aligned"""
    if call["sf"] in ("P10", "P12") and ((call["W"] + 1) // 2) * ((call["H"] + 1) // 2) < 7:
        call["sf"] = {"P10": "NV12", "P12": "YUV420"}[call["sf"]]
    for f in call["frames"]:
        if f["align"] == 64:
            f["extra"] = 2 if call["sf"] in ("P10", "P12") else 3
    return call


def job_geo(kind, dw, dh, e, nhwc):
    """one job's planes inside a part of its own: TensorBuf / NhwcBuf keywords (n = 1) and the part's size in bytes, a multiple of 256 so that the
    next part starts as aligned as the buffer"""
    rb = (3 if nhwc else 1) * dw * e
    if kind == "contiguous":
        row, gap, lead = rb, 0, 256
    elif kind == "off_by_one_element":
        row, gap, lead = rb, 0, 256 + e
    elif kind == "padded":          # rows padded by 16 B + 1 element: no row but the first is vector aligned
        row, gap, lead = rb + 16 + e, 40 * e, 24 * e
    else:                           # rows padded to the next 64 B and 64 B more
        row, gap, lead = (rb + 63) // 64 * 64 + 64, 64, 512
    body = lead + (dh - 1) * row + rb + (0 if nhwc else 2 * (dh * row + gap))
    tail = 64 + (-(body + 64)) % 256
    geo = dict(kind=kind, lead=lead, row=row, tail=tail, size=body + tail)
    if not nhwc:
        geo["plane"] = dh * row + gap
    return geo


def pack(call, kinds):
    """lay the jobs' parts one after the other: job i's part starts at jobs[i]["layout"]["off"]"""
    off = 0
    for job, kind in zip(call["jobs"], kinds):
        geo = job_geo(kind, call["dw"], call["dh"], ELEM[call["dtype"]], call["nhwc"])
        geo["off"] = off
        off += geo["size"]
        job["layout"] = geo
    call["size"] = off
    return call


def plane_offsets(call, job):
    """[(byte offset from the buffer's base, pitch)] of the job's planes: what the alignment rules of include/vpf_hip.h speak about"""
    g = job["layout"]
    if call["nhwc"]:
        return [(g["off"] + g["lead"], g["row"])]
    return [(g["off"] + g["lead"] + c * g["plane"], g["row"]) for c in range(3)]


def dev_geo(rng, n, dw, dh, e, nhwc):
    """the ONE destination of a device-table call: TensorBuf / NhwcBuf keywords for n jobs, the job stride (`frame`) and the base (`lead`) drawn"""
    geo = job_geo(_pick(rng, LAYOUT_KINDS), dw, dh, e, nhwc)
    out = dict(kind=geo["kind"], lead=geo["lead"], row=geo["row"])
    if nhwc:
        out["frame"] = dh * geo["row"] + e * (_i(rng, 0, 40) if rng.integers(2) else 0)
    else:
        out["plane"] = geo["plane"]
        out["frame"] = 3 * geo["plane"] + e * (_i(rng, 0, 40) if rng.integers(2) else 0)
    return out


def draw_job_count(rng, entry):
    """mostly 1 .. 12; one call in eight crosses the job table"""
    if rng.integers(8) == 0:
        return _i(rng, *OVER_TABLE[entry]), True
    return _i(rng, 1, 12), False


# ------------------------------------------------------------------------------------------------ rectangles
def draw_rect(rng, W, H, dw, dh):
    """(x, y, w, h) inside W x H: the whole frame, 1 .. 4 px sides, touching the right / bottom edge, arbitrary at odd offsets, a large down-scale of
    dw x dh (the per-tap job class), the identity scale"""
    k = int(rng.integers(7))
    if k == 0:
        return (0, 0, W, H)
    if k == 1:
        w, h = _i(rng, 1, min(4, W)), _i(rng, 1, min(4, H))
    elif k == 4 or k == 5:
        w, h = _i(rng, min(W, 3 * dw), W), _i(rng, min(H, 2 * dh), H)
    elif k == 6:
        w, h = min(W, dw), min(H, dh)
    else:
        w, h = _i(rng, 1, W), _i(rng, 1, H)
    x, y = _i(rng, 0, W - w), _i(rng, 0, H - h)
    if k == 2:
        edge = int(rng.integers(3))
        x = W - w if edge != 1 else x
        y = H - h if edge != 0 else y
    elif k == 3:
        x, y = min(x | 1, W - w), min(y | 1, H - h)
    return (x, y, w, h)


def draw_inner(rng, w, h, dw, dh):
    """(ix, iy, iw, ih) inside dw x dh for a w x h rectangle: vpf_letterbox_fit's own answer, one pixel, the whole destination, an odd ix, anything"""
    k = int(rng.integers(6))
    if k <= 1:
        return tuple(fit_reference(w, h, dw, dh))
    if k == 2:
        return (_i(rng, 0, dw - 1), _i(rng, 0, dh - 1), 1, 1)
    if k == 3:
        return (0, 0, dw, dh)
    iw, ih = _i(rng, 1, dw), _i(rng, 1, dh)
    ix, iy = _i(rng, 0, dw - iw), _i(rng, 0, dh - ih)
    if k == 4:
        ix = min(ix | 1, dw - iw)
    return (ix, iy, iw, ih)


def roi_case(rng, entry="rois"):
    call = draw_common(rng, entry)
    n, over = draw_job_count(rng, entry)
    call["dw"], call["dh"] = (_i(rng, 1, 24), _i(rng, 1, 16)) if over else draw_dst_size(rng)
    call["jobs"] = [dict(frame=_i(rng, 0, len(call["frames"]) - 1), rect=draw_rect(rng, call["W"], call["H"], call["dw"], call["dh"])) for _ in range(n)]
    if entry == "letterbox":
        call["pad"] = (_i(rng, 0, 255), _i(rng, 0, 255), _i(rng, 0, 255))
        for job in call["jobs"]:
            job["dst_rect"] = draw_inner(rng, job["rect"][2], job["rect"][3], call["dw"], call["dh"])
    return pack(settle_sources(call), [_pick(rng, LAYOUT_KINDS) for _ in range(n)])


def letterbox_case(rng):
    return roi_case(rng, "letterbox")


# ------------------------------------------------------------------------------------------------ the antialiased letterbox
# what a call's jobs are held to (the per-call class draw), so that all three dispatch kinds of csrc/vpf_aa_plan.h occur:
#   mild   every job within about 0.4 .. 3 x per axis, up-scales included: the staged dispatch takes the 64 x 16 tile
#   steep  one job or more between 3.6 x and 6.5 x on BOTH axes on a picture of at least 32 x 8, and none steeper: the 32 x 8 tile
#   any    unrestricted: thumbnails (1 x 1 and 2 x 2 pictures) of large rectangles, which sample per tap, next to small rectangles at large factors,
#          which still stage
AA_CLASSES = ("mild", "steep", "steep", "any", "any", "any")
AA_MILD, AA_STEEP_LO, AA_STEEP_HI = 3.0, 3.6, 6.5


def cap_factor(rect, W, H, iw, ih, top):
    """the rectangle shrunk until neither axis is more than `top` times its picture; an edge that touched the frame's right / bottom edge still does"""
    x, y, w, h = rect
    nw, nh = min(w, max(1, int(top * iw))), min(h, max(1, int(top * ih)))
    return (W - nw if x + w == W else x, H - nh if y + h == H else y, nw, nh)


def letterbox_aa_case(rng):
    """vpf_convert_letterbox_tensor_aa: roi_case(rng, "letterbox") with the class draw above.  A steep call takes a frame of at least 240 x 120 and
    a destination of at least 40 x 12 (32 x 8 across the job table) so that its steep jobs exist"""
    call = draw_common(rng, "letterbox_aa")
    cls = _pick(rng, AA_CLASSES)
    n, over = draw_job_count(rng, "letterbox_aa")
    if cls == "steep":
        call["W"], call["H"] = _i(rng, 240, 420), _i(rng, 120, 300)
        call["dw"], call["dh"] = (_i(rng, 32, 40), _i(rng, 8, 16)) if over else (_i(rng, 40, 90), _i(rng, 12, 70))
    else:
        call["dw"], call["dh"] = (_i(rng, 1, 24), _i(rng, 1, 16)) if over else draw_dst_size(rng)
    call["cls"] = cls
    call["pad"] = (_i(rng, 0, 255), _i(rng, 0, 255), _i(rng, 0, 255))
    W, H, dw, dh = call["W"], call["H"], call["dw"], call["dh"]
    hot = _i(rng, 0, n - 1)   # the job a steep call is steep by
    call["jobs"] = []
    for i in range(n):
        job = dict(frame=_i(rng, 0, len(call["frames"]) - 1))
        if cls == "any" and rng.integers(2) == 0:        # a thumbnail of a large rectangle
            w, h = _i(rng, (W + 1) // 2, W), _i(rng, (H + 1) // 2, H)
            iw, ih = _i(rng, 1, min(2, dw)), _i(rng, 1, min(2, dh))
            job["rect"] = (_i(rng, 0, W - w), _i(rng, 0, H - h), w, h)
            job["dst_rect"] = (_i(rng, 0, dw - iw), _i(rng, 0, dh - ih), iw, ih)
        elif cls == "steep" and (i == hot or rng.integers(4) == 0):
            iw, ih = _i(rng, 32, min(dw, int(W / 3.7))), _i(rng, 8, min(dh, int(H / 3.7)))
            w = min(max(int(iw * rng.uniform(AA_STEEP_LO, AA_STEEP_HI)), math.ceil(AA_STEEP_LO * iw)), int(AA_STEEP_HI * iw), W)
            h = min(max(int(ih * rng.uniform(AA_STEEP_LO, AA_STEEP_HI)), math.ceil(AA_STEEP_LO * ih)), int(AA_STEEP_HI * ih), H)
            job["rect"] = (_i(rng, 0, W - w), _i(rng, 0, H - h), w, h)
            job["dst_rect"] = (_i(rng, 0, dw - iw), _i(rng, 0, dh - ih), iw, ih)
        else:
            rect = draw_rect(rng, W, H, dw, dh)
            job["dst_rect"] = draw_inner(rng, rect[2], rect[3], dw, dh)
            job["rect"] = rect if cls == "any" else cap_factor(rect, W, H, job["dst_rect"][2], job["dst_rect"][3], AA_MILD if cls == "mild" else AA_STEEP_HI)
        call["jobs"].append(job)
    return pack(settle_sources(call), [_pick(rng, LAYOUT_KINDS) for _ in range(n)])


def box_valid(f, x, y, w, h, n_frames, W, H):
    """the header's rule for a device box, in Python's exact integers"""
    return 0 <= f < n_frames and w >= 1 and h >= 1 and x >= 0 and y >= 0 and x + w <= W and y + h <= H


def draw_count(rng, max_n):
    """None (all of max_n), below, at and above max_n"""
    k = int(rng.integers(5))
    if k <= 1:
        return None
    return (_i(rng, 0, max_n - 1), max_n, max_n + _i(rng, 1, 5))[k - 2]


def rois_dev_case(rng):
    call = draw_common(rng, "rois_dev")
    W, H = call["W"], call["H"]
    n = _i(rng, 1, 14)
    call["dw"], call["dh"] = draw_dst_size(rng)
    nf = len(call["frames"])
    boxes = [(_i(rng, 0, nf - 1),) + draw_rect(rng, W, H, call["dw"], call["dh"]) for _ in range(n)]
    # a few entries the header defines as invalid (the spellings of tests/test_gpu_rois_dev.py::test_invalid_boxes_are_zero_filled): zero fill
    bad = [(1, 3, 5, 0, 10), (0, 3, 5, 20, -3), (0, -1, 5, 2, 2), (1, W - 1, 0, 2, 1), (0, 0, H - 1, 1, 2), (-1, 0, 0, 1, 1), (nf, 0, 0, 1, 1),
           (0, INT_MAX, 0, INT_MAX, 1), (0, 0, INT_MIN, 1, 1), (0, 1, 1, INT_MIN, 2), (0, 0, 0, W + 1, H)]
    for _ in range(int(rng.integers(3)) if n > 1 else 0):
        boxes[_i(rng, 0, n - 1)] = _pick(rng, bad)
    call["boxes"] = boxes
    call["valid"] = [box_valid(*b, nf, W, H) for b in boxes]
    call["box_ints"] = _pick(rng, (5, 5, 6, 8, 9))  # the box stride in int32s; the padding holds a pattern the kernel must not read
    call["max_n"] = n
    call["count"] = draw_count(rng, n)
    call["geo"] = dev_geo(rng, n, call["dw"], call["dh"], ELEM[call["dtype"]], call["nhwc"])
    return settle_sources(call)


# ------------------------------------------------------------------------------------------------ matrices
def f32(v):
    return float(F(v))


def centred(a, b, c, d, W, H, dw, dh, tx=0.0, ty=0.0):
    """the matrix with linear part (a b; c d) that takes the destination's centre to the frame's centre, moved by (tx, ty)"""
    cx, cy, ex, ey = (W - 1) / 2.0, (H - 1) / 2.0, (dw - 1) / 2.0, (dh - 1) / 2.0
    return tuple(f32(v) for v in (a, b, cx - (a * ex + b * ey) + tx, c, d, cy - (c * ex + d * ey) + ty))


def draw_matrix(rng, W, H, dw, dh, steep=False):
    """identity plus integer / half-integer translations, the four right angles, rotations at scales 0.3 .. 9, shear, a zero row, wholly outside, and
    — `steep` — 5 .. 9 x down-scales (windows that outgrow the staged form); the interesting ones centred on the frame"""
    k = 7 if steep and rng.integers(4) else int(rng.integers(8))
    if k == 0:
        return tuple(f32(v) for v in (1, 0, _i(rng, -3, max(W - dw + 3, -3)), 0, 1, _i(rng, -3, max(H - dh + 3, -3))))
    if k == 1:
        return tuple(f32(v) for v in (1, 0, _i(rng, -3, max(W - dw + 3, -3)) + 0.5, 0, 1, _i(rng, -3, max(H - dh + 3, -3)) + 0.5))
    if k == 2:
        a, b = ((1, 0), (0, -1), (-1, 0), (0, 1))[int(rng.integers(4))]
        return centred(a, b, -b, a, W, H, dw, dh, _i(rng, -2, 2), _i(rng, -2, 2))
    if k == 3:
        t, s = rng.uniform(0, 2 * math.pi), math.exp(rng.uniform(math.log(0.3), math.log(9.0)))
        return centred(s * math.cos(t), -s * math.sin(t), s * math.sin(t), s * math.cos(t), W, H, dw, dh, rng.uniform(-4, 4), rng.uniform(-4, 4))
    if k == 4:
        return centred(1, rng.uniform(-0.6, 0.6), rng.uniform(-0.6, 0.6), 1, W, H, dw, dh)
    if k == 5:
        z = int(rng.integers(3))
        a, b, c, d = (0, 0, rng.uniform(-1, 1), 1) if z == 0 else (1, rng.uniform(-1, 1), 0, 0) if z == 1 else (0, 0, 0, 0)
        m = centred(a, b, c, d, W, H, dw, dh)
        return tuple(f32(v) for v in (m[0], m[1], rng.uniform(0, W - 1) if z != 1 else m[2], m[3], m[4], rng.uniform(0, H - 1) if z != 0 else m[5]))
    if k == 6:
        far = _pick(rng, (500.0 + W, -700.0 - dw, 3.0e6, -LIMIT))
        return tuple(f32(v) for v in ((1, 0, far, 0, 1, 0) if rng.integers(2) else (1, 0, 0, 0, 1, far)))
    sx, sy = rng.uniform(5, 9), rng.uniform(5, 9)
    t = rng.uniform(-0.2, 0.2) if rng.integers(2) else 0.0
    return centred(sx * math.cos(t), -sy * math.sin(t), sx * math.sin(t), sy * math.cos(t), W, H, dw, dh)


def draw_warp_shape(rng, call):
    """the destination of a warp call; one call in four is the steep family: a frame of at least 200 x 200 and a destination of whole 32 x 32
    tiles, so that a 5 .. 9 x down-scale's tile window outgrows the staged form's 64 KiB (on smaller frames no window does)"""
    steep = rng.integers(4) == 0
    if steep:
        call["W"], call["H"] = _i(rng, 200, 420), _i(rng, 200, 300)
        call["dw"], call["dh"] = _i(rng, 32, 90), _i(rng, 32, 70)
    else:
        call["dw"], call["dh"] = draw_dst_size(rng)
    return bool(steep)


def warp_case(rng):
    call = draw_common(rng, "warp")
    steep = draw_warp_shape(rng, call)
    n, over = draw_job_count(rng, "warp")
    if over:
        call["dw"], call["dh"] = (_i(rng, 32, 40), _i(rng, 32, 36)) if steep else (_i(rng, 1, 24), _i(rng, 1, 16))
    call["mode"] = _i(rng, 0, 1)
    call["border"] = (_i(rng, 0, 255), _i(rng, 0, 255), _i(rng, 0, 255))
    call["jobs"] = [dict(frame=_i(rng, 0, len(call["frames"]) - 1), m=draw_matrix(rng, call["W"], call["H"], call["dw"], call["dh"], steep)) for _ in range(n)]
    return pack(settle_sources(call), [_pick(rng, LAYOUT_KINDS) for _ in range(n)])


def matrix_valid(f, m, n_frames):
    return 0 <= f < n_frames and all(abs(v) <= LIMIT for v in m)  # (NaN fails the comparison)


def warp_dev_case(rng):
    call = draw_common(rng, "warp_dev")
    steep = draw_warp_shape(rng, call)
    W, H, dw, dh = call["W"], call["H"], call["dw"], call["dh"]
    n = _i(rng, 1, 14)
    nf = len(call["frames"])
    call["mode"] = _i(rng, 0, 1)
    call["border"] = (_i(rng, 0, 255), _i(rng, 0, 255), _i(rng, 0, 255))
    rows = [(_i(rng, 0, nf - 1), draw_matrix(rng, W, H, dw, dh, steep)) for _ in range(n)]
    # a few entries the header defines as invalid (the spellings of tests/test_gpu_warps_dev.py::test_invalid_entries_take_the_border): the border
    nan, inf, above = math.nan, math.inf, float(np.nextafter(F(LIMIT), F(np.inf)))
    bad = [(1, (nan, 0, 33, 0, 1, 5)), (0, (1, inf, 33, 0, 1, 5)), (0, (1, 0, -inf, 0, 1, 5)), (1, (1, 0, 33, above, 1, 5)), (1, (1, 0, 33, 0, -above, 5)),
           (-1, (1, 0, 3, 0, 1, 5)), (nf, (1, 0, 3, 0, 1, 5)), (1, (1, 0, 33, 0, 1, nan)), (INT_MIN, (1, 0, 3, 0, 1, 5)), (INT_MAX, (1, 0, 3, 0, 1, 5)), (0, (nan,) * 6)]
    for _ in range(int(rng.integers(3)) if n > 1 else 0):
        f, m = _pick(rng, bad)
        rows[_i(rng, 0, n - 1)] = (f, tuple(float(v) for v in m))
    call["index"] = [f for f, _ in rows]
    call["mats"] = [m for _, m in rows]
    call["valid"] = [matrix_valid(f, m, nf) for f, m in rows]
    call["mat_floats"] = _pick(rng, (6, 6, 7, 8, 10))   # the matrix stride in floats; the padding holds NaNs the kernel must not read
    call["index_ints"] = _pick(rng, (1, 1, 2, 5))       # the frame-index stride in int32s; the gaps name a frame that does not exist
    call["max_n"] = n
    call["count"] = draw_count(rng, n)
    # the LDS hint: none, or a true bound of the valid matrices (never a correctness input, so it is never drawn short)
    steps = [max(abs(m[0]) + abs(m[1]), abs(m[3]) + abs(m[4])) for m, ok in zip(call["mats"], call["valid"]) if ok]
    call["max_step"] = 0.0 if rng.integers(2) or not steps else f32(max(steps) * rng.uniform(1.0, 1.5) + 1e-3)
    call["geo"] = dev_geo(rng, n, dw, dh, ELEM[call["dtype"]], call["nhwc"])
    return settle_sources(call)


# ------------------------------------------------------------------------------------------------ homographies
# the classes draw_homography draws from, with their weights in a mixed call.  "behind" (no pixel has w > 0: a job whose strip need is 0 bytes)
# and "degenerate" (w > 0 but tiny, or a signed zero) are apart so that a call of ONE class can be a table whose staged dispatch gets no LDS.
PERSP_CLASSES = ("lifted", "moderate", "steep", "horizon", "behind", "degenerate", "outside", "cancelling", "sawtooth")
PERSP_WEIGHTS = (3, 4, 1, 3, 1, 1, 2, 3, 1)
# what a call of one class picks from: the two classes that make a dispatch no mixed call has (0 bytes of LDS; per-tap jobs only) come up more often
PERSP_ONLY = ("behind", "behind", "behind", "steep", "steep", "lifted", "moderate", "horizon", "degenerate", "outside", "cancelling", "sawtooth")
PERSP_MIX = tuple(c for c, w in zip(PERSP_CLASSES, PERSP_WEIGHTS) for _ in range(w))
SAWTOOTH, SAWTOOTH_SHAPE = NAMED["sawtooth"][0], (131, 79, 33, 33)  # the named matrix and the shape it was found for (W, H, dw, dh)


def nine(m):
    """nine float32 values within the entry's limit"""
    return tuple(f32(min(max(float(v), -LIMIT), LIMIT)) for v in m)


def _sign(rng):
    return 1 - 2 * int(rng.integers(2))


def _log_uniform(rng, lo, hi):
    return math.exp(rng.uniform(math.log(lo), math.log(hi)))


def moderate_homography(rng, W, H, dw, dh):
    """tests/test_persp_bounds_cpu.py::moderate on the call's own sizes: rotation x scale 0.3 .. 3 x shear about a point of the frame, a perspective
    row that keeps w within [0.4, 1.6] x m22 over the destination, the whole matrix times 0.25 .. 4"""
    th, s = rng.uniform(0, 2 * math.pi), _log_uniform(rng, 0.3, 3.0)
    a, b, c, d = s * math.cos(th), -s * math.sin(th) + rng.uniform(-0.2, 0.2), s * math.sin(th), s * math.cos(th) * rng.uniform(0.8, 1.25)
    cx, cy = rng.uniform(-0.1 * W, 1.1 * W), rng.uniform(-0.1 * H, 1.1 * H)
    tx, ty = cx - a * (dw - 1) / 2 - b * (dh - 1) / 2, cy - c * (dw - 1) / 2 - d * (dh - 1) / 2
    budget, split = rng.uniform(0, 0.6), rng.uniform(0, 1)
    p, q = _sign(rng) * budget * split / max(dw - 1, 1), _sign(rng) * budget * (1 - split) / max(dh - 1, 1)
    g = _log_uniform(rng, 0.25, 4.0)
    return [g * v for v in (a, b, tx, c, d, ty, p, q, 1.0)]


def cancelling_homography(rng, W, H, dw, dh):
    """classes 0 .. 5 of tests/test_persp_bounds_cpu.py::adversarial: coefficients up to 2^24 whose offsets cancel them somewhere inside the
    destination, in the numerators, the denominator or all three"""
    def big():
        return _sign(rng) * _log_uniform(rng, 1e3, 2.0 ** 24)

    cls = int(rng.integers(6))
    x0, y0 = rng.uniform(0, dw), rng.uniform(0, dh)
    m = [1.0, 0.0, rng.uniform(0, W), 0.0, 1.0, rng.uniform(0, H), 0.0, 0.0, 1.0]
    if cls in (0, 3, 5):
        g = big()
        m[0], m[2] = g, -g * x0 + rng.uniform(0, W)
    if cls in (1, 3, 5):
        g = big()
        m[4], m[5] = g, -g * y0 + rng.uniform(0, H)
    if cls in (2, 5):
        g = big()
        m[6], m[8] = g, -g * x0 + rng.uniform(0.5, 2)
    if cls == 4:
        g, q = abs(big()), abs(big())
        m = [g * rng.uniform(0.5, 2), g * rng.uniform(-0.2, 0.2), g * rng.uniform(0, W), g * rng.uniform(-0.2, 0.2), g * rng.uniform(0.5, 2), g * rng.uniform(0, H),
             q * rng.uniform(0, 0.01), q * rng.uniform(0, 0.01), q]
        s = max(abs(v) for v in m) / 2.0 ** 24
        if s > 1:
            m = [v / s for v in m]
    return m


def draw_homography(rng, W, H, dw, dh, steep=False, cls=None):
    """nine coefficients of the class `cls` (drawn by PERSP_WEIGHTS when None):
    lifted      the affine family's matrices with the last row (0, 0, 1)
    moderate    moderate_homography
    steep       5 .. 9 x down-scales with a small perspective row (on a frame of 200 x 200 and more the tile window outgrows the staged form)
    horizon     w changes sign inside the destination, along dx, dy or both; one in three in powers of two, w exactly 0 on a column, row or diagonal
    behind      no pixel has w > 0: w < 0 everywhere, the last row all zero, m22 = -0.0
    degenerate  w > 0 but denormal (coordinates of +-inf) or 1e-30 (finite coordinates above 1e29); w = m20 dx - 0.0: exactly 0 on column 0
    outside     w > 0 everywhere, the footprint wholly beside the frame
    cancelling  cancelling_homography
    sawtooth    class 6 of adversarial: nx cancels on the destination's last row and sx is a sawtooth along it (the kernel's per-pixel fallback)"""
    if cls is None:
        cls = _pick(rng, PERSP_MIX)
    if cls == "lifted":
        return nine(draw_matrix(rng, W, H, dw, dh, steep) + (0.0, 0.0, 1.0))
    if cls == "moderate":
        return nine(moderate_homography(rng, W, H, dw, dh))
    if cls == "steep":
        sx, sy, t = rng.uniform(5, 9), rng.uniform(5, 9), rng.uniform(-0.2, 0.2) if rng.integers(2) else 0.0
        p, q = _sign(rng) * rng.uniform(0, 0.05) / max(dw - 1, 1), _sign(rng) * rng.uniform(0, 0.05) / max(dh - 1, 1)
        return nine(centred(sx * math.cos(t), -sy * math.sin(t), sx * math.sin(t), sy * math.cos(t), W, H, dw, dh) + (p, q, 1.0))
    if cls == "horizon":
        ux, uy = ((1, 0), (0, 1), (1, 1))[int(rng.integers(3))]
        T, sg = ux * (dw - 1) + uy * (dh - 1), _sign(rng)
        if rng.integers(3) == 0:   # exact: w = +-2^-k (t - t0) with t = ux dx + uy dy and t0 a whole number
            s, t0 = 2.0 ** -_i(rng, 3, 7), float(_i(rng, 0, T))
        else:
            s, t0 = rng.uniform(0.5, 2.0) / max(T, 1), rng.uniform(0, T)
        return nine(draw_matrix(rng, W, H, dw, dh, steep) + (sg * s * ux, sg * s * uy, -sg * s * t0))
    if cls == "behind":
        k = int(rng.integers(3))
        row = (-rng.uniform(0, 0.01), -rng.uniform(0, 0.01), -rng.uniform(0.5, 2)) if k == 0 else (0.0, 0.0, 0.0) if k == 1 else (0.0, 0.0, -0.0)
        return nine(draw_matrix(rng, W, H, dw, dh) + row)
    if cls == "degenerate":
        k = int(rng.integers(4))
        if k == 0:   # denormal w: +-inf by the sign of the numerators
            return nine(draw_matrix(rng, W, H, dw, dh) + (0.0, 0.0, 1e-40))
        if k == 1:   # denormal w that grows along dx from the smallest denormal
            return nine((1.0, 0.0, _i(rng, -3, 3), 0.0, _sign(rng), _i(rng, -3, 3), 1e-45, 0.0, 1e-45))
        if k == 2:   # `huge`: finite coordinates above 1e29
            return nine((1.0, 0.0, _i(rng, 1, 50), 0.0, 1.0, _i(rng, 1, 50), 0.0, 0.0, 1e-30))
        return nine(draw_matrix(rng, W, H, dw, dh) + (rng.uniform(0.01, 0.1), 0.0, -0.0))
    if cls == "outside":
        m = moderate_homography(rng, W, H, dw, dh)
        axis = int(rng.integers(2))
        far = _sign(rng) * ((2 * (W, H)[axis] + 10 * (dw + dh) + 500) if rng.integers(3) else 3.0e6)   # sx (sy) moves by `far`: nx += far w
        for k in range(3):
            m[3 * axis + k] += far * m[6 + k]
        return nine(m)
    if cls == "cancelling":
        return nine(cancelling_homography(rng, W, H, dw, dh))
    assert cls == "sawtooth"
    g = _sign(rng) * _log_uniform(rng, 1e4, 2.0 ** 24 / max(dh, 2))
    return nine((rng.uniform(0.05, 0.9), g, -g * (dh - 1) + rng.uniform(2, 80), 0.0, 0.0, rng.uniform(1, 3), rng.uniform(1e-4, 3e-3), 0.0, rng.uniform(0.04, 0.1)))


def persp_case(rng):
    """vpf_convert_persp_tensor: warp_case with nine-coefficient matrices.  One call in sixteen draws all of its jobs from ONE class (a call of steep
    jobs takes the steep shape); one in ten of the others is a sawtooth call: the shape the named sawtooth matrix was found for, or a destination of
    33 / 65 rows, with that matrix and fresh draws of its class among jobs of every class"""
    call = draw_common(rng, "persp")
    only = _pick(rng, PERSP_ONLY) if rng.integers(16) == 0 else None
    steep = draw_warp_shape(rng, call)
    if only == "steep" and not steep:
        steep = True
        call["W"], call["H"], call["dw"], call["dh"] = _i(rng, 200, 420), _i(rng, 200, 300), _i(rng, 32, 90), _i(rng, 32, 70)
    n, over = draw_job_count(rng, "persp")
    if over:
        call["dw"], call["dh"] = (_i(rng, 32, 40), _i(rng, 32, 36)) if steep else (_i(rng, 1, 24), _i(rng, 1, 16))
    saw = not over and (only == "sawtooth" or (only is None and rng.integers(10) == 0))
    named = saw and bool(rng.integers(3))
    if named:
        call["W"], call["H"], call["dw"], call["dh"] = SAWTOOTH_SHAPE
    elif saw:
        call["W"], call["H"], call["dw"], call["dh"] = _i(rng, 100, 420), _i(rng, 80, 300), _i(rng, 20, 90), _pick(rng, (33, 65))
    call["mode"] = _i(rng, 0, 1)
    call["border"] = (_i(rng, 0, 255), _i(rng, 0, 255), _i(rng, 0, 255))
    W, H, dw, dh = call["W"], call["H"], call["dw"], call["dh"]
    call["jobs"] = []
    for _ in range(n):
        cls = only if only is not None else "sawtooth" if saw and rng.integers(3) == 0 else "steep" if steep and rng.integers(3) == 0 else None
        call["jobs"].append(dict(frame=_i(rng, 0, len(call["frames"]) - 1), m=draw_homography(rng, W, H, dw, dh, steep, cls)))
    if named:
        call["jobs"][_i(rng, 0, n - 1)]["m"] = nine(SAWTOOTH)
    return pack(settle_sources(call), [_pick(rng, LAYOUT_KINDS) for _ in range(n)])


# ------------------------------------------------------------------------------------------------ per-pixel maps
# A description stays one printable line, so a job names its maps instead of holding them: call["maps"] is a list of map PAIRS — kind, parameters,
# seed, pitches and leads — and job["maps"] an index into it (two jobs may share a pair on different frames); pair_maps / maps_of build the
# coordinates on the host.  Kinds:
#   affine      draw_matrix written out by warp_maps(..., mode 0): unclamped, the kernel clamps under REPLICATE (bit for bit the affine entry)
#   homography  draw_homography through persp_maps, pixels where w > 0 fails set to NaN
#   barrel      lens undistortion (the float64 restatement of tests/test_remap_tensor_cpu.py) with drawn k1, k2
#   local       a smooth affine map plus a jitter of a few pixels: moderate windows
#   random      every pixel anywhere in [-5, W + 5] x [-5, H + 5]: the window is the whole frame
#   outside     every coordinate out of range      nan   all NaN      one   a single in-range pixel, everything else NaN or left of the frame
#   strip_*     REMAP_NAMED: tile (0, 0) spans an exact window, the rest is NaN
# Any kind may pass through sprinkle (the special coordinates of tests/test_remap_tensor_cpu.py at seeded places).
REMAP_KINDS = ("affine", "homography", "barrel", "local", "random", "outside", "nan", "one")
REMAP_WEIGHTS = (4, 3, 3, 4, 4, 3, 1, 1)
REMAP_MIX = tuple(c for c, w in zip(REMAP_KINDS, REMAP_WEIGHTS) for _ in range(w))
REMAP_SMOOTH = ("affine", "barrel", "local")   # the kinds a true max_step is taken from
# name: (W, H, x_hi, y_hi, strip bytes) — the in-range pixels of destination tile (0, 0) span frame columns 0 .. x_hi and rows 0 .. y_hi.  A strip row
# is 32 B per unit of eight columns plus 16 (warp_strip, csrc/vpf_job_bounds.h), and without a hint the launch gives 65 536 - 32 bytes:
#   strip_65504   44 units, 46 rows x 1 424 B = 65 504: exactly what the launch gives — it stages
#   strip_65520   31 units, 65 rows x 1 008 B = 65 520: the smallest strip above it (a strip is a multiple of 16 and no odd multiple gives 65 536) — per tap
REMAP_NAMED = {"strip_65504": (360, 140, 351, 45, 65504), "strip_65520": (300, 140, 247, 64, 65520)}


def pair_maps(call, pair):
    """(sx, sy): float32 [dh, dw] of one map pair of a remap call"""
    from test_remap_tensor_cpu import _undistort_numpy, sprinkle
    from test_persp_tensor_cpu import persp_maps
    from test_warp_tensor_cpu import warp_maps
    W, H, dw, dh, kind = call["W"], call["H"], call["dw"], call["dh"], pair["kind"]
    rng = np.random.default_rng(pair["seed"])
    nan = np.full((dh, dw), np.nan, F)
    if kind == "affine":
        sx, sy = warp_maps(pair["m"], dw, dh, W, H, 0)
    elif kind == "homography":
        sx, sy, front = persp_maps(pair["m"], dw, dh, W, H, 0)
        sx, sy = np.where(front, sx, F(np.nan)).astype(F), np.where(front, sy, F(np.nan)).astype(F)
    elif kind == "barrel":   # a camera whose principal point is the frame's centre, onto a dw x dh view of the whole frame
        K = [[0.8 * W, 0, (W - 1) / 2], [0, 0.8 * W, (H - 1) / 2], [0, 0, 1]]
        Kn = [[0.8 * dw, 0, (dw - 1) / 2], [0, 0.8 * W * dh / H, (dh - 1) / 2], [0, 0, 1]]
        sx, sy = _undistort_numpy(K, (pair["k1"], pair["k2"], 0.002, -0.001, 0.01), (dw, dh), Kn)
    elif kind == "local":
        sx, sy = warp_maps(pair["m"], dw, dh, W, H, 0)
        sx, sy = (sx + rng.uniform(-pair["jitter"], pair["jitter"], (dh, dw)).astype(F)).astype(F), (sy + rng.uniform(-pair["jitter"], pair["jitter"], (dh, dw)).astype(F)).astype(F)
    elif kind == "random":
        sx, sy = rng.uniform(-5, W + 5, (dh, dw)).astype(F), rng.uniform(-5, H + 5, (dh, dw)).astype(F)
    elif kind == "outside":
        sx, sy = np.full((dh, dw), pair["at"][0], F), np.full((dh, dw), pair["at"][1], F)
    elif kind == "nan":
        sx, sy = nan.copy(), nan.copy()
    elif kind == "one":
        sx, sy = np.full((dh, dw), -7.0, F), nan.copy()
        sx[:, :dw // 2] = np.nan
        k = int(rng.integers(dw * dh))
        sx.flat[k], sy.flat[k] = F(W - 1), F(rng.uniform(0, H - 1))
    else:
        _, _, x_hi, y_hi, _ = REMAP_NAMED[kind]
        sx, sy = nan.copy(), nan.copy()
        tw, th = min(dw, 32), min(dh, 32)
        sx[:th, :tw], sy[:th, :tw] = rng.uniform(0, x_hi - 0.5, (th, tw)).astype(F), rng.uniform(0, y_hi - 0.5, (th, tw)).astype(F)
        sx[:th, :tw][rng.uniform(size=(th, tw)) < 0.2] = np.nan                # (some pixels of the tile take the border)
        sx[0, 0], sy[0, 0] = 0.25, 0.5                                         # taps 0 | 1: the window's first column and row
        sx[th - 1, tw - 1], sy[th - 1, tw - 1] = x_hi - 0.5, y_hi - 0.5        # taps x_hi - 1 | x_hi: its last
    sx, sy = np.ascontiguousarray(sx, dtype=F), np.ascontiguousarray(sy, dtype=F)
    return sprinkle(sx, sy, W, H, pair["sprinkle"]) if pair["sprinkle"] is not None else (sx, sy)


def maps_of(call, job):
    return pair_maps(call, call["maps"][job["maps"]])


def maps_step(sx, sy):
    """the largest |d s / d dx| + |d s / d dy| over both maps, differences that are not finite left out (what PytorchNvCodec.maps_max_step bounds)"""
    best = 0.0
    for m in (sx.astype(np.float64), sy.astype(np.float64)):
        with np.errstate(invalid="ignore"):
            gx, gy = np.abs(np.diff(m, axis=1, append=m[:, -1:])), np.abs(np.diff(m, axis=0, append=m[-1:, :]))
        gx, gy = np.where(np.isfinite(gx), gx, 0.0), np.where(np.isfinite(gy), gy, 0.0)
        best = max(best, float((gx + gy).max()))
    return best


def draw_pair(rng, call, kind=None):
    W, H, dw, dh = call["W"], call["H"], call["dw"], call["dh"]
    kind = _pick(rng, REMAP_MIX) if kind is None else kind
    pair = dict(kind=kind, seed=_i(rng, 0, (1 << 30) - 1))
    if kind == "affine":
        pair["m"] = draw_matrix(rng, W, H, dw, dh)
    elif kind == "homography":
        pair["m"] = draw_homography(rng, W, H, dw, dh)
    elif kind == "barrel":
        pair["k1"], pair["k2"] = round(float(rng.uniform(-0.4, 0.3)), 4), round(float(rng.uniform(-0.1, 0.1)), 4)
    elif kind == "local":
        s, t = _log_uniform(rng, 0.4, 2.0), rng.uniform(0, 2 * math.pi)
        pair["m"] = centred(s * math.cos(t), -s * math.sin(t), s * math.sin(t), s * math.cos(t), W, H, dw, dh, rng.uniform(-4, 4), rng.uniform(-4, 4))
        pair["jitter"] = round(float(rng.uniform(0.5, 4.0)), 2)
    elif kind == "outside":
        pair["at"] = _pick(rng, ((-3.5, H / 2.0), (W + 0.5, -0.25), (W / 2.0, H + 2.0), (-1e30, 0.0)))
    pair["sprinkle"] = _i(rng, 0, (1 << 30) - 1) if kind not in REMAP_NAMED and rng.integers(2) else None
    # map rows padded by 0 .. 32 bytes, the bases at 0, 4, 8, 12 mod 16: both loads of remap_load4 (tests/test_gpu_remap_tensor.py::test_seeded_calls)
    pair.update(xpitch=4 * dw + 4 * _i(rng, 0, 8), ypitch=4 * dw + 4 * _i(rng, 0, 8), xlead=4 * _i(rng, 0, 3), ylead=4 * _i(rng, 0, 3))
    return pair


def remap_case(rng):
    """vpf_convert_remap_tensor: per job the frame, the map pair (a new one, or an earlier job's), the destination layout; per call the border mode,
    the border, the hint (0, 1e-3 — nothing fits —, a true bound of the smooth maps x 1 .. 1.5, 50) and 1 .. 12 jobs, or 97 .. 110 at a small
    destination.  One wide frame in three is wider than 2048 (the packed window's 16-bit halves above 2047).  About one call in ten holds a named
    map (REMAP_NAMED) on its frame, without a hint and with the knob at 0"""
    call = draw_common(rng, "remap")
    if call["W"] >= 900 and rng.integers(3) == 0:
        call["W"] = _i(rng, 2049, 2100)
    named = _pick(rng, tuple(REMAP_NAMED)) if rng.integers(10) == 0 else None
    n, over = draw_job_count(rng, "remap")
    call["dw"], call["dh"] = (_i(rng, 1, 24), _i(rng, 1, 16)) if over else draw_dst_size(rng)
    if named is not None:
        call["W"], call["H"], call["tune"] = REMAP_NAMED[named][0], REMAP_NAMED[named][1], 0
        call["dw"], call["dh"] = max(call["dw"], 2), max(call["dh"], 2)
    call["mode"] = _i(rng, 0, 1)
    call["border"] = (_i(rng, 0, 255), _i(rng, 0, 255), _i(rng, 0, 255))
    call["maps"], call["jobs"] = [], []
    for _ in range(n):
        if call["maps"] and rng.integers(4) == 0:
            k = _i(rng, 0, len(call["maps"]) - 1)
        else:
            k = len(call["maps"])
            call["maps"].append(draw_pair(rng, call))
        call["jobs"].append(dict(frame=_i(rng, 0, len(call["frames"]) - 1), maps=k))
    if named is not None:
        call["maps"][call["jobs"][_i(rng, 0, n - 1)]["maps"]] = draw_pair(rng, call, named)
    hint = int(rng.integers(4))
    call["max_step"] = (0.0, f32(1e-3), None, 50.0)[hint] if named is None else 0.0
    if call["max_step"] is None:
        steps = [maps_step(*pair_maps(call, dict(p, sprinkle=None))) for p in call["maps"] if p["kind"] in REMAP_SMOOTH]
        call["max_step"] = f32(min(max(steps) * rng.uniform(1.0, 1.5) + 1e-3, 1e6)) if steps else 0.0
    return pack(settle_sources(call), [_pick(rng, LAYOUT_KINDS) for _ in range(n)])


# ------------------------------------------------------------------------------------------------ whole frames and the way back
def whole_case(rng):
    """vpf_convert_resize_tensor(_batch): (W, H) -> (dw, dh) drawn like tests/test_gpu_parity.py::test_fuzz_resize_and_fused — a ratio of 0.15 .. 3
    per axis, one call in four an exact integer ratio per axis (2 x and 3 x among them) — and n = 1 .. 40 frames, each with a layout of its own"""
    call = draw_common(rng, "whole")
    n = _i(rng, 1, 40) if rng.integers(3) == 0 else _i(rng, 1, 6)
    W, H = call["W"], call["H"]
    dw, dh = max(1, int(W * rng.uniform(0.15, 3.0))), max(1, int(H * rng.uniform(0.15, 3.0)))
    dw, dh = min(dw, 600 if n <= 6 else 128), min(dh, 300 if n <= 6 else 64)
    if rng.integers(4) == 0:
        kx, ky = _i(rng, 1, 5), _i(rng, 1, 5)
        dw, dh = max(2, min(dw, 300)), max(2, min(dh, 40))
        W, H = dw * kx, dh * ky
    call.update(W=W, H=H, dw=dw, dh=dh, batch=bool(n > 1 or rng.integers(2)))
    call["jobs"] = [dict(frame=i % len(call["frames"])) for i in range(n)]
    return pack(settle_sources(call), [_pick(rng, LAYOUT_KINDS) for _ in range(n)])


def encode_case(rng):
    """vpf_tensor_convert(_batch): w x h (odd sizes included; one call in three a multiple of 16 wide and even high: the fast kernel's shape),
    NV12 or YUV420, dtype, channel order, layout of the source tensor and of the destination picture, 1 .. 4 frames"""
    w, h = (16 * _i(rng, 1, 70), 2 * _i(rng, 1, 12)) if rng.integers(3) == 0 else (_i(rng, 1, 300), _i(rng, 1, 80))
    dtype, nhwc = _i(rng, 0, 2), bool(rng.integers(2))
    e = ELEM[dtype]
    n = _i(rng, 1, 4)
    call = dict(entry="encode", dst_fmt=_pick(rng, ("NV12", "YUV420")), cr=_i(rng, 0, 1), w=w, h=h, dtype=dtype, bgr=bool(rng.integers(2)), nhwc=nhwc,
                params=_pick(rng, ("imagenet", "unit")), tune=0 if rng.integers(5) else 9, n=n, batch=bool(n > 1 or rng.integers(2)),
                input=_pick(rng, ("planted", "special")), seed=_i(rng, 0, (1 << 30) - 1))
    # the source tensor: TensorSrc / NhwcSrc keywords
    rb = (3 if nhwc else 1) * w * e
    kind = _pick(rng, LAYOUT_KINDS)
    row = rb if kind in ("contiguous", "off_by_one_element") else rb + 16 + e if kind == "padded" else (rb + 63) // 64 * 64 + 64
    src = dict(kind=kind, row=row, lead=e if kind == "off_by_one_element" else 0 if kind == "contiguous" else 24 * e if kind == "padded" else 512)
    if nhwc:
        src["frame"] = h * row + e * _i(rng, 0, 9)
    else:
        src["plane"] = h * row + e * _i(rng, 0, 9)
        src["frame"] = 3 * src["plane"] + e * _i(rng, 0, 9)
    call["src"] = src
    call["dst"] = _pick(rng, (dict(align=256, extra=0, offset=0), dict(align=64, extra=3, offset=0), dict(align=1, extra=0, offset=0), dict(align=16, extra=0, offset=8)))
    return call


GENERATORS = {"whole": whole_case, "rois": roi_case, "rois_dev": rois_dev_case, "letterbox": letterbox_case, "warp": warp_case, "warp_dev": warp_dev_case,
              "encode": encode_case, "persp": persp_case, "letterbox_aa": letterbox_aa_case, "remap": remap_case}
