"""The cases of tests/test_gpu_mixed_layouts.py, importable without a GPU: calls of the 8-bit entries (vpf_convert(_batch), vpf_resize_batch(_ws),
vpf_convert_resize(_batch), vpf_remap(_batch)) whose planes do NOT all lie alike.  The C ABI takes a pointer and a pitch per plane and per frame,
and every launcher decides from them which kernel may run; tests that give all planes of a call one (align, extra, offset) cannot see a gate that
looks at the wrong plane or frame, nor a kernel that indexes with the wrong pitch.  tests/test_mixed_layout_cases_cpu.py checks on the CPU that
the generator is deterministic and emits only calls the ABI accepts.

A case is a plain dict, printable in one line (describe), reproducible from (entry, key) for the directed ones and from (entry, seed, index) for
the seeded ones.  case["src"] / case["dst"] hold one frame layout per frame: a list of (align, extra, offset) per plane, each plane in an
allocation of its own (pitch = round_up(row_bytes, align) + extra, first byte `offset` bytes in), or {"stacked": (align, extra, offset)} —
all planes in one allocation with one pitch (gpu_util.plane_geometry).

Three kinds of directed case per entry and format:
  P  pitch-only: every plane of every frame 256-B aligned, no two planes of the call with the same pitch.  The kernel selection must not
     change; only indexing with another plane's or frame's pitch can go wrong.
  O  one odd plane: everything on the A256 rung but ONE plane (source or destination) of ONE frame, which goes down the rungs A8 .. A1 (no
     launcher has a gate above 16 B, so A16 — which every gate passes — appears in the seeded family only).
  S  stacked: planar formats in one allocation with pitch = row bytes at sizes whose plane size is odd; NV12 as one W x 1.5 H plane.
The seeded family (cases(entry, seed)) draws the rung per plane and per frame."""
import numpy as np

FMT = dict(Y=1, RGB=2, NV12=3, YUV420=4, RGB_PLANAR=5, BGR=6, YCBCR=7, YUV444=8, RGB_32F=9, P10=12)  # Pixel_Format (capi.py, oracle/__init__.py)
NEAREST, LINEAR, LANCZOS3 = 0, 1, 2
INTERP = dict(nearest=NEAREST, linear=LINEAR, lanczos=LANCZOS3)
RUNGS = {"A256": (256, 0, 0), "A16": (16, 16, 16), "A8": (8, 8, 8), "A4": (4, 4, 4), "A2": (2, 2, 2), "A1": (1, 1, 1)}
A256 = RUNGS["A256"]
LADDER = ("A8", "A4", "A2", "A1")       # what the ONE odd plane of an (O) case goes down
ENTRIES = ("convert", "resize", "fused", "remap")
BASE = {"convert": 41000, "resize": 43000, "fused": 45000, "remap": 47000}
CASES_PER_SEED = {"convert": 4, "resize": 4, "fused": 3, "remap": 3}
FUZZ_N = (1, 2, 3, 5, 33, 40, 130)
# the frame positions of the odd frame in a batch: first, last and middle of a small batch; alone in the second dispatch of a 32-frame entry (the
# scalar-argument `_one` kernels of vpf_convert_batch) and in the last slot of the first one
POSITIONS = ((5, 0), (5, 4), (5, 2), (33, 32), (33, 31))
# vpf_convert_batch: per position the rungs the odd plane takes — the bottom rung of its ladder everywhere, a middle rung as well at two of them
# (a rung below the plane's element size is left out); the planes of the format take turns over the positions
CONVERT_BATCH_RUNGS = {(5, 0): ("bottom",), (5, 4): ("bottom", "A4"), (5, 2): ("bottom",), (33, 32): ("bottom", "A8"), (33, 31): ("bottom",)}


def round_up(v, a):
    return (v + a - 1) // a * a


def plane_shapes(fmt, w, h):
    """[(rows, row_bytes, element size)] per plane (row_bytes of include/vpf_hip.h)"""
    cw, ch = (w + 1) // 2, (h + 1) // 2
    f = {v: k for k, v in FMT.items()}[fmt]
    if f == "Y":
        return [(h, w, 1)]
    if f in ("RGB", "BGR"):
        return [(h, 3 * w, 1)]
    if f == "NV12":
        return [(h, w, 1), (ch, 2 * cw, 1)]
    if f in ("YUV420", "YCBCR"):
        return [(h, w, 1), (ch, cw, 1), (ch, cw, 1)]
    if f in ("YUV444", "RGB_PLANAR"):
        return [(h, w, 1)] * 3
    if f == "RGB_32F":
        return [(h, 12 * w, 4)]
    assert f == "P10"
    return [(h, 2 * w, 2), (ch, 4 * cw, 2)]


def side_shape(case, side):
    """(format, width, height) of the planes on one side of the call"""
    if side == "src":
        return case["sf"], case["sw"], case["sh"]
    return case["df"], case["dw"], case["dh"]


def layout_args(frame_layout):
    """(layouts, stacked) as gpu_util.plane_geometry / LaidOutPlanes take them"""
    if isinstance(frame_layout, dict):
        return tuple(frame_layout["stacked"]), True
    return [tuple(t) for t in frame_layout], False


def describe(case):
    """one line that names the whole call"""
    return repr(case)


def call_key(case):
    """what two cases share when they are the same call in another layout"""
    return tuple(case[k] for k in ("entry", "api", "sf", "df", "cs", "cr", "interp", "sw", "sh", "dw", "dh", "n"))


def family(case):
    """entry and format family — for resize per filter, so that no filter passes on the strength of another: the (O) cases of one family
    together must reach more than one kernel"""
    return (case["entry"], case["sf"], case["df"], case["interp"] if case["entry"] == "resize" else None)


def uniform(case, variant=0):
    """the same call with every plane on the A256 rung (remap: dense maps on a 256-B base)"""
    u = dict(case, kind="U", variant=variant, odd=None, flag_only=False, tier=None)
    for side in ("src", "dst"):
        fmt, w, h = side_shape(case, side)
        u[side] = [[A256] * len(plane_shapes(fmt, w, h)) for _ in range(case["n"])]
    if case["entry"] == "remap":
        u["maps"] = dict(xp=4 * case["dw"], yp=4 * case["dw"], xoff=0, yoff=0)
    return u


def _call(entry, api, n, sf, df, sw, sh, dw, dh, cs=0, cr=0, interp=LINEAR, shape=None, seed=0):
    c = dict(entry=entry, kind="U", api=api, n=n, sf=sf, df=df, cs=cs, cr=cr, interp=interp, sw=sw, sh=sh, dw=dw, dh=dh, shape=shape, variant=0,
             seed=seed, odd=None, flag_only=False, tier=None)
    return uniform(c)


def min_rung(elem):
    """16-bit and float planes start at the rung that equals their element size (planes_ok and the float rule of vpf_resize_batch)"""
    return [r for r in LADDER if RUNGS[r][0] >= elem]


def pitch_only(call):
    """(P): plane k of frame i gets round_up(row_bytes, 256) + 256 (1 + k + 3 i); where that pitch is taken already (source and destination
    planes with the same row bytes) it grows by 256 * 3 n until it is free"""
    c = dict(call, kind="P")
    used, n = set(), call["n"]
    for side in ("src", "dst"):
        fmt, w, h = side_shape(call, side)
        frames = []
        for i in range(n):
            fl = []
            for k, (_, rb, _) in enumerate(plane_shapes(fmt, w, h)):
                extra = 256 * (1 + k + 3 * i)
                while round_up(rb, 256) + extra in used:
                    extra += 256 * 3 * n
                used.add(round_up(rb, 256) + extra)
                fl.append((256, extra, 0))
            frames.append(fl)
        c[side] = frames
    if call["entry"] == "remap":
        c["maps"] = dict(xp=4 * call["dw"] + 16, yp=4 * call["dw"] + 48, xoff=16, yoff=16)
    return c


def one_odd(call, side, frame, plane, rung, flag_only=False, tier=None):
    """(O): ONE plane of ONE frame on `rung`"""
    c = dict(call, kind="O", odd=dict(side=side, frame=frame, plane=plane, rung=rung), flag_only=flag_only, tier=tier)
    c[side] = [list(fl) for fl in call[side]]
    c[side][frame][plane] = RUNGS[rung]
    return c


def stacked(call, nv12_extra=True):
    """(S): multi-plane formats in ONE allocation with pitch = the widest row's bytes (NV12 / P10: one element more, so that the shared pitch of
    the W x 1.5 H plane is odd in elements); one-plane formats tight"""
    c = dict(call, kind="S")
    for side in ("src", "dst"):
        fmt, w, h = side_shape(call, side)
        ps = plane_shapes(fmt, w, h)
        if len(ps) == 1:
            c[side] = [[(ps[0][2], 0, 0)] for _ in range(call["n"])]
        else:
            two = len(ps) == 2 and nv12_extra
            c[side] = [{"stacked": (ps[0][2], ps[0][2] if two else 0, 0)} for _ in range(call["n"])]
    return c


def planes_of(call):
    """[(side, plane index, element size)] of every plane of one frame of the call"""
    out = []
    for side in ("src", "dst"):
        fmt, w, h = side_shape(call, side)
        out += [(side, k, e) for k, (_, _, e) in enumerate(plane_shapes(fmt, w, h))]
    return out


# ------------------------------------------------------------------------------------------------ vpf_convert / vpf_convert_batch
# (source, destination, width, height, alignment thresholds per source plane, per destination plane).  The thresholds restate the launchers' gates
# (convert_aligned of csrc/vpf_convert_plan.h, asked by the rules of all three units): a plane whose pointer and pitch are multiples of t for
# the first j thresholds t is on tier j, the kernel is picked by the lowest tier of the call, and with ONE plane off A256 two calls take the
# same kernel exactly when that plane is on the same tier.  1040 x 6 / 640 x 4: the p16x / p16 / r16 converters; 1056 x 4: a multiple of 32
# above 1024 for the r16 form of NV12 <-> YUV420.
T, C, R = (16, 4), (8, 2), (16,)   # the 16-B kernel then the 4-B one; 4:2:0 chroma planes of half the width; one fast kernel only
CONVERT = [
    ("NV12", "RGB", 1040, 6, [T, T], [T]), ("NV12", "BGR", 640, 4, [T, T], [T]), ("NV12", "RGB_PLANAR", 1040, 6, [T, T], [T] * 3),
    ("YUV420", "RGB", 1040, 6, [T, C, C], [T]), ("YUV420", "RGB_PLANAR", 640, 4, [T, C, C], [T] * 3),
    ("YUV444", "RGB", 1040, 6, [T] * 3, [T]), ("YUV444", "RGB_PLANAR", 640, 4, [T] * 3, [T] * 3),
    ("RGB", "YUV420", 1040, 6, [T], [T, C, C]), ("RGB", "YUV444", 640, 4, [T], [T] * 3), ("RGB", "YCBCR", 1040, 6, [T], [T, C, C]),
    ("RGB_PLANAR", "YUV420", 640, 4, [T] * 3, [T, C, C]), ("RGB_PLANAR", "YUV444", 1040, 6, [T] * 3, [T] * 3),
    # NV12 <-> YUV420: r16 asks 16 B of every plane, the p16 form behind it 8 B of the half-width planes
    ("NV12", "YUV420", 1056, 4, [R, R], [R, (16, 8), (16, 8)]), ("YUV420", "NV12", 1056, 4, [R, (16, 8), (16, 8)], [R, R]),
    ("RGB", "RGB_PLANAR", 1040, 6, [T], [T] * 3), ("RGB_PLANAR", "RGB", 1040, 6, [T] * 3, [T]), ("RGB", "BGR", 640, 4, [T], [T]),
    ("RGB_PLANAR", "Y", 1040, 6, [T] * 3, [T]),
    ("P10", "NV12", 1040, 6, [R, R], [(16, 8), (16, 8)]),   # x16 asks 16 B everywhere, p8 16 B of the source and 8 B of the destination
    ("RGB", "RGB_32F", 1040, 6, [(4,)], [R]),               # both fast kernels ask 4 B of the source and 16 B of the destination
]


def tier_of(rung, thresholds):
    return sum(1 for t in thresholds if RUNGS[rung][0] % t == 0)


def convert_key(sf, df):
    return f"{sf}-{df}"


def _convert_directed(key):
    sf, df, w, h, sthr, dthr = next(c for c in CONVERT if convert_key(c[0], c[1]) == key)
    cr = 1 if sf.startswith("RGB") and df in ("YUV420", "YUV444") else 0  # (RGB -> YUV takes BT.601 only; both ranges get their turn)
    def call(api, n, ww=w, hh=h):
        return _call("convert", api, n, FMT[sf], FMT[df], ww, hh, ww, hh, cs=0, cr=cr, seed=100)
    out = [pitch_only(call("single", 1)), pitch_only(call("batch", 3)), pitch_only(call("batch", 33))]   # (33: the second dispatch has frame 32 alone)
    one = call("single", 1)
    planes = planes_of(one)
    thr = {("src", k): t for k, t in enumerate(sthr)}
    thr.update({("dst", k): t for k, t in enumerate(dthr)})
    for side, k, e in planes:
        for rung in min_rung(e):
            out.append(one_odd(one, side, 0, k, rung, tier=(tier_of(rung, thr[side, k]), len(thr[side, k]))))
    for turn, (n, pos) in enumerate(POSITIONS):
        side, k, e = planes[turn % len(planes)]
        ladder = min_rung(e)
        for name in CONVERT_BATCH_RUNGS[n, pos]:
            rung = ladder[-1] if name == "bottom" else name
            if rung in ladder and (name == "bottom" or rung != ladder[-1]):
                out.append(one_odd(call("batch", n), side, pos, k, rung, tier=(tier_of(rung, thr[side, k]), len(thr[side, k]))))
    for (ww, hh) in ((227, 227), (225, 15)):
        out.append(stacked(call("single", 1, ww, hh)))
    out.append(stacked(call("batch", 2, 225, 15)))
    return out


# ------------------------------------------------------------------------------------------------ vpf_resize_batch / vpf_resize_batch_ws
RESIZE_FORMATS = ("Y", "NV12", "YUV420", "YUV444", "RGB", "RGB_PLANAR", "RGB_32F")
# an exact 2x (sw % 32 == 0: Half3R16Task), a general down-scale, an up-scale, a 3x - 5x down-scale (two-chunk windows / half tiles)
RESIZE_SHAPES = (("2x", 1056, 32, 528, 16), ("down", 1040, 48, 700, 32), ("up", 320, 20, 704, 44), ("steep", 1088, 64, 300, 17))
# The (O) cases of resize and fused: every plane goes down its ladder once.  Plane number p (source planes first) on rung number r takes shape
# number (p + r) mod the number of shapes — every plane starts one shape later, so over the planes every rung meets every shape — and the
# cases, counted through, take 2, 1, 3 frames (resize) or 1, 2, 3 (fused) in turn, the odd frame moving along: case c of n frames has frame c mod n.
RESIZE_FRAMES, FUSED_FRAMES = (2, 1, 3), (1, 2, 3)


def odd_turns(planes, shapes, frames, ladder_of):
    """[(side, plane, rung, shape name, frames, odd frame)] by the rule above"""
    out = []
    for p, (side, k, e) in enumerate(planes):
        for r, rung in enumerate(ladder_of(e)):
            n = frames[len(out) % len(frames)]
            out.append((side, k, rung, shapes[(p + r) % len(shapes)], n, len(out) % n))
    return out


def _resize_flag_only(fmt, interp, shape, side, n):
    """a destination plane decides the kernel only where the kernel's stores need it: the exact-2x kernels (the `aligned(p, 7, 3 | 7)` and
    `aligned(p, 15, 15)` tests of `resize_plan`, csrc/vpf_resize_plan.h) and the matrix-core Lanczos kernel (16-B rows on both sides; one frame per dispatch takes the tile
    kernel, whose stores do not).  Everywhere else the gate of a destination plane sets the runtime flag vec_ok of the same kernel, so the
    reach test asserts no change of kernel there."""
    if side == "src":
        return False
    if fmt == "RGB_32F":
        return True
    return not ((interp == LINEAR and shape == "2x") or (interp == LANCZOS3 and n > 1))


def _resize_directed(key):
    fmt, iname = key.split("-")
    interp = INTERP[iname]
    def call(shape, n, api="batch"):
        name, sw, sh, dw, dh = next(s for s in RESIZE_SHAPES if s[0] == shape)
        return _call("resize", api, n, FMT[fmt], FMT[fmt], sw, sh, dw, dh, interp=interp, shape=name, seed=200)
    names = [s[0] for s in RESIZE_SHAPES]
    out = [pitch_only(call(s, 3)) for s in names] + [pitch_only(call("down", 1))]
    planes = planes_of(call("2x", 1))
    # (a Lanczos batch of at least 2 frames takes the matrix-core kernel, one frame the tile kernel)
    for side, k, rung, shape, n, frame in odd_turns(planes, names, RESIZE_FRAMES, min_rung):
        out.append(one_odd(call(shape, n), side, frame, k, rung, flag_only=_resize_flag_only(fmt, interp, shape, side, n)))
    for turn, (n, pos) in enumerate(POSITIONS):   # the planes take turns over the positions, the exact 2x and the general down-scale too
        side, k, e = planes[turn % len(planes)]
        shape = ("2x", "down")[turn % 2]
        out.append(one_odd(call(shape, n), side, pos, k, min_rung(e)[-1], flag_only=_resize_flag_only(fmt, interp, shape, side, n)))
    if len(planes) > 2:
        # the per-plane fallbacks of launch_resize_planned: only the last SOURCE plane odd, in a batch of two
        out.append(one_odd(call("down", 2), "src", 1, len(planes) // 2 - 1, "A1"))
        for (ww, hh, dw, dh) in ((227, 227, 113, 113), (225, 15, 150, 10)):
            out.append(stacked(_call("resize", "batch", 2, FMT[fmt], FMT[fmt], ww, hh, dw, dh, interp=interp, shape="odd", seed=200)))
    if interp == LANCZOS3 and fmt == "NV12":
        out.append(pitch_only(call("down", 2, api="batch_ws")))   # vpf_resize_batch_ws, once
    return out


# ------------------------------------------------------------------------------------------------ vpf_convert_resize / vpf_convert_resize_batch
FUSED_PAIRS = [(s, d) for s in ("NV12", "YUV420") for d in ("RGB", "BGR", "RGB_PLANAR")]
FUSED_SHAPES = (("2x", 1056, 32, 528, 16), ("below2x", 1040, 48, 700, 32), ("beyond2x", 1088, 64, 300, 17))


def _fused_directed(key):
    sf, df = key.split("-")
    def call(shape, api, n):
        name, sw, sh, dw, dh = next(s for s in FUSED_SHAPES if s[0] == shape)
        return _call("fused", api, n, FMT[sf], FMT[df], sw, sh, dw, dh, cs=1, cr=0, shape=name, seed=300)
    names = [s[0] for s in FUSED_SHAPES]
    out = [pitch_only(call(s, "batch", 3)) for s in names] + [pitch_only(call("2x", "single", 1))]
    planes = planes_of(call("2x", "single", 1))
    for side, k, rung, shape, n, frame in odd_turns(planes, names, FUSED_FRAMES, lambda e: LADDER):
        # the OR over all planes into dst_bits decides the kernel for the exact 2x only (vpf_fused_plan.h); else it sets vec_ok
        out.append(one_odd(call(shape, "single" if n == 1 else "batch", n), side, frame, k, rung, flag_only=side == "dst" and shape != "2x"))
    for turn, (n, pos) in enumerate(POSITIONS):
        side, k, e = planes[turn % len(planes)]
        shape = ("2x", "below2x")[turn % 2]
        out.append(one_odd(call(shape, "batch", n), side, pos, k, "A1", flag_only=side == "dst" and shape != "2x"))
    for api, n in (("single", 1), ("batch", 2)):
        out.append(stacked(_call("fused", api, n, FMT[sf], FMT[df], 227, 227, 113, 113, cs=1, cr=0, shape="odd", seed=300)))
    out.append(stacked(_call("fused", "single", 1, FMT[sf], FMT[df], 225, 15, 150, 10, cs=1, cr=0, shape="odd", seed=300)))
    return out


# ------------------------------------------------------------------------------------------------ vpf_remap / vpf_remap_batch
def _remap_directed(key):
    out = []
    for dw in (256, 253):   # dw % 4 == 0: the four-pixel kernel; else the general one
        def call(api, n):
            c = _call("remap", api, n, FMT[key], FMT[key], 320, 24, dw, 20, shape=f"dw{dw}", seed=400)
            return c
        out += [pitch_only(call("single", 1)), pitch_only(call("batch", 3)), pitch_only(call("batch", 33))]
        for api, n, pos in (("single", 1, 0), ("batch", 3, 1), ("batch", 3, 0), ("batch", 3, 2), ("batch", 33, 32), ("batch", 33, 31)):
            base = call(api, n)
            full = n < 33 and pos < 2   # the whole ladder and all four map cases; the other positions: one map case, the bottom rung
            # the ONE odd thing: xmap rows (pitch 4 dw + 4), xmap base (+ 4 B), ymap likewise — the maps' gate asks 16 B —, the source
            # (4 B asked), the destination (sets vec_ok of the same kernel)
            for what, maps in (("xmap_rows", dict(xp=4 * dw + 4)), ("xmap_base", dict(xoff=4)), ("ymap_rows", dict(yp=4 * dw + 4)), ("ymap_base", dict(yoff=4))):
                if not full and what != ("xmap_rows", "ymap_base")[pos % 2]:
                    continue
                out.append(dict(base, kind="O", odd=dict(side="maps", frame=0, plane=what, rung="A4"), maps=dict(base["maps"], **maps)))
            for rung in LADDER if full else ("A1",):
                out.append(one_odd(base, "src", pos, 0, rung))
                out.append(one_odd(base, "dst", pos, 0, rung, flag_only=True))
    return out


DIRECTED = {"convert": _convert_directed, "resize": _resize_directed, "fused": _fused_directed, "remap": _remap_directed}
KEYS = {"convert": [convert_key(c[0], c[1]) for c in CONVERT], "resize": [f"{f}-{i}" for f in RESIZE_FORMATS for i in INTERP],
        "fused": [f"{s}-{d}" for s, d in FUSED_PAIRS], "remap": ["RGB", "BGR"]}


def directed(entry, key):
    """the directed cases of one entry and format, in the order the GPU test runs them"""
    return DIRECTED[entry](key)


# ------------------------------------------------------------------------------------------------ the seeded family
def _i(rng, lo, hi):
    return int(rng.integers(lo, hi + 1))


def _pick(rng, seq):
    return seq[int(rng.integers(len(seq)))]


def _draw_layouts(rng, call):
    """the rung of every plane of every frame, drawn independently"""
    for side in ("src", "dst"):
        fmt, w, h = side_shape(call, side)
        call[side] = [[RUNGS[_pick(rng, ["A256", "A16"] + min_rung(e))] for (_, _, e) in plane_shapes(fmt, w, h)] for _ in range(call["n"])]
    return call


def _small(rng, shape):
    """a directed shape at a quarter to a sixteenth of its width and a quarter of its height, for the calls of 33 frames and more; the exact 2x
    stays one, and its source a multiple of 32 wide"""
    name, sw, sh, dw, dh = shape
    f = 4 * _pick(rng, (1, 2, 4))
    if name == "2x":
        sw, sh = max(sw // f // 32 * 32, 32), max(sh // 4 // 2 * 2, 2)
        return sw, sh, sw // 2, sh // 2
    return max(sw // f // 4 * 4, 8), max(sh // 4, 4), max(dw // f, 4), max(dh // 4, 2)


def _fuzz_case(entry, rng):
    n = _pick(rng, FUZZ_N)
    small = n >= 33
    variant = _pick(rng, (0, 0, 0, 40, 9))
    seed = _i(rng, 0, (1 << 30) - 1)
    if entry == "convert":
        sf, df, w, h = _pick(rng, CONVERT)[:4]
        if small:
            w, h = 16 * _i(rng, 2, 5), 2 * _i(rng, 1, 3)
        elif rng.integers(3) == 0:
            w, h = _i(rng, 1, 300), _i(rng, 1, 40)
        c = _call("convert", "batch" if n > 1 or rng.integers(2) else "single", n, FMT[sf], FMT[df], w, h, w, h, cs=0, cr=_i(rng, 0, 1), seed=seed)
    elif entry == "resize":
        fmt = _pick(rng, RESIZE_FORMATS)
        sw, sh, dw, dh = _small(rng, _pick(rng, RESIZE_SHAPES)) if small else _pick(rng, RESIZE_SHAPES)[1:]
        c = _call("resize", "batch", n, FMT[fmt], FMT[fmt], sw, sh, dw, dh, interp=_i(rng, 0, 2), shape="fuzz", seed=seed)
    elif entry == "fused":
        sf, df = _pick(rng, FUSED_PAIRS)
        sw, sh, dw, dh = _small(rng, _pick(rng, FUSED_SHAPES)) if small else _pick(rng, FUSED_SHAPES)[1:]
        c = _call("fused", "batch" if n > 1 or rng.integers(2) else "single", n, FMT[sf], FMT[df], sw, sh, dw, dh, cs=_i(rng, 0, 1), cr=_i(rng, 0, 1),
                  shape="fuzz", seed=seed)
    else:
        dw = _pick(rng, (64, 61)) if small else _pick(rng, (256, 253, 96))
        c = _call("remap", "batch" if n > 1 or rng.integers(2) else "single", n, *[FMT[_pick(rng, ("RGB", "BGR"))]] * 2, 80 if small else 320, 24, dw, 12 if small else 20,
                  shape="fuzz", seed=seed)
        c["maps"] = dict(xp=4 * dw + 4 * _pick(rng, (0, 1, 4, 12)), yp=4 * dw + 4 * _pick(rng, (0, 1, 4, 12)), xoff=_pick(rng, (0, 4, 16)), yoff=_pick(rng, (0, 4, 16)))
    c.update(kind="F", variant=variant)
    return _draw_layouts(rng, c)


def cases(entry, seed):
    """the calls of one seed, in the order the GPU test runs them"""
    rng = np.random.default_rng(BASE[entry] + seed)
    return [_fuzz_case(entry, rng) for _ in range(CASES_PER_SEED[entry])]


# ------------------------------------------------------------------------------------------------ the call itself
def remap_maps(case):
    """the two float maps of a remap case, tight: the destination grid scaled onto the source with +-0.7 px of jitter, a few NaNs, a column
    left of the picture and a row below it — those pixels keep what the destination held"""
    rng = np.random.default_rng(case["seed"] + 7)
    sw, sh, dw, dh = case["sw"], case["sh"], case["dw"], case["dh"]
    xm = (np.tile(np.arange(dw, dtype=np.float32), (dh, 1)) * (sw / dw) + rng.uniform(-0.7, 0.7, (dh, dw))).astype(np.float32)
    ym = (np.tile(np.arange(dh, dtype=np.float32)[:, None], (1, dw)) * (sh / dh) + rng.uniform(-0.7, 0.7, (dh, dw))).astype(np.float32)
    xm[1, 2:6] = np.nan
    xm[:, dw // 3] = -3.0
    ym[dh - 2, :] = sh + 2.0
    return xm, ym


def reference(oracle, case, src, maps=None, fill=77):
    """(FP32 planes, EXACT planes) of the call on the tight planes `src`: what the kernels must equal bit for bit, and what they must stay within 1
    LSB of (nearest: the caller skips that).  maps = remap_maps(case) for remap, whose destination starts filled with `fill`.

    The fused entries are DEFINED as two steps through an 8-bit temporary (oracle/vpf_oracle.c).  The DIRECTED cases are held to 1 LSB of the
    EXACT chain, as tests/test_gpu_parity.py::test_fuzz_resize_and_fused holds the fused entry.  For arbitrary input that is no bound: the
    temporaries of the two modes differ by at most 1, a blend with weights that sum to 1 passes on at most 1 and round-half-up keeps that, and the
    FP32 filter adds its own 1 — 2 in all, and it is reached: YUV420 -> BGR, BT.601 JPEG, 1040 x 48 -> 700 x 32, cases("fused", 80)[0]: 2 codes
    at 1 of 67 200 bytes, in the oracle alone.  So the SEEDED family (kind "F") holds the 1-LSB bar per link, as _convert and _resize hold it per
    operation: the FP32 temporary is within 1 LSB of the EXACT conversion and the chain within 2 of the EXACT chain (both asserted here), and the
    EXACT planes returned are the EXACT bilinear resize OF THE FP32 TEMPORARY."""
    e, sf, df, cs, cr, sw, sh, dw, dh = (case[k] for k in ("entry", "sf", "df", "cs", "cr", "sw", "sh", "dw", "dh"))

    def ok(result):
        assert result[0] == 0, describe(case)
        return result[1]

    def gap(a, b):
        return max(int(np.abs(p.astype(np.int16) - q.astype(np.int16)).max()) for p, q in zip(a, b))

    if e == "convert":
        return tuple(ok(oracle.convert(sf, df, cs, cr, sw, sh, src, mode)) for mode in (oracle.FP32, oracle.EXACT))
    if e == "resize":
        return tuple(ok(oracle.resize(sf, case["interp"], sw, sh, src, dw, dh, mode)) for mode in (oracle.FP32, oracle.EXACT))
    if e == "remap":
        return tuple(ok(oracle.remap(sf, sw, sh, src, maps[0], maps[1], mode=mode, dst=oracle.alloc(sf, dw, dh, fill=fill))) for mode in (oracle.FP32, oracle.EXACT))
    fp32, chain = (ok(oracle.convert_resize(sf, df, cs, cr, sw, sh, src, dw, dh, mode)) for mode in (oracle.FP32, oracle.EXACT))
    if case["kind"] != "F":
        return fp32, chain
    mid = ok(oracle.convert(sf, df, cs, cr, sw, sh, src, oracle.FP32))
    assert gap(mid, ok(oracle.convert(sf, df, cs, cr, sw, sh, src, oracle.EXACT))) <= 1, describe(case)
    assert gap(fp32, chain) <= 2, describe(case)
    return fp32, ok(oracle.resize(df, LINEAR, sw, sh, mid, dw, dh, oracle.EXACT))


def launch(capi, ex, case, src_descs, dst_descs, maps=None):
    """the ABI call of `case` on planes that lie where the descriptors say: src_descs / dst_descs = one [(pointer, pitch)] per frame;
    maps = (xmap pointer, ymap pointer) for remap.  -> the vpf_status (nothing raises: the reach test's child wants the log only)"""
    e, n = case["entry"], case["n"]
    batch = capi.make_batch(list(zip(src_descs, dst_descs))) if case["api"] != "single" else None
    prev = capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, case["variant"])
    try:
        if e == "convert":
            if batch is None:
                return capi.convert(ex, case["sf"], case["df"], case["cs"], case["cr"], case["sw"], case["sh"], src_descs[0], dst_descs[0], check=False)
            return capi.convert_batch(ex, case["sf"], case["df"], case["cs"], case["cr"], case["sw"], case["sh"], batch, check=False)
        if e == "resize":
            if case["api"] == "batch_ws":
                return capi.resize_batch_ws(ex, case["sf"], case["interp"], case["sw"], case["sh"], case["dw"], case["dh"], batch, maps, check=False)
            return capi.resize_batch(ex, case["sf"], case["interp"], case["sw"], case["sh"], case["dw"], case["dh"], batch, check=False)
        if e == "fused":
            if batch is None:
                return capi.convert_resize(ex, case["sf"], case["df"], case["cs"], case["cr"], case["sw"], case["sh"], src_descs[0], case["dw"], case["dh"],
                                           dst_descs[0], check=False)
            return capi.convert_resize_batch(ex, case["sf"], case["df"], case["cs"], case["cr"], case["sw"], case["sh"], case["dw"], case["dh"], batch, check=False)
        m = case["maps"]
        if batch is None:
            return capi.remap(ex, case["sf"], case["sw"], case["sh"], src_descs[0][0], maps[0], m["xp"], maps[1], m["yp"], case["dw"], case["dh"], dst_descs[0][0],
                              check=False)
        return capi.remap_batch(ex, case["sf"], case["sw"], case["sh"], maps[0], m["xp"], maps[1], m["yp"], case["dw"], case["dh"], batch, check=False)
    finally:
        capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, prev)


# ------------------------------------------------------------------------------------------------ reach: what the cases must steer
def reach_cases():
    """(tag, case) of every launch the reach test's child makes: the (P) and (O) cases of every entry and format, and once per distinct call
    its uniform A256 twin under the policy (U0) and under the forced-generic tuning value 9 (U9: the family's most general kernel)"""
    seen = set()
    for entry in ENTRIES:
        for key in KEYS[entry]:
            for idx, case in enumerate(directed(entry, key)):
                if case["kind"] not in ("P", "O"):
                    continue
                ck = call_key(case)
                if ck not in seen:
                    seen.add(ck)
                    yield f"U0|{ck}", uniform(case)
                    yield f"U9|{ck}", uniform(case, 9)
                yield f"{case['kind']}|{entry}|{key}|{idx}", case


def bottom_rung(case, odd):
    """the last rung of the odd plane's ladder: A1, for 16-bit planes A2, for float planes A4"""
    fmt, w, h = side_shape(case, odd["side"])
    return min_rung(plane_shapes(fmt, w, h)[odd["plane"]][2])[-1]


def MFMA(line):
    """a launch line of the matrix-core Lanczos kernel (k_lanczos_mfma.hip)"""
    return "LzMfma" in line or "k_lanczos_mfma" in line


def kernels_seen(logs):
    """{entry: sorted names of the kernels and tasks its launches took}: the template arguments dropped, a task named by its `Task = ` part"""
    seen = {}
    for tag, case in reach_cases():
        for line in logs.get(tag, ()):
            name = line.split(" = vpf::")[1].rstrip("]") if " = vpf::" in line else line.strip("()").split("<")[0]
            seen.setdefault(case["entry"], set()).add(name)
    return {e: sorted(v) for e, v in seen.items()}


def check_reach(logs):
    """the assertions of test_reach_of_the_cases on logs = {tag: [kernel expression of every launch of that call]}"""
    differs, groups, seen_special = {}, {}, set()
    for tag, case in reach_cases():
        if tag[0] == "U":
            assert logs[tag], f"no launch logged: {tag}"
            continue
        what = describe(case)
        ck = call_key(case)
        log, u0, u9 = tuple(logs[tag]), tuple(logs[f"U0|{ck}"]), tuple(logs[f"U9|{ck}"])
        assert log, f"no launch logged: {what}"
        if case["kind"] == "P":
            assert log == u0, f"a pitch changed the kernel: {log} against {u0} on uniform planes: {what}"
            continue
        odd = case["odd"]
        leaves, could = differs.get(family(case), (False, False))
        differs[family(case)] = (leaves or log != u0, could or u0 != u9)
        if case["tier"] is not None:   # vpf_convert(_batch): the thresholds of the gates, restated in CONVERT
            tier, top = case["tier"]
            assert (log == u0) == (tier == top), f"tier {tier} of {top}: {log} against {u0} on uniform planes: {what}"
            g = groups.setdefault((ck, odd["side"], odd["frame"], odd["plane"]), {})
            for t2, l2 in g.items():
                assert (l2 == log) == (t2 == tier), f"tiers {t2} and {tier} of one plane: {l2} and {log}: {what}"
            g.setdefault(tier, log)
        elif case["entry"] == "resize" and case["interp"] == LANCZOS3 and odd["side"] == "dst" and not any(MFMA(l) for l in u0):
            pass   # (a shape the matrix-core kernel does not take: the tile kernel's destination gate sets vec_ok only)
        elif (odd["side"] == "maps" or odd["rung"] == bottom_rung(case, odd)) and not case["flag_only"] and u0 != u9:
            assert log != u0, f"the odd plane did not change the kernel {u0} (most general: {u9}): {what}"
        if case["entry"] == "resize" and case["shape"] == "down" and case["n"] == 2 and odd == dict(side="src", frame=1, plane=odd["plane"], rung="A1"):
            if case["sf"] == FMT["NV12"] and case["interp"] == LANCZOS3 and odd["plane"] == 1:
                seen_special.add("lanczos")
                assert any(MFMA(l) for l in log) and any("LanczosGatherTask" in l for l in log), f"{log}: {what}"
            if case["sf"] == FMT["YUV420"] and case["interp"] == LINEAR and odd["plane"] == 2:
                seen_special.add("bilinear")
                assert len(u0) == 1 and len(log) > 1, f"{log} against {u0} on uniform planes: {what}"
    assert seen_special == {"lanczos", "bilinear"}, seen_special
    for fam, (leaves, could) in differs.items():   # (nearest and the float bilinear resize are the gather kernel on any planes: nothing to leave)
        assert leaves or not could, f"no (O) case of {fam} takes another kernel than the uniform call"
