"""The antialiased letterbox's filter (vpf_convert_letterbox_tensor_aa) written a second time, from the comment of include/vpf_hip.h alone: numpy,
no GPU, no library, nothing of csrc/ or tests/c/.  tests/test_letterbox_aa_definition_cpu.py holds it against aa_ref (tests/c/aa_ref_capi.cpp, which
compiles the header the kernels include): a slip in csrc/vpf_aa_plan.h is shared by the kernels and aa_ref, and is not shared by this file.

aa_definition_u8   the header's text operation for operation in float32, as TWO PASSES: the whole H(j, dx) image, then the vertical fold
triangle_f64_u8    the plain float64 triangle filter: per-axis weight matrices normalised by their sum, clip(floor(v + 0.5), 0, 255)
fmaf32             fmaf as numpy does not have it: one rounding (the test checks it bit for bit against libm's fmaf)"""
import numpy as np

F = np.float32
D = np.float64


def fmaf32(a, b, c):
    """round_f32(a * b + c) with ONE rounding, element-wise on float32 arrays of finite values.
    The product of two float32 values has at most 48 significant bits: exact in float64.  s = p + c is rounded once to float64, and TwoSum gives
    its error e exactly (p + c = s + e).  Casting s to float32 would round a second time, and goes wrong where s lies on (or was rounded onto) a
    float32 midpoint.  So s is first turned into the ROUND-TO-ODD float64 of the exact sum: where e != 0 and the last mantissa bit of s is even, s
    moves one float64 ulp towards e (the neighbour on the exact sum's side, whose last bit is odd — mantissas alternate, across a power of two as
    well).  A round-to-odd value of 53 bits rounds to nearest-even at 24 bits (at 24 + 2 bits or more, and for float32 denormals too) exactly as the
    exact sum does: the odd last bit is a sticky bit that no midpoint of the narrower format can have."""
    a, b, c = (np.asarray(v, F).astype(D) for v in (a, b, c))
    a, b, c = np.broadcast_arrays(a, b, c)
    p = a * b
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    even = (np.ascontiguousarray(s).view(np.int64) & 1) == 0
    s = np.where((e != 0) & even, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    return s.astype(F)


def _axis(n_in, n_out):
    """per destination index d: (lo [out], taps [out], weights t [out, T] float32 (0 beyond hi), r = 1 / S [out] float32), the header's lines one by one"""
    s = F(n_in) / F(n_out)
    fs = max(s, F(1.0))
    inv = F(1.0) / fs
    d = np.arange(n_out, dtype=F)
    c = (d + F(0.5)) * s
    lo = np.maximum(0, np.trunc((c - fs) + F(0.5)).astype(np.int64))      # C truncation, then the clamp
    hi = np.minimum(n_in, np.trunc((c + fs) + F(0.5)).astype(np.int64))
    assert (hi > lo).all()
    T = int((hi - lo).max())
    k = lo[:, None] + np.arange(T)[None, :]
    x = np.abs((k.astype(F) + F(0.5)) - c[:, None])
    t = np.maximum(F(0.0), F(1.0) - x * inv)                               # multiply and subtract rounded separately
    t = np.where(k < hi[:, None], t, F(0.0)).astype(F)
    S = np.zeros(n_out, F)
    for j in range(T):                                                     # plain adds, ascending (a tap beyond hi adds 0.0f: nothing)
        S = S + t[:, j]
    assert (S >= F(0.5)).all()
    return lo, hi - lo, t, F(1.0) / S


def aa_definition_u8(rgb, rect, iw, ih):
    """rgb: three [H, W] byte planes of the frame (or one [3, H, W] array), rect = (x, y, w, h) -> [3, ih, iw] bytes.

    Both folds walk the taps of ALL pictures pixels in lockstep (tap 0 of every window, tap 1, ...): per pixel the order is the header's, ascending
    from acc = 0.0f, and a window shorter than the longest one folds fmaf(0.0f, P, acc) = acc at its end, which changes nothing.

    fmaf is one rounding in both folds:
      horizontal  a weight is a multiple of 2^-24 (t = 1 - x: for x <= 1/2 a float32 in [1/2, 1]; for x in (1/2, 1) x itself is a multiple of 2^-24
                  and the subtraction is exact), P is an integer up to 255, so every product and — a float32 that is a multiple of 2^-24 rounds to
                  one — every accumulator is a multiple of 2^-24.  A window has at most 2 fs + 3 taps of weight <= 1, so the accumulator stays
                  below 255 (2 fs + 3): below 2^16 up to a factor of 127, below 2^26 for the entry's in <= 65536.  A multiple of 2^-24 below 2^26
                  has at most 50 bits: the float64 a * b + c is EXACT, and the cast to float32 is the one rounding.
      vertical    H = r_x * acc is any float32: no such bound.  fmaf32 above: float64 TwoSum, round to odd, one cast."""
    planes = np.stack([np.asarray(p, np.uint8) for p in rgb])
    x, y, w, h = rect
    assert x >= 0 and y >= 0 and x + w <= planes.shape[2] and y + h <= planes.shape[1]
    P = planes[:, y:y + h, x:x + w].astype(D)                              # [3, h, w]: nothing outside the rectangle contributes
    lox, nx, tx, rx = _axis(w, iw)
    loy, ny, ty, ry = _axis(h, ih)
    # pass 1: H(j, dx) = r_x(dx) * fold_k fmaf(tx_k, P(lo_x + k, j), acc), every row j of the rectangle
    acc = np.zeros((3, h, iw), F)
    for k in range(tx.shape[1]):
        col = np.minimum(lox + k, w - 1)                                   # (beyond hi: weight 0.0f, any pixel)
        acc = (tx[:, k].astype(D)[None, None, :] * P[:, :, col] + acc.astype(D)).astype(F)
    Himg = rx[None, None, :] * acc                                         # float32 multiply
    # pass 2: V(dx, dy) = r_y(dy) * fold_j fmaf(ty_j, H(lo_y + j, dx), acc)
    acc = np.zeros((3, ih, iw), F)
    for j in range(ty.shape[1]):
        row = np.minimum(loy + j, h - 1)
        acc = fmaf32(ty[:, j][None, :, None], Himg[:, row, :], acc)
    V = ry[None, :, None] * acc
    return np.minimum(F(255.0), np.trunc(V + F(0.5))).astype(np.uint8)


def _weights_f64(n_in, n_out):
    s = D(n_in) / D(n_out)
    fs = max(s, 1.0)
    c = (np.arange(n_out, dtype=D) + 0.5) * s
    k = np.arange(n_in, dtype=D) + 0.5
    m = np.maximum(0.0, 1.0 - np.abs(k[None, :] - c[:, None]) / fs)
    return m / m.sum(axis=1, keepdims=True)


def triangle_f64_u8(rgb, rect, iw, ih):
    """the plain triangle filter in float64: weight max(0, 1 - |k + 0.5 - (d + 0.5) s| / max(s, 1)) over the whole axis, every row of the [out, in]
    matrix divided by its sum, My P Mx^T, rounded half up"""
    planes = np.stack([np.asarray(p, np.uint8) for p in rgb])
    x, y, w, h = rect
    P = planes[:, y:y + h, x:x + w].astype(D)
    v = np.einsum("ij,cjk,lk->cil", _weights_f64(h, ih), P, _weights_f64(w, iw), optimize=True)
    return np.clip(np.floor(v + 0.5), 0, 255).astype(np.uint8)
