"""Which refusal wins when a call of a fused tensor entry is wrong in TWO independent ways, without a GPU.

The single refusals are pinned one at a time by the entries' own CPU tests; this table pins their ORDER ("One host path for the
tensor entries"): source class / colour model (UNSUPPORTED), norm == NULL (BAD_ARG), dtype / flags (UNSUPPORTED), warp border mode
(UNSUPPORTED), opts->reserved (BAD_ARG), non-finite scale / bias (BAD_ARG), pointers / n / sizes (BAD_ARG), the device tables' frame and
job counts (BAD_ARG).  Options are looked at before finiteness.  Every case carries two refusals, so no single slip can turn one into a
launch: every pointer below is fake."""
import math

import pytest

W, H, DW, DH = 64, 32, 16, 8
SRC = [(0x100000, 64), (0x200000, 64)]                      # NV12 planes of a W x H frame
F32 = [(0x400000, 64), (0x500000, 64), (0x600000, 64)]      # three f32 planes of DW elements
F32_FULL = [(0x400000, 256), (0x500000, 256), (0x600000, 256)]  # ... of W elements (the encode entry's source)
JOB = 3 * DH * 64
ENTRIES = ("batch", "rois", "rois_dev", "letterbox", "warp", "warp_dev", "encode")
WARPS = ("warp", "warp_dev")
DEVS = ("rois_dev", "warp_dev")

NAN_SCALE = dict(scale=(0.01, math.nan, 0.01))
NAN_BIAS = dict(bias=(-1.0, -1.0, math.nan))
UNSUPPORTED, BAD_ARG = 1, 2
GOOD_NORM = {}   # _norm()'s defaults; None is the NULL pointer

# (case id, the entries it holds for, the two faults as keyword arguments of _call, the status)
CASES = [
    ("format+null_norm", ENTRIES, dict(bad_format=True, norm=None), UNSUPPORTED),
    ("null_norm+n0", ENTRIES, dict(norm=None, n=0), BAD_ARG),
    ("dtype3+n0", ENTRIES, dict(norm=dict(dtype=3), n=0), UNSUPPORTED),
    ("flags8+nan_scale", ENTRIES, dict(norm=dict(flags=8, **NAN_SCALE)), UNSUPPORTED),
    ("dtype3+nan_bias", ENTRIES, dict(norm=dict(dtype=3, **NAN_BIAS)), UNSUPPORTED),
    ("nan_scale+width0", ENTRIES, dict(norm=NAN_SCALE, sw=0, sh=64), BAD_ARG),
    ("border2+nan_scale", WARPS, dict(border_mode=2, norm=NAN_SCALE), UNSUPPORTED),
    ("border2+reserved", WARPS, dict(border_mode=2, reserved=1), UNSUPPORTED),
    ("border2+null_norm", WARPS, dict(border_mode=2, norm=None), BAD_ARG),
    ("reserved+dtype3", WARPS, dict(reserved=1, norm=dict(dtype=3)), UNSUPPORTED),
    ("reserved+flags8", ("letterbox",), dict(reserved=1, norm=dict(flags=8)), UNSUPPORTED),
    ("reserved+nan_scale", ("letterbox",), dict(reserved=1, norm=NAN_SCALE), BAD_ARG),
    ("frames129+dtype3", DEVS, dict(n=129, norm=dict(dtype=3)), UNSUPPORTED),
    ("max_n0+null_norm", DEVS, dict(max_n=0, norm=None), BAD_ARG),
]


def _norm(capi, dtype=0, flags=0, scale=(0.01, 0.01, 0.01), bias=(-1.0, -1.0, -1.0)):
    n = capi.TensorNorm()
    for c in range(3):
        n.scale[c], n.bias[c] = scale[c], bias[c]
    n.dtype, n.flags = dtype, flags
    return n


def _call(capi, entry, bad_format=False, norm=GOOD_NORM, n=1, sw=W, sh=H, border_mode=None, reserved=0, max_n=7):
    """one call of `entry` that is right in everything the keywords do not name; n is the job count, or the frame count of a device-table entry"""
    L, ref = capi.lib(), capi.C.byref
    ex = capi.make_exec(0, -1)
    fmt = capi.RGB if bad_format else capi.NV12
    pn = ref(_norm(capi, **norm)) if norm is not None else None
    ss, ds = capi.Size(sw, sh), capi.Size(DW, DH)
    rows = max(n, 1)  # the arrays hold what n says, and one element where it says none
    opts = None
    if entry in WARPS and (border_mode is not None or reserved):
        opts = capi.make_warp_opts(border_mode or 0)
        opts.reserved = reserved
    if entry == "letterbox" and reserved:
        opts = capi.make_letterbox_opts()
        opts.reserved = reserved
    po = ref(opts) if opts is not None else None
    if entry == "batch":
        return L.vpf_convert_resize_tensor_batch(ref(ex), fmt, 1, 0, ss, ds, n, capi.make_batch([(SRC, F32)] * rows), pn)
    if entry == "rois":
        return L.vpf_convert_resize_tensor_rois(ref(ex), fmt, 1, 0, ss, ds, n, capi.make_rois([(SRC, F32, (4, 2, 32, 16))] * rows), pn)
    if entry == "rois_dev":
        t = capi.make_rois_dev(0x700000, max_n, F32, JOB, 0x800000)
        return L.vpf_convert_resize_tensor_rois_dev(ref(ex), fmt, 1, 0, ss, ds, n, capi.make_frame_srcs([SRC] * rows), ref(t), pn)
    if entry == "letterbox":
        jobs = capi.make_letterbox_jobs([(SRC, F32, (4, 2, 32, 16), (0, 0, DW, DH))] * rows)
        return L.vpf_convert_letterbox_tensor(ref(ex), fmt, 1, 0, ss, ds, n, jobs, pn, po)
    if entry == "warp":
        return L.vpf_convert_warp_tensor(ref(ex), fmt, 1, 0, ss, ds, n, capi.make_warps([(SRC, F32, (1, 0, 0, 0, 1, 0))] * rows), pn, po)
    if entry == "warp_dev":
        t = capi.make_warps_dev(0x700000, max_n, F32, JOB, 0x780000, 0x800000)
        return L.vpf_convert_warp_tensor_dev(ref(ex), fmt, 1, 0, ss, ds, n, capi.make_frame_srcs([SRC] * rows), ref(t), pn, po)
    assert entry == "encode"  # tensor -> NV12: `fmt` is the DESTINATION format, `norm` the denorm, one size
    return L.vpf_tensor_convert_batch(ref(ex), fmt, 0, 0, ss, n, capi.make_batch([(F32_FULL, SRC)] * rows), pn)


@pytest.mark.parametrize("entry,faults,status", [pytest.param(e, f, s, id=f"{e}-{cid}") for cid, entries, f, s in CASES for e in entries])
def test_first_refusal_wins(capi, entry, faults, status):
    assert (capi.ERR_UNSUPPORTED, capi.ERR_BAD_ARG) == (UNSUPPORTED, BAD_ARG)
    assert _call(capi, entry, **faults) == status

