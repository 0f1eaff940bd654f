"""The eight per-job tensor entries at the rows of tests/cases_job_families.py: which job of a call lands in which job table and slot, which LDS
figure goes to the kernel and which to the launch, and the grids are policy (csrc/vpf_job_plan.h), and a policy regression writes one job's pixels
into another job's planes or leaves them unwritten.  Two checks per row:
  - ONE child process makes every row's call under VPF_HIP_LOG=2 (frames of zeros: only the selection log is read); the logged labels must be the
    row's, exactly and in launch order (tests/test_job_plan_cpu.py derives them from the plan alone, without a device);
  - in this process every job's planes must hold the oracle's bits with the canaries intact.  Ground truth as the sibling files compose it: roi.ref_u8
    (the letterbox: placed into the padded plane, test_gpu_letterbox_tensor.place), warp.want_bits, persp.want_bits; P10 frames through the 16-bit
    tests' planted frames (test_gpu_job_shapes.roi_u8 / warp_bits).  Bit patterns, no tolerance.
The job order of the host rows — staged, per tap, staged, each into a destination of its own — is the point: a slot mix-up moves pixels between jobs."""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:   # (the child process starts this file as a script)
    sys.path.insert(0, ROOT)

import cases_job_families as cases  # noqa: E402
import test_gpu_job_shapes as shapes
import test_gpu_letterbox_dev as lbdev
import test_gpu_letterbox_tensor as lb
import test_gpu_p16_tensor as p16
import test_gpu_persp_tensor as persp
import test_gpu_persps_dev as pdev
import test_gpu_rois_dev as rdev
import test_gpu_warps_dev as wdev
from test_gpu_tensor_nhwc import NhwcBuf, hwc
from test_gpu_tensor_out import ELEM, MATRICES, PARAMS, TensorBuf, assert_bits, reference_bits
from test_persp_tensor_cpu import persp_reference_u8

pytestmark = pytest.mark.gpu
BORDER, PAD, MODE, PARAM = shapes.BORDER, lb.PAD, 0, "imagenet"
ROI, LETTERBOX, WARP, PERSP = range(4)


@pytest.fixture(scope="module")
def orc(oracle):
    oracle.set_threads(16)
    return oracle


class ZeroFrame:
    """the planes of a frame of zeros (the child process: only the selection log is read)"""

    def __init__(self, sf, W, H):
        e = 2 if sf == "P10" else 1
        cw, ch = (W + 1) // 2, (H + 1) // 2
        shapes_ = [(H, W * e), (ch, 2 * cw * e)] if sf != "YUV420" else [(H, W), (ch, cw), (ch, cw)]
        self.bufs = [torch.zeros((rows, (rb + 63) // 64 * 64), dtype=torch.uint8, device="cuda") for rows, rb in shapes_]

    def desc(self):
        return [(b.data_ptr(), b.shape[1]) for b in self.bufs]


def make_buf(row):
    n, e = len(row["jobs"]), ELEM[row["dtype"]]
    if row["dev"]:
        return rdev.make_buf(n, row["dw"], row["dh"], row["dtype"], row["nhwc"], False)
    return (NhwcBuf if row["nhwc"] else TensorBuf)(n, row["dw"], row["dh"], e)


def invoke(capi, row, dev, buf, cs=1, cr=0):
    """the row's one call: job i writes buf.planes(i); `dev`: the device planes of the row's frame"""
    f, sf, nhwc, dtype, jobs = row["family"], row["sf"], row["nhwc"], row["dtype"], row["jobs"]
    size = (row["W"], row["H"], row["dw"], row["dh"])
    with shapes.tuned(capi, row["knob"]):
        if not row["dev"]:
            if f == ROI:
                shapes.run_rois(capi, sf, cs, cr, *size, dev, jobs, dtype, False, PARAM, buf, nhwc=nhwc, variant=row["knob"])
            elif f == LETTERBOX:
                lb.run_lb(capi, sf, cs, cr, *size, [(dev, r, p) for r, p in jobs], dtype, False, PARAM, buf, pad=PAD, nhwc=nhwc)
            elif f == WARP:
                shapes.run_warps(capi, sf, cs, cr, *size, dev, jobs, dtype, False, PARAM, buf, MODE, nhwc=nhwc, variant=row["knob"])
            else:
                persp.run_persps(capi, sf, cs, cr, *size, [(dev, m) for m in jobs], dtype, False, PARAM, buf, border=BORDER, mode=MODE, nhwc=nhwc)
        elif f == ROI:
            rdev.run_dev(capi, sf, cs, cr, *size, [dev], rdev.boxes_tensor([(0, r) for r in jobs]), buf, dtype, False, PARAM, nhwc)
        elif f == LETTERBOX:
            lbdev.run_dev(capi, sf, cs, cr, *size, [dev], rdev.boxes_tensor([(0, r) for r in jobs]), buf, dtype, False, PARAM, nhwc, pad=PAD)
        elif f == WARP:
            wdev.run_dev(capi, sf, cs, cr, *size, [dev], wdev.mats_tensor(jobs), None, buf, dtype, False, PARAM, nhwc, max_step=row["max_step"], border=BORDER, mode=MODE)
        else:
            pdev.run_dev(capi, sf, cs, cr, *size, [dev], pdev.mats_tensor(jobs), None, buf, dtype, False, PARAM, nhwc, max_step=row["max_step"], border=BORDER, mode=MODE)
        torch.cuda.synchronize()


_PERSP_P10 = {}


def want_bits(capi, orc, row, job, cs, cr):
    """planar reference bits [3, dh, dw] of one job of the row"""
    f, sf, dtype = row["family"], row["sf"], row["dtype"]
    W, H, dw, dh = row["W"], row["H"], row["dw"], row["dh"]
    if f == ROI:
        return reference_bits(shapes.roi_u8(orc, sf, cs, cr, W, H, tuple(job), dw, dh), *PARAMS[PARAM], dtype, False)
    if f == LETTERBOX:
        rect, place = job if not row["dev"] else (job, capi.letterbox_fit(job[2], job[3], dw, dh))   # a device row: the kernel fits the box
        inner = shapes.roi_u8(orc, sf, cs, cr, W, H, tuple(rect), place[2], place[3])
        return reference_bits(lb.place(inner, place, dw, dh, PAD), *PARAMS[PARAM], dtype, False)
    if f == WARP:
        return shapes.warp_bits(orc, sf, cs, cr, W, H, job, dw, dh, MODE, PARAM, dtype, False)
    if sf != "P10":
        return persp.want_bits(orc, sf, cs, cr, W, H, job, dw, dh, BORDER, MODE, PARAM, dtype, False)
    key = (cs, cr, W, H, tuple(job), dw, dh)
    if key not in _PERSP_P10:
        _PERSP_P10[key] = persp_reference_u8(orc, "NV12", cs, cr, W, H, job, dw, dh, BORDER, MODE, rgb=p16.rgb_of(orc, "P10", cs, cr, W, H, 0))
        _PERSP_P10[key].setflags(write=False)
    return reference_bits(_PERSP_P10[key], *PARAMS[PARAM], dtype, False)


@pytest.mark.parametrize("row", cases.CASES, ids=[r["name"] for r in cases.CASES])
def test_every_job_holds_the_oracles_bits(capi, orc, row):
    cs, cr = MATRICES[cases.CASES.index(row) % 4]
    dev = shapes.dev_frame(orc, row["sf"], row["W"], row["H"], "roi" if row["family"] <= LETTERBOX else "warp")
    buf = make_buf(row)
    invoke(capi, row, dev, buf, cs, cr)
    got, intact = buf.frames()
    assert intact, row["name"] + ": bytes outside the jobs' elements were written"
    for i, job in enumerate(row["jobs"]):
        want = want_bits(capi, orc, row, job, cs, cr)
        assert_bits(got[i], hwc(want) if row["nhwc"] else want, f"{row['name']} job {i} {job}")


def child():
    from videoprocessingframework_amd import capi
    frames = {}
    for i, row in enumerate(cases.CASES):
        key = (row["sf"], row["W"], row["H"])
        if key not in frames:
            frames[key] = ZeroFrame(*key)
        buf = make_buf(row)
        print("ROW %d" % i, file=sys.stderr, flush=True)
        invoke(capi, row, frames[key], buf)
    print("ROW end", file=sys.stderr, flush=True)
    print("done")


def test_logged_labels_are_the_plans():
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, env=dict(os.environ, VPF_HIP_LOG="2"), timeout=300)
    assert r.returncode == 0 and "done" in r.stdout, r.stdout + r.stderr
    logged, row = {}, None
    for line in r.stderr.splitlines():
        if line.startswith("ROW "):
            row = line[4:]
            logged[row] = []
        elif line.startswith("libvpfhip: launch ") and row is not None:
            logged[row].append(line[len("libvpfhip: launch "):])
    wrong = [(case["name"], logged.get(str(i)), cases.labels(case)) for i, case in enumerate(cases.CASES) if logged.get(str(i)) != cases.labels(case)]
    assert not wrong, wrong


if __name__ == "__main__":
    child()
