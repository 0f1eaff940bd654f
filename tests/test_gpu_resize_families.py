"""Which kernel a plain resize takes is policy, and policy regressions are silent (same pixels): ONE child process runs every row of
tests/cases_resize_families.py under VPF_HIP_LOG=2, checks the bytes of every frame against the oracle and prints a marker per row; the
test then asserts the exact selection labels the library logged for each row, in launch order.  (The same table is checked against the
plan alone, without a device, in tests/test_resize_plan_cpu.py.)"""
import os
import subprocess
import sys

import pytest

from cases_resize_families import CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child():
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import torch

    import oracle
    from gpu_util import LaidOutPlanes, assert_planes_equal, stream_handle
    from videoprocessingframework_amd import capi
    ex = capi.make_exec(stream_handle())
    keys = (capi.TUNE_NV12_RGB_VARIANT, capi.TUNE_RESIZE_TILE, capi.TUNE_RESIZE_BAND, capi.TUNE_RESIZE_MFMA)
    for i, (name, fmt, interp, sw, sh, dw, dh, n, knobs, off, _) in enumerate(CASES):
        srcs = [oracle.synth(fmt, sw, sh, 2020 + 7 * i + f) for f in range(n)]
        wants = [oracle.resize(fmt, interp, sw, sh, s, dw, dh, oracle.FP32)[1] for s in srcs]
        offs = off if isinstance(off, tuple) else (off,) * len(srcs[0])
        S = [LaidOutPlanes(s, [(256, 0, o) for o in offs]) for s in srcs]
        D = [LaidOutPlanes(oracle.alloc(fmt, dw, dh), [(256, 0, 0)] * len(offs)) for _ in range(n)]
        print("ROW %d" % i, file=sys.stderr, flush=True)
        try:
            for key, v in zip(keys, knobs):
                assert capi.set_tuning(key, v) >= 0, (name, key, v)
            if n == 1:
                capi.resize(ex, fmt, interp, sw, sh, S[0].desc(), dw, dh, D[0].desc())
            else:
                capi.resize_batch(ex, fmt, interp, sw, sh, dw, dh, capi.make_batch([(s.desc(), d.desc()) for s, d in zip(S, D)]))
            torch.cuda.synchronize()
        finally:
            for key in keys:
                capi.set_tuning(key, 0)
        for f in range(n):
            got, intact = D[f].download()
            assert intact, (name, f)
            assert_planes_equal(got, wants[f], "%s, frame %d" % (name, f))
    print("ROW end", file=sys.stderr, flush=True)
    print("done")


@pytest.mark.gpu
def test_every_family_is_selected_and_writes_the_oracles_bytes():
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, env=dict(os.environ, VPF_HIP_LOG="2"), timeout=300)
    assert r.returncode == 0 and "done" in r.stdout, r.stdout + r.stderr
    logged = {}
    row = None
    for line in r.stderr.splitlines():
        if line.startswith("ROW "):
            row = line[4:]
            logged[row] = []
        elif line.startswith("libvpfhip: launch ") and row is not None:
            logged[row].append(line[len("libvpfhip: launch "):])
    wrong = [(case[0], logged[str(i)]) for i, case in enumerate(CASES) if logged[str(i)] != case[-1]]
    assert not wrong, wrong


if __name__ == "__main__":
    child()
