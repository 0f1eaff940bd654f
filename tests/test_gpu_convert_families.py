"""Which kernel a conversion takes is policy, and policy regressions are silent (same pixels): ONE child process runs every row of
tests/cases_convert_families.py under VPF_HIP_LOG=2, checks the bytes of every frame against the oracle and prints a marker per row; the
test then asserts the exact selection labels the library logged for each row, in launch order.  (The same table is checked against the
plan alone, without a device, in tests/test_convert_plan_cpu.py.)"""
import os
import subprocess
import sys

import pytest

from cases_convert_families import CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child():
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import numpy as np
    import torch

    import oracle
    import test_gpu_tensor_in as tin
    from gpu_util import LaidOutPlanes, assert_planes_equal, stream_handle
    from videoprocessingframework_amd import capi
    ex = {0: capi.make_exec(stream_handle()), 1: capi.make_exec(stream_handle(), flags=capi.EXEC_DST_REUSED)}

    def laid_out(planes, off):
        return LaidOutPlanes(planes, [(256, 0, off)] * len(planes))

    for i, (name, entry, src, dst, w, h, n, knob, reused, soff, doff, _) in enumerate(CASES):
        if entry == "convert":
            cs, cr = next((cs, cr) for cs, cr in ((1, 0), (0, 1)) if capi.convert_supported(src, dst, cs, cr))
            srcs = [oracle.synth(src, w, h, 3030 + 7 * i + f) for f in range(n)]
            wants = []
            for s in srcs:
                st, want = oracle.convert(src, dst, cs, cr, w, h, s, oracle.FP32)
                assert st == 0, name
                wants.append(want)
            S = [laid_out(s, soff) for s in srcs]
            descs = [s.desc() for s in S]
        else:
            dtype, nhwc, bgr = src
            cr, e = 1, tin.ELEM[dtype]
            scale, bias = tin.denorm_scale_bias_f32(*tin.PARAMS["imagenet"])
            ins = [tin.tensor_input(w, h, 3030 + 7 * i + f, "imagenet", dtype) for f in range(n)]
            wants = [tin.reference(oracle, wide, scale, bias, bgr, cr, "NV12" if dst == capi.NV12 else "YUV420") for _, wide in ins]
            if nhwc:   # ONE interleaved plane [h, w, 3] per frame
                S = [laid_out([t.permute(1, 2, 0).contiguous().view(torch.uint8).numpy().reshape(h, 3 * w * e)], soff * e) for t, _ in ins]
                descs = [s.desc() + [(0, 0), (0, 0)] for s in S]
            else:
                S = [laid_out([p for p in t.contiguous().view(torch.uint8).numpy().reshape(3, h, w * e)], soff * e) for t, _ in ins]
                descs = [s.desc() for s in S]
            dn = capi.make_tensor_denorm(dtype=dtype, bgr=bgr, scale=[float(v) for v in scale], bias=[float(v) for v in bias], nhwc=nhwc)
        D = [laid_out(oracle.alloc(dst, w, h), doff) for _ in range(n)]
        print("ROW %d" % i, file=sys.stderr, flush=True)
        try:
            assert capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, knob) >= 0, (name, knob)
            if entry == "convert" and n == 1:
                capi.convert(ex[reused], src, dst, cs, cr, w, h, descs[0], D[0].desc())
            elif entry == "convert":
                capi.convert_batch(ex[reused], src, dst, cs, cr, w, h, capi.make_batch([(s, d.desc()) for s, d in zip(descs, D)]))
            elif n == 1:
                capi.tensor_convert(ex[0], dst, 0, cr, w, h, descs[0], D[0].desc(), dn)
            else:
                capi.tensor_convert_batch(ex[0], dst, 0, cr, w, h, capi.make_batch([(s, d.desc()) for s, d in zip(descs, D)]), dn)
            torch.cuda.synchronize()
        finally:
            capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, 0)
        for f in range(n):
            got, intact = D[f].download()
            assert intact, (name, f)
            assert_planes_equal(got, [np.asarray(p) for p in wants[f]], "%s, frame %d" % (name, f))
    print("ROW end", file=sys.stderr, flush=True)
    print("done")


@pytest.mark.gpu
def test_every_form_is_selected_and_writes_the_oracles_bytes():
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
