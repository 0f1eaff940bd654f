"""Kernel times of the two forms of vpf_convert_warp_tensor (k_warp_strip against k_warp_gather) from a rocprofv3 kernel trace: what the
staged / gather break-even and the tile shape of k_convert_warp.hip are chosen from.  Host time is not in these numbers.

K = 64 jobs over four 1080p NV12 frames, f16, every case once under the default policy (the staged form wherever its strip fits the LDS limit)
and once with the gather form forced (VPF_TUNE_NV12_RGB_VARIANT = 9); the median of REPS dispatches per case, microseconds per region.  Cases: the footprints of
tools/warp_tensor_bench.py at 0 / 15 / 45 degrees, and a sweep of the scale factor (source pixels per destination pixel, per axis) into 224 x 224
at 0 and 30 degrees, and 2.7 x at 45 degrees, whose 62 KiB strip lies between the two LDS limits measured.  `--lib` measures another build of
the library (hipcc ... -DVPF_WARP_TILE_W=64 -DVPF_WARP_TILE_H=16, or -DVPF_WARP_STRIP_MAX_KIB=53, on k_convert_warp.hip, linked with the
other objects).

  python tools/warp_kernel_ab.py [--lib PATH] [--out FILE]          (runs itself under rocprofv3 --kernel-trace and reads the trace)"""
import argparse
import csv
import glob
import math
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, FRAMES, W, H, REPS = 64, 4, 1920, 1080, 21
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def cases():
    out = []
    for w, h, dw, dh in ((96, 192, 128, 256), (400, 300, 224, 224), (640, 640, 224, 224), (112, 112, 112, 112)):
        for deg in (0, 15, 45):
            out.append((f"{w}x{h} -> {dw}x{dh} {deg:2d} deg", w, h, dw, dh, deg))
    for s in (1.0, 1.25, 1.5, 1.75, 2.0, 2.5):
        for deg in (0, 30):
            side = int(round(224 * s))
            out.append((f"scale {s:4.2f} -> 224x224 {deg:2d} deg", side, side, 224, 224, deg))
    out.append(("scale 2.70 -> 224x224 45 deg", 605, 605, 224, 224, 45))
    return out


def matrices(w, h, dw, dh, deg):
    import numpy as np

    rng = np.random.default_rng(w * 31 + h)
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    sx, sy = w / dw, h / dh
    out = []
    for i in range(K):
        x, y = 2 * int(rng.integers(0, (W - w) // 2 + 1)), 2 * int(rng.integers(0, (H - h) // 2 + 1))
        cx, cy, ox, oy = x + 0.5 * w - 0.5, y + 0.5 * h - 0.5, 0.5 * dw - 0.5, 0.5 * dh - 0.5
        out.append((i % FRAMES, (c * sx, -s * sy, cx - (c * sx * ox - s * sy * oy), s * sx, c * sy, cy - (s * sx * ox + c * sy * oy))))
    return out


def child(lib):
    sys.path.insert(0, ROOT)
    import torch

    from videoprocessingframework_amd import capi

    if lib:
        capi.LIB_PATH = os.path.abspath(lib)
    dev = torch.device("cuda", 0)
    ex = capi.make_exec(torch.cuda.current_stream().cuda_stream)
    sp = (W + 255) // 256 * 256
    src = torch.randint(0, 256, (FRAMES, H * 3 // 2, sp), dtype=torch.uint8, device=dev)
    fdesc = [[(src[i].data_ptr(), sp), (src[i].data_ptr() + H * sp, sp)] for i in range(FRAMES)]
    norm = capi.make_tensor_norm(MEAN, STD, dtype=1)
    tiny = torch.zeros((3, 1, 1), dtype=torch.float16, device=dev)
    mark = capi.make_warps([(fdesc[0], [(tiny[c].data_ptr(), 2) for c in range(3)], (1, 0, 0, 0, 1, 0))])
    for _, w, h, dw, dh, deg in cases():
        out = torch.empty((K, 3, dh, dw), dtype=torch.float16, device=dev)
        warps = capi.make_warps([(fdesc[f], [(out[i, c].data_ptr(), 2 * dw) for c in range(3)], m) for i, (f, m) in enumerate(matrices(w, h, dw, dh, deg))])
        for variant in (0, 9):
            capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, 9)
            capi.convert_warp_tensor(ex, capi.NV12, 1, 0, W, H, 1, 1, mark, norm)  # the marker between groups: a one-workgroup gather dispatch
            capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, variant)
            for _ in range(REPS):
                capi.convert_warp_tensor(ex, capi.NV12, 1, 0, W, H, dw, dh, warps, norm)
            torch.cuda.synchronize()
    capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, 0)


def parent(lib, outfile):
    tmp = tempfile.mkdtemp(prefix="warp_ab_")
    cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__), "--child"] + (["--lib", lib] if lib else [])
    subprocess.run(cmd, check=True, timeout=600)
    files = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)
    assert files, f"no kernel trace under {tmp}"
    rows = []
    for row in csv.DictReader(open(files[0])):
        if "k_warp_" in row["Kernel_Name"]:
            rows.append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]), "strip" if "k_warp_strip" in row["Kernel_Name"] else "gather",
                         int(row["Grid_Size_X"]) * int(row["Grid_Size_Y"]) * int(row["Grid_Size_Z"])))
    rows.sort()
    groups = []
    for st, en, kind, grid in rows:
        if grid <= 256:
            groups.append([])
        else:
            groups[-1].append((st, en, kind))
    cs = cases()
    assert len(groups) == 2 * len(cs), (len(groups), len(cs))
    lines = [f"tools/warp_kernel_ab.py{' --lib ' + lib if lib else ''}: kernel time from rocprofv3 --kernel-trace, K = {K} jobs over {FRAMES} NV12 {W}x{H} frames, f16; "
             f"us per region, median of {REPS} calls (a call = every dispatch it made); staged = the default policy, gather = variant 9"]
    for i, c in enumerate(cs):
        per = []
        for g in (groups[2 * i], groups[2 * i + 1]):
            n = len(g) // REPS  # dispatches per call
            calls = [sum(en - st for st, en, _ in g[r * n:(r + 1) * n]) for r in range(REPS)]
            per.append((statistics.median(calls) / 1000.0 / K, n, sorted({k for _, _, k in g})))
        lines.append(f"{c[0]:34s} staged {per[0][0]:6.3f} ({per[0][1]} dispatch {'+'.join(per[0][2])})  gather {per[1][0]:6.3f}  staged / gather = {per[0][0] / per[1][0]:5.2f}")
    text = "\n".join(lines)
    print(text)
    if outfile:
        open(outfile, "w").write(text + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--lib")
    ap.add_argument("--out")
    a = ap.parse_args()
    child(a.lib) if a.child else parent(a.lib, a.out)
