"""The fused multi-ROI affine warp into a normalised tensor (vpf_convert_warp_tensor) against the chain it replaces and against the axis-aligned
ROI entry, timed with the project's sustained-clock protocol (bench.sustained: 300 ms pre-heat of the same calls, median of five >= 60 ms
blocks, shader clock beside every number; one fresh process per run).

K = 64 jobs spread over four 1080p NV12 frames (BT.709 MPEG, ImageNet mean / std), f16 and f32, per footprint (w x h of the frame -> dw x dh) and
angle (0, 15, 45 degrees about the footprint's centre; the matrix maps destination pixel centres as vpf_resize does: m00 = s cos, m02 folds
0.5 s - 0.5 and the corner):
  warp    vpf_convert_warp_tensor, one call, default policy                                                           (`gather`: tuning variant 9)
  chain   what a user had before: one vpf_convert NV12 -> RGB per frame, K vpf_remap calls on PREBUILT device maps (their construction is not
          timed, in the chain's favour), then torch permute, cast and normalise; the warp call must be faster in every case
  rois    vpf_convert_resize_tensor_rois on the same axis-aligned footprints (0 degree rows only): warp / rois is recorded

  python tools/warp_tensor_bench.py [--out profiles/r10_warp_tensor.txt]"""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, FRAMES, W, H = 64, 4, 1920, 1080
SHAPES = [(96, 192, 128, 256), (400, 300, 224, 224), (640, 640, 224, 224), (112, 112, 112, 112)]  # the last one: a face crop
ANGLES = (0, 15, 45)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
DTYPES = ("f16", "f32")


def jobs_of(w, h, dw, dh, deg):
    """K (frame, rect, matrix): rect corners on an even grid inside the frame; the matrix rotates about the rect's centre by `deg` and scales by
    w / dw, h / dh with vpf_resize's pixel-centre convention"""
    import numpy as np

    rng = np.random.default_rng(w * 31 + h)
    out = []
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    sx, sy = w / dw, h / dh
    for i in range(K):
        x, y = 2 * int(rng.integers(0, (W - w) // 2 + 1)), 2 * int(rng.integers(0, (H - h) // 2 + 1))
        cx, cy = x + 0.5 * w - 0.5, y + 0.5 * h - 0.5  # centre of the footprint in pixel indices
        ox, oy = 0.5 * dw - 0.5, 0.5 * dh - 0.5        # centre of the destination
        m = (c * sx, -s * sy, cx - (c * sx * ox - s * sy * oy), s * sx, c * sy, cy - (s * sx * ox + c * sy * oy))
        out.append((i % FRAMES, (x, y, w, h), m))
    return out


def measure():
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    import bench
    from videoprocessingframework_amd import capi

    dev = torch.device("cuda", 0)
    tdt = {"f32": torch.float32, "f16": torch.float16}
    ex = capi.make_exec(torch.cuda.current_stream().cuda_stream)
    pci = bench.device_pci(0)
    sp = (W + 255) // 256 * 256
    src = torch.randint(0, 256, (FRAMES, H * 3 // 2, sp), dtype=torch.uint8, device=dev)
    fdesc = [[(src[i].data_ptr(), sp), (src[i].data_ptr() + H * sp, sp)] for i in range(FRAMES)]
    rgb = torch.empty((FRAMES, H, 3 * W), dtype=torch.uint8, device=dev)
    scale, bias = capi.norm_params(MEAN, STD)
    lines, ok = [], True
    for w, h, dw, dh in SHAPES:
        for deg in ANGLES:
            for dt in DTYPES:
                out = torch.empty((K, 3, dh, dw), dtype=tdt[dt], device=dev)
                e = out.element_size()
                dst = [[(out[i, c].data_ptr(), dw * e) for c in range(3)] for i in range(K)]
                norm = capi.make_tensor_norm(MEAN, STD, dtype={"f32": 0, "f16": 1}[dt])
                jobs = jobs_of(w, h, dw, dh, deg)
                warps = capi.make_warps([(fdesc[f], dst[i], m) for i, (f, _, m) in enumerate(jobs)])
                res = {"warp": bench.sustained(lambda: capi.convert_warp_tensor(ex, capi.NV12, 1, 0, W, H, dw, dh, warps, norm), pci=pci)}
                prev = capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, 9)
                res["gather"] = bench.sustained(lambda: capi.convert_warp_tensor(ex, capi.NV12, 1, 0, W, H, dw, dh, warps, norm), pci=pci)
                capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, prev)
                # the chain: maps prebuilt on the device (not timed), one conversion per frame, K remaps, torch permute + cast + normalise
                dx, dy = np.arange(dw, dtype=np.float32)[None, :], np.arange(dh, dtype=np.float32)[:, None]
                xm = torch.from_numpy(np.stack([(np.float32(m[0]) * dx + np.float32(m[1]) * dy) + np.float32(m[2]) for _, _, m in jobs])).to(dev)
                ym = torch.from_numpy(np.stack([(np.float32(m[3]) * dx + np.float32(m[4]) * dy) + np.float32(m[5]) for _, _, m in jobs])).to(dev)
                packed = torch.zeros((K, dh, 3 * dw), dtype=torch.uint8, device=dev)
                sc = torch.tensor(scale, dtype=torch.float32, device=dev).view(1, 3, 1, 1)
                bi = torch.tensor(bias, dtype=torch.float32, device=dev).view(1, 3, 1, 1)

                def run_chain():
                    for f in range(FRAMES):
                        capi.convert(ex, capi.NV12, capi.RGB, 1, 0, W, H, fdesc[f], [(rgb[f].data_ptr(), 3 * W)])
                    for i, (f, _, _) in enumerate(jobs):
                        capi.remap(ex, capi.RGB, W, H, (rgb[f].data_ptr(), 3 * W), xm[i].data_ptr(), 4 * dw, ym[i].data_ptr(), 4 * dw, dw, dh,
                                   (packed[i].data_ptr(), 3 * dw))
                    out.copy_(packed.view(K, dh, dw, 3).permute(0, 3, 1, 2).to(torch.float32) * sc + bi)

                res["chain"] = bench.sustained(run_chain, pci=pci)
                if deg == 0:
                    rois = capi.make_rois([(fdesc[f], dst[i], r) for i, (f, r, _) in enumerate(jobs)])
                    res["rois"] = bench.sustained(lambda: capi.convert_resize_tensor_rois(ex, capi.NV12, 1, 0, W, H, dw, dh, rois, norm), pci=pci)
                per = {k: r["us"] / K for k, r in res.items()}
                c1 = per["warp"] < per["chain"]
                ok = ok and c1
                lines.append(f"{w}x{h} -> {dw}x{dh} {deg:2d} deg {dt}: " + "  ".join(
                    f"{k} {per[k]:7.3f} us/region (spread {(max(res[k]['blocks_us']) - min(res[k]['blocks_us'])) / K:.3f}, sclk {res[k]['sclk_mhz']})" for k in res))
                lines.append(f"    chain / warp = {per['chain'] / per['warp']:6.2f}x [a: {'pass' if c1 else 'FAIL'}]   gather / warp = {per['gather'] / per['warp']:5.2f}"
                             + (f"   warp / rois = {per['warp'] / per['rois']:5.2f} [b: 1.25 was allowed the ROI entry]" if "rois" in per else ""))
                print("\n".join(lines[-2:]), flush=True)
                del out, xm, ym, packed
                torch.cuda.empty_cache()
    lines.append("")
    lines.append(f"a (faster than the convert + K remaps + torch chain): {'every case passes' if ok else 'SOME CASES FAIL'}")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    a = ap.parse_args()
    head = (f"tools/warp_tensor_bench.py: K = {K} jobs over {FRAMES} NV12 {W}x{H} frames, BT.709 MPEG, ImageNet mean / std; microseconds per region, "
            f"median of five >= 60 ms blocks after 300 ms of pre-heat\n")
    text = head + measure()
    print(text.splitlines()[-1])
    if a.out:
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
