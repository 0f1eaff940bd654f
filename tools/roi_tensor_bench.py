"""The fused multi-ROI crop + resize into a normalised tensor (vpf_convert_resize_tensor_rois) against the two entries it is measured by, timed with
the project's sustained-clock protocol (bench.sustained: 300 ms pre-heat of the same calls, median of five >= 60 ms blocks, shader clock beside
every number; one fresh process per run).

K = 64 rectangles spread over four 1080p NV12 frames (BT.709 MPEG, ImageNet mean / std), f16 and f32, per rect shape:
  rois    vpf_convert_resize_tensor_rois, one call                                                   (odd-offset rects too: `rois_odd`)
  lone    the route a user had before: K lone vpf_convert_resize_tensor calls on plane pointers advanced to the rect's corner (legal for even
          offsets only: these rects are even); the ROI call must be faster in every case
  batch   the same-shape yardstick: vpf_convert_resize_tensor_batch on K standalone frames of w x h -> dw x dh (16-B aligned rows, one scale
          factor per launch); the ROI call is allowed 1.25 x its time per region

  python tools/roi_tensor_bench.py [--out profiles/r09_roi_tensor.txt]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, FRAMES, W, H = 64, 4, 1920, 1080
SHAPES = [(96, 192, 128, 256), (400, 300, 224, 224), (640, 640, 224, 224), (1500, 900, 224, 224)]  # the last one takes the gather form
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
DTYPES = ("f16", "f32")


def rects_of(w, h, odd):
    """K rects of w x h spread over the frames on a grid of even corners (`odd`: every corner moved by (1, 1) where it fits, else (-1, -1))"""
    import numpy as np

    rng = np.random.default_rng(w * 31 + h)
    out = []
    for i in range(K):
        x, y = 2 * int(rng.integers(0, (W - w) // 2 + 1)), 2 * int(rng.integers(0, (H - h) // 2 + 1))
        if odd:
            x, y = (x + 1 if x + 1 + w <= W else x - 1), (y + 1 if y + 1 + h <= H else y - 1)
        out.append((i % FRAMES, x, y, w, h))
    return out


def measure():
    sys.path.insert(0, ROOT)
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
    lines, ok1, ok2 = [], True, True
    for w, h, dw, dh in SHAPES:
        for dt in DTYPES:
            out = torch.empty((K, 3, dh, dw), dtype=tdt[dt], device=dev)
            e = out.element_size()
            dst = [[(out[i, c].data_ptr(), dw * e) for c in range(3)] for i in range(K)]
            norm = capi.make_tensor_norm(MEAN, STD, dtype={"f32": 0, "f16": 1}[dt])
            res = {}
            for leg, odd in (("rois", False), ("rois_odd", True)):
                rois = capi.make_rois([(fdesc[f], dst[i], (x, y, rw, rh)) for i, (f, x, y, rw, rh) in enumerate(rects_of(w, h, odd))])
                res[leg] = bench.sustained(lambda rois=rois: capi.convert_resize_tensor_rois(ex, capi.NV12, 1, 0, W, H, dw, dh, rois, norm), pci=pci)
            # the lone route: plane pointers advanced to the (even) corner, one call per rect
            lone = [([(fdesc[f][0][0] + y * sp + x, sp), (fdesc[f][1][0] + (y // 2) * sp + x, sp)], dst[i]) for i, (f, x, y, _, _) in enumerate(rects_of(w, h, False))]
            lone = [(capi.planes(s), capi.planes(d)) for s, d in lone]

            def run_lone():
                for s, d in lone:
                    capi.convert_resize_tensor(ex, capi.NV12, 1, 0, w, h, s, dw, dh, d, norm)

            res["lone"] = bench.sustained(run_lone, pci=pci)
            # the yardstick: K standalone w x h frames, 256-B pitched
            p = (w + 255) // 256 * 256
            alone = torch.randint(0, 256, (K, h * 3 // 2 + 1, p), dtype=torch.uint8, device=dev)
            bt = capi.make_batch([([(alone[i].data_ptr(), p), (alone[i].data_ptr() + h * p, p)], dst[i]) for i in range(K)])
            res["batch"] = bench.sustained(lambda: capi.convert_resize_tensor_batch(ex, capi.NV12, 1, 0, w, h, dw, dh, bt, norm), pci=pci)
            per = {k: r["us"] / K for k, r in res.items()}
            c1, c2 = per["rois"] < per["lone"], per["rois"] <= 1.25 * per["batch"]
            ok1, ok2 = ok1 and c1, ok2 and c2
            lines.append(f"{w}x{h} -> {dw}x{dh} {dt}: " + "  ".join(
                f"{k} {per[k]:7.3f} us/region (spread {(max(res[k]['blocks_us']) - min(res[k]['blocks_us'])) / K:.3f}, sclk {res[k]['sclk_mhz']})" for k in res))
            lines.append(f"    lone / rois = {per['lone'] / per['rois']:6.2f}x [1: {'pass' if c1 else 'FAIL'}]   rois / batch = {per['rois'] / per['batch']:5.2f} "
                         f"(allowed 1.25) [2: {'pass' if c2 else 'MISS'}]   rois_odd / rois = {per['rois_odd'] / per['rois']:5.2f}")
            print("\n".join(lines[-2:]), flush=True)
            del out, alone
            torch.cuda.empty_cache()
    lines.append("")
    lines.append(f"1 (faster than K lone calls): {'every case passes' if ok1 else 'SOME CASES FAIL'};  2 (within 1.25 x the same-shape batch): "
                 f"{'every case passes' if ok2 else 'some cases miss (DESIGN.md 4.8)'}")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    a = ap.parse_args()
    head = (f"tools/roi_tensor_bench.py: K = {K} rects over {FRAMES} NV12 {W}x{H} frames, BT.709 MPEG, ImageNet mean / std; microseconds per region, "
            f"median of five >= 60 ms blocks after 300 ms of pre-heat\n")
    text = head + measure()
    print(text.splitlines()[-1])
    if a.out:
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
