"""The device-resident letterbox entry (vpf_convert_letterbox_tensor_dev) against the host-table entry it mirrors, with the protocol of
tools/rois_dev_bench.py (bench.sustained: 300 ms pre-heat of the same calls, median of five >= 60 ms blocks, shader clock beside every number; one
fresh process per run): K = 64 rectangles over four 1080p NV12 frames (BT.709 MPEG, ImageNet mean / std, pad 114), f16 and f32, per rect shape, each
fitted into 128 x 256 (ReID) or 224 x 224:
  (a) host      vpf_convert_letterbox_tensor on the same rectangles with vpf_letterbox_fit's placements, one call: the baseline
      dev       vpf_convert_letterbox_tensor_dev, dst_rects = NULL (the kernel fits), count = K
  (c) dev_spare the same with max_n = 256, count = 64: what 192 idle jobs cost (a workgroup that loads the count and leaves)
  (d) dev_tap   dev under VPF_TUNE_NV12_RGB_VARIANT = 9: the dispatch takes no LDS and every tile samples per tap — what the per-tap form costs when
                the staged form's LDS does not bound the workgroups per CU
  (b) pipeline  the stage as a detector pipeline runs it — the boxes are produced on the GPU in every step (a device copy stands in for the NMS):
                boxes.cpu() + PytorchNvCodec.letterbox_to_normalized_tensor (sync, copy, table build, host-table entry) against
                PytorchNvCodec.device_letterbox_to_normalized_tensor, HOST-timed over blocks of steps with one synchronize at the end of a block (what
                the caller's thread waits for), median of five blocks
No number is promised: dev / host is reported against the band the device-ROI entry showed against its own host-table entry (1.05 - 1.32 x,
profiles/r13_rois_dev.txt) plus the spread between this tool's own blocks; dev_spare / dev and (b) as measured.

  python tools/letterbox_dev_bench.py [--out profiles/r17_letterbox_dev.txt]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from roi_tensor_bench import DTYPES, FRAMES, H, K, MEAN, STD, W, rects_of  # noqa: E402
from rois_dev_bench import pipeline_us  # noqa: E402

SPARE = 256
PAD = (114, 114, 114)
# (w, h, dw, dh): a box of the destination's aspect (nothing padded), a squarer one (side bars), a flat one (bars above and below); 224 x 224 likewise,
# the last one a large down-scale (per tap)
SHAPES = [(96, 192, 128, 256), (150, 200, 128, 256), (200, 120, 128, 256), (400, 300, 224, 224), (300, 400, 224, 224), (1500, 900, 224, 224)]
BAND = (1.05, 1.32)


def measure():
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    import bench
    from videoprocessingframework_amd import capi

    sys.path.insert(0, os.path.join(ROOT, "videoprocessingframework_amd"))
    import PyNvCodec as nvc
    from videoprocessingframework_amd import PytorchNvCodec as pnc

    dev = torch.device("cuda", 0)
    tdt = {"f32": torch.float32, "f16": torch.float16}
    ex = capi.make_exec(torch.cuda.current_stream().cuda_stream)
    pci = bench.device_pci(0)
    sp = (W + 255) // 256 * 256
    src = torch.randint(0, 256, (FRAMES, H * 3 // 2, sp), dtype=torch.uint8, device=dev)
    fdesc = [[(src[i].data_ptr(), sp), (src[i].data_ptr() + H * sp, sp)] for i in range(FRAMES)]
    frames = capi.make_frame_srcs(fdesc)
    up = nvc.PyFrameUploader(W, H, nvc.PixelFormat.NV12, 0)
    rng = np.random.default_rng(17)
    surfs = [up.UploadSingleFrame(rng.integers(0, 256, W * H * 3 // 2, dtype=np.uint8)).Clone(0) for _ in range(FRAMES)]
    cc = nvc.ColorspaceConversionContext(nvc.ColorSpace.BT_709, nvc.ColorRange.MPEG)
    opts = capi.make_letterbox_opts(PAD)
    torch.cuda.synchronize()
    lines, worst, worst_spread, worst_spare = [], 0.0, 0.0, 0.0
    for w, h, dw, dh in SHAPES:
        for dt in DTYPES:
            out = torch.empty((SPARE, 3, dh, dw), dtype=tdt[dt], device=dev)
            e = out.element_size()
            dst = [[(out[i, c].data_ptr(), dw * e) for c in range(3)] for i in range(K)]
            norm = capi.make_tensor_norm(MEAN, STD, dtype={"f32": 0, "f16": 1}[dt])
            rects = rects_of(w, h, False)
            fit = capi.letterbox_fit(w, h, dw, dh)
            jobs = capi.make_letterbox_jobs([(fdesc[f], dst[i], (x, y, rw, rh), fit) for i, (f, x, y, rw, rh) in enumerate(rects)])
            boxes = torch.zeros((SPARE, 5), dtype=torch.int32)
            boxes[:K] = torch.tensor(rects, dtype=torch.int32)
            boxes = boxes.to(dev)
            count = torch.tensor([K], dtype=torch.int32, device=dev)
            t64 = capi.make_letterbox_dev(boxes.data_ptr(), K, dst[0], 3 * dh * dw * e, count.data_ptr())
            tsp = capi.make_letterbox_dev(boxes.data_ptr(), SPARE, dst[0], 3 * dh * dw * e, count.data_ptr())
            res = {}
            res["host"] = bench.sustained(lambda: capi.convert_letterbox_tensor(ex, capi.NV12, 1, 0, W, H, dw, dh, jobs, norm, opts), pci=pci)
            res["dev"] = bench.sustained(lambda: capi.convert_letterbox_tensor_dev(ex, capi.NV12, 1, 0, W, H, dw, dh, frames, t64, norm, opts), pci=pci)
            res["dev_spare"] = bench.sustained(lambda: capi.convert_letterbox_tensor_dev(ex, capi.NV12, 1, 0, W, H, dw, dh, frames, tsp, norm, opts), pci=pci)
            prev = capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, 9)
            try:
                res["dev_tap"] = bench.sustained(lambda: capi.convert_letterbox_tensor_dev(ex, capi.NV12, 1, 0, W, H, dw, dh, frames, t64, norm, opts), pci=pci)
            finally:
                capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, prev)
            per = {k: r["us"] / K for k, r in res.items()}
            spread = {k: (max(r["blocks_us"]) - min(r["blocks_us"])) / K for k, r in res.items()}
            ba, cb = per["dev"] / per["host"], per["dev_spare"] / per["dev"]
            rel = (spread["dev"] + spread["host"]) / per["host"]
            if ba > worst:
                worst, worst_spread = ba, rel
            worst_spare = max(worst_spare, cb)
            lines.append(f"{w}x{h} -> {dw}x{dh} (picture {fit[2]}x{fit[3]} at {fit[0]},{fit[1]}) {dt}: " + "  ".join(
                f"{k} {per[k]:7.3f} us/region (spread {spread[k]:.3f}, sclk {res[k]['sclk_mhz']})" for k in res))
            # (b) the stage in a pipeline: the producer of the boxes runs on the GPU in every step
            rs = nvc.PySurfaceConvertResizer(W, H, nvc.PixelFormat.NV12, dw, dh, nvc.PixelFormat.RGB_PLANAR, 0, torch.cuda.current_stream().cuda_stream)
            live = boxes[:K].clone()
            o64 = out[:K]

            def via_host():
                live.copy_(boxes[:K])  # the NMS's last kernel
                pnc.letterbox_to_normalized_tensor(rs, surfs, MEAN, STD, rois=live.cpu(), pad=PAD, dtype=tdt[dt], out=o64, cc_ctx=cc)

            def via_device():
                live.copy_(boxes[:K])
                pnc.device_letterbox_to_normalized_tensor(rs, surfs, live, MEAN, STD, count=count, pad=PAD, dtype=tdt[dt], out=o64, cc_ctx=cc)

            steps = 400
            ph, ph_all = pipeline_us(via_host, steps)
            pd, pd_all = pipeline_us(via_device, steps)
            lines.append(f"    dev / host = {ba:5.2f} (blocks' spread of the two, relative: {rel:4.2f})   dev_spare / dev = {cb:5.2f}   "
                         f"pipeline, host us per step: boxes.cpu() + letterbox_to_normalized_tensor {ph:7.1f} (blocks {min(ph_all):.1f} .. {max(ph_all):.1f})  "
                         f"device_letterbox_to_normalized_tensor {pd:7.1f} (blocks {min(pd_all):.1f} .. {max(pd_all):.1f})  host / device = {ph / pd:5.2f}")
            print("\n".join(lines[-2:]), flush=True)
            del out, o64, rs
            torch.cuda.empty_cache()
    lines.append("")
    lines.append(f"largest dev / host = {worst:.2f} (its blocks' relative spread {worst_spread:.2f}; the device-ROI entry's band against its host-table entry: "
                 f"{BAND[0]:.2f} - {BAND[1]:.2f}), largest dev_spare / dev = {worst_spare:.2f} (kernel time per region)")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    a = ap.parse_args()
    head = (f"tools/letterbox_dev_bench.py: K = {K} rects over {FRAMES} NV12 {W}x{H} frames, BT.709 MPEG, ImageNet mean / std, pad {PAD[0]}; (a), (c), (d) microseconds "
            f"per region, median of five >= 60 ms blocks after 300 ms of pre-heat; (b) host microseconds per pipeline step of {K} regions, median of five "
            f"blocks of 400 steps\n")
    text = head + measure()
    print(text.splitlines()[-1])
    if a.out:
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
