"""The device-resident ROI entry (vpf_convert_resize_tensor_rois_dev) against the host-table entry it mirrors, with the protocol and the shapes of
tools/roi_tensor_bench.py (bench.sustained: 300 ms pre-heat of the same calls, median of five >= 60 ms blocks, shader clock beside every number; one
fresh process per run): K = 64 rectangles over four 1080p NV12 frames (BT.709 MPEG, ImageNet mean / std), f16 and f32, per rect shape:
  (a) host      vpf_convert_resize_tensor_rois, one call, as profiles/r09_roi_tensor.txt measures it
  (b) dev       vpf_convert_resize_tensor_rois_dev on the same rectangles, count = K
  (c) dev_spare the same with max_n = 128, count = 64: what 64 idle jobs cost (a workgroup that loads the count and leaves)
  (d) pipeline  the stage as a detector pipeline runs it — the boxes are produced on the GPU in every step (a device copy stands in for the NMS):
                boxes.cpu() + PytorchNvCodec.rois_to_normalized_tensor against PytorchNvCodec.device_rois_to_normalized_tensor, HOST-timed over blocks of
                steps with one synchronize at the end of a block (what the caller's thread waits for), median of five blocks
No number is promised: (b) / (a) and (c) / (b) are reported against the 1.25 x the ROI bench allows between two forms of the same work, (d) as measured.

  python tools/rois_dev_bench.py [--out profiles/r13_rois_dev.txt]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from roi_tensor_bench import DTYPES, FRAMES, H, K, MEAN, SHAPES, STD, W, rects_of  # noqa: E402

SPARE = 128


def pipeline_us(step, steps, blocks=5):
    """host microseconds per step: `blocks` blocks of `steps` steps, one synchronize at the end of each, the median block"""
    import torch

    for _ in range(max(8, steps // 4)):
        step()
    torch.cuda.synchronize()
    per = []
    for _ in range(blocks):
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
        per.append((time.perf_counter() - t0) * 1e6 / steps)
    per.sort()
    return per[len(per) // 2], per


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
    rng = np.random.default_rng(13)
    surfs = [up.UploadSingleFrame(rng.integers(0, 256, W * H * 3 // 2, dtype=np.uint8)).Clone(0) for _ in range(FRAMES)]
    cc = nvc.ColorspaceConversionContext(nvc.ColorSpace.BT_709, nvc.ColorRange.MPEG)
    torch.cuda.synchronize()
    lines, worst_ba, worst_cb = [], 0.0, 0.0
    for w, h, dw, dh in SHAPES:
        for dt in DTYPES:
            out = torch.empty((SPARE, 3, dh, dw), dtype=tdt[dt], device=dev)
            e = out.element_size()
            dst = [[(out[i, c].data_ptr(), dw * e) for c in range(3)] for i in range(K)]
            norm = capi.make_tensor_norm(MEAN, STD, dtype={"f32": 0, "f16": 1}[dt])
            rects = rects_of(w, h, False)
            rois = capi.make_rois([(fdesc[f], dst[i], (x, y, rw, rh)) for i, (f, x, y, rw, rh) in enumerate(rects)])
            boxes = torch.zeros((SPARE, 5), dtype=torch.int32)
            boxes[:K] = torch.tensor(rects, dtype=torch.int32)
            boxes = boxes.to(dev)
            count = torch.tensor([K], dtype=torch.int32, device=dev)
            t64 = capi.make_rois_dev(boxes.data_ptr(), K, dst[0], 3 * dh * dw * e, count.data_ptr())
            t128 = capi.make_rois_dev(boxes.data_ptr(), SPARE, dst[0], 3 * dh * dw * e, count.data_ptr())
            res = {}
            res["host"] = bench.sustained(lambda: capi.convert_resize_tensor_rois(ex, capi.NV12, 1, 0, W, H, dw, dh, rois, norm), pci=pci)
            res["dev"] = bench.sustained(lambda: capi.convert_resize_tensor_rois_dev(ex, capi.NV12, 1, 0, W, H, dw, dh, frames, t64, norm), pci=pci)
            res["dev_spare"] = bench.sustained(lambda: capi.convert_resize_tensor_rois_dev(ex, capi.NV12, 1, 0, W, H, dw, dh, frames, t128, norm), pci=pci)
            per = {k: r["us"] / K for k, r in res.items()}
            ba, cb = per["dev"] / per["host"], per["dev_spare"] / per["dev"]
            worst_ba, worst_cb = max(worst_ba, ba), max(worst_cb, cb)
            lines.append(f"{w}x{h} -> {dw}x{dh} {dt}: " + "  ".join(
                f"{k} {per[k]:7.3f} us/region (spread {(max(res[k]['blocks_us']) - min(res[k]['blocks_us'])) / K:.3f}, sclk {res[k]['sclk_mhz']})" for k in res))
            # (d) the stage in a pipeline: the producer of the boxes runs on the GPU in every step
            rs = nvc.PySurfaceConvertResizer(W, H, nvc.PixelFormat.NV12, dw, dh, nvc.PixelFormat.RGB_PLANAR, 0, torch.cuda.current_stream().cuda_stream)
            live = boxes[:K].clone()
            o64 = out[:K]

            def via_host():
                live.copy_(boxes[:K])  # the NMS's last kernel
                pnc.rois_to_normalized_tensor(rs, surfs, live.cpu(), MEAN, STD, dtype=tdt[dt], out=o64, cc_ctx=cc)

            def via_device():
                live.copy_(boxes[:K])
                pnc.device_rois_to_normalized_tensor(rs, surfs, live, MEAN, STD, count=count, dtype=tdt[dt], out=o64, cc_ctx=cc)

            steps = 400
            ph, ph_all = pipeline_us(via_host, steps)
            pd, pd_all = pipeline_us(via_device, steps)
            lines.append(f"    dev / host = {ba:5.2f}   dev_spare / dev = {cb:5.2f}   (1.25 allowed between two forms of the same work)   "
                         f"pipeline, host us per step: boxes.cpu() + rois_to_normalized_tensor {ph:7.1f} (blocks {min(ph_all):.1f} .. {max(ph_all):.1f})  "
                         f"device_rois_to_normalized_tensor {pd:7.1f} (blocks {min(pd_all):.1f} .. {max(pd_all):.1f})  host / device = {ph / pd:5.2f}")
            print("\n".join(lines[-2:]), flush=True)
            del out, o64, rs
            torch.cuda.empty_cache()
    lines.append("")
    lines.append(f"largest dev / host = {worst_ba:.2f}, largest dev_spare / dev = {worst_cb:.2f} (kernel time per region; 1.25 is what tools/roi_tensor_bench.py allows "
                 f"between two forms of the same work)")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    a = ap.parse_args()
    head = (f"tools/rois_dev_bench.py: K = {K} rects over {FRAMES} NV12 {W}x{H} frames, BT.709 MPEG, ImageNet mean / std; (a)-(c) microseconds per region, median "
            f"of five >= 60 ms blocks after 300 ms of pre-heat; (d) host microseconds per pipeline step of {K} regions, median of five blocks of 400 steps\n")
    text = head + measure()
    print(text.splitlines()[-1])
    if a.out:
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
