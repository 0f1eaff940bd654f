"""The device-resident warp entry (vpf_convert_warp_tensor_dev) against the host-table entry it mirrors, with the protocol, the shapes and the matrices
of tools/warp_tensor_bench.py (bench.sustained: 300 ms pre-heat of the same calls, median of five >= 60 ms blocks, shader clock beside every number;
one fresh process per run; host and device entries interleaved per case): K = 64 jobs over four 1080p NV12 frames (BT.709 MPEG, ImageNet mean / std),
f16 and f32, per footprint and angle (0 / 15 / 45 degrees):
  (a) host      vpf_convert_warp_tensor, one call, as profiles/r10_warp_tensor.txt measures it (its kernels' code objects are the parent's)
      dev       vpf_convert_warp_tensor_dev on the same matrices, count = K, max_step = the jobs' true |m00| + |m01| / |m10| + |m11|
      dev0      the same with max_step = 0: what the 64 KiB default costs small warps
  (c) dev_spare `dev` with max_n = 128, count = 64: what 64 idle jobs cost (a workgroup that loads the count and leaves)
  (b) pipeline  the stage as an alignment pipeline runs it — the matrices are produced on the GPU in every step (a device copy stands in for the
                landmark network's last kernel): matrices.cpu() + PytorchNvCodec.warps_to_normalized_tensor against
                PytorchNvCodec.device_warps_to_normalized_tensor, HOST-timed over blocks of 400 steps with one synchronize at the end of a block
                (what the caller's thread waits for), median of five blocks
No number is promised: dev / host, dev0 / host and dev_spare / dev are reported against the 1.25 x the ROI bench allows between two forms of the same
work, (b) as measured.

  python tools/warps_dev_bench.py [--out profiles/r14_warps_dev.txt]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from rois_dev_bench import pipeline_us  # noqa: E402
from warp_tensor_bench import ANGLES, DTYPES, FRAMES, H, K, MEAN, SHAPES, STD, W, jobs_of  # noqa: E402

SPARE = 128


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
    lines, worst = [], {"dev / host": 0.0, "dev0 / host": 0.0, "dev_spare / dev": 0.0}
    for w, h, dw, dh in SHAPES:
        for deg in ANGLES:
            for dt in DTYPES:
                out = torch.empty((SPARE, 3, dh, dw), dtype=tdt[dt], device=dev)
                e = out.element_size()
                dst = [[(out[i, c].data_ptr(), dw * e) for c in range(3)] for i in range(K)]
                norm = capi.make_tensor_norm(MEAN, STD, dtype={"f32": 0, "f16": 1}[dt])
                jobs = jobs_of(w, h, dw, dh, deg)
                warps = capi.make_warps([(fdesc[f], dst[i], m) for i, (f, _, m) in enumerate(jobs)])
                mats = torch.zeros((SPARE, 6), dtype=torch.float32)
                mats[:K] = torch.tensor([m for _, _, m in jobs], dtype=torch.float64).to(torch.float32)
                step = float(max(max(abs(float(r[0])) + abs(float(r[1])), abs(float(r[3])) + abs(float(r[4]))) for r in mats[:K])) * (1 + 2.0 ** -20)
                mats = mats.to(dev)
                index = torch.zeros(SPARE, dtype=torch.int32)
                index[:K] = torch.tensor([f for f, _, _ in jobs], dtype=torch.int32)
                index = index.to(dev)
                count = torch.tensor([K], dtype=torch.int32, device=dev)
                job = 3 * dh * dw * e
                tabs = {"dev": capi.make_warps_dev(mats.data_ptr(), K, dst[0], job, index.data_ptr(), count.data_ptr(), max_step=step),
                        "dev0": capi.make_warps_dev(mats.data_ptr(), K, dst[0], job, index.data_ptr(), count.data_ptr(), max_step=0.0),
                        "dev_spare": capi.make_warps_dev(mats.data_ptr(), SPARE, dst[0], job, index.data_ptr(), count.data_ptr(), max_step=step)}
                res = {"host": bench.sustained(lambda: capi.convert_warp_tensor(ex, capi.NV12, 1, 0, W, H, dw, dh, warps, norm), pci=pci)}
                for name, t in tabs.items():
                    res[name] = bench.sustained(lambda: capi.convert_warp_tensor_dev(ex, capi.NV12, 1, 0, W, H, dw, dh, frames, t, norm), pci=pci)
                per = {k: r["us"] / K for k, r in res.items()}
                ratios = {"dev / host": per["dev"] / per["host"], "dev0 / host": per["dev0"] / per["host"], "dev_spare / dev": per["dev_spare"] / per["dev"]}
                for k, v in ratios.items():
                    worst[k] = max(worst[k], v)
                lines.append(f"{w}x{h} -> {dw}x{dh} {deg:2d} deg {dt} (max_step {step:.3f}): " + "  ".join(
                    f"{k} {per[k]:7.3f} us/region (spread {(max(res[k]['blocks_us']) - min(res[k]['blocks_us'])) / K:.3f}, sclk {res[k]['sclk_mhz']})" for k in res))
                # (b) the stage in a pipeline: the producer of the matrices runs on the GPU in every step
                rs = nvc.PySurfaceConvertResizer(W, H, nvc.PixelFormat.NV12, dw, dh, nvc.PixelFormat.RGB_PLANAR, 0, torch.cuda.current_stream().cuda_stream)
                live = mats[:K].reshape(K, 2, 3).clone()
                idx_host = [f for f, _, _ in jobs]
                idx_dev = index[:K]
                o64 = out[:K]

                def via_host():
                    live.copy_(mats[:K].view(K, 2, 3))  # the landmark stage's last kernel
                    pnc.warps_to_normalized_tensor(rs, surfs, idx_host, live.cpu(), MEAN, STD, dtype=tdt[dt], out=o64, cc_ctx=cc)

                def via_device():
                    live.copy_(mats[:K].view(K, 2, 3))
                    pnc.device_warps_to_normalized_tensor(rs, surfs, live, MEAN, STD, surface_index=idx_dev, count=count, max_step=step, dtype=tdt[dt], out=o64,
                                                          cc_ctx=cc)

                ph, ph_all = pipeline_us(via_host, 400)
                pd, pd_all = pipeline_us(via_device, 400)
                lines.append("    " + "   ".join(f"{k} = {v:5.2f}" for k, v in ratios.items()) + "   (1.25 allowed between two forms of the same work)   "
                             f"pipeline, host us per step: matrices.cpu() + warps_to_normalized_tensor {ph:7.1f} (blocks {min(ph_all):.1f} .. {max(ph_all):.1f})  "
                             f"device_warps_to_normalized_tensor {pd:7.1f} (blocks {min(pd_all):.1f} .. {max(pd_all):.1f})  host / device = {ph / pd:5.2f}")
                print("\n".join(lines[-2:]), flush=True)
                del out, o64, rs
                torch.cuda.empty_cache()
    lines.append("")
    lines.append("largest " + ", ".join(f"{k} = {v:.2f}" for k, v in worst.items()) + " (kernel time per region; 1.25 is what tools/roi_tensor_bench.py allows "
                 "between two forms of the same work)")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    a = ap.parse_args()
    head = (f"tools/warps_dev_bench.py: K = {K} jobs over {FRAMES} NV12 {W}x{H} frames, BT.709 MPEG, ImageNet mean / std; (a), (c) microseconds per region, median "
            f"of five >= 60 ms blocks after 300 ms of pre-heat; (b) host microseconds per pipeline step of {K} regions, median of five blocks of 400 steps\n")
    text = head + measure()
    print(text.splitlines()[-1])
    if a.out:
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
