"""The fused per-pixel remap into a tensor (vpf_convert_remap_tensor) against the chain it replaces, with the protocol of tools/persps_dev_bench.py
(bench.sustained: 300 ms pre-heat of the same calls, median of five >= 60 ms blocks, shader clock beside every number; one fresh process per run; the
forms interleaved per case): NV12 frames (BT.709 MPEG, ImageNet mean / std) through ONE shared barrel-distortion map (undistort_maps, k1 = -0.25),
1080p -> 1080p and 4K -> 640 x 640, batches of 1, 8 and 32 frames, f32 and f16:
  chain     vpf_convert_batch(NV12 -> RGB) + vpf_remap_batch + the torch chain (permute to NCHW, .float() / 255, (x - mean) / std, .to(dtype)): three
            steps and two intermediates of entries the library already had — the baseline
  fused     vpf_convert_remap_tensor, no hint (64 KiB of LDS per workgroup)
  hint      the same with max_step = maps_max_step of the maps
  per tap   the same under VPF_TUNE_NV12_RGB_VARIANT = 9 (no LDS: every tile samples per tap)
No number is promised: microseconds per frame as measured, fused / chain and staged / per tap beside them, every row where the fused entry or the
staged form loses named at the end.

  python tools/remap_tensor_bench.py [--out profiles/r25_remap_tensor.txt]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
SHAPES = [(1920, 1080, 1920, 1080), (3840, 2160, 640, 640)]
BATCHES = [1, 8, 32]
DTYPES = ["f32", "f16"]


def barrel(pnc, W, H, dw, dh, device):
    """the maps that undistort a barrel-distorted W x H frame into a dw x dh view of it"""
    f = 0.9 * W
    K = [[f, 0, (W - 1) / 2], [0, f, (H - 1) / 2], [0, 0, 1]]
    Kn = [[f * dw / W, 0, (dw - 1) / 2], [0, f * dh / H, (dh - 1) / 2], [0, 0, 1]]
    return pnc.undistort_maps(K, (-0.25, 0.06, 0.001, -0.0005, 0.0), (dw, dh), new_camera_matrix=Kn, device=device)


def measure():
    sys.path.insert(0, ROOT)
    import torch

    import bench
    from videoprocessingframework_amd import PytorchNvCodec as pnc
    from videoprocessingframework_amd import capi

    dev = torch.device("cuda", 0)
    tdt = {"f32": torch.float32, "f16": torch.float16}
    ex = capi.make_exec(torch.cuda.current_stream().cuda_stream)
    pci = bench.device_pci(0)
    mean_t = torch.tensor(MEAN, device=dev).view(1, 3, 1, 1)
    std_t = torch.tensor(STD, device=dev).view(1, 3, 1, 1)
    lines, lost = [], []
    for W, H, dw, dh in SHAPES:
        sp = (W + 255) // 256 * 256
        xm, ym = barrel(pnc, W, H, dw, dh, dev)
        step = pnc.maps_max_step(xm, ym)
        inside = float(((xm >= 0) & (xm <= W - 1) & (ym >= 0) & (ym <= H - 1)).float().mean())
        lines.append(f"{W}x{H} -> {dw}x{dh}: barrel map, maps_max_step {step:.3f}, {100 * inside:.1f} % of the pixels in range")
        for n in BATCHES:
            src = torch.randint(0, 256, (n, H * 3 // 2, sp), dtype=torch.uint8, device=dev)
            fdesc = [[(src[i].data_ptr(), sp), (src[i].data_ptr() + H * sp, sp)] for i in range(n)]
            rgb = torch.empty((n, H, 3 * W), dtype=torch.uint8, device=dev)
            rgb2 = torch.zeros((n, dh, 3 * dw), dtype=torch.uint8, device=dev)
            to_rgb = capi.make_batch([(fdesc[i], [(rgb[i].data_ptr(), 3 * W)]) for i in range(n)])
            to_map = capi.make_batch([([(rgb[i].data_ptr(), 3 * W)], [(rgb2[i].data_ptr(), 3 * dw)]) for i in range(n)])
            for dt in DTYPES:
                out = torch.empty((n, 3, dh, dw), dtype=tdt[dt], device=dev)
                e = out.element_size()
                norm = capi.make_tensor_norm(MEAN, STD, dtype={"f32": 0, "f16": 1}[dt])
                jobs = capi.make_remap_jobs([(fdesc[i], [(out[i, c].data_ptr(), dw * e) for c in range(3)], (xm.data_ptr(), 4 * dw), (ym.data_ptr(), 4 * dw))
                                             for i in range(n)])
                opts = {"fused": capi.make_remap_opts(), "hint": capi.make_remap_opts(max_step=step)}

                def chain():
                    capi.convert_batch(ex, capi.NV12, capi.RGB, 1, 0, W, H, to_rgb)
                    capi.remap_batch(ex, capi.RGB, W, H, xm.data_ptr(), 4 * dw, ym.data_ptr(), 4 * dw, dw, dh, to_map)
                    x = rgb2.view(n, dh, dw, 3).permute(0, 3, 1, 2).float() / 255.0
                    return ((x - mean_t) / std_t).to(tdt[dt])

                res = {"chain": bench.sustained(chain, pci=pci)}
                for name, o in opts.items():
                    res[name] = bench.sustained(lambda: capi.convert_remap_tensor(ex, capi.NV12, 1, 0, W, H, dw, dh, jobs, norm, o), pci=pci)
                prev = capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, 9)
                try:
                    res["per tap"] = bench.sustained(lambda: capi.convert_remap_tensor(ex, capi.NV12, 1, 0, W, H, dw, dh, jobs, norm, opts["fused"]), pci=pci)
                finally:
                    capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, prev)
                per = {k: r["us"] / n for k, r in res.items()}
                row = f"{W}x{H} -> {dw}x{dh} n={n:2d} {dt}"
                lines.append(f"{row}: " + "  ".join(
                    f"{k} {per[k]:8.2f} us/frame (spread {(max(res[k]['blocks_us']) - min(res[k]['blocks_us'])) / n:.2f}, sclk {res[k]['sclk_mhz']})" for k in res))
                ratios = {"fused / chain": per["fused"] / per["chain"], "hint / chain": per["hint"] / per["chain"], "fused / per tap": per["fused"] / per["per tap"],
                          "hint / per tap": per["hint"] / per["per tap"]}
                lines.append("    " + "   ".join(f"{k} = {v:5.2f}" for k, v in ratios.items()))
                lost += [f"{row} {k} = {v:.2f}" for k, v in ratios.items() if v > 1.0]
                print("\n".join(lines[-2:]), flush=True)
                del out
            del src, rgb, rgb2
            torch.cuda.empty_cache()
    lines.append("")
    lines.append("rows where the fused entry loses to the chain or a staged form to the per-tap form: " + ("none" if not lost else "; ".join(lost)))
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    a = ap.parse_args()
    head = ("tools/remap_tensor_bench.py: NV12 frames, BT.709 MPEG, ImageNet mean / std, one shared barrel map; microseconds per frame, median of five >= 60 ms "
            "blocks after 300 ms of pre-heat\n")
    text = head + measure()
    print(text.splitlines()[-1])
    if a.out:
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
