"""The antialiased letterbox into the tensor (vpf_convert_letterbox_tensor_aa) against the chain it replaces, against the bare-bilinear entry and
against its own per-tap form, with the protocol of tools/letterbox_tensor_bench.py (bench.sustained: 300 ms pre-heat of the same calls, median of
five >= 60 ms blocks, shader clock beside every number; one fresh process per run).  NV12 frames, BT.709 MPEG, ImageNet mean / std, pad 114.

Rows:
  4K -> 640 x 640 and 1080p -> 640 x 640, the whole frame letterboxed by vpf_letterbox_fit (640 x 360 at (0, 140): 6 x and 3 x), 1 and 32 frames;
  64 rectangles of four 1080p frames -> 224 x 224 at 1.5 x, 3 x and 6 x (336 x 189, 672 x 378, 1344 x 756 -> 224 x 126 at (0, 49));
  f32 and f16 throughout, channels-last f32 on the 1080p batch row.
Columns, per job:
  aa        (a) vpf_convert_letterbox_tensor_aa, one call
  chain     (b) vpf_convert_batch NV12 -> RGB_PLANAR of the frames, F.interpolate(mode="bilinear", antialias=True) of the crops on the device, pad
                and normalise in torch: it writes the full-size RGB frames to HBM and reads them back
  bilinear  (c) vpf_convert_letterbox_tensor on the same jobs: the price of the filter over the bare bilinear pair
  per tap   (d) the new entry under VPF_TUNE_NV12_RGB_VARIANT = 9: staged against per tap

  python tools/letterbox_aa_bench.py [--out profiles/r26_letterbox_aa.txt]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
PAD = (114, 114, 114)


def rows(capi):
    """(name, W, H, frames, dw, dh, [(frame, rect)], layouts and dtypes)"""
    import numpy as np

    out = []
    for W, H in ((3840, 2160), (1920, 1080)):
        for n in (1, 32):
            kinds = [("f32", False), ("f16", False)] + ([("f32", True)] if (W, n) == (1920, 32) else [])
            out.append((f"{W}x{H} -> 640x640 n={n}", W, H, n, 640, 640, [(i, (0, 0, W, H)) for i in range(n)], kinds))
    rng = np.random.default_rng(26)
    for k, (w, h) in ((1.5, (336, 189)), (3, (672, 378)), (6, (1344, 756))):
        jobs = [(i % 4, (int(rng.integers(0, 1920 - w + 1)), int(rng.integers(0, 1080 - h + 1)), w, h)) for i in range(64)]
        out.append((f"64 rois {w}x{h} of 4 x 1080p -> 224x224 ({k} x)", 1920, 1080, 4, 224, 224, jobs, [("f32", False), ("f16", False)]))
    return out


def measure():
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import torch.nn.functional as F

    import bench
    from videoprocessingframework_amd import capi

    dev = torch.device("cuda", 0)
    tdt = {"f32": torch.float32, "f16": torch.float16}
    ex = capi.make_exec(torch.cuda.current_stream().cuda_stream)
    pci = bench.device_pci(0)
    opts = capi.make_letterbox_opts(PAD)
    scale, bias = capi.norm_params(MEAN, STD)
    f32 = np.float32
    scale_t = torch.tensor([float(f32(v)) for v in scale], device=dev).view(1, 3, 1, 1)
    bias_t = torch.tensor([float(f32(v)) for v in bias], device=dev).view(1, 3, 1, 1)
    lines, lost_chain, lost_tap = [], [], []
    for name, W, H, nf, dw, dh, jobs, kinds in rows(capi):
        K = len(jobs)
        sp = (W + 255) // 256 * 256
        src = torch.randint(0, 256, (nf, H * 3 // 2, sp), dtype=torch.uint8, device=dev)
        fdesc = [[(src[i].data_ptr(), sp), (src[i].data_ptr() + H * sp, sp)] for i in range(nf)]
        rgb = torch.empty((nf, 3, H, W), dtype=torch.uint8, device=dev)
        to_rgb = capi.make_batch([(fdesc[i], [(rgb[i, c].data_ptr(), W) for c in range(3)]) for i in range(nf)])
        w, h = jobs[0][1][2:]
        ix, iy, iw, ih = capi.letterbox_fit(w, h, dw, dh)
        whole = all(r == (0, 0, W, H) for _, r in jobs)
        for dt, nhwc in kinds:
            out = torch.empty((K, dh, dw, 3) if nhwc else (K, 3, dh, dw), dtype=tdt[dt], device=dev)
            e = out.element_size()
            if nhwc:
                dst = [[(out[i].data_ptr(), 3 * dw * e), (0, 0), (0, 0)] for i in range(K)]
            else:
                dst = [[(out[i, c].data_ptr(), dw * e) for c in range(3)] for i in range(K)]
            norm = capi.make_tensor_norm(MEAN, STD, dtype={"f32": 0, "f16": 1}[dt], nhwc=nhwc)
            lb = capi.make_letterbox_jobs([(fdesc[f], dst[i], rect, (ix, iy, iw, ih)) for i, (f, rect) in enumerate(jobs)])
            padv = (torch.tensor([float(v) for v in PAD], device=dev).view(1, 3, 1, 1) * scale_t + bias_t).to(tdt[dt])
            view = out.permute(0, 3, 1, 2) if nhwc else out

            def chain():
                capi.convert_batch(ex, capi.NV12, capi.RGB_PLANAR, 1, 0, W, H, to_rgb)
                crops = rgb if whole else torch.stack([rgb[f, :, y:y + rh, x:x + rw] for f, (x, y, rw, rh) in jobs])
                x = F.interpolate(crops.float(), size=(ih, iw), mode="bilinear", antialias=True, align_corners=False)
                view.copy_(padv.expand_as(view))
                view[:, :, iy:iy + ih, ix:ix + iw] = (x * scale_t + bias_t).to(tdt[dt])

            res = {"aa": bench.sustained(lambda: capi.convert_letterbox_tensor_aa(ex, capi.NV12, 1, 0, W, H, dw, dh, lb, norm, opts), pci=pci)}
            res["chain"] = bench.sustained(chain, pci=pci)
            res["bilinear"] = bench.sustained(lambda: capi.convert_letterbox_tensor(ex, capi.NV12, 1, 0, W, H, dw, dh, lb, norm, opts), pci=pci)
            prev = capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, 9)
            try:
                res["per tap"] = bench.sustained(lambda: capi.convert_letterbox_tensor_aa(ex, capi.NV12, 1, 0, W, H, dw, dh, lb, norm, opts), pci=pci)
            finally:
                capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, prev)
            per = {k: r["us"] / K for k, r in res.items()}
            row = f"{name} {dt}{' nhwc' if nhwc else ''}"
            lines.append(f"{row}: " + "  ".join(
                f"{k} {per[k]:8.2f} us/job (spread {(max(res[k]['blocks_us']) - min(res[k]['blocks_us'])) / K:.2f}, sclk {res[k]['sclk_mhz']})" for k in res))
            lines.append(f"    chain / aa = {per['chain'] / per['aa']:6.2f}   aa / bilinear = {per['aa'] / per['bilinear']:6.2f}   aa / per tap = {per['aa'] / per['per tap']:5.2f}")
            if per["aa"] > per["chain"]:
                lost_chain.append(row)
            if per["aa"] > per["per tap"]:
                lost_tap.append(row)
            print("\n".join(lines[-2:]), flush=True)
            del out, view
        del src, rgb
        torch.cuda.empty_cache()
    lines.append("")
    lines.append("rows where the new entry loses to the chain: " + ("none" if not lost_chain else "; ".join(lost_chain)))
    lines.append("rows where the staged form loses to the per-tap form: " + ("none" if not lost_tap else "; ".join(lost_tap)))
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    a = ap.parse_args()
    head = (f"tools/letterbox_aa_bench.py: NV12 frames, BT.709 MPEG, ImageNet mean / std, pad {PAD}; microseconds per job, median of five >= 60 ms blocks "
            f"after 300 ms of pre-heat\n")
    text = head + measure()
    print(text.splitlines()[-1])
    if a.out:
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
