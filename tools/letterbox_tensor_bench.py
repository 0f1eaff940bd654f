"""Letterbox into the tensor (vpf_convert_letterbox_tensor) against the route it replaces and against its floor, timed with the project's
sustained-clock protocol (bench.sustained: 300 ms pre-heat of the same calls, median of five >= 60 ms blocks, shader clock beside every number;
one fresh process per run).  NV12 1080p frames, BT.709 MPEG, ImageNet mean / std, pad 114, f16 and f32.

Cases:
  frames     32 whole frames -> 640 x 640, the picture 640 x 360 at (0, 140): a detector's input batch
  crops      64 rects of mixed aspect over four frames -> 224 x 224, each job's dst_rect from vpf_letterbox_fit
  crops_odd  the same rects, every dst_rect moved or narrowed to an odd ix
Legs, per job:
  letterbox  vpf_convert_letterbox_tensor, one call
  chain (a)  the route a user had before: one broadcast copy_ of the pad's epilogue over the tensor, then one vpf_convert_resize_tensor_rois call
             per DISTINCT inner size on planes advanced by iy * pitch + ix * element size.  The new entry must not be slower
  floor (b)  vpf_convert_resize_tensor_rois stretching the same rects to the full destination: the same jobs without placement

  python tools/letterbox_tensor_bench.py [--out profiles/r12_letterbox_tensor.txt]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES, W, H = 4, 1920, 1080
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
PAD = (114, 114, 114)
DTYPES = ("f16", "f32")
CROP_SHAPES = [(96, 192), (192, 96), (400, 300), (300, 400), (640, 360), (200, 200), (120, 360), (360, 120)]


def cases(capi):
    """name -> (dw, dh, [(frame, rect, dst_rect)])"""
    import numpy as np

    out = {"frames": (640, 640, [(i % FRAMES, (0, 0, W, H), capi.letterbox_fit(W, H, 640, 640)) for i in range(32)])}
    rng = np.random.default_rng(12)
    crops = []
    for i in range(64):
        w, h = CROP_SHAPES[i % len(CROP_SHAPES)]
        rect = (int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1)), w, h)
        crops.append((i % FRAMES, rect, capi.letterbox_fit(w, h, 224, 224)))
    out["crops"] = (224, 224, crops)
    odd = []
    for f, rect, (ix, iy, iw, ih) in crops:
        if ix % 2 == 0:
            ix, iw = (1, iw - 1) if iw == 224 else (ix + 1, iw)
        odd.append((f, rect, (ix, iy, iw, ih)))
    out["crops_odd"] = (224, 224, odd)
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
    opts = capi.make_letterbox_opts(PAD)
    scale, bias = capi.norm_params(MEAN, STD)
    lines, ok = [], True
    for name, (dw, dh, jobs) in cases(capi).items():
        K = len(jobs)
        for dt in DTYPES:
            out = torch.empty((K, 3, dh, dw), dtype=tdt[dt], device=dev)
            e = out.element_size()
            dst = [[(out[i, c].data_ptr(), dw * e) for c in range(3)] for i in range(K)]
            norm = capi.make_tensor_norm(MEAN, STD, dtype={"f32": 0, "f16": 1}[dt])
            res = {}
            lb = capi.make_letterbox_jobs([(fdesc[f], dst[i], rect, d) for i, (f, rect, d) in enumerate(jobs)])
            res["letterbox"] = bench.sustained(lambda: capi.convert_letterbox_tensor(ex, capi.NV12, 1, 0, W, H, dw, dh, lb, norm, opts), pci=pci)
            want = out.clone()
            # (a) fill, then one ROI call per distinct inner size on sliced planes
            f32 = np.float32  # the library rounds scale and bias to fp32 first; the fma's exact value fits a double
            padv = torch.tensor([PAD[c] * float(f32(scale[c])) + float(f32(bias[c])) for c in range(3)], dtype=torch.float32, device=dev).to(tdt[dt]).view(1, 3, 1, 1)
            groups = {}
            for i, (f, rect, (ix, iy, iw, ih)) in enumerate(jobs):
                sliced = [(p + (iy * dw + ix) * e, pitch) for p, pitch in dst[i]]
                groups.setdefault((iw, ih), []).append((fdesc[f], sliced, rect))
            calls = [(iw, ih, capi.make_rois(g)) for (iw, ih), g in groups.items()]

            def chain():
                out.copy_(padv.expand_as(out))
                for iw, ih, rois in calls:
                    capi.convert_resize_tensor_rois(ex, capi.NV12, 1, 0, W, H, iw, ih, rois, norm)

            res["chain"] = bench.sustained(chain, pci=pci)
            torch.cuda.synchronize()
            same = bool(torch.equal(out.view(torch.int16 if e == 2 else torch.int32), want.view(torch.int16 if e == 2 else torch.int32)))
            # (b) the floor: the same rects stretched to the full destination
            rois = capi.make_rois([(fdesc[f], dst[i], rect) for i, (f, rect, _) in enumerate(jobs)])
            res["floor"] = bench.sustained(lambda: capi.convert_resize_tensor_rois(ex, capi.NV12, 1, 0, W, H, dw, dh, rois, norm), pci=pci)
            per = {k: r["us"] / K for k, r in res.items()}
            c = per["letterbox"] <= per["chain"]
            ok = ok and c
            lines.append(f"{name} K={K} -> {dw}x{dh} {dt} ({len(calls)} distinct inner sizes): " + "  ".join(
                f"{k} {per[k]:7.3f} us/job (spread {(max(res[k]['blocks_us']) - min(res[k]['blocks_us'])) / K:.3f}, sclk {res[k]['sclk_mhz']})" for k in res))
            lines.append(f"    chain / letterbox = {per['chain'] / per['letterbox']:6.2f}x [{'pass' if c else 'FAIL'}]   letterbox / floor = "
                         f"{per['letterbox'] / per['floor']:5.2f}   chain bits == letterbox bits: {same}")
            print("\n".join(lines[-2:]), flush=True)
            del out, want
            torch.cuda.empty_cache()
    lines.append("")
    lines.append(f"never slower than the chain it fuses: {'every case passes' if ok else 'SOME CASES FAIL (DESIGN.md 4.12)'}")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    a = ap.parse_args()
    head = (f"tools/letterbox_tensor_bench.py: NV12 {W}x{H} frames, BT.709 MPEG, ImageNet mean / std, pad {PAD}; microseconds per job, median of five "
            f">= 60 ms blocks after 300 ms of pre-heat\n")
    text = head + measure()
    print(text.splitlines()[-1])
    if a.out:
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
