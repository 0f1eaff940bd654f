"""P10 sources of the fused tensor entries (vpf_convert_resize_tensor_batch, vpf_convert_resize_tensor_rois, vpf_convert_warp_tensor) against the
route a user had before them, timed with the project's sustained-clock protocol (bench.sustained: 300 ms pre-heat of the same calls, median of five
>= 60 ms blocks, shader clock beside every number; one fresh process per run).  Per row, on P10 sources (BT.709 MPEG, ImageNet mean / std), f16 and f32:
  fused   the entry on the P10 frames, one call
  chain   vpf_convert_batch(P10 -> NV12) of the WHOLE frames into NV12 planes, then the same entry on those (both untouched by the 16-bit sources)
  nv12    the same entry on an 8-bit source of the same shape (recorded, not gated: a P10 source is twice the source bytes)
The legs of a row are alternated (fused, chain, nv12, fused, chain, nv12) in this one process; a row passes when the SLOWER fused pass beats the
FASTER chain pass by more than the run-to-run spread, which is measured by repeating one row's fused leg.  Bytes are computed, not measured: what
each route must move at least (a region's own samples; whole frames for the narrowing pass).

  python tools/p16_tensor_bench.py [--out profiles/r11_p16_tensor.txt]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
N = 32                                                        # whole frames per batched call
WHOLE = [(3840, 2160, 1920, 1080, "half"), (1920, 1080, 1280, 720, "strip"), (3840, 2160, 1280, 720, "gather fallback"), (3840, 2160, 224, 224, "gather fallback")]
K, FRAMES, W, H = 64, 4, 1920, 1080                           # regions over four 1080p frames
ROI_SHAPES = [(96, 192, 128, 256), (400, 300, 224, 224), (640, 640, 224, 224), (1500, 900, 224, 224)]  # tools/roi_tensor_bench.py's
WARP_SHAPES = [((400, 300, 224, 224), 15), ((112, 112, 112, 112), 45)]                                  # two of tools/warp_tensor_bench.py's
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
DTYPES = ("f16", "f32")
SPREAD_REPEATS = 5


def measure():
    sys.path.insert(0, ROOT)
    import torch

    import bench
    import roi_tensor_bench
    import warp_tensor_bench
    from videoprocessingframework_amd import capi

    dev = torch.device("cuda", 0)
    tdt = {"f32": torch.float32, "f16": torch.float16}
    ex = capi.make_exec(torch.cuda.current_stream().cuda_stream)
    pci = bench.device_pci(0)
    lines, rows = [], []

    def p16_frames(n, w, h):
        """n P10 frames (one allocation each row-pitched to 256 B: Y rows then UV rows) + their NV12 twins for the chain and the nv12 leg"""
        p16, p8 = (2 * w + 255) // 256 * 256, (w + 255) // 256 * 256
        s16 = torch.randint(0, 256, (n, h * 3 // 2, p16), dtype=torch.uint8, device=dev)
        s8 = torch.randint(0, 256, (n, h * 3 // 2, p8), dtype=torch.uint8, device=dev)
        d16 = [[(s16[i].data_ptr(), p16), (s16[i].data_ptr() + h * p16, p16)] for i in range(n)]
        d8 = [[(s8[i].data_ptr(), p8), (s8[i].data_ptr() + h * p8, p8)] for i in range(n)]
        return (s16, s8), d16, d8

    def row(label, legs, per, mb):
        """legs: {name: fn}; two alternated passes; `per` = regions / frames per call; mb = {leg: computed MB per call}"""
        res = {k: [] for k in legs}
        for _ in range(2):
            for k, fn in legs.items():
                res[k].append(bench.sustained(fn, pci=pci))
        us = {k: [r["us"] / per for r in v] for k, v in res.items()}
        rows.append((label, us))
        lines.append(f"{label}: " + "  ".join(f"{k} {us[k][0]:8.3f} / {us[k][1]:8.3f} us (sclk {res[k][0]['sclk_mhz']} / {res[k][1]['sclk_mhz']}, {mb[k]:7.2f} MB per call)" for k in legs))
        lines.append(f"    chain / fused = {min(us['chain']) / max(us['fused']):5.2f}x (faster chain pass over slower fused pass)   fused / nv12 = {max(us['fused']) / min(us['nv12']):5.2f}")
        print("\n".join(lines[-2:]), flush=True)

    # ---- whole frames, batched
    for sw, sh, dw, dh, form in WHOLE:
        keep, d16, d8 = p16_frames(N, sw, sh)
        batch_nv = capi.make_batch([(d16[i], d8[i]) for i in range(N)])
        for dt in DTYPES:
            out = torch.empty((N, 3, dh, dw), dtype=tdt[dt], device=dev)
            e = out.element_size()
            dst = [[(out[i, c].data_ptr(), dw * e) for c in range(3)] for i in range(N)]
            norm = capi.make_tensor_norm(MEAN, STD, dtype={"f32": 0, "f16": 1}[dt])
            b16, b8 = capi.make_batch([(d16[i], dst[i]) for i in range(N)]), capi.make_batch([(d8[i], dst[i]) for i in range(N)])

            def chain():
                capi.convert_batch(ex, capi.P10, capi.NV12, 0, 0, sw, sh, batch_nv)
                capi.convert_resize_tensor_batch(ex, capi.NV12, 1, 0, sw, sh, dw, dh, b8, norm)

            o = 3 * dw * dh * e
            mb = {"fused": N * (3 * sw * sh + o) / 1e6, "chain": N * (3 * sw * sh + 1.5 * sw * sh + 1.5 * sw * sh + o) / 1e6, "nv12": N * (1.5 * sw * sh + o) / 1e6}
            row(f"whole {sw}x{sh} -> {dw}x{dh} {dt} ({form}), per frame of {N}",
                {"fused": lambda: capi.convert_resize_tensor_batch(ex, capi.P10, 1, 0, sw, sh, dw, dh, b16, norm), "chain": chain,
                 "nv12": lambda: capi.convert_resize_tensor_batch(ex, capi.NV12, 1, 0, sw, sh, dw, dh, b8, norm)}, N, mb)
            del out
        del keep
        torch.cuda.empty_cache()

    # ---- regions of four 1080p frames
    keep, d16, d8 = p16_frames(FRAMES, W, H)
    batch_nv = capi.make_batch([(d16[i], d8[i]) for i in range(FRAMES)])
    narrow_mb = FRAMES * (3 * W * H + 1.5 * W * H) / 1e6
    spread_fn = None
    for w, h, dw, dh in ROI_SHAPES:
        for dt in DTYPES:
            out = torch.empty((K, 3, dh, dw), dtype=tdt[dt], device=dev)
            e = out.element_size()
            dst = [[(out[i, c].data_ptr(), dw * e) for c in range(3)] for i in range(K)]
            norm = capi.make_tensor_norm(MEAN, STD, dtype={"f32": 0, "f16": 1}[dt])
            rects = roi_tensor_bench.rects_of(w, h, False)
            r16 = capi.make_rois([(d16[f], dst[i], (x, y, rw, rh)) for i, (f, x, y, rw, rh) in enumerate(rects)])
            r8 = capi.make_rois([(d8[f], dst[i], (x, y, rw, rh)) for i, (f, x, y, rw, rh) in enumerate(rects)])

            def chain(r8=r8, dw=dw, dh=dh, norm=norm):
                capi.convert_batch(ex, capi.P10, capi.NV12, 0, 0, W, H, batch_nv)
                capi.convert_resize_tensor_rois(ex, capi.NV12, 1, 0, W, H, dw, dh, r8, norm)

            fused = lambda r16=r16, dw=dw, dh=dh, norm=norm: capi.convert_resize_tensor_rois(ex, capi.P10, 1, 0, W, H, dw, dh, r16, norm)
            o = 3 * dw * dh * e
            mb = {"fused": K * (3 * w * h + o) / 1e6, "chain": narrow_mb + K * (1.5 * w * h + o) / 1e6, "nv12": K * (1.5 * w * h + o) / 1e6}
            row(f"rois {w}x{h} -> {dw}x{dh} {dt}, per region of {K}",
                {"fused": fused, "chain": chain, "nv12": lambda: capi.convert_resize_tensor_rois(ex, capi.NV12, 1, 0, W, H, dw, dh, r8, norm)}, K, mb)
            if (w, h, dt) == (400, 300, "f16"):
                spread_fn, spread_keep = fused, out
    for (w, h, dw, dh), deg in WARP_SHAPES:
        for dt in DTYPES:
            out = torch.empty((K, 3, dh, dw), dtype=tdt[dt], device=dev)
            e = out.element_size()
            dst = [[(out[i, c].data_ptr(), dw * e) for c in range(3)] for i in range(K)]
            norm = capi.make_tensor_norm(MEAN, STD, dtype={"f32": 0, "f16": 1}[dt])
            jobs = warp_tensor_bench.jobs_of(w, h, dw, dh, deg)
            w16 = capi.make_warps([(d16[f], dst[i], m) for i, (f, _, m) in enumerate(jobs)])
            w8 = capi.make_warps([(d8[f], dst[i], m) for i, (f, _, m) in enumerate(jobs)])

            def chain():
                capi.convert_batch(ex, capi.P10, capi.NV12, 0, 0, W, H, batch_nv)
                capi.convert_warp_tensor(ex, capi.NV12, 1, 0, W, H, dw, dh, w8, norm)

            o = 3 * dw * dh * e
            mb = {"fused": K * (3 * w * h + o) / 1e6, "chain": narrow_mb + K * (1.5 * w * h + o) / 1e6, "nv12": K * (1.5 * w * h + o) / 1e6}
            row(f"warps {w}x{h} at {deg} deg -> {dw}x{dh} {dt}, per region of {K}",
                {"fused": lambda: capi.convert_warp_tensor(ex, capi.P10, 1, 0, W, H, dw, dh, w16, norm), "chain": chain,
                 "nv12": lambda: capi.convert_warp_tensor(ex, capi.NV12, 1, 0, W, H, dw, dh, w8, norm)}, K, mb)
            del out
    # ---- run-to-run spread: one row's fused leg repeated
    rep = [bench.sustained(spread_fn, pci=pci)["us"] / K for _ in range(SPREAD_REPEATS)]
    spread = (max(rep) - min(rep)) / sorted(rep)[len(rep) // 2]
    lines.append("")
    lines.append(f"run-to-run spread: rois 400x300 -> 224x224 f16 fused, {SPREAD_REPEATS} repeats: " + " ".join(f"{r:.3f}" for r in rep) + f" us/region: (max - min) / median = {100 * spread:.1f} %")
    lost = [label for label, us in rows if not max(us["fused"]) * (1.0 + spread) < min(us["chain"])]
    lines.append("fused beats chain by more than the spread (slower fused pass x (1 + spread) < faster chain pass): " +
                 ("every row" if not lost else "NOT in: " + "; ".join(lost)))
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    a = ap.parse_args()
    head = ("tools/p16_tensor_bench.py: P10 sources of the fused tensor entries, BT.709 MPEG, ImageNet mean / std; microseconds per frame / region, two "
            "alternated passes per leg, each the median of five >= 60 ms blocks after 300 ms of pre-heat; MB per call computed\n")
    text = head + measure()
    print("\n".join(text.splitlines()[-2:]))
    if a.out:
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
