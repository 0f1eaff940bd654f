"""The fused planar float tensor -> NV12 path (vpf_tensor_convert_batch) against what it replaces, timed with the project's sustained-clock
protocol (bench.sustained: 300 ms pre-heat of the same calls, median of five >= 60 ms blocks, shader clock beside every number).

Legs, per (shape, dtype, frames), BT.601 JPEG, ImageNet mean / std, a contiguous [n, 3, H, W] tensor in, every frame its own NV12 surface out:
  fused_<dt>  vpf_tensor_convert_batch straight to NV12                                                            (needs the new entry point)
  chain_<dt>  what a user writes on the parent commit: torch mul / add / clamp / round / to(uint8) into a [n, 3, H, W] u8 tensor, then
              vpf_convert_batch RGB_PLANAR -> YUV420, then vpf_convert_batch YUV420 -> NV12
  conv        vpf_convert_batch RGB_PLANAR -> YUV420 alone: the same arithmetic on 4.5 B/px, the yardstick for the kernel itself

  python tools/tensor_in_bench.py --root DIR --legs chain,conv --out parent.json     (DIR = a checkout of the parent commit, built)
  python tools/tensor_in_bench.py --legs fused --out pr.json
  python tools/tensor_in_bench.py --report parent.json pr.json --out profiles/r08_tensor_in.txt

The report checks (1) fused faster than the parent's chain in every case, by more than the five-block spread of either leg, and (2) for
the batched cases, the fused kernel's fraction of 8 TB/s on its algorithmic bytes ((3 elem + 1.5) W H per frame) within 10 % (relative) of
conv's fraction on its 4.5 W H, same session.  A case that misses is printed with its numbers, not hidden."""
import argparse
import json
import os
import sys

SHAPES = [(3840, 2160), (1920, 1080), (1280, 720)]
FRAMES = (1, 32)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
DTYPES = ("f32", "f16", "bf16")
ELEM = {"f32": 4, "f16": 2, "bf16": 2}
PEAK_GBS = 8000.0


def measure(root, legs):
    sys.path.insert(0, root)
    import torch

    import bench
    from videoprocessingframework_amd import capi

    dev = torch.device("cuda", 0)
    tdt = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
    ex = capi.make_exec(torch.cuda.current_stream().cuda_stream)
    pci = bench.device_pci(0)
    sc = torch.tensor([255.0 * s for s in STD], device=dev).view(1, 3, 1, 1)
    bi = torch.tensor([255.0 * m for m in MEAN], device=dev).view(1, 3, 1, 1)
    rows = []
    for w, h in SHAPES:
        for n in FRAMES:
            yp = (w + 255) // 256 * 256
            nv = torch.empty((n, h * 3 // 2, yp), dtype=torch.uint8, device=dev)
            nvd = [[(nv[i].data_ptr(), yp), (nv[i].data_ptr() + h * yp, yp)] for i in range(n)]
            u8 = torch.randint(0, 256, (n, 3, h, w), dtype=torch.uint8, device=dev)
            i420 = torch.empty((n, h * 3 // 2, w), dtype=torch.uint8, device=dev)
            yuvd = [[(i420[i].data_ptr(), w), (i420[i].data_ptr() + h * w, w // 2), (i420[i].data_ptr() + h * w + (h // 2) * (w // 2), w // 2)] for i in range(n)]
            b1 = capi.make_batch([([(u8[i, c].data_ptr(), w) for c in range(3)], yuvd[i]) for i in range(n)])
            b2 = capi.make_batch([(yuvd[i], nvd[i]) for i in range(n)])
            run_conv = lambda: capi.convert_batch(ex, capi.RGB_PLANAR, capi.YUV420, 0, 1, w, h, b1)  # noqa: E731
            res = {}
            if "conv" in legs:
                res["conv"] = bench.sustained(run_conv, pci=pci)
            for dt in DTYPES:
                x = torch.randn((n, 3, h, w), dtype=torch.float32, device=dev).to(tdt[dt])
                if "chain" in legs:
                    def chain(x=x):
                        u8.copy_(torch.clamp(torch.add(torch.mul(x, sc), bi), 0.0, 255.0).round_())
                        run_conv()
                        capi.convert_batch(ex, capi.YUV420, capi.NV12, 0, 1, w, h, b2)
                    res["chain_" + dt] = bench.sustained(chain, pci=pci)
                if "fused" in legs:
                    e = x.element_size()
                    bt = capi.make_batch([([(x[i, c].data_ptr(), w * e) for c in range(3)], nvd[i]) for i in range(n)])
                    dn = capi.make_tensor_denorm(MEAN, STD, dtype=DTYPES.index(dt))
                    res["fused_" + dt] = bench.sustained(lambda bt=bt, dn=dn: capi.tensor_convert_batch(ex, capi.NV12, 0, 1, w, h, bt, dn), pci=pci)
                del x
            for k, r in res.items():
                r["us_per_frame"] = r["us"] / n
                r["spread_per_frame"] = (max(r["blocks_us"]) - min(r["blocks_us"])) / n
                print(f"{w}x{h} n{n} {k:11s} {r['us_per_frame']:9.3f} us/frame  spread {r['spread_per_frame']:.3f}  sclk {r['sclk_mhz']}", flush=True)
            rows.append({"shape": [w, h, n], "legs": res})
            del nv, u8, i420
            torch.cuda.empty_cache()
    return {"root": os.path.abspath(root), "rows": rows}


def report(parent, pr):
    lines = ["fused = vpf_tensor_convert_batch -> NV12; chain = torch mul / add / clamp / round / to-uint8 + RGB_PLANAR -> YUV420 + YUV420 -> NV12 (parent commit);",
             "conv = RGB_PLANAR -> YUV420 alone (parent commit); fractions are of 8 TB/s on the algorithmic bytes; pixel parity unpinned (NPP has no such call)", ""]
    ok1 = ok2 = True
    for prow, row in zip(parent["rows"], pr["rows"]):
        w, h, n = row["shape"]
        assert prow["shape"] == row["shape"]
        P, R = prow["legs"], row["legs"]
        conv = P["conv"]
        fconv = 4.5 * w * h / (conv["us_per_frame"] * 1e-6) / 1e9 / PEAK_GBS
        lines.append(f"{w}x{h}, {n} frame(s): conv {conv['us_per_frame']:.3f} us/frame (spread {conv['spread_per_frame']:.3f}, sclk {conv['sclk_mhz']}) = "
                     f"{fconv:.3f} of 8 TB/s")
        for dt in DTYPES:
            c, f = P["chain_" + dt], R["fused_" + dt]
            spread = max(c["spread_per_frame"], f["spread_per_frame"])
            c1 = c["us_per_frame"] - f["us_per_frame"] > spread
            ff = (3 * ELEM[dt] + 1.5) * w * h / (f["us_per_frame"] * 1e-6) / 1e9 / PEAK_GBS
            c2 = ff >= 0.9 * fconv
            ok1 &= c1
            tag2 = ""
            if n > 1:
                ok2 &= c2
                tag2 = f"  [2: {'pass' if c2 else 'MISS'}: {ff / fconv:.2f} of conv's fraction]"
            lines.append(f"  {dt:5s} fused {f['us_per_frame']:9.3f} us/frame (spread {f['spread_per_frame']:.3f}, sclk {f['sclk_mhz']}) = {ff:.3f} of 8 TB/s   "
                         f"chain {c['us_per_frame']:9.3f} (spread {c['spread_per_frame']:.3f}, sclk {c['sclk_mhz']})  "
                         f"speed-up {c['us_per_frame'] / f['us_per_frame']:5.2f}x  [1: {'pass' if c1 else 'FAIL'}]{tag2}")
        lines.append("")
    lines.append("criterion 1 (fused faster than the chain everywhere): " + ("pass" if ok1 else "FAIL"))
    lines.append("criterion 2 (batched fused within 10 % of conv's roofline fraction): " + ("pass" if ok2 else "SOME CASES MISS"))
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--legs", default="fused,chain,conv")
    ap.add_argument("--out")
    ap.add_argument("--report", nargs=2, metavar=("PARENT_JSON", "PR_JSON"))
    a = ap.parse_args()
    if a.report:
        text = report(json.load(open(a.report[0])), json.load(open(a.report[1])))
        print(text)
        if a.out:
            open(a.out, "w").write(text + "\n")
        return
    res = measure(a.root, set(a.legs.split(",")))
    if a.out:
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
