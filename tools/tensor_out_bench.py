"""The normalised planar-tensor output of the fused path (vpf_convert_resize_tensor_batch) against what it replaces, timed with the project's
sustained-clock protocol (bench.sustained: 300 ms pre-heat of the same calls, median of five >= 60 ms blocks, shader clock beside every number).

Legs, per shape (batched NV12, BT.709 MPEG, ImageNet mean / std, every frame its own source and destination):
  u8          vpf_convert_resize_batch -> RGB_PLANAR into a uint8 [n, 3, H, W] tensor (the fused kernel the tensor path extends)
  chain_<dt>  the same, then torch's .float().div(255).sub(mean).div(std) (+ .half() / .bfloat16()): what the samples run today
  tensor_<dt> vpf_convert_resize_tensor_batch straight into a [n, 3, H, W] tensor of <dt>                          (needs the new entry point)

  python tools/tensor_out_bench.py --root DIR --legs u8,chain --out parent.json     (DIR = a checkout of the parent commit, built)
  python tools/tensor_out_bench.py --legs u8,chain,tensor --out pr.json
  python tools/tensor_out_bench.py --report parent.json pr.json --write-gbs W       (W = the write-only line of tools/bw_ceilings.py)

The report checks (1) tensor faster per frame than the parent's chain by more than the five-block spread of either leg, and (2)
t_tensor <= 1.10 t_u8(parent) + extra_bytes / write_rate, extra_bytes = (elem - 1) x 3 x W x H per frame."""
import argparse
import json
import os
import sys

SHAPES = [(1920, 1080, 224, 224, 128), (1920, 1080, 640, 360, 128), (1920, 1080, 1280, 720, 128), (3840, 2160, 1920, 1080, 32)]
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
DTYPES = ("f32", "f16", "bf16")
ELEM = {"f32": 4, "f16": 2, "bf16": 2}


def measure(root, legs):
    sys.path.insert(0, root)
    import torch

    import bench
    from videoprocessingframework_amd import capi

    dev = torch.device("cuda", 0)
    tdt = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
    ex = capi.make_exec(torch.cuda.current_stream().cuda_stream)
    pci = bench.device_pci(0)
    m_t, s_t = torch.tensor(MEAN, device=dev).view(1, 3, 1, 1), torch.tensor(STD, device=dev).view(1, 3, 1, 1)
    rows = []
    for sw, sh, dw, dh, n in SHAPES:
        sp = (sw + 255) // 256 * 256
        src = torch.randint(0, 256, (n, sh * 3 // 2, sp), dtype=torch.uint8, device=dev)
        sdesc = [[(src[i].data_ptr(), sp), (src[i].data_ptr() + sh * sp, sp)] for i in range(n)]
        u8 = torch.empty((n, 3, dh, dw), dtype=torch.uint8, device=dev)
        b8 = capi.make_batch([(sdesc[i], [(u8[i, c].data_ptr(), dw) for c in range(3)]) for i in range(n)])
        run_u8 = lambda: capi.convert_resize_batch(ex, capi.NV12, capi.RGB_PLANAR, 1, 0, sw, sh, dw, dh, b8)  # noqa: E731
        res = {}
        if "u8" in legs:
            res["u8"] = bench.sustained(run_u8, pci=pci)
        for dt in DTYPES:
            if "chain" in legs:
                def chain(dt=dt):
                    run_u8()
                    y = u8.float().div(255).sub(m_t).div(s_t)
                    return y if dt == "f32" else y.to(tdt[dt])
                res["chain_" + dt] = bench.sustained(chain, pci=pci)
            if "tensor" in legs:
                out = torch.empty((n, 3, dh, dw), dtype=tdt[dt], device=dev)
                e = out.element_size()
                bt = capi.make_batch([(sdesc[i], [(out[i, c].data_ptr(), dw * e) for c in range(3)]) for i in range(n)])
                norm = capi.make_tensor_norm(MEAN, STD, dtype=DTYPES.index(dt))
                res["tensor_" + dt] = bench.sustained(lambda bt=bt, norm=norm: capi.convert_resize_tensor_batch(ex, capi.NV12, 1, 0, sw, sh, dw, dh, bt, norm), pci=pci)
        for k, r in res.items():
            r["us_per_frame"] = r["us"] / n
            r["spread_per_frame"] = (max(r["blocks_us"]) - min(r["blocks_us"])) / n
            print(f"{sw}x{sh}->{dw}x{dh} n{n} {k:12s} {r['us_per_frame']:8.3f} us/frame  spread {r['spread_per_frame']:.3f}  sclk {r['sclk_mhz']}", flush=True)
        rows.append({"shape": [sw, sh, dw, dh, n], "legs": res})
        del src, u8
        torch.cuda.empty_cache()
    return {"root": os.path.abspath(root), "rows": rows}


def report(parent, pr, write_gbs):
    lines = [f"write rate (tools/bw_ceilings.py, torch fill_ write-only line): {write_gbs:.0f} GB/s", ""]
    ok_all = True
    for prow, row in zip(parent["rows"], pr["rows"]):
        sw, sh, dw, dh, n = row["shape"]
        assert prow["shape"] == row["shape"]
        P, R = prow["legs"], row["legs"]
        u8p = P["u8"]["us_per_frame"]
        lines.append(f"{sw}x{sh} -> {dw}x{dh}, {n} frames: parent u8 fused {u8p:.3f} us/frame (spread {P['u8']['spread_per_frame']:.3f}, "
                     f"sclk {P['u8']['sclk_mhz']}); PR u8 fused {R['u8']['us_per_frame']:.3f} us/frame (spread {R['u8']['spread_per_frame']:.3f})")
        for dt in DTYPES:
            c, t = P["chain_" + dt], R["tensor_" + dt]
            spread = max(c["spread_per_frame"], t["spread_per_frame"])
            c1 = c["us_per_frame"] - t["us_per_frame"] > spread
            extra = (ELEM[dt] - 1) * 3 * dw * dh
            bound = 1.10 * u8p + extra / (write_gbs * 1e3)  # bytes / (GB/s) -> us: bytes / (W x 1e9) x 1e6
            c2 = t["us_per_frame"] <= bound
            ok_all &= c1 and c2
            lines.append(f"  {dt:5s} tensor {t['us_per_frame']:8.3f} us/frame (spread {t['spread_per_frame']:.3f}, sclk {t['sclk_mhz']})  "
                         f"parent chain {c['us_per_frame']:8.3f} (spread {c['spread_per_frame']:.3f}, sclk {c['sclk_mhz']})  "
                         f"speed-up {c['us_per_frame'] / t['us_per_frame']:5.2f}x  [1: {'pass' if c1 else 'FAIL'}]  "
                         f"bound 1.10 x u8 + {extra} B / write rate = {bound:.3f}  [2: {'pass' if c2 else 'FAIL'}]")
        lines.append("")
    lines.append("all criteria pass" if ok_all else "SOME CRITERIA FAIL")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--legs", default="u8,chain,tensor")
    ap.add_argument("--out")
    ap.add_argument("--report", nargs=2, metavar=("PARENT_JSON", "PR_JSON"))
    ap.add_argument("--write-gbs", type=float)
    a = ap.parse_args()
    if a.report:
        text = report(json.load(open(a.report[0])), json.load(open(a.report[1])), a.write_gbs)
        print(text)
        if a.out:
            open(a.out, "w").write(text + "\n")
        return
    res = measure(a.root, set(a.legs.split(",")))
    if a.out:
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
