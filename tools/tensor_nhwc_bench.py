"""Channels-last (NHWC) tensors in the fused tensor entries (VPF_TENSOR_NHWC) against what a channels-last model's user runs without them, timed
with the project's sustained-clock protocol (bench.sustained: 300 ms pre-heat of the same calls, median of five >= 60 ms blocks, shader clock
beside every number).  The shapes and batch sizes of tools/tensor_out_bench.py.

Legs, per shape and dtype (batched NV12, BT.709 MPEG, ImageNet mean / std, every frame its own source and destination):
  planar_<dt>      vpf_convert_resize_tensor_batch into a planar [n, 3, H, W] tensor
  chain_<dt>       the same, then .contiguous(memory_format=torch.channels_last): one more read and write of the whole tensor — today's way
  nhwc_<dt>        vpf_convert_resize_tensor_batch with VPF_TENSOR_NHWC straight into a channels-last tensor            (needs the flag)
the way back at 720p and 1080p (32 frames, NV12, JPEG range):
  enc_chain_<dt>   .contiguous() of a channels-last tensor, then vpf_tensor_convert_batch on the planar copy — today's way
  enc_nhwc_<dt>    vpf_tensor_convert_batch with VPF_TENSOR_NHWC on the channels-last tensor itself                      (needs the flag)

  python tools/tensor_nhwc_bench.py --root DIR --legs planar,chain,enc_chain --out parent.json    (DIR = a checkout of the parent commit, built)
  python tools/tensor_nhwc_bench.py --legs planar,nhwc,enc_nhwc --out pr.json
  python tools/tensor_nhwc_bench.py --report parent.json pr.json
  python tools/tensor_nhwc_bench.py --legs nhwc --ab --lib OTHER/libvpfhip.so --out ab.json   (the A/B of the store forms: a second build of csrc/
                                                                   with -DVPF_NHWC_DENSE=<mask>, vpf_internal.h; --ab adds a shape per family)

The report checks (1, required) nhwc faster per frame than the parent's chain by more than the five-block spread of either leg, and (2, target)
t_nhwc <= 1.10 t_planar(parent): the bytes are the same."""
import argparse
import json
import os
import sys

SHAPES = [(1920, 1080, 224, 224, 128, 0), (1920, 1080, 640, 360, 128, 0), (1920, 1080, 1280, 720, 128, 0), (3840, 2160, 1920, 1080, 32, 0)]
# one more shape per family the four above do not reach: (.., VPF_TUNE_NV12_RGB_VARIANT)
AB_SHAPES = [(3840, 2160, 1600, 900, 32, 0), (1920, 1080, 1280, 720, 32, 9), (1280, 720, 1920, 1080, 32, 0)]
ENC_SHAPES = [(1280, 720, 32), (1920, 1080, 32)]
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
DTYPES = ("f32", "f16", "bf16")


def measure(root, legs, lib, ab):
    sys.path.insert(0, root)
    import torch

    import bench
    from videoprocessingframework_amd import capi

    if lib:
        capi.LIB_PATH = os.path.abspath(lib)
    capi.lib()
    dev = torch.device("cuda", 0)
    tdt = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
    ex = capi.make_exec(torch.cuda.current_stream().cuda_stream)
    pci = bench.device_pci(0)
    rows = []

    def finish(shape, res, n):
        for k, r in res.items():
            r["us_per_frame"] = r["us"] / n
            r["spread_per_frame"] = (max(r["blocks_us"]) - min(r["blocks_us"])) / n
            print(f"{shape} n{n} {k:14s} {r['us_per_frame']:8.3f} us/frame  spread {r['spread_per_frame']:.3f}  sclk {r['sclk_mhz']}", flush=True)

    for sw, sh, dw, dh, n, variant in SHAPES + (AB_SHAPES if ab else []):
        if not legs & {"planar", "chain", "nhwc"}:
            break
        sp = (sw + 255) // 256 * 256
        src = torch.randint(0, 256, (n, sh * 3 // 2, sp), dtype=torch.uint8, device=dev)
        sdesc = [[(src[i].data_ptr(), sp), (src[i].data_ptr() + sh * sp, sp)] for i in range(n)]
        prev = capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, variant)
        res = {}
        for dt in DTYPES:
            out = torch.empty((n, 3, dh, dw), dtype=tdt[dt], device=dev)
            e = out.element_size()
            bt = capi.make_batch([(sdesc[i], [(out[i, c].data_ptr(), dw * e) for c in range(3)]) for i in range(n)])
            norm = capi.make_tensor_norm(MEAN, STD, dtype=DTYPES.index(dt))
            planar = lambda bt=bt, norm=norm: capi.convert_resize_tensor_batch(ex, capi.NV12, 1, 0, sw, sh, dw, dh, bt, norm)  # noqa: E731
            if "planar" in legs:
                res["planar_" + dt] = bench.sustained(planar, pci=pci)
            if "chain" in legs:
                def chain(planar=planar, out=out):
                    planar()
                    return out.contiguous(memory_format=torch.channels_last)
                res["chain_" + dt] = bench.sustained(chain, pci=pci)
            if "nhwc" in legs:
                cl = torch.empty((n, 3, dh, dw), dtype=tdt[dt], device=dev, memory_format=torch.channels_last)
                bn = capi.make_batch([(sdesc[i], [(cl[i].data_ptr(), 3 * dw * e), (0, 0), (0, 0)]) for i in range(n)])
                nn = capi.make_tensor_norm(MEAN, STD, dtype=DTYPES.index(dt), nhwc=True)
                res["nhwc_" + dt] = bench.sustained(lambda bn=bn, nn=nn: capi.convert_resize_tensor_batch(ex, capi.NV12, 1, 0, sw, sh, dw, dh, bn, nn), pci=pci)
                del cl
            del out
        capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, prev)
        finish(f"{sw}x{sh}->{dw}x{dh}" + (f" variant {variant}" if variant else ""), res, n)
        rows.append({"shape": [sw, sh, dw, dh, n, variant], "legs": res})
        del src
        torch.cuda.empty_cache()
    for w, h, n in ENC_SHAPES:
        if not legs & {"enc_chain", "enc_nhwc"}:
            break
        dst = torch.empty((n, h * 3 // 2, w), dtype=torch.uint8, device=dev)
        ddesc = [[(dst[i].data_ptr(), w), (dst[i].data_ptr() + h * w, w)] for i in range(n)]
        res = {}
        for dt in DTYPES:
            cl = torch.randn((n, 3, h, w), device=dev).to(tdt[dt]).contiguous(memory_format=torch.channels_last)
            e = cl.element_size()
            if "enc_chain" in legs:
                dn = capi.make_tensor_denorm(MEAN, STD, dtype=DTYPES.index(dt))
                x = torch.empty((n, 3, h, w), dtype=tdt[dt], device=dev)  # (.contiguous() is this copy into a new planar tensor; the batch is built once)
                bp = capi.make_batch([([(x[i, c].data_ptr(), w * e) for c in range(3)], ddesc[i]) for i in range(n)])

                def enc_chain(cl=cl, dn=dn, x=x, bp=bp):
                    x.copy_(cl)
                    capi.tensor_convert_batch(ex, capi.NV12, 0, 1, w, h, bp, dn)
                res["enc_chain_" + dt] = bench.sustained(enc_chain, pci=pci)
                del x
            if "enc_nhwc" in legs:
                dn = capi.make_tensor_denorm(MEAN, STD, dtype=DTYPES.index(dt), nhwc=True)
                bt = capi.make_batch([([(cl[i].data_ptr(), 3 * w * e), (0, 0), (0, 0)], ddesc[i]) for i in range(n)])
                res["enc_nhwc_" + dt] = bench.sustained(lambda bt=bt, dn=dn: capi.tensor_convert_batch(ex, capi.NV12, 0, 1, w, h, bt, dn), pci=pci)
            del cl
        finish(f"tensor {w}x{h} -> NV12", res, n)
        rows.append({"shape": [w, h, n], "legs": res})
        del dst
        torch.cuda.empty_cache()
    return {"root": os.path.abspath(root), "lib": lib, "rows": rows}


def report(parent, pr):
    lines = []
    ok1 = ok2 = True
    prows = {tuple(r["shape"]): r["legs"] for r in parent["rows"]}
    for row in pr["rows"]:
        P, R = prows.get(tuple(row["shape"])), row["legs"]
        if P is None:
            continue
        if len(row["shape"]) == 3:
            w, h, n = row["shape"]
            lines.append(f"tensor {w}x{h} -> NV12, {n} frames (the way back):")
            for dt in DTYPES:
                c, t = P["enc_chain_" + dt], R["enc_nhwc_" + dt]
                c1 = c["us_per_frame"] - t["us_per_frame"] > max(c["spread_per_frame"], t["spread_per_frame"])
                ok1 &= c1
                lines.append(f"  {dt:5s} nhwc {t['us_per_frame']:8.3f} us/frame (spread {t['spread_per_frame']:.3f}, sclk {t['sclk_mhz']})  parent .contiguous() + planar "
                             f"{c['us_per_frame']:8.3f} (spread {c['spread_per_frame']:.3f}, sclk {c['sclk_mhz']})  speed-up {c['us_per_frame'] / t['us_per_frame']:5.2f}x  "
                             f"[1: {'pass' if c1 else 'FAIL'}]")
            lines.append("")
            continue
        sw, sh, dw, dh, n, variant = row["shape"]
        lines.append(f"{sw}x{sh} -> {dw}x{dh}, {n} frames" + (f", variant {variant}" if variant else "") + ":")
        for dt in DTYPES:
            p, c, t = P["planar_" + dt], P["chain_" + dt], R["nhwc_" + dt]
            c1 = c["us_per_frame"] - t["us_per_frame"] > max(c["spread_per_frame"], t["spread_per_frame"])
            c2 = t["us_per_frame"] <= 1.10 * p["us_per_frame"]
            ok1 &= c1
            ok2 &= c2
            here = f"  PR planar {R['planar_' + dt]['us_per_frame']:8.3f}" if "planar_" + dt in R else ""
            lines.append(f"  {dt:5s} nhwc {t['us_per_frame']:8.3f} us/frame (spread {t['spread_per_frame']:.3f}, sclk {t['sclk_mhz']})  parent planar "
                         f"{p['us_per_frame']:8.3f} (spread {p['spread_per_frame']:.3f})  parent chain {c['us_per_frame']:8.3f} (spread {c['spread_per_frame']:.3f}, "
                         f"sclk {c['sclk_mhz']})  vs chain {c['us_per_frame'] / t['us_per_frame']:5.2f}x [1: {'pass' if c1 else 'FAIL'}]  "
                         f"vs planar {t['us_per_frame'] / p['us_per_frame']:5.2f}x [2: {'pass' if c2 else 'miss'}]{here}")
        lines.append("")
    lines.append("criterion 1 (required): " + ("holds in every case" if ok1 else "FAILS SOMEWHERE"))
    lines.append("criterion 2 (target, 1.10 x planar): " + ("met in every case" if ok2 else "missed somewhere"))
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--legs", default="planar,nhwc,enc_nhwc")
    ap.add_argument("--lib", help="another build of libvpfhip.so to load (the A/B of the store forms)")
    ap.add_argument("--ab", action="store_true", help="add one shape per fused family the four standard shapes do not reach")
    ap.add_argument("--out")
    ap.add_argument("--report", nargs=2, metavar=("PARENT_JSON", "PR_JSON"))
    a = ap.parse_args()
    if a.report:
        text = report(json.load(open(a.report[0])), json.load(open(a.report[1])))
        print(text)
        if a.out:
            open(a.out, "w").write(text + "\n")
        return
    res = measure(a.root, set(a.legs.split(",")), a.lib, a.ab)
    if a.out:
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
