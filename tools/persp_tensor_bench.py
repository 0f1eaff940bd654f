"""The fused multi-ROI perspective warp into a normalised tensor (vpf_convert_persp_tensor) against the chain it replaces and against the affine
entry it generalises, timed with the project's sustained-clock protocol (bench.sustained: 300 ms pre-heat of the same calls, median of five >= 60 ms
blocks, shader clock beside every number; one fresh process per run).

K = 64 jobs spread over four 1080p NV12 frames (BT.709 MPEG, ImageNet mean / std), f16 and f32, per footprint (w x h of the frame -> dw x dh: the
footprints of tools/warp_tensor_bench.py), each footprint twice:
  keystone  the quad whose top edge is the footprint's shrunk by 15 % on either side, through quads_to_homographies (corner to corner)
  affine    the footprint itself, corner to corner: the 2 x 3 matrix with the last row (0, 0, 1) appended
  persp   vpf_convert_persp_tensor, one call, default policy                                                          (`gather`: tuning variant 9)
  chain   what a user had before: one vpf_convert NV12 -> RGB per frame, K vpf_remap calls on PREBUILT device maps (their construction is not
          timed, in the chain's favour), then torch permute, cast and normalise; the fused call must be faster in every row (a)
  warp    vpf_convert_warp_tensor on the same 2 x 3 matrices (affine rows only): persp / warp is the cost of the generalisation — a division, a
          third row, the window test; the allowance for a generalised entry against its special case is 1.25 (b), rows above it are reported

  python tools/persp_tensor_bench.py [--out profiles/r16_persp_tensor.txt]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, FRAMES, W, H = 64, 4, 1920, 1080
SHAPES = [(96, 192, 128, 256), (400, 300, 224, 224), (640, 640, 224, 224), (112, 112, 112, 112)]
KINDS = ("keystone", "affine")
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
DTYPES = ("f16", "f32")


def jobs_of(w, h, dw, dh, kind):
    """K (frame, nine floats, six floats or None): footprint corners on an even grid inside the frame"""
    import numpy as np

    from videoprocessingframework_amd import PytorchNvCodec as pnc

    rng = np.random.default_rng(w * 31 + h)
    out = []
    for i in range(K):
        x, y = 2 * int(rng.integers(0, (W - w) // 2 + 1)), 2 * int(rng.integers(0, (H - h) // 2 + 1))
        if kind == "affine":
            m6 = ((w - 1) / (dw - 1), 0.0, float(x), 0.0, (h - 1) / (dh - 1), float(y))
            out.append((i % FRAMES, m6 + (0.0, 0.0, 1.0), m6))
        else:
            quad = [[x + 0.15 * w, y], [x + 0.85 * w, y], [x + w - 1, y + h - 1], [x, y + h - 1]]
            m9 = pnc.quads_to_homographies(np.array([quad]), (dw, dh))[0].reshape(9).tolist()
            out.append((i % FRAMES, tuple(m9), None))
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
    rgb = torch.empty((FRAMES, H, 3 * W), dtype=torch.uint8, device=dev)
    scale, bias = capi.norm_params(MEAN, STD)
    lines, ok_a, over_b = [], True, []
    F = np.float32
    for w, h, dw, dh in SHAPES:
        for kind in KINDS:
            for dt in DTYPES:
                out = torch.empty((K, 3, dh, dw), dtype=tdt[dt], device=dev)
                e = out.element_size()
                dst = [[(out[i, c].data_ptr(), dw * e) for c in range(3)] for i in range(K)]
                norm = capi.make_tensor_norm(MEAN, STD, dtype={"f32": 0, "f16": 1}[dt])
                jobs = jobs_of(w, h, dw, dh, kind)
                persps = capi.make_persps([(fdesc[f], dst[i], m) for i, (f, m, _) in enumerate(jobs)])
                res = {"persp": bench.sustained(lambda: capi.convert_persp_tensor(ex, capi.NV12, 1, 0, W, H, dw, dh, persps, norm), pci=pci)}
                prev = capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, 9)
                res["gather"] = bench.sustained(lambda: capi.convert_persp_tensor(ex, capi.NV12, 1, 0, W, H, dw, dh, persps, norm), pci=pci)
                capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, prev)
                # the chain: maps prebuilt on the device with the definition's arithmetic (not timed), one conversion per frame, K remaps, torch
                dx, dy = np.arange(dw, dtype=F)[None, :], np.arange(dh, dtype=F)[:, None]
                xs, ys = [], []
                for _, m, _ in jobs:
                    m = np.array(m, dtype=F)
                    den = (m[6] * dx + m[7] * dy) + m[8]
                    xs.append(((m[0] * dx + m[1] * dy) + m[2]) / den)
                    ys.append(((m[3] * dx + m[4] * dy) + m[5]) / den)
                xm, ym = torch.from_numpy(np.stack(xs).astype(F)).to(dev), torch.from_numpy(np.stack(ys).astype(F)).to(dev)
                packed = torch.zeros((K, dh, 3 * dw), dtype=torch.uint8, device=dev)
                sc = torch.tensor(scale, dtype=torch.float32, device=dev).view(1, 3, 1, 1)
                bi = torch.tensor(bias, dtype=torch.float32, device=dev).view(1, 3, 1, 1)

                def run_chain():
                    for f in range(FRAMES):
                        capi.convert(ex, capi.NV12, capi.RGB, 1, 0, W, H, fdesc[f], [(rgb[f].data_ptr(), 3 * W)])
                    for i, (f, _, _) in enumerate(jobs):
                        capi.remap(ex, capi.RGB, W, H, (rgb[f].data_ptr(), 3 * W), xm[i].data_ptr(), 4 * dw, ym[i].data_ptr(), 4 * dw, dw, dh,
                                   (packed[i].data_ptr(), 3 * dw))
                    out.copy_(packed.view(K, dh, dw, 3).permute(0, 3, 1, 2).to(torch.float32) * sc + bi)

                res["chain"] = bench.sustained(run_chain, pci=pci)
                if kind == "affine":
                    warps = capi.make_warps([(fdesc[f], dst[i], m6) for i, (f, _, m6) in enumerate(jobs)])
                    res["warp"] = bench.sustained(lambda: capi.convert_warp_tensor(ex, capi.NV12, 1, 0, W, H, dw, dh, warps, norm), pci=pci)
                per = {k: r["us"] / K for k, r in res.items()}
                c1 = per["persp"] < per["chain"]
                ok_a = ok_a and c1
                row = f"{w}x{h} -> {dw}x{dh} {kind:8s} {dt}"
                lines.append(f"{row}: " + "  ".join(
                    f"{k} {per[k]:7.3f} us/region (spread {(max(res[k]['blocks_us']) - min(res[k]['blocks_us'])) / K:.3f}, sclk {res[k]['sclk_mhz']})" for k in res))
                tail = ""
                if "warp" in per:
                    r = per["persp"] / per["warp"]
                    tail = f"   persp / warp = {r:5.2f} [b: 1.25 allowed{'' if r <= 1.25 else ', ABOVE'}]"
                    if r > 1.25:
                        over_b.append(f"{row} ({r:.2f})")
                lines.append(f"    chain / persp = {per['chain'] / per['persp']:6.2f}x [a: {'pass' if c1 else 'FAIL'}]   gather / persp = {per['gather'] / per['persp']:5.2f}" + tail)
                print("\n".join(lines[-2:]), flush=True)
                del out, xm, ym, packed
                torch.cuda.empty_cache()
    lines.append("")
    lines.append(f"b (persp / warp on the affine-equivalent matrices, 1.25 allowed): {'every row within it' if not over_b else 'above it: ' + '; '.join(over_b)}")
    lines.append(f"a (faster than the convert + K remaps + torch chain): {'every case passes' if ok_a else 'SOME CASES FAIL'}")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    a = ap.parse_args()
    head = (f"tools/persp_tensor_bench.py: K = {K} jobs over {FRAMES} NV12 {W}x{H} frames, BT.709 MPEG, ImageNet mean / std; microseconds per region, "
            f"median of five >= 60 ms blocks after 300 ms of pre-heat\n")
    text = head + measure()
    print(text.splitlines()[-1])
    if a.out:
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
