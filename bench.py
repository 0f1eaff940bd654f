#!/usr/bin/env python3
"""bench.py — headline benchmark of the surface-conversion hot path on MI355X.

Metric (BASELINE.json): Gpix/s of NV12 -> RGB conversion of 3840x2160 frames + achieved fraction of the
HBM roofline, on 1/2/4/8 GPUs.  A "step" is one pass of the hot path over one batch of synthetic
input: `vpf_convert_batch` over a ring of RING distinct device-resident 4K NV12 frames into RING distinct
RGB frames (RING*37.3 MB >> the 256 MiB Infinity Cache, so the traffic is really HBM).  Inputs are resident
in HBM before the timed region starts.

  python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
         bench.py --gpus N --steps K --warmup W

A plain run does only what the headline needs: build the ring, pre-heat and warm up, time exactly K steps
in one block, and print one JSON line (ms_per_step = milliseconds per timed step).  --dump-outputs DIR
then also writes what the last timed step computed (a fixed sample of the ring's outputs) as DIR/<name>.npy.
--full adds what the headline does not need: the timed block repeated (--repeats, default 5 there; median reported),
the CPU baseline (cpu_baseline, unless --no-cpu) and the other BASELINE configs (other_configs).

Multi-GPU: frames are independent, so the ring is replicated per rank (weak scaling), no data-path
collective; ranks only meet at the timing barriers.  value = pixels converted by all ranks / max-over-ranks time.

Extra flags (not used by the driver): --variant V (kernel variant), --mode single (one dispatch per frame,
what the unmodified per-Execute() API does), --workload {nv12_rgb_4k, nv12_planar_1080p, resize_4k_720p,
fused_4k_720p}, --sweep (table of variants on stderr), --no-cpu, --extra (other_configs alone).
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
from videoprocessingframework_amd import capi, sharding  # noqa: E402  (capi raises if libvpfhip.so is missing: no fallback)

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md)
PMC_TRAFFIC_FILE = "r06_pmc_traffic.json"  # newest PMC traffic summary of the headline kernel under profiles/


def _pitched(rows, row_bytes, dev, gen=None, align=256):
    pitch = (row_bytes + align - 1) // align * align
    if gen is None:
        t = torch.empty((rows, pitch), dtype=torch.uint8, device=dev)
    else:
        t = torch.randint(0, 256, (rows, pitch), dtype=torch.uint8, device=dev, generator=gen)
    return t, pitch


def _rows_touched(S: int, D: int):
    """source rows a D-row bilinear resize of S rows reads, in the kernels' fp32 arithmetic: tap i0 always, tap i1 only when
    its weight is non-zero (4K -> 720p is exactly 3x: every centre falls on a source row, so one row per output row)"""
    d = np.arange(D, dtype=np.float32)
    s_ = np.clip((d + np.float32(0.5)) * np.float32(np.float32(S) / np.float32(D)) - np.float32(0.5), 0, S - 1).astype(np.float32)
    i0 = s_.astype(np.int64)
    i1 = np.minimum(i0 + 1, S - 1)
    rows = set(i0.tolist()) | set(i1[(s_ - i0.astype(np.float32)) != 0].tolist())
    return rows


class Workload:
    """Device-resident ring of frames + the launch closure for one step."""

    def __init__(self, name, dev, ring, variant, mode):
        self.name, self.dev, self.ring, self.mode = name, dev, ring, mode
        gen = torch.Generator(device=dev)
        gen.manual_seed(1000)
        self.ex = capi.make_exec(torch.cuda.current_stream().cuda_stream)
        self.keep = []
        capi.set_tuning(capi.TUNE_NV12_RGB_VARIANT, variant)
        if name in ("nv12_rgb_4k", "nv12_planar_1080p"):
            self.w, self.h = (3840, 2160) if name == "nv12_rgb_4k" else (1920, 1080)
            self.dst_fmt = capi.RGB if name == "nv12_rgb_4k" else capi.RGB_PLANAR
            w, h = self.w, self.h
            frames, dsts = [], []
            for _ in range(ring):
                src, sp = _pitched(h * 3 // 2, w, dev, gen)  # NV12: one W x 1.5H plane, shared pitch (reference layout)
                if self.dst_fmt == capi.RGB:
                    dst, dp = _pitched(h, 3 * w, dev)
                    dd = [(dst.data_ptr(), dp)]
                else:
                    dst, dp = _pitched(3 * h, w, dev)  # one W x 3H allocation, plane i at base + i*H*pitch
                    dd = [(dst.data_ptr() + i * h * dp, dp) for i in range(3)]
                self.keep += [src, dst]
                dsts.append(dst)
                frames.append(([(src.data_ptr(), sp), (src.data_ptr() + h * sp, sp)], dd))
            self.outputs = [("rgb", dsts, h, 3 * w) if self.dst_fmt == capi.RGB else ("rgb_planar", dsts, 3 * h, w)]  # --dump-outputs
            self.frames = [(capi.planes(s_), capi.planes(d_)) for s_, d_ in frames]  # descriptors built once, like a C caller
            self.batch = capi.make_batch(frames)
            self.px_per_step = ring * w * h
            self.bytes_per_step = ring * (w * h * 3 // 2 + 3 * w * h)  # algorithmic: 1.5 B/px read + 3 B/px written
            self.launches_per_step = (ring + 31) // 32 if mode == "batch" else ring
            self.kernel = ("k_nv12_rgb_p16x<RGB, NT stores, 4 workgroups/CU, NV12> (16 px x 2 rows per lane, blocks numbered straight through the picture, LDS-transposed non-temporal stores)" if self.dst_fmt == capi.RGB
                           else "k_nv12_planar_r16 (one row x 1024 px per wave, 16 px/lane, three 1-KiB non-temporal plane stores)")
        elif name in ("resize_4k_720p", "fused_4k_720p"):
            self.w, self.h, self.dw, self.dh = 3840, 2160, 1280, 720
            w, h = self.w, self.h
            self.items = []
            for _ in range(ring):
                src, sp = _pitched(h * 3 // 2, w, dev, gen)
                mid, mp = _pitched(h, 3 * w, dev)
                dst, dp = _pitched(self.dh, 3 * self.dw, dev)
                self.keep += [src, mid, dst]
                self.items.append((capi.planes([(src.data_ptr(), sp), (src.data_ptr() + h * sp, sp)]), capi.planes([(mid.data_ptr(), mp)]), capi.planes([(dst.data_ptr(), dp)])))
            self.outputs = [("rgb_720p", self.keep[2::3], self.dh, 3 * self.dw)]  # --dump-outputs: the 720p frames (the 4K intermediate is not returned by the fused path)
            self.px_per_step = ring * w * h
            luma_rows = _rows_touched(h, self.dh)  # algorithmic bytes at row granularity: only the rows the taps touch
            chroma_rows = {r >> 1 for r in luma_rows}
            if name == "fused_4k_720p":
                self.bytes_per_step = ring * (len(luma_rows) * w + len(chroma_rows) * w + 3 * self.dw * self.dh)
                self.launches_per_step = ring if mode == "single" else (ring + 31) // 32
                self.fbatch = capi.make_batch([(s_, d_) for s_, _, d_ in self.items])
            else:
                self.bytes_per_step = ring * (w * h * 3 // 2 + 3 * w * h + len(luma_rows) * 3 * w + 3 * self.dw * self.dh)
                self.launches_per_step = 2 * ring
            self.kernel = ("k_convert_resize_lds (exact-alignment shortcuts at 3x)" if name == "fused_4k_720p"
                           else "k_nv12_rgb_p16 + k_resize (odd integer factor: centre-sample kernel)")
        elif name in ("rgb_resize_1080p_720p_bilinear", "rgb_resize_1080p_720p_lanczos"):  # vpf_resize_batch: every frame of the ring, 32 per dispatch
            self.w, self.h, self.dw, self.dh = 1920, 1080, 1280, 720
            self.interp = capi.INTERP_LINEAR if name.endswith("bilinear") else capi.INTERP_LANCZOS3
            frames = []
            for _ in range(ring):
                src, sp = _pitched(self.h, 3 * self.w, dev, gen)
                dst, dp = _pitched(self.dh, 3 * self.dw, dev)
                self.keep += [src, dst]
                frames.append(([(src.data_ptr(), sp)], [(dst.data_ptr(), dp)]))
            self.outputs = [("rgb_720p", self.keep[1::2], self.dh, 3 * self.dw)]  # --dump-outputs
            self.batch = capi.make_batch(frames)
            self.px_per_step = ring * self.w * self.h
            self.bytes_per_step = ring * 3 * (self.w * self.h + self.dw * self.dh)  # algorithmic: source read once, destination written once
            self.launches_per_step = (ring + 31) // 32
            self.kernel = "RowBandTask (4 destination rows per wave)" if name.endswith("bilinear") else "k_lanczos_mfma (i8 matrix cores, per-shape weight tables)"
        else:
            raise SystemExit(f"unknown workload {name}")

    def step(self):
        ex = self.ex
        if self.name.startswith("rgb_resize_"):
            capi.resize_batch(ex, capi.RGB, self.interp, self.w, self.h, self.dw, self.dh, self.batch)
            return
        if self.name in ("nv12_rgb_4k", "nv12_planar_1080p"):
            if self.mode == "batch":
                capi.convert_batch(ex, capi.NV12, self.dst_fmt, capi.BT_709, capi.MPEG, self.w, self.h, self.batch)
            else:
                for s, d in self.frames:
                    capi.convert(ex, capi.NV12, self.dst_fmt, capi.BT_709, capi.MPEG, self.w, self.h, s, d)
        elif self.name == "fused_4k_720p" and self.mode == "batch":
            capi.convert_resize_batch(ex, capi.NV12, capi.RGB, capi.BT_709, capi.MPEG, self.w, self.h, self.dw, self.dh, self.fbatch)
        elif self.name == "fused_4k_720p":
            for s, _, d in self.items:
                capi.convert_resize(ex, capi.NV12, capi.RGB, capi.BT_709, capi.MPEG, self.w, self.h, s, self.dw, self.dh, d)
        else:
            for s, m, d in self.items:
                capi.convert(ex, capi.NV12, capi.RGB, capi.BT_709, capi.MPEG, self.w, self.h, s, m)
                capi.resize(ex, capi.RGB, capi.INTERP_LINEAR, self.w, self.h, m, self.dw, self.dh, d)

    def frame0(self):
        """(NV12 planes of ring slot 0 as numpy, GPU output of slot 0 as numpy) for the cpu_baseline leg's cross-check."""
        if self.name not in ("nv12_rgb_4k", "nv12_planar_1080p"):
            return None
        w, h = self.w, self.h
        src = self.keep[0].cpu().numpy()
        return [np.ascontiguousarray(src[:h, :w]), np.ascontiguousarray(src[h:, :w])], self.keep[1].cpu().numpy()


class RehearsalWorkload:
    """--rehearse-host: NO conversion happens and nothing is measured.  A host no-op of fixed duration stands in for the
    step so that the multi-rank control flow of this file (rendezvous, LOCAL_RANK handling, barrier placement, sum-units /
    max-time reduction, rank-0-only JSON line) can be executed by the CPU test suite under torch.distributed.run + gloo
    (tests/test_sharding_gloo.py).  The line it prints says "data": "rehearsal" and carries no roofline."""

    name, dev, w, h, ring, launches_per_step, kernel = "rehearsal", None, 3840, 2160, 32, 1, "none (host rehearsal)"

    def __init__(self, rank):
        self.px_per_step = self.ring * self.w * self.h
        self.bytes_per_step = self.px_per_step * 9 // 2
        self.sleep = 0.002 * (1 + rank)  # ranks differ on purpose: the reduction must pick the slowest

    def step(self):
        time.sleep(self.sleep)


def timed_block(wl, steps: int):
    """EXACTLY `steps` steps bracketed by barrier + torch.cuda.synchronize on both sides -> (this rank's own host-clock seconds from its first
    launch to the return of its own synchronize, wall seconds incl. the closing barrier, this rank's device seconds from HIP events on the
    launch stream).  The job's time is the MAX over ranks of the FIRST figure: every rank starts behind the opening barrier, the slowest
    rank's launch -> synchronize span is when the job's work is done, and the closing collective's own latency (tens to hundreds of
    microseconds over RCCL — percent of a 3.7 ms region) is reported beside it (`barrier_ms`), not inside it."""
    gpu = wl.dev is not None
    if gpu:
        torch.cuda.synchronize()
    sharding.barrier(wl.dev)
    if gpu:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)  # on the launch stream
    t0 = time.perf_counter()
    if gpu:
        e0.record()
    for _ in range(steps):
        wl.step()
    if gpu:
        e1.record()
        torch.cuda.synchronize()
    t_own = time.perf_counter() - t0
    sharding.barrier(wl.dev)
    wall = time.perf_counter() - t0
    return t_own, wall, (e0.elapsed_time(e1) * 1e-3 if gpu else t_own)


def preheat(wl, ms: float):
    """Untimed and DECLARED (`preheat_ms` in the JSON line): the same dispatch repeated for ~ms milliseconds before the warm-up steps, so that
    clocks, the power state and the caches' steady state are those of a long run.  `--warmup 5` of this workload is 1 ms of work — a chip
    that idled during the build of the ring has not left its idle clocks by then, which showed as a 4 % spread between driver runs."""
    if ms <= 0 or wl.dev is None:
        return 0.0
    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < ms:
        for _ in range(8):
            wl.step()
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def sustained(fn, preheat_ms: float = 300.0, block_ms: float = 60.0, blocks: int = 5, pci=None):
    """THE timing protocol of every secondary table (round 6; VERDICT r5 item 2: two tools disagreed by 17 % on one kernel because one timed 0.65 ms
    after a single warm call and the other a few steps after ten idle seconds).  `fn` = one host call sequence (one step).  >= `preheat_ms` of the
    SAME calls untimed, then `blocks` blocks of >= `block_ms` each (HIP events on the current stream around the block, back to back: >= 300 ms
    timed in total), the MEDIAN block reported; the shader clock (sysfs pp_dpm_sclk, the starred level) read while the first and while the last
    timed block is still running on the GPU.  -> dict(us = microseconds per fn(), blocks_us, reps, sclk_mhz = (first, last), preheat_ms, timed_ms)."""
    fn(); torch.cuda.synchronize()
    t0, calls = time.perf_counter(), 0
    while True:
        for _ in range(4):
            fn()
        calls += 4
        torch.cuda.synchronize()
        el = (time.perf_counter() - t0) * 1e3
        if el >= preheat_ms:
            break
    per_call_ms = el / calls
    reps = max(3, int(np.ceil(block_ms / max(per_call_ms, 1e-6))))
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(blocks + 1)]
    sclk = [None, None]
    ev[0].record()
    for b in range(blocks):
        for _ in range(reps):
            fn()
        ev[b + 1].record()
        if b == 0 or b == blocks - 1:  # the host runs ahead of the queue: the GPU is inside this block's work now
            sclk[0 if b == 0 else 1] = sharding.current_sclk_mhz(pci)
    torch.cuda.synchronize()
    per = sorted(ev[b].elapsed_time(ev[b + 1]) * 1e3 / reps for b in range(blocks))
    return {"us": per[len(per) // 2], "blocks_us": [round(x, 3) for x in per], "reps": reps, "sclk_mhz": tuple(sclk), "preheat_ms": round(el, 1),
            "timed_ms": round(sum(per) * reps / 1e3, 1)}


def device_pci(index: int = 0):
    """PCI address of a device for `sustained(pci=...)` (None where it cannot be told: the clock columns then read None)"""
    return sharding.rank_identity(index).get("pci")


def timed(wl, steps: int, warmup: int, dist_on: bool):
    """one warm-up + one timed block (the sweeps' form) -> (own host seconds, device seconds)"""
    for _ in range(warmup):
        wl.step()
    t_own, _, ev = timed_block(wl, steps)
    return t_own, ev


def effective_cpus() -> int:
    """Hardware threads this process may really use: the affinity mask capped by the cgroup CPU quota (a container can
    see 256 CPUs and be throttled to 16; bursts shorter than one CFS period hide that, sustained work does not)."""
    n = len(os.sched_getaffinity(0))
    try:
        q, p = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            n = min(n, max(1, int(q) // int(p)))
    except (OSError, ValueError):
        try:
            q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            p = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0:
                n = min(n, max(1, q // p))
        except (OSError, ValueError):
            pass
    return n


def cpu_baseline(wl: Workload, budget_s=10.0):
    """The cpu_baseline leg — the only place bench.py touches oracle/.  The oracle's FP32 port of NV12->RGB (vectorised
    AVX2+FMA rows, OpenMP over rows) converts ring slot 0 of the SAME workload on the host cores for a bounded ~10 s
    sample; its output doubles as the checker of the GPU's slot-0 result (`matches_gpu`).  The thread count is the
    best of a calibration over {1, n/4, n/2, n} of the usable hardware threads (affinity capped by the cgroup quota), each
    trial long enough (>= 0.7 s) that CFS burst credit cannot flatter it; `cores` reports the count used."""
    import oracle as o  # test infrastructure: checker + reported baseline, never on the measured GPU path

    avail = effective_cpus()
    w, h = wl.w, wl.h
    src, gpu_out = wl.frame0()
    dst = o.alloc(o.RGB, w, h, fill=1)  # pre-touched

    def rate(threads, seconds=0.7):
        o.set_threads(threads)
        o.convert(o.NV12, o.RGB, o.BT_709, o.MPEG, w, h, src, o.FP32, dst)
        frames, t0 = 0, time.perf_counter()
        while time.perf_counter() - t0 < seconds:
            o.convert(o.NV12, o.RGB, o.BT_709, o.MPEG, w, h, src, o.FP32, dst)
            frames += 1
        return frames * w * h / (time.perf_counter() - t0)

    cands = sorted({1, max(1, avail // 4), max(1, avail // 2), avail})
    calib = {}
    for t in cands:  # ascending; stop as soon as more threads stop helping (SMT siblings / oversubscription)
        calib[t] = rate(t)
        if len(calib) > 1 and calib[t] < 1.05 * max(v for k, v in calib.items() if k != t):
            break
    best = max(calib, key=calib.get)
    o.release_threads()  # workers left over from a larger trial team must not idle-spin beside the timed team
    o.set_threads(best)
    n, t0 = 0, time.perf_counter()
    while True:
        o.convert(o.NV12, o.RGB, o.BT_709, o.MPEG, w, h, src, o.FP32, dst)
        n += 1
        el = time.perf_counter() - t0
        if el > budget_s:
            break
    o.set_threads(1)
    matches = bool(np.array_equal(gpu_out[:, :3 * w], dst[0]))
    return {"value": round(n * w * h / el / 1e9, 4), "unit": "Gpix/s", "cores": best, "kind": "port", "matches_gpu": matches,
            "decode_leg": decode_leg(),
            "sample": f"{n} frames of 3840x2160 NV12->RGB BT.709 limited in {el:.1f} s; oracle FP32 mode (AVX2+FMA rows, OpenMP), "
                      f"{best} threads; {avail} usable CPUs (affinity {len(os.sched_getaffinity(0))}, cgroup quota applied) (calibration Gpix/s: " +
                      ", ".join(f"{t}t={v / 1e9:.2f}" for t, v in calib.items()) + ")"}


def decode_leg():
    """The reference's only software component is libav decode (src/TC/src/FfmpegSwDecoder.cpp).  Where the bindings were built against libav
    (PyNvCodec.HAVE_LIBAV) and VPF_BENCH_CLIP names a clip, tools/clip_pipeline.py's decode-only leg is timed on it; this image has no libav."""
    clip = os.environ.get("VPF_BENCH_CLIP")
    try:
        sys.path.insert(0, os.path.join(ROOT, "videoprocessingframework_amd"))
        import PyNvCodec as nvc
        have = bool(getattr(nvc, "HAVE_LIBAV", False))
    except Exception:  # noqa: BLE001
        have = False
    if have and clip and os.path.exists(clip):
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import clip_pipeline
        n, dt, _, (cw, ch) = clip_pipeline.decode_only(nvc, clip, 2000)
        return {"clip": os.path.basename(clip), "size": f"{cw}x{ch}", "frames": n, "frames_per_s": round(n / dt, 1), "Gpix_per_s": round(n * cw * ch / dt / 1e9, 4),
                "threads": 1, "what": "libav demux + software decode + NV12 repack through PyFfmpegDecoder (host only)"}
    return ("not measurable here: the reference's only software component is libav decode, and this image has no libav" if not have
            else "no clip given (VPF_BENCH_CLIP)") + "; this is the conversion half only (the reference itself has no CPU converter)"


DUMP_VALUES = 12 << 20  # float32 values written by --dump-outputs in all: 48 MiB, under the 64 MB cap


def dump_outputs(wl: Workload, out_dir: str):
    """--dump-outputs: what the last timed step left in the ring's destination frames, as float32 `<name>.npy` of shape (ring, rows, row bytes).
    Every frame in full when the ring fits DUMP_VALUES, else the same rows of every frame: the first, the last and a sample drawn with a fixed seed
    (so two runs, or two builds, with the same arguments write the same positions).  Pitch padding is never written."""
    torch.cuda.synchronize()
    os.makedirs(out_dir, exist_ok=True)
    for name, frames, rows, row_bytes in wl.outputs:
        frames = frames[:max(1, DUMP_VALUES // (2 * row_bytes))]  # (a ring so long that two rows per frame would not fit: its first frames)
        keep = max(2, DUMP_VALUES // (len(frames) * row_bytes))
        if keep >= rows:
            idx = np.arange(rows)
        else:
            rng = np.random.default_rng(1000)
            idx = np.union1d([0, rows - 1], rng.choice(np.arange(1, rows - 1), keep - 2, replace=False))
        sel = torch.from_numpy(idx).to(frames[0].device)
        arr = torch.stack([f[:rows, :row_bytes].index_select(0, sel) for f in frames]).to(torch.float32).cpu().numpy()
        np.save(os.path.join(out_dir, f"{name}.npy"), arr)
        print(f"[dump] {name}.npy: {arr.shape} float32, rows {idx.size} of {rows} per frame", file=sys.stderr, flush=True)


def other_configs(dev, main_wl):
    """Short (a few steps each, median of three blocks) measurements of BASELINE.json's other configs and of the per-Execute() dispatch mode, so
    the one JSON line also carries them.  Same ring discipline (device-resident, > Infinity Cache); informational only."""
    res = {}
    pci = device_pci(dev.index or 0)
    del main_wl.keep[:]
    main_wl.outputs = []
    torch.cuda.empty_cache()
    for key, name, ring, mode, steps in (
            ("4k_nv12_rgb_one_dispatch_per_frame", "nv12_rgb_4k", 32, "single", 10),         # unmodified per-Execute() API
            ("1080p_nv12_rgb_planar_batched", "nv12_planar_1080p", 128, "batch", 10),          # configs[1]
            ("4k_nv12_rgb_then_resize_720p_per_frame", "resize_4k_720p", 16, "single", 4),     # configs[2], API-faithful
            ("4k_nv12_to_720p_rgb_fused_batched", "fused_4k_720p", 32, "batch", 10),           # configs[2], fused
            ("1080p_rgb_to_720p_bilinear_batched", "rgb_resize_1080p_720p_bilinear", 64, "batch", 10),   # vpf_resize_batch, north_star's filter
            ("1080p_rgb_to_720p_lanczos3_batched", "rgb_resize_1080p_720p_lanczos", 64, "batch", 10)):   # vpf_resize_batch, the reference resizer's filter
        wl = Workload(name, dev, ring, 0, mode)
        m = sustained(wl.step, pci=pci)  # the one protocol of every secondary number: 300 ms pre-heat of this very step, median of five >= 60 ms blocks, clocks beside it
        ev = m["us"] * 1e-6  # seconds per step
        res[key] = {"Gpix_s_src": round(wl.px_per_step / ev / 1e9, 1),
                    "algorithmic_GB_s": round(wl.bytes_per_step / ev / 1e9, 0),
                    "frac_of_8TB_s": round(wl.bytes_per_step / ev / 1e9 / HBM_PEAK_GBS, 3),
                    "us_per_frame": round(m["us"] / ring, 3), "sclk_mhz": m["sclk_mhz"], "timed_ms": m["timed_ms"], "reps_per_block": m["reps"]}
        del wl
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=None, help="ranks = GPUs of this node (default: WORLD_SIZE under torch.distributed.run, else 1)")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=None, help="the timed block of --steps steps is run this many times; the MEDIAN block is reported "
                    "(ms_per_step, value, roofline), all of them in per_repeat_ms (SURVEY 8d: median of 5).  Default 1 (exactly --steps timed "
                    "steps), 5 with --full")
    ap.add_argument("--preheat-ms", type=float, default=300.0, help="untimed, declared pre-heat of the same dispatch before --warmup (0 = none)")
    ap.add_argument("--ring", type=int, default=32, help="distinct frame pairs in the ring (32 x 37.3 MB = 1.19 GB)")
    ap.add_argument("--variant", type=int, default=0)
    ap.add_argument("--mode", choices=["batch", "single"], default="batch")
    ap.add_argument("--workload", default="nv12_rgb_4k")
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--extra", action="store_true", help="also measure the other BASELINE configs / dispatch modes (adds 'other_configs'); "
                    "off by default so the default run launches ONE kernel shape and its rocprofv3 average is the headline's")
    ap.add_argument("--full", action="store_true", help="everything beyond the headline: --repeats 5 unless given, the CPU baseline (unless --no-cpu) "
                    "and the other BASELINE configs (as --extra)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="after the timed steps, write what the last step computed (a fixed, "
                    "seeded sample of the ring's outputs, float32, <= 64 MB) as DIR/<name>.npy")
    ap.add_argument("--rehearse-host", action="store_true", help="control-flow rehearsal without a GPU (CPU test suite only): no conversion, "
                    "nothing measured, prints a line marked \"data\": \"rehearsal\"")
    ap.add_argument("--backend", default="nccl", help="process-group backend for N>1 (nccl = RCCL; gloo lets several ranks share one GPU for testing)")
    a = ap.parse_args()
    if a.repeats is None:
        a.repeats = 5 if a.full else 1

    rank, world, local = sharding.env_rank()
    dist_on = world > 1
    if a.gpus is None:
        a.gpus = world  # a torchrun line that does not repeat --gpus: the launcher's WORLD_SIZE is the answer
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` typed by hand: run the launch line the driver uses (one rank per GPU) as a child process; --standalone
        # lets the c10d rendezvous pick its own free port (binding one here and handing the number over would race with other processes)
        sys.exit(subprocess.call([sys.executable, "-m", "torch.distributed.run", "--standalone", "--local-addr", "127.0.0.1", "--nnodes=1",
                                  f"--nproc-per-node={a.gpus}", os.path.abspath(__file__)] + sys.argv[1:]))
    if a.gpus != world:
        raise SystemExit(f"--gpus {a.gpus} but WORLD_SIZE is {world}")
    if a.rehearse_host:
        if a.backend == "nccl":
            a.backend = "gloo"
        dev = red_dev = None
    else:
        if not torch.cuda.is_available():
            raise SystemExit("bench.py needs a GPU (the conversion path has no CPU fallback)")
        ndev = torch.cuda.device_count()
        if a.backend == "nccl" and world > ndev:
            raise SystemExit(f"{world} ranks over RCCL need {world} GPUs, this node shows {ndev} (use --backend gloo to let ranks share a GPU for testing)")
        local = local % ndev
        torch.cuda.set_device(local)
        dev = torch.device("cuda", local)
        red_dev = dev if a.backend == "nccl" else None  # gloo reduces CPU tensors
    sharding.init(a.backend, dev)  # one process per GPU over RCCL; ranks only meet at the timing barriers

    if a.sweep and rank == 0:
        # product kernels through the tuning hook (4 p4, 8 p16, 30 p16 at 4 workgroups/CU, 37 planar r16), then the measurement lab
        # (tools/lab/libvpfhip_lab.so: round 1's other forms + the bandwidth probes 15 / 22 / 23, which are NOT conversions)
        import ctypes as C
        sys.path.insert(0, os.path.join(ROOT, "tools", "lab"))
        import build_lab
        labso = C.CDLL(build_lab.build())
        labso.vpf_lab_nv12_rgb.argtypes = [C.POINTER(capi.Exec), C.c_int, C.c_int, C.c_int, C.c_int, capi.Size, C.c_uint32, C.POINTER(capi.FrameIO)]
        for wlname in ("nv12_rgb_4k", "nv12_planar_1080p"):
            for mode in ("batch", "single"):
                for v in (4, 8, 30, 45, 46, 37, -38, -41, -43, -15, -22, -23):   # negative: lab variant |v|
                    wl = Workload(wlname, dev, a.ring if wlname == "nv12_rgb_4k" else 4 * a.ring, max(v, 0), mode)
                    if v < 0:
                        frames_all = [capi.make_batch([(s_, d_) for s_, d_ in wl.frames[i:i + 32]]) for i in range(0, len(wl.frames), 32)]
                        one = [capi.make_batch([(s_, d_)]) for s_, d_ in wl.frames]

                        def lab_step(wl=wl, v=-v, frames_all=frames_all, one=one):
                            if wl.mode == "batch":
                                rc = 0
                                for chunk in frames_all:
                                    rc |= labso.vpf_lab_nv12_rgb(C.byref(wl.ex), v, wl.dst_fmt, capi.BT_709, capi.MPEG, capi.Size(wl.w, wl.h), len(chunk), chunk)
                            else:
                                rc = 0
                                for io in one:
                                    rc |= labso.vpf_lab_nv12_rgb(C.byref(wl.ex), v, wl.dst_fmt, capi.BT_709, capi.MPEG, capi.Size(wl.w, wl.h), 1, io)
                            if rc:
                                raise RuntimeError(f"lab variant {v}: rc {rc}")
                        if labso.vpf_lab_nv12_rgb(C.byref(wl.ex), -v, wl.dst_fmt, capi.BT_709, capi.MPEG, capi.Size(wl.w, wl.h), 1, one[0]) == 1:
                            continue  # this form does not exist for this output class
                        wl.step = lab_step
                    _, ev = timed(wl, a.steps, a.warmup, False)
                    nbytes = wl.bytes_per_step * (1 / 3 if v == -22 else 2 / 3 if v == -23 else 1)  # probes move only the reads / writes
                    gbs = nbytes * a.steps / ev / 1e9
                    tag = f"variant {v}" if v >= 0 else f"lab {-v}" + (" (probe, not a conversion)" if labso.vpf_lab_is_conversion(-v) == 0 else "")
                    print(f"[sweep] {wlname:18s} {mode:6s} {tag}: {wl.px_per_step * a.steps / ev / 1e9:8.1f} Gpix/s "
                          f"{gbs:7.0f} GB/s ({gbs / HBM_PEAK_GBS:.3f} of 8 TB/s)", file=sys.stderr, flush=True)
                    del wl
                    torch.cuda.empty_cache()
        for wlname in ("resize_4k_720p", "fused_4k_720p"):
            wl = Workload(wlname, dev, 8, 0, "single")
            _, ev = timed(wl, max(2, a.steps // 5), 1, False)
            st = max(2, a.steps // 5)
            print(f"[sweep] {wlname:18s}: {wl.px_per_step * st / ev / 1e9:8.1f} Gpix/s(src) {wl.bytes_per_step * st / ev / 1e9:7.0f} GB/s algorithmic",
                  file=sys.stderr, flush=True)
            del wl
            torch.cuda.empty_cache()

    wl = RehearsalWorkload(rank) if a.rehearse_host else Workload(a.workload, dev, a.ring, a.variant, a.mode)
    ident = sharding.rank_identity(None if a.rehearse_host else local)  # per-rank diagnostics (device, PCI address, NUMA node, clocks): the "ranks" array of the JSON line
    heated_ms = preheat(wl, 0.0 if a.rehearse_host else a.preheat_ms)
    ident["sclk_mhz_start"] = sharding.current_sclk_mhz(ident["pci"])
    for _ in range(a.warmup):
        wl.step()
    blocks = []  # per repeat: (whole-job pixels, MAX over ranks of the own launch -> synchronize time, this rank's device seconds, every rank's device ms per step, MAX wall incl. the closing barrier)
    for _ in range(max(1, a.repeats)):
        t_own, wall, ev = timed_block(wl, a.steps)
        px, tmax = sharding.aggregate(wl.px_per_step * a.steps, t_own, red_dev)  # sum of pixels, MAX time over ranks
        _, wmax = sharding.aggregate(0, wall, red_dev)
        blocks.append((px, tmax, ev, [round(t / a.steps * 1e3, 4) for t in sharding.gather(ev, red_dev)], wmax, t_own))
    order = sorted(range(len(blocks)), key=lambda i: blocks[i][1])
    total_px, wall_max, ev, per_rank_ms, wall_with_barrier, own = blocks[order[len(order) // 2]]  # the median block (same index on every rank: the times are all-reduced)
    # every rank's own account of the median block, next to where it ran: a slow rank in a scaling run is then visible in the line itself
    ident.update(sclk_mhz_end=sharding.current_sclk_mhz(ident["pci"]), own_ms_per_step=round(own / a.steps * 1e3, 4), event_ms_per_step=round(ev / a.steps * 1e3, 4))
    ranks = sharding.gather_objects(ident)

    if rank == 0:
        n_launch = wl.launches_per_step * a.steps
        avg_launch_s = ev / n_launch  # rank 0's HIP-event time over the timed region / launches in it
        bytes_per_launch = wl.bytes_per_step / wl.launches_per_step
        achieved = bytes_per_launch / avg_launch_s / 1e9
        traffic, traffic_source = None, None
        pmc = os.path.join(ROOT, "profiles", PMC_TRAFFIC_FILE)
        if a.workload == "nv12_rgb_4k" and a.variant == 0 and a.mode == "batch" and os.path.exists(pmc):
            # HBM bytes per launch from rocprofv3 PMC (FETCH_SIZE x2 + WRITE_SIZE, separate passes, calibrated on
            # known-byte copy kernels: tools/pmc_calib.hip, tools/gpu_pmc.sh) — collected OFFLINE (PMC passes cannot run
            # inside this process), scaled to this launch; `traffic_source` says so
            traffic = int(json.load(open(pmc))["hbm_bytes_per_frame"] * wl.ring / wl.launches_per_step)
            traffic_source = (f"offline: profiles/{PMC_TRAFFIC_FILE} (rocprofv3 --pmc passes of this kernel on an earlier box, tools/gpu_pmc.sh), "
                              "not measured in this run")
        out = {
            "metric": "Gpix/s NV12->RGB 3840x2160 + achieved %HBM-BW",
            "value": round(total_px / wall_max / 1e9, 2),
            "unit": "Gpix/s",
            "n_gpus": world,
            "steps": a.steps,
            "warmup": a.warmup,
            "ms_per_step": round(wall_max / a.steps * 1e3, 4),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "f32",  # u8 pixels in/out, fp32 FMA arithmetic, round-to-nearest-even saturating pack
            "data": "synthetic",
            "per_rank_ms_per_step": per_rank_ms,
            "ranks": ranks,  # per rank: device, pci, numa_node, sclk_mhz_start / _end, own_ms_per_step (host clock, launch -> synchronize), event_ms_per_step (HIP events), cpus
            "barrier_ms": round(max(0.0, wall_with_barrier - wall_max) * 1e3, 4),  # the closing barrier's own cost over the timed block: outside `value`; ms_per_step x steps + barrier_ms = the block's wall time
            "repeats": len(blocks), "per_repeat_ms": [round(b[1] / a.steps * 1e3, 4) for b in blocks],  # ms_per_step is their median
            "preheat_ms": round(heated_ms, 1),
            "config": {"workload": f"{a.workload}: {wl.w}x{wl.h} NV12 -> {'RGB' if a.workload != 'nv12_planar_1080p' else 'RGB_PLANAR'}, BT.709 limited range, "
                                   f"ring of {a.ring} device-resident frames per GPU, {wl.launches_per_step} dispatch(es) per step",
                       "mode": a.mode, "frames_per_step_per_gpu": a.ring, "variant": a.variant,
                       "sharding": "independent frame rings, one process per GPU, no collective"},
            "roofline": {"bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": traffic, "traffic_source": traffic_source,
                         "kernel": wl.kernel, "bytes_per_launch": int(bytes_per_launch),
                         "avg_launch_us": round(avg_launch_s * 1e6, 3), "launches": n_launch},
        }
        if a.rehearse_host:
            out["data"] = "rehearsal"
            out["rehearsal_units_per_s"], out["value"] = out["value"] * 1e9, None  # not a measurement of anything
            out["roofline"] = None
            out["config"] = {"workload": "host rehearsal of the multi-rank control flow: no conversion, nothing measured"}
        if a.dump_outputs and not a.rehearse_host:
            dump_outputs(wl, a.dump_outputs)
        if a.full and not a.no_cpu and world == 1 and a.workload == "nv12_rgb_4k" and not a.rehearse_host:
            out["cpu_baseline"] = cpu_baseline(wl)
        if (a.full or a.extra) and world == 1 and a.workload == "nv12_rgb_4k" and a.variant == 0 and a.mode == "batch":
            out["other_configs"] = other_configs(dev, wl)
        print(json.dumps(out), flush=True)
    if dist_on:
        sharding.barrier(dev)
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
