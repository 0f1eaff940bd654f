#!/usr/bin/env python3
"""Static ISA statistics of one translation unit's gfx950 kernels (no GPU needed): instruction mix per kernel, VGPR / SGPR / LDS use,
occupancy-relevant numbers, and per-loop-body counts.  python tools/isa_stats.py csrc/k_resize.hip [name-substring ...]
python tools/isa_stats.py --spills csrc/k_lanczos_mfma.hip: one line per kernel (VGPRs, spilled VGPRs / SGPRs, scratch bytes) and exit status 1 when any
kernel of the translation unit spills a VGPR or uses scratch (tests/test_isa_no_spills.py: VERDICT r4 item 5).
python tools/isa_stats.py --compare OLD_ROOT NEW_ROOT k_convert_roi.hip ...: the same translation units compiled from two source roots (a `git worktree`
of the parent commit and the working tree), per kernel the resources and whether the instruction stream is the same; exit status 1 when any differs."""
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def asm_of(src):
    out = os.path.join(tempfile.mkdtemp(), "k.s")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize", "-mllvm",
                           "-amdgpu-kernarg-preload-count=16", f"-I{ROOT}/include", f"-I{ROOT}/videoprocessingframework_amd/csrc", "-S", "--cuda-device-only",
                           src, "-o", out], stderr=subprocess.DEVNULL)
    return open(out).read()


def klass(i):
    if i.startswith("v_"):
        return "valu"
    if i.startswith("s_"):
        return "salu"
    if i.startswith("ds_"):
        return "lds"
    if i.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vmem"
    return "other"


def spills(src):
    """[(kernel, vgprs, spilled vgprs, spilled sgprs, scratch bytes)] from the code object's metadata"""
    s = asm_of(src)
    out = []
    for blk in s.split("  - .agpr_count:")[1:]:
        g = lambda key: int(re.search(key + r":\s+(\d+)", blk).group(1))
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        out.append((subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip() or name, g(r"\.vgpr_count"), g(r"\.vgpr_spill_count"),
                    g(r"\.sgpr_spill_count"), g(r"\.private_segment_fixed_size")))
    return out


def kernels_of(s):
    """{demangled name: (instruction lines with comments stripped and local labels numbered in order of appearance, vgpr, sgpr, static lds, scratch,
    spilled vgprs + sgprs)}"""
    lines = s.split("\n")
    spilled = {re.search(r"\.name:\s+(\S+)", b).group(1): sum(int(v) for v in re.findall(r"\.[sv]gpr_spill_count:\s+(\d+)", b)) for b in s.split("  - .agpr_count:")[1:]}
    idx = {l.split(":")[0]: n for n, l in enumerate(lines) if ":" in l and not l.startswith((".", " ", "\t", ";"))}
    found = [(m.group(1), m.group(2)) for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", s, flags=re.S) if m.group(1) in idx]
    dems = subprocess.run(["c++filt"], input="\n".join(n for n, _ in found), capture_output=True, text=True).stdout.split("\n")  # one call for all
    out = {}
    for (name, md), dem in zip(found, dems):
        body, n, labels = [], idx[name] + 1, {}
        while n < len(lines) and not lines[n].startswith(".Lfunc_end"):
            l = lines[n].split(";")[0].rstrip()
            n += 1
            if re.match(r"\.LBB\d+_\d+:", l):
                labels.setdefault(l[:-1], f".L{len(labels)}")
            elif l.startswith("\t") and not l.strip().startswith("."):
                body.append(" ".join(l.split()))
        ins = [re.sub(r"\.LBB\d+_\d+", lambda t: labels.get(t.group(0), "?"), l) for l in body]
        g = lambda key: int(re.search(key + r" (\d+)", md).group(1))
        out[re.sub(r"^void (vpf::)?|\(.*$", "", dem.strip() or name)] = (ins, g("next_free_vgpr"), g("next_free_sgpr"), g("group_segment_fixed_size"), g("private_segment_fixed_size"),
                                                               spilled[name])
    return out


def old_name(new):
    """the parent's spelling of a kernel whose layout became its last template argument: k_x<S..., 8> was k_x_nhwc<S...>, k_x<S..., 6> was k_x<S...>
    (FC_TENSOR_NHWC = 8, FC_TENSOR = 6); k_tensor_yuv_*<..., true> was k_tensor_yuv_*_nhwc<...>, <..., false> k_tensor_yuv_*<...>"""
    m = re.match(r"(k_(?:roi|warp|persp)_(?:strip|gather|dev))<(.*), ([68])>$", new)
    if m:
        return f"{m.group(1)}{'_nhwc' if m.group(3) == '8' else ''}<{m.group(2)}>"
    m = re.match(r"(k_tensor_yuv_(?:quad|r))<(.*), (true|false)>$", new)
    if m:
        return f"{m.group(1)}{'_nhwc' if m.group(3) == 'true' else ''}<{m.group(2)}>"
    m = re.match(r"(k_convert_half(?:_one)?)<(\d+), (\d+)(.*)>$", new)  # <SRC, DST, ...> was <DST, SRC, ...>
    if m:
        return f"{m.group(1)}<{m.group(3)}, {m.group(2)}{m.group(4)}>"
    return new


def compare(old_root, new_root, units):
    """per kernel of `units` (paths below videoprocessingframework_amd/csrc) compiled from two source roots: instructions, VGPR, SGPR, static LDS, scratch and
    spilled registers of the new root (and of the old one where they differ), and whether the normalised instruction streams are the same"""
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize", "-mllvm", "-amdgpu-kernarg-preload-count=16", "-S",
             "--cuda-device-only"]

    def asm(root, unit):
        out = os.path.join(tempfile.mkdtemp(), "k.s")
        subprocess.check_call(["/opt/rocm/bin/hipcc", *flags, f"-I{root}/include", f"-I{root}/videoprocessingframework_amd/csrc",
                               os.path.join(root, "videoprocessingframework_amd", "csrc", unit), "-o", out], stderr=subprocess.DEVNULL)
        return open(out).read()

    n_id = n_diff = 0
    for unit in units:
        old, new = kernels_of(asm(old_root, unit)), kernels_of(asm(new_root, unit))
        print(f"== {unit}: {len(new)} kernels ({len(old)} in the old root)")
        for name in sorted(new):
            ins, *res = new[name]
            o = old.pop(old_name(name) if old_name(name) in old else name, None)  # (an old root that already spells the kernel as the new one does)
            if o is None:
                print(f"  {name:60s} {len(ins):5d} instr  vgpr {res[0]:3d} sgpr {res[1]:3d} lds {res[2]} scratch {res[3]} spills {res[4]}  NEW: no counterpart in the old root")
                n_diff += 1
                continue
            same = o[0] == ins and list(o[1:]) == res
            n_id, n_diff = n_id + same, n_diff + (not same)
            was = "" if same else f"  (old {old_name(name)}: {len(o[0])} instr vgpr {o[1]} sgpr {o[2]} lds {o[3]} scratch {o[4]} spills {o[5]}; stream {'same' if o[0] == ins else 'differs'})"
            print(f"  {name:60s} {len(ins):5d} instr  vgpr {res[0]:3d} sgpr {res[1]:3d} lds {res[2]} scratch {res[3]} spills {res[4]}  {'identical' if same else 'CHANGED'}{was}")
        for name in sorted(old):
            print(f"  {name:60s} GONE: no counterpart in the new root")
            n_diff += 1
    print(f"== {n_id} kernels identical, {n_diff} not")
    return n_diff


def main():
    if sys.argv[1] == "--compare":  # --compare OLD_ROOT NEW_ROOT unit.hip ...: e.g. a `git worktree` of the parent commit against the working tree
        sys.exit(1 if compare(os.path.abspath(sys.argv[2]), os.path.abspath(sys.argv[3]), sys.argv[4:]) else 0)
    if sys.argv[1] == "--spills":
        src = sys.argv[2]
        if not os.path.isabs(src):
            src = os.path.join(ROOT, "videoprocessingframework_amd", src) if not os.path.exists(src) else src
        bad = 0
        for name, vg, vs, ss, scr in spills(src):
            print(f"{name[:110]:110s} vgpr {vg:3d} spilled {vs} (sgpr {ss}) scratch {scr} B")
            bad += vs > 0 or scr > 0
        sys.exit(1 if bad else 0)
    src = sys.argv[1]
    if not os.path.isabs(src):
        src = os.path.join(ROOT, "videoprocessingframework_amd", src) if not os.path.exists(src) else src
    want = sys.argv[2:]
    s = asm_of(src)
    meta = {m.group(1): m.group(2) for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", s, flags=re.S)}
    lines = s.split("\n")
    idx = {l.split(":")[0]: n for n, l in enumerate(lines) if ":" in l and not l.startswith((".", " ", "\t", ";"))}
    for name, md in meta.items():
        dem = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip() or name
        if want and not any(w in dem for w in want):
            continue
        body, n = [], idx[name] + 1
        while n < len(lines) and not lines[n].startswith(".Lfunc_end"):
            body.append(lines[n])
            n += 1
        ins = [(l.strip().split()[0], l) for l in body if l.startswith("\t") and not l.strip().startswith((";", "."))]
        c = collections.Counter(klass(i) for i, _ in ins)
        special = collections.Counter()
        for i, _ in ins:
            for key in ("dot2", "dot4", "fma", "cvt", "perm", "alignb", "div_", "rcp", "mul_lo", "mad_u64", "ds_read", "ds_write", "ds_load", "ds_store", "global_load", "global_store", "s_waitcnt", "s_barrier"):
                if key in i:
                    special[key] += 1
        vg = re.search(r"next_free_vgpr (\d+)", md).group(1)
        sg = re.search(r"next_free_sgpr (\d+)", md).group(1)
        lds = re.search(r"group_segment_fixed_size (\d+)", md).group(1)
        scr = re.search(r"private_segment_fixed_size (\d+)", md).group(1)
        print(f"{dem[:140]}\n    vgpr {vg} sgpr {sg} static-lds {lds} scratch {scr} | static instr: {dict(c)}\n    {dict(special)}")


if __name__ == "__main__":
    main()
