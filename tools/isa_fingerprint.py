"""DIAGNOSTIC: a fingerprint of the gfx950 ISA of every kernel and out-of-line device function, to
show that a change elsewhere in the library (another kernel, host code, a refactor) leaves the device
code as it was.
    python tools/isa_fingerprint.py [--csrc DIR] [extra hipcc flags ...]
Compiles csrc/ptmi_kernels.hip and csrc/ptmi_image_kernels.hip (those of DIR's that exist: a revision from
before the image passes had a file of their own has the first alone) to device assembly and prints
  - per trace_kernel<FL>: the instruction count, VGPRs, scratch bytes and a hash of the instruction
    stream up to the kernel's first s_endpgm, with labels renumbered in order of appearance (function
    numbering changes when other kernels come or go) -- the format of the committed fingerprint files;
  - then one `fn` line per function in the assembly (the trace kernels again, every other kernel, and
    the out-of-line device functions such as the ocml sin fallback), over the whole function: the same
    columns, registers and scratch from the function's own info block.  These are sorted by function name,
    so the listing does not depend on which file holds a function, or where in it."""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pathtracer-ocl_amd", "csrc")
SRCS = ("ptmi_kernels.hip", "ptmi_image_kernels.hip")  # the trace kernels are in the first


def device_asm(extra, src=os.path.join(CSRC, SRCS[0])):
    """The device assembly of one file: the trace kernels' by default (tools/isa_moves.py)."""
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "k.s")
        cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
               "-fno-fast-math", "-Wno-unused-result", "--cuda-device-only", "-S", "-o", out, src] + list(extra)
        subprocess.run(cmd, check=True)
        return open(out).read()


def stream_hashes(body):
    """(instruction count, hash, hash with kernel-argument offsets masked) of a block of assembly."""
    names, ins = {}, []
    for l in body.split("\n"):
        t = l.split(";")[0].strip()
        if not t or t.startswith("."):
            if t.endswith(":") and t.startswith(".LBB"):
                names.setdefault(t[:-1], "L%d" % len(names))
            continue
        if t.endswith(":"):
            continue
        ins.append(t)
    # (labels outside the block are not in `names`: drop the function number)
    norm = [re.sub(r"\.LBB\d+_(\d+)", lambda x: names.get(x.group(0), ".LBB_" + x.group(1)), t) for t in ins]
    h = hashlib.sha256("\n".join(norm).encode()).hexdigest()[:16]
    # the same with kernel-argument offsets masked (a field appended to a by-value argument
    # struct moves the later arguments' offsets and nothing else)
    ka = [re.sub(r"(s\[0:1\]), 0x[0-9a-f]+", r"\1, KA", t) for t in norm]
    hk = hashlib.sha256("\n".join(ka).encode()).hexdigest()[:16]
    return len(ins), h, hk


def fingerprints(asm):
    res = {}
    for m in re.finditer(r"^(_ZN4ptmi12trace_kernelILi(\d+)EEEv\w*):[^\n]*\n(.*?)\n\s*s_endpgm", asm, re.S | re.M):
        res[int(m.group(2))] = stream_hashes(m.group(3))
    # resource usage from the metadata block (one entry per kernel, in .amdgpu_metadata)
    meta = {}
    for mm in re.finditer(r"\.name:\s+(_ZN4ptmi12trace_kernelILi(\d+)EEEv\w*)", asm):
        fl = int(mm.group(2))
        blk = asm[mm.end():].split("- .agpr_count", 1)[0]  # the rest of this kernel's entry
        vg = re.search(r"\.vgpr_count:\s+(\d+)", blk)
        sc = re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk)
        meta[fl] = (vg.group(1) if vg else "?", sc.group(1) if sc else "?")
    return res, meta


def function_fingerprints(asm):
    """Every function of the assembly, kernel or not, label to .Lfunc_end: [(name, n, h, hk, vgpr, scratch)]."""
    out = []
    for m in re.finditer(r"^\t\.type\t(\S+),@function\n\1:[^\n]*\n(.*?)^\.Lfunc_end\d+:(.*?)^; MemoryBound", asm,
                         re.S | re.M):
        info = m.group(3)  # the function's info block: "; NumVgprs: N", "; ScratchSize: N"
        vg = re.search(r"^; NumVgprs: (\d+)", info, re.M)
        sc = re.search(r"^; ScratchSize: (\d+)", info, re.M)
        out.append((m.group(1),) + stream_hashes(m.group(2)) + (vg.group(1) if vg else "?", sc.group(1) if sc else "?"))
    return out


if __name__ == "__main__":
    args = sys.argv[1:]
    csrc = CSRC
    if args[:1] == ["--csrc"]:
        csrc, args = args[1], args[2:]
    asms = [device_asm(args, os.path.join(csrc, f)) for f in SRCS if os.path.exists(os.path.join(csrc, f))]
    res, meta = fingerprints(asms[0])
    for fl in sorted(res):
        n, h, hk = res[fl]
        vg, sc = meta.get(fl, ("?", "?"))
        print("trace_kernel<%-3d> insts %6d  vgpr %-4s scratch %-4s isa %s  isa-ka %s" % (fl, n, vg, sc, h, hk))
    for name, n, h, hk, vg, sc in sorted(fn for asm in asms for fn in function_fingerprints(asm)):
        print("fn %s insts %6d  vgpr %-4s scratch %-4s isa %s  isa-ka %s" % (name, n, vg, sc, h, hk))
