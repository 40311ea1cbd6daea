"""DIAGNOSTIC: register-to-register moves in the bounce stages of a lockstep trace_kernel<FL>.
    python tools/isa_moves.py [FL ...] [extra hipcc flags ...]        (FL default 0 8: the C2 and C3 kernels)
Compiles csrc/ptmi_kernels.hip to gfx950 assembly (tools/isa_fingerprint.py's command) and splits the
kernel at the start of each inlined find_closest_prims -- its scalar load of DevScene::n_planes /
n_planes_y, kernel-argument offset 0x1c -- which is where a bounce stage's work begins: the segments
are the prologue with the camera block, then one per stage (the last one runs on into the epilogue).
Per segment it prints the instructions, the VGPR-to-VGPR v_mov_b64 and v_mov_b32, the longest run of
consecutive v_mov_b64 copies (a copy of ro, rd and the mask is a run of nine), and scratch accesses.
The path state is 64-bit, so its copies are the v_mov_b64 column; the v_mov_b32 copies are the noise
arguments and the return values of normalize3, which every build has.  Last line: the kernel's
instruction count, VGPRs and scratch bytes.  A build of a revision with the single bounce loop (before
the staged loop; tools/build_variant.sh FROMREV) has one find_closest_prims and so two segments; its
loop-entry copies sit at the end of the first."""
import re
import sys

import isa_fingerprint as F

MOV64 = re.compile(r"v_mov_b64_e32 v\[\d+:\d+\], v\[\d+:\d+\]$")
MOV32 = re.compile(r"v_mov_b32_e32 v\d+, v\d+$")
MARK = re.compile(r"s_load_dwordx2 s\[\d+:\d+\], s\[\d+:\d+\], 0x1c$")  # S.n_planes, S.n_planes_y


def kernel_body(asm, fl):
    m = re.search(r"^(_ZN4ptmi12trace_kernelILi%dEEEv\w*):[^\n]*\n(.*?)\n\s*s_endpgm" % fl, asm, re.S | re.M)
    if not m:
        raise SystemExit("no trace_kernel<%d>" % fl)
    ins = []
    for l in m.group(2).split("\n"):
        t = l.split(";")[0].strip()
        if t and not t.startswith(".") and not t.endswith(":"):
            ins.append(t)
    return ins


def segments(ins):
    cuts = [i for i, t in enumerate(ins) if MARK.match(t)]
    segs, a = [], 0
    for c in cuts:
        segs.append(ins[a:c])
        a = c
    segs.append(ins[a:])
    return segs


def row(name, seg):
    run = best = 0
    for t in seg:
        run = run + 1 if MOV64.match(t) else 0
        best = max(best, run)
    return "| %-28s | %5d | %3d | %3d | %3d | %3d |" % (
        name, len(seg), sum(1 for t in seg if MOV64.match(t)), best, sum(1 for t in seg if MOV32.match(t)),
        sum(1 for t in seg if t.startswith("scratch_")))


if __name__ == "__main__":
    fls = [int(a) for a in sys.argv[1:] if a.isdigit()] or [0, 8]
    extra = [a for a in sys.argv[1:] if not a.isdigit()]
    asm = F.device_asm(extra)
    res, meta = F.fingerprints(asm)
    for fl in fls:
        ins = kernel_body(asm, fl)
        segs = segments(ins)
        print("trace_kernel<%d>%s" % (fl, "  (" + " ".join(extra) + ")" if extra else ""))
        print("| segment                      | insts | v_mov_b64 v,v | longest run | v_mov_b32 v,v | scratch |")
        print("|---|---|---|---|---|---|")
        for i, s in enumerate(segs):
            name = ("prologue, camera block" if i == 0 else
                    "bounce code %d" % (i - 1) if i + 1 < len(segs) else "bounce code %d, epilogue" % (i - 1))
            print(row(name, s))
        print("total: %d instructions, %s VGPRs, %s B/lane scratch\n" % (len(ins), meta[fl][0], meta[fl][1]))
