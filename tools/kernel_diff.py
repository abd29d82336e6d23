#!/usr/bin/env python
"""Compares the kernels of two builds of libaten_amd.so: registers, LDS and scratch from the AMDGPU metadata, and the
disassembly with literal constants, addresses and branch targets masked (a build id compiled into the library, or a kernel
that moved inside its code object, is no difference).  Prints the kernels only one build has and every kernel that differs;
exit status 1 when a kernel both builds have differs.   usage: tools/kernel_diff.py old.so new.so"""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_regs import LLVM, code_objects  # noqa: E402

META = ("vgpr_count", "sgpr_count", "agpr_count", "private_segment_fixed_size", "group_segment_fixed_size", "vgpr_spill_count",
        "sgpr_spill_count", "kernarg_segment_size", "max_flat_workgroup_size")


def kernels(lib):
    """{mangled kernel name: (metadata tuple, masked disassembly)}"""
    out = {}
    for co in code_objects(lib):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(co); f.flush()
            notes = subprocess.check_output([LLVM + "/llvm-readelf", "--notes", f.name]).decode()
            dis = subprocess.check_output([LLVM + "/llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", f.name]).decode()
        meta = {}
        for blk in notes.split("- .agpr_count:")[1:]:
            blk = ".agpr_count:" + blk
            g = lambda k: (re.search(r"\.%s:\s+(\S+)" % k, blk) or [None, "?"])[1]
            meta[g("name")] = tuple(g(k) for k in META)
        body, name = {}, None
        for line in dis.splitlines():
            m = re.match(r"^[0-9a-f]* ?<([^>]+)>:$", line)
            if m:
                name = m.group(1)
                body[name] = []
                continue
            if name is None or not line.strip() or line.strip() == "...":      # ("...": objdump's mark for the zero padding behind a kernel)
                continue
            t = line.split("//")[0].strip()
            t = re.sub(r"<[^>]+>", "<L>", t)                       # branch targets, symbol references
            t = re.sub(r"\b0x[0-9a-fA-F]+\b", "C", t)              # literal constants
            t = re.sub(r"(?<![\w\[:.])-?\d+(\.\d+)?(?![\w\]:])", "C", t)  # decimal immediates (not register numbers)
            body[name].append(t)
        for k, v in meta.items():
            out[k] = (v, "\n".join(body.get(k, [])))
    return out


def main():
    if len(sys.argv) != 3:
        raise SystemExit(__doc__)
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    both = sorted(set(a) & set(b))
    bad = 0
    for k in both:
        what = []
        if a[k][0] != b[k][0]:
            what.append("metadata %s -> %s" % (a[k][0], b[k][0]))
        if a[k][1] != b[k][1]:
            what.append("disassembly")
        if what:
            bad += 1
            print("DIFFERS %s: %s" % (k, "; ".join(what)))
    for k in only_a:
        print("only in %s: %s" % (sys.argv[1], k))
    for k in only_b:
        print("only in %s: %s" % (sys.argv[2], k))
    print("%d kernels in both builds, %d differ; %d only in the first, %d only in the second" % (len(both), bad, len(only_a), len(only_b)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
