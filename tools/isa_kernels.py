#!/usr/bin/env python3
"""Per-kernel identity of the gfx950 device code of two trees (the method of profiles/points_home/isa_identity.txt).

Usage: tools/isa_kernels.py dump <tree> <out.json>      compile every source of <tree>'s build.py SOURCES to assembly
                                                         (build.py's flags, --cuda-device-only -S, a fixed -cuid) and record
                                                         for every kernel its file, stripped line count and sha256
       tools/isa_kernels.py compare <before.json> <after.json>   the table: one row per kernel of `before`

A kernel is its code block (`name:` .. `.Lfunc_end`) and its `.amdhsa_kernel` descriptor.  Comments and `.file` / `.ident`
lines are dropped (a label's comment names its loop header by the kernel's index), and the local labels lose the kernel's index in its file (.LBB<n>_<m> -> .LBB#_<m>), so a kernel that moved to
another file, or behind another kernel, compares equal when its instructions are."""
import hashlib
import importlib.util
import json
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor


def kernels_of(asm):
    """{kernel: [stripped lines]} of one assembly file"""
    lines = [l.split(";")[0].rstrip() for l in asm.splitlines() if not re.match(r"\s*(;|\.ident|\.file)", l)]
    names = [m.group(1) for l in lines for m in [re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l)] if m]
    out = {}
    for name in names:
        start = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
        end = next(i for i in range(start, len(lines)) if re.match(r"\.Lfunc_end\d+:", lines[i]))
        d0 = next(i for i, l in enumerate(lines) if re.match(r"\s*\.amdhsa_kernel\s+" + re.escape(name) + r"$", l))
        d1 = next(i for i in range(d0, len(lines)) if ".end_amdhsa_kernel" in lines[i])
        out[name] = [re.sub(r"\.L([A-Za-z_]+?)\d+", r".L\1#", l) for l in lines[start:end + 1] + lines[d0:d1 + 1]]
    return out


def dump(tree, out_path):
    spec = importlib.util.spec_from_file_location("apd_build", os.path.join(tree, "apd-mvs_amd", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    tmp = os.path.splitext(out_path)[0] + "_asm"   # kept: ISA_REUSE=1 hashes the assembly that is there again
    os.makedirs(tmp, exist_ok=True)
    with open(os.path.join(tmp, "apd_build_id.inc"), "w") as f:
        f.write('"isa_identity"\n')

    def one(src):
        s = os.path.join(tmp, src + ".s")
        cmd = [build.HIPCC] + build.FLAGS + build.FILE_FLAGS.get(src, []) + ["-I" + tmp, "-cuid=isa_identity", "--cuda-device-only", "-S",
                                                                             os.path.join(build.CSRC, src), "-o", s]
        if not (os.environ.get("ISA_REUSE") and os.path.exists(s)):
            subprocess.run(cmd, check=True)
        with open(s) as f:
            return src, kernels_of(f.read())

    table = {}
    with ThreadPoolExecutor(max_workers=int(os.environ.get("MAX_JOBS", "6"))) as ex:
        for src, ks in ex.map(one, build.SOURCES):
            for name, body in ks.items():
                assert name not in table, name
                n_inst = sum(1 for l in body if re.match(r"\s+[a-z]+_[a-z0-9_]+\s", l + " ") and not l.strip().startswith("."))
                table[name] = {"file": src, "lines": len(body), "instructions": n_inst,
                               "sha256": hashlib.sha256("\n".join(body).encode()).hexdigest()[:16]}
    with open(out_path, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
    print("%d kernels -> %s" % (len(table), out_path))


def compare(before_path, after_path):
    before, after = json.load(open(before_path)), json.load(open(after_path))
    demangle = lambda n: subprocess.run(["c++filt", n], stdout=subprocess.PIPE, text=True).stdout.strip().replace("(anonymous namespace)::", "").split("(")[0]
    print("%-64s %-24s %-24s %7s %7s  %-16s  %-16s  %s" % ("kernel", "file before", "file after", "lines", "lines", "sha256 before", "sha256 after", "cmp"))
    differ = 0
    for name in sorted(before, key=lambda n: (before[n]["file"], n)):
        b, a = before[name], after.get(name)
        verdict = "MISSING" if a is None else "identical" if a["sha256"] == b["sha256"] else "DIFFERS"
        differ += verdict != "identical"
        print("%-64s %-24s %-24s %7d %7s  %-16s  %-16s  %s" % (demangle(name)[-64:], b["file"], a["file"] if a else "-", b["lines"], a["lines"] if a else "-",
                                                              b["sha256"], a["sha256"] if a else "-", verdict))
    new = sorted(set(after) - set(before))
    print("kernels before: %d, after: %d, not identical: %d, only after: %s" % (len(before), len(after), differ, [demangle(n) for n in new] or "none"))
    return 1 if differ or new else 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "dump":
        dump(sys.argv[2], sys.argv[3])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
