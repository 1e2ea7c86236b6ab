#!/usr/bin/env python3
"""Compare the gfx950 code objects of this tree's kernels with those of another checkout (CPU only: cross-compiles, runs nothing).

    python tools/codeobj_diff.py <other csrc dir> [--rename OLD=NEW]... [--allow KERNEL]... [--only FILE.hip]...

<other csrc dir> is booster_amd/csrc of a WHOLE checkout or worktree (of the parent, say): its build.py and include/ are used.
Every .hip of SOURCES is compiled from both directories, each with the flags of its own booster_amd/build.py (flags_of), plus --genco --no-gpu-bundle-output.
One row per kernel: VGPRs, SGPRs, scratch bytes, static LDS bytes, instruction count (other -> this where they differ) and `identical` / `differs` /
`only here` / `only there`.  `identical` = the disassembly without addresses and encodings is literally equal; nothing is normalised.
--rename replaces OLD by NEW (plain substrings) in the other side's demangled kernel names, to pair kernels whose names changed.
Exit status 1 if a kernel present on both sides under the SAME name differs and is not listed (demangled, or a substring of it) with --allow.
"""
import argparse
import importlib.util
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from booster_amd import build as B  # noqa: E402

LLVM = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")))), "llvm", "bin")
KEYS = (".vgpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size")


def tool(name):
    p = os.path.join(LLVM, name)
    return p if os.path.exists(p) else shutil.which(name)


def demangle(names):
    filt = tool("llvm-cxxfilt") or shutil.which("c++filt")
    if not filt or not names:
        return {n: n for n in names}
    out = subprocess.run([filt], input="\n".join(names) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
    return dict(zip(names, out))


def build_of(csrc):
    """the build module that belongs to a csrc directory: its file list and its flags"""
    spec = importlib.util.spec_from_file_location("other_build", os.path.join(os.path.dirname(csrc), "build.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    if not hasattr(m, "flags_of"):                     # a checkout from before flags_of was a module-level function: the same expression
        m.flags_of = lambda s: m.FLAGS + (["-fno-slp-vectorize"] if s in m.NO_SLP else []) + m.KERNARG_PRELOAD.get(s, []) + m.MFMA_VGPR_FORM.get(s, [])
    return m


def compile_one(bm, csrc, s, outdir):
    co = os.path.join(outdir, os.path.splitext(s)[0] + ".co")
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + [f for f in bm.flags_of(s) if f != "-fPIC"] + ["--genco", "--no-gpu-bundle-output", os.path.join(csrc, s), "-o", co]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("compile failed: %s\n%s" % (" ".join(cmd), r.stderr[-2000:]))
    return co


def kernels_of(co):
    """{demangled name: (vgprs, sgprs, scratch, lds, instruction count, text)} of one code object"""
    meta, cur = {}, None
    for line in subprocess.run([tool("llvm-readelf"), "--notes", co], capture_output=True, text=True, check=True).stdout.splitlines():
        m = re.match(r"^( *)(- )?(\.\w+):\s*(.*)$", line)
        if not m:
            continue
        if m.group(2) and len(m.group(1)) == 2:        # "  - .key": the next entry of amdhsa.kernels
            cur = {}
        if cur is not None and len(m.group(1)) + len(m.group(2) or "") == 4:
            cur[m.group(3)] = m.group(4)
            if m.group(3) == ".name":
                meta[m.group(4)] = cur
    text, name = {}, None
    for line in subprocess.run([tool("llvm-objdump"), "-d", co], capture_output=True, text=True, check=True).stdout.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            name = m.group(1)
            text[name] = []
        elif name and line.startswith("\t") and line.strip() != "...":      # "...": zero padding behind a kernel, not code
            text[name].append(re.sub(r"\s*//.*$", "", line).strip())
    dm = demangle(list(meta))
    return {dm[n]: tuple(int(meta[n].get(k, -1)) for k in KEYS) + (len(text.get(n, [])), "\n".join(text.get(n, []))) for n in meta}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("other")
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW")
    ap.add_argument("--allow", action="append", default=[], metavar="KERNEL")
    ap.add_argument("--only", action="append", default=[], metavar="FILE.hip")
    a = ap.parse_args()
    renames = [r.split("=", 1) for r in a.rename]
    for need in ("../build.py", "../../include/bamd.h"):
        if not os.path.exists(os.path.join(a.other, need)):
            sys.exit("%s: no %s beside it: point at booster_amd/csrc of a whole checkout" % (a.other, need))
    sides = {}
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(16) as pool:
        jobs = []
        for side, csrc, bm in (("this", B.CSRC, B), ("other", os.path.abspath(a.other), build_of(os.path.abspath(a.other)))):
            os.makedirs(os.path.join(tmp, side))
            for s in bm.SOURCES:
                if s.endswith(".hip") and os.path.exists(os.path.join(csrc, s)) and (not a.only or s in a.only):
                    jobs.append((side, pool.submit(compile_one, bm, csrc, s, os.path.join(tmp, side))))
        for side, j in jobs:
            sides.setdefault(side, {}).update(kernels_of(j.result()))
    this, other = sides.get("this", {}), {}
    same_name = set()
    for n, v in sides.get("other", {}).items():
        new = n
        for old, rep in renames:
            new = new.replace(old, rep)
        other[new] = v
        if new == n:
            same_name.add(n)
    bad = 0
    print("%-9s %-19s %-9s %-9s %-13s %-15s %s" % ("", "VGPRs", "SGPRs", "scratch", "static LDS", "instructions", "kernel"))
    for n in sorted(set(this) | set(other)):
        t, o = this.get(n), other.get(n)
        if t is None or o is None:
            v = t or o
            print("%-9s %-19s %-9s %-9s %-13s %-15s %s" % ("only here" if t else "only there", v[0], v[1], v[2], v[3], v[4], n))
            continue
        verdict = "identical" if t[5] == o[5] and t[:4] == o[:4] else "differs"
        if verdict == "differs" and n in same_name and not any(k in n for k in a.allow):
            bad += 1
        cols = ["%d" % t[i] if t[i] == o[i] else "%d -> %d" % (o[i], t[i]) for i in range(5)]
        print("%-9s %-19s %-9s %-9s %-13s %-15s %s" % (verdict, cols[0], cols[1], cols[2], cols[3], cols[4], n))
    print("%d kernels here, %d there; %d of the same name differ and are not allowed" % (len(this), len(other), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
