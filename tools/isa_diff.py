#!/usr/bin/env python3
"""Which kernels of a HIP source kept their instruction stream?  Compares two device assemblies kernel by kernel.
usage: tools/isa_diff.py before.{s,hip} after.{s,hip}     (a source is compiled with the Makefile's flags, -S --cuda-device-only)
Per kernel of `after`: demangled name, instruction count, and `== <kernel of before>` or DIFFERS.  The stream is compared with
symbol names and block labels normalised, directives and comments dropped (so a kernel descriptor never counts)."""
import collections, os, re, subprocess, sys, tempfile
CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "sc_gameengine_amd", "csrc")
FLAGS = ["--offload-arch=gfx950", "-std=c++17", "-O3", "-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt",
         "-fno-fast-math", "-fno-slp-vectorize", "-fPIC", "-I", CSRC]

def assembly(path):
    if path.endswith(".s"): return open(path).read()
    with tempfile.TemporaryDirectory() as t:
        if subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, "-S", "--cuda-device-only", "-x", "hip", path, "-o", t + "/a.s"]).returncode:
            sys.exit(f"{path} does not compile")
        return open(t + "/a.s").read()

def kernels(text):
    """{mangled name: normalised instruction stream (labels included)} of every .amdhsa_kernel of the assembly"""
    names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)); out = {}; cur = None
    for line in text.splitlines():
        line = line.split(";")[0].strip()
        if line.endswith(":") and line[:-1] in names: cur = line[:-1]; out[cur] = []; continue
        if cur is None or not line: continue
        if line.startswith(".Lfunc_end"): cur = None; continue
        if line.startswith(".") and not line.endswith(":"): continue                      # a directive
        out[cur].append(re.sub(r"\b_Z\w+", "SYM", re.sub(r"\.L(BB|tmp)\d+_", r".L\1_", line)))
    return {k: "\n".join(v) for k, v in out.items()}

def demangle(name):
    d = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
    return re.sub(r"\(.*", "", d.replace("(anonymous namespace)::", "").replace("sctick::", ""))

before, after = kernels(assembly(sys.argv[1])), kernels(assembly(sys.argv[2]))
same = collections.defaultdict(list)
for k, v in before.items(): same[v].append(demangle(k))
differ = 0
for k, v in after.items():
    count = sum(1 for l in v.splitlines() if not l.endswith(":"))
    differ += v not in same
    print(f"{demangle(k):64s} {count:6d}  " + ("== " + ", ".join(same[v]) if v in same else "DIFFERS"))
print(f"{len(after)} kernels ({len(before)} before), {differ} differ")
