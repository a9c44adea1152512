#!/usr/bin/env python3
"""Do two source trees give the same gfx950 machine code?  No GPU needed.

usage: tools/kernel_text_diff.py [--functions] OLD [NEW]      OLD / NEW = a checkout's root directory or a git revision; NEW defaults to the work tree

engine.hip and every rollout_*.hip of both trees are compiled device-only with the flags of __graft_entry__.build_engine, the
gfx950 code object is unbundled and its .text (instructions), .rodata (kernel descriptors) and .note (registers, LDS, scratch
per kernel) are compared.  Prints size and SHA-256 per unit and section for both trees; exit status 1 on any difference.

--functions: instead, disassemble both code objects of every unit and list the functions whose instruction streams differ, with
the instruction counts of both sides.  What moves when a neighbour changes length is masked: the literal of a pc-relative address
add (the s_add_u32 / s_addc_u32 pair behind s_getpc_b64), branch and call targets, and the alignment padding between a function's
end and the kernel symbol behind it.  Exit status 1 if any function is listed.
"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc", "-Wno-unused-result", "-Wno-unused-value"]
SECTIONS = (".text", ".rodata", ".note")


def tree_of(arg, tmp):
    """Root directory holding mujoco_mpc_amd/csrc and include/ for a directory or a git revision."""
    if os.path.isdir(os.path.join(arg, "mujoco_mpc_amd", "csrc")):
        return os.path.abspath(arg)
    dst = tempfile.mkdtemp(prefix="src_", dir=tmp)
    tar = subprocess.run(["git", "-C", ROOT, "archive", arg, "mujoco_mpc_amd/csrc", "include"], check=True, stdout=subprocess.PIPE).stdout
    subprocess.run(["tar", "-x", "-C", dst], input=tar, check=True)
    return dst


def units(tree):
    return sorted(f for f in os.listdir(os.path.join(tree, "mujoco_mpc_amd", "csrc"))
                  if f == "engine.hip" or (f.startswith("rollout_") and f.endswith(".hip")))


def sections(tree, unit, out):
    """{section: (size, sha256)} of one unit's gfx950 code object."""
    csrc = os.path.join(tree, "mujoco_mpc_amd", "csrc")
    base = os.path.join(out, unit[:-4])
    subprocess.check_call([HIPCC] + FLAGS + ["--cuda-device-only", "-c", "-o", base + ".bundle", os.path.join(csrc, unit)], cwd=csrc)
    subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                           "--input=" + base + ".bundle", "--output=" + base + ".co"])
    res = {}
    for s in SECTIONS:
        subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=" + s, base + ".co", base + s])
        data = open(base + s, "rb").read()
        res[s] = (len(data), hashlib.sha256(data).hexdigest())
    return res


GETPC = re.compile(r"s_getpc_b64 s\[(\d+):(\d+)\]")
PCADD = re.compile(r"(s_addc?_u32) s(\d+), s(\d+), \S+$")
TARGET = re.compile(r"(s_c?branch\w*|s_call_b64( \S+)?) \S+$")
PADDING = ("s_nop 0", "s_code_end", "...")


def functions(co):
    """{demangled symbol: [masked instruction, ...]} of one code object's .text, in address order."""
    objdump = os.path.join(LLVM, "llvm-objdump")
    # a kernel is a symbol with a descriptor: "NAME.kd", which --demangle prints as "DEMANGLED (.kd)"
    kernels = set()
    for line in subprocess.check_output([objdump, "-t", "--demangle", co], text=True).splitlines():
        name = re.sub(r"^\S+ +(\.\w+ )?", "", line.split("\t")[-1])          # behind the tab: size, visibility, name
        if name.endswith(".kd") or name.endswith(" (.kd)"):
            kernels.add(name[:-6] if name.endswith(")") else name[:-3])
    funcs, order, pc = {}, [], set()
    for line in subprocess.check_output([objdump, "-d", "--demangle", "--no-show-raw-insn", co], text=True).splitlines():
        m = re.match(r"[0-9a-f]+ <(.*)>:$", line)
        if m:
            order.append(m.group(1)); funcs[order[-1]] = []; pc = set()
            continue
        ins = " ".join(line.split("//")[0].split())
        if not order or not ins or not line[:1].isspace():
            continue
        m = GETPC.match(ins)
        if m:
            pc = set(m.groups())                        # the two halves, each until the add that turns it into an address
        elif pc:
            m = PCADD.match(ins)
            if m and m.group(2) == m.group(3) and m.group(2) in pc:
                ins = f"{m.group(1)} s{m.group(2)}, s{m.group(3)}, <pc-relative>"
                pc.discard(m.group(2))
        ins = TARGET.sub(lambda t: t.group(1) + " <target>", ins)
        funcs[order[-1]].append(ins)
    for name, after in zip(order, order[1:] + [None]):
        if after is None or after in kernels:
            while funcs[name] and funcs[name][-1] in PADDING:
                funcs[name].pop()
    return funcs


def main_functions(argv):
    with tempfile.TemporaryDirectory() as tmp:
        trees = [tree_of(argv[0], tmp), tree_of(argv[1], tmp) if len(argv) == 2 else ROOT]
        names = sorted(set(units(trees[0])) | set(units(trees[1])))
        jobs, outs = {}, [tempfile.mkdtemp(prefix="obj_", dir=tmp) for _ in trees]
        with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
            for k, tree in enumerate(trees):
                for u in units(tree):
                    jobs[k, u] = pool.submit(sections, tree, u, outs[k])
        listed = 0
        for u in names:
            for k in (0, 1):
                if (k, u) in jobs:
                    jobs[k, u].result()
            a, b = (functions(os.path.join(outs[k], u[:-4] + ".co")) if (k, u) in jobs else {} for k in (0, 1))
            moved = [f for f in list(a) + [f for f in b if f not in a] if a.get(f) != b.get(f)]
            print(f"{u:24s} {len(a):4d} / {len(b):4d} functions, {len(moved)} differ")
            for f in moved:
                print(f"    {f}: {len(a[f]) if f in a else 'missing'} -> {len(b[f]) if f in b else 'missing'} instructions")
            listed += len(moved)
    print("every function identical" if not listed else f"{listed} function(s) differ")
    return 1 if listed else 0


def main(argv):
    if len(argv) > 1 and argv[1] == "--functions" and len(argv) in (3, 4):
        return main_functions(argv[2:])
    if len(argv) not in (2, 3):
        sys.exit(__doc__)
    with tempfile.TemporaryDirectory() as tmp:
        trees = [tree_of(argv[1], tmp), tree_of(argv[2], tmp) if len(argv) == 3 else ROOT]
        names = sorted(set(units(trees[0])) | set(units(trees[1])))
        jobs = {}
        with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
            for k, tree in enumerate(trees):
                out = tempfile.mkdtemp(prefix="obj_", dir=tmp)
                for u in units(tree):
                    jobs[k, u] = pool.submit(sections, tree, u, out)
        differ = 0
        for u in names:
            for s in SECTIONS:
                a, b = (jobs[k, u].result()[s] if (k, u) in jobs else (0, "missing") for k in (0, 1))
                same = a == b
                differ += not same
                print(f"{u:20s} {s:8s} {a[0]:8d} {a[1]}  {b[0]:8d} {b[1]}  {'same' if same else 'DIFFERENT'}")
    print("identical" if not differ else f"{differ} section(s) differ")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
