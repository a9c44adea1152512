#!/usr/bin/env python3
"""Do two source trees give the same gfx950 machine code?  No GPU needed.

usage: tools/kernel_text_diff.py OLD [NEW]      OLD / NEW = a checkout's root directory or a git revision; NEW defaults to the work tree

engine.hip and every rollout_*.hip of both trees are compiled device-only with the flags of __graft_entry__.build_engine, the
gfx950 code object is unbundled and its .text (instructions), .rodata (kernel descriptors) and .note (registers, LDS, scratch
per kernel) are compared.  Prints size and SHA-256 per unit and section for both trees; exit status 1 on any difference.
"""
import hashlib
import os
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


def main(argv):
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
