"""csrc/carve.h, the layouts of the device scratch of the engine's one-step calls, on the CPU: a stand-alone program
(tests/host/carve_main.cpp) compiled with plain g++, once as it is and once under the address and undefined-behaviour sanitizers.  It lays
every layout on a null base and on a heap block of exactly the reported size, writes every field's full extent, and compares every offset
and total with the closed forms the entry points used when they carved their blocks by hand."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [[], ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "sanitized"])
def test_layouts_are_sound_and_where_they_were(tmp_path, flags):
    exe = str(tmp_path / "carve_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror"] + flags +
                          ["-I" + os.path.join(ROOT, "mujoco_mpc_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "host", "carve_main.cpp")])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0 and run.stdout.strip().startswith("carve ok"), run.stdout
