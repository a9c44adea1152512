"""csrc/devbuf.h, the owner of every device / pinned buffer of the engine's host side, on the CPU: a stand-alone program
(tests/host/devbuf_main.cpp) compiled with plain g++ against fake allocation calls (tests/stubs_hip) that count live allocations,
catch a double free and fail on request."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_devbuf_grows_fails_and_releases_cleanly(tmp_path):
    exe = str(tmp_path / "devbuf_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "tests", "stubs_hip"),
                           "-I" + os.path.join(ROOT, "mujoco_mpc_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "host", "devbuf_main.cpp")])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "devbuf ok", run.stdout
