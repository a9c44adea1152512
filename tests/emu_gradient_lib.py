"""Loader for the 1-lane emulation build of the Sample-Gradient device functions (tests/emu/emu_gradient.cpp; TEST INFRASTRUCTURE ONLY)."""
import ctypes as C
import fcntl
import os
import subprocess

import numpy as np

import emu_lib

EMU_SO = os.path.join(emu_lib.EMU_DIR, "libmjpc_emu_gradient.so")
c_double_p = emu_lib.c_double_p
c_int_p = emu_lib.c_int_p

_lib = None


def lib():
    global _lib
    if _lib is None:
        csrc = os.path.join(emu_lib.ROOT, "mujoco_mpc_amd", "csrc")
        src = os.path.join(emu_lib.EMU_DIR, "emu_gradient.cpp")
        srcs = [src] + [os.path.join(csrc, f) for f in ("gradient.h", "spmd.h", "dmath.h")]
        asan = bool(os.environ.get("MJPC_EMU_ASAN"))      # memory-checked build, as for emu_lib
        so = EMU_SO[:-3] + "_asan.so" if asan else EMU_SO
        flags = ["-O1", "-g", "-fsanitize=address"] if asan else ["-O2"]
        with open(os.path.join(emu_lib.EMU_DIR, ".build.lock"), "w") as lock:
            fcntl.flock(lock, fcntl.LOCK_EX)
            if (not os.path.exists(so)) or any(os.path.getmtime(s_) > os.path.getmtime(so) for s_ in srcs):
                tmp = so + f".{os.getpid()}.tmp"
                subprocess.check_call(["g++"] + flags + ["-fPIC", "-shared", "-std=c++17", "-ffp-contract=off", "-o", tmp, src])
                os.replace(tmp, so)
        _lib = C.CDLL(so)
        _lib.emu_sg_assemble.argtypes = [c_double_p] * 4 + [c_double_p, c_double_p, C.c_longlong] + [C.c_int] * 6
        _lib.emu_sg_assemble.restype = None
        _lib.emu_sg_gradient.argtypes = [c_double_p, C.c_longlong, c_int_p, c_double_p, C.c_int, C.c_int, c_double_p]
        _lib.emu_sg_gradient.restype = None
        _lib.emu_sg_shape.argtypes = [c_int_p]
        _lib.emu_sg_shape.restype = None
    return _lib


def _dp(a):
    return a.ctypes.data_as(c_double_p)


def assemble(nominal, noise_std, eps, ctrlrange, cand, hist, offset, nominal_index, first_explicit):
    """runs sg_assemble over the table in place: cand [nlocal][P][nu] (rows >= first_explicit: the caller's, left alone), hist
    [max_local][stride]; eps [nlocal][P][nu] are the local rows' normals"""
    nl, P, nu = eps.shape
    for a in (nominal, noise_std, eps, ctrlrange, cand, hist):
        assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    assert cand.shape == eps.shape and hist.shape[0] >= nl and hist.shape[1] >= P * nu
    lib().emu_sg_assemble(_dp(nominal), _dp(noise_std), _dp(eps), _dp(ctrlrange), _dp(cand), _dp(hist), hist.shape[1], int(offset), nl,
                          P * nu, nu, int(nominal_index), int(first_explicit))


def gradient(hist, slot, scale, PN):
    slot = np.ascontiguousarray(slot, np.int32); scale = np.ascontiguousarray(scale, np.float64)
    assert hist.dtype == np.float64 and hist.flags["C_CONTIGUOUS"] and slot.min() >= 0 and slot.max() < hist.shape[0] and PN <= hist.shape[1]
    g = np.full(PN, np.nan)
    lib().emu_sg_gradient(_dp(hist), hist.shape[1], slot.ctypes.data_as(c_int_p), _dp(scale), int(slot.size), int(PN), _dp(g))
    return g


def shape():
    o = np.zeros(4, np.int32)
    lib().emu_sg_shape(o.ctypes.data_as(c_int_p))
    return dict(KT=int(o[0]), U=int(o[1]), PROD=int(o[2]), T=int(o[3]))
