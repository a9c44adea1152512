"""Lone-wave timing of the multi-value wave reductions (tests/hip/reduce_hooks.hip: mjpc_hip_debug_wave_sum_time).

One wave per CU repeats a reduction in a dependent chain, as the owner wave's line search does; prints s_memtime ticks (the
unit of tools/calib_valu.hip: 4.3 per independent fp64 instruction) per repetition for the butterfly reference, the transposed form of csrc/spmd.h and the hybrid (butterflies inside the rows, shared
register for the two swap levels), each less the empty loop.  usage: tools/wavesum_time.py [LIB.so] [REPS]"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_wave_sum_bits as t  # noqa: E402

lib = C.CDLL(sys.argv[1] if len(sys.argv) > 1 else t.build_reduce_hooks())
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
MODES = ((5, "empty loop"), (0, "wave_sum3 butterflies (before)"), (1, "wave_sum3 transposed (spmd.h)"), (2, "wave_sum3 hybrid"),
         (3, "wave_sum4 butterflies (before)"), (4, "wave_sum4 transposed (spmd.h)"))
for rnd in range(3):
    base = None
    for mode, name in MODES:
        out = np.zeros(2)
        rc = lib.mjpc_hip_debug_wave_sum_time(mode, reps, out.ctypes.data_as(C.c_void_p), 0)
        assert rc == 0, rc
        if mode == 5:
            base = out[0]
        print(f"round {rnd} {name:34s} {out[0]:8.2f} ticks / rep   {out[0] - base:8.2f} above the empty loop", flush=True)
