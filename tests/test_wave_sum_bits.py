"""wave_sum3 / wave_sum4 of csrc/spmd.h reduce several values through ONE shared register (a transposed tree with row rotations
and gfx950's permlane swaps) instead of one butterfly chain per value.  Every add still combines the two partial sums the
butterfly tree combined, only in another lane, so no bit of a result may move.  tests/hip/reduce_hooks.hip holds the reductions
as they were before (the reference) next to kernels that call the product's; this test builds it into a library of its own, runs
one launch of 64 workgroups x 64 lanes over a few thousand input sets and compares everything as uint64.  A NaN result only has to
be a NaN: NaN + NaN keeps one operand's payload, which is the one thing that depends on the operand order.

The reference kernel itself is pinned to the same tree written in numpy (IEEE doubles on both sides), so reference and product
cannot agree on a wrong value, nor on the buffer's initial contents."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hip", "reduce_hooks.hip")
SO = os.path.join(ROOT, "tests", "hip", "libmjpc_hip_reducehooks.so")
SPMD = os.path.join(ROOT, "mujoco_mpc_amd", "csrc", "spmd.h")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
PER_KIND = 512


def build_reduce_hooks():
    """the flags of __graft_entry__.build_test_hooks(); rebuilt when the source or spmd.h is newer"""
    if not os.path.exists(SO) or any(os.path.getmtime(s) > os.path.getmtime(SO) for s in (SRC, SPMD)):
        tmp = f"{SO}.{os.getpid()}.tmp"
        subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc", "-shared", "-Wno-unused-result",
                               "-Wno-unused-value", "-o", tmp, SRC], cwd=os.path.dirname(SRC))
        os.replace(tmp, SO)
    return SO


def input_sets():
    """name -> (sets, 4, 64) doubles; PER_KIND sets of each kind"""
    rng = np.random.default_rng(0x5EED5)
    shape = (PER_KIND, 4, 64)
    kinds = {}
    kinds["wide_range"] = rng.standard_normal(shape) * 10.0 ** rng.integers(-12, 13, shape)
    kinds["extreme_range"] = rng.standard_normal(shape) * 10.0 ** rng.integers(-300, 309, shape).astype(np.float64)      # some sums (and inputs) overflow to inf, some to NaN
    # heavy cancellation: 32 values and their negatives in shuffled lanes, plus noise 1e-16 .. 1e-9 of their size on half of the sets
    half = rng.standard_normal((PER_KIND, 4, 32)) * 10.0 ** rng.integers(-3, 9, (PER_KIND, 4, 32))
    canc = rng.permuted(np.concatenate([half, -half], axis=2), axis=2)
    noise = canc * rng.standard_normal(shape) * 10.0 ** rng.integers(-16, -8, shape)
    noise[::2] = 0.0
    kinds["cancellation"] = canc + noise
    # denormals: random mantissas with a zero exponent field, either sign; every fourth set mixed with the smallest normals
    den = (rng.integers(0, 1 << 52, shape, dtype=np.uint64) | (rng.integers(0, 2, shape, dtype=np.uint64) << np.uint64(63))).view(np.float64)
    den[::4] = np.where(rng.random(shape)[::4] < 0.5, den[::4], rng.standard_normal(shape)[::4] * 2.3e-308)
    kinds["denormals"] = den
    # signed zeros: all +0, all -0 (the sum is -0), random signs, and zeros of random sign around one or two finite values
    z = np.where(rng.random(shape) < 0.5, 0.0, -0.0)
    z[0::4] = 0.0
    z[1::4] = -0.0
    sprinkle = rng.random(shape) < 0.02
    z[3::4] = np.where(sprinkle[3::4], rng.standard_normal(shape)[3::4], z[3::4])
    kinds["signed_zeros"] = z
    # infinities: +inf only, -inf only, both (NaN), in a few random lanes of wide-range values; plus NaN inputs
    inf = kinds["wide_range"].copy()
    hit = rng.random(shape) < 0.03
    inf[0::4] = np.where(hit[0::4], np.inf, inf[0::4])
    inf[1::4] = np.where(hit[1::4], -np.inf, inf[1::4])
    inf[2::4] = np.where(hit[2::4], np.where(rng.random(shape)[2::4] < 0.5, np.inf, -np.inf), inf[2::4])
    inf[3::4] = np.where(hit[3::4] & (rng.random(shape)[3::4] < 0.2), np.nan, inf[3::4])
    kinds["infinities"] = inf
    # all lanes equal (one value per set and sum): ordinary, tiny, huge (64 x overflows), denormal
    val = rng.standard_normal((PER_KIND, 4, 1)) * 10.0 ** rng.integers(-12, 13, (PER_KIND, 4, 1))
    val[1::4] *= 1e-300
    val[2::4] = np.sign(val[2::4]) * 1e307 * rng.integers(1, 18, (PER_KIND, 4, 1))[2::4]
    val[3::4] = 5e-324 * rng.integers(1, 1 << 20, (PER_KIND, 4, 1))[3::4]
    kinds["all_equal"] = np.broadcast_to(val, shape).copy()
    return kinds


def tree_sum(x):
    """the butterfly tree of wave_sum over the last axis (64 lanes): xor 1, xor 2, the two quads of an octet, the two octets of a
    row, rows 0 + 1 and 2 + 3, their sum - one IEEE add each"""
    lane = np.arange(64)
    v = x
    with np.errstate(all="ignore"):
        for perm in (lane ^ 1, lane ^ 2, (lane & ~7) | (7 - (lane & 7)), (lane & ~15) | (15 - (lane & 15))):
            v = v + v[..., perm]
        r = v[..., ::16]
        return (r[..., 3] + r[..., 2]) + (r[..., 1] + r[..., 0])


@pytest.fixture(scope="module")
def sums():
    """name -> (inputs, device words (sets, 4 variants, 4 sums)) from ONE launch over all kinds"""
    lib = ctypes.CDLL(build_reduce_hooks())
    lib.mjpc_hip_reducehooks_last_error.restype = ctypes.c_char_p
    kinds = input_sets()
    x = np.ascontiguousarray(np.concatenate(list(kinds.values()), axis=0))
    out = np.zeros((x.shape[0], 4, 4), dtype=np.uint64)
    rc = lib.mjpc_hip_debug_wave_sums(ctypes.c_int(x.shape[0]), x.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p), ctypes.c_int(0))
    assert rc == 0, lib.mjpc_hip_reducehooks_last_error().decode()
    res, at = {}, 0
    for name, v in kinds.items():
        res[name] = (v, out[at:at + v.shape[0]])
        at += v.shape[0]
    return res


def same_bits_or_both_nan(got, want):
    nan = np.isnan(want.view(np.float64))
    return np.where(nan, np.isnan(got.view(np.float64)), got == want)


KINDS = ["wide_range", "extreme_range", "cancellation", "denormals", "signed_zeros", "infinities", "all_equal"]


@pytest.mark.parametrize("kind", KINDS)
def test_wave_sums_equal_the_butterfly_tree_in_every_bit(kind, sums):
    x, out = sums[kind]
    ref3, new3, ref4, new4 = out[:, 0, :3], out[:, 1, :3], out[:, 2, :], out[:, 3, :]
    want = np.ascontiguousarray(tree_sum(x)).view(np.uint64)
    finite = np.isfinite(want.view(np.float64))
    print(f"{kind}: {x.shape[0]} sets, {int(finite.sum())} of {want.size} sums finite, {int(np.isnan(want.view(np.float64)).sum())} NaN")
    for name, got, w in (("reference wave_sum3", ref3, want[:, :3]), ("reference wave_sum4", ref4, want),
                         ("wave_sum3", new3, want[:, :3]), ("wave_sum4", new4, want)):
        ok = same_bits_or_both_nan(got, w)
        print(f"  {name} against the tree in numpy: {int((~ok).sum())} of {ok.size} words differ")
    # the reference kernels are the tree (so they ran, on these inputs) ...
    assert same_bits_or_both_nan(ref3, want[:, :3]).all() and same_bits_or_both_nan(ref4, want).all()
    # ... and the product's reductions give the reference's words
    assert same_bits_or_both_nan(new3, ref3).all()
    assert same_bits_or_both_nan(new4, ref4).all()
    if kind in ("wide_range", "cancellation", "denormals", "signed_zeros"):
        assert finite.all()
    if kind == "signed_zeros":
        assert (new3[1::4] == np.uint64(1) << np.uint64(63)).all() and (new3[0::4] == 0).all()
