"""ldl_load_row of csrc/linalg.h (lane i picks row i of the Hessian up from LDS, the worker waves' partial Hessians added on the
way) forms its offsets once per call, clamps the lane index once and masks the inactive lanes once at the end, instead of one
address select per entry and matrix and one value select per load and per add.  Every load and every add of an active lane is the
one it was, so no bit of a row, of a diagonal entry or of the solution behind them may move.  tests/hip/ldl_load_hooks.hip holds
the row load as it was before (the reference) next to a one-wave kernel that runs reference and product on the same LDS image;
this test builds it into a library of its own, runs one launch per matrix size (one workgroup of one wave per input set) and
compares everything as uint64.

The strict upper triangles of A and of every partial, the spare columns of the LDS rows and the partials beyond `nx` are NaN:
neither form may read them.  The reference's rows are pinned to the same sums written in numpy (IEEE doubles on both sides), so
reference and product cannot agree on a wrong value, nor on the buffer's initial contents."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hip", "ldl_load_hooks.hip")
SO = os.path.join(ROOT, "tests", "hip", "libmjpc_hip_ldlloadhooks.so")
CSRC = os.path.join(ROOT, "mujoco_mpc_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

# the dof trees of csrc/model.h (DofTree<N>::parent): the pattern of the matrices the level-ordered elimination is given
PARENT = {
    18: [-1, 0, 1, 2, 3, 4, 5, 6, 7, 5, 9, 10, 5, 12, 13, 5, 15, 16],
    27: [-1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 8, 15, 16, 17, 18, 19, 5, 21, 22, 5, 24, 25],
    33: [-1, 0, 1, -1, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 10, 15, 16, 17, 10, 19, 20, 21, 10, 23, 24, 25, 26, 10, 28, 29, 30, 31],
}
KINDS = ("plain", "wide_range", "cancellation", "zeros_denormals")
SEEDS = 8            # input sets per (nx, order, kind): 32 per case, 256 per matrix size
ONE = np.float64(1.0).view(np.uint64)


def build_hooks():
    """the flags of __graft_entry__.build_test_hooks(); rebuilt when the source or a kernel header is newer"""
    srcs = [SRC] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    if not os.path.exists(SO) or any(os.path.getmtime(s) > os.path.getmtime(SO) for s in srcs):
        tmp = f"{SO}.{os.getpid()}.tmp"
        subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc", "-shared", "-Wno-unused-result",
                               "-Wno-unused-value", "-o", tmp, SRC], cwd=os.path.dirname(SRC))
        os.replace(tmp, SO)
    return SO


def pattern(n, tree):
    """symmetric boolean mask of the entries a matrix may hold: everything (dense order) or (i, ancestors of i) (level order)"""
    if not tree:
        return np.ones((n, n), dtype=bool)
    m = np.eye(n, dtype=bool)
    for i in range(n):
        a = PARENT[n][i]
        while a >= 0:
            m[i, a] = m[a, i] = True
            a = PARENT[n][a]
    return m


def dominant(rng, mask, amp=1.0):
    """symmetric, strictly diagonally dominant (eigenvalues >= amp), zero outside the mask"""
    n = mask.shape[0]
    off = np.tril(rng.uniform(-1.0, 1.0, (n, n)), -1) * amp
    off = (off + off.T) * mask
    return off + np.diag(amp + np.abs(off).sum(axis=1))


def signed_zeros(rng, m):
    """the zeros of m with random signs, symmetric positions drawn independently (only the lower triangle is read)"""
    return np.where(m == 0.0, np.where(rng.random(m.shape) < 0.5, 0.0, -0.0), m)


def denormals(rng, shape):
    return (rng.integers(1, 1 << 52, shape, dtype=np.uint64) | (rng.integers(0, 2, shape, dtype=np.uint64) << np.uint64(63))).view(np.float64)


def one_set(rng, n, nx, tree, kind):
    """A, X[3], b with A + X[0] + .. + X[nx - 1] symmetric positive definite on the pattern of the order (so that the elimination
    meets no clamped pivot and nothing overflows: every word of every output is finite)"""
    mask = pattern(n, tree)
    if kind == "zeros_denormals":
        keep = np.tril(rng.random((n, n)) < 0.6, -1)
        mask = mask & (keep | keep.T | np.eye(n, dtype=bool))
    s = 10.0 ** rng.uniform(-6.0, 6.0, n) if kind == "wide_range" else np.ones(n)
    scale = s[:, None] * s[None, :]
    H = dominant(rng, mask) * scale
    X = np.full((3, n, n), np.nan)
    A = H.copy()
    for w in range(nx):
        if kind == "cancellation":
            # partials several orders above the sum: A carries their negative, only rounding is left of them
            R = np.tril(rng.standard_normal((n, n))) * 10.0 ** rng.integers(2, 7)
            X[w] = (R + np.tril(R, -1).T) * mask
            A = A - X[w]
        else:
            X[w] = dominant(rng, mask, 0.05) * scale
    if kind == "zeros_denormals":
        A = signed_zeros(rng, A)
        low = np.tril(np.ones((n, n), dtype=bool), -1)
        for w in range(nx):
            X[w] = signed_zeros(rng, X[w])
            hit = low & (rng.random((n, n)) < 0.25)
            X[w] = np.where(hit, denormals(rng, (n, n)), X[w])
        hit = low & (rng.random((n, n)) < 0.1)
        A = np.where(hit, denormals(rng, (n, n)), A)
    up = np.triu(np.ones((n, n), dtype=bool), 1)
    A = np.where(up, np.nan, A)
    X[:nx] = np.where(up, np.nan, X[:nx])
    b = rng.standard_normal(n) * s
    return A, X, b


def input_sets(n):
    rng = np.random.default_rng(0x1D1 + n)
    A, X, b, nxs, trees, kinds = [], [], [], [], [], []
    for nx in range(4):
        for tree in (0, 1):
            for k, kind in enumerate(KINDS):
                for _ in range(SEEDS):
                    a, x, bb = one_set(rng, n, nx, tree, kind)
                    A.append(a); X.append(x); b.append(bb); nxs.append(nx); trees.append(tree); kinds.append(k)
    return (np.ascontiguousarray(A), np.ascontiguousarray(X), np.ascontiguousarray(b), np.array(nxs, dtype=np.int32),
            np.array(trees, dtype=np.int32), np.array(kinds))


def rows_in_numpy(A, X, nx):
    """what lane i < n loads: entry j of its row is (max(i, j), min(i, j)) of ((A + X0) + X1) + X2, one IEEE add per partial"""
    low = A.copy()
    with np.errstate(all="ignore"):
        for w in range(nx):
            low = low + X[w]
    n = A.shape[0]
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    return low[np.maximum(i, j), np.minimum(i, j)]


_runs = {}


def run(n):
    """(inputs, device words (sets, 64 lanes, 2 (n + 1) + 2)) of ONE launch over all cases of matrix size n"""
    if n not in _runs:
        lib = ctypes.CDLL(build_hooks())
        lib.mjpc_hip_ldlloadhooks_last_error.restype = ctypes.c_char_p
        A, X, b, nxs, trees, kinds = input_sets(n)
        out = np.zeros((A.shape[0], 64, 2 * (n + 1) + 2), dtype=np.uint64)
        p = lambda v: v.ctypes.data_as(ctypes.c_void_p)
        rc = lib.mjpc_hip_debug_ldl_load(ctypes.c_int(n), ctypes.c_int(A.shape[0]), p(A), p(X), p(b), p(nxs), p(trees), p(out), ctypes.c_int(0))
        assert rc == 0, lib.mjpc_hip_ldlloadhooks_last_error().decode()
        _runs[n] = (A, X, b, nxs, trees, kinds, out)
    return _runs[n]


@pytest.mark.parametrize("tree", [0, 1], ids=["dense_order", "level_order"])
@pytest.mark.parametrize("nx", [0, 1, 2, 3])
@pytest.mark.parametrize("n", [18, 27, 33])
def test_row_load_keeps_every_bit_of_the_rows_and_of_the_solution(n, nx, tree):
    A, X, b, nxs, trees, kinds, out = run(n)
    sel = np.flatnonzero((nxs == nx) & (trees == tree))
    assert sel.size == SEEDS * len(KINDS)
    words = out[sel]
    ref_a, ref_d, new_a, new_d = words[:, :, :n], words[:, :, n], words[:, :, n + 1:2 * n + 1], words[:, :, 2 * n + 1]
    ref_x, new_x = words[:, :, 2 * n + 2], words[:, :, 2 * n + 3]
    want = np.stack([rows_in_numpy(A[s], X[s], nx) for s in sel])
    assert not np.isnan(want).any()                  # (the sums themselves never touch a NaN of the inputs)
    want_a = np.ascontiguousarray(want).view(np.uint64)
    want_d = np.ascontiguousarray(np.diagonal(want, axis1=1, axis2=2)).view(np.uint64)
    nan = int(np.isnan(words.view(np.float64)).sum())
    print(f"n {n} nx {nx} {'level' if tree else 'dense'} order, {sel.size} sets: "
          f"reference rows against numpy {int((ref_a[:, :n] != want_a).sum())} + {int((ref_d[:, :n] != want_d).sum())} words differ, "
          f"product rows against reference {int((new_a != ref_a).sum())} + {int((new_d != ref_d).sum())}, "
          f"solutions {int((new_x != ref_x).sum())} of {new_x.size}, NaN words {nan}, "
          f"|x| {np.abs(ref_x[:, :n].view(np.float64)).min():.3g} .. {np.abs(ref_x[:, :n].view(np.float64)).max():.3g}")
    # the reference kernel loads the rows we think it loads (so it ran, on these inputs) ...
    assert (ref_a[:, :n] == want_a).all() and (ref_d[:, :n] == want_d).all()
    # ... and the product gives the reference's words: rows, diagonal entries, solution, on all 64 lanes
    assert (new_a == ref_a).all() and (new_d == ref_d).all()
    assert (new_x == ref_x).all()
    assert nan == 0
    # inactive lanes: +0.0 and 1.0 exactly (the row-local broadcasts multiply them by exact zeros)
    assert (new_a[:, n:] == 0).all() and (new_d[:, n:] == ONE).all()
    assert (ref_a[:, n:] == 0).all() and (ref_d[:, n:] == ONE).all()
    # the inputs were what the docstring says: signed zeros and denormals reach the rows of their kind
    zd = kinds[sel] == KINDS.index("zeros_denormals")
    f = want[zd]
    assert ((f != 0) & (np.abs(f) < 2.2e-308)).any() and (np.signbit(f) & (f == 0)).any() and (~np.signbit(f) & (f == 0)).any()
