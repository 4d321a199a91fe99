"""Shared plumbing of tests/test_solve_multi.py and tests/test_gpu_solve_multi.py (pangulu_amd_gstrs_multi).

Every case compares column j of a block solve with single-vector pangulu_gstrs calls on that column alone: the oracle library's
(computed once per case and kept) and the tested path's own.
"""
import ctypes

import numpy as np

import pangulu_amd as pa
from pangulu_amd import _lib
from pangulu_amd import matrices as M

from .helpers import library_for, oracle_library

# max |dx| <= TOL * max |x| per column: the project's own bounds for the device sweep against the host sweep and the oracle
# (tests/test_gpu_parity_scale.py::test_device_solve_matches_host_sweep); they absorb the reordering of sums by atomics
TOL = {"r64": 1e-11, "cr64": 1e-11, "r32": 2e-4, "cr32": 2e-4}


def rhs_block(mat, nrhs, seed=20261018):
    """Right-hand sides that show cross-talk between columns: column 0 = A 1, column 1 all zero (must come back exactly zero),
    column 2 a unit vector, the rest seeded random.  The first k columns are the same for every nrhs >= k."""
    n, cp, ri, va, _ = mat
    dt = va.dtype
    B = np.zeros((n, nrhs), dtype=dt)
    for j in range(3, nrhs):
        rng = np.random.default_rng(seed + j)  # (per column: a narrower block is a prefix of a wider one)
        col = rng.uniform(-1.0, 1.0, size=n)
        if np.issubdtype(dt, np.complexfloating):
            col = col + 1j * rng.uniform(-1.0, 1.0, size=n)
        B[:, j] = col
    B[:, 0] = M.rhs_of_ones(n, cp, ri, va)
    if nrhs > 1:
        B[:, 1] = 0
    if nrhs > 2:
        B[:, 2] = 0
        B[n // 3, 2] = 1
    return B


def open_handle(mat, nb, platform, vtype="r64", ordering="nd", scaling=False, gstrf=True):
    """pangulu_init (+ gstrf) as helpers.factorize does, with the handle left open."""
    n, cp, ri, va, coords = mat
    lib = library_for(platform, vtype)
    if platform == "hip":  # (the options helpers.factorize runs the HIP path with)
        for opt, val in ((_lib.HIP_OPT_GETRF_STRICT_ORDER, 0), (_lib.HIP_OPT_DENSE_THRESHOLD_PERMILLE, 2), (_lib.HIP_OPT_COUNT_FLOPS, 1),
                         (_lib.HIP_OPT_SSSSM_GROUP_CHUNK, 8), (_lib.HIP_OPT_TRSM_DENSE_PERMILLE, 5), (_lib.HIP_OPT_SMALL_LAUNCH_TASKS, 2048),
                         (_lib.HIP_OPT_FRONT_STAGES, 2), (_lib.HIP_OPT_TILES_STAGES, 2), (_lib.HIP_OPT_BACKGROUND_UPDATES, 1)):
            lib.pangulu_platform_0201001_set_option(opt, val)
    h = pa.pangulu_init(n, len(va), cp, ri, va, nb=nb, vtype=vtype, ordering=ordering, coords=coords if ordering == "nd" else None,
                        nthread=4, lib=lib, scaling=scaling)
    if gstrf:
        pa.pangulu_gstrf(h)
    return h


def solve_columns(h, B):
    """pangulu_gstrs on every column alone."""
    return np.stack([pa.pangulu_gstrs(h, np.ascontiguousarray(B[:, j])) for j in range(B.shape[1])], axis=1)


_oracle_cache = {}


def oracle_columns(key, mat, nb, vtype, B, ordering="nd", scaling=False):
    """The oracle library's pangulu_gstrs on each column of B; computed once per `key`, handed out read-only."""
    if key not in _oracle_cache:
        h = open_handle(mat, nb, oracle_library(vtype), vtype, ordering, scaling)
        X = solve_columns(h, B)
        pa.pangulu_finalize(h)
        X.setflags(write=False)
        _oracle_cache[key] = X
    return _oracle_cache[key]


def assert_columns_match(X, ref, B, vtype, what):
    assert X.shape == ref.shape == B.shape
    for j in range(B.shape[1]):
        if not B[:, j].any():
            assert not X[:, j].any(), "%s: the all-zero column %d came back non-zero (max %g)" % (what, j, np.abs(X[:, j]).max())
            continue
        scale = np.abs(ref[:, j]).max()
        err = np.abs(X[:, j] - ref[:, j]).max()
        assert err <= TOL[vtype] * scale, "%s: column %d differs by %g (scale %g)" % (what, j, err, scale)


def raw_gstrs_multi(h, buf, nrhs, ldb):
    """The C call as it is, return code included; `buf` a Fortran-ordered array (or None)."""
    opt = _lib.GstrsOptions()
    ptr = buf.ctypes.data_as(ctypes.c_void_p) if buf is not None else None
    return h.lib.pangulu_amd_gstrs_multi(ptr, int(nrhs), int(ldb), ctypes.byref(opt), h.ref)
