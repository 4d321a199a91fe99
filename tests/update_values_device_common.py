"""Shared plumbing of tests/test_update_values_device.py and tests/test_gpu_update_values_device.py (pangulu_amd_update_values_device).

Reference for every comparison: a twin handle on the same matrix that gets the same values through pa.update_values from numpy (the
host path).  Before pangulu_gstrf every value of every record must be equal bit for bit: both paths only copy values, so no tolerance
applies.  Then the checks of tests/test_update_values.py::run_case: factors within 1e-12 of a fresh handle's (1e-5 in single
precision, tests/test_gpu_parity.py), factor check and residual <= 1e-12 (single precision: 2e-5, the residual bound of
tests/test_gpu_parity.py::test_other_value_types)."""
import ctypes

import numpy as np

import pangulu_amd as pa
from pangulu_amd import _lib
from pangulu_amd import matrices as M

from . import factor_stats_common as C
from .helpers import max_rel_diff
from .solve_multi_common import open_handle
from .test_update_values import perturbed

FACTOR_TOL = {"r64": 1e-12, "cr64": 1e-12, "r32": 1e-5, "cr32": 1e-5}
CHECK_TOL = {"r64": 1e-12, "cr64": 1e-12, "r32": 2e-5, "cr32": 2e-5}

_cases = {}


def case(name):
    """(mat, vtype, nb) by name: the inputs of tests/factor_stats_common.py and a few matrices of pangulu_amd.matrices (built once)"""
    if name not in _cases:
        plain = {"fem27_10_nb32": (lambda: M.fem27(10), 32), "fem27_12_nb64": (lambda: M.fem27(12), 64),
                 "shell_40_nb256": (lambda: M.shell(40, 40), 256), "poisson_12_nb32": (lambda: M.poisson3d(12), 32)}
        if name in plain:
            _cases[name] = (plain[name][0](), "r64", plain[name][1])
        else:
            mat, vtype, nb, ordering, scaling = C.case(name)
            assert ordering == "nd" and not scaling
            _cases[name] = (mat, vtype, nb)
    return _cases[name]


_new_values = {}


def new_values(name, seed=1):
    """the matrix of case(name) with tests/test_update_values.perturbed's values, in the handle's value type (computed once)"""
    if (name, seed) not in _new_values:
        mat, vtype, _ = case(name)
        m2 = perturbed(mat, seed)
        va = np.ascontiguousarray(m2[3], dtype=_lib.VALUE_TYPES[vtype][0])
        va.setflags(write=False)
        _new_values[(name, seed)] = (m2[0], m2[1], m2[2], va, m2[4])
    return _new_values[(name, seed)]


def records(h):
    """[(brow, bcol, is_upper, values)] of every record the handle owns"""
    return [(br, bc, up, va) for br, bc, up, _, _, va in pa.owned_blocks(h)]


def assert_records_bit_equal(got, want):
    assert len(got) == len(want) and len(got) > 0
    for (br, bc, up, va), (br2, bc2, up2, va2) in zip(got, want):
        assert (br, bc, up) == (br2, bc2, up2)
        assert va.dtype == va2.dtype and va.shape == va2.shape
        assert va.tobytes() == va2.tobytes(), "record (%d, %d, upper=%d) differs from the twin's" % (br, bc, up)


def raw_update_device(h, address, stream=None):
    """The C call as it is, with the address of the values as an integer (None: NULL)"""
    return h.lib.pangulu_amd_update_values_device(h.ref, ctypes.c_void_p(address), ctypes.c_void_p(stream))


def twin_records(name, platform, values):
    """the records of a handle on case(name) that was given `values` through the host path (which refills every record whatever it
    held)"""
    mat, vtype, nb = case(name)
    t = open_handle(mat, nb, platform, vtype, gstrf=False)
    try:
        pa.update_values(t, values)
        return records(t)
    finally:
        pa.pangulu_finalize(t)


def assert_norms_describe(h, m2):
    """pangulu_amd_rcond's anorm and pangulu_amd_factor_stats' max_abs_a are those of the matrix m2 (h factorised): the 1-norm within
    1e-14 of numpy's in double (the bound of tests/factor_stats_common.py), the largest modulus exactly"""
    n, cp, ri, va, _ = m2
    wide = va.astype(np.complex128 if np.iscomplexobj(va) else np.float64)
    anorm = float(abs(M.to_scipy(n, cp, ri, wide)).sum(axis=0).max())
    got = pa.rcond(h, details=True)["anorm"]
    assert abs(got - anorm) <= 1e-14 * anorm, (got, anorm)
    assert pa.factor_stats(h)["max_abs_a"] == float(C.modulus(wide).max())


def factor_solve_and_compare(h, name, m2, platform):
    """pangulu_gstrf on h (which holds m2's values) and the checks of tests/test_update_values.py::run_case against a fresh handle
    on m2; returns h.info() after the factorisation"""
    mat, vtype, nb = case(name)
    n, cp, ri, va, _ = m2
    pa.pangulu_gstrf(h)
    info = h.info()
    check = pa.factor_check(h)
    L, U = pa.factors_as_scipy(h)
    b = M.rhs_of_ones(n, cp, ri, va)
    res = M.relative_residual(n, cp, ri, va, pa.pangulu_gstrs(h, b), b)
    f = open_handle(m2, nb, platform, vtype)
    try:
        L2, U2 = pa.factors_as_scipy(f)
    finally:
        pa.pangulu_finalize(f)
    print("%s: factor check %.3g, residual %.3g, L %.3g, U %.3g from a fresh handle's" % (name, check, res, max_rel_diff(L, L2), max_rel_diff(U, U2)))
    assert max_rel_diff(L, L2) <= FACTOR_TOL[vtype] and max_rel_diff(U, U2) <= FACTOR_TOL[vtype]
    assert check <= CHECK_TOL[vtype] and res <= CHECK_TOL[vtype]
    return info
