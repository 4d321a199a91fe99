"""Shared plumbing of tests/test_factor_stats.py and tests/test_gpu_factor_stats.py (pangulu_amd_factor_stats, pangulu_amd_rcond).

References: numpy on the dense double matrix (inv for the exact norm of the inverse, slogdet for the determinant) and the SAME
handle's downloaded factors (pa.factors_as_scipy) for everything that must agree bit for bit.  Bounds, with n the order and TOL the
project's per-column bound of tests/solve_multi_common.py:
  * 0.5 true <= ainv_norm <= true (1 + n TOL): every estimate is the 1-norm of one computed solution column (max|dx|/max|x| <= TOL and
    max|x| <= ||x||_1); the lower bound is a condition on the algorithm -- xLACN2 with SuperLU solves gave est/true in [0.766, 1] on
    these inputs, the first iterate alone (the 1/n row mean) falls far below 0.5;
  * |log|det| - numpy's| <= n TOL (n log terms, each with at most the relative error a factor entry is allowed), sign / phase
    within n TOL;
  * against the handle's own factors: mantissa within 4 n 2^-53 (n - 1 multiplications of at most one rounding each, four for a
    complex product), the exponent equal, minima and maxima equal bit for bit (a maximum does not round).
"""
import ctypes
import math

import numpy as np
import scipy.sparse as sp

import pangulu_amd as pa
from pangulu_amd import _lib
from pangulu_amd import matrices as M

from .solve_trans_common import TOL, conv, open_handle, rand, scaled_saddle  # noqa: F401  (re-exported)


def graded(dtype=np.float64):
    """diag(10^(-8 i / (n - 1))) conv(10): still row diagonally dominant (no pivoting needed), condition number about 4e8, and
    log|det| = -7302 (real) / -7383 (complex): a plain product of the pivots underflows, as conv(10)'s +1908 overflows"""
    n, cp, ri, va, coords = conv(10, dtype)
    d = 10.0 ** (-8.0 * np.arange(n) / (n - 1))
    return M._finish((sp.diags(d) @ M.to_scipy(n, cp, ri, va)).tocsc(), dtype, coords)


def negated():
    """conv(10) with row 7 negated: determinant sign -1"""
    n, cp, ri, va, coords = conv(10)
    d = np.ones(n)
    d[7] = -1.0
    return M._finish((sp.diags(d) @ M.to_scipy(n, cp, ri, va)).tocsc(), np.float64, coords)


def zero_pivot():
    """order 40: diag(2) with [[1, 1], [1, 1]] at rows / columns 20, 21 -- elimination in the identity ordering gives an exact zero
    pivot at column 21"""
    A = sp.lil_matrix(sp.identity(40) * 2.0)
    A[20, 20] = A[20, 21] = A[21, 20] = A[21, 21] = 1.0
    return M._finish(A.tocsc(), np.float64, None)


INPUTS = {
    # name: (vtype, generator, nb, ordering, scaling)
    "r64_conv10": ("r64", lambda: conv(10), 64, "nd", False),
    "r64_conv14": ("r64", lambda: conv(14), 128, "nd", False),
    "cr64_conv12": ("cr64", lambda: conv(12, np.complex128), 128, "nd", False),
    "cr64_conv12_nb32": ("cr64", lambda: conv(12, np.complex128), 32, "nd", False),
    "r64_rand3000": ("r64", lambda: rand(3000, 0.002), 64, "nd", False),
    "cr64_rand1536": ("cr64", lambda: rand(1536, 0.004, np.complex128), 64, "nd", False),
    "r32_rand1536": ("r32", lambda: rand(1536, 0.004, np.float32), 64, "nd", False),
    "cr32_conv10": ("cr32", lambda: conv(10, np.complex64), 64, "nd", False),
    "graded_r64": ("r64", lambda: graded(np.float64), 64, "nd", False),
    "graded_cr64": ("cr64", lambda: graded(np.complex128), 64, "nd", False),
    "negated": ("r64", negated, 64, "nd", False),
    "zero_pivot": ("r64", zero_pivot, 16, "identity", False),
    "scaled_saddle": ("r64", scaled_saddle, 32, "nd", True),
    "r64_conv8": ("r64", lambda: conv(8), 16, "nd", False),
}
_mats, _dense, _inv_norms, _slogdets = {}, {}, {}, {}


def case(name):
    if name not in _mats:
        _mats[name] = INPUTS[name][1]()
    vtype, _, nb, ordering, scaling = INPUTS[name]
    return _mats[name], vtype, nb, ordering, scaling


def open_case(name, platform, gstrf=True):
    mat, vtype, nb, ordering, scaling = case(name)
    return open_handle(mat, nb, platform, vtype, ordering=ordering, scaling=scaling, gstrf=gstrf)


def dense(name):
    """the user's matrix, dense, in double (computed once)"""
    if name not in _dense:
        n, cp, ri, va, _ = case(name)[0]
        A = M.to_scipy(n, cp, ri, va).toarray()
        A = A.astype(np.complex128 if np.iscomplexobj(A) else np.float64)
        A.setflags(write=False)
        _dense[name] = A
    return _dense[name]


def exact_norms(name, norm):
    """(||A||, ||inv(A)||) of the dense double matrix in the 1-norm ("1") or the infinity norm ("I"); the inverse is computed once"""
    if name not in _inv_norms:
        A = dense(name)
        Ai = np.linalg.inv(A)
        _inv_norms[name] = {k: (float(np.linalg.norm(A, o)), float(np.linalg.norm(Ai, o))) for k, o in (("1", 1), ("I", np.inf))}
    return _inv_norms[name][norm]


def reference_slogdet(name):
    if name not in _slogdets:
        _slogdets[name] = np.linalg.slogdet(dense(name))
    return _slogdets[name]


def assert_rcond_within_bounds(name, norm, d, on_device):
    """d = pa.rcond(h, norm, details=True)"""
    vtype = case(name)[1]
    n = dense(name).shape[0]
    anorm, true = exact_norms(name, norm)
    print("%s norm %s: ainv_norm %.6g (true %.6g, ratio %.4f), anorm %.6g, rcond %.3g, %d solves, on_device %d"
          % (name, norm, d["ainv_norm"], true, d["ainv_norm"] / true, d["anorm"], d["rcond"], d["solves"], d["on_device"]))
    assert d["on_device"] == on_device
    assert abs(d["anorm"] - anorm) <= 1e-14 * anorm, (d["anorm"], anorm)
    assert 0.5 * true <= d["ainv_norm"] <= true * (1.0 + n * TOL[vtype]), (d["ainv_norm"], true)
    assert 1 <= d["solves"] <= 12
    assert d["rcond"] == (1.0 / d["ainv_norm"]) / d["anorm"]


def frexp_product(values):
    """prod(values) as (mantissa, exponent), renormalised with math.frexp at every step, in double"""
    cplx = np.iscomplexobj(values)
    re, im, ex = 0.5, 0.0, 1
    for v in values:
        v = complex(v)
        if cplx:
            re, im = re * v.real - im * v.imag, re * v.imag + im * v.real
        else:
            re = re * v.real
        top = max(abs(re), abs(im))
        if top == 0.0:
            return (0j if cplx else 0.0), 0
        _, k = math.frexp(top)
        re, im, ex = math.ldexp(re, -k), math.ldexp(im, -k), ex + k
    return (complex(re, im) if cplx else re), ex


def modulus(values):
    """|v| in double as the C library's hypot gives it (numpy's absolute of a complex array takes vectorised paths of its own on
    some CPUs, a unit in the last place away); real values: exact"""
    v = np.asarray(values)
    return np.hypot(v.real, v.imag) if np.iscomplexobj(v) else np.abs(v)


def factors_reference(h):
    """the quantities of pangulu_amd_factor_stats from the handle's downloaded factors, in double"""
    info = h.info()
    n = int(info["n"])
    perm = pa.permutation(h).astype(np.int64)
    L, U = pa.factors_as_scipy(h)
    wide = np.complex128 if np.iscomplexobj(U.data) else np.float64
    L, U = L.astype(wide), U.astype(wide)
    d = np.asarray(U.diagonal())
    keep = np.flatnonzero(perm < n)  # padding rows are not the user's
    dk = d[keep]
    ak = modulus(dk)
    imin = int(np.argmin(ak))  # the first minimum
    strict_l = L - sp.identity(L.shape[0], dtype=wide, format="csc")
    return {
        "det": frexp_product(dk),
        "min_abs_pivot": float(ak.min()), "max_abs_pivot": float(ak.max()),
        "min_pivot_index": int(perm[keep[imin]]),
        "clamped_pivots": int((np.abs(dk.real) < 1e-16).sum()),
        "max_abs_l": float(modulus(strict_l.data).max()) if strict_l.nnz else 0.0,
        "max_abs_u": float(modulus(U.data).max()),
        "entries": int(sum(len(va) for _, _, _, _, _, va in pa.owned_blocks(h))),
        "nonfinite_entries": int((~np.isfinite(L.data)).sum() + (~np.isfinite(U.data)).sum()),
    }


def assert_stats_match_own_factors(name, h, st, scaled=False):
    """everything that must agree with the handle's own factors: bit for bit, the mantissa within 4 n 2^-53"""
    n = dense(name).shape[0]
    ref = factors_reference(h)
    for k in ("min_abs_pivot", "max_abs_pivot", "max_abs_l", "max_abs_u", "entries", "clamped_pivots", "nonfinite_entries"):
        assert st[k] == ref[k], (k, st[k], ref[k])
    if not scaled:  # (with scaling on the row of the user's matrix is the same, checked there against the scaled factors as well)
        assert st["min_pivot_index"] == ref["min_pivot_index"], (st["min_pivot_index"], ref["min_pivot_index"])
        (m, e), (mr, er) = st["det"], ref["det"]
        assert e == er, (e, er)
        assert abs(m - mr) <= 4.0 * n * 2.0 ** -53 * abs(mr), (m, mr)
    return ref


def assert_determinant_matches_numpy(name, st, sl):
    """st = pa.factor_stats(h), sl = pa.slogdet(h)"""
    vtype = case(name)[1]
    n = dense(name).shape[0]
    sign, logabs = reference_slogdet(name)
    print("%s: log|det| %.6f (numpy %.6f), sign %s (numpy %s), det = %s * 2^%d" % (name, st["log_abs_det"], logabs, sl[0], sign, st["det"][0], st["det"][1]))
    assert abs(st["log_abs_det"] - logabs) <= n * TOL[vtype], (st["log_abs_det"], logabs)
    assert abs(sl[0] - sign) <= n * TOL[vtype], (sl[0], sign)
    assert sl[1] == st["log_abs_det"]
    m, e = st["det"]
    top = max(abs(m.real), abs(m.imag)) if isinstance(m, complex) else abs(m)
    assert 0.5 <= top < 1.0 and math.isfinite(top)
    assert abs(math.log(abs(m)) + e * math.log(2.0) - st["log_abs_det"]) <= 1e-12 * max(1.0, abs(st["log_abs_det"]))
    assert st["pivot_growth"] == st["max_abs_u"] / st["max_abs_a"]


def raw_rcond(h, norm, outputs=True):
    """The C call as it is: (return code, rcond, anorm, ainv_norm, solves, on_device); outputs=False passes NULL everywhere"""
    r, a, i = ctypes.c_double(-7.0), ctypes.c_double(-7.0), ctypes.c_double(-7.0)
    s, d = ctypes.c_int(-7), ctypes.c_int(-7)
    if outputs:
        rc = h.lib.pangulu_amd_rcond(int(norm), ctypes.byref(r), ctypes.byref(a), ctypes.byref(i), ctypes.byref(s), ctypes.byref(d), h.ref)
    else:
        rc = h.lib.pangulu_amd_rcond(int(norm), None, None, None, None, None, h.ref)
    return rc, r.value, a.value, i.value, s.value, d.value


def raw_factor_stats(h, with_output=True):
    st = _lib.FactorStats()
    st.entries = 12345
    rc = h.lib.pangulu_amd_factor_stats(h.ref, ctypes.byref(st) if with_output else None)
    return rc, st
