"""Shared plumbing of tests/test_solve_trans.py and tests/test_gpu_solve_trans.py (pangulu_amd_gstrs_trans: A^T X = B, A^H X = B on
the factors of A).

Symmetric matrices prove nothing about a transposed solve, and nearly every generator of pangulu_amd/matrices.py is symmetric: the
inputs here are not.  The reference is SuperLU through scipy (splu(A).solve(B, trans=...)), which knows nothing of this code; the
bound is TOL of tests/solve_multi_common.py per column, the project's own bound for a device sweep against another solver's answer.
"""
import ctypes

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import pangulu_amd as pa
from pangulu_amd import _lib
from pangulu_amd import matrices as M

from .solve_multi_common import TOL, open_handle, rhs_block  # noqa: F401  (re-exported)

TRANS = {"N": 0, "T": 1, "H": 2}


def conv(nx, dtype=np.float64):
    """Convection-diffusion: poisson3d(nx, shift = 0.5 / 0.5j) + 0.8 (I - S), S the one-step shift along x (entry (v, v - ny nz) for
    x > 0).  Strictly diagonally dominant, symmetric pattern, unsymmetric values, with coordinates for the dissection."""
    cplx = np.issubdtype(dtype, np.complexfloating)
    n, cp, ri, va, coords = M.poisson3d(nx, dtype=dtype, shift=0.5j if cplx else 0.5)
    A = M.to_scipy(n, cp, ri, va)
    v = np.arange(nx * nx, n)  # the vertices with x > 0 (vertex id = (x ny + y) nz + z)
    S = sp.csc_matrix((np.ones(len(v)), (v, v - nx * nx)), shape=(n, n))
    A = A + 0.8 * (sp.identity(n, format="csc") - S)
    return M._finish(A, dtype, coords)


def rand(n, density, dtype=np.float64):
    """Unsymmetric pattern as well (n no multiple of nb: padding rows)."""
    return M.random_pattern(n, density, 7, dtype, symmetric_pattern=False)


def scaled_saddle():
    """tests/test_scaling.saddle(6) with row i multiplied by 1 + 0.5 cos(i), so that A^T != A; solved with scaling on"""
    from .test_scaling import saddle

    n, cp, ri, va, _ = saddle(6)
    A = sp.diags(1.0 + 0.5 * np.cos(np.arange(n))) @ M.to_scipy(n, cp, ri, va)
    return M._finish(A.tocsc(), np.float64, None)


_splu_cache = {}


def splu_columns(key, mat, B, trans):
    """splu(A).solve(B, trans): SuperLU's answer, computed once per (key, trans) and handed out read-only"""
    k = (key, trans, B.shape[1])
    if k not in _splu_cache:
        n, cp, ri, va, _ = mat
        lu = _splu_cache.get((key, "lu"))
        if lu is None:
            lu = _splu_cache[(key, "lu")] = spla.splu(M.to_scipy(n, cp, ri, va).tocsc())
        X = lu.solve(np.asfortranarray(B), trans=trans)
        X.setflags(write=False)
        _splu_cache[k] = X
    return _splu_cache[k]


def column_errors(X, ref):
    """max |dx| / max |x| per column"""
    return [float(np.abs(X[:, j] - ref[:, j]).max() / np.abs(ref[:, j]).max()) if ref[:, j].any() else float(np.abs(X[:, j]).max())
            for j in range(ref.shape[1])]


def assert_trans_columns_match(X, ref, B, vtype, what):
    assert X.shape == ref.shape == B.shape
    errs = column_errors(X, ref)
    print("%s: max |dx| / max |x| per column: %s (bound %g)" % (what, " ".join("%.2e" % e for e in errs), TOL[vtype]))
    for j in range(B.shape[1]):
        if not B[:, j].any():
            assert not X[:, j].any(), "%s: the all-zero column %d came back non-zero (max %g)" % (what, j, np.abs(X[:, j]).max())
            continue
        assert errs[j] <= TOL[vtype], "%s: column %d differs by %g of its scale" % (what, j, errs[j])


def relative_difference(X, Y):
    return float(np.abs(X - Y).max() / np.abs(Y).max())


def assert_trans_is_honoured(h, B, X, trans):
    """A path that ignored `trans` would pass a comparison on a symmetric input: the T result differs from the N result of the same
    handle, and for complex types the H result from the T result, by more than 1e-3 relative."""
    XN = pa.pangulu_gstrs_multi(h, B)
    XT = X if trans == "T" else pa.pangulu_gstrs_multi(h, B, trans="T")
    d = relative_difference(XT, XN)
    print("T against N on the same handle: %.3g" % d)
    assert d > 1e-3, d
    if np.issubdtype(B.dtype, np.complexfloating):
        XH = X if trans == "H" else pa.pangulu_gstrs_multi(h, B, trans="H")
        d = relative_difference(XH, XT)
        print("H against T on the same handle: %.3g" % d)
        assert d > 1e-3, d


def raw_gstrs_trans(h, buf, nrhs, ldb, trans):
    """The C call as it is, return code included; `buf` a Fortran-ordered array (or None)."""
    opt = _lib.GstrsOptions()
    ptr = buf.ctypes.data_as(ctypes.c_void_p) if buf is not None else None
    return h.lib.pangulu_amd_gstrs_trans(ptr, int(nrhs), int(ldb), int(trans), ctypes.byref(opt), h.ref)


def transposed_residual(mat, x, b, trans="T"):
    """||op(A) x - b|| / ||b||"""
    n, cp, ri, va, _ = mat
    A = M.to_scipy(n, cp, ri, va)
    At = A.T if trans == "T" else A.conj().T
    return float(np.linalg.norm(At @ x - b) / np.linalg.norm(b))
