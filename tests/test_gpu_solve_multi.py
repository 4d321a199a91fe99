"""pangulu_amd_gstrs_multi on the device: panels of right-hand sides through pangulu_platform_0201001_block_trsm_multi
(pg_hip_block_solve_multi.h).  Column j of the block solve must be what pangulu_gstrs gives for that column alone -- the oracle
library's and the HIP path's own -- within the bounds of test_device_solve_matches_host_sweep."""
import numpy as np
import pytest

import pangulu_amd as pa
from pangulu_amd import _lib
from pangulu_amd import matrices as M

from .solve_multi_common import assert_columns_match, open_handle, oracle_columns, raw_gstrs_multi, rhs_block, solve_columns

pytestmark = pytest.mark.gpu

CASES = {
    # name: (vtype, generator, nb, columns of the case's reference)
    "r64_shell40": ("r64", lambda dt: M.shell(40, 40, dtype=dt), 256, 19),  # n = 9 600: padding rows, 38 block rows
    "r64_kkt8": ("r64", lambda dt: M.kkt(8, dtype=dt), 64, 5),
    "cr64_poisson12": ("cr64", lambda dt: M.poisson3d(12, dtype=dt, shift=0.5j), 128, 9),
    "r32_fem27_10": ("r32", lambda dt: M.fem27(10, dtype=dt), 64, 7),
    "cr32_poisson10": ("cr32", lambda dt: M.poisson3d(10, dtype=dt, shift=0.5j), 64, 4),
}
_mats = {}


def case(name):
    """matrix, nb, vtype, the case's right-hand sides and the oracle's column-by-column solutions (made once, read-only)"""
    vtype, gen, nb, ncol = CASES[name]
    if name not in _mats:
        mat = gen(_lib.VALUE_TYPES[vtype][0])
        B = rhs_block(mat, ncol)
        B.setflags(write=False)
        _mats[name] = (mat, B)
    mat, B = _mats[name]
    return mat, nb, vtype, B, oracle_columns(name, mat, nb, vtype, B)


# (nrhs, widest panel, panels): a tile row is at most 128 bytes -- 16 real values, 8 double-complex ones; a panel is as wide as the
# smallest power of two that holds the columns left, at most that
@pytest.mark.parametrize("name,nrhs,width,panels", [
    ("r64_shell40", 1, 1, 1), ("r64_shell40", 3, 4, 1), ("r64_shell40", 16, 16, 1), ("r64_shell40", 19, 16, 2),
    ("r64_kkt8", 5, 8, 1),
    ("cr64_poisson12", 5, 8, 1), ("cr64_poisson12", 9, 8, 2),
    ("r32_fem27_10", 7, 8, 1),
    ("cr32_poisson10", 4, 4, 1),
])
def test_block_solve_matches_single_vector_solves(name, nrhs, width, panels, monkeypatch):
    monkeypatch.setenv("PANGULU_AMD_DEVICE_SOLVE", "1")
    mat, nb, vtype, B, ref = case(name)
    B, ref = B[:, :nrhs], ref[:, :nrhs]
    h = open_handle(mat, nb, "hip", vtype)
    try:
        X = pa.pangulu_gstrs_multi(h, B)
        path = pa.last_solve_path(h)
        own = solve_columns(h, B)
    finally:
        pa.pangulu_finalize(h)
    assert path == {"device_columns": nrhs, "panel_width": width, "panels": panels}, path
    assert_columns_match(X, ref, B, vtype, "against the oracle")
    assert_columns_match(X, own, B, vtype, "against pangulu_gstrs on the HIP path")


def test_leading_dimension_and_memory_order(monkeypatch):
    """ldb = n + 5: the slack rows keep their sentinel; the binding takes B in either memory order"""
    monkeypatch.setenv("PANGULU_AMD_DEVICE_SOLVE", "1")
    mat, nb, vtype, B, ref = case("r64_kkt8")
    n, nrhs = B.shape
    h = open_handle(mat, nb, "hip", vtype)
    try:
        buf = np.full((n + 5, nrhs), -777.25, dtype=B.dtype, order="F")
        buf[:n] = B
        assert raw_gstrs_multi(h, buf, nrhs, n + 5) == 0
        Xc = pa.pangulu_gstrs_multi(h, np.ascontiguousarray(B))
        Xf = pa.pangulu_gstrs_multi(h, np.asfortranarray(B))
    finally:
        pa.pangulu_finalize(h)
    assert (buf[n:] == -777.25).all()
    assert_columns_match(buf[:n], ref, B, vtype, "ldb = n + 5")
    assert_columns_match(Xc, ref, B, vtype, "C-ordered B")
    assert_columns_match(Xf, ref, B, vtype, "Fortran-ordered B")


def test_scaled_handle(monkeypatch):
    """matching + scaling are applied per column: residuals against the oracle's on the same scaled matrix"""
    from .test_scaling import saddle

    monkeypatch.setenv("PANGULU_AMD_DEVICE_SOLVE", "1")
    mat = saddle(6)
    n, cp, ri, va, _ = mat
    B = rhs_block(mat, 3)
    ref = oracle_columns("saddle6_scaled", mat, 32, "r64", B, scaling=True)
    h = open_handle(mat, 32, "hip", "r64", scaling=True)
    try:
        X = pa.pangulu_gstrs_multi(h, B)
        path = pa.last_solve_path(h)
    finally:
        pa.pangulu_finalize(h)
    assert path["device_columns"] == 3
    assert not X[:, 1].any()
    for j in (0, 2):
        res = M.relative_residual(n, cp, ri, va, X[:, j], B[:, j])
        res_ref = M.relative_residual(n, cp, ri, va, ref[:, j], B[:, j])
        assert res <= 1e-10 and abs(res - res_ref) <= 1e-10, (j, res, res_ref)


def test_second_factorisation_on_the_same_handle(monkeypatch):
    """update_values + gstrf keep the cached sweep plan: the second block solve is that of the NEW matrix"""
    monkeypatch.setenv("PANGULU_AMD_DEVICE_SOLVE", "1")
    mat, nb, vtype, B, ref = case("r64_kkt8")
    n, cp, ri, va, coords = mat
    va2 = va * (1.0 + 0.05 * np.cos(np.arange(len(va))))  # same pattern, every entry moved by up to 5 %
    mat2 = (n, cp, ri, va2, coords)
    ref2 = oracle_columns("r64_kkt8_new_values", mat2, nb, vtype, B)
    h = open_handle(mat, nb, "hip", vtype)
    try:
        X1 = pa.pangulu_gstrs_multi(h, B)
        pa.update_values(h, va2)
        pa.pangulu_gstrf(h)
        X2 = pa.pangulu_gstrs_multi(h, B)
        path = pa.last_solve_path(h)
    finally:
        pa.pangulu_finalize(h)
    assert path["device_columns"] == B.shape[1]
    assert_columns_match(X1, ref, B, vtype, "first factorisation")
    assert_columns_match(X2, ref2, B, vtype, "after update_values")
    assert np.abs(X2[:, 0] - X1[:, 0]).max() > 1e-3 * np.abs(X1[:, 0]).max()  # (the two systems do differ)


def test_host_sweep_when_the_device_solve_is_off(monkeypatch):
    monkeypatch.setenv("PANGULU_AMD_DEVICE_SOLVE", "0")
    mat, nb, vtype, B, ref = case("r64_kkt8")
    h = open_handle(mat, nb, "hip", vtype)
    try:
        X = pa.pangulu_gstrs_multi(h, B)
        path = pa.last_solve_path(h)
    finally:
        pa.pangulu_finalize(h)
    assert path["device_columns"] == 0, path
    assert_columns_match(X, ref, B, vtype, "host sweep")


def test_return_codes():
    mat, nb, vtype, B, _ = case("r64_kkt8")
    n, nrhs = B.shape
    h = open_handle(mat, nb, "hip", vtype, gstrf=False)
    try:
        buf = np.asfortranarray(B).copy(order="F")
        assert raw_gstrs_multi(h, buf, nrhs, n) == 1  # not factorised
        assert (buf == B).all()
        pa.pangulu_gstrf(h)
        assert raw_gstrs_multi(h, buf, nrhs, n - 1) == 2
        assert raw_gstrs_multi(h, None, nrhs, n) == 2
        assert raw_gstrs_multi(h, buf, 0, n) == 0
        assert (buf == B).all()
    finally:
        pa.pangulu_finalize(h)
