"""pangulu_amd_gstrs_trans without a device: on the checker's build of the host with the oracle's CPU operators (which have no
transposed operator) every transposed solve is the host sweep over block columns of pg_sptrsv.cpp, on one rank and on several.
Compared with SuperLU's transposed solve (tests/solve_trans_common.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch.distributed  # noqa: F401  (pages the library in once, here, instead of in every rank under a timeout)

import pangulu_amd as pa
from pangulu_amd import _lib

from .helpers import ROOT, oracle_library
from .solve_multi_common import raw_gstrs_multi
from .solve_trans_common import (TOL, TRANS, assert_trans_columns_match, assert_trans_is_honoured, conv, open_handle, rand, raw_gstrs_trans,
                                 relative_difference, rhs_block, scaled_saddle, splu_columns)
from .test_multirank import free_port

# name: (generator by dtype, scaling, does the matrix have an imaginary part in a complex type)
INPUTS = {
    "conv8": (lambda dt: conv(8, dt), False, True),
    "rand600": (lambda dt: rand(600, 0.01, dt), False, True),
    # the saddle is a real matrix: in cr64 its values are cast, so there A^H = A^T and only the right-hand sides are complex
    "saddle6_scaled": (lambda dt: tuple(v.astype(dt) if i == 3 else v for i, v in enumerate(scaled_saddle())), True, False),
}
_mats = {}


def case(name, vtype):
    if (name, vtype) not in _mats:
        mat = INPUTS[name][0](_lib.VALUE_TYPES[vtype][0])
        B = rhs_block(mat, 5)
        B.setflags(write=False)
        _mats[(name, vtype)] = (mat, B)
    return _mats[(name, vtype)]


@pytest.mark.parametrize("vtype,trans", [("r64", "T"), ("cr64", "T"), ("cr64", "H")])
@pytest.mark.parametrize("nb", [16, 64])
@pytest.mark.parametrize("name", list(INPUTS))
def test_host_sweep_matches_splu(name, nb, vtype, trans):
    mat, B5 = case(name, vtype)
    scaling, has_imag = INPUTS[name][1], INPUTS[name][2]
    h = open_handle(mat, nb, oracle_library(vtype), vtype, scaling=scaling)
    try:
        for nrhs in (1, 5):
            B = B5[:, :nrhs]
            ref = splu_columns((name, vtype), mat, B5, trans)[:, :nrhs]
            X = pa.pangulu_gstrs_multi(h, B, trans=trans)
            assert pa.last_solve_path(h) == {"device_columns": 0, "panel_width": 1, "panels": nrhs}
            assert h.info()["time_solve"] > 0
            assert_trans_columns_match(X, ref, B, vtype, "%s nb=%d %s trans=%s nrhs=%d" % (name, nb, vtype, trans, nrhs))
            x0 = pa.pangulu_gstrs(h, np.ascontiguousarray(B[:, 0]), trans=trans)  # the single-vector keyword: the same sweep
            assert (x0 == X[:, 0]).all()
        if has_imag or vtype == "r64":
            assert_trans_is_honoured(h, B5, X, trans)
        else:
            assert relative_difference(X, pa.pangulu_gstrs_multi(h, B5)) > 1e-3
    finally:
        pa.pangulu_finalize(h)


def test_return_codes_and_leading_dimension():
    mat, B = case("conv8", "r64")
    n, nrhs = B.shape
    ref = splu_columns(("conv8", "r64"), mat, B, "T")
    h = open_handle(mat, 16, oracle_library("r64"), "r64", gstrf=False)
    try:
        buf = np.full((n + 5, nrhs), -777.25, order="F")
        buf[:n] = B
        before = buf.copy(order="F")
        assert raw_gstrs_trans(h, buf, nrhs, n + 5, TRANS["T"]) == 1  # not factorised
        with pytest.raises(RuntimeError):  # (the binding turns a non-zero code into an exception)
            pa.pangulu_gstrs_multi(h, B, trans="T")
        pa.pangulu_gstrf(h)
        assert raw_gstrs_trans(h, buf, nrhs, n - 1, TRANS["T"]) == 2
        assert raw_gstrs_trans(h, None, nrhs, n + 5, TRANS["H"]) == 2
        for bad in (3, -1, 77):
            assert raw_gstrs_trans(h, buf, nrhs, n + 5, bad) == 3
        assert raw_gstrs_trans(h, buf, 0, n + 5, TRANS["T"]) == 0
        assert raw_gstrs_trans(h, None, 0, 0, TRANS["T"]) == 0  # (nothing to do: nothing is looked at)
        assert (buf == before).all()
        assert raw_gstrs_trans(h, buf, nrhs, n + 5, TRANS["T"]) == 0
        with pytest.raises(ValueError):
            pa.pangulu_gstrs_multi(h, B, trans="C")
        with pytest.raises(ValueError):
            pa.pangulu_gstrs(h, B[:, 0], trans="t")
    finally:
        pa.pangulu_finalize(h)
    assert (buf[n:] == -777.25).all()  # the slack rows of ldb = n + 5 are not touched
    assert_trans_columns_match(buf[:n], ref, B, "r64", "ldb = n + 5")


def test_trans_none_is_gstrs_multi():
    mat, B = case("rand600", "r64")
    n, nrhs = B.shape
    h = open_handle(mat, 64, oracle_library("r64"), "r64")
    try:
        a = np.asfortranarray(B).copy(order="F")
        b = a.copy(order="F")
        assert raw_gstrs_multi(h, a, nrhs, n) == 0
        assert raw_gstrs_trans(h, b, nrhs, n, TRANS["N"]) == 0
        Xn = pa.pangulu_gstrs_multi(h, B, trans="N")
    finally:
        pa.pangulu_finalize(h)
    assert (a == b).all() and (Xn == a).all()  # bit for bit


def test_second_factorisation_on_the_same_handle():
    """update_values + gstrf: the transposed solve is that of the NEW matrix"""
    mat, B = case("conv8", "r64")
    n, cp, ri, va, coords = mat
    va2 = va * (1.0 + 0.05 * np.cos(np.arange(len(va))))  # same pattern, every entry moved by up to 5 %
    mat2 = (n, cp, ri, va2, coords)
    h = open_handle(mat, 16, oracle_library("r64"), "r64")
    try:
        X1 = pa.pangulu_gstrs_multi(h, B, trans="T")
        pa.update_values(h, va2)
        pa.pangulu_gstrf(h)
        X2 = pa.pangulu_gstrs_multi(h, B, trans="T")
    finally:
        pa.pangulu_finalize(h)
    assert_trans_columns_match(X1, splu_columns(("conv8", "r64"), mat, B, "T"), B, "r64", "first factorisation")
    assert_trans_columns_match(X2, splu_columns(("conv8_new_values", "r64"), mat2, B, "T"), B, "r64", "after update_values")
    assert relative_difference(X2[:, 0], X1[:, 0]) > 1e-3  # (the two systems do differ)


def test_python_keyword_in_both_memory_orders():
    mat, B = case("conv8", "cr64")
    ref = splu_columns(("conv8", "cr64"), mat, B, "H")
    h = open_handle(mat, 64, oracle_library("cr64"), "cr64")
    try:
        Xc = pa.pangulu_gstrs_multi(h, np.ascontiguousarray(B), trans="H")
        Xf = pa.pangulu_gstrs_multi(h, np.asfortranarray(B), trans="H")
    finally:
        pa.pangulu_finalize(h)
    assert Xc.dtype == B.dtype
    assert_trans_columns_match(Xc, ref, B, "cr64", "C-ordered B")
    assert_trans_columns_match(Xf, ref, B, "cr64", "Fortran-ordered B")


@pytest.mark.parametrize("world", [2, 3])
def test_multirank_host_sweep_matches_splu(world, tmp_path):
    """N > 1 ranks: the distributed host sweep over block columns, partial sums under tags of their own"""
    out = str(tmp_path / "out.npz")
    port = free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   OMP_NUM_THREADS="1", PANGULU_AMD_SEPARATOR_MAP="cyclic")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "mp_solve_trans_worker.py"), "conv8", "16", out, "5"],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=int(os.environ.get("PANGULU_TEST_RANK_TIMEOUT", "420")))
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        outs.append(o)
    failed = [r for r, p in enumerate(procs) if p.returncode != 0]
    assert not failed, "ranks %s failed:\n%s" % (failed, "\n".join("--- rank %d ---\n%s" % (r, outs[r][-3000:]) for r in range(world)))
    z = np.load(out)
    assert int(z["device_columns"]) == 0
    for vtype, trans in (("r64", "T"), ("cr64", "T"), ("cr64", "H")):
        mat, B = case("conv8", vtype)
        assert_trans_columns_match(z["X_%s_%s" % (vtype, trans)], splu_columns(("conv8", vtype), mat, B, trans), B, vtype,
                                   "%d ranks %s trans=%s" % (world, vtype, trans))
    assert relative_difference(z["X_cr64_H"], z["X_cr64_T"]) > 1e-3
    assert relative_difference(z["X_r64_T"], z["X_r64_N"]) > 1e-3
