"""pangulu_amd_gstrs_multi without a device: the checker's build of the host on the oracle's CPU operators loops the host sweep
over the columns, on one rank and on several.  Column j must be what pangulu_gstrs gives for that column alone."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch.distributed  # noqa: F401  (pages the library in once, here, instead of in every rank under a timeout)

import pangulu_amd as pa
from pangulu_amd import _lib
from pangulu_amd import matrices as M

from .helpers import ROOT, oracle_library
from .solve_multi_common import assert_columns_match, open_handle, oracle_columns, raw_gstrs_multi, rhs_block, solve_columns
from .test_multirank import free_port

GENS = {"fem27_6": (lambda dt: M.fem27(6, dtype=dt), 32), "trefethen": (lambda dt: M.trefethen(dtype=dt), 4)}


@pytest.mark.parametrize("nrhs", [1, 4, 17])
@pytest.mark.parametrize("name", ["fem27_6", "trefethen"])
def test_columns_match_single_vector_solves(name, nrhs):
    gen, nb = GENS[name]
    mat = gen(np.float64)
    Ball = rhs_block(mat, 17)
    ref = oracle_columns(name + "_identity", mat, nb, "r64", Ball, ordering="identity")[:, :nrhs]
    B = Ball[:, :nrhs]
    h = open_handle(mat, nb, oracle_library("r64"), "r64", ordering="identity")
    try:
        X = pa.pangulu_gstrs_multi(h, B)
        path = pa.last_solve_path(h)
        t_multi = h.info()["time_solve"]
        own = solve_columns(h, B)
    finally:
        pa.pangulu_finalize(h)
    assert path == {"device_columns": 0, "panel_width": 1, "panels": nrhs}
    assert t_multi > 0
    assert_columns_match(X, ref, B, "r64", "against the oracle, column by column")
    assert_columns_match(X, own, B, "r64", "against pangulu_gstrs on the same handle")


@pytest.mark.parametrize("vtype", ["r64", "r32", "cr64", "cr32"])
def test_all_value_types(vtype):
    dt = _lib.VALUE_TYPES[vtype][0]
    mat = M.trefethen(dtype=dt)
    B = rhs_block(mat, 5)
    ref = oracle_columns("trefethen_" + vtype, mat, 4, vtype, B, ordering="identity")
    h = open_handle(mat, 4, oracle_library(vtype), vtype, ordering="identity")
    try:
        X = pa.pangulu_gstrs_multi(h, np.ascontiguousarray(B))  # (row-major input: the binding reorders)
    finally:
        pa.pangulu_finalize(h)
    assert X.dtype == dt
    assert_columns_match(X, ref, B, vtype, vtype)


def test_return_codes_and_leading_dimension():
    mat = M.fem27(6)
    B = rhs_block(mat, 4)
    n, nrhs = B.shape
    ref = oracle_columns("fem27_6_identity", mat, 32, "r64", rhs_block(mat, 17), ordering="identity")[:, :nrhs]
    h = open_handle(mat, 32, oracle_library("r64"), "r64", ordering="identity", gstrf=False)
    try:
        buf = np.full((n + 5, nrhs), -777.25, order="F")
        buf[:n] = B
        before = buf.copy(order="F")
        assert raw_gstrs_multi(h, buf, nrhs, n + 5) == 1  # not factorised
        with pytest.raises(RuntimeError):  # (the binding turns a non-zero code into an exception)
            pa.pangulu_gstrs_multi(h, B)
        pa.pangulu_gstrf(h)
        assert raw_gstrs_multi(h, buf, nrhs, n - 1) == 2
        assert raw_gstrs_multi(h, None, nrhs, n + 5) == 2
        assert raw_gstrs_multi(h, buf, 0, n + 5) == 0
        assert raw_gstrs_multi(h, None, 0, 0) == 0  # (nothing to do: nothing is looked at)
        assert (buf == before).all()
        assert raw_gstrs_multi(h, buf, nrhs, n + 5) == 0
    finally:
        pa.pangulu_finalize(h)
    assert (buf[n:] == -777.25).all()  # the slack rows of ldb = n + 5 are not touched
    assert_columns_match(buf[:n], ref, B, "r64", "ldb = n + 5")


@pytest.mark.parametrize("world", [2, 4])
def test_multirank_columns_match_single_vector_solves(world, tmp_path):
    """N > 1 ranks: the distributed host sweep per column, collective, same tags as pangulu_gstrs"""
    out = str(tmp_path / "out.npz")
    port = free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   OMP_NUM_THREADS="1", PANGULU_AMD_SEPARATOR_MAP="cyclic")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "mp_solve_multi_worker.py"), "fem27_6", "32", out, "5"],
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
    assert float(z["zero_column"]) == 0.0
    assert float(z["worst"]) <= 1e-11, float(z["worst"])  # the same sweep in the same run
    assert float(z["residual"]) <= 1e-12, float(z["residual"])
