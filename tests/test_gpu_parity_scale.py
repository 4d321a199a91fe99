"""GPU parity at the scales and workload classes where the bench-path kernels engage (VERDICT r1 "Next #1").

* KKT class (BASELINE config 4, nlpkkt120): indefinite 2x2 block system, small pivots, tile inverses in the dense solves.
* mid-size at nb = 256 with the DEFAULT thresholds: hundreds of blocks, look-ahead GETRF, work lists, K-split launches,
  records stream, dense TSTRF/GESSM, GETRF batches above 128 blocks -- all compared with the oracle at 1e-12.
* CR64 / R32 at nb = 128.
Tolerance: factors within 1e-12 (R64/CR64) / 1e-5 (R32) of the oracle relative to the largest factor entry; the reference's
factor check ||L(U 1) - A 1|| / ||A 1|| (src/pangulu_numeric.c:1082-1341) and ||Ax-b||/||b|| within 1e-10 of the oracle's.
"""
import numpy as np
import os

import pytest

from pangulu_amd import _lib
from pangulu_amd import matrices as M

from .helpers import factorize, lu_check, max_rel_diff, oracle_library

pytestmark = pytest.mark.gpu


def _check(mat, nb, gpu, ref, tol=1e-12, res_tol=1e-12):
    assert gpu["info"]["flop"] == ref["info"]["flop"]
    assert gpu["info"]["symbolic_nnz"] == ref["info"]["symbolic_nnz"]
    assert (gpu["perm"] == ref["perm"]).all()
    for f in ("L", "U"):
        assert gpu[f].nnz == ref[f].nnz
        assert max_rel_diff(gpu[f], ref[f]) <= tol, f
    assert abs(gpu["residual"] - ref["residual"]) <= 1e-10
    assert gpu["residual"] <= res_tol
    assert lu_check(mat, gpu) <= res_tol
    counted = sum(v["flops"] for v in gpu["hip_stats"].values())
    assert counted == gpu["info"]["flop"], (counted, gpu["info"]["flop"])


@pytest.mark.parametrize("permille", [10, 0])
@pytest.mark.parametrize("nx,nb", [(6, 16), (7, 64), (8, 128), (10, 256)])
def test_kkt_class(nx, nb, permille):
    mat = M.kkt(nx)
    gpu = factorize(mat, nb, "hip", hip_options={_lib.HIP_OPT_DENSE_THRESHOLD_PERMILLE: permille,
                                                 _lib.HIP_OPT_TRSM_DENSE_PERMILLE: permille})
    ref = factorize(mat, nb, oracle_library("r64"))
    _check(mat, nb, gpu, ref)
    if permille == 0 and nb in (128, 256):
        st = gpu["hip_stats"]
        assert st["ssssm_dense_mfma"]["tasks"] > 0 and st["tstrf"]["dense_path_tasks"] > 0, st


MID = [
    ("shell_60x60", lambda: M.shell(60, 60)),
    ("fem27_20", lambda: M.fem27(20)),
    ("shell_120x120", lambda: M.shell(120, 120)),
    ("fem27_32", lambda: M.fem27(32)),
    ("poisson_40", lambda: M.poisson3d(40)),
    ("kkt_16", lambda: M.kkt(16)),
    ("elastic3d_14", lambda: M.elastic3d(14)),   # the default bench class (round 4): 3 unknowns per node, 45 entries per row
]


@pytest.mark.parametrize("name,gen", MID, ids=[m[0] for m in MID])
def test_midsize_nb256_default_thresholds(name, gen):
    mat = gen()
    gpu = factorize(mat, 256, "hip")
    ref = factorize(mat, 256, oracle_library("r64"))
    _check(mat, 256, gpu, ref, res_tol=2e-12)
    st = gpu["hip_stats"]
    assert st["ssssm_dense_mfma"]["launches"] > 0 and st["tstrf"]["dense_path_tasks"] > 0 and st["getrf"]["launches"] > 0, st


@pytest.mark.parametrize("name,gen", [("fem27_24", lambda: M.fem27(24)), ("shell_90x90", lambda: M.shell(90, 90)), ("poisson_32", lambda: M.poisson3d(32))],
                         ids=["fem27_24", "shell_90x90", "poisson_32"])
def test_midsize_nb256_without_coordinates(name, gen):
    """The graph-only ordering (multilevel nested dissection, separators in k-d order on pseudo-coordinates) on the device: what a
    matrix file without coordinates gets.  Same checks as with coordinates."""
    n, cp, ri, va, _ = gen()
    mat = (n, cp, ri, va, None)
    gpu = factorize(mat, 256, "hip")
    ref = factorize(mat, 256, oracle_library("r64"))
    _check(mat, 256, gpu, ref, res_tol=2e-12)
    assert gpu["hip_stats"]["ssssm_dense_mfma"]["launches"] > 0


def test_largest_factor_comparison_nb256():
    """The largest HIP-vs-oracle comparison of the suite: elastic3d(20) (24 000 unknowns of the default bench class, F = 2.0e10:
    about a minute of the oracle's triple loops), every entry of L and U at 1e-12."""
    mat = M.elastic3d(20)
    gpu = factorize(mat, 256, "hip")
    ref = factorize(mat, 256, oracle_library("r64"))
    _check(mat, 256, gpu, ref, res_tol=2e-12)
    assert gpu["hip_stats"]["ssssm_dense_mfma"]["launches"] > 0


@pytest.mark.skipif(not os.environ.get("PG_LARGE_PARITY"), reason="opt-in (PG_LARGE_PARITY=1): minutes of the oracle on one core")
def test_factor_comparison_at_eight_times_the_suite_size():
    """Opt-in, run by the builder once per round (profiles/r06q_*): elastic3d(40) -- 192 000 unknowns of the default bench class, eight
    times the unknowns of the largest comparison of the suite, deep enough for launches of thousands of work items on both MFMA update
    kernels -- every entry of L and U of the HIP path against the oracle (its SSSSM on OpenBLAS dgemm like the reference,
    ...0100000.c:317-327) at 1e-12 of the largest entry."""
    import bench

    blas = bench.find_openblas()
    if blas:
        os.environ["PANGULU_ORACLE_BLAS"] = blas
        os.environ.setdefault("OPENBLAS_NUM_THREADS", "1")
    size = int(os.environ.get("PG_LARGE_PARITY_SIZE", "40"))
    # PG_LARGE_PARITY_CLASS: elastic3d (default, R64, nb = 256) | kkt (the quasi-definite class of BASELINE configs[3], R64, nb = 256) |
    # cpoisson (complex-shifted Poisson of configs[4], CR64, nb = 128: the oracle's complex products are its own loops) |
    # shell (the ldoor class of configs[1]; size 398 is the FULL size of the bench's secondary line, n = 950 424)
    cls = os.environ.get("PG_LARGE_PARITY_CLASS", "elastic3d")
    vtype, nb = ("cr64", 128) if cls == "cpoisson" else ("r64", 256)
    if cls == "kkt":
        mat = M.kkt(size)
    elif cls == "cpoisson":
        mat = M.poisson3d(size, dtype=np.complex128, shift=0.5j)
    elif cls == "shell":
        mat = M.shell(size, size)
    else:
        mat = M.elastic3d(size)
    gpu = factorize(mat, nb, "hip", vtype=vtype)
    ref = factorize(mat, nb, oracle_library(vtype), vtype=vtype, solve=False)
    dl, du = max_rel_diff(gpu["L"], ref["L"]), max_rel_diff(gpu["U"], ref["U"])
    print("%s:" % cls, end=" ")
    print("size %d: n = %d, flop = %.3e, max rel |dL| = %.2e, |dU| = %.2e, residual %.2e, factor check %.2e, front / general workgroups %d / %d" % (
        size, mat[0], gpu["info"]["flop"], dl, du, gpu["residual"], gpu["factor_check"],
        gpu["hip_stats"]["ssssm_dense_mfma"]["front_workgroups"], gpu["hip_stats"]["ssssm_dense_mfma"]["general_workgroups"]))
    assert dl <= 1e-12 and du <= 1e-12 and gpu["residual"] <= 1e-11 and gpu["info"]["flop"] == ref["info"]["flop"]


def test_large_getrf_batches_nb256():
    """shell(180,180): 792 diagonal blocks, leaf levels with more than 128 GETRFs per batch (panel-tile look-ahead)."""
    mat = M.shell(180, 180)
    gpu = factorize(mat, 256, "hip")
    ref = factorize(mat, 256, oracle_library("r64"))
    _check(mat, 256, gpu, ref, res_tol=2e-12)


@pytest.mark.parametrize("vtype,gen,nb", [
    ("cr64", lambda dt: M.poisson3d(14, dtype=dt, shift=0.5j), 128),
    ("cr64", lambda dt: M.fem27(12, dtype=dt), 128),
    ("r32", lambda dt: M.fem27(12, dtype=dt), 128),
    ("cr32", lambda dt: M.poisson3d(12, dtype=dt, shift=0.5j), 128),
    ("cr64", lambda dt: M.shell(40, 40, dtype=dt), 256),
], ids=["cr64_poisson14", "cr64_fem27_12", "r32_fem27_12", "cr32_poisson12", "cr64_shell40_nb256"])
def test_other_value_types_nb128(vtype, gen, nb):
    dt = _lib.VALUE_TYPES[vtype][0]
    mat = gen(dt)
    gpu = factorize(mat, nb, "hip", vtype=vtype)
    ref = factorize(mat, nb, oracle_library(vtype), vtype=vtype)
    tol = 1e-12 if vtype == "cr64" else 1e-5
    for f in ("L", "U"):
        assert max_rel_diff(gpu[f], ref[f]) <= tol, f
    assert gpu["info"]["flop"] == ref["info"]["flop"]
    # residual within the type's rounding of the oracle's
    assert gpu["residual"] <= (1e-12 if vtype == "cr64" else 5e-5)
    assert abs(gpu["residual"] - ref["residual"]) <= (1e-10 if vtype == "cr64" else 5e-5)
    assert lu_check(mat, gpu) <= (1e-12 if vtype == "cr64" else 5e-5)


@pytest.mark.parametrize("vtype,gen,nb", [
    ("r64", lambda dt: M.shell(40, 40, dtype=dt), 256),
    ("r64", lambda dt: M.kkt(8, dtype=dt), 64),
    ("cr64", lambda dt: M.poisson3d(12, dtype=dt, shift=0.5j), 128),
    ("r32", lambda dt: M.fem27(10, dtype=dt), 64),
], ids=["r64_shell40", "r64_kkt8", "cr64_poisson12", "r32_fem27_10"])
def test_device_solve_matches_host_sweep(vtype, gen, nb, monkeypatch):
    """pangulu_gstrs on one rank runs both sweeps on the device-resident factors, level by level
    (pangulu_platform_0201001_block_trsm_multi, one panel of width 1); the reference-style host sweep (src/pangulu_sptrsv.c:24-191) on downloaded
    factors must give the same solution to rounding, and both the oracle's."""
    dt = _lib.VALUE_TYPES[vtype][0]
    mat = gen(dt)
    monkeypatch.setenv("PANGULU_AMD_DEVICE_SOLVE", "1")
    dev = factorize(mat, nb, "hip", vtype=vtype, keep_factors=False)
    monkeypatch.setenv("PANGULU_AMD_DEVICE_SOLVE", "0")
    host = factorize(mat, nb, "hip", vtype=vtype, keep_factors=False)
    ref = factorize(mat, nb, oracle_library(vtype), vtype=vtype, keep_factors=False)
    tol = 1e-11 if vtype in ("r64", "cr64") else 2e-4
    scale = np.abs(ref["x"]).max()
    assert np.abs(dev["x"] - host["x"]).max() <= tol * scale
    assert np.abs(dev["x"] - ref["x"]).max() <= tol * scale
    assert dev["residual"] <= (1e-12 if vtype in ("r64", "cr64") else 5e-5)


@pytest.mark.parametrize("nx,nb", [(6, 32), (8, 128), (10, 256), (24, 256), (32, 256)])
def test_saddle_point_with_matching_on_the_hip_path(nx, nb):
    """nlpkkt class without regularisation: [[H, J^T], [J, 0]].  With the maximum-product matching + scaling (MC64's job) in
    front, the factorisation without pivoting goes through on the device and matches the oracle on the same scaled matrix.
    nx = 24 / 32 (n = 27 648 / 65 536, F = 6.5e9 / 3.9e10): sizes at which the dense paths carry the factorisation (VERDICT r4
    next #5; the oracle needs 6 / 25 s for them, nx = 48 would take it minutes)."""
    from .test_scaling import saddle

    mat = saddle(nx)
    gpu = factorize(mat, nb, "hip", scaling=True)
    ref = factorize(mat, nb, oracle_library("r64"), scaling=True)
    assert (gpu["perm"] == ref["perm"]).all()
    for f in ("L", "U"):
        assert max_rel_diff(gpu[f], ref[f]) <= 1e-11, f
    assert gpu["residual"] <= 1e-10 and abs(gpu["residual"] - ref["residual"]) <= 1e-10


@pytest.mark.parametrize("permille", [10, 0, 1001])
@pytest.mark.parametrize("name,gen,nb", [
    ("poisson14c_nb128", lambda: M.poisson3d(14, dtype=np.complex128, shift=0.5j), 128),
    ("fem27c_14_nb256", lambda: M.fem27(14, dtype=np.complex128), 256),
    ("randomc_700_nb128", lambda: M.random_pattern(700, 0.02, 4, dtype=np.complex128), 128),
], ids=["poisson14c_nb128", "fem27c_14_nb256", "randomc_700_nb128"])
def test_cr64_updates_on_the_matrix_cores(name, gen, nb, permille):
    """CR64 dense-mode updates: a complex block's mirror is two real planes, a complex update four real MFMA products
    (pg_hip_dense.h; the reference calls cublasZgemm here, ...0201000.cu:778-816).  Every mix of mirrored and sparse
    blocks must give the oracle's factors; threshold 0 puts every update on the matrix cores, 1001 none."""
    mat = gen()
    gpu = factorize(mat, nb, "hip", vtype="cr64", hip_options={_lib.HIP_OPT_DENSE_THRESHOLD_PERMILLE: permille})
    ref = factorize(mat, nb, oracle_library("cr64"), vtype="cr64")
    st = gpu["hip_stats"]
    if permille == 0:
        assert st["ssssm_dense_mfma"]["tasks"] > 0 and st["ssssm_sparse"]["tasks"] == 0, st
    if permille == 1001:
        assert st["ssssm_dense_mfma"]["tasks"] == 0
    if permille == 10 and nb == 256:
        assert st["ssssm_dense_mfma"]["tasks"] > 0, st
    for f in ("L", "U"):
        assert max_rel_diff(gpu[f], ref[f]) <= 1e-12, (name, f, permille)
    assert gpu["residual"] <= 1e-12 and lu_check(mat, gpu) <= 1e-12
    counted = sum(v["flops"] for v in st.values())
    assert counted == gpu["info"]["flop"], (counted, gpu["info"]["flop"])


@pytest.mark.parametrize("vtype", ["r64", "r32", "cr64", "cr32"])
def test_dense_paths_of_every_value_type_at_nb256(vtype):
    """Round 3: the mirrors and LU images of R32 / CR32 blocks are double (densify widens, sparsify rounds) and every dense kernel
    is the f64 one -- the reference densifies + cuBLAS/cuSOLVER for every type (...0201000.cu:547-641, 778-816).  At nb = 256 on
    a 3D problem all four types must put their updates on the matrix cores and their panels on the dense kernels (real types:
    tiled GETRF + MFMA solves; complex types: GETRF and solves on the two-plane mirrors), and give the oracle's factors within the
    type's tolerance."""
    dt = {"r64": np.float64, "r32": np.float32, "cr64": np.complex128, "cr32": np.complex64}[vtype]
    cplx = np.issubdtype(dt, np.complexfloating)
    mat = M.fem27(20, dtype=dt) if not cplx else M.poisson3d(20, dtype=dt, shift=0.5j)
    gpu = factorize(mat, 256, "hip", vtype=vtype)
    ref = factorize(mat, 256, oracle_library(vtype), vtype=vtype)
    st = gpu["hip_stats"]
    assert st["ssssm_dense_mfma"]["tasks"] > 0, st
    assert st["tstrf"]["dense_path_tasks"] > 0, st  # (complex types: solves on the two-plane mirrors, pg_hip_panels_complex.h)
    single = vtype in ("r32", "cr32")
    tol = 1e-5 if single else 1e-12
    for f in ("L", "U"):
        assert max_rel_diff(gpu[f], ref[f]) <= tol, (vtype, f)
    assert gpu["residual"] <= (5e-5 if single else 1e-12)
    assert lu_check(mat, gpu) <= (5e-5 if single else 1e-12)
    counted = sum(v["flops"] for v in st.values() if isinstance(v, dict))
    assert counted == gpu["info"]["flop"], (counted, gpu["info"]["flop"])


@pytest.mark.parametrize("nb", [384, 512, 96, 48])
def test_block_orders_beyond_the_tuned_ones(nb):
    """nb = 384 / 512: above the 256 the occupancy maps, the tiled GETRF and the dense solves are built for (the MFMA update
    kernel then treats every 16 x 16 piece as live, GETRF and the solves fall back to the pattern-driven kernels); nb = 96 / 48:
    not a multiple of 128, no dense mode at all.  The reference accepts any nb (16-bit in-block indices)."""
    mat = M.fem27(12)
    gpu = factorize(mat, nb, "hip")
    ref = factorize(mat, nb, oracle_library("r64"))
    _check(mat, nb, gpu, ref, res_tol=2e-12)
