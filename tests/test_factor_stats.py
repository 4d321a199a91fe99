"""pangulu_amd_factor_stats and pangulu_amd_rcond without a device: the checker's build of the host on the oracle's CPU operators (a
host-memory platform without the two optional operators), so the record loops and the host vector of pg_condest.cpp run.  References
and bounds: tests/factor_stats_common.py."""
import math
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import pangulu_amd as pa

from . import factor_stats_common as C
from .helpers import ROOT, oracle_library


def open_cpu(name, gstrf=True):
    return C.open_case(name, oracle_library(C.case(name)[1]), gstrf=gstrf)


@pytest.mark.parametrize("name", ["r64_conv10", "cr64_conv12_nb32", "graded_r64", "graded_cr64", "scaled_saddle"])
def test_rcond_both_norms_on_the_host_path(name):
    h = open_cpu(name)
    try:
        d = {norm: pa.rcond(h, norm, details=True) for norm in ("1", "I")}
        plain = pa.rcond(h)
        assert h.info()["time_solve"] > 0
    finally:
        pa.pangulu_finalize(h)
    assert plain == d["1"]["rcond"]
    for norm in ("1", "I"):
        C.assert_rcond_within_bounds(name, norm, d[norm], on_device=0)
        if name.startswith("graded"):
            anorm, true = C.exact_norms(name, norm)
            assert 0.5 <= d[norm]["rcond"] * true * anorm <= 2.0
            assert d[norm]["rcond"] < 1e-7  # (the condition number is about 4e8)


@pytest.mark.parametrize("name", ["r64_conv10", "graded_r64", "graded_cr64", "negated", "cr64_conv12_nb32", "r64_rand3000", "scaled_saddle"])
def test_factor_stats_and_slogdet(name):
    scaled = C.case(name)[4]
    h = open_cpu(name)
    try:
        st, sl = pa.factor_stats(h), pa.slogdet(h)
        again = pa.factor_stats(h)
        info = h.info()
        ref = C.assert_stats_match_own_factors(name, h, st, scaled=scaled)
    finally:
        pa.pangulu_finalize(h)
    assert again == st  # the same bits from call to call
    C.assert_determinant_matches_numpy(name, st, sl)
    assert st["nonfinite_entries"] == 0 and st["clamped_pivots"] == 0
    if name == "r64_rand3000":
        assert info["block_length"] * info["nb"] > info["n_padded"]  # (the last block has rows without a pivot)
    if name == "cr64_conv12_nb32":
        assert info["n_padded"] > info["n"]  # (padding rows: unit pivots that must not enter the pivot figures)
        assert st["min_abs_pivot"] == ref["min_abs_pivot"] > 1.0 and ref["max_abs_u"] >= 1.0
    if name in ("r64_conv10", "graded_r64", "graded_cr64"):
        assert abs(st["log_abs_det"]) > 1000  # outside double's range as a plain product; mantissa and exponent are finite
        assert math.isfinite(st["det"][1]) and abs(st["det"][1]) > 1074
    if name == "negated":
        assert sl[0] == -1.0
    if name == "scaled_saddle":
        A = C.dense(name)
        assert st["max_abs_a"] <= 1.0 + 1e-12 < np.abs(A).max()  # the growth refers to the scaled matrix


def test_zero_pivot():
    h = open_cpu("zero_pivot")
    try:
        st, sl = pa.factor_stats(h), pa.slogdet(h)
        d = pa.rcond(h, "1", details=True)
        di = pa.rcond(h, "I", details=True)
    finally:
        pa.pangulu_finalize(h)
    assert st["clamped_pivots"] == 1 and st["min_abs_pivot"] == 0.0 and st["min_pivot_index"] == 21
    assert st["log_abs_det"] == -math.inf and st["det"] == (0.0, 0)
    assert sl == (0.0, -math.inf)
    assert st["nonfinite_entries"] == 0 and st["entries"] == 42
    for r in (d, di):
        assert 0.0 <= r["rcond"] <= 1e-15 and r["solves"] <= 12, r


def test_return_codes_and_new_values():
    name = "r64_conv10"
    (n, cp, ri, va, coords) = C.case(name)[0]
    h = open_cpu(name, gstrf=False)
    try:
        assert C.raw_rcond(h, 0)[0] == 1  # not factorised
        rc, st = C.raw_factor_stats(h)
        assert rc == 1 and st.entries == 12345
        pa.pangulu_gstrf(h)
        for bad in (2, -1, 7):
            assert C.raw_rcond(h, bad) == (3, -7.0, -7.0, -7.0, -7, -7)  # outputs untouched
        assert C.raw_rcond(h, 1, outputs=False)[0] == 0  # NULL outputs
        assert C.raw_factor_stats(h, with_output=False)[0] == 0
        d1, st1 = pa.rcond(h, "1", details=True), pa.factor_stats(h)
        pa.update_values(h, 2.0 * va)
        pa.pangulu_gstrf(h)
        d2, st2 = pa.rcond(h, "1", details=True), pa.factor_stats(h)
    finally:
        pa.pangulu_finalize(h)
    C.assert_rcond_within_bounds(name, "1", d1, on_device=0)
    assert d2["anorm"] == 2.0 * d1["anorm"]
    true = C.exact_norms(name, "1")[1] / 2.0
    assert 0.5 * true <= d2["ainv_norm"] <= true * (1.0 + n * C.TOL["r64"])
    assert abs(d2["rcond"] - d1["rcond"]) <= n * C.TOL["r64"] * d1["rcond"]
    assert abs(st2["log_abs_det"] - st1["log_abs_det"] - n * math.log(2.0)) <= n * C.TOL["r64"]
    assert st2["max_abs_u"] == 2.0 * st1["max_abs_u"]


def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.parametrize("world", [2, 3])
def test_multirank_matches_one_rank(world, tmp_path):
    """N > 1 ranks: the records' partials gathered in rank order, rank 0 drives the estimator on the distributed host sweeps"""
    name = "r64_conv8"
    out = str(tmp_path / "out.npz")
    port = free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   OMP_NUM_THREADS="1", PANGULU_AMD_SEPARATOR_MAP="cyclic")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "mp_factor_stats_worker.py"), name, out],
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
    z = np.load(out, allow_pickle=True)
    st, sl = z["stats"].item(), tuple(z["slogdet"])
    h = open_cpu(name)
    try:
        one = pa.factor_stats(h)
    finally:
        pa.pangulu_finalize(h)
    for norm in ("1", "I"):
        C.assert_rcond_within_bounds(name, norm, z["rcond_" + norm].item(), on_device=0)
    C.assert_determinant_matches_numpy(name, st, sl)
    assert st["entries"] == one["entries"]
    for k in ("min_abs_pivot", "max_abs_pivot", "min_pivot_index", "clamped_pivots", "nonfinite_entries", "max_abs_l", "max_abs_u", "max_abs_a"):
        assert st[k] == one[k], (k, st[k], one[k])  # (the ranks ran the same operators on the same blocks)
    assert list(z["return_codes"]) == [0] * (3 * world)
    assert z["other_ranks_agree"].item() is True


@pytest.mark.parametrize("flags", [[], ["-DPANGULU_COMPLEX"], ["-DPG_CONDEST_MAX_GROUPS=4"]], ids=["real", "complex", "real-grid-stride"])
def test_kernels_against_serial_formulas(flags, tmp_path):
    """pg_hip_factor_stats.h compiled as host C++ behind tests/hip_emulation_shims.h (tests/factor_stats_kernel_emulation.cpp); with
    at most 4 workgroups the vector kernels take more than one grid stride at n = 2744"""
    exe = str(tmp_path / "emulation")
    subprocess.run(["g++", "-std=c++20", "-O1", "-pthread", "-I", os.path.join(ROOT, "pangulu_amd", "csrc", "platform"),
                    os.path.join(ROOT, "tests", "factor_stats_kernel_emulation.cpp"), "-o", exe] + flags, check=True)
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert out.returncode == 0 and "0 failures OK" in out.stdout, out.stdout


def test_example_program_prints_the_diagnostics_with_c(tmp_path):
    """examples/solve_mtx -c on the reference's fixture: the three lines after the residual, and nothing of them without the flag"""
    from .test_example_program import TREFETHEN, build, residual_of, run

    exe = build(tmp_path, test_platform=True)
    plain = run(exe, "-f", TREFETHEN, "-n", "8")
    text = run(exe, "-f", TREFETHEN, "-n", "8", "-c")
    assert "rcond_1" not in plain and "growth" not in plain
    assert residual_of(text) < 1e-12
    tail = text[text.index("|| Ax - b ||"):].splitlines()[1:4]
    assert [ln.split(" = ")[0] for ln in tail] == ["rcond_1", "pivots clamped", "growth"], text
    A = np.asarray(__import__("scipy.io", fromlist=["mmread"]).mmread(TREFETHEN).todense())
    true = 1.0 / (np.linalg.norm(A, 1) * np.linalg.norm(np.linalg.inv(A), 1))
    # (the estimate of ||inv(A)|| is a lower bound of at least half the norm; %le prints seven digits)
    assert true * (1.0 - 1e-6) <= float(tail[0].split(" = ")[1]) <= 2.0 * true * (1.0 + 1e-6)
    assert int(tail[1].split(" = ")[1]) == 0 and 0.0 < float(tail[2].split(" = ")[1]) < 10.0  # (max|U| / max|A| of a diagonally dominant matrix)


@pytest.mark.parametrize("flags", [[], ["-DPANGULU_COMPLEX"]], ids=["real", "complex"])
def test_reproducible_gather_kernels_against_the_serial_formula(flags, tmp_path):
    """solve_gather_part_kernel / solve_gather_sum_kernel (pg_hip_block_solve_multi.h: the gathers of pangulu_amd_rcond's solves, no
    atomics) as host C++ (tests/solve_repro_gather_kernel_emulation.cpp): the formula, and the same bits from two runs"""
    exe = str(tmp_path / "emulation")
    subprocess.run(["g++", "-std=c++20", "-O1", "-pthread", "-I", os.path.join(ROOT, "pangulu_amd", "csrc", "platform"),
                    os.path.join(ROOT, "tests", "solve_repro_gather_kernel_emulation.cpp"), "-o", exe] + flags, check=True)
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert out.returncode == 0 and "0 failures OK" in out.stdout, out.stdout
