"""Directed block patterns and pivot-clamp values through the dense-mode HIP kernels (GETRF, TSTRF / GESSM, the MFMA updates)
and, once, the sparse ones: matrices whose 16 x 16 tile occupancy and tiny pivots are DESIGNED (tests/directed_blocks.py, pinned
without a GPU by tests/test_directed_blocks_cpu.py), compared entry by entry against an extended-precision LU with the bound
|L U~ - A'| <= c gamma_n |L||U~|  (c: largest condition number of a 16 x 16 diagonal tile of the reference's factors).

Every block is forced into dense mode (thresholds 0), so a block of seven entries runs the same kernels as a full one."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from pangulu_amd import _lib

from . import directed_blocks as D

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GENERAL_KERNEL_ONLY = {_lib.HIP_OPT_FRONT_STAGES: 0}
MODES = {"general": GENERAL_KERNEL_ONLY, "defaults": {}}


@pytest.fixture(scope="module")
def ref_cache(tmp_path_factory):
    return str(tmp_path_factory.mktemp("directed_refs"))


def _pattern(name, nb, vtype, mode, ref_cache):
    key = "%s-%d-%s" % (name, nb, vtype)
    mat = D.pattern_case(name, nb, vtype)
    ref = D.reference(key, mat, cache_dir=ref_cache)
    f = D.shared_figures(key, mat, nb, vtype, D.hip_factors(mat, nb, vtype, MODES[mode]), ref)
    print(json.dumps(f))
    D.assert_shared(f)
    if mode == "general":
        assert f["front_workgroups"] == 0 and f["general_workgroups"] > 0, f


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("nb", [128, 256])
@pytest.mark.parametrize("name", sorted(D.PATTERN_CASES))
def test_pattern_case_r64(name, nb, mode, ref_cache):
    _pattern(name, nb, "r64", mode, ref_cache)


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("name", D.CR64_PATTERN_CASES)
def test_pattern_case_cr64(name, mode, ref_cache):
    """The complex plane kernels (pg_hip_panels_complex.h)."""
    _pattern(name, 128, "cr64", mode, ref_cache)


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("name", D.R32_PATTERN_CASES)
def test_pattern_case_r32(name, mode, ref_cache):
    _pattern(name, 128, "r32", mode, ref_cache)


CLAMP_PARAMS = [(name, nb, "r64") for nb in (256, 128, 32) for name in D.CLAMP_VALUES] + \
               [(name, nb, "cr64") for nb in (256, 128, 32) for name in D.CLAMP_VALUES_COMPLEX]


@pytest.mark.parametrize("name,nb,vtype", CLAMP_PARAMS)
def test_pivot_clamp(name, nb, vtype, ref_cache):
    """The clamp rule |Re p| < 1e-16 -> +1e-16 (divisor only; the stored diagonal keeps its value) in every place it is written out:
    nb = 256 / 128 the dense GETRF kernels, the diagonal-tile inverses of the dense solves and z_pivot_rcp; nb = 32 with no block
    in dense mode getrf_kernel and the sparse solves.  The pivot sits at local index 0, 15, 16 and nb-1 of the first and the last
    diagonal block; its row holds nothing else, so nothing downstream depends on the huge column of L.  Why every value would
    fail without the rule: D.check_clamp_case.  No solve: the system is singular by design."""
    dense = nb >= 128
    key = "clamp-%s-%d-%s" % (name, nb, vtype)
    mat = D.clamp_case(name, nb, vtype)
    ref = D.reference(key, mat, D.clamp_pivots(nb), cache_dir=ref_cache)
    res = D.hip_factors(mat, nb, vtype, dense=dense)
    f = D.shared_figures(key, mat, nb, vtype, res, ref, backward=False)
    f["ratio"], f["column_ratio"] = D.check_clamp_case(name, nb, vtype, res["L"], res["U"], ref, mat, "hip")
    print(json.dumps(f))
    D.assert_shared(f, dense=dense)


@pytest.mark.parametrize("grouping", D.ARROW_GROUPINGS)
@pytest.mark.parametrize("depth", D.QUEUE_DEPTHS)
def test_update_queue_depth(depth, grouping):
    """A block arrow: `depth` updates into the last diagonal block, around the general update kernel's window of 16 queued updates
    (1, 15, 16, 17, 33).  The panels are exact by design (leading diagonal blocks 2 I), so the last block factorises
    S = A_last - sum_k L_k U_k, known in extended precision from `depth` 128 x 128 products.  Asserted on the last block:
    componentwise_check on S (gamma over S's own size 128, denominator |L_last||U_last|), the forward bound against the
    extended-precision factors of S, and the entry-wise difference from the oracle's factors within twice that bound.
    How the queue reaches the kernel (D.ARROW_GROUPINGS, argued from launch_ssssm): with the suite's settings every update is a group
    of ONE task, so the kernel's task windows hold one task at every depth; "one_group" leaves the whole queue in one group, so a
    workgroup walks 1 / 15 / 16 / 17 / 33 tasks in one, one, one, two and three windows; "one_group_first_kernel" the same on the
    first general kernel.  All groups are K-split by four and merge with atomics (launches of at most 64 tasks).  One workgroup
    per (group, K quarter) with a live step: exactly 4 with the queue in one group, more with a group per update -- asserted.
    Observed on an MI355X with the default scheduler: the `depth` updates arrive in one call of the update launch at every depth
    (ssssm_dense_mfma: tasks = depth, launches = 1).  Backward ratios at depths 1 / 15 / 16 / 17 / 33: group per update
    0.14 / 0.28 / 0.22 / 0.29 / 0.51 to 0.74 (two runs: the order of the atomic merges is not fixed), one group 0.14 / 0.26 / 0.27 / 0.65 / 0.60 (both kernels alike), the oracle
    0.17 / 0.26 / 0.20 / 0.26 / 0.74; against the oracle's factors at most 0.025 of the allowed difference."""
    f = D.arrow_figures(depth, 128, D.arrow_grouping_options(grouping))
    print(json.dumps(f))
    assert f["dense_update_launches"] == 1 and f["front_workgroups"] == 0, f
    if grouping != "group_per_update" or depth == 1:
        assert f["general_workgroups"] == 4, f
    else:
        assert 4 < f["general_workgroups"] <= 4 * depth, f
    D.assert_arrow(f)


_children = {}


def _child(env, group, ref_cache, timeout):
    key = (tuple(sorted(env.items())), group)
    if key in _children:
        return _children[key]
    e = dict(os.environ)
    e.update(env)
    e["PYTHONPATH"] = ROOT + os.pathsep + e.get("PYTHONPATH", "")
    e["PG_DIRECTED_REF_CACHE"] = ref_cache
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "directed_blocks_worker.py"), group], env=e, cwd=ROOT,
                         capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stderr[-2000:]
    _children[key] = [json.loads(ln) for ln in out.stdout.splitlines() if ln.startswith("{")]
    return _children[key]


SWITCHES = [{}, {"PANGULU_HIP_GETRF_PIPE": "0"}, {"PANGULU_HIP_TRSM_RING": "0"}, {"PANGULU_HIP_TRSM_DIRECT": "0"}]


@pytest.mark.parametrize("env", SWITCHES, ids=["+".join("%s=%s" % kv for kv in e.items()) or "defaults" for e in SWITCHES])
def test_non_default_kernels(env, ref_cache):
    """The tiled GETRF, the barrier-free dense solves and the LDS-staged dense solves are chosen by switches read once per process:
    one fresh child per switch (and one for the defaults) runs the pattern cases and the clamp cases at nb = 256.
    That a switch selected another kernel shows in the factors' bits (another kernel sums in another order): each run carries a
    fingerprint of its factors' values, and a switched child must differ from the defaults' child on at least one case.  Observed:
    GETRF_PIPE=0 differs on all 14 cases, TRSM_RING=0 and TRSM_DIRECT=0 on 12 (not on corners and single_tiles)."""
    runs = _child(env, "nb256", ref_cache, 300)
    assert len(runs) == len(D.PATTERN_CASES) + len(D.CLAMP_VALUES) + len(D.CLAMP_VALUES_COMPLEX), runs
    for r in runs:
        assert "clamp_failure" not in r, r
        D.assert_shared(r)
    base = {r["case"]: r["bits"] for r in _child({}, "nb256", ref_cache, 300)}
    differ = sorted(r["case"] for r in runs if r["bits"] != base[r["case"]])
    print(json.dumps({"switch": env, "worst_ratio": max(r["ratio"] for r in runs), "worst_column_ratio": max(r.get("column_ratio", 0) for r in runs),
                      "cases_with_other_bits_than_defaults": differ}))
    if env:
        assert differ, "%r gave the same bits as the defaults on every case: the switch selected nothing" % (env,)


def test_update_queue_depth_as_one_queue(ref_cache):
    """The same depths, every queue in one group, with every update deferred to the destination's own panel task
    (PANGULU_AMD_LOOKAHEAD_MAX_GETRF=0, read once per process: a child)."""
    runs = _child({"PANGULU_AMD_LOOKAHEAD_MAX_GETRF": "0"}, "arrow", ref_cache, 300)
    assert [r["depth"] for r in runs] == D.QUEUE_DEPTHS, runs
    for r in runs:
        assert r["dense_update_launches"] == 1 and r["general_workgroups"] == 4, r
        D.assert_arrow(r)
    print(json.dumps({"launches_per_depth": {r["depth"]: r["dense_update_launches"] for r in runs}, "worst_ratio": max(r["ratio"] for r in runs)}))
