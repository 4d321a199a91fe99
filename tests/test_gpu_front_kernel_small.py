"""The dense-front update kernel (ssssm_front_f64_kernel, pg_hip_front.h) at the smallest shapes at which its pipeline can go
wrong: all-tiles-live block matrices of K x K blocks (tests/front_kernel_worker.py), compared entry by entry against an
extended-precision LU with the bound and the tolerances of tests/directed_blocks.py.

How the kernel is reached.  It gets a launch of its own from PANGULU_HIP_FRONT_MIN_WGS qualifying (destination, tile) pairs on
(default 2 048), and a pair qualifies only if its group is not K-split -- but EVERY update launch of at most 64 workgroups is K-split
by four (launch_ssssm), which is every launch of these matrices: tests/test_gpu_directed_blocks.py observes front_workgroups == 0
on its all-live case for that reason (observed here too: PANGULU_HIP_FRONT_MIN_WGS=1 alone, K = 3, nb = 128: front_workgroups 0,
general_workgroups 20).  So the children here run with PANGULU_HIP_FRONT_MIN_WGS=1 AND PANGULU_HIP_KSPLIT=0; with
PANGULU_AMD_LOOKAHEAD_MAX_GETRF=0, which defers every update to its destination's own panel task, so that a destination's updates
arrive in ONE call (with the default look-ahead they arrive one per call: observed 30 workgroups of one update each at K = 5,
16 of up to four with the deferral); and with the group chunk at 0, so that the queue is ONE group that one workgroup per tile
walks.  The three switches are read once per process: fresh children, like test_non_default_kernels.  Every case asserts
front_workgroups > 0 first, then that there is exactly one workgroup per (destination, tile): the queues are whole.

What the shapes exercise.  A task is nb / 16 slab steps: 8 at nb = 128, 16 at nb = 256.  Block (I,J) of a K x K matrix takes
min(I,J) updates, so K = 2, 3, 5 give queues of up to 1, 2 and 4 tasks:
  * one task at nb = 128 is the shortest pipeline -- T = 8 steps, all requests of one task, the operand pointers never handed over;
  * queues of 2 and 4 have requests that cross one and three task boundaries: the pointer pair of the next task is loaded one step
    before the first request that needs it and takes over after that step's request;
  * 2, 3 and 4 LDS stages (HIP_OPT_FRONT_STAGES, the option behind PANGULU_HIP_FRONT_STAGES) move the request 1, 2 and 3 slabs
    ahead of the products: the counted waits, and the hand-over at every distance;
  * CR64: four real products per update, the sign of a product changes per task -- the sign of the task being CONSUMED is handed
    over at another step than the pointers of the task being REQUESTED.
With PANGULU_HIP_FRONT_MIN_WGS at its default the same pairs stay inside the general launch (work items with pad_ = 1), where
ssssm_tilesv_f64_kernel branches into the same step loop at entry."""
import json
import os
import subprocess
import sys

import pytest

from . import front_kernel_worker as W

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WHOLE_QUEUES = {"PANGULU_HIP_KSPLIT": "0", "PANGULU_AMD_LOOKAHEAD_MAX_GETRF": "0"}
OWN_LAUNCH = {"PANGULU_HIP_FRONT_MIN_WGS": "1", **WHOLE_QUEUES}

QUEUE_CASES = [("r64", nb, K, 2) for nb in (128, 256) for K in (2, 3, 5)]
STAGE_CASES = [("r64", 128, 3, stages) for stages in (2, 3, 4)]
CR64_CASE = ("cr64", 128, 3, 2)
OWN_LAUNCH_CASES = QUEUE_CASES + [c for c in STAGE_CASES if c not in QUEUE_CASES] + [CR64_CASE]
INSIDE_GENERAL_CASE = ("r64", 128, 3, 2)


@pytest.fixture(scope="module")
def ref_cache(tmp_path_factory):
    return str(tmp_path_factory.mktemp("front_refs"))


_children = {}


def _child(env, cases, ref_cache):
    """One fresh child per environment runs all of its cases; {(vtype, nb, K, stages): figures}."""
    key = tuple(sorted(env.items()))
    if key not in _children:
        e = dict(os.environ)
        e.update(env)
        e["PYTHONPATH"] = ROOT + os.pathsep + e.get("PYTHONPATH", "")
        e["PG_DIRECTED_REF_CACHE"] = ref_cache
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "front_kernel_worker.py")] + ["%s:%d:%d:%d" % c for c in cases],
                             env=e, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        runs = [json.loads(ln) for ln in out.stdout.splitlines() if ln.startswith("{")]
        assert len(runs) == len(cases), out.stdout[-2000:]
        _children[key] = {(r["vtype"], r["nb"], r["K"], r["stages"]): r for r in runs}
    return _children[key]


def _assert_front(f):
    from . import directed_blocks as D

    print(json.dumps(f))
    tiles = (f["nb"] // 128) ** 2 * (2 if f["vtype"] == "cr64" else 1)  # (CR64: a group per destination PLANE)
    assert f["front_workgroups"] > 0, f  # otherwise the case tests nothing
    # every update is a dense-front product on every tile: no workgroup of the general kind, no sparse update
    assert f["general_workgroups"] == 0 and f["sparse_updates"] == 0, f
    assert f["dense_updates"] == W.queued_updates(f["K"]), f
    # one workgroup per (group, tile), and a destination's whole queue is one group: block (I,J) walks min(I,J) tasks
    assert f["front_workgroups"] == (f["K"] - 1) ** 2 * tiles, f
    # one update launch per call, as tests/test_gpu_directed_blocks.py counts them.  With every update deferred to its destination's
    # panel task, panel step k = 1 .. K-1 makes one call for the queue of the diagonal block (k,k) in front of its GETRF and, unless
    # it is the last step, one for the queues of the blocks (i,k), (k,j), i, j > k, in front of their solves: 2 (K-2) + 1 calls
    assert f["dense_update_launches"] == 2 * f["K"] - 3, f
    D.assert_shared(f)


@pytest.mark.parametrize("vtype,nb,K,stages", QUEUE_CASES, ids=["%s-nb%d-K%d-S%d" % c for c in QUEUE_CASES])
def test_front_kernel_queues(vtype, nb, K, stages, ref_cache):
    """Queues of up to 1, 2 and 4 updates at 8 and 16 steps per task, two stages."""
    _assert_front(_child(OWN_LAUNCH, OWN_LAUNCH_CASES, ref_cache)[(vtype, nb, K, stages)])


@pytest.mark.parametrize("stages", [2, 3, 4])
def test_front_kernel_stages(stages, ref_cache):
    """2, 3 and 4 LDS stages on the K = 3 case: the counted waits with the request behind the first products."""
    _assert_front(_child(OWN_LAUNCH, OWN_LAUNCH_CASES, ref_cache)[("r64", 128, 3, stages)])


def test_front_kernel_cr64(ref_cache):
    """Complex updates as four real products per update: the sign changes per task inside a queue."""
    _assert_front(_child(OWN_LAUNCH, OWN_LAUNCH_CASES, ref_cache)[CR64_CASE])


def test_front_pairs_inside_the_general_launch(ref_cache):
    """PANGULU_HIP_FRONT_MIN_WGS at its default: the qualifying pairs stay in the general launch as work items with pad_ = 1 and
    count as front workgroups."""
    f = _child(WHOLE_QUEUES, [INSIDE_GENERAL_CASE], ref_cache)[INSIDE_GENERAL_CASE]
    _assert_front(f)
