"""Child process of tests/test_gpu_front_kernel_small.py: all-tiles-live block matrices on the HIP back-end, with whatever
back-end environment switches the parent set (they are read once per process).  Prints one JSON line per case.

    front_kernel_worker.py <vtype>:<nb>:<K>:<front stages> [...]

PG_DIRECTED_REF_CACHE: a directory where the references' small parts are kept, so that a case that runs under several settings
pays for its extended-precision LU once."""
import json
import os
import sys

from tests import directed_blocks as D


def front_case(nb, K, vtype="r64"):
    """K x K blocks, every 16 x 16 tile of every block live: every update is a dense-front product on every tile.
    Block (I,J) takes min(I,J) updates -- the last diagonal block a queue of K - 1."""
    off = {(I, J): "full" for I in range(K) for J in range(K) if I != J}
    return D.block_matrix(nb, K, ["dense"] * K, off, vtype=vtype, seed=4000 + 10 * K + nb // 128)


def case_key(vtype, nb, K):
    return "front-%s-%d-K%d" % (vtype, nb, K)


def queued_updates(K):
    """Updates of a K x K all-live block matrix: sum over destinations (I,J), I, J >= 1, of min(I,J)."""
    return sum(min(I, J) for I in range(1, K) for J in range(1, K))


def run_case(vtype, nb, K, stages, cache=None):
    from pangulu_amd import _lib

    key = case_key(vtype, nb, K)
    mat = front_case(nb, K, vtype)
    ref = D.reference(key, mat, cache_dir=cache)
    # group chunk 0: a destination's queue stays ONE group (D.ARROW_GROUPINGS, "one_group"), so a workgroup walks the whole queue
    opts = {_lib.HIP_OPT_SSSSM_GROUP_CHUNK: 0, _lib.HIP_OPT_FRONT_STAGES: stages}
    f = D.shared_figures(key, mat, nb, vtype, D.hip_factors(mat, nb, vtype, opts), ref)
    f.update({"vtype": vtype, "nb": nb, "K": K, "stages": stages})
    return f


def main():
    cache = os.environ.get("PG_DIRECTED_REF_CACHE")
    for spec in sys.argv[1:]:
        vtype, nb, K, stages = spec.split(":")
        print(json.dumps(run_case(vtype, int(nb), int(K), int(stages), cache)), flush=True)


if __name__ == "__main__":
    main()
