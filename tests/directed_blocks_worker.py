"""Child process of tests/test_gpu_directed_blocks.py: the directed block cases (tests/directed_blocks.py) on the HIP back-end with
whatever back-end environment switches the parent set (they are read once per process).  Prints one JSON line per run.

    directed_blocks_worker.py nb256     the pattern cases and the pivot-clamp cases at nb = 256
    directed_blocks_worker.py arrow     the queue-depth cases, every queue in one group (D.ARROW_GROUPINGS)

PG_DIRECTED_REF_CACHE: a directory where the parent keeps the references' small parts, so that no child repeats the
extended-precision LU."""
import json
import os
import sys

import numpy as np

from tests import directed_blocks as D


def main():
    which = sys.argv[1] if len(sys.argv) > 1 else "nb256"
    cache = os.environ.get("PG_DIRECTED_REF_CACHE")
    if which == "nb256":
        nb = 256
        for name in sorted(D.PATTERN_CASES):
            key = "%s-%d-r64" % (name, nb)
            mat = D.pattern_case(name, nb)
            ref = D.reference(key, mat, cache_dir=cache)
            print(json.dumps(D.shared_figures(key, mat, nb, "r64", D.hip_factors(mat, nb, "r64"), ref)), flush=True)
        for vtype, values in (("r64", D.CLAMP_VALUES), ("cr64", D.CLAMP_VALUES_COMPLEX)):
            for name in values:
                key = "clamp-%s-%d-%s" % (name, nb, vtype)
                mat = D.clamp_case(name, nb, vtype)
                ref = D.reference(key, mat, D.clamp_pivots(nb), cache_dir=cache)
                res = D.hip_factors(mat, nb, vtype)
                f = D.shared_figures(key, mat, nb, vtype, res, ref)
                try:
                    f["ratio"], f["column_ratio"] = D.check_clamp_case(name, nb, vtype, res["L"], res["U"], ref, mat, "hip")
                except AssertionError as e:
                    f["clamp_failure"] = str(e)[:500]
                print(json.dumps(f), flush=True)
    elif which == "arrow":
        for depth in D.QUEUE_DEPTHS:
            print(json.dumps(D.arrow_figures(depth, 128, D.arrow_grouping_options("one_group"))), flush=True)
    else:
        raise SystemExit("unknown group %r" % which)


if __name__ == "__main__":
    main()
