"""One rank of a multi-process CPU run of pangulu_amd_factor_stats and pangulu_amd_rcond (launched by tests/test_factor_stats.py;
modelled on mp_solve_trans_worker.py).

With more than one rank every rank examines the records it owns and rank 0 combines the partial results in rank order; the estimator
runs on rank 0's host vector, the other ranks follow its solves.  Every rank gets the values: rank 0 writes its own to the output
file and says whether the others reported the same.
"""
import faulthandler
import os
import sys

faulthandler.enable()

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch.distributed as dist  # noqa: E402

import pangulu_amd as pa  # noqa: E402
from pangulu_amd import _lib  # noqa: E402
from tests import factor_stats_common as C  # noqa: E402
from tests.helpers import oracle_library  # noqa: E402


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    name, out_path = sys.argv[1], sys.argv[2]
    dist.init_process_group("gloo", rank=rank, world_size=world)
    base_port = 20000 + (int(os.environ["MASTER_PORT"]) * 7) % 8000  # (as mp_worker.py: below the ephemeral range)
    mat, vtype, nb, ordering, scaling = C.case(name)
    lib = _lib.load(vtype, test_hooks=True)  # the checker's build of the host, operators routed to the CPU restatement
    assert lib.pangulu_amd_use_platform_library(oracle_library(vtype).encode(), _lib.PLATFORM_CPU_NAIVE) == 0
    assert lib.pangulu_amd_comm_init(rank, world, b"127.0.0.1", base_port, _lib.TRANSPORT_HOST, None) == 0
    n, cp, ri, va, co = mat
    if rank == 0:
        h = pa.pangulu_init(n, len(va), cp, ri, va, nb=nb, vtype=vtype, ordering=ordering, coords=co, lib=lib, scaling=scaling)
    else:
        h = pa.pangulu_init(0, 0, None, None, None, nb=nb, vtype=vtype, ordering=ordering, lib=lib, scaling=scaling)  # rank 0 broadcasts the matrix
    pa.pangulu_gstrf(h)
    codes = []
    rc, raw = C.raw_factor_stats(h)
    codes.append(rc)
    stats, sl = pa.factor_stats(h), pa.slogdet(h)
    assert stats == dict(raw.as_dict(), det=stats["det"])
    rcond = {}
    for norm, code in (("1", 0), ("I", 1)):
        # (the other ranks' `norm` is ignored: rank 0's decides -- they pass the other one to show it)
        res = C.raw_rcond(h, code if rank == 0 else 1 - code)
        codes.append(res[0])
        rcond[norm] = dict(zip(("rcond", "anorm", "ainv_norm", "solves", "on_device"), res[1:]))
    mine = [stats[k] for k in sorted(stats) if k != "det"] + [rcond[k][f] for k in "1I" for f in sorted(rcond[k])]
    everyone = [None] * world
    dist.all_gather_object(everyone, (codes, mine))
    pa.pangulu_finalize(h)
    lib.pangulu_amd_comm_finalize()
    dist.barrier()
    if rank == 0:
        np.savez(out_path, stats=np.array(stats, dtype=object), slogdet=np.array(sl), rcond_1=np.array(rcond["1"], dtype=object),
                 rcond_I=np.array(rcond["I"], dtype=object), return_codes=np.array([c for cs, _ in everyone for c in cs]),
                 other_ranks_agree=np.array(all(m == mine for _, m in everyone)))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
