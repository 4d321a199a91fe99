"""One rank of a multi-process CPU run of pangulu_amd_gstrs_multi (launched by tests/test_solve_multi.py; modelled on mp_worker.py).

With more than one rank the call loops the distributed host sweep over the columns; rank 0 compares every column with
pangulu_gstrs on that column alone in the same run and writes the largest relative difference to the output file.
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
from pangulu_amd import matrices as M  # noqa: E402
from tests.helpers import oracle_library  # noqa: E402
from tests.solve_multi_common import rhs_block  # noqa: E402


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    spec, nb, out_path, nrhs = sys.argv[1], int(sys.argv[2]), sys.argv[3], int(sys.argv[4])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    lib = _lib.load("r64", test_hooks=True)  # the checker's build of the host, operators routed to the CPU restatement
    assert lib.pangulu_amd_use_platform_library(oracle_library("r64").encode(), _lib.PLATFORM_CPU_NAIVE) == 0
    base_port = 20000 + (int(os.environ["MASTER_PORT"]) * 7) % 8000  # (as mp_worker.py: below the ephemeral range)
    assert lib.pangulu_amd_comm_init(rank, world, b"127.0.0.1", base_port, _lib.TRANSPORT_HOST, None) == 0
    mat = {"fem27_6": lambda: M.fem27(6)}[spec]()
    n, cp, ri, va, co = mat
    if rank == 0:
        h = pa.pangulu_init(n, len(va), cp, ri, va, nb=nb, vtype="r64", ordering="nd", coords=co, lib=lib)
    else:
        h = pa.pangulu_init(0, 0, None, None, None, nb=nb, vtype="r64", ordering="nd", lib=lib)  # rank 0 broadcasts the matrix
    pa.pangulu_gstrf(h)
    B = rhs_block(mat, nrhs) if rank == 0 else None
    X = pa.pangulu_gstrs_multi(h, B, nrhs=nrhs)  # (the other ranks' nrhs is ignored: rank 0's decides)
    path = pa.last_solve_path(h)
    singles = [pa.pangulu_gstrs(h, np.ascontiguousarray(B[:, j]) if rank == 0 else None) for j in range(nrhs)]
    if rank == 0:
        worst = 0.0
        for j in range(nrhs):
            scale = np.abs(singles[j]).max()
            worst = max(worst, float(np.abs(X[:, j] - singles[j]).max() / scale) if scale else float(np.abs(X[:, j]).max()))
        residual = max(M.relative_residual(n, cp, ri, va, X[:, j], B[:, j]) for j in range(nrhs) if B[:, j].any())
        np.savez(out_path, worst=worst, residual=residual, zero_column=float(np.abs(X[:, 1]).max()), device_columns=path["device_columns"])
    pa.pangulu_finalize(h)
    lib.pangulu_amd_comm_finalize()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
