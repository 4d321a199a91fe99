"""One rank of a multi-process CPU run of pangulu_amd_gstrs_trans (launched by tests/test_solve_trans.py; modelled on
mp_solve_multi_worker.py).

With more than one rank the call runs the distributed host sweep over block columns once per right-hand side; rank 0 writes the
gathered answers -- r64 with trans N and T, cr64 with T and H -- to the output file, where the test compares them with SuperLU's.
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
from tests.helpers import oracle_library  # noqa: E402
from tests.solve_trans_common import conv, rhs_block  # noqa: E402


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    spec, nb, out_path, nrhs = sys.argv[1], int(sys.argv[2]), sys.argv[3], int(sys.argv[4])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    base_port = 20000 + (int(os.environ["MASTER_PORT"]) * 7) % 8000  # (as mp_worker.py: below the ephemeral range)
    results = {}
    for k, (vtype, transes) in enumerate((("r64", "NT"), ("cr64", "TH"))):
        lib = _lib.load(vtype, test_hooks=True)  # the checker's build of the host, operators routed to the CPU restatement
        assert lib.pangulu_amd_use_platform_library(oracle_library(vtype).encode(), _lib.PLATFORM_CPU_NAIVE) == 0
        assert lib.pangulu_amd_comm_init(rank, world, b"127.0.0.1", base_port + 64 * k, _lib.TRANSPORT_HOST, None) == 0
        mat = {"conv8": lambda: conv(8, _lib.VALUE_TYPES[vtype][0])}[spec]()
        n, cp, ri, va, co = mat
        if rank == 0:
            h = pa.pangulu_init(n, len(va), cp, ri, va, nb=nb, vtype=vtype, ordering="nd", coords=co, lib=lib)
        else:
            h = pa.pangulu_init(0, 0, None, None, None, nb=nb, vtype=vtype, ordering="nd", lib=lib)  # rank 0 broadcasts the matrix
        pa.pangulu_gstrf(h)
        B = rhs_block(mat, nrhs) if rank == 0 else None
        for trans in transes:
            # (inside pangulu_amd_gstrs_trans the other ranks' nrhs and trans are ignored: rank 0's decide -- they pass something else
            # to show it; "N" is the untransposed entry point on every rank)
            other = {"N": "N", "T": "H", "H": "T"}[trans]
            X = pa.pangulu_gstrs_multi(h, B, nrhs=nrhs if rank == 0 else 1, trans=trans if rank == 0 else other)
            results["X_%s_%s" % (vtype, trans)] = X
        results["device_columns"] = pa.last_solve_path(h)["device_columns"]
        pa.pangulu_finalize(h)
        lib.pangulu_amd_comm_finalize()
        dist.barrier()
    if rank == 0:
        np.savez(out_path, **results)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
