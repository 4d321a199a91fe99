"""One rank of a two-process CPU run of pangulu_amd_update_values_device (launched by tests/test_update_values_device.py; modelled on
mp_factor_stats_worker.py).

With more than one rank the call has no path: every rank gets 4 without any exchange and nothing has been touched -- the records are
the ones pangulu_init made, and the factorisation that follows is that of the original matrix.
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
from tests import update_values_device_common as U  # noqa: E402
from tests.helpers import oracle_library  # noqa: E402


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    out_path = sys.argv[1]
    dist.init_process_group("gloo", rank=rank, world_size=world)
    base_port = 20000 + (int(os.environ["MASTER_PORT"]) * 7) % 8000  # (as mp_worker.py: below the ephemeral range)
    name = "fem27_10_nb32"
    mat, vtype, nb = U.case(name)
    lib = _lib.load(vtype, test_hooks=True)  # the checker's build of the host, operators routed to the CPU restatement
    assert lib.pangulu_amd_use_platform_library(oracle_library(vtype).encode(), _lib.PLATFORM_CPU_NAIVE) == 0
    assert lib.pangulu_amd_comm_init(rank, world, b"127.0.0.1", base_port, _lib.TRANSPORT_HOST, None) == 0
    n, cp, ri, va, co = mat
    if rank == 0:
        h = pa.pangulu_init(n, len(va), cp, ri, va, nb=nb, vtype=vtype, ordering="nd", coords=co, lib=lib)
    else:
        h = pa.pangulu_init(0, 0, None, None, None, nb=nb, vtype=vtype, ordering="nd", lib=lib)  # rank 0 broadcasts the matrix
    before = U.records(h)
    rc = U.raw_update_device(h, U.new_values(name)[3].ctypes.data)
    after = U.records(h)
    unchanged = len(before) == len(after) and all(a[3].tobytes() == b[3].tobytes() for a, b in zip(before, after))
    pa.pangulu_gstrf(h)
    check = pa.factor_check(h)  # (collective; the original matrix)
    everyone = [None] * world
    dist.all_gather_object(everyone, (rc, unchanged))
    pa.pangulu_finalize(h)
    lib.pangulu_amd_comm_finalize()
    dist.barrier()
    if rank == 0:
        np.savez(out_path, return_codes=np.array([c for c, _ in everyone]), records_unchanged=np.array([u for _, u in everyone]),
                 factor_check=np.array(check))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
