"""pangulu_gstrs_multi on the HIP path in a process of its own (launched by tests/test_gpu_solve_multi.py with the back-end
switch under test in the environment: the switches are read once per process).  Writes the solutions of the first `nrhs` columns
of the case's right-hand sides and what pangulu_amd_last_solve_path reports to the output file.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import pangulu_amd as pa  # noqa: E402
from pangulu_amd import _lib  # noqa: E402
from tests.solve_multi_common import open_handle, rhs_block  # noqa: E402
from tests.test_gpu_solve_multi import CASES  # noqa: E402


def main():
    name, nrhs, out_path = sys.argv[1], int(sys.argv[2]), sys.argv[3]
    vtype, gen, nb, _ = CASES[name]
    mat = gen(_lib.VALUE_TYPES[vtype][0])
    B = rhs_block(mat, nrhs)
    h = open_handle(mat, nb, "hip", vtype)
    X = pa.pangulu_gstrs_multi(h, B)
    path = pa.last_solve_path(h)
    pa.pangulu_finalize(h)
    np.savez(out_path, X=X, **path)


if __name__ == "__main__":
    main()
