"""The transposed solve on the HIP path in a process of its own (launched by tests/test_gpu_solve_trans.py with
PANGULU_HIP_SOLVE_CHUNKED=0 in the environment: the switch is read once per process).  Writes what the back-end's transposed
operator answers when asked for its widest panel, the solutions of the first `nrhs` columns of the case's right-hand sides with
trans = "T", and what pangulu_amd_last_solve_path reports after the transposed and after an untransposed solve.
"""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import pangulu_amd as pa  # noqa: E402
from pangulu_amd import _lib  # noqa: E402
from tests.solve_trans_common import open_handle, rhs_block  # noqa: E402
from tests.test_gpu_solve_trans import INPUTS, _declare_trans_operator  # noqa: E402


def main():
    name, nb, nrhs, out_path = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
    vtype, gen, _ = INPUTS[name]
    mat = gen(_lib.VALUE_TYPES[vtype][0])
    B = rhs_block(mat, nrhs)
    h = open_handle(mat, nb, "hip", vtype)
    widest = _declare_trans_operator(h.lib)(nb, None, None, 0, None, 0, 0, None)
    X = pa.pangulu_gstrs_multi(h, B, trans="T")
    path = pa.last_solve_path(h)
    pa.pangulu_gstrs_multi(h, B)
    untransposed = pa.last_solve_path(h)["device_columns"]
    pa.pangulu_finalize(h)
    np.savez(out_path, X=X, operator_widest_panel=widest, untransposed_device_columns=untransposed, **path)


if __name__ == "__main__":
    main()
