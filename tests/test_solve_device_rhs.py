"""pangulu_amd_gstrs_device and the torch tensors of pa.pangulu_gstrs_multi without a device: on the checker's build of the host with
the oracle's CPU operators (a host-memory platform) the device-resident path does not exist, so the C call answers with its return
codes and touches nothing, and a CPU tensor takes the numpy path of the same handle."""
import ctypes

import numpy as np
import pytest
import torch

import pangulu_amd as pa
from pangulu_amd import _lib

from .helpers import oracle_library
from .solve_trans_common import conv, open_handle, rhs_block

_mats = {}


def case(vtype):
    if vtype not in _mats:
        mat = conv(8, _lib.VALUE_TYPES[vtype][0])
        B = rhs_block(mat, 5)
        B.setflags(write=False)
        _mats[vtype] = (mat, B)
    return _mats[vtype]


def raw_gstrs_device(h, ptr, nrhs, ldb, trans, stream=None):
    """The C call as it is, return code included."""
    opt = _lib.GstrsOptions()
    return h.lib.pangulu_amd_gstrs_device(ptr, int(nrhs), int(ldb), int(trans), stream, ctypes.byref(opt), h.ref)


def test_return_codes_on_a_host_memory_platform():
    mat, B = case("r64")
    n, nrhs = B.shape
    h = open_handle(mat, 16, oracle_library("r64"), "r64", gstrf=False)
    try:
        buf = np.full((n + 5, nrhs), -777.25, order="F")
        buf[:n] = B
        before = buf.copy(order="F")
        ptr = buf.ctypes.data_as(ctypes.c_void_p)
        assert raw_gstrs_device(h, ptr, nrhs, n + 5, 0) == 1  # not factorised
        pa.pangulu_gstrf(h)
        for bad in (7, 3, -1):
            assert raw_gstrs_device(h, ptr, nrhs, n + 5, bad) == 3
        assert raw_gstrs_device(h, ptr, nrhs, n - 1, 1) == 2
        assert raw_gstrs_device(h, None, nrhs, n + 5, 0) == 2
        assert raw_gstrs_device(h, None, 0, 0, 0) == 0  # (nothing to do: nothing is looked at)
        for trans in (0, 1, 2):
            assert raw_gstrs_device(h, ptr, nrhs, n + 5, trans) == 4  # no device-resident path here
        assert (buf == before).all()
    finally:
        pa.pangulu_finalize(h)


@pytest.mark.parametrize("vtype", ["r64", "cr64"])
@pytest.mark.parametrize("trans", ["N", "T"])
def test_cpu_tensor_takes_the_numpy_path(vtype, trans):
    mat, B = case(vtype)
    h = open_handle(mat, 16, oracle_library(vtype), vtype)
    try:
        want = pa.pangulu_gstrs_multi(h, B, trans=trans)
        T = torch.from_numpy(B.copy())
        keep = T.clone()
        X = pa.pangulu_gstrs_multi(h, T, trans=trans)
        x0 = pa.pangulu_gstrs(h, T[:, 3].contiguous(), trans=trans)
        with pytest.raises(TypeError):
            pa.pangulu_gstrs_multi(h, torch.zeros(B.shape, dtype=torch.float32 if vtype == "r64" else torch.float64), trans=trans)
        with pytest.raises(ValueError):
            pa.pangulu_gstrs_multi(h, T[:-1], trans=trans)
    finally:
        pa.pangulu_finalize(h)
    assert isinstance(X, torch.Tensor) and X.device.type == "cpu" and tuple(X.shape) == B.shape
    assert (X.numpy() == want).all()  # the same path on the same handle: bit for bit
    assert torch.equal(T, keep)  # the input is not modified
    assert isinstance(x0, torch.Tensor) and tuple(x0.shape) == (B.shape[0],)
    assert (x0.numpy() == want[:, 3]).all()
