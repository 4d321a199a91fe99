"""pangulu_amd_update_values_device without a device: the checker's build of the host on the oracle's CPU operators, whose memory is
host memory -- the pointer is a numpy buffer and the map (pg_values_refresh.cpp) is applied by the host loop.  What the map must get
right is the same as on the device: every value in its record, padding rows' unit diagonals and inserted diagonals kept, fill zeroed.
Reference and bounds: tests/update_values_device_common.py."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import pangulu_amd as pa

from . import update_values_device_common as U
from .helpers import ROOT, oracle_library
from .solve_multi_common import open_handle
from .test_scaling import saddle


@pytest.mark.parametrize("name", ["fem27_10_nb32", "cr64_conv12_nb32", "r64_rand3000", "r32_rand1536"])
def test_records_factors_and_norms_after_values_from_a_buffer(name):
    mat, vtype, nb = U.case(name)
    m2 = U.new_values(name)
    plat = oracle_library(vtype)
    want = U.twin_records(name, plat, m2[3])
    h = open_handle(mat, nb, plat, vtype)  # (factorised: the records hold factors, fill included)
    try:
        info = h.info()
        if name == "cr64_conv12_nb32":
            assert info["n_padded"] > info["n"]
        if name == "r64_rand3000":
            assert info["n"] % nb != 0  # a short last block
        assert U.raw_update_device(h, m2[3].ctypes.data) == 0
        got = U.records(h)
        U.assert_records_bit_equal(got, want)
        if name == "cr64_conv12_nb32":
            # the padding rows are isolated identity rows: their unit diagonals are not the user's values and survive
            perm = pa.permutation(h)
            pad = np.flatnonzero(perm >= info["n"])
            assert len(pad) == info["n_padded"] - info["n"]
            diag = {}
            for br, bc, up, cp, ri, va in pa.owned_blocks(h):
                if br == bc and up:
                    for r in range(nb):
                        if cp[r + 1] > cp[r] and ri[cp[r]] == r:
                            diag[br * nb + r] = va[cp[r]]
            assert all(diag[int(i)] == 1.0 for i in pad)
        # a second call on the same handle reuses the map and gives the same records
        assert U.raw_update_device(h, m2[3].ctypes.data) == 0
        U.assert_records_bit_equal(U.records(h), want)
        U.factor_solve_and_compare(h, name, m2, plat)
        # Aperm and the norms describe the new matrix
        U.assert_norms_describe(h, m2)
    finally:
        pa.pangulu_finalize(h)


def test_inserted_diagonals_are_kept():
    """saddle(5) without scaling: half of the diagonal is structurally empty and gets 1e-8 entries that are not the user's.  Only
    the records are compared: this factorisation is inaccurate by design."""
    mat = saddle(5)
    n, cp, ri, va, _ = mat
    plat = oracle_library("r64")
    new = np.ascontiguousarray(va * np.random.default_rng(3).uniform(0.5, 1.5, len(va)))
    handles = [open_handle(mat, 16, plat, "r64", gstrf=True) for _ in range(2)]
    try:
        h, t = handles
        assert h.info()["inserted_diagonals"] == n // 2
        pa.update_values(t, new)
        assert U.raw_update_device(h, new.ctypes.data) == 0
        got, want = U.records(h), U.records(t)
        U.assert_records_bit_equal(got, want)
        assert sum(int((v == 1e-8).sum()) for _, _, up, v in got if up) == n // 2
    finally:
        for x in handles:
            pa.pangulu_finalize(x)


def test_refusals_touch_nothing():
    name = "fem27_10_nb32"
    mat, vtype, nb = U.case(name)
    m2 = U.new_values(name)
    plat = oracle_library(vtype)
    h = open_handle(mat, nb, plat, vtype, gstrf=False)
    try:
        before = U.records(h)
        assert U.raw_update_device(h, None) == 2
        U.assert_records_bit_equal(U.records(h), before)
        pa.pangulu_gstrf(h)  # (still armed: a refused call has not touched the counters either)
        assert pa.factor_check(h) <= 1e-12
    finally:
        pa.pangulu_finalize(h)
    s = open_handle(mat, nb, plat, vtype, scaling=True, gstrf=False)
    try:
        before = U.records(s)
        assert U.raw_update_device(s, m2[3].ctypes.data) == 1
        U.assert_records_bit_equal(U.records(s), before)
    finally:
        pa.pangulu_finalize(s)


def test_cpu_tensor_takes_the_numpy_path():
    import torch

    name = "fem27_10_nb32"
    mat, vtype, nb = U.case(name)
    m2 = U.new_values(name)
    plat = oracle_library(vtype)
    want = U.twin_records(name, plat, m2[3])
    h = open_handle(mat, nb, plat, vtype)
    try:
        pa.update_values(h, torch.from_numpy(m2[3].copy()))
        U.assert_records_bit_equal(U.records(h), want)
        with pytest.raises(TypeError):
            pa.update_values(h, torch.from_numpy(m2[3].astype(np.float32)))
        with pytest.raises(ValueError):
            pa.update_values(h, torch.from_numpy(m2[3][:-1].copy()))
    finally:
        pa.pangulu_finalize(h)


def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_ranks_get_code_4(tmp_path):
    out = str(tmp_path / "out.npz")
    port = free_port()
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   OMP_NUM_THREADS="1", PANGULU_AMD_SEPARATOR_MAP="cyclic")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "mp_update_values_device_worker.py"), out],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=int(os.environ.get("PANGULU_TEST_RANK_TIMEOUT", "420")))
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        outs.append(o)
    failed = [r for r, p in enumerate(procs) if p.returncode != 0]
    assert not failed, "ranks %s failed:\n%s" % (failed, "\n".join("--- rank %d ---\n%s" % (r, outs[r][-3000:]) for r in range(2)))
    z = np.load(out)
    assert list(z["return_codes"]) == [4, 4]
    assert z["records_unchanged"].all() and z["factor_check"] <= 1e-12
