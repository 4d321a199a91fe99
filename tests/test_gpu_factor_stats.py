"""pangulu_amd_factor_stats and pangulu_amd_rcond on the device: the statistics kernel over the device-resident records
(pangulu_platform_0201001_factor_stats) and the estimator on device vectors (pangulu_platform_0201001_condest_vector between
device-resident solves), pg_hip_factor_stats.h.  References and bounds: tests/factor_stats_common.py.  The reductions are fixed trees
without atomics, so two calls must agree in every bit; the device and the host path of one handle read the same factors, so maxima,
minima and counts must be equal and the determinant's mantissa within 4 n 2^-53."""
import ctypes
import math

import numpy as np
import pytest
import torch  # (before the library initialises the device: torch finds none on a HIP runtime that is not its own)

import pangulu_amd as pa

from . import factor_stats_common as C
from . import slots
from .helpers import library_for

pytestmark = pytest.mark.gpu

RCOND_INPUTS = ["r64_conv10", "r64_conv14", "cr64_conv12", "r64_rand3000", "r32_rand1536", "cr32_conv10", "graded_r64"]


@pytest.mark.parametrize("name", RCOND_INPUTS)
def test_rcond_on_device_vectors(name, monkeypatch):
    monkeypatch.setenv("PANGULU_AMD_DEVICE_SOLVE", "1")
    vtype = C.case(name)[1]
    lib = library_for("hip", vtype)
    h = C.open_case(name, "hip")
    try:
        first = {norm: pa.rcond(h, norm, details=True) for norm in ("1", "I")}
        assert h.info()["time_solve"] > 0
        assert pa.hip_memory(h)["solve_workspace_bytes"] > 0
        monkeypatch.setenv("PANGULU_AMD_DEVICE_SOLVE", "0")
        host = {norm: pa.rcond(h, norm, details=True) for norm in ("1", "I")}
        monkeypatch.setenv("PANGULU_AMD_DEVICE_SOLVE", "1")
    finally:
        pa.pangulu_finalize(h)
    assert pa.hip_memory(lib)["solve_workspace_bytes"] == 0  # released with the handle
    for norm in ("1", "I"):
        C.assert_rcond_within_bounds(name, norm, first[norm], on_device=1)
        C.assert_rcond_within_bounds(name, norm, host[norm], on_device=0)  # (a near-tie in argmax may pick another column: no equality)
    if name == "graded_r64":
        for norm in ("1", "I"):
            anorm, true = C.exact_norms(name, norm)
            assert 0.5 <= first[norm]["rcond"] * true * anorm <= 2.0


@pytest.mark.parametrize("name", RCOND_INPUTS)
def test_rcond_twice_gives_the_same_bits(name, monkeypatch):
    """Two consecutive calls on one handle, both norms: ainv_norm bit for bit.  The estimator's own reductions are fixed trees without
    atomics (test_vector_operator_twice_gives_the_same_bits: the operator alone), and its solves are the REPRODUCIBLE variant of the
    device-resident solve (PANGULU_HIP_SOLVE_REPRODUCIBLE: every block's contribution stored, a segment's contributions added in
    the order of the descriptor list).  The ordinary solve kernels add with floating-point atomics and do not repeat their bits:
    four repeats of one ordinary device-resident solve of x = 1/n differed from the first in 120 .. 770 entries (r64_conv10,
    r64_conv14, cr64_conv12), and with them this test failed on two to four of its seven inputs per run, by one unit in the last
    place for the double types."""
    monkeypatch.setenv("PANGULU_AMD_DEVICE_SOLVE", "1")
    h = C.open_case(name, "hip")
    try:
        first = {norm: pa.rcond(h, norm, details=True) for norm in ("1", "I")}
        second = {norm: pa.rcond(h, norm, details=True) for norm in ("1", "I")}
    finally:
        pa.pangulu_finalize(h)
    for norm in ("1", "I"):
        print("%s norm %s: ainv_norm %r then %r" % (name, norm, first[norm]["ainv_norm"], second[norm]["ainv_norm"]))
    for norm in ("1", "I"):
        assert first[norm]["on_device"] == 1
        assert second[norm]["ainv_norm"] == first[norm]["ainv_norm"], (norm, second[norm], first[norm])


def test_vector_operator_twice_gives_the_same_bits():
    """pangulu_platform_0201001_condest_vector alone on one device vector of 100 003 values (more than one grid stride of 256
    workgroups): norm, sign vector and argmax twice, every bit; the norm within n 2^-53 of numpy's sum, argmax the first maximum"""
    vtype, n = "r64", 100003
    lib = library_for("hip", vtype)
    fn = lib.pangulu_platform_0201001_condest_vector
    fn.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint16, ctypes.c_uint64,
                   ctypes.c_uint64, ctypes.POINTER(ctypes.c_void_p), ctypes.c_void_p]
    fn.restype = ctypes.c_int
    lib.pangulu_platform_0201001_solve_workspace_free.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
    lib.pangulu_platform_0201001_solve_workspace_free.restype = None
    rng = np.random.default_rng(20261021)
    x0 = rng.uniform(-1.0, 1.0, n)
    x0[[70001, 99000]] = 3.0  # two equal maxima far apart: the first one wins
    x0[5] = 0.0
    ws = ctypes.c_void_p()

    class Result(ctypes.Structure):
        _fields_ = [("norm1", ctypes.c_double), ("absmax", ctypes.c_double), ("abs_prev", ctypes.c_double), ("argmax", ctypes.c_ulonglong),
                    ("unchanged", ctypes.c_ulonglong)]

    outs = []
    try:
        for _ in range(2):
            x, save = torch.from_numpy(x0.copy()).cuda(), torch.zeros(n, dtype=torch.float64, device="cuda")
            r_arg, r_norm, r_again = Result(), Result(), Result()
            assert fn(2, x.data_ptr(), save.data_ptr(), n, 7, ctypes.byref(r_arg), 64, 128, 100, ctypes.byref(ws), None) == 1
            assert fn(1, x.data_ptr(), save.data_ptr(), n, 0, ctypes.byref(r_norm), 64, 128, 100, ctypes.byref(ws), None) == 1
            signs = x.cpu().numpy().copy()
            assert fn(1, x.data_ptr(), save.data_ptr(), n, 1, ctypes.byref(r_again), 64, 128, 100, ctypes.byref(ws), None) == 1
            assert r_norm.unchanged == 0 and r_again.unchanged == 1 and r_again.norm1 == float(n)
            assert (save.cpu().numpy() == signs).all()
            outs.append((r_arg.argmax, r_arg.absmax, r_arg.abs_prev, r_norm.norm1, signs.tobytes()))
        assert lib.pangulu_platform_0201001_get_solve_workspace_bytes() > 0
    finally:
        lib.pangulu_platform_0201001_solve_workspace_free(ctypes.byref(ws))
    assert lib.pangulu_platform_0201001_get_solve_workspace_bytes() == 0
    assert outs[0] == outs[1]
    argmax, absmax, abs_prev, norm1, signs = outs[0]
    assert (argmax, absmax, abs_prev) == (70001, 3.0, abs(x0[7]))
    total = float(np.abs(x0).sum())
    assert abs(norm1 - total) <= n * 2.0 ** -53 * total
    assert (np.frombuffer(signs) == np.where(np.signbit(x0), -1.0, 1.0)).all()


STATS_INPUTS = RCOND_INPUTS + ["cr64_rand1536", "graded_cr64", "negated", "zero_pivot", "scaled_saddle"]


def _same_but_for_the_mantissa(dev, host, n):
    for k in dev:
        if k in ("det", "det_mantissa_re", "det_mantissa_im", "log_abs_det"):
            continue
        assert dev[k] == host[k], (k, dev[k], host[k])
    (m, e), (mh, eh) = dev["det"], host["det"]
    assert e == eh and abs(m - mh) <= 4.0 * n * 2.0 ** -53 * abs(mh), (dev["det"], host["det"])
    if mh != 0:
        assert abs(dev["log_abs_det"] - host["log_abs_det"]) <= 4.0 * n * 2.0 ** -53 + 1e-15 * abs(host["log_abs_det"])
    else:
        assert dev["log_abs_det"] == host["log_abs_det"] == -math.inf


@pytest.mark.parametrize("name", STATS_INPUTS)
def test_factor_stats_on_device_records(name, monkeypatch):
    monkeypatch.setenv("PANGULU_AMD_DEVICE_SOLVE", "1")
    scaled = C.case(name)[4]
    n = C.dense(name).shape[0]
    h = C.open_case(name, "hip")
    try:
        st, sl = pa.factor_stats(h), pa.slogdet(h)
        again = pa.factor_stats(h)
        monkeypatch.setenv("PANGULU_AMD_DEVICE_SOLVE", "0")  # the host loops on the downloaded factors of the same handle
        host = pa.factor_stats(h)
        monkeypatch.setenv("PANGULU_AMD_DEVICE_SOLVE", "1")
        if name != "zero_pivot":
            C.assert_stats_match_own_factors(name, h, st, scaled=scaled)
        else:
            ref = C.factors_reference(h)
            assert (st["entries"], st["max_abs_l"], st["max_abs_u"]) == (ref["entries"], ref["max_abs_l"], ref["max_abs_u"])
    finally:
        pa.pangulu_finalize(h)
    assert again == st  # every bit
    _same_but_for_the_mantissa(st, host, n)
    if name == "zero_pivot":
        assert st["clamped_pivots"] == 1 and st["min_abs_pivot"] == 0.0 and st["min_pivot_index"] == 21
        assert st["log_abs_det"] == -math.inf and st["det"] == (0.0, 0) and sl == (0.0, -math.inf)
        return
    C.assert_determinant_matches_numpy(name, st, sl)
    assert st["nonfinite_entries"] == 0 and st["clamped_pivots"] == 0
    if name == "negated":
        assert sl[0] == -1.0


def test_zero_pivot_rcond_terminates(monkeypatch):
    monkeypatch.setenv("PANGULU_AMD_DEVICE_SOLVE", "1")
    h = C.open_case("zero_pivot", "hip")
    try:
        d = pa.rcond(h, "1", details=True)
    finally:
        pa.pangulu_finalize(h)
    assert d["on_device"] == 1 and 0.0 <= d["rcond"] <= 1e-15 and d["solves"] <= 12, d


class _Partial(ctypes.Structure):
    """pangulu_factor_stats_partial_t (include/pangulu_platform.h)"""
    _fields_ = [("max_re", ctypes.c_double), ("max_im", ctypes.c_double), ("nonfinite", ctypes.c_ulonglong), ("entries", ctypes.c_ulonglong),
                ("minp_re", ctypes.c_double), ("minp_im", ctypes.c_double), ("minp_row", ctypes.c_ulonglong),
                ("maxp_re", ctypes.c_double), ("maxp_im", ctypes.c_double), ("clamped", ctypes.c_ulonglong), ("pivots", ctypes.c_ulonglong),
                ("prod_re", ctypes.c_double), ("prod_im", ctypes.c_double), ("prod_exp", ctypes.c_longlong)]


def test_operator_on_hand_built_slots():
    """pangulu_platform_0201001_factor_stats called as a reference host would call it: the factors of conv(6) at nb = 16 as hand-made
    slots, one record emptied, a padding mask over two rows, against numpy on the same records"""
    nb, vtype = 16, "r64"
    lib = library_for("hip", vtype)
    recs, perm = slots.exported_records(C.conv(6), nb, vtype, factorise=True)
    recs = [list(r) for r in recs]
    off = next(i for i, r in enumerate(recs) if r[0] != r[1])
    recs[off][3] = np.zeros(nb + 1, np.uint32)  # an off-diagonal record without entries
    recs[off][4], recs[off][5] = np.zeros(0, np.uint16), np.zeros(0, np.float64)
    bm = slots.BlockMatrix([tuple(r) for r in recs], nb, np.float64, hip_lib=lib)
    try:
        blocks = list(bm.blocks.values())
        nblk = len(blocks)
        xlen = bm.nblk * nb
        pad = np.zeros(xlen, np.uint8)
        pad[[3, nb + 7]] = 1
        arr = (ctypes.c_void_p * nblk)(*[b.addr() for b in blocks])
        upper = (ctypes.c_int * nblk)(*[1 if (b.brow == b.bcol and b.is_upper) else 0 for b in blocks])
        out = (_Partial * nblk)()
        fn = lib.pangulu_platform_0201001_factor_stats
        fn.argtypes = [ctypes.c_uint16, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
        fn.restype = ctypes.c_int
        assert fn(nb, nblk, arr, upper, pad.ctypes.data_as(ctypes.c_void_p), xlen, out) == 0
        out2 = (_Partial * nblk)()
        assert fn(nb, nblk, arr, upper, pad.ctypes.data_as(ctypes.c_void_p), xlen, out2) == 0
        assert bytes(out) == bytes(out2)
    finally:
        bm.free()
    empties = 0
    for b, o in zip(blocks, out):
        va = np.asarray(b.values)
        assert o.entries == len(va) and o.nonfinite == 0
        if len(va) == 0:
            empties += 1
            assert (o.max_re, o.max_im) == (0.0, 0.0)
        else:
            assert abs(o.max_re) == np.abs(va).max() and o.max_im == 0.0
        if not (b.brow == b.bcol and b.is_upper):
            assert (o.pivots, o.clamped, o.minp_row, o.prod_re, o.prod_im, o.prod_exp) == (0, 0, 2 ** 64 - 1, 0.5, 0.0, 1)
            continue
        cp = np.asarray(b.colptr).astype(np.int64)
        rows = [r for r in range(nb) if cp[r + 1] > cp[r] and not pad[b.brow * nb + r]]
        piv = va[cp[rows]]
        assert o.pivots == len(rows) and o.clamped == 0
        assert abs(o.minp_re) == np.abs(piv).min() and abs(o.maxp_re) == np.abs(piv).max()
        assert o.minp_row == b.brow * nb + rows[int(np.argmin(np.abs(piv)))]
        m, e = C.frexp_product(piv)
        assert o.prod_exp == e and abs(o.prod_re - m) <= 4.0 * nb * 2.0 ** -53 * abs(m) and o.prod_im == 0.0
    assert empties == 1


def test_new_factors_after_a_second_gstrf(monkeypatch):
    """update_values + gstrf on the same handle: both calls describe the NEW factors (the cached device state was dropped)"""
    monkeypatch.setenv("PANGULU_AMD_DEVICE_SOLVE", "1")
    name = "r64_conv10"
    (n, cp, ri, va, coords) = C.case(name)[0]
    h = C.open_case(name, "hip")
    try:
        d1, st1 = pa.rcond(h, "1", details=True), pa.factor_stats(h)
        pa.update_values(h, 2.0 * va)
        assert pa.hip_memory(h)["solve_workspace_bytes"] == 0
        pa.pangulu_gstrf(h)
        d2, st2 = pa.rcond(h, "1", details=True), pa.factor_stats(h)
        C.assert_stats_match_own_factors(name, h, st2)  # (against the handle's factors as they are now)
    finally:
        pa.pangulu_finalize(h)
    C.assert_rcond_within_bounds(name, "1", d1, on_device=1)
    assert d2["on_device"] == 1 and d2["anorm"] == 2.0 * d1["anorm"]
    true = C.exact_norms(name, "1")[1] / 2.0
    assert 0.5 * true <= d2["ainv_norm"] <= true * (1.0 + n * C.TOL["r64"])
    assert abs(st2["log_abs_det"] - st1["log_abs_det"] - n * math.log(2.0)) <= n * C.TOL["r64"]
    assert st2["max_abs_u"] == 2.0 * st1["max_abs_u"] and st2["max_abs_pivot"] == 2.0 * st1["max_abs_pivot"]
