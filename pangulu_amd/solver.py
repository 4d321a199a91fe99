"""Python mirror of the solver API: same call sequence and argument meaning as include/pangulu.h.

    h = pangulu_init(n, nnz, colptr, rowidx, value, nb=256)     # reorder + symbolic + block records + upload
    pangulu_gstrf(h)                                            # numeric LU on the GPU (the hot path)
    x = pangulu_gstrs(h, b)                                     # triangular solves
    pangulu_finalize(h)

(reference: src/pangulu.c:11-345, driver examples/example.c:282-300).  This is a binding, not an
implementation: every call goes through the C-ABI of libpangulu_amd_<type>.so.
"""
import ctypes
import sys

import numpy as np

from . import _lib


class Handle:
    """Opaque solver handle (the reference's ``void *pangulu_handle``) plus the arrays that must outlive it."""

    def __init__(self, lib, vtype):
        self.lib = lib
        self.vtype = vtype
        self.dtype = _lib.VALUE_TYPES[vtype][0]
        self.ptr = ctypes.c_void_p(None)
        self.n = 0
        self._keep = []

    @property
    def ref(self):
        return ctypes.byref(self.ptr)

    def info(self):
        out = _lib.Info()
        self.lib.pangulu_amd_get_info(self.ref, ctypes.byref(out))
        return out.as_dict()


def _as(arr, dtype):
    a = np.ascontiguousarray(arr, dtype=dtype)
    return a


def pangulu_init(n, nnz, csc_colptr, csc_rowidx, csc_value, nb=256, nthread=1, vtype="r64",
                 ordering=None, coords=None, user_perm=None, recv_buffer_level=0.5, eager_host_mirror=False, lib=None, scaling=False):
    """CSC input with 64-bit column pointers and 32-bit row indices, as the reference (src/pangulu_common.h:67-70).

    ordering: None/"nd" (built-in nested dissection, geometric when ``coords`` is given), "identity" (what the
    reference does when built without METIS/MC64) or "user" with ``user_perm`` (perm[new] = old).
    On ranks other than 0 the matrix arguments may be None (rank 0 broadcasts them, as examples/example.c does).
    """
    lib = lib or _lib.load(vtype)  # (tests pass the checker's build of the library, _lib.load(vtype, test_hooks=True))
    h = Handle(lib, vtype)
    dtype, sizeof_value, is_complex = _lib.VALUE_TYPES[vtype]
    if ordering in (None, "nd"):
        lib.pangulu_amd_set_ordering(_lib.ORDER_ND)
    elif ordering == "identity":
        lib.pangulu_amd_set_ordering(_lib.ORDER_IDENTITY)
    elif ordering == "user":
        p = _as(user_perm, np.uint32)
        lib.pangulu_amd_set_user_perm(p.ctypes.data_as(ctypes.c_void_p), len(p))
    else:
        raise ValueError("unknown ordering %r" % (ordering,))
    if coords is not None:
        c = _as(coords, np.float64)
        lib.pangulu_amd_set_coordinates(c.ctypes.data_as(ctypes.c_void_p), c.shape[0], c.shape[1])
    lib.pangulu_amd_set_eager_host_mirror(1 if eager_host_mirror else 0)
    lib.pangulu_amd_set_scaling(1 if scaling else 0)  # maximum-product matching + scaling before the ordering (MC64's job)
    opt = _lib.InitOptions()
    opt.nthread = nthread
    opt.nb = nb
    opt.gpu_kernel_warp_per_block = 4
    opt.gpu_data_move_warp_per_block = 4
    opt.sizeof_value = sizeof_value
    opt.is_complex_matrix = is_complex
    opt.mpi_recv_buffer_level = recv_buffer_level
    if csc_colptr is not None:
        cp = _as(csc_colptr, np.uint64)
        ri = _as(csc_rowidx, np.uint32)
        va = _as(csc_value, dtype)
        h._keep = [cp, ri, va]
        args = (cp.ctypes.data_as(ctypes.c_void_p), ri.ctypes.data_as(ctypes.c_void_p), va.ctypes.data_as(ctypes.c_void_p))
    else:
        args = (None, None, None)
    lib.pangulu_init(n, nnz, args[0], args[1], args[2], ctypes.byref(opt), h.ref)
    h.n = int(h.info()["n"])
    return h


def pangulu_gstrf(h):
    opt = _lib.GstrfOptions()
    h.lib.pangulu_gstrf(ctypes.byref(opt), h.ref)


TRANS = {"N": 0, "T": 1, "H": 2}  # PANGULU_AMD_TRANS_*


def _trans_code(trans):
    if trans not in TRANS:
        raise ValueError("trans must be 'N', 'T' or 'H', got %r" % (trans,))
    return TRANS[trans]


_GSTRS_ERRORS = {1: "the handle has not been factorised", 2: "bad rhs / ldb", 3: "unknown trans", 4: "no device-resident path"}


def _torch_if_tensor(x):
    """The torch module if x is a torch.Tensor, else None.  torch is not imported for the question: whoever holds a tensor has
    imported it already."""
    if x is None or isinstance(x, (np.ndarray, list, tuple)):
        return None
    torch = sys.modules.get("torch")
    return torch if torch is not None and isinstance(x, torch.Tensor) else None


def _gstrs_torch(torch, h, T, code, trans):
    """pangulu_gstrs / pangulu_gstrs_multi for a torch tensor of shape (n,) or (n, nrhs); returns a new tensor on T's device.

    On the device the factors are on, nothing passes through the host: the columns are solved in place in a column-major copy by
    pangulu_amd_gstrs_device, ordered behind torch's current stream.  Where that call has no device-resident path for the handle
    (return code 4) and for a CPU tensor the numpy path runs on a host copy."""
    want = getattr(torch, np.dtype(h.dtype).name)
    if T.dtype != want:
        raise TypeError("the handle solves %s systems, the tensor holds %s" % (want, T.dtype))
    if T.ndim not in (1, 2) or T.shape[0] != h.n:
        raise ValueError("a tensor of shape (%d,) or (%d, nrhs) is expected, got %r" % (h.n, h.n, tuple(T.shape)))
    M = T.detach()
    M = M.reshape(h.n, 1) if M.ndim == 1 else M
    nrhs = int(M.shape[1])
    if M.is_cuda:
        # column-major with columns h.n apart: one clone() of an input that is laid out that way already, one strided copy otherwise
        if nrhs > 0 and M.stride() == (1, h.n):
            X = M.clone()
        else:
            X = torch.empty((nrhs, h.n), dtype=want, device=M.device).t()
            X.copy_(M)
        opt = _lib.GstrsOptions()
        with torch.cuda.device(M.device):
            stream = torch.cuda.current_stream().cuda_stream
        rc = h.lib.pangulu_amd_gstrs_device(ctypes.c_void_p(X.data_ptr() if nrhs else None), nrhs, h.n, code, ctypes.c_void_p(stream),
                                            ctypes.byref(opt), h.ref)
        if rc == 2:
            raise ValueError("the tensor is on %s, not on the device the factors are on" % (M.device,))
        if rc not in (0, 4):
            raise RuntimeError("pangulu_amd_gstrs_device failed (%d): %s" % (rc, _GSTRS_ERRORS.get(rc, "?")))
        if rc == 4:  # no device-resident path for this handle: through the host
            X = torch.from_numpy(pangulu_gstrs_multi(h, M.cpu().numpy(), trans=trans)).to(M.device)
    else:
        X = torch.from_numpy(pangulu_gstrs_multi(h, M.numpy(), trans=trans))
    return X.reshape(h.n) if T.ndim == 1 else X


def pangulu_gstrs(h, rhs, trans="N"):
    """Solves A x = rhs (trans="N"), A^T x = rhs ("T") or A^H x = rhs ("H") with the factors; returns x (rank 0; other ranks get
    their input back).  rhs: anything numpy takes, or a torch tensor (see pangulu_gstrs_multi)."""
    code = _trans_code(trans)
    torch = _torch_if_tensor(rhs)
    if torch is not None:
        if rhs.ndim != 1:
            raise ValueError("rhs must have shape (%d,), got %r" % (h.n, tuple(rhs.shape)))
        return _gstrs_torch(torch, h, rhs, code, trans)
    opt = _lib.GstrsOptions()
    x = np.array(rhs, dtype=h.dtype, copy=True) if rhs is not None else np.zeros(h.n, dtype=h.dtype)
    if code == 0:
        h.lib.pangulu_gstrs(x.ctypes.data_as(ctypes.c_void_p), ctypes.byref(opt), h.ref)
        return x
    rc = h.lib.pangulu_amd_gstrs_trans(x.ctypes.data_as(ctypes.c_void_p), 1, h.n, code, ctypes.byref(opt), h.ref)
    if rc != 0:
        raise RuntimeError("pangulu_amd_gstrs_trans failed (%d): %s" % (rc, _GSTRS_ERRORS.get(rc, "?")))
    return x


def pangulu_gstrs_multi(h, B, nrhs=None, trans="N"):
    """Solves A X = B (trans="N"), A^T X = B ("T") or A^H X = B ("H") for all columns of B, shape (n, nrhs) in any memory order, with
    one pass over the factors per panel of columns (pangulu_amd_gstrs_multi / pangulu_amd_gstrs_trans); returns X of the same shape
    (rank 0).  Other ranks pass None and nrhs, and "N" exactly where rank 0 does (it selects the entry point; between "T" and "H"
    rank 0 decides).

    B may be a torch tensor of the handle's dtype, shape (n, nrhs) (one rank): the result is a new tensor on the same device and the
    input is not modified.  A tensor on the device the factors are on is solved there, behind torch's current stream, without a copy
    to the host (pangulu_amd_gstrs_device; the result is column-major); a CPU tensor takes the numpy path."""
    code = _trans_code(trans)
    torch = _torch_if_tensor(B)
    if torch is not None:
        if B.ndim != 2:
            raise ValueError("B must have shape (%d, nrhs), got %r" % (h.n, tuple(B.shape)))
        return _gstrs_torch(torch, h, B, code, trans)
    opt = _lib.GstrsOptions()
    if B is not None:
        B = np.asarray(B)
        if B.ndim != 2 or B.shape[0] != h.n:
            raise ValueError("B must have shape (%d, nrhs), got %r" % (h.n, B.shape))
        x = np.array(B, dtype=h.dtype, order="F", copy=True)  # column j at x + j * n
        nrhs = B.shape[1]
        ptr = x.ctypes.data_as(ctypes.c_void_p)
    else:
        x, ptr = None, None
    if code != 0:
        rc = h.lib.pangulu_amd_gstrs_trans(ptr, int(nrhs), h.n, code, ctypes.byref(opt), h.ref)
        if rc != 0:
            raise RuntimeError("pangulu_amd_gstrs_trans failed (%d): %s" % (rc, _GSTRS_ERRORS.get(rc, "?")))
        return x
    rc = h.lib.pangulu_amd_gstrs_multi(ptr, int(nrhs), h.n, ctypes.byref(opt), h.ref)
    if rc != 0:
        raise RuntimeError("pangulu_amd_gstrs_multi failed (%d): %s" % (rc, "the handle has not been factorised" if rc == 1 else "bad rhs / ldb"))
    return x


def last_solve_path(h):
    """What the last pangulu_gstrs_multi (or transposed solve) on this handle did: columns swept on the device (0: host sweep), the widest panel, the
    number of panels."""
    d, w, p = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    h.lib.pangulu_amd_last_solve_path(h.ref, ctypes.byref(d), ctypes.byref(w), ctypes.byref(p))
    return {"device_columns": int(d.value), "panel_width": int(w.value), "panels": int(p.value)}


def pangulu_gssv(h, rhs):
    pangulu_gstrf(h)
    return pangulu_gstrs(h, rhs)


def pangulu_finalize(h):
    if h.ptr:
        h.lib.pangulu_finalize(h.ref)
    h.ptr = ctypes.c_void_p(None)


# ---- introspection used by tests and bench.py ------------------------------------------------------------------

def owned_blocks(h):
    """Yields (brow, bcol, is_upper, colptr, rowidx, values) for every block record this rank owns.

    For is_upper == 1 diagonal halves colptr/rowidx are the CSR row pointer / column index."""
    nb = int(h.info()["nb"])
    cnt = h.lib.pangulu_amd_owned_block_count(h.ref)
    for i in range(cnt):
        brow, bcol = ctypes.c_uint32(), ctypes.c_uint32()
        up, nnz = ctypes.c_int(), ctypes.c_ulonglong()
        cp, ri, va = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        rc = h.lib.pangulu_amd_owned_block(h.ref, i, ctypes.byref(brow), ctypes.byref(bcol), ctypes.byref(up), ctypes.byref(nnz),
                                           ctypes.byref(cp), ctypes.byref(ri), ctypes.byref(va))
        assert rc == 0
        k = int(nnz.value)
        colptr = np.ctypeslib.as_array(ctypes.cast(cp, ctypes.POINTER(ctypes.c_uint32)), shape=(nb + 1,)).copy()
        if k:
            rowidx = np.ctypeslib.as_array(ctypes.cast(ri, ctypes.POINTER(ctypes.c_uint16)), shape=(k,)).copy()
            raw = np.ctypeslib.as_array(ctypes.cast(va, ctypes.POINTER(ctypes.c_uint8)), shape=(k * np.dtype(h.dtype).itemsize,))
            values = raw.view(h.dtype).copy()
        else:
            rowidx = np.zeros(0, np.uint16)
            values = np.zeros(0, h.dtype)
        yield int(brow.value), int(bcol.value), int(up.value), colptr, rowidx, values


def permutation(h):
    p = h.lib.pangulu_amd_get_perm(h.ref)
    return np.ctypeslib.as_array(p, shape=(int(h.info()["n_padded"]),)).copy()


def factors_as_scipy(h):
    """Assemble L (unit lower) and U from this rank's blocks as scipy CSC matrices in the PERMUTED ordering
    (order n_padded: a block-aligned dissection adds isolated unit rows, see pangulu_amd_ext.h)."""
    import scipy.sparse as sp

    info = h.info()
    nb, n = int(info["nb"]), int(info["n_padded"])
    npad = int(info["block_length"]) * nb
    rows_l, cols_l, vals_l, rows_u, cols_u, vals_u = [], [], [], [], [], []
    for brow, bcol, up, cp, ri, va in owned_blocks(h):
        major = np.repeat(np.arange(nb, dtype=np.int64), np.diff(cp.astype(np.int64)))
        minor = ri.astype(np.int64)
        if brow == bcol and up:
            r, c = major + brow * nb, minor + bcol * nb  # CSR
            rows_u.append(r), cols_u.append(c), vals_u.append(va)
        elif brow < bcol:
            r, c = minor + brow * nb, major + bcol * nb
            rows_u.append(r), cols_u.append(c), vals_u.append(va)
        else:
            r, c = minor + brow * nb, major + bcol * nb
            rows_l.append(r), cols_l.append(c), vals_l.append(va)

    def build(rows, cols, vals):
        if not rows:
            return sp.csc_matrix((npad, npad), dtype=h.dtype)
        return sp.csc_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(npad, npad))

    L = build(rows_l, cols_l, vals_l)[:n, :n] + sp.identity(n, dtype=h.dtype, format="csc")
    U = build(rows_u, cols_u, vals_u)[:n, :n]
    return L.tocsc(), U.tocsc()


def _update_values_torch(torch, h, T):
    """update_values for a torch tensor of nnz values.  Where pangulu_amd_update_values_device has no path for the handle (return
    code 4: several ranks) the values are staged through the host."""
    want = getattr(torch, np.dtype(h.dtype).name)
    if T.dtype != want:
        raise TypeError("the handle holds %s values, the tensor holds %s" % (want, T.dtype))
    nnz = int(h.info()["nnz"])
    if T.ndim != 1 or T.shape[0] != nnz:
        raise ValueError("a tensor of shape (%d,) is expected, got %r" % (nnz, tuple(T.shape)))
    V = T.detach()
    if not V.is_cuda:
        return update_values(h, V.numpy())
    V = V.contiguous()
    with torch.cuda.device(V.device):
        stream = torch.cuda.current_stream().cuda_stream
    rc = h.lib.pangulu_amd_update_values_device(h.ref, ctypes.c_void_p(V.data_ptr()), ctypes.c_void_p(stream))
    if rc == 2:
        raise ValueError("the tensor is on %s, not on the device the records are on" % (V.device,))
    if rc == 4:
        return update_values(h, V.cpu().numpy())
    if rc != 0:
        raise RuntimeError("pangulu_amd_update_values_device failed (%d)" % rc)


def update_values(h, csc_value):
    """New values on the pattern the handle was initialised with (same order as the csc_rowidx given to pangulu_init; rank 0):
    the next pangulu_gstrf factorises the new matrix, re-using ordering, symbolic factorisation, records and -- on one rank --
    the recorded launch schedule.

    csc_value may be a torch tensor of the handle's dtype holding the nnz values (one rank).  A tensor on the device the records are
    on is taken from there, behind torch's current stream, by pangulu_amd_update_values_device: only the nnz values cross the host
    link, not the records.  A CPU tensor takes the numpy path."""
    torch = _torch_if_tensor(csc_value)
    if torch is not None:
        return _update_values_torch(torch, h, csc_value)
    if csc_value is not None:
        va = np.ascontiguousarray(csc_value, dtype=h.dtype)  # (alive until the call returns: the library copies the values)
        ptr = va.ctypes.data_as(ctypes.c_void_p)
    else:
        ptr = None
    rc = h.lib.pangulu_amd_update_values(h.ref, ptr)
    if rc != 0:
        raise RuntimeError("pangulu_amd_update_values failed (%d)" % rc)


def factor_check(h):
    """||L(U 1) - A 1||_2 / ||A 1||_2 on the factors where they are (the reference's pangulu_numeric_check,
    src/pangulu_numeric.c:1082-1341); collective over the ranks."""
    out = ctypes.c_double(0.0)
    rc = h.lib.pangulu_amd_factor_check(h.ref, ctypes.byref(out))
    if rc != 0:
        raise RuntimeError("pangulu_amd_factor_check: the handle has not been factorised")
    return float(out.value)


def factor_check_vectors(h, nvec=8, seed=20251003):
    """The factor check on the all-ones vector and nvec - 1 seeded random +-1 vectors: the largest quotient (collective)."""
    out = ctypes.c_double(0.0)
    rc = h.lib.pangulu_amd_factor_check_vectors(h.ref, int(nvec), int(seed), ctypes.byref(out))
    if rc != 0:
        raise RuntimeError("pangulu_amd_factor_check_vectors: the handle has not been factorised")
    return float(out.value)


def factor_stats(h):
    """pangulu_amd_factor_stats as a dict of the struct's fields plus "det": (mantissa, exponent) with det(A) = mantissa * 2**exponent
    (a complex mantissa for complex value types); collective over the ranks."""
    st = _lib.FactorStats()
    rc = h.lib.pangulu_amd_factor_stats(h.ref, ctypes.byref(st))
    if rc != 0:
        raise RuntimeError("pangulu_amd_factor_stats: the handle has not been factorised")
    out = st.as_dict()
    cplx = np.issubdtype(np.dtype(h.dtype), np.complexfloating)
    mant = complex(st.det_mantissa_re, st.det_mantissa_im) if cplx else float(st.det_mantissa_re)
    out["det"] = (mant, int(st.det_exponent))
    return out


def slogdet(h):
    """(sign, log|det(A)|) of the user's matrix from the factors, with numpy.linalg.slogdet's conventions: sign is +-1 (a complex
    number of modulus 1 for complex value types), and (0, -inf) for a zero determinant."""
    st = factor_stats(h)
    mant, _ = st["det"]
    if mant == 0:
        return (0j if isinstance(mant, complex) else 0.0), -np.inf
    sign = mant / abs(mant)
    return sign, float(st["log_abs_det"])


def rcond(h, norm="1", details=False):
    """pangulu_amd_rcond: the estimated reciprocal condition number of the user's matrix in the 1-norm ("1", "O") or the infinity
    norm ("I"); with details a dict of rcond, anorm, ainv_norm, solves and on_device.  Collective over the ranks."""
    key = str(norm).upper()
    if key in ("1", "O"):
        code = _lib.NORM_ONE
    elif key == "I":
        code = _lib.NORM_INF
    else:
        raise ValueError("norm must be '1' or 'I', not %r" % (norm,))
    rc_, an, ai = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
    ns, dev = ctypes.c_int(), ctypes.c_int()
    rc = h.lib.pangulu_amd_rcond(code, ctypes.byref(rc_), ctypes.byref(an), ctypes.byref(ai), ctypes.byref(ns), ctypes.byref(dev), h.ref)
    if rc != 0:
        raise RuntimeError("pangulu_amd_rcond failed (%d): %s" % (rc, "the handle has not been factorised" if rc == 1 else "unknown norm"))
    if not details:
        return float(rc_.value)
    return {"rcond": float(rc_.value), "anorm": float(an.value), "ainv_norm": float(ai.value), "solves": int(ns.value), "on_device": int(dev.value)}


MODEL_FIELDS = ("T_star_s", "sum_over_ranks_s", "link_term_s_max", "sent_bytes", "critical_path_s", "latency_chain_s", "rank_flop_share",
                "rank_T_star_share", "hbm_bytes_fullest_rank", "hbm_records_owned", "hbm_records_received", "hbm_dense_mirrors")


def model_for_ranks(h, nranks):
    """The structure-only model of this handle's factorisation on `nranks` ranks (pangulu_amd_model_for_ranks): a dict of
    MODEL_FIELDS, or None when the model is not available."""
    out = (ctypes.c_double * 12)()
    if h.lib.pangulu_amd_model_for_ranks(h.ref, int(nranks), out) != 0:
        return None
    return dict(zip(MODEL_FIELDS, (float(x) for x in out)))


def hip_memory(h_or_lib):
    """Device memory the back-end holds for itself (bytes): mirror pool, descriptor twins of a recorded schedule, GETRF scratch,
    the workspaces of device-resident solves, the maps of update_values from device memory; and the number of blocks in dense mode."""
    lib = h_or_lib.lib if isinstance(h_or_lib, Handle) else h_or_lib
    v = (ctypes.c_ulonglong * 4)()
    lib.pangulu_platform_0201001_get_memory(v)
    return {"mirror_pool_bytes": int(v[0]), "schedule_descriptor_bytes": int(v[1]), "getrf_scratch_bytes": int(v[2]), "dense_mode_blocks": int(v[3]),
            "solve_workspace_bytes": int(lib.pangulu_platform_0201001_get_solve_workspace_bytes()),
            "values_refresh_bytes": int(lib.pangulu_platform_0201001_get_values_refresh_bytes())}


def hip_stats(h_or_lib, reset=False):
    lib = h_or_lib.lib if isinstance(h_or_lib, Handle) else h_or_lib
    st = _lib.HipStats()
    lib.pangulu_platform_0201001_get_stats(ctypes.byref(st), 1 if reset else 0)
    out = {}
    for k, name in _lib.KERNEL_CLASSES.items():
        out[name] = dict(launches=int(st.launches[k]), tasks=int(st.tasks[k]), alg_bytes=float(st.alg_bytes[k]),
                         flops=float(st.flops[k]), elapsed_ms=float(st.elapsed_ms[k]))
    out["ssssm_dense_mfma"]["mfma_flops_executed"] = float(st.mfma_flops_executed)
    out["tstrf"]["dense_path_tasks"] = int(st.trsm_dense_tasks)  # TSTRF + GESSM tasks solved on the matrix cores
    out["ssssm_dense_mfma"]["front_workgroups"] = int(st.ssssm_front_workgroups)      # dense-front kernel (pg_hip_front.h)
    out["ssssm_dense_mfma"]["general_workgroups"] = int(st.ssssm_general_workgroups)  # general MFMA kernel (pg_hip_dense.h)
    # class 5 by kernel: time of each kernel's launches (PROFILE on) and the flops its 16 x 16 x 16 products executed (COUNT_FLOPS on)
    out["ssssm_dense_mfma"]["front_kernel_ms"] = float(st.ssssm_kernel_ms[0])
    out["ssssm_dense_mfma"]["general_kernel_ms"] = float(st.ssssm_kernel_ms[1])
    out["ssssm_dense_mfma"]["front_flops_executed"] = float(st.ssssm_front_flops_executed)
    out["getrf"]["chase_launches"] = int(st.chase_launches)  # launches that carried a level's factorisations and its dense solves
    out["tstrf"]["chase_solves"] = int(st.chase_solves)
    return out
