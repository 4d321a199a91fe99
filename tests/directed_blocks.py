"""Directed inputs for the dense-mode kernels: matrices whose block records are DESIGNED (through the identity ordering matrix
block (I,J) is block record (I,J)), an extended-precision dense LU as the reference, and an entry-wise bound.

Plain numpy; nothing here needs a GPU.  tests/test_directed_blocks_cpu.py pins the designs and the reference on the oracle,
tests/test_gpu_directed_blocks.py runs the same cases through the HIP kernels.

The bound (componentwise_check): for a no-pivot LU computed in ANY summation order with unit round-off u,
|L U - A| <= gamma_n |L||U| entry-wise, gamma_n = n u / (1 - n u) (Higham, Accuracy and Stability of Numerical Algorithms,
theorem 9.3).  The dense solves multiply by inverted 16 x 16 diagonal tiles instead of substituting, which costs a factor of the
tile's condition number; c = max(1, largest kappa_inf of the 16 x 16 diagonal tiles of the reference's L and U) pays for it.
"""
import zlib

import numpy as np

TILE = 16
TOL = 1e-16  # PANGULU_TOL: |Re p| < TOL -> the divisor is +TOL (oracle/pangulu_oracle.c:57-75); the stored diagonal keeps its value

UNIT_ROUNDOFF = {"r64": 2.0 ** -53, "cr64": 2.0 ** -53, "r32": 2.0 ** -24, "cr32": 2.0 ** -24}
DTYPES = {"r64": np.float64, "cr64": np.complex128, "r32": np.float32, "cr32": np.complex64}


def _extended(vtype_or_dtype):
    assert np.finfo(np.longdouble).nmant >= 63, "np.longdouble is no extended type here (nmant = %d): the reference would be no reference" % np.finfo(np.longdouble).nmant
    dt = np.dtype(DTYPES.get(vtype_or_dtype, vtype_or_dtype))
    return np.clongdouble if dt.kind == "c" else np.longdouble


# ---------------------------------------------------------------------------------------------------------------------
# tile patterns: boolean nb x nb masks of the entries a block holds
# ---------------------------------------------------------------------------------------------------------------------
def _tiles(nb, tiles):
    m = np.zeros((nb, nb), bool)
    for ti, tj in tiles:
        m[ti * TILE:(ti + 1) * TILE, tj * TILE:(tj + 1) * TILE] = True
    return m


def corner_entries(nb):
    """Single entries at tile corners: first / last entry of the block, both sides of the first tile border."""
    return [(0, 0), (15, 15), (16, 16), (15, 16), (nb - 1, 0), (0, nb - 1), (nb - 1, nb - 1)]


def pattern_mask(name, nb):
    """Off-diagonal patterns.  Tile indices are taken modulo the tile count, so (9,12) is tile (1,4) at nb = 128."""
    nt = nb // TILE
    if name == "empty":
        return np.zeros((nb, nb), bool)
    if name == "corners":
        m = np.zeros((nb, nb), bool)
        for i, j in corner_entries(nb):
            m[i, j] = True
        return m
    if name == "tile_1_2":     # the pipe GETRF's band region at nb = 256 (min(i,j) < 4)
        return _tiles(nb, [(1, 2)])
    if name == "tile_9_12":    # ... its resident region
        return _tiles(nb, [(9 % nt, 12 % nt)])
    if name == "tile_row":
        return _tiles(nb, [(3, j) for j in range(nt)])
    if name == "tile_col":
        return _tiles(nb, [(i, 5) for i in range(nt)])
    if name == "checker":
        return _tiles(nb, [(i, j) for i in range(nt) for j in range(nt) if (i + j) % 2 == 0])
    if name == "full":
        return np.ones((nb, nb), bool)
    if name == "last_tile":    # the last tile alone: the "diagonal tile last" end of the ring TRSM's walk
        return _tiles(nb, [(nt - 1, nt - 1)])
    raise KeyError(name)


def diagonal_mask(name, nb):
    """Diagonal block shapes; "diagtiles+<pattern>" adds an off-diagonal pattern to the 16 diagonal tiles."""
    nt = nb // TILE
    i, j = np.indices((nb, nb))
    if name == "identity":
        return i == j
    if name == "diagtiles":    # no panel or strip tile live at any step
        return _tiles(nb, [(t, t) for t in range(nt)])
    if name == "band17":       # half-width 17: crosses every tile border
        return abs(i - j) <= 17
    if name == "arrow":        # dense last tile row and column
        return _tiles(nb, [(t, t) for t in range(nt)] + [(nt - 1, t) for t in range(nt)] + [(t, nt - 1) for t in range(nt)])
    if name == "dense":
        return np.ones((nb, nb), bool)
    if name.startswith("diagtiles+"):
        return diagonal_mask("diagtiles", nb) | pattern_mask(name[len("diagtiles+"):], nb)
    raise KeyError(name)


# ---------------------------------------------------------------------------------------------------------------------
# the builder
# ---------------------------------------------------------------------------------------------------------------------
def _pack(A, mask, dtype):
    """CSC tuple with every masked entry STORED (explicit zeros included)."""
    n = A.shape[0]
    rows, cols = np.nonzero(mask.T)  # column-major walk: cols ascending, rows ascending inside a column
    cols, rows = rows, cols
    colptr = np.zeros(n + 1, np.uint64)
    np.cumsum(np.bincount(cols, minlength=n), out=colptr[1:])
    return (n, colptr, rows.astype(np.uint32), np.ascontiguousarray(A[rows, cols], dtype=dtype), None)


def dense_of(mat):
    """The matrix as a dense array in its own type, and the mask of stored entries."""
    n, cp, ri, va, _ = mat
    cols = np.repeat(np.arange(n), np.diff(cp.astype(np.int64)))
    A = np.zeros((n, n), va.dtype)
    A[ri.astype(np.int64), cols] = va
    mask = np.zeros((n, n), bool)
    mask[ri.astype(np.int64), cols] = True
    return A, mask


def block_matrix(nb, K, diag, off, vtype="r64", seed=0, pivots=()):
    """n = K nb.  `diag`: K shape names (diagonal_mask), `off`: {(I,J): pattern name} (pattern_mask; a name ending in ".T" is the
    transposed pattern).  Values: seeded uniform in [-1,1] (both parts for complex), then every diagonal entry is set to
    2 x (the sum of the moduli of the other entries of its column) + 1 with a seeded sign / phase: the whole matrix, hence every
    diagonal tile of it and of every Schur complement, is strictly column-diagonally dominant.
    `pivots`: (d, k, p) triples -- in diagonal block d, local index k: row k of A keeps ONLY its diagonal entry, with the value p,
    and column k gets entries in every other row of its own block (above and below the diagonal) and in every third row of the
    blocks below (it is the one column that is not dominant; nothing above block d, so its inner products have at most nb terms)."""
    dtype = DTYPES[vtype]
    n = K * nb
    rng = np.random.default_rng(seed)
    mask = np.zeros((n, n), bool)
    for d, name in enumerate(diag):
        mask[d * nb:(d + 1) * nb, d * nb:(d + 1) * nb] = diagonal_mask(name, nb)
    for (I, J), name in off.items():
        assert I != J
        m = pattern_mask(name[:-2], nb).T if name.endswith(".T") else pattern_mask(name, nb)
        mask[I * nb:(I + 1) * nb, J * nb:(J + 1) * nb] = m
    glob = [d * nb + k for d, k, _ in pivots]
    for (d, k, _), g in zip(pivots, glob):
        mask[d * nb:(d + 1) * nb:2, g] = True
        mask[(d + 1) * nb::3, g] = True
    for g in glob:
        mask[g, :] = False
        mask[g, g] = True
    A = rng.uniform(-1.0, 1.0, (n, n))
    if np.dtype(dtype).kind == "c":
        A = A + 1j * rng.uniform(-1.0, 1.0, (n, n))
    A = np.where(mask, A, 0.0)
    idx = np.arange(n)
    A[idx, idx] = 0.0
    mag = 2.0 * np.abs(A).sum(axis=0) + 1.0
    if np.dtype(dtype).kind == "c":
        A[idx, idx] = mag * np.exp(1j * rng.uniform(0.0, 2.0 * np.pi, n))
    else:
        A[idx, idx] = mag * rng.choice([-1.0, 1.0], n)
    for (_, _, p), g in zip(pivots, glob):
        A[g, g] = p
    return _pack(A.astype(dtype), mask, dtype)


# ---------------------------------------------------------------------------------------------------------------------
# occupancy: which 16 x 16 tiles of the symbolic pattern hold entries
# ---------------------------------------------------------------------------------------------------------------------
def tile_occupancy_of_mask(mask):
    n = mask.shape[0]
    nt = n // TILE
    return mask.reshape(nt, TILE, nt, TILE).any(axis=(1, 3))


def symbolic_tile_occupancy(mat, nb, vtype="r64"):
    """Tile occupancy (n/16 x n/16 booleans) of the block records the HOST builds for this matrix under the identity ordering:
    patterns closed under fill.  From exported_records on the oracle platform -- no GPU."""
    from . import slots

    n = mat[0]
    mask = np.zeros((n, n), bool)
    for brow, bcol, up, cp, ri, _ in slots.exported_records(mat, nb, vtype, ordering="identity"):
        major = np.repeat(np.arange(nb, dtype=np.int64), np.diff(cp.astype(np.int64)))
        minor = ri.astype(np.int64)
        if brow == bcol and up:
            mask[major + brow * nb, minor + bcol * nb] = True  # CSR
        else:
            mask[minor + brow * nb, major + bcol * nb] = True
    mask[np.arange(n), np.arange(n)] = True
    return tile_occupancy_of_mask(mask)


def predicted_tile_occupancy(mat):
    """The same by an independent route: boolean right-looking elimination of the pattern of A + A^T (the symbolic
    factorisation works on the symmetrised pattern), entry by entry."""
    _, mask = dense_of(mat)
    m = mask | mask.T
    n = m.shape[0]
    m[np.arange(n), np.arange(n)] = True
    for k in range(n - 1):
        r = np.nonzero(m[k + 1:, k])[0] + k + 1
        if len(r):
            m[np.ix_(r, r)] = True  # symmetric pattern: row k's columns are column k's rows
    return tile_occupancy_of_mask(m)


def live_tiles_per_block(occ, nb):
    """{(I,J): number of live tiles} of a tile occupancy map."""
    nt = nb // TILE
    K = occ.shape[0] // nt
    return {(I, J): int(occ[I * nt:(I + 1) * nt, J * nt:(J + 1) * nt].sum()) for I in range(K) for J in range(K)}


# ---------------------------------------------------------------------------------------------------------------------
# the reference and the bound
# ---------------------------------------------------------------------------------------------------------------------
def clamp_divisor(p):
    """The reference's rule when DIVIDING by a pivot: |Re p| < 1e-16 -> +1e-16 (the imaginary part goes with it)."""
    p = np.asarray(p)
    tiny = np.abs(p.real) < TOL
    return np.where(tiny, p.dtype.type(TOL), p), tiny


def reference_lu(mat):
    """Dense right-looking no-pivot LU of the whole matrix in np.longdouble / np.clongdouble with the reference's clamp rule.
    Returns L (unit lower), U (the stored diagonal is NOT clamped) and the boolean vector of clamped pivots.  Rows and columns
    that are exactly zero in a step are skipped: their products are exact zeros."""
    A, _ = dense_of(mat)
    xt = _extended(A.dtype)
    W = A.astype(xt)
    n = W.shape[0]
    clamped = np.zeros(n, bool)
    for k in range(n):
        piv, tiny = clamp_divisor(W[k, k])
        clamped[k] = bool(tiny)
        r = np.nonzero(W[k + 1:, k])[0] + k + 1
        if not len(r):
            continue
        W[r, k] = W[r, k] / piv
        c = np.nonzero(W[k, k + 1:])[0] + k + 1
        if len(c):
            W[np.ix_(r, c)] -= np.outer(W[r, k], W[k, c])
    L = np.tril(W, -1)
    L[np.arange(n), np.arange(n)] = 1
    return L, np.triu(W), clamped


def matmul_ext(A, B):
    """A @ B in the extended type, 16 inner indices at a time, restricted to the rows of A and columns of B that are not exactly
    zero there (numpy has no BLAS for long double; the factors of the designed cases are mostly empty tiles)."""
    C = np.zeros((A.shape[0], B.shape[1]), np.result_type(A, B))
    for k0 in range(0, A.shape[1], TILE):
        a, b = A[:, k0:k0 + TILE], B[k0:k0 + TILE, :]
        r, c = np.nonzero(a.any(axis=1))[0], np.nonzero(b.any(axis=0))[0]
        if len(r) and len(c):
            C[np.ix_(r, c)] += a[r] @ b[:, c]
    return C


def _kappa_inf(T):
    T = T.astype(np.clongdouble if T.dtype.kind == "c" else np.longdouble)
    # 16 x 16 triangular: invert by substitution in the extended type (np.linalg has no long double)
    m = T.shape[0]
    X = np.zeros_like(T)
    upper = not np.tril(T, -1).any()
    order = range(m - 1, -1, -1) if upper else range(m)
    E = np.eye(m, dtype=T.dtype)
    for i in order:
        X[i] = (E[i] - T[i] @ X) / T[i, i]  # (X[i] is still zero, so T[i] @ X is the sum over the rows solved so far)
    return float(np.abs(T).sum(axis=1).max() * np.abs(X).sum(axis=1).max())


def tile_condition(Lref, Uref, clamped):
    """c = max(1, largest kappa_inf of the 16 x 16 diagonal tiles of the reference's L and U).
    A designed pivot index k (`clamped`: a boolean vector, the clamped pivots and the tiny ones that just escape the clamp) is taken
    out of its tiles first (row k of U becomes e_k, column k of L becomes e_k): the pivot cases give row k
    of A only its diagonal entry, so row k of U is p e_k and column k of L meets nothing but that row -- the index decouples from
    every solve, and column k of L has a bound of its own (clamp_column_check).  Left in, its 1e-16 would make c about 1e16 and the
    bound vacuous; taking it out only makes the check stricter than the plain definition."""
    n = Lref.shape[0]
    Ut = Uref.copy()
    Lt = Lref.copy()
    for k in np.nonzero(clamped)[0]:
        Ut[k, :] = 0
        Ut[k, k] = 1
        Lt[:, k] = 0
        Lt[k, k] = 1
    c = 1.0
    for t0 in range(0, n, TILE):
        s = slice(t0, t0 + TILE)
        c = max(c, _kappa_inf(Lt[s, s]), _kappa_inf(Ut[s, s]))
    return c


def componentwise_check(mat, L, U, u, c):
    """max over (i,j) of |(L U~ - A')_ij| / (c gamma_n (|L||U~|)_ij), everything in the extended type.  U~: U with the clamp rule
    applied to its diagonal, A': A with clamped diagonal entries replaced by the clamp value.  Where the denominator is 0 the
    numerator must be exactly 0 (else: inf).  `c` from tile_condition() of the reference's factors.  Passing means <= 1."""
    A, _ = dense_of(mat)
    xt = _extended(A.dtype)
    n = A.shape[0]
    L = np.asarray(L.toarray() if hasattr(L, "toarray") else L).astype(xt)
    Ut = np.asarray(U.toarray() if hasattr(U, "toarray") else U).astype(xt)
    if not (np.isfinite(L).all() and np.isfinite(Ut).all()):
        return float("inf")
    A1 = A.astype(xt)
    idx = np.arange(n)
    d, tiny = clamp_divisor(Ut[idx, idx])
    Ut[idx, idx] = d
    A1[idx[tiny], idx[tiny]] = TOL
    gamma = np.longdouble(n) * np.longdouble(u) / (1 - np.longdouble(n) * np.longdouble(u))
    num = np.abs(matmul_ext(L, Ut) - A1)
    den = np.longdouble(c) * gamma * matmul_ext(np.abs(L), np.abs(Ut))
    zero = den == 0
    if (num[zero] != 0).any():
        return float("inf")
    return float((num[~zero] / den[~zero]).max()) if (~zero).any() else 0.0


def forward_check(Lref, Uref, L, U, u, c, against=None):
    """Entry-wise forward comparison with the reference, for cases without clamped pivots.  If L^ U^ = A + E with
    |E| <= eps |L||U| entry-wise (eps = c gamma_n, what componentwise_check asserts), then (Higham, theorem 9.15)
        |dL| <= |L| stril((I - G)^-1 G),   |dU| <= triu(G (I - G)^-1) |U|,   G = eps |L^-1| |L||U| |U^-1|,
    provided the spectral radius of G is below 1.  Here n max(G) < 1/2 is asserted, so (I - G)^-1 G <= 2 G entry-wise.
    The bound itself is evaluated in float64 (it needs two correct digits, not nineteen).  Returns the worst quotient
    |computed - reference| / bound.
    `against` = (L2, U2), a second computed factorisation that meets the same backward bound: both lie within the bound of the
    reference, hence within TWICE the bound of each other; the quotient returned is then |computed - second| / (2 bound)."""
    n = Lref.shape[0]
    xt = Lref.dtype
    L = np.asarray(L.toarray() if hasattr(L, "toarray") else L).astype(xt)
    U = np.asarray(U.toarray() if hasattr(U, "toarray") else U).astype(xt)
    ft = np.complex128 if xt == np.clongdouble else np.float64
    aL, aU = np.abs(Lref).astype(np.float64), np.abs(Uref).astype(np.float64)
    Li, Ui = np.abs(np.linalg.inv(Lref.astype(ft))), np.abs(np.linalg.inv(Uref.astype(ft)))
    eps = float(c) * n * u / (1.0 - n * u)
    G = eps * (Li @ (aL @ aU) @ Ui)
    assert n * G.max() < 0.5, "the first-order perturbation bound does not apply (n max G = %g)" % (n * G.max())
    bL = aL @ np.tril(2.0 * G, -1)
    bU = np.triu(2.0 * G) @ aU
    if against is not None:
        Lref, Uref = (np.asarray(M.toarray() if hasattr(M, "toarray") else M).astype(xt) for M in against)
        bL, bU = 2.0 * bL, 2.0 * bU
    worst = 0.0
    for dif, bound in ((np.abs(U - Uref), bU), (np.abs(L - Lref), bL)):
        zero = bound == 0
        if (dif[zero] != 0).any():
            return float("inf")
        if (~zero).any():
            worst = max(worst, float((dif[~zero] / bound[~zero]).max()))
    return worst


def clamp_column_scales(mat, Lref, Uref, columns):
    """For each designed pivot column k (global index): the reference's column k of L and (|a_ik| + sum_j |L_ij||U_jk|) / 1e-16."""
    A, _ = dense_of(mat)
    xt = Lref.dtype
    out = {}
    for k in columns:
        scale = (np.abs(A[:, k].astype(xt)) + np.abs(Lref[:, :k]) @ np.abs(Uref[:k, k])) / np.longdouble(TOL)
        out[int(k)] = (Lref[:, k].copy(), scale)
    return out


def clamp_column_check(ref, L, nb, u):
    """Columns k of L below the diagonal against the reference, entry-wise:
    |L_ik - Lref_ik| <= c gamma_nb (|a_ik| + sum_j |L_ij||U_jk|) / 1e-16  -- the numerator of L_ik is an inner product of at most
    nb live terms (column k of A has nothing above its own block, so U_jk lives in the block alone), divided by the clamped pivot.
    Returns the worst quotient per column, {k: quotient}."""
    gamma = np.longdouble(nb) * np.longdouble(u) / (1 - np.longdouble(nb) * np.longdouble(u))
    out = {}
    for k, (Lcol, scale) in ref["columns"].items():
        dif = np.abs(L[k + 1:, k].astype(Lcol.dtype) - Lcol[k + 1:])
        bound = np.longdouble(ref["c"]) * gamma * scale[k + 1:]
        zero = bound == 0
        if (dif[zero] != 0).any():
            out[k] = float("inf")
        else:
            out[k] = float((dif[~zero] / bound[~zero]).max()) if (~zero).any() else 0.0
    return out


_references = {}


def reference(key, mat, pivots=(), keep_factors=False, cache_dir=None):
    """reference_lu once per case and process: {"c": tile_condition, "clamped": ..., "columns": clamp_column_scales of the designed
    pivot columns `pivots` (global indices), "L"/"U" when keep_factors}.  With `cache_dir` the small parts are kept in a file there,
    for worker processes that run the same cases."""
    import os

    if key in _references and (not keep_factors or "L" in _references[key]):
        return _references[key]
    path = os.path.join(cache_dir, "ref_%s.npz" % key) if cache_dir else None
    if path and os.path.exists(path) and not keep_factors:
        z = np.load(path)
        ref = {"c": float(z["c"]), "clamped": z["clamped"], "columns": {int(k): (z["Lcol_%d" % k], z["scale_%d" % k]) for k in z["pivots"]}}
    else:
        L, U, clamped = reference_lu(mat)
        out = clamped.copy()
        out[list(pivots)] = True
        ref = {"c": tile_condition(L, U, out), "clamped": clamped, "columns": clamp_column_scales(mat, L, U, pivots)}
        if keep_factors:
            ref["L"], ref["U"] = L, U
        if path:
            arrays = {"c": np.float64(ref["c"]), "clamped": clamped, "pivots": np.array(sorted(ref["columns"]), np.int64)}
            for k, (Lcol, scale) in ref["columns"].items():
                arrays["Lcol_%d" % k], arrays["scale_%d" % k] = Lcol, scale
            tmp = path + ".%d.tmp.npz" % os.getpid()
            np.savez(tmp, **arrays)
            os.replace(tmp, path)
    _references[key] = ref
    return ref


# ---------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------
def _sym(a, b, c):
    """Pattern a in block (1,0), b in (2,1), c in (2,0), their transposes mirrored: the symbolic factorisation symmetrises the
    pattern anyway, so a design that is not symmetric would only get the union."""
    return {(1, 0): a, (0, 1): a + ".T", (2, 1): b, (1, 2): b + ".T", (2, 0): c, (0, 2): c + ".T"}


# name -> (diagonal shapes, off-diagonal patterns).  K = 3: one factorisation runs 3 GETRF, 3 TSTRF, 3 GESSM and 5 SSSSM (two into
# block (2,2), one each into (1,1), (2,1), (1,2)) on the chosen tiles.
PATTERN_CASES = {
    # single entries; diagonal tiles only, so the solves add no fill outside the entries' tile columns / rows
    "corners": (["diagtiles", "diagtiles", "diagtiles"], _sym("corners", "corners", "corners")),
    # one full tile in the pipe GETRF's band region and one in its resident region, in the diagonal blocks AND in the panels
    "single_tiles": (["diagtiles+tile_1_2", "diagtiles+tile_9_12", "diagtiles"], _sym("tile_1_2", "tile_9_12", "last_tile")),
    "tile_row_col": (["diagtiles", "band17", "arrow"], _sym("tile_row", "tile_col", "checker")),
    "checker": (["band17", "diagtiles", "dense"], _sym("checker", "checker", "tile_1_2")),
    "arrow": (["arrow", "arrow", "arrow"], _sym("tile_col", "tile_row", "corners")),
    "dense": (["dense", "dense", "dense"], _sym("checker", "tile_col", "tile_row")),
    # every tile of every block live.  (Its updates are dense-front products, but five of them are far below the number of
    # workgroups from which the dense-front kernel gets a launch: observed front_workgroups = 0, they run on the general kernel.)
    "full": (["dense", "dense", "dense"], _sym("full", "full", "full")),
}
CR64_PATTERN_CASES = ["single_tiles", "tile_row_col"]  # a representative third, at nb = 128
R32_PATTERN_CASES = ["corners", "checker"]

# live tiles per block of the symbolic pattern AFTER fill, {nb: {case: rows of the 3 x 3 block grid}}; checked against the records
# the host builds (symbolic_tile_occupancy) and against an independent boolean elimination (predicted_tile_occupancy)
EXPECTED_LIVE_TILES = {
    128: {
        "corners": [[8, 6, 6], [6, 14, 9], [6, 9, 14]],          # the products of single entries add single entries: 6 new tiles
        "single_tiles": [[10, 1, 1], [1, 10, 1], [1, 1, 8]],     # no fill at all: (1,2)(2,1) lands on a diagonal tile
        "tile_row_col": [[8, 8, 32], [8, 34, 40], [32, 40, 64]],
        "checker": [[34, 60, 6], [60, 64, 61], [6, 61, 64]],     # the band diagonal smears the checkerboard: nearly full panels
        "arrow": [[22, 16, 7], [16, 64, 32], [7, 32, 28]],
        "dense": [[64, 60, 8], [60, 64, 29], [8, 29, 64]],
        "full": [[64, 64, 64], [64, 64, 64], [64, 64, 64]],
    },
    256: {
        "corners": [[16, 6, 6], [6, 22, 9], [6, 9, 22]],
        "single_tiles": [[18, 1, 1], [1, 18, 1], [1, 1, 16]],
        "tile_row_col": [[16, 16, 128], [16, 74, 208], [128, 208, 256]],
        "checker": [[74, 248, 14], [248, 256, 249], [14, 249, 256]],
        "arrow": [[46, 32, 7], [32, 256, 64], [7, 64, 52]],
        "dense": [[256, 248, 16], [248, 256, 181], [16, 181, 256]],
        "full": [[256, 256, 256], [256, 256, 256], [256, 256, 256]],
    },
}


def pattern_case(name, nb, vtype="r64"):
    diag, off = PATTERN_CASES[name]
    seed = 1000 + list(PATTERN_CASES).index(name)
    return block_matrix(nb, 3, diag, off, vtype=vtype, seed=seed)


CLAMP_VALUES = {
    # name: (p, clamped?)
    "3e-17": (3e-17, True),
    "-3e-17": (-3e-17, True),       # becomes PLUS 1e-16
    "zero": (0.0, True),            # an explicit stored zero
    "1e-16": (1e-16, False),        # strict <: not clamped
    "0.99e-16": (0.99e-16, True),
}
CLAMP_VALUES_COMPLEX = {
    "3e-17+2j": (3e-17 + 2j, True),   # only the real part is looked at; the imaginary part is dropped with it
    "2+3e-17j": (2 + 3e-17j, False),
}


def clamp_positions(nb, K=3):
    return [(d, k) for d in (0, K - 1) for k in (0, 15, 16, nb - 1)]


def clamp_case(name, nb, vtype="r64", K=3):
    """One matrix per pivot value: the value sits at local index k in {0, 15, 16, nb-1} of diagonal blocks 0 and K-1 -- eight pivots.
    They do not interact: row k of U is p e_k, so column k of L (the only thing the pivot scales) multiplies zeros everywhere."""
    p = (CLAMP_VALUES_COMPLEX if name in CLAMP_VALUES_COMPLEX else CLAMP_VALUES)[name][0]
    diag = ["band17", "diagtiles", "band17"]
    off = _sym("tile_col", "tile_row", "corners") if nb >= 128 else _sym("corners", "corners", "corners")
    seed = 2000 + nb + sorted(list(CLAMP_VALUES) + list(CLAMP_VALUES_COMPLEX)).index(name)
    return block_matrix(nb, K, diag, off, vtype=vtype, seed=seed, pivots=[(d, k, p) for d, k in clamp_positions(nb, K)])


# queue depth: a block arrow, K - 1 panels into the last diagonal block
ARROW_PANEL_PATTERNS = ["checker", "tile_row", "tile_col", "tile_1_2", "corners", "tile_9_12", "last_tile"]
QUEUE_DEPTHS = [1, 15, 16, 17, 33]


def arrow_case(depth, nb=128, vtype="r64", seed=3000):
    """K = depth + 1 blocks: A_kk = 2 I for k < K-1, blocks (K-1,k) and (k,K-1) hold partly live tile patterns that vary with k, the
    last diagonal block is dense.  Then L_{K-1,k} = A_{K-1,k} / 2 and U_{k,K-1} = A_{k,K-1} exactly, and the last block factorises
    S = A_{K-1,K-1} - sum_k L_{K-1,k} U_{k,K-1}.  Returns the matrix and S in the extended type."""
    K = depth + 1
    off = {}
    for k in range(depth):
        off[(K - 1, k)] = ARROW_PANEL_PATTERNS[k % len(ARROW_PANEL_PATTERNS)]
        off[(k, K - 1)] = ARROW_PANEL_PATTERNS[(k + 3) % len(ARROW_PANEL_PATTERNS)]
    mat = block_matrix(nb, K, ["identity"] * depth + ["dense"], off, vtype=vtype, seed=seed + depth)
    # the builder made the diagonal dominant; the leading diagonal blocks become exactly 2 I
    n, cp, ri, va, _ = mat
    A, mask = dense_of(mat)
    lead = np.arange((K - 1) * nb)
    A[lead, lead] = 2.0
    # the last block's diagonal: dominant over its own column of the block AND over the column sums the K-1 products can add,
    # sum_i |sum_k (L_k U_k)_ij| <= sum_t (sum_i |L_it|) |U_tj|: S stays strictly column-diagonally dominant
    last = np.arange((K - 1) * nb, n)
    own = np.abs(A[np.ix_(last, last)]).sum(axis=0) - np.abs(A[last, last])
    added = (np.abs(A[np.ix_(last, lead)]).sum(axis=0) / 2.0) @ np.abs(A[np.ix_(lead, last)])
    A[last, last] = np.sign(A[last, last]) * (2.0 * (own + added) + 1.0)
    mat = _pack(A, mask, va.dtype)
    xt = _extended(va.dtype)
    S = A[np.ix_(last, last)].astype(xt)
    for k in range(depth):
        s = slice(k * nb, (k + 1) * nb)
        S -= matmul_ext(A[last, s].astype(xt) / 2, A[s, last].astype(xt))
    return mat, S


def dense_as_mat(S, dtype):
    """A dense array (rounded to `dtype`) as a matrix tuple with every entry stored."""
    return _pack(np.asarray(S).astype(dtype), np.ones(S.shape, bool), dtype)


def clamp_pivots(nb, K=3):
    return [d * nb + k for d, k in clamp_positions(nb, K)]


def check_clamp_case(name, nb, vtype, L, U, ref, mat, who):
    """The assertions of a pivot-clamp case, for the oracle and for the HIP kernels alike; returns (backward ratio, worst column
    ratio).  Why each value tests the rule, from the arithmetic:
    p = 0 unclamped divides by zero: L gets inf / nan -- the finiteness assertion;
    p = -3e-17 unclamped (or clamped to MINUS 1e-16) gives column k of L the opposite sign: an error of 200 % against a bound of 1e-13;
    p = 3e-17 and 0.99e-16 unclamped give L = a / p instead of a / 1e-16: off by a factor 3.3 resp. 1.01, against the same bound;
    p = 3e-17 + 2j unclamped divides by a number of modulus 2 instead of 1e-16, and a clamp that kept the imaginary part likewise;
    p = 2 + 3e-17j is NOT clamped; clamping it (looking at the wrong part) divides by 1e-16 instead of 2;
    p = 1e-16 is NOT clamped and clamping it changes nothing: for it only the stored diagonal and finiteness say anything."""
    values = CLAMP_VALUES_COMPLEX if name in CLAMP_VALUES_COMPLEX else CLAMP_VALUES
    p, is_clamped = values[name]
    u = UNIT_ROUNDOFF[vtype]
    L = np.asarray(L.toarray() if hasattr(L, "toarray") else L)
    U = np.asarray(U.toarray() if hasattr(U, "toarray") else U)
    assert np.isfinite(L).all() and np.isfinite(U).all(), "%s: factors not finite" % who
    glob = clamp_pivots(nb, mat[0] // nb)
    clamped = ref["clamped"]
    assert clamped[glob].all() == is_clamped and clamped.sum() == (len(glob) if is_clamped else 0)
    want = np.array([p], DTYPES[vtype]).tobytes()
    for g in glob:
        assert np.array([U[g, g]], DTYPES[vtype]).tobytes() == want, "%s: stored U[%d,%d] = %r, input %r" % (who, g, g, U[g, g], p)
    ratio = componentwise_check(mat, L, U, u, ref["c"])
    assert ratio <= 1, "%s: entry-wise backward ratio %.3g (c = %.3g)" % (who, ratio, ref["c"])
    cols = clamp_column_check(ref, L, nb, u)
    assert sorted(cols) == sorted(glob)
    for g, col in cols.items():
        assert col <= 1, "%s: column %d of L against the reference: ratio %.3g (c = %.3g)" % (who, g, col, ref["c"])
    return ratio, max(cols.values())


# ---------------------------------------------------------------------------------------------------------------------
# running a case: shared by the GPU tests and their worker processes
# ---------------------------------------------------------------------------------------------------------------------
_oracle_nnz = {}


def oracle_nnz(key, mat, nb, vtype):
    from .helpers import factorize, oracle_library

    if key not in _oracle_nnz:
        res = factorize(mat, nb, oracle_library(vtype), vtype=vtype, ordering="identity", solve=False)
        _oracle_nnz[key] = (int(res["L"].nnz), int(res["U"].nnz))
    return _oracle_nnz[key]


def hip_factors(mat, nb, vtype, options=None, dense=True):
    """The HIP back-end's factors of a designed matrix.  dense: every block gets a mirror and takes the dense kernels, however few
    entries it has (thresholds 0); otherwise none does (threshold above 1000 per mille)."""
    from pangulu_amd import _lib

    from .helpers import factorize

    opts = {_lib.HIP_OPT_DENSE_THRESHOLD_PERMILLE: 0, _lib.HIP_OPT_TRSM_DENSE_PERMILLE: 0} if dense else {_lib.HIP_OPT_DENSE_THRESHOLD_PERMILLE: 1001}
    opts.update(options or {})
    return factorize(mat, nb, "hip", vtype=vtype, ordering="identity", solve=False, hip_options=opts)


def shared_figures(key, mat, nb, vtype, res, ref, backward=True):
    """What every HIP case asserts, as figures: the entry-wise backward ratio, factor sizes against the oracle's, counted against
    structural flops, and the task counts of the kernel classes."""
    st = res["hip_stats"]
    return {
        "case": key, "c": ref["c"],
        "ratio": componentwise_check(mat, res["L"], res["U"], UNIT_ROUNDOFF[vtype], ref["c"]) if backward else None,
        "nnz": [int(res["L"].nnz), int(res["U"].nnz)], "nnz_oracle": list(oracle_nnz(key, mat, nb, vtype)),
        "flop_counted": sum(v["flops"] for v in st.values()), "flop": int(res["info"]["flop"]),
        "dense_updates": st["ssssm_dense_mfma"]["tasks"], "dense_update_launches": st["ssssm_dense_mfma"]["launches"],
        "sparse_updates": st["ssssm_sparse"]["tasks"], "dense_solves": st["tstrf"]["dense_path_tasks"],
        "getrf_launches": st["getrf"]["launches"], "front_workgroups": st["ssssm_dense_mfma"]["front_workgroups"],
        "general_workgroups": st["ssssm_dense_mfma"]["general_workgroups"], "deferred_queues": int(res["info"]["deferred_queues"]),
        "bits": zlib.crc32(res["U"].data.tobytes(), zlib.crc32(res["L"].data.tobytes())),  # fingerprint of the factors' values
        "factor_check_device": res["factor_check"],  # read, not asserted: the clamp cases are singular by design
    }


def assert_shared(f, dense=True):
    assert f["ratio"] <= 1, "entry-wise backward ratio %.3g (c = %.3g): %r" % (f["ratio"], f["c"], f)
    assert f["nnz"] == f["nnz_oracle"], f
    assert f["flop_counted"] == f["flop"], f
    if dense:
        assert f["dense_updates"] > 0 and f["dense_solves"] > 0 and f["getrf_launches"] > 0, f
    else:
        assert f["dense_updates"] == 0 and f["dense_solves"] == 0 and f["sparse_updates"] > 0 and f["getrf_launches"] > 0, f


# how a destination's queue of updates is cut into groups (launch_ssssm, pg_hip_launch_ssssm.h): a group is what one workgroup of
# the update kernel walks, in windows of 16 tasks.  The suite's settings (tests/helpers.py: chunk 8, small launches up to 2048
# tasks) give every update of a launch of at most 2048 tasks a group of its own -- one task per group at every depth here, no
# window is ever refilled.  Group chunk 0 leaves the whole queue in ONE group: launch_ssssm then takes chunk = 1 << 30, and its
# one-task-per-group rule for small launches applies only while opt_group_chunk > 0.  (No statistic exposes group sizes; the
# workgroup count, four per group here, does.)  In both, a launch of at most 64 tasks at nb = 128 is K-split by four: every group appears four times, each on a quarter
# of the K-slabs, merged with atomics -- so the kernels' non-atomic branches (destination preloaded when the whole queue fits one
# window) are NOT reached by these cases.
ARROW_GROUPINGS = ["group_per_update", "one_group", "one_group_first_kernel"]


def arrow_grouping_options(name):
    from pangulu_amd import _lib

    one_group = {_lib.HIP_OPT_SSSSM_GROUP_CHUNK: 0}
    return {"group_per_update": {}, "one_group": one_group,
            # the first general update kernel, ssssm_dense_f64_kernel (pg_hip_dense.h), with windows of 16 of its own
            "one_group_first_kernel": {**one_group, _lib.HIP_OPT_TILES_STAGES: 0}}[name]


_arrow_refs = {}


def arrow_reference(depth, nb=128):
    """Per depth and process: the matrix, S, the extended-precision factors of S with their tile condition, and the oracle's factors
    of the whole matrix (last diagonal block, panels_exact, nnz)."""
    from .helpers import factorize, oracle_library

    if depth not in _arrow_refs:
        mat, S = arrow_case(depth, nb)
        n = mat[0]
        smat = dense_as_mat(S, np.longdouble)
        Lr, Ur, clamped = reference_lu(smat)
        assert not clamped.any()
        res = factorize(mat, nb, oracle_library("r64"), vtype="r64", ordering="identity", solve=False)
        _oracle_nnz["arrow-%d" % depth] = (int(res["L"].nnz), int(res["U"].nnz))
        _arrow_refs[depth] = {"mat": mat, "smat": smat, "L": Lr, "U": Ur, "c": tile_condition(Lr, Ur, clamped),
                              "oracle": arrow_last_block(mat, nb, res["L"], res["U"])}
    return _arrow_refs[depth]


def arrow_last_block(mat, nb, L, U):
    """(L_last, U_last, panels exact?) of a factorisation of an arrow_case, without forming anything dense but the last block row
    and column."""
    n = mat[0]
    A = _csc_of(mat)
    L, U = L.tocsc(), U.tocsc()
    lead, last = slice(0, n - nb), slice(n - nb, n)
    exact = (L[last, lead] != A[last, lead] / 2).nnz == 0 and (U[lead, last] != A[lead, last]).nnz == 0
    return L[last, last].toarray(), U[last, last].toarray(), bool(exact)


def _csc_of(mat):
    import scipy.sparse as sp

    n, cp, ri, va, _ = mat
    return sp.csc_matrix((va, ri.astype(np.int64), cp.astype(np.int64)), shape=(n, n))


def arrow_ratios(ref, L_last, U_last, against=None):
    """The figures of a queue-depth case for one computed last block: componentwise_check on S (gamma over S's own size nb, the
    denominator |L_last||U_last|), the forward comparison with the extended-precision factors of S, and -- `against` = the oracle's
    last block -- the entry-wise comparison with the oracle's factors (within twice the forward bound)."""
    u = UNIT_ROUNDOFF["r64"]
    out = {"ratio": componentwise_check(ref["smat"], L_last, U_last, u, ref["c"]),
           "forward_ratio": forward_check(ref["L"], ref["U"], L_last, U_last, u, ref["c"])}
    if against is not None:
        out["oracle_difference_ratio"] = forward_check(ref["L"], ref["U"], L_last, U_last, u, ref["c"], against=against)
    return out


def arrow_figures(depth, nb=128, options=None):
    """A queue-depth case on the HIP back-end: the shared figures with the ratios of arrow_ratios (and the oracle's own backward
    ratio beside them), whether the panels came out exact, and how the `depth` updates of the last block were launched."""
    ref = arrow_reference(depth, nb)
    mat = ref["mat"]
    res = hip_factors(mat, nb, "r64", options)
    f = shared_figures("arrow-%d" % depth, mat, nb, "r64", res, ref, backward=False)  # (the ratio: below)
    L_last, U_last, f["panels_exact"] = arrow_last_block(mat, nb, res["L"], res["U"])
    Lo, Uo, _ = ref["oracle"]
    f.update(arrow_ratios(ref, L_last, U_last, against=(Lo, Uo)))
    f["oracle_ratio"] = componentwise_check(ref["smat"], Lo, Uo, UNIT_ROUNDOFF["r64"], ref["c"])
    f["depth"] = depth
    return f


def assert_arrow(f):
    assert f["panels_exact"], f
    assert f["dense_updates"] == f["depth"], "updates into the last block: %d tasks in %d launches: %r" % (f["dense_updates"], f["dense_update_launches"], f)
    assert_shared(f)
    assert f["forward_ratio"] <= 1, "last block against the extended-precision factors of S: %.3g: %r" % (f["forward_ratio"], f)
    assert f["oracle_difference_ratio"] <= 1, "last block against the oracle's factors: %.3g: %r" % (f["oracle_difference_ratio"], f)
