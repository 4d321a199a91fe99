"""The directed block cases (tests/directed_blocks.py) on the oracle platform: pins the case designs -- every pattern reports the
tile occupancy it claims after fill -- and the extended-precision reference, and shows that the inputs stay inside the entry-wise
bound under the reference's own arithmetic, before any GPU sees them.  No GPU."""
import numpy as np
import pytest

from . import directed_blocks as D
from .helpers import factorize, oracle_library

def reference(key, mat, pivots=()):
    return D.reference(key, mat, pivots, keep_factors=True)


def oracle_factors(mat, nb, vtype):
    return factorize(mat, nb, oracle_library(vtype), vtype=vtype, ordering="identity", solve=False)


def test_long_double_is_an_extended_type():
    assert np.finfo(np.longdouble).nmant >= 63


def test_reference_lu_on_a_matrix_with_known_factors():
    """L and U chosen (small integers, exact in every type), A = L U formed exactly: reference_lu must return them bit for bit;
    and a 2 x 2 with a tiny pivot shows the clamp rule: divisor +1e-16, stored diagonal untouched."""
    rng = np.random.default_rng(5)
    n = 48
    L = np.tril(rng.integers(-2, 3, (n, n)), -1) + np.eye(n)
    U = np.triu(rng.integers(-2, 3, (n, n)), 1) + np.diag(rng.choice([-2.0, -1.0, 1.0, 2.0], n))
    A = L @ U
    Lr, Ur, clamped = D.reference_lu(D.dense_as_mat(A, np.float64))
    assert (Lr == L).all() and (Ur == U).all() and not clamped.any()
    for p in (-3e-17, 0.0):
        Lr, Ur, clamped = D.reference_lu(D.dense_as_mat(np.array([[p, 0.0], [0.5, 1.0]]), np.float64))
        assert clamped.tolist() == [True, False] and Ur[0, 0] == p and Lr[1, 0] == np.longdouble(0.5) / np.longdouble(1e-16)
    Lr, Ur, clamped = D.reference_lu(D.dense_as_mat(np.array([[3e-17 + 2j, 0.0], [0.5, 1.0]]), np.complex128))
    assert clamped[0] and Lr[1, 0].imag == 0 and Lr[1, 0].real == np.longdouble(0.5) / np.longdouble(1e-16)
    Lr, Ur, clamped = D.reference_lu(D.dense_as_mat(np.array([[1e-16, 0.0], [0.5, 1.0]]), np.float64))
    assert not clamped.any()


def test_componentwise_check_notices_one_wrong_small_entry():
    """What the suite's 1e-12-of-the-largest-entry comparisons cannot see: one small entry of L off by 1e-9 relative."""
    mat = D.pattern_case("corners", 128)
    ref = reference("corners-128-r64", mat)
    L, U, c = ref["L"], ref["U"], ref["c"]
    u = D.UNIT_ROUNDOFF["r64"]
    assert D.componentwise_check(mat, L.astype(np.float64), U.astype(np.float64), u, c) <= 1
    Lw = L.astype(np.float64)
    i, j = 128 + 127, 0  # the corner entry (nb-1, 0) of block (1,0)
    assert Lw[i, j] != 0 and abs(Lw[i, j]) < 1e-2 * abs(U).max()
    Lw[i, j] *= 1 + 1e-9
    assert D.componentwise_check(mat, Lw, U.astype(np.float64), u, c) > 1


@pytest.mark.parametrize("nb", [128, 256])
@pytest.mark.parametrize("name", sorted(D.PATTERN_CASES))
def test_pattern_case_occupancy_after_fill(name, nb):
    mat = D.pattern_case(name, nb)
    occ = D.symbolic_tile_occupancy(mat, nb)
    assert (occ == D.predicted_tile_occupancy(mat)).all(), "the host's symbolic pattern and the boolean elimination disagree"
    live = D.live_tiles_per_block(occ, nb)
    rows = [[live[(I, J)] for J in range(3)] for I in range(3)]
    assert rows == D.EXPECTED_LIVE_TILES[nb][name], "live tiles per block after fill: %r" % (rows,)


def _oracle_case(key, mat, nb, vtype, pivots=()):
    ref = reference(key, mat, pivots)
    Lr, Ur, c = ref["L"], ref["U"], ref["c"]
    res = oracle_factors(mat, nb, vtype)
    u = D.UNIT_ROUNDOFF[vtype]
    ratio = D.componentwise_check(mat, res["L"], res["U"], u, c)
    assert ratio <= 1, "oracle: entry-wise backward ratio %.3g (c = %.3g)" % (ratio, c)
    # the reference itself, rounded to nothing: far inside the bound of the working type
    assert D.componentwise_check(mat, Lr, Ur, u, c) <= 2.0 ** -8
    if not len(pivots):
        fw = D.forward_check(Lr, Ur, res["L"], res["U"], u, c)
        assert fw <= 1, "oracle: entry-wise forward ratio %.3g (c = %.3g)" % (fw, c)
    return res, ref


@pytest.mark.parametrize("nb", [128, 256])
@pytest.mark.parametrize("name", sorted(D.PATTERN_CASES))
def test_pattern_case_oracle_r64(name, nb):
    _oracle_case("%s-%d-r64" % (name, nb), D.pattern_case(name, nb), nb, "r64")


@pytest.mark.parametrize("name", D.CR64_PATTERN_CASES)
def test_pattern_case_oracle_cr64(name):
    _oracle_case("%s-128-cr64" % name, D.pattern_case(name, 128, "cr64"), 128, "cr64")


@pytest.mark.parametrize("name", D.R32_PATTERN_CASES)
def test_pattern_case_oracle_r32(name):
    _oracle_case("%s-128-r32" % name, D.pattern_case(name, 128, "r32"), 128, "r32")


CLAMP_PARAMS = [(name, nb, "r64") for nb in (256, 128, 32) for name in D.CLAMP_VALUES] + \
               [(name, nb, "cr64") for nb in (256, 128, 32) for name in D.CLAMP_VALUES_COMPLEX]


@pytest.mark.parametrize("name,nb,vtype", CLAMP_PARAMS)
def test_clamp_case_oracle(name, nb, vtype):
    mat = D.clamp_case(name, nb, vtype)
    res, ref = _oracle_case("clamp-%s-%d-%s" % (name, nb, vtype), mat, nb, vtype, pivots=D.clamp_pivots(nb))
    D.check_clamp_case(name, nb, vtype, res["L"], res["U"], ref, mat, "oracle")


@pytest.mark.parametrize("depth", D.QUEUE_DEPTHS)
def test_arrow_case_oracle(depth):
    """The oracle's last diagonal block of a queue-depth case: componentwise_check on S = A_last - sum_k L_k U_k (gamma over S's own
    size, the denominator |L_last||U_last|), and entry-wise against the extended-precision factors of S."""
    ref = D.arrow_reference(depth, 128)
    Lo, Uo, panels_exact = ref["oracle"]
    assert panels_exact  # by design: the leading diagonal blocks are 2 I
    f = D.arrow_ratios(ref, Lo, Uo)
    print(depth, f)
    assert f["ratio"] <= 1, "oracle, depth %d: ratio %.3g (c = %.3g)" % (depth, f["ratio"], ref["c"])
    assert f["forward_ratio"] <= 1, "oracle, depth %d: forward ratio %.3g (c = %.3g)" % (depth, f["forward_ratio"], ref["c"])
