"""The contract of multigrid's direct coarse solve on the CPU (tests/mg_direct_restated.py): the two restatements agree bit
for bit, the inverse is an inverse, the pivot rule picks what it says, an exact coarse solve keeps the two-level iteration
count where eight sweeps lose it, and a singular level is refused at the step the rule gives."""
import numpy as np
import pytest

import aggregate_restated as AG
import algebra_restated as R
import mg_direct_restated as DR
import mg_restated as MG
from sigma_amd import problems as PB

OMEGA = 0.8
_cases = DR.cases()
_lev = {}


def levels(name):
    if name not in _lev:
        A, Ps = _cases[name]
        _lev[name] = MG.levels(A, Ps)
    return _lev[name]


@pytest.mark.parametrize("name", DR.LITERAL)
def test_the_two_restatements_agree_bit_for_bit(name):
    A, Ps = _cases[name]
    lev = levels(name)
    lit = DR.Literal(A, Ps, OMEGA, 1, 1, lev=lev)
    vec = DR.Vectorised(A, Ps, OMEGA, 1, 1, lev=lev)
    assert lit.Ainv.shape == (lev[-1][0],) * 2
    assert np.array_equal(R.bits(lit.Ainv), R.bits(vec.Ainv))
    assert np.array_equal(lit.piv, vec.piv)
    rs = np.random.RandomState(5)
    for b in (PB.test_vector(lev[-1][0]), rs.standard_normal(lev[-1][0])):
        assert np.array_equal(R.bits(DR.apply_literal(lit.Ainv, b)), R.bits(DR.apply_vectorised(vec.Ainv, b)))
    if A[0] <= 128:                                      # the whole V-cycle, where the literal levels above are small too
        r = PB.test_vector(A[0])
        assert np.array_equal(R.bits(lit.apply(r)), R.bits(vec.apply(r)))


def test_the_chunks_of_the_apply_are_part_of_the_sum():
    # 300 columns: two chunks.  The chunked sum and the plain ascending sum differ in the last bits for some row
    rs = np.random.RandomState(9)
    M, b = rs.standard_normal((300, 300)), rs.standard_normal(300)
    x = DR.apply_vectorised(M, b)
    assert np.array_equal(R.bits(x), R.bits(DR.apply_literal(M, b)))
    plain = np.zeros(300)
    for j in range(300):
        plain = plain + M[:, j] * b[j]
    assert not np.array_equal(x, plain)
    assert np.abs(x - plain).max() <= 1e-12


@pytest.mark.parametrize("name", DR.SPD)
def test_the_inverse_times_the_matrix_is_the_identity_on_the_spd_cases(name):
    A, Ps = _cases[name]
    vec = DR.Vectorised(A, Ps, OMEGA, 1, 1, lev=levels(name))
    n = vec.D.shape[0]
    err = np.abs(vec.Ainv @ vec.D - np.eye(n)).max()
    print(f"{name}: n = {n}, max |Ainv D - I| = {err:.3e}")
    assert err <= 1e-8


def test_a_pivot_off_the_diagonal_and_a_tie_follow_the_rule():
    A, Ps = _cases["pivoting"]
    vec = DR.Vectorised(A, Ps, OMEGA, 1, 1, lev=levels("pivoting"))
    assert np.array_equal(vec.D, np.array([[0.0, 2.0, 1.0], [2.0, 0.0, 0.0], [1.0, 0.0, 3.0]]))
    assert vec.piv.tolist() == [2, 2, 3]
    assert np.abs(vec.Ainv @ vec.D - np.eye(3)).max() <= 1e-15
    A, Ps = _cases["tie_L0"]
    for cls in (DR.Literal, DR.Vectorised):
        assert cls(A, Ps, OMEGA, 1, 1).piv[0] == 2       # |-3| = |3|: the smaller index
    # a NaN counts as larger than everything -- and is then refused as a pivot
    D = np.array([[1.0, 0.0], [np.nan, 1.0]])
    for inv in (DR.invert_literal, DR.invert_vectorised):
        with pytest.raises(DR.Refused) as e:
            inv(D)
        assert e.value.step == 1


def test_a_zero_row_is_refused_at_the_expected_step():
    A, _ = DR.zero_row_case(7, 4)
    D = DR.dense(A)
    for inv in (DR.invert_literal, DR.invert_vectorised):
        with pytest.raises(DR.Refused) as e:
            inv(D)
        assert e.value.step == 5
        assert "step 5" in str(e.value) and "singular or non-finite coarse level" in str(e.value)
    with pytest.raises(DR.Refused) as e:
        DR.invert_vectorised(np.zeros((1, 1)))
    assert e.value.step == 1


def test_an_exact_coarse_solve_keeps_the_two_level_iteration_count():
    A = DR.poisson(96, 96)
    Ps = AG.hierarchy(A, max_levels=2)
    assert len(Ps) == 1 and Ps[0][1] == 1297
    lev = MG.levels(A, Ps)
    rows = MG._Rows(A)
    b = rows.matvec(PB.test_vector(A[0]))
    direct = DR.Vectorised(A, Ps, OMEGA, 1, 1, lev=lev)
    sweeps = MG.Vectorised(A, Ps, OMEGA, 1, 1, 8, lev=lev)
    xd, it_direct, _ = MG.pcg(rows, b, direct.apply, tol=1e-10)
    xs, it_sweeps, _ = MG.pcg(rows, b, sweeps.apply, tol=1e-10)
    print(f"96^2, {Ps[0][1]} coarse rows: PCG {it_direct} iterations with the direct coarse level, {it_sweeps} with 8 sweeps")
    assert it_direct <= 30
    assert it_sweeps >= 40
    assert np.abs(xd - PB.test_vector(A[0])).max() <= 1e-8
