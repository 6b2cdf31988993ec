"""The two restatements of the coarsening contract (tests/aggregate_restated.py) against each other, the invariants of the
contract, and whether the hierarchy it defines is of any use -- no GPU."""
import numpy as np
import pytest

import aggregate_restated as AG
import algebra_restated as R
import mg_restated as MG

CASES = AG.cases()
THETAS = (0.0, 0.08, 0.3)


def _neighbours(M, theta):
    r, c = AG.strong_entries(M, theta)
    N = [set() for _ in range(M[0])]
    for i, j in zip(r.tolist(), c.tolist()):
        N[i].add(j)
        N[j].add(i)
    return N


@pytest.mark.parametrize("name", sorted(CASES))
def test_literal_and_vectorised_aggregates_agree(name):
    M = CASES[name]
    for theta in THETAS:
        a, na = AG.literal(M, theta)
        b, nb = AG.vectorised(M, theta)
        assert na == nb, (name, theta)
        assert np.array_equal(a, b), (name, theta)


# (stencil27 at theta = 0.08 has no strong entry and no level; theta = 0.03 coarsens it)
@pytest.mark.parametrize("name,theta", [(n, 0.08) for n in sorted(CASES)] + [("stencil27_9x8x8", 0.03)])
@pytest.mark.parametrize("smooth_omega", [0.0, 2.0 / 3.0])
def test_literal_and_vectorised_hierarchies_agree(name, theta, smooth_omega):
    M = CASES[name]
    a = AG.hierarchy(M, theta, smooth_omega, 25, 8, aggregate=AG.literal)
    b = AG.hierarchy(M, theta, smooth_omega, 25, 8, aggregate=AG.vectorised)
    assert len(a) == len(b)
    if theta == 0.03:
        assert len(a) >= 1
    for Pa, Pb in zip(a, b):
        assert R.same(Pa, Pb), name


@pytest.mark.parametrize("name", sorted(CASES))
def test_invariants_of_the_aggregates(name):
    M = CASES[name]
    n = M[0]
    for theta in THETAS:
        agg, nagg = AG.vectorised(M, theta)
        N = _neighbours(M, theta)
        assert agg.min() >= 1 and agg.max() <= nagg
        assert len(np.unique(agg)) == nagg                          # every aggregate has a member
        # the roots: the first vertex of every number in the order the contract numbers them -- the greedy set itself
        key = [AG.key_of(i) for i in range(n)]
        root = [False] * n
        for i in sorted(range(n), key=lambda v: -key[v]):
            root[i] = not (any(root[j] for j in N[i]) or any(root[k] for j in N[i] for k in N[j] if k != i))
        roots = [i for i in range(n) if root[i]]
        assert len(roots) == nagg
        assert [int(agg[i]) for i in roots] == list(range(1, nagg + 1))
        for i in roots:                                             # no two roots within distance 2
            two = set(N[i]) | {k for j in N[i] for k in N[j]}
            assert not any(root[k] for k in two if k != i)
        for i in range(n):                                          # every vertex within distance 2 of its aggregate's root
            r = roots[int(agg[i]) - 1]
            assert r == i or r in N[i] or any(r in N[j] for j in N[i])
        assert all(root[i] for i in range(n) if not N[i])           # no strong neighbour: always a root


@pytest.mark.parametrize("name", ["poisson_31x31", "laplace3d_8x7x6", "random_spd_300", "pattern_asymmetric_150", "duplicates_16"])
def test_theta_zero_makes_every_stored_off_diagonal_strong(name):
    M = CASES[name]
    n, ptr, node, val = AG._csr0(M)
    assert np.isfinite(val).all()
    row = np.repeat(np.arange(n), np.diff(ptr))
    r, c = AG.strong_entries(M, 0.0)
    off = node != row
    assert np.array_equal(r, row[off]) and np.array_equal(c, node[off])


def test_a_diagonal_matrix_gives_singletons_and_no_level():
    M = CASES["diagonal_40"]
    agg, nagg = AG.vectorised(M, 0.08)
    assert nagg == 40 and np.array_equal(agg, np.arange(1, 41))
    assert AG.hierarchy(M, min_coarse=8) == []
    assert AG.hierarchy(M, min_coarse=8, aggregate=AG.literal) == []


def test_the_stop_rules_of_the_hierarchy():
    M = CASES["poisson_33x29"]
    full = AG.hierarchy(M, smooth_omega=0.0, min_coarse=8)
    assert len(full) >= 2
    assert all(P[0] == Q[1] for P, Q in zip(full[1:], full[:-1]))   # the shapes chain
    assert full[-1][1] <= 8 or len(full) == 24
    assert len(AG.hierarchy(M, smooth_omega=0.0, max_levels=2, min_coarse=8)) == 1
    assert AG.hierarchy(M, max_levels=1) == []
    assert AG.hierarchy(M, min_coarse=M[0]) == []


def test_keys_are_distinct_and_the_two_forms_agree():
    k = AG.keys(5000)
    assert len(np.unique(k)) == 5000 and (k != 0).all()
    assert [int(v) for v in k[:300]] == [AG.key_of(i) for i in range(300)]


@pytest.mark.parametrize("smooth_omega", [0.0, 2.0 / 3.0])
def test_the_hierarchy_at_least_halves_the_iterations_of_cg(smooth_omega):
    """Poisson 100 x 70, b = A x* with x* = problems.test_vector, CG to 1e-10: V(1,1) with omega 0.8 and 8 coarse sweeps on the
    restated hierarchy needs fewer than half the iterations of plain CG."""
    from sigma_amd import problems as Pr
    A = CASES["poisson_100x70"]
    rows = MG._Rows(A)
    b = rows.matvec(Pr.test_vector(A[0]))
    stats = []
    Ps = AG.hierarchy(A, 0.08, smooth_omega, 25, 64, stats=stats)
    assert len(Ps) >= 2
    mg = MG.Vectorised(A, Ps, 0.8, 1, 1, 8)
    _, it_mg, _ = MG.pcg(rows, b, mg.apply, tol=1e-10)
    _, it_plain, _ = MG.pcg(rows, b, None, tol=1e-10)
    print(f"smooth_omega {smooth_omega}: {it_mg} iterations against {it_plain}; levels {[(s['rows'], s['aggregates'], s['rounds']) for s in stats]}")
    assert 2 * it_mg < it_plain
