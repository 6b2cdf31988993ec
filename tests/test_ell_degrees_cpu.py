"""ELLPACK degrees without a GPU: the row shapes of tests/ell_degree_cases.py against the reference's own delete_edge (a fixture),
the recovery rule the library runs on the host (sgm_ell_degrees_host), and the reference side of the GPU tests -- the oracle's
Jacobi / ILDU / permutations and tests/edit_restated.py with EXPLICIT degrees -- against one dense, plain-Python statement:
the real entries of row i are its first degrees(i) slots, and of a column stored twice the last one answers."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ell_degree_cases as K  # noqa: E402
import edit_restated as R  # noqa: E402

CASES = K.cases()


def test_delete_edge_restatement_equals_the_reference():
    """tests/golden/ell_degrees/ell_delete_edge_12.npz: the reference's ellpack_graph after a list of delete_edge calls (oracle/ref_driver.f90
    mode `del:`), node / degrees / max_d -- a last neighbour, an only neighbour, a diagonal stored last, middle neighbours, edges
    that are not there, and the array shrinking from 5 to 4 slots."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "ell_degrees", "ell_delete_edge_12.npz"))
    g = K.EllGraph(int(z["n"]))
    for i, j in zip(z["ei"], z["ej"]):
        g.add_edge(int(i), int(j))
    assert g.max_d == 5
    for i, j in zip(z["di"], z["dj"]):
        g.delete_edge(int(i), int(j))
    assert g.max_d == int(z["ref_del_max_d"][0]) == 4
    assert np.array_equal(g.degrees, z["ref_del_degrees"])
    assert np.array_equal(g.node.reshape(-1), z["ref_del_node"])
    # the rows the issue is about are in it: [9, 8, 4, 4] holds 2 neighbours, [2, 2, 2, 2] and [11, 11, 11, 11] none
    assert list(g.node[8]) == [9, 8, 4, 4] and g.degrees[8] == 2
    assert list(g.node[1]) == [2, 2, 2, 2] and g.degrees[1] == 0 and g.degrees[10] == 0


@pytest.mark.parametrize("name", K.NAMES)
def test_host_recovery_per_shape(name):
    """sg.ell_degrees_host = the rule of include/sigma_hip.h, row by row: the true degrees on shapes 1, 2, 3, 7, 8 and 10, -1 on
    the rows of shape 9, and on shapes 4 to 6 the documented wrong answer (one more than the graph holds)."""
    import sigma_amd as sg
    c = CASES[name]
    got = sg.ell_degrees_host(c.node)
    assert np.array_equal(got, K.recovered_degrees(c.node))
    sp = np.array(c.special) - 1
    if name in K.RECOVERABLE:
        assert np.array_equal(got, c.degrees)
    elif name in K.UNKNOWN:
        assert np.all(got[sp] == -1)
        rest = np.setdiff1d(np.arange(c.n), sp)
        assert np.array_equal(got[rest], c.degrees[rest])
    else:
        assert name in K.DELETED
        assert np.array_equal(got, c.recovered) and np.all(got[sp] == c.degrees[sp] + 1)


def test_first_occurrence_rule_is_wrong_on_shapes_4_5_8_9():
    """Why sgm_ell_set_degrees exists: the rule every handle used to get its degrees by (first occurrence of the last slot's
    column, a last slot of 0 = empty) misses the true degrees on exactly the special rows of these shapes -- and is right on the
    add_edge-shaped controls."""
    for name, wrong in (("4_last_neighbour_deleted", 3), ("5_only_neighbour_deleted", 1), ("8_zero_tail", 0), ("9_repeated_column", 2)):
        c = CASES[name]
        old = K.old_rule_degrees(c.node)
        sp = np.array(c.special) - 1
        if name == "9_repeated_column":         # (the repeated column is slot 1 or slot 2 in turn: cut there)
            wrong = 1 + np.arange(len(sp)) % 2
        assert np.all(old[sp] == wrong) and np.all(old[sp] != c.degrees[sp]), name
        rest = np.setdiff1d(np.arange(c.n), sp)
        assert np.array_equal(old[rest], c.degrees[rest]), name
    for name in ("1_add_edge_padding", "2_full_row", "3_empty_row", "7_middle_neighbour_deleted"):
        assert np.array_equal(K.old_rule_degrees(CASES[name].node), CASES[name].degrees)


def _oracle(c):
    import oracle as orc
    return orc, orc.EllMatrix(*c[:6])


@pytest.mark.parametrize("name", K.NAMES)
def test_oracle_jacobi_reads_the_real_entries(name):
    orc, E = _oracle(CASES[name])
    D, present = K.dense_real(CASES[name])
    with np.errstate(divide="ignore"):
        want = 1.0 / np.diag(D)
    got = orc.Jacobi(E).idiag
    assert np.array_equal(got.view(np.int64), want.view(np.int64))
    if name == "9_repeated_column":             # the diagonal stored twice: the later slot answers, not the first
        s = CASES[name].special[0]
        assert got[s - 1] == 1.0 / CASES[name].val[s - 1, -1] != 1.0 / CASES[name].val[s - 1, 0]
    assert np.array_equal(np.isinf(got), ~np.diag(present) | (np.diag(D) == 0.0))


@pytest.mark.parametrize("name", K.NAMES)
def test_oracle_ildu_pattern_and_factors_are_those_of_the_real_entries(name):
    """The pattern: row by row the real entries' columns in stored order, below the diagonal into L, above into U.  The factors:
    sparse_static_pattern_ldu_factorization (ldu_solvers.f90:275-387) written out on dense arrays whose entries are the real
    entries (last write wins) -- the same operations in the same order, so the bits agree (NaNs by position).  Skipped for the
    values of shape 9 only: with a column stored twice the factor rows hold it twice, which a dense array cannot show."""
    c = CASES[name]
    orc, E = _oracle(c)
    F = orc.Ildu(E)
    Lrows, Urows = [], []
    for i in range(c.n):
        cols = [int(j) - 1 for j in c.node[i, :c.degrees[i]]]
        Lrows.append([j for j in cols if j < i])
        Urows.append([j for j in cols if j > i])
    assert np.array_equal(F.Lptr, 1 + np.cumsum([0] + [len(r) for r in Lrows]))
    assert np.array_equal(F.Uptr, 1 + np.cumsum([0] + [len(r) for r in Urows]))
    nl, nu = F.Lptr[-1] - 1, F.Uptr[-1] - 1
    assert np.array_equal(F.Lnode[:nl], [j + 1 for r in Lrows for j in r])
    assert np.array_equal(F.Unode[:nu], [j + 1 for r in Urows for j in r])
    if name in K.UNKNOWN:
        return
    A, present = K.dense_real(c)
    L, U, d = np.tril(A, -1), np.triu(A, 1), np.diag(A).copy()
    with np.errstate(all="ignore"):
        for i in range(c.n):
            for k in Lrows[i]:
                Uki = U[k, i]
                L[i, k] = L[i, k] / d[k]
                Lik = L[i, k]
                for j in Lrows[i]:
                    if j > k:
                        L[i, j] = L[i, j] + -Lik * d[k] * U[k, j]
                d[i] = d[i] - Lik * d[k] * Uki
                for j in Urows[i]:
                    U[i, j] = U[i, j] + -Lik * d[k] * U[k, j]
            for k in Urows[i]:
                U[i, k] = U[i, k] / d[i]

    def same(x, y):
        x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
        nan = np.isnan(x)
        return np.array_equal(nan, np.isnan(y)) and np.array_equal(x[~nan].view(np.int64), y[~nan].view(np.int64))
    assert same(F.D, d)
    assert same(F.Lval[:nl], [L[i, j] for i in range(c.n) for j in Lrows[i]])
    assert same(F.Uval[:nu], [U[i, j] for i in range(c.n) for j in Urows[i]])


@pytest.mark.parametrize("name", K.NAMES)
def test_oracle_permutations_carry_degrees_and_zeros(name):
    c = CASES[name]
    orc, E = _oracle(c)
    rs = np.random.RandomState(3)
    p, q = (rs.permutation(c.n) + 1).astype(np.int32), (rs.permutation(c.n) + 1).astype(np.int32)
    node, val, deg = orc.ell_permuted(E, p, q)
    for i in range(c.n):
        d = p[i] - 1
        assert deg[d] == c.degrees[i]
        assert np.array_equal(val[d].view(np.int64), c.val[i].view(np.int64))
        for k in range(c.max_d):
            assert node[d, k] == (0 if c.node[i, k] == 0 else q[c.node[i, k] - 1])
    D, present = K.dense_real(c)
    D2, present2 = K.dense_real(c._replace(node=node, val=val, degrees=deg))
    inv_p, inv_q = np.argsort(p), np.argsort(q)
    assert np.array_equal(D2[np.ix_(p - 1, q - 1)], D) and np.array_equal(present2[np.ix_(p - 1, q - 1)], present)
    assert np.array_equal(D2, D[np.ix_(inv_p, inv_q)])


@pytest.mark.parametrize("name", K.NAMES)
def test_edit_restatement_goes_by_degrees(name):
    c = CASES[name]
    S = R.ell(c.n, c.m, c.node, c.degrees)
    D, present = K.dense_real(c)
    real, pad, absent = K.probes(c)
    if name in K.DELETED:
        assert len(pad) == len(c.special)               # the slots delete_edge left behind
    ij = np.array(real + pad + absent, np.int32)
    want = np.array([D[i - 1, j - 1] for i, j in ij])
    for get in (R.get_literal, R.get_vectorised):
        assert np.array_equal(get(S, c.val, ij[:, 0], ij[:, 1]).view(np.int64), want.view(np.int64))
    # set / add on the real entries, every entry twice: the later triple wins / both are added, one rounding each
    rs = np.random.RandomState(5)
    pick = rs.randint(len(real), size=min(400, 2 * len(real)))
    ti, tj = np.array([real[k][0] for k in pick], np.int32), np.array([real[k][1] for k in pick], np.int32)
    z = rs.standard_normal(len(pick))
    Dset, Dadd = D.copy(), D.copy()
    for t in range(len(pick)):
        Dset[ti[t] - 1, tj[t] - 1] = z[t]
        Dadd[ti[t] - 1, tj[t] - 1] = Dadd[ti[t] - 1, tj[t] - 1] + z[t]
    for mode, Dw in (("set", Dset), ("add", Dadd)):
        for apply in (R.apply_literal, R.apply_vectorised):
            v2 = apply(S, c.val, ti, tj, z, mode)
            D2, _ = K.dense_real(c._replace(val=v2))
            dupcols = name in K.UNKNOWN and mode == "add"
            if not dupcols:          # (a column stored twice: add touches both slots, the dense statement shows the later one)
                assert np.array_equal(D2.view(np.int64), Dw.view(np.int64)), (mode, apply.__name__)
            live = np.arange(c.max_d)[None, :] < c.degrees[:, None]
            assert np.array_equal(v2[~live].view(np.int64), c.val[~live].view(np.int64))       # padding values untouched
    for i, j in pad[:3] + absent[:2]:
        with pytest.raises(LookupError):
            R.apply_literal(S, c.val, np.array([real[0][0], i], np.int32), np.array([real[0][1], j], np.int32), np.ones(2), "set")
