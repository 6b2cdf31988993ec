"""The restatement of sgm_lanczos and sgm_generalized_lanczos (tests/lanczos_restated.py) tied to the oracle, host only:

  1  with the sum taken first element to last it equals orc.lanczos / orc.generalized_lanczos in every bit of T and Q, NaN for
     NaN, on every case of tests/test_gpu_lanczos.py the oracle can hold (CSR and ELLPACK leaves; the pencil on CSR) -- the
     oracle is what the eig_* fixtures tie to the reference;
  2  the restated CG that stands in for B%solve where the oracle cannot hold B equals orc.cg bit for bit;
  3  the accuracy table: the oracle's own deviation from the longdouble run on every symmetric case, which the GPU tests' bars
     are 8 x of (MEASURED below; this test fails if the oracle exceeds an entry);
  4  sensitivity: two mutations of the restatement -- the last element of an odd n left out of one update, the last
     re-orthogonalisation correction dropped -- both break 1, and the 1e-9 bar of tests/test_gpu_parity.py misses the second."""
import numpy as np
import pytest

import fused_dot_cases as F
import lanczos_restated as LR
import oracle as orc

# The oracle's deviations from the longdouble run, rounded up to two digits: case -> (max |T - T_ld|, max |Q - Q_ld| over all
# columns, max |Q^T Q - I|; the pencil: |Q^T B Q - I|).  profiles/lanczos_pin/README.md carries the same table.
MEASURED = {
    "grid15x17": (6.2e-15, 5.3e-16, 2.4e-15),
    "grid32x32": (1.6e-14, 5.5e-16, 4.6e-15),
    "grid41x25": (2.2e-14, 7.5e-16, 6.4e-15),
    "tri2049": (5.5e-14, 1.9e-15, 2.7e-14),
    "tri262147": (3.2e-14, 1.7e-16, 2.3e-14),
    "grid33x31": (2.6e-14, 7.5e-16, 6.4e-15),
    "grid33x31_ell": (2.6e-14, 7.5e-16, 6.4e-15),
    "pencil33x31": (3.8e-14, 1.3e-14, 1.0e-14),
}
OLD_BAR_T, OLD_BAR_Q = 1e-9, 1e-10              # tests/test_gpu_parity.py


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _oracle_run(name):
    c = LR.case(name)
    if name == "pencil33x31":
        A, B = LR.oracle_matrix(name)
        return orc.generalized_lanczos(A, B, c.steps, c.q1, 1e-14)
    return orc.lanczos(LR.oracle_matrix(name), c.steps, c.q1)


PLAIN = [n for n in LR.SYMMETRIC if n != "pencil33x31"] + list(LR.DEGENERATE)


@pytest.mark.parametrize("name", PLAIN)
def test_restated_lanczos_is_the_oracle_bit_for_bit(name):
    c = LR.case(name)
    A = LR.oracle_matrix(name)
    To, Qo = _oracle_run(name)
    T, Q = LR.lanczos(A.matvec, c.q1, c.steps, "seq")
    assert _same(T, To) and _same(Q, Qo)
    assert _same(T[0], T[2]) and T[2, -1] == 0.0 and To.shape == (3, c.steps) and Qo.shape == (c.n, c.steps)
    if name in LR.DEGENERATE:
        # n = 1: beta_1 = 0 exactly, q_2 = 0/0; n = 3: steps 4 and 5 run on rounding residue, every entry finite
        assert np.isnan(To).any() == (name == "n1") and np.isnan(Qo).any() == (name == "n1")
    else:
        Td, Qd = LR.lanczos(A.matvec, c.q1, c.steps, "device")
        print(f"{name}: device order against the oracle: T {np.abs(Td - To).max():.2e}, Q {np.abs(Qd - Qo).max():.2e}")
        assert not (_same(Td, To) and _same(Qd, Qo))            # the order of the sums is visible in the bits


@pytest.mark.parametrize("family", [f for f in LR.FAMILY if f != "composite"])
def test_restated_lanczos_is_the_oracle_on_the_kernel_family_cases(family):
    """the `real` matrices of tests/fused_dot_cases.py, one per SpMV kernel family: unsymmetric, empty rows, duplicates"""
    R = F.reference(LR.FAMILY[family], "real")
    assert R.case.key == family
    q1 = LR.start_vector(R.n, 9)
    To, Qo = orc.lanczos(R.A, LR.FAMILY_STEPS, q1)
    T, Q = LR.lanczos(R.A.matvec, q1, LR.FAMILY_STEPS, "seq")
    assert _same(T, To) and _same(Q, Qo) and np.isfinite(To).all() and np.isfinite(Qo).all()
    # not symmetric: x . A y != y . A x
    x, y = LR.start_vector(R.n, 1), LR.start_vector(R.n, 2)
    assert abs(x @ R.A.matvec(y) - y @ R.A.matvec(x)) > 1e-6


def test_every_kernel_family_has_a_case():
    assert set(LR.FAMILY) == set(F.KERNEL_KEYS)
    assert all(F.CASE_BY_NAME[name].key == key for key, name in LR.FAMILY.items())


def test_restated_generalized_lanczos_is_the_oracle_bit_for_bit():
    c = LR.case("pencil33x31")
    A, B = LR.oracle_matrix("pencil33x31")
    To, Qo = _oracle_run("pencil33x31")
    for solve in (lambda w, v: orc.cg(B, v, x0=w, tol=1e-14)[0], lambda w, v: LR.cg(B.matvec, v, w, 1e-14)):
        T, Q = LR.generalized_lanczos(A.matvec, B.matvec, solve, c.q1, c.steps, "seq")
        assert _same(T, To) and _same(Q, Qo)
    assert _same(To[0], To[2]) and To[2, -1] == 0.0 and np.isfinite(To).all()


def test_restated_cg_is_the_oracle_bit_for_bit():
    c = LR.case("pencil33x31")
    _, B = LR.oracle_matrix("pencil33x31")
    x0 = LR.start_vector(c.n, 5)
    xo, it, _, _ = orc.cg(B, c.q1, x0=x0, tol=1e-14)
    assert it > 5 and _same(LR.cg(B.matvec, c.q1, x0, 1e-14), xo)


def test_composite_products_are_not_the_assembled_rows():
    """why the composite cases of the GPU tests restate the block loop: a row that crosses the cut adds two sums"""
    c = LR.case("grid33x31")
    q = LR.start_vector(c.n, 3)
    yb = LR.composite_matvec(LR.composite_leaves(c.n, c.ptr, c.node, c.val, LR.CUT), LR.CUT, c.n)(q)
    ya = LR.oracle_matrix("grid33x31").matvec(q)
    assert np.abs(yb - ya).max() <= 8 * np.finfo(float).eps * np.abs(ya).max() and not np.array_equal(yb, ya)


@pytest.mark.parametrize("name", LR.SYMMETRIC)
def test_accuracy_table_holds_for_the_oracle(name):
    To, Qo = _oracle_run(name)
    dev = LR.deviations(name, To, Qo)
    print(f"{name}: oracle against longdouble: T {dev[0]:.4e}, Q {dev[1]:.4e}, orthogonality {dev[2]:.4e}; table {MEASURED[name]}")
    assert all(d <= m for d, m in zip(dev, MEASURED[name]))
    assert all(d > m / 4 for d, m in zip(dev, MEASURED[name]))             # the table is the measurement, not a loose cap
    assert 8 * MEASURED[name][0] <= OLD_BAR_T and 8 * max(MEASURED[name][1:]) <= OLD_BAR_Q


@pytest.mark.parametrize("name", ["grid15x17", "grid41x25", "tri2049", "grid33x31"])
def test_mutations_break_the_bits_and_the_old_bar_misses_one(name):
    c = LR.case(name)
    A = LR.oracle_matrix(name)
    To, Qo = _oracle_run(name)
    seen = {}
    for mut in LR.MUTATIONS[1:]:
        T, Q = LR.lanczos(A.matvec, c.q1, c.steps, "seq", mutate=mut)
        assert not _same(T, To) and not _same(Q, Qo), mut
        seen[mut] = (np.abs(T - To).max(), np.abs(Q - Qo).max())
        print(f"{name} {mut}: T off by {seen[mut][0]:.2e}, Q by {seen[mut][1]:.2e}")
    assert seen["skip_single"][0] > OLD_BAR_T and seen["skip_single"][1] > OLD_BAR_Q
    assert seen["drop_last_correction"][0] <= OLD_BAR_T and seen["drop_last_correction"][1] <= OLD_BAR_Q
