"""The extended-precision GMRES restatement (tests/gmres_restated.py) checked on the host, and the oracle's textbook GMRES
measured against it on every case of tests/gmres_cases.py, with both orthogonalisations.  The deviations measured here are the
constants of tests/test_gpu_gmres.py (MEASURED_T1, MEASURED_T3, T2_C) that the device's bars are 8 x of: a test below fails when
the oracle exceeds what is recorded there, so the record cannot drift."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gmres_cases as GC              # noqa: E402
import gmres_restated as GR           # noqa: E402
import test_gpu_gmres as DEVICE       # noqa: E402   (the recorded constants only: nothing of it runs here)

ORTH = pytest.mark.parametrize("orth", ["mgs", "cgs2"])


_oracle = GC.oracle_solve


# ------------------------------------------------------------------ the restatement itself
def test_optimal_history_is_the_least_squares_minimum():
    """against the definition: min_y |r0 - A K_k y| by a dense least-squares solve on the (orthonormalised) Krylov matrix"""
    rs = np.random.RandomState(3)
    n = 12
    a = rs.standard_normal((n, n)) + 3 * np.eye(n)
    r0 = rs.standard_normal(n)
    res, closed = GR.optimal_history(lambda v: np.asarray(a, GR.LD) @ v, r0, n, n)
    assert closed in (None, n) and len(res) == n        # (the last vector is rounding: zero or not by a hair)
    K = np.zeros((n, 0))
    v = r0.copy()
    for k in range(n - 1):
        K = np.linalg.qr(np.column_stack([K, v]))[0]
        v = a @ K[:, -1]
        want = np.linalg.norm(r0 - a @ K @ np.linalg.lstsq(a @ K, r0, rcond=None)[0])
        assert abs(float(res[k]) - want) <= 1e-12 * np.linalg.norm(r0)
    assert np.all(np.diff(res.astype(np.float64)) <= 0)
    assert float(res[-1]) <= 1e-15 * np.linalg.norm(r0)


@pytest.mark.parametrize("name, step", [("lucky-shift", 20), ("lucky-identity", 1), ("lucky-diag248", 3)])
def test_the_step_at_which_the_krylov_space_closes(name, step):
    c, r = GC.case(name), GC.reference(name)
    res, closed = GR.optimal_history(r.op, c["b"], c["restart"], c["cap"])
    assert closed == step == len(res) == c["expect_iterations"] == r.it
    assert float(res[-1]) <= 64 * GR.EPS_LD * np.linalg.norm(c["b"])
    assert float(GR.true_residual(r.op, r.x, c["b"])) <= 64 * GR.EPS_LD * np.linalg.norm(c["b"])


def test_restarted_reports_the_true_residual():
    """within a cycle and across restarts the recurrence's residual is |M^-1 (b - A x)| of the x it returns"""
    for name in ("cap-29", "cap-31", "cap-45", "jacobi-advdiff", "indef-m13"):
        c, r = GC.case(name), GC.reference(name)
        true = GR.true_residual(r.op, r.x, c["b"], r.apply_pc)
        assert abs(float(true - r.res[-1])) <= 1e-15 * float(r.cycles[0][1]), name


def test_stagnation_and_an_empty_operator():
    c, r = GC.case("stagnation"), GC.reference("stagnation")
    assert r.it == 40 and np.array_equal(r.res, np.ones(40)) and np.array_equal(r.x, np.zeros(c["n"]))
    for orth in ("mgs", "cgs2"):
        x, it, res, h = _oracle("stagnation", orth)
        assert it == 40 and res == 1.0 and np.array_equal(h, np.ones(40)) and np.array_equal(x, np.zeros(c["n"]))
    # all-empty A: the restatement takes no step and keeps x; the oracle's rotation is 0 / 0
    c, r = GC.case("nan"), GC.reference("nan")
    assert r.it == 1 and np.array_equal(r.x, c["x0"]) and float(r.res[0]) == float(np.sqrt(GR.LD(5)))
    x, it, res, _ = _oracle("nan", "mgs")
    assert it == 1 and np.isnan(res)


# ------------------------------------------------------------------ the oracle against it: where the bars come from
@ORTH
@pytest.mark.parametrize("name", GC.T1_CASES)
def test_oracle_history_and_iterate(name, orth):
    """T1 / T1x: the oracle stays within what tests/test_gpu_gmres.py records for it, the restatement alone keeps 80 % of the
    steps inside the window, and the recorded T1 is below the 1e-8 of test_gmres on every case (8 x it is not on the
    ill-conditioned one: there the device's bar is the 1e-8)"""
    c, r = GC.case(name), GC.reference(name)
    x, it, _, h = _oracle(name, orth)
    dev, share, xdev = GC.compare(name, x, h)
    t1, t1x = DEVICE.MEASURED_T1[name]
    print(f"{name} {orth}: T1 {dev:.3e} (recorded {t1:.1e}), share {share:.3f}, T1x {xdev:.3e} (recorded {t1x:.1e})")
    assert it == r.it == c["cap"]
    assert share >= 0.8
    assert dev <= t1 <= 1e-8
    assert xdev <= t1x
    assert t1x <= 1e-10 or name.startswith("illcond")


@ORTH
@pytest.mark.parametrize("name", GC.TINY + GC.LUCKY + GC.NEAR + ["guess"])
def test_oracle_counts_and_true_residuals(name, orth):
    """S and T2: the oracle takes the restatement's number of steps (exactly, on the breakdown cases) and its x needs c = 0"""
    c, r = GC.case(name), GC.reference(name)
    x, it, _, _ = _oracle(name, orth)
    assert GC.count_ok(it, r.it)
    if name in GC.LUCKY:
        assert it == r.it == c["expect_iterations"]
    if name in GC.TINY:
        assert r.it <= c["n"]
    need = GC.t2_needed(name, x)
    print(f"{name} {orth}: {it} iterations (restated {r.it}), T2 needs c = {need:.3e}")
    assert 8 * need <= DEVICE.T2_C


@ORTH
@pytest.mark.parametrize("name", GC.CAPS)
def test_oracle_reported_against_true_residual(name, orth):
    x, it, res, _ = _oracle(name, orth)
    gap = GC.t3_gap(name, x, res * res)
    print(f"{name} {orth}: T3 {gap:.3e} (recorded {DEVICE.MEASURED_T3[name]:.1e})")
    assert it == GC.case(name)["cap"]
    assert gap <= DEVICE.MEASURED_T3[name]


def test_vcycle_case_stays_in_its_window():
    """the oracle has no V-cycle: only the restatement runs here.  4 of its 5 steps lie inside the narrower window."""
    c, r = GC.case("mg"), GC.reference("mg")
    dev, share, _ = GC.compare("mg", r.x, np.asarray(r.res * r.res, np.float64))
    assert r.it == c["cap"] == 5 and share >= 0.8 and dev <= 4 * GR.EPS_D
    assert float(r.res[3]) >= GC.MG_WINDOW * float(r.cycles[0][1]) > float(r.res[4])
