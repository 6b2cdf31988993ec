"""GMRES(m) on the device against the extended-precision restatement (tests/gmres_restated.py), under both orthogonalisations
(gmres_cgs2 = 1: the low-synchronisation kernels up to restart 32; 0: modified Gram-Schmidt), every solve capped.

What each bar is measured against (none is read off the device code; tests/test_gmres_cpu.py re-measures them on the host):
  T1   sqrt(history[k]) against the optimal residual, step by step from the start of every cycle down to sqrt(eps_double) of
       the cycle's starting norm; at least 80 % of the steps run are inside that window.  Bar: 8 x the deviation of the
       oracle's own double-precision GMRES (the worse of "mgs" and "cgs2") on the same case, never above the 1e-8 of test_gmres.
  T1x  |x - x_ref|_inf / |x_ref|_inf at the cap: 8 x the oracle's, never above the 1e-10 of test_gmres -- except on the
       ill-conditioned matrix, where the measured 8 x 2.9e-10 is the bar.
  T2   |b - A x|_2 <= tol + c eps_double (|A|_inf |x|_2 + |b|_2), c = 8 x what the oracle's x needs.  The oracle's x needs
       c = 0 on every converged case here (its true residual is below tol), so the bar is tol itself.
  T3   |sqrt(res2) - |M^-1 (b - A x)|| / beta at a cap: 8 x the oracle's gap.
  S    abs(it - it_oracle) <= max(2, 0.02 it_oracle), the suite's bar on iteration counts: against the oracle's count with
       the same orthogonalisation, and against the restatement's."""
import numpy as np
import pytest

import gmres_cases as GC
import gmres_restated as GR
import sigma_amd as sg

pytestmark = pytest.mark.gpu

# The oracle's own deviations from the restatement, the worse of orth = "mgs" and "cgs2", rounded up to two digits
# (measured by tests/test_gmres_cpu.py, which fails when the oracle exceeds one of them): case -> (T1, T1x)
MEASURED_T1 = {
    "opt-n63-m1": (1.1e-16, 3.6e-16),
    "opt-n63-m2": (3.2e-16, 5.1e-16),
    "opt-n63-m5": (7.0e-16, 9.1e-16),
    "opt-n63-m30": (3.9e-14, 4.0e-15),
    "opt-n63-m32": (5.9e-14, 3.1e-15),
    "opt-n63-m33": (6.4e-14, 7.5e-15),
    "opt-n63-m48": (7.4e-13, 2.8e-14),
    "opt-n63-m64": (3.1e-14, 4.2e-14),
    "opt-n257-m1": (3.7e-16, 5.4e-16),
    "opt-n257-m2": (2.6e-16, 1.5e-15),
    "opt-n257-m5": (2.5e-16, 1.9e-15),
    "opt-n257-m30": (4.3e-15, 2.2e-14),
    "opt-n257-m32": (7.9e-15, 9.2e-15),
    "opt-n257-m33": (7.0e-15, 3.6e-14),
    "opt-n257-m48": (7.0e-14, 8.3e-14),
    "opt-n257-m64": (4.6e-14, 2.3e-14),
    "opt-n1001-m1": (3.2e-16, 1.4e-15),
    "opt-n1001-m2": (4.8e-16, 2.0e-15),
    "opt-n1001-m5": (5.8e-16, 5.7e-15),
    "opt-n1001-m30": (3.6e-15, 4.2e-14),
    "opt-n1001-m32": (2.3e-15, 2.0e-14),
    "opt-n1001-m33": (3.3e-15, 2.0e-14),
    "opt-n1001-m48": (1.5e-14, 6.5e-14),
    "opt-n1001-m64": (1.8e-14, 2.3e-14),
    "opt-n4099-m1": (1.4e-15, 2.6e-15),
    "opt-n4099-m2": (7.5e-16, 2.0e-15),
    "opt-n4099-m5": (9.8e-16, 1.2e-15),
    "opt-n4099-m30": (5.5e-16, 2.2e-14),
    "opt-n4099-m32": (1.8e-15, 2.6e-14),
    "opt-n4099-m33": (2.4e-15, 2.0e-14),
    "opt-n4099-m48": (3.7e-15, 7.2e-14),
    "opt-n4099-m64": (2.7e-15, 1.9e-13),
    "skew-m30": (6.5e-15, 1.3e-15),
    "skew-m13": (2.1e-10, 4.1e-16),
    "indef-m30": (1.5e-12, 3.6e-12),
    "indef-m13": (7.6e-15, 9.5e-15),
    "illcond-m30": (5.7e-10, 2.9e-10),
    "illcond-m32": (1.3e-09, 1.3e-11),
    "skew-m30-jacobi": (2.9e-15, 1.7e-15),
    "jacobi-advdiff": (1.1e-14, 1.2e-13),
    "part-plain-m13": (3.7e-15, 6.6e-14),
    "part-plain-m32": (2.3e-15, 2.0e-14),
    "part-jacobi-m13": (1.8e-15, 2.6e-14),
    "part-jacobi-m32": (1.3e-14, 1.3e-13),
}
# case -> the oracle's T3 gap
MEASURED_T3 = {
    "cap-29": 1.2e-15,
    "cap-30": 4.3e-16,
    "cap-31": 5.4e-16,
    "cap-45": 6.5e-16,
}
T2_C = 0.0          # 8 x 0: see T2 above

ORTH = pytest.mark.parametrize("cgs2", [1, 0], ids=["lowsync", "mgs"])


def _check_count(name, s, cgs2):
    """S, against the oracle (orth as on the device) and the restatement"""
    r, ito = GC.reference(name), GC.oracle_count(name, "cgs2" if cgs2 else "mgs")
    print(f"{name}: {s.last_iterations} iterations (oracle {ito}, restated {r.it}), converged {s.converged}, res2 {s.res2:.3e}")
    assert GC.count_ok(s.last_iterations, ito)
    assert GC.count_ok(s.last_iterations, r.it)


def bar_t1(name):
    return min(1e-8, 8 * MEASURED_T1[name][0])


def bar_t1x(name):
    if name.startswith("illcond"):
        return 8 * MEASURED_T1[name][1]
    return min(1e-10, 8 * MEASURED_T1[name][1])


@pytest.fixture(scope="module", autouse=True)
def _init():
    sg.init(0)


def _matrix(c, parts=False):
    if parts:
        return sg.partitioned_csr_matrix(c["n"], c["n"], c["ptr"], c["node"], c["val"], c["starts"])
    return sg.csr_matrix(c["n"], c["n"], c["ptr"], c["node"], c["val"])


def _pc(c, A):
    if c["pc"] == "none":
        return None, ()
    if c["pc"] == "jacobi":
        pc = sg.jacobi()
        pc.setup(A)
        return pc, ()
    Ps = [sg.csr_matrix(P[0], P[1], np.asarray(P[2], np.int32), np.asarray(P[3], np.int32), np.asarray(P[4], np.float64))
          for P in c["mg"][1]]
    pc = sg.multigrid(Ps, omega=0.8, nu_pre=1, nu_post=1, coarse_sweeps=8)
    pc.setup(A)
    return pc, Ps


def _solve(name, cgs2, parts=False, on_device=False):
    """the capped device solve of a case: (solver, x)"""
    c = GC.case(name)
    A = _matrix(c, parts)
    pc, keep = _pc(c, A)
    s = sg.gmres(c["tol"], c["restart"])
    s.set_option("gmres_cgs2", cgs2)
    s.set_max_iter(c["cap"])
    s.set_history(c["cap"] + 8)
    s.setup(A)
    x, b = c["x0"].copy(), c["b"]
    if on_device:
        import torch
        x, b = torch.tensor(x, device="cuda"), torch.tensor(b, device="cuda")
    s.solve(A, x, b, pc, check=False)
    if on_device:
        x = x.cpu().numpy()
    return s, x


def _check_t1(name, s, x):
    c = GC.case(name)
    dev, share, xdev = GC.compare(name, x, s.history)
    print(f"{name}: iterations {s.last_iterations}, T1 {dev:.3e} (bar {bar_t1(name):.3e}), share {share:.3f}, "
          f"T1x {xdev:.3e} (bar {bar_t1x(name):.3e})")
    assert s.last_iterations == c["cap"] == len(s.history)
    assert np.isfinite(x).all()
    assert share >= 0.8
    assert dev <= bar_t1(name)
    assert xdev <= bar_t1x(name)


def _check_t2(name, x):
    c, r = GC.case(name), GC.reference(name)
    res = float(GR.true_residual(r.op, x, c["b"]))
    bound = c["tol"] + T2_C * GR.EPS_D * (r.anorm * np.linalg.norm(x) + np.linalg.norm(c["b"]))
    print(f"{name}: true residual {res:.3e} (bar {bound:.3e})")
    assert np.isfinite(x).all()
    assert res <= bound


@ORTH
@pytest.mark.parametrize("name", GC.OPTIMALITY + GC.HARD + GC.ILLCOND + GC.JACOBI)
def test_history_is_the_optimal_residual_and_the_iterate_the_restated_one(name, cgs2):
    """optimality (odd tails, pair loads, several blocks of partials; restarts on both sides of the 32-vector kernels),
    non-normal and indefinite operators, the ill-conditioned one, Jacobi from the left (op = D^-1 A)"""
    s, x = _solve(name, cgs2)
    _check_t1(name, s, x)


@ORTH
@pytest.mark.parametrize("name", GC.PARTS)
def test_three_row_parts_meet_the_same_bars(name, cgs2):
    """No existing partition test demands bit-equality of GMRES with the one-part run (the dot products of a partition are
    summed part by part), so the partitioned solve meets T1 / T1x like the one-part solve."""
    s, x = _solve(name, cgs2, parts=True)
    _check_t1(name, s, x)


@ORTH
@pytest.mark.parametrize("name", GC.TINY)
def test_tiny_systems_with_a_restart_longer_than_n(name, cgs2):
    c = GC.case(name)
    s, x = _solve(name, cgs2)
    _check_count(name, s, cgs2)
    assert s.converged
    assert s.last_iterations <= c["n"] + max(2, 0.02 * c["n"])
    _check_t2(name, x)


@ORTH
@pytest.mark.parametrize("name", GC.LUCKY)
def test_exact_breakdown_ends_the_solve(name, cgs2):
    """The Krylov space closes at step 20 (cyclic shift, b = e_1), 1 (identity) and 3 (three distinct eigenvalues): the new
    vector of that step is zero, H(j+1, j) = 0, the residual estimate 0, and the solve ends there as the oracle's does.
    Before the fix the low-synchronisation path put 1e-12 sqrt(t) in place of the zero norm, reported a residual of 1e-12,
    and -- with a tolerance below that -- ran on over a zero column."""
    c, r = GC.case(name), GC.reference(name)
    s, x = _solve(name, cgs2)
    assert r.it == c["expect_iterations"]
    _check_count(name, s, cgs2)
    assert s.converged
    _check_t2(name, x)


@ORTH
@pytest.mark.parametrize("name", GC.NEAR)
def test_a_small_new_vector_is_not_a_breakdown(name, cgs2):
    """Three eigenvalue clusters of width w = 1e-6 ... 1e-10: the new vector of step 4 is about w of A v and the residual
    there still about w |b|.  From 1e-8 down the difference t - uu of k_gmres_ls1 is cancellation noise, zero or negative,
    while the vector is 1e6 ... 1e8 roundings long: only the norm measured by the second pass can tell it from a closed
    Krylov space.  The solve goes on through it and takes the oracle's 9 (w = 1e-6) or 6 steps."""
    s, x = _solve(name, cgs2)
    _check_count(name, s, cgs2)
    assert s.converged
    _check_t2(name, x)


@ORTH
def test_stagnation_is_exact(cgs2):
    """GMRES(10) on the 20-cycle makes no progress at all: every Arnoldi vector is a unit vector, every number exact"""
    c = GC.case("stagnation")
    s, x = _solve("stagnation", cgs2)
    assert s.last_iterations == 40 and not s.converged
    assert np.array_equal(x, np.zeros(c["n"]))
    assert len(s.history) == 40 and np.array_equal(s.history, np.ones(40))
    assert s.res2 == 1.0


@ORTH
def test_initial_guess_and_device_tensors(cgs2):
    s, x = _solve("guess", cgs2)
    _check_count("guess", s, cgs2)
    assert s.converged
    _check_t2("guess", x)
    s2, x2 = _solve("guess", cgs2, on_device=True)
    assert s2.last_iterations == s.last_iterations and s2.res2 == s.res2
    assert np.array_equal(x2, x)


@ORTH
@pytest.mark.parametrize("name", GC.CAPS)
def test_reported_residual_is_the_true_one_at_a_cap(name, cgs2):
    """the cap before the end of the first cycle, at it, one step into the second, and in its middle"""
    c = GC.case(name)
    s, x = _solve(name, cgs2)
    gap = GC.t3_gap(name, x, s.res2)
    print(f"{name}: T3 {gap:.3e} (bar {8 * MEASURED_T3[name]:.3e})")
    assert s.last_iterations == c["cap"] and not s.converged
    assert gap <= 8 * MEASURED_T3[name]


@ORTH
def test_vcycle_from_the_left(cgs2):
    """op = M^-1 A with M^-1 the restated V-cycle, 5 steps (tol 1e-30).  That V-cycle is linear but runs in double precision,
    so the restated residual is itself known only to about n eps_double beta: the window ends at 1e-5 beta
    (gmres_cases.MG_WINDOW), not at sqrt(eps_double) beta, which 4 of the 5 steps are inside.  The oracle has no V-cycle to
    measure, so the bars are the 1e-8 (T1) and 1e-10 (T1x) of test_gmres; the step count is the cap, exactly."""
    c = GC.case("mg")
    s, x = _solve("mg", cgs2)
    dev, share, xdev = GC.compare("mg", x, s.history)
    print(f"mg: {s.last_iterations} iterations, T1 {dev:.3e}, share {share:.3f}, T1x {xdev:.3e}")
    assert s.last_iterations == c["cap"] == len(s.history) and not s.converged
    assert np.isfinite(x).all()
    assert share >= 0.8 and dev <= 1e-8
    assert xdev <= 1e-10


@ORTH
def test_a_residual_that_is_not_a_number_is_not_convergence(cgs2):
    """All-empty A, b = 1: A v_0 = 0, the rotation is 0 / 0.  The solve stops, is NOT converged, raises like a solve that hit
    its cap (check=False returns), and x is the last iterate that was a number: the initial guess."""
    c = GC.case("nan")
    s, x = _solve("nan", cgs2)
    assert not s.converged and np.isnan(s.res2)
    assert s.last_iterations == 1
    assert np.array_equal(x, c["x0"])
    A = _matrix(c)
    s = sg.gmres(c["tol"], c["restart"])
    s.set_option("gmres_cgs2", cgs2)
    s.set_max_iter(c["cap"])
    s.setup(A)
    with pytest.raises(sg.SigmaError) as e:
        s.solve(A, c["x0"].copy(), c["b"])
    assert e.value.code == 5
