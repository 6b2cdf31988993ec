"""The algebraic coarsening on the device (sgm_mat_aggregate, sgm_mg_aggregation_hierarchy) against the restated contract
(tests/aggregate_restated.py): aggregates integer for integer, prolongations bit for bit, the hierarchy inside the multigrid
preconditioner and CG, what the calls leave alone, and every refusal."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import aggregate_restated as AG
import algebra_restated as R
import mg_restated as MG
import sigma_amd as sg
from sigma_amd import problems as PB

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = AG.cases()
THETAS = (0.0, 0.08, 0.3)
OMEGA = 0.8
_hier = {}


@pytest.fixture(scope="module", autouse=True)
def _init():
    sg.init(0)


def _dev(m):
    nrow, ncol, ptr, node, val = m
    return sg.csr_matrix(nrow, ncol, np.asarray(ptr, np.int32), np.asarray(node, np.int32), np.asarray(val, np.float64))


def _host(M):
    return M.nrow, M.ncol, M.get("ptr", np.int32), M.get("node", np.int32), M.get("val", np.float64)


def restated_hierarchy(name, smooth_omega, min_coarse=8, theta=0.08):
    """computed once per (case, smooth_omega, min_coarse, theta), shared, never changed"""
    k = (name, smooth_omega, min_coarse, theta)
    if k not in _hier:
        _hier[k] = AG.hierarchy(CASES[name], theta, smooth_omega, 25, min_coarse)
    return _hier[k]


def _destroy(Ms):
    for M in Ms:
        M.destroy()


# ------------------------------------------------------------------ 1. the aggregates
@pytest.mark.parametrize("name", sorted(CASES))
def test_aggregates_equal_the_restatement(name):
    M = CASES[name]
    Ad = _dev(M)
    for theta in THETAS:
        want, nwant = AG.vectorised(M, theta)
        got, ngot = sg.aggregate(Ad, theta=theta)
        assert ngot == nwant, (name, theta)
        assert got.dtype == np.int32 and np.array_equal(got, want), (name, theta)
        dgot, dn = sg.aggregate(Ad, theta=theta, device=True)
        assert dn == nwant and np.array_equal(dgot.cpu().numpy(), want), (name, theta)
    Ad.destroy()


def test_the_default_theta_is_the_contracts():
    M = CASES["random_spd_300"]
    Ad = _dev(M)
    got, n = sg.aggregate(Ad)
    want, nwant = AG.vectorised(M, 0.08)
    assert n == nwant and np.array_equal(got, want)


# ------------------------------------------------------------------ 2. the hierarchy
# (the 27-point matrix has 27 on the diagonal and -1 beside it: at theta = 0.08 nothing is strong and the hierarchy is empty, on
#  both sides; theta = 0.03 is the run that coarsens its rows of 27 entries)
@pytest.mark.parametrize("name,theta", [(n, 0.08) for n in AG.HIERARCHY_CASES] + [("stencil27_9x8x8", 0.03)])
@pytest.mark.parametrize("smooth_omega", [0.0, 2.0 / 3.0])
def test_hierarchy_equals_the_restatement_level_by_level(name, theta, smooth_omega):
    want = restated_hierarchy(name, smooth_omega, theta=theta)
    Ad = _dev(CASES[name])
    got = sg.aggregation_hierarchy(Ad, theta=theta, smooth_omega=smooth_omega, max_levels=25, min_coarse=8)
    print(f"{name} theta {theta} smooth_omega {smooth_omega}: levels {[(P.nrow, P.ncol, P.nnz) for P in got]}")
    assert len(got) == len(want)
    assert len(want) >= 1 or (name, theta) == ("stencil27_9x8x8", 0.08)
    for l, (Pd, Pw) in enumerate(zip(got, want)):
        P = _host(Pd)
        assert (P[0], P[1]) == (Pw[0], Pw[1]), (name, l)
        assert np.array_equal(P[2], Pw[2]) and np.array_equal(P[3], Pw[3]), (name, l)
        assert np.array_equal(R.bits(P[4]), R.bits(Pw[4])), (name, l)
    _destroy(got)


def test_level_counts_and_stop_rules():
    name = "poisson_33x29"
    M = CASES[name]
    Ad = _dev(M)
    full = restated_hierarchy(name, 0.0)
    assert len(full) >= 2
    one = sg.aggregation_hierarchy(Ad, smooth_omega=0.0, max_levels=2, min_coarse=8)
    assert len(one) == 1 and R.same(_host(one[0]), full[0])
    two = sg.aggregation_hierarchy(Ad, smooth_omega=0.0, max_levels=3, min_coarse=8)
    assert len(two) == 2 and R.same(_host(two[1]), full[1])
    assert sg.aggregation_hierarchy(Ad, max_levels=1) == []
    assert sg.aggregation_hierarchy(Ad, min_coarse=M[0]) == []
    assert sg.aggregation_hierarchy(Ad, min_coarse=M[0] + 5) == []
    # min_coarse stops the descent at the first level that is small enough
    n1 = full[0][1]
    cut = sg.aggregation_hierarchy(Ad, smooth_omega=0.0, min_coarse=n1)
    assert len(cut) == 1
    Dd = _dev(CASES["diagonal_40"])                                  # no reduction: no level
    assert sg.aggregation_hierarchy(Dd, min_coarse=8) == []
    _destroy(one + two + cut)


def test_the_default_arguments_are_the_documented_ones():
    name = "poisson_100x70"
    Ad = _dev(CASES[name])
    got = sg.aggregation_hierarchy(Ad)
    want = restated_hierarchy(name, 2.0 / 3.0, 64)
    assert len(got) == len(want)
    for Pd, Pw in zip(got, want):
        assert R.same(_host(Pd), Pw)
    _destroy(got)


# ------------------------------------------------------------------ 3. inside the preconditioner and CG
@pytest.mark.parametrize("name,smooth_omega,theta", [("poisson_33x29", 0.0, 0.08), ("poisson_33x29", 2.0 / 3.0, 0.08),
                                                     ("random_spd_300", 2.0 / 3.0, 0.08), ("stencil27_9x8x8", 0.0, 0.03)])
def test_the_multigrid_on_the_hierarchy_applies_like_the_restatement(name, smooth_omega, theta):
    A = CASES[name]
    want_P = restated_hierarchy(name, smooth_omega, theta=theta)
    assert len(want_P) >= 1
    Ad = _dev(A)
    Pd = sg.aggregation_hierarchy(Ad, theta=theta, smooth_omega=smooth_omega, min_coarse=8)
    pc = sg.multigrid(Pd, omega=OMEGA)
    pc.setup(Ad)
    want = MG.Vectorised(A, want_P, OMEGA, 1, 1, 8)
    assert pc.levels == len(want_P) + 1
    rs = np.random.RandomState(5)
    for r in (PB.test_vector(A[0]), rs.standard_normal(A[0])):
        z = np.zeros(A[0])
        pc.solve(Ad, z, r)
        assert np.array_equal(R.bits(z), R.bits(want.apply(r))), name
    pc.destroy()
    _destroy(Pd)


@pytest.mark.parametrize("smooth_omega", [0.0, 2.0 / 3.0])
def test_cg_with_the_hierarchy_equals_cg_with_the_restated_p_uploaded_by_hand(smooth_omega):
    name = "poisson_100x70"
    A = CASES[name]
    rows = MG._Rows(A)
    b = rows.matvec(PB.test_vector(A[0]))
    want_P = restated_hierarchy(name, smooth_omega, 64)

    def solve(Pd):
        Ad = _dev(A)
        pc = sg.multigrid(Pd, omega=OMEGA)
        pc.setup(Ad)
        solver = sg.cg(1e-10)
        solver.setup(Ad)
        x = np.zeros(A[0])
        solver.solve(Ad, x, b, pc)
        return x, solver.iterations

    Ad = _dev(A)
    mine = sg.aggregation_hierarchy(Ad, smooth_omega=smooth_omega)
    x1, it1 = solve(mine)
    x2, it2 = solve([_dev(P) for P in want_P])
    mg = MG.Vectorised(A, want_P, OMEGA, 1, 1, 8)
    _, it_cpu, _ = MG.pcg(rows, b, mg.apply, tol=1e-10)
    print(f"smooth_omega {smooth_omega}: device {it1} / {it2} iterations, restated {it_cpu}")
    assert it1 == it2 and np.array_equal(R.bits(x1), R.bits(x2))
    assert abs(it1 - it_cpu) <= 2
    _destroy(mine)


# ------------------------------------------------------------------ 4. what the calls leave alone
def test_a_is_unchanged_by_either_call():
    M = CASES["random_skew_128"]
    Ad = _dev(M)
    before = Ad.get("versions", np.int64).copy()
    sg.aggregate(Ad, theta=0.08)
    Ps = sg.aggregation_hierarchy(Ad, min_coarse=8)
    assert len(Ps) >= 1
    assert np.array_equal(Ad.get("versions", np.int64), before)
    got = _host(Ad)
    assert np.array_equal(got[2], M[2]) and np.array_equal(got[3], M[3]) and np.array_equal(R.bits(got[4]), R.bits(M[4]))
    y0, y1 = np.zeros(M[0]), np.zeros(M[0])
    x = PB.test_vector(M[0])
    _dev(M).matvec(x, y0)
    Ad.matvec(x, y1)
    assert np.array_equal(R.bits(y0), R.bits(y1))
    _destroy(Ps)


def test_the_prolongations_outlive_a():
    name = "laplace3d_8x7x6"
    want = restated_hierarchy(name, 2.0 / 3.0)
    Ad = _dev(CASES[name])
    Ps = sg.aggregation_hierarchy(Ad, min_coarse=8)
    Ad.destroy()
    for Pd, Pw in zip(Ps, want):
        assert R.same(_host(Pd), Pw)
        y = np.zeros(Pd.nrow)
        Pd.matvec(np.ones(Pd.ncol), y)
        assert np.isfinite(y).all()
    _destroy(Ps)


# ------------------------------------------------------------------ 5. refusals
def _raw_hierarchy(h, theta=0.08, smooth_omega=2.0 / 3.0, max_levels=25, min_coarse=8, null_p=False, null_n=False):
    slots = (C.c_void_p * 32)()
    made = C.c_int32(-7)
    rc = sg.lib().sgm_mg_aggregation_hierarchy(h, C.c_double(theta), C.c_double(smooth_omega), C.c_int32(max_levels),
                                               C.c_int32(min_coarse), None if null_p else slots, None if null_n else C.byref(made))
    assert all(not s for s in slots), "a refused call created a matrix"
    return rc


def _raw_aggregate(h, n, theta=0.08, null_agg=False, null_n=False):
    agg = np.full(max(n, 1), -5, np.int32)
    nagg = C.c_int32(-7)
    rc = sg.lib().sgm_mat_aggregate(h, C.c_double(theta), None if null_agg else C.c_void_p(agg.ctypes.data),
                                    None if null_n else C.byref(nagg), C.c_int(0))
    assert (agg == -5).all() and nagg.value == -7, "a refused call wrote its outputs"
    return rc


def test_every_refusal_returns_its_code_and_creates_nothing():
    M = CASES["poisson_33x29"]
    n = M[0]
    Ad = _dev(M)
    BAD_ARG, DIMS, UNSUPPORTED = 1, 2, 8
    rect = _dev((3, 4, np.array([1, 2, 3, 4], np.int32), np.array([1, 2, 4], np.int32), np.ones(3)))
    assert _raw_aggregate(rect._h, 3) == DIMS
    assert _raw_hierarchy(rect._h) == DIMS
    ell = sg.ellpack_matrix(n, n, np.arange(1, n + 1, dtype=np.int32).reshape(n, 1), np.ones((n, 1)))
    part = sg.partitioned_csr_matrix(n, n, M[2], M[3], M[4], np.array([0, 512, n], np.int64))
    comp = sg.sparse_matrix(np.array([1, n + 1], np.int32), np.array([1, n + 1], np.int32))
    comp.set_submatrix(1, 1, Ad)
    for other in (ell, part, comp):
        if hasattr(other, "_build"):
            other._build()
        assert _raw_aggregate(other._h, n) == UNSUPPORTED
        assert _raw_hierarchy(other._h) == UNSUPPORTED
    for theta in (-0.1, float("nan")):
        assert _raw_aggregate(Ad._h, n, theta=theta) == BAD_ARG
        assert _raw_hierarchy(Ad._h, theta=theta) == BAD_ARG
    for om in (-1.0, float("nan"), float("inf")):
        assert _raw_hierarchy(Ad._h, smooth_omega=om) == BAD_ARG
    assert _raw_hierarchy(Ad._h, max_levels=0) == BAD_ARG
    assert _raw_hierarchy(Ad._h, min_coarse=0) == BAD_ARG
    assert _raw_hierarchy(Ad._h, null_p=True) == BAD_ARG
    assert _raw_hierarchy(Ad._h, null_n=True) == BAD_ARG
    assert _raw_hierarchy(None) == BAD_ARG
    assert _raw_aggregate(Ad._h, n, null_agg=True) == BAD_ARG
    assert _raw_aggregate(Ad._h, n, null_n=True) == BAD_ARG
    assert _raw_aggregate(None, n) == BAD_ARG
    with pytest.raises(sg.SigmaError) as e:                          # the Python surface raises with the code
        sg.aggregation_hierarchy(Ad, theta=-1.0)
    assert e.value.code == BAD_ARG
    # A still works after all of that
    got, nagg = sg.aggregate(Ad)
    want, nwant = AG.vectorised(M, 0.08)
    assert nagg == nwant and np.array_equal(got, want)


# ------------------------------------------------------------------ 6. the Fortran host layer
def test_fortran_program_builds_the_same_hierarchy_and_solves_with_the_same_iteration_count():
    exe = os.path.join(ROOT, "sigma_amd", "fortran", "aggregate_test_hip")
    if not os.path.exists(exe):
        pytest.skip("sigma_amd/fortran/aggregate_test_hip was not built (no amdflang at build time)")
    A, _ = MG.poisson_case(63, 63)
    rows = MG._Rows(A)
    b = rows.matvec(PB.test_vector(A[0]))
    Ad = _dev(A)
    Ps = sg.aggregation_hierarchy(Ad, theta=0.08, smooth_omega=2.0 / 3.0, max_levels=25, min_coarse=64)
    pc = sg.multigrid(Ps, omega=OMEGA)
    pc.setup(Ad)
    solver = sg.cg(1e-10)
    solver.setup(Ad)
    x = np.zeros(A[0])
    solver.solve(Ad, x, b, pc)
    sizes = " ".join(str(v) for v in [A[0]] + [P.ncol for P in Ps])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout.replace("\n ", "")
    assert "aggregate_test_hip: ok" in out, r.stdout
    found = re.search(r"level sizes\s+([\d ]+)", out)
    assert found and " ".join(found.group(1).split()) == sizes, (r.stdout, sizes)
    found = re.search(r"V\(1,1\)-PCG iterations\s+(\d+)", out)
    assert found and int(found.group(1)) == solver.iterations, (r.stdout, solver.iterations)
    _destroy(Ps)
