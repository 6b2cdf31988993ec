"""Multigrid's direct coarse solve on the device (option "mg_coarse_direct"): the inverse and the pivots
setup computes, one apply, a second setup and the switch between the two coarse treatments equal the restated contract
(tests/mg_direct_restated.py) bit for bit; the Krylov solvers reach it; every refusal returns its code; and with the option
at its default nothing changes."""
import numpy as np
import pytest

import algebra_restated as R
import mg_direct_restated as DR
import mg_restated as MG
import sigma_amd as sg
from sigma_amd import problems as PB

pytestmark = pytest.mark.gpu
OMEGA = 0.8
BAD_ARG, UNSUPPORTED = 1, 8


@pytest.fixture(scope="module", autouse=True)
def _init():
    sg.init(0)


def _dev(m):
    nrow, ncol, ptr, node, val = m
    return sg.csr_matrix(nrow, ncol, np.asarray(ptr, np.int32), np.asarray(node, np.int32), np.asarray(val, np.float64))


def _host(M):
    return M.nrow, M.ncol, M.get("ptr", np.int32), M.get("node", np.int32), M.get("val", np.float64)


_cases = DR.cases()
_cache = {}


def _poisson_case():
    """64 x 64 Poisson with the device's two-level smoothed aggregation: 578 coarse rows -- three chunks, the last block a
    partial wave"""
    A = DR.poisson(64, 64)
    Pd = sg.aggregation_hierarchy(_dev(A), max_levels=2)
    assert len(Pd) == 1
    return A, [_host(Pd[0])]


def case(name):
    """(A, Ps, the restated V-cycle with the direct coarse level): computed once, shared, never changed"""
    if name not in _cache:
        A, Ps = _poisson_case() if name == "poisson64" else _cases[name]
        _cache[name] = (A, Ps, DR.Vectorised(A, Ps, OMEGA, 1, 1))
    return _cache[name]


NAMES = list(_cases) + ["poisson64"]


def _pc(Ad, Pd, coarse="direct", **kw):
    pc = sg.multigrid(Pd, omega=OMEGA, coarse=coarse, **kw)
    pc.setup(Ad)
    return pc


def test_the_poisson_case_crosses_two_chunk_boundaries_and_ends_in_a_partial_wave():
    n = case("poisson64")[2].D.shape[0]
    assert n > 512 and n % 64 != 0, n


# ------------------------------------------------------------------ 1. + 2. inverse, pivots, one apply
@pytest.mark.parametrize("name", NAMES)
def test_inverse_pivots_and_one_apply_equal_the_restatement_bit_for_bit(name):
    import torch
    A, Ps, want = case(name)
    n = A[0]
    Ad, Pd = _dev(A), [_dev(P) for P in Ps]
    pc = _pc(Ad, Pd)
    inv, piv = pc.coarse_inverse(), pc.coarse_pivots()
    nL = want.D.shape[0]
    assert inv.shape == (nL, nL) and piv.dtype == np.int32
    print(f"{name}: coarse level of {nL} rows, max |Ainv - restated| = {np.abs(inv - want.Ainv).max():.3e}")
    assert np.array_equal(piv, want.piv)
    assert np.array_equal(R.bits(inv), R.bits(want.Ainv))
    assert pc.info()["name"].endswith(f"direct coarse solve ({nL} rows)")
    assert pc.info()["levels"] == (len(Ps) + 1, len(Ps) + 1)
    rs = np.random.RandomState(11)
    for r in (PB.test_vector(n), rs.standard_normal(n)):
        w = want.apply(r)
        z = np.zeros(n)
        pc.solve(Ad, z, r)
        assert np.array_equal(R.bits(z), R.bits(w)), (name, np.abs(z - w).max())
    r = PB.test_vector(n)
    w = want.apply(r)
    rt = torch.from_numpy(r).cuda()
    zt = torch.zeros(n, dtype=torch.float64, device="cuda")
    pc.solve(Ad, zt, rt)
    assert np.array_equal(R.bits(zt.cpu().numpy()), R.bits(w))
    zt.copy_(rt)                                                 # in place
    pc.solve(Ad, zt, zt)
    assert np.array_equal(R.bits(zt.cpu().numpy()), R.bits(w))
    pc.destroy()


def test_the_pivoting_case_swaps_and_the_tie_takes_the_smaller_index():
    assert case("pivoting")[2].piv.tolist() == [2, 2, 3]
    A, Ps, _ = case("pivoting")
    assert _pc(_dev(A), [_dev(P) for P in Ps]).coarse_pivots().tolist() == [2, 2, 3]
    A, Ps, _ = case("tie_L0")
    assert _pc(_dev(A), []).coarse_pivots()[0] == 2


# ------------------------------------------------------------------ 3. solves
_solve = {}


def _restated_pcg():
    if not _solve:
        A, Ps, want = case("poisson64")
        rows = MG._Rows(A)
        b = rows.matvec(PB.test_vector(A[0]))
        _, it, _ = MG.pcg(rows, b, want.apply, tol=1e-10)
        _solve["v"] = (b, it)
    return _solve["v"]


def _device_solve(solver, with_pc=True):
    A, Ps, _ = case("poisson64")
    b, _ = _restated_pcg()
    Ad, Pd = _dev(A), [_dev(P) for P in Ps]
    pc = _pc(Ad, Pd) if with_pc else None
    solver.setup(Ad)
    x = np.zeros(A[0])
    solver.solve(Ad, x, b, pc)
    return x, solver.iterations


def test_cg_with_the_direct_coarse_level_takes_the_restated_iteration_count():
    A = case("poisson64")[0]
    _, it_restated = _restated_pcg()
    x, it = _device_solve(sg.cg(1e-10))
    err = np.abs(x - PB.test_vector(A[0])).max()
    print(f"64^2: PCG {it} iterations with the direct coarse level (restated {it_restated}), max |x - x*| = {err:.3e}")
    assert abs(it - it_restated) <= 1
    assert err <= 1e-9


@pytest.mark.parametrize("make", [lambda: sg.bicgstab(1e-10), lambda: sg.gmres(1e-10, 30)], ids=["bicgstab", "gmres30"])
def test_bicgstab_and_gmres_converge_faster_with_the_direct_coarse_level(make):
    A = case("poisson64")[0]
    x, it = _device_solve(make())
    _, it_plain = _device_solve(make(), with_pc=False)
    print(f"64^2: {it} iterations with the V-cycle and the direct coarse level, {it_plain} without")
    assert it < it_plain
    assert np.abs(x - PB.test_vector(A[0])).max() <= 1e-8


# ------------------------------------------------------------------ 4. second setup, switching the option
def test_second_setup_inverts_the_new_values_and_the_option_switches_between_setups():
    A, Ps, want = case("spd75")
    n = A[0]
    Ad, Pd = _dev(A), [_dev(P) for P in Ps]
    pc = _pc(Ad, Pd)
    assert np.array_equal(R.bits(pc.coarse_inverse()), R.bits(want.Ainv))
    handle = pc.level_handle(1)._h.value
    val2 = A[4] * (1.0 + 0.25 * np.cos(np.arange(len(A[4]))))
    val2[np.asarray(A[3]) == np.repeat(np.arange(1, n + 1), np.diff(A[2]))] += 1.0       # keep the diagonal dominant
    Ad.set_values(val2)
    pc.setup(Ad)
    A2 = (n, n, A[2], A[3], val2)
    want2 = DR.Vectorised(A2, Ps, OMEGA, 1, 1)
    assert pc.level_handle(1)._h.value == handle                                        # refilled, not rebuilt
    assert np.array_equal(R.bits(pc.coarse_inverse()), R.bits(want2.Ainv))
    assert np.array_equal(pc.coarse_pivots(), want2.piv)
    assert not np.array_equal(want2.Ainv, want.Ainv)
    r = PB.test_vector(n)
    z = np.zeros(n)
    pc.solve(Ad, z, r)
    assert np.array_equal(R.bits(z), R.bits(want2.apply(r)))
    # off: the sweeps of the existing path, and nothing to read back
    pc.set_option("mg_coarse_direct", 0)
    pc.setup(Ad)
    pc.solve(Ad, z, r)
    assert np.array_equal(R.bits(z), R.bits(MG.Vectorised(A2, Ps, OMEGA, 1, 1, 8, lev=want2.lev).apply(r)))
    assert pc.info()["name"].endswith("8 coarse sweeps")
    with pytest.raises(sg.SigmaError) as e:
        pc.coarse_inverse()
    assert e.value.code == BAD_ARG
    # on again
    pc.set_option("mg_coarse_direct", 1)
    pc.setup(Ad)
    assert np.array_equal(R.bits(pc.coarse_inverse()), R.bits(want2.Ainv))
    pc.solve(Ad, z, r)
    assert np.array_equal(R.bits(z), R.bits(want2.apply(r)))


# ------------------------------------------------------------------ 5. refusals
def test_a_coarse_level_above_the_limit_is_refused_with_the_limit_in_the_message():
    n = 4097
    Ad = _dev((n, n, np.arange(1, n + 2), np.arange(1, n + 1), np.full(n, 2.0)))
    Pd = [_dev(MG.piecewise_constant(n, width=1))]
    pc = sg.multigrid(Pd, omega=OMEGA, coarse="direct")
    with pytest.raises(sg.SigmaError) as e:
        pc.setup(Ad)
    assert e.value.code == UNSUPPORTED, str(e.value)
    assert "4097" in str(e.value) and "4096" in str(e.value)
    with pytest.raises(sg.SigmaError):
        pc.solve(Ad, np.zeros(n), np.ones(n))
    pc.set_option("mg_coarse_direct", 0)                         # the same handle with the sweeps: set up and usable
    pc.setup(Ad)
    z = np.zeros(n)
    pc.solve(Ad, z, np.ones(n))
    assert np.isfinite(z).all()


def test_a_singular_coarse_level_is_refused_and_the_message_names_the_step():
    A = DR.poisson(5, 5)
    n, nc, ptr, node, val = MG.piecewise_constant(25, width=9)   # 3 columns in use ...
    P = (n, nc + 1, ptr, node, val)                              # ... and an empty fourth: row and column 4 of P^T A P are empty
    with pytest.raises(DR.Refused) as r:
        DR.Vectorised(A, [P], OMEGA, 1, 1)
    assert r.value.step == 4
    Ad, Pd = _dev(A), [_dev(P)]
    pc = sg.multigrid(Pd, omega=OMEGA, coarse="direct")
    with pytest.raises(sg.SigmaError) as e:
        pc.setup(Ad)
    assert e.value.code == UNSUPPORTED, str(e.value)
    assert "singular or non-finite coarse level" in str(e.value) and "step 4" in str(e.value)
    z = np.zeros(n)
    with pytest.raises(sg.SigmaError):                           # nothing to apply until a setup succeeds
        pc.solve(Ad, z, np.ones(n))
    with pytest.raises(sg.SigmaError):
        pc.coarse_pivots()
    P3 = MG.piecewise_constant(25, width=9)
    pc3 = _pc(Ad, [_dev(P3)])                                    # the same level without the empty column sets up
    pc3.solve(Ad, z, np.ones(n))
    assert np.array_equal(R.bits(z), R.bits(DR.Vectorised(A, [P3], OMEGA, 1, 1).apply(np.ones(n))))
    pc.destroy()


def test_the_option_and_the_arrays_belong_to_multigrid_with_the_option_on():
    A, Ps, _ = case("spd19")
    Ad, Pd = _dev(A), [_dev(P) for P in Ps]
    jac = sg.jacobi()
    jac.setup(Ad)
    with pytest.raises(sg.SigmaError) as e:
        jac.set_option("mg_coarse_direct", 1)
    assert e.value.code == BAD_ARG
    pc = _pc(Ad, Pd, coarse="sweeps")
    for name, dt in (("mg_coarse_inverse", np.float64), ("mg_coarse_pivots", np.int32)):
        with pytest.raises(sg.SigmaError) as e:
            pc.get(name, dt)
        assert e.value.code == BAD_ARG
    with pytest.raises(ValueError):
        sg.multigrid(Pd, omega=OMEGA, coarse="lu")


# ------------------------------------------------------------------ 6. the default is the existing path
def test_with_the_option_at_its_default_info_and_one_apply_are_the_sweeps():
    A, Ps, want = case("poisson64")
    Ad, Pd = _dev(A), [_dev(P) for P in Ps]
    pc = sg.multigrid(Pd, omega=OMEGA)
    pc.setup(Ad)
    info = pc.info()
    assert info["name"] == "V(1,1) omega 0.8, 2 levels, 8 coarse sweeps"
    assert info["levels"] == (2, 2) and info["path"] == 5 and info["colours"] == 0
    r = PB.test_vector(A[0])
    z = np.zeros(A[0])
    pc.solve(Ad, z, r)
    assert np.array_equal(R.bits(z), R.bits(MG.Vectorised(A, Ps, OMEGA, 1, 1, 8, lev=want.lev).apply(r)))


# ------------------------------------------------------------------ 7. the Fortran host layer
def test_fortran_program_goes_through_coarse_direct_with_the_same_iteration_count():
    import os
    import re
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sigma_amd", "fortran", "mg_direct_test_hip")
    if not os.path.exists(exe):
        pytest.skip("sigma_amd/fortran/mg_direct_test_hip was not built (no amdflang at build time)")
    A, Ps = MG.poisson_case(63, 63)
    Ps = Ps[:2]                                                  # 63 -> 32 -> 16: the descent stops at 256 rows
    Ad, Pd = _dev(A), [_dev(P) for P in Ps]
    b = MG._Rows(A).matvec(PB.test_vector(A[0]))
    its = {}
    for coarse in ("direct", "sweeps"):
        solver = sg.cg(1e-10)
        solver.setup(Ad)
        solver.solve(Ad, np.zeros(A[0]), b, _pc(Ad, Pd, coarse=coarse))
        its[coarse] = solver.iterations
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout.replace("\n ", "")
    assert "mg_direct_test_hip: ok" in out, r.stdout
    assert "direct coarse solve (256 rows)" in out
    for key, word in (("direct", "direct"), ("sweeps", "8-sweep")):
        found = re.search(word + r" PCG iterations\s+(\d+)", out)
        assert found and int(found.group(1)) == its[key], (r.stdout, its)
