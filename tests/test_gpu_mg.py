"""The multigrid preconditioner on the device (sgm_mg_create): one V-cycle apply equals the restated contract
(tests/mg_restated.py) bit for bit on the fused and on the unfused path, the levels are sgm_mat_ptap's, the Krylov solvers
reach it, a second setup refills, and every refusal returns its code."""
import os
import re
import subprocess

import numpy as np
import pytest

import algebra_restated as R
import mg_restated as MG
import sigma_amd as sg
from sigma_amd import problems as PB

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = [(1, 1, 8), (2, 2, 1), (3, 0, 2)]
OMEGA = 0.8


@pytest.fixture(scope="module", autouse=True)
def _init():
    sg.init(0)


def _dev(m):
    nrow, ncol, ptr, node, val = m
    return sg.csr_matrix(nrow, ncol, np.asarray(ptr, np.int32), np.asarray(node, np.int32), np.asarray(val, np.float64))


def _laplace3d_case():
    ptr, node, val = PB.laplace3d_csr(8, 7, 6)
    return (336, 336, ptr, node, val), []


CASES = {
    "poisson31": lambda: MG.poisson_case(31, 31),
    "poisson33x29": lambda: MG.poisson_case(33, 29),
    "poisson100x70": lambda: MG.poisson_case(100, 70),
    "random_spd": lambda: MG.random_spd_case(300),
    "laplace3d_L0": _laplace3d_case,
    "stencil27": lambda: MG.stencil27_case(9, 8, 8),
}
_cache = {}


def case(name):
    """(A, Ps, levels) of a case: computed once, shared, never changed"""
    if name not in _cache:
        A, Ps = CASES[name]()
        _cache[name] = (A, Ps, MG.levels(A, Ps))
    return _cache[name]


def _pc(Ad, Pd, nu_pre=1, nu_post=1, coarse=8, omega=OMEGA):
    pc = sg.multigrid(Pd, omega=omega, nu_pre=nu_pre, nu_post=nu_post, coarse_sweeps=coarse)
    pc.setup(Ad)
    return pc


# ------------------------------------------------------------------ 1. one apply, bit for bit
@pytest.mark.parametrize("name", list(CASES))
def test_one_apply_equals_the_restatement_bit_for_bit(name):
    import torch
    A, Ps, lev = case(name)
    n = A[0]
    Ad, Pd = _dev(A), [_dev(P) for P in Ps]
    rs = np.random.RandomState(11)
    rhs = (PB.test_vector(n), rs.standard_normal(n))
    if name == "stencil27":         # the case exists to run the 27-wide fused kernels: say so when the layout stops being that
        assert Ad.kernel == "k_csr_slb<W=27>"
    for nu_pre, nu_post, coarse in PARAMS:
        pc = _pc(Ad, Pd, nu_pre, nu_post, coarse)
        want = MG.Vectorised(A, Ps, OMEGA, nu_pre, nu_post, coarse, lev=lev)
        for k, r in enumerate(rhs):
            w = want.apply(r)
            z = np.zeros(n)
            pc.solve(Ad, z, r)                                   # host vectors
            diff = np.abs(z - w).max()
            print(f"{name} V({nu_pre},{nu_post}) coarse {coarse} rhs {k}: paths {pc.paths().tolist()}, max |z - restated| = {diff:.3e}")
            assert np.array_equal(R.bits(z), R.bits(w)), (name, nu_pre, nu_post, coarse, k, diff)
        rt = torch.from_numpy(rhs[0]).cuda()                     # device vectors
        zt = torch.zeros(n, dtype=torch.float64, device="cuda")
        pc.solve(Ad, zt, rt)
        assert np.array_equal(R.bits(zt.cpu().numpy()), R.bits(want.apply(rhs[0])))
        zt.copy_(rt)                                             # in place: r and z the same device vector
        pc.solve(Ad, zt, zt)
        assert np.array_equal(R.bits(zt.cpu().numpy()), R.bits(want.apply(rhs[0])))
        if name == "stencil27":
            assert pc.paths()[0] == 2
        pc.destroy()


# ------------------------------------------------------------------ 2. levels and inverse diagonals
@pytest.mark.parametrize("name", ["poisson100x70", "random_spd", "laplace3d_L0"])
def test_level_matrices_and_inverse_diagonals_are_the_restated_ones(name):
    A, Ps, lev = case(name)
    Ad, Pd = _dev(A), [_dev(P) for P in Ps]
    pc = _pc(Ad, Pd)
    want = MG.Vectorised(A, Ps, OMEGA, 1, 1, 8, lev=lev)
    assert pc.levels == len(lev)
    for l, M in enumerate(lev):
        got = pc.level_matrix(l)
        assert (got[0], got[1]) == (M[0], M[1])
        assert np.array_equal(got[2], M[2]) and np.array_equal(got[3], M[3])
        assert np.array_equal(R.bits(got[4]), R.bits(M[4]))
        assert np.array_equal(R.bits(pc.idiag(l)), R.bits(want.idiag[l]))
    info = pc.info()
    assert info["name"] == f"V(1,1) omega 0.8, {len(lev)} level{'s' if len(lev) > 1 else ''}, 8 coarse sweeps"
    assert info["levels"] == (len(lev), len(lev)) and info["est_us"] > 0.0
    with pytest.raises(sg.SigmaError):
        pc.get(f"mg_idiag_{len(lev)}", np.float64)
    with pytest.raises(sg.SigmaError):
        pc.level_matrix(len(lev))


# ------------------------------------------------------------------ 3. which path serves which level
def test_paths_follow_the_layout_of_every_level():
    A, Ps, lev = case("poisson100x70")
    Ad, Pd = _dev(A), [_dev(P) for P in Ps]
    pc = _pc(Ad, Pd)
    paths = pc.paths()
    kernels = [pc.level_handle(l).kernel for l in range(len(lev))]
    print("poisson100x70 paths", paths.tolist(), kernels)
    assert len(paths) == len(lev) and paths[0] == 1 and kernels[0].startswith("k_csr_sl<")
    for l in range(1, len(lev)):
        if kernels[l].startswith("k_csr_slb<"):
            assert paths[l] == 2, (l, kernels[l])
        elif not kernels[l].startswith("k_csr_sl<"):
            assert paths[l] == 0, (l, kernels[l])
    assert 2 in paths[1:].tolist(), "no Galerkin level of the 100 x 70 hierarchy took the 1-byte sliced form"
    A2, Ps2, _ = case("random_spd")
    Ad2, Pd2 = _dev(A2), [_dev(P) for P in Ps2]
    pc2 = _pc(Ad2, Pd2)
    assert pc2.paths().tolist() == [0, 0, 0]
    # the layout decides at every apply: with the sliced kernels switched off the same bits come from the composition
    r = PB.test_vector(A[0])
    z1, z2 = np.zeros(A[0]), np.zeros(A[0])
    pc.solve(Ad, z1, r)
    Ad.set_option("csr_sliced", 0)
    assert pc.paths()[0] == 0
    pc.solve(Ad, z2, r)
    assert np.array_equal(R.bits(z1), R.bits(z2))


# ------------------------------------------------------------------ 4. solves
_solves = {}


def _restated_pcg(nx):
    if nx not in _solves:
        A, Ps = MG.poisson_case(nx, nx)
        rows = MG._Rows(A)
        b = rows.matvec(PB.test_vector(A[0]))
        vc = MG.Vectorised(A, Ps, OMEGA, 1, 1, 8)
        _, it, _ = MG.pcg(rows, b, vc.apply, tol=1e-10)
        _solves[nx] = (A, Ps, b, it)
    return _solves[nx]


def _device_solve(solver, A, Ps, b, with_pc=True):
    Ad, Pd = _dev(A), [_dev(P) for P in Ps]
    pc = _pc(Ad, Pd) if with_pc else None
    solver.setup(Ad)
    x = np.zeros(A[0])
    solver.solve(Ad, x, b, pc)
    return x, solver.iterations


def test_cg_with_the_vcycle_converges_in_a_grid_independent_handful_of_iterations():
    counts = []
    for nx in (63, 127, 255):
        A, Ps, b, it_restated = _restated_pcg(nx)
        x, it = _device_solve(sg.cg(1e-10), A, Ps, b)
        err = np.abs(x - PB.test_vector(A[0])).max()
        print(f"{nx}^2: V(1,1)-PCG {it} iterations (restated {it_restated}), max |x - x*| = {err:.3e}")
        assert abs(it - it_restated) <= 1
        assert it <= 14
        assert err <= 1e-9
        counts.append(it)
    assert max(counts) - min(counts) <= 2
    A, Ps, b, _ = _restated_pcg(255)
    _, it_plain = _device_solve(sg.cg(1e-10), A, Ps, b, with_pc=False)
    print(f"255^2: plain CG {it_plain} iterations")
    assert it_plain >= 10 * counts[-1]


@pytest.mark.parametrize("make", [lambda: sg.bicgstab(1e-10), lambda: sg.gmres(1e-10, 30)], ids=["bicgstab", "gmres30"])
def test_bicgstab_and_gmres_converge_faster_with_the_vcycle(make):
    A, Ps, b, _ = _restated_pcg(127)
    x, it = _device_solve(make(), A, Ps, b)
    _, it_plain = _device_solve(make(), A, Ps, b, with_pc=False)
    print(f"127^2: {it} iterations with the V-cycle, {it_plain} without")
    assert it < it_plain
    assert np.abs(x - PB.test_vector(A[0])).max() <= 1e-8


def test_cg_in_the_references_dot_order_converges_with_the_vcycle():
    A, Ps, b, _ = _restated_pcg(63)
    solver = sg.cg(1e-10)
    solver.set_option("dot_order", 1)
    x, it = _device_solve(solver, A, Ps, b)
    assert it <= 14
    assert np.abs(x - PB.test_vector(A[0])).max() <= 1e-9


# ------------------------------------------------------------------ 5. second setup
def test_second_setup_refills_and_a_changed_pattern_rebuilds():
    A, Ps, lev = case("poisson33x29")
    n = A[0]
    Ad, Pd = _dev(A), [_dev(P) for P in Ps]
    pc = _pc(Ad, Pd)
    idiag = [pc.idiag(l) for l in range(len(lev))]
    handles = [pc.level_handle(l)._h.value for l in range(len(lev))]
    rows = [pc.level_handle(l).algebra_rows() for l in range(1, len(lev))]
    Ad.scalar_multiply(2.0)
    pc.setup(Ad)
    A2 = (n, n, A[2], A[3], 2.0 * A[4])
    want = MG.Vectorised(A2, Ps, OMEGA, 1, 1, 8)
    for l in range(len(lev)):
        assert np.array_equal(R.bits(pc.idiag(l)), R.bits(0.5 * idiag[l]))
        assert np.array_equal(R.bits(pc.level_matrix(l)[4]), R.bits(want.lev[l][4]))
    assert [pc.level_handle(l)._h.value for l in range(len(lev))] == handles          # refilled, not rebuilt
    assert [pc.level_handle(l).algebra_rows() for l in range(1, len(lev))] == rows
    r = PB.test_vector(n)
    z = np.zeros(n)
    pc.solve(Ad, z, r)
    assert np.array_equal(R.bits(z), R.bits(want.apply(r)))
    # a changed pattern: rows rotated by one.  Either a refusal with a message, or levels of the matrix as it is now
    p = np.roll(np.arange(1, n + 1, dtype=np.int32), 1)
    Ad.left_permute(p)
    A3 = (n, n, Ad.get("ptr", np.int32), Ad.get("node", np.int32), Ad.get("val", np.float64))
    try:
        pc.setup(Ad)
    except sg.SigmaError as e:
        assert str(e)
        with pytest.raises(sg.SigmaError):
            pc.solve(Ad, z, r)
        return
    want3 = MG.Vectorised(A3, Ps, OMEGA, 1, 1, 8)
    for l in range(len(lev)):
        got = pc.level_matrix(l)
        assert np.array_equal(got[2], want3.lev[l][2]) and np.array_equal(got[3], want3.lev[l][3])
        assert np.array_equal(R.bits(got[4]), R.bits(want3.lev[l][4]))
        assert np.array_equal(R.bits(pc.idiag(l)), R.bits(want3.idiag[l]))
    pc.solve(Ad, z, r)
    assert np.array_equal(R.bits(z), R.bits(want3.apply(r)))


# ------------------------------------------------------------------ 6. refusals
def _refused(pc, Ad, code, word=None):
    with pytest.raises(sg.SigmaError) as e:
        pc.setup(Ad)
    assert e.value.code == code, str(e.value)
    if word:
        assert word in str(e.value), str(e.value)
    n = max(Ad.nrow, 1)
    with pytest.raises(sg.SigmaError):                           # unusable ...
        pc.solve(Ad, np.zeros(n), np.ones(n))
    pc.destroy()                                                 # ... but destroyable


def test_every_refusal_returns_its_code():
    A, Ps, _ = case("poisson31")
    B, Qs, _ = case("poisson33x29")
    Ad, Bd = _dev(A), _dev(B)
    Pd, Qd = [_dev(P) for P in Ps], [_dev(Q) for Q in Qs]
    mk = lambda P: sg.multigrid(P, omega=OMEGA)      # noqa: E731
    # SGM_ERR_DIMS = 2
    _refused(mk(Pd), Bd, 2)                                      # nrow(P_0) != n(A)
    _refused(mk([Pd[0], Qd[1]]), Ad, 2)                          # nrow(P_1) != ncol(P_0)
    _refused(mk([]), Pd[0], 2)                                   # A is not square
    # SGM_ERR_UNSUPPORTED = 8, the message names the level
    n = A[0]
    ell = sg.ellpack_matrix(n, n, np.arange(1, n + 1, dtype=np.int32).reshape(n, 1), np.ones((n, 1)))
    _refused(mk(Pd), ell, 8, "level 0")
    part = sg.partitioned_csr_matrix(n, n, A[2], A[3], A[4], np.array([0, 512, n], np.int64))
    _refused(mk(Pd), part, 8, "level 0")
    comp = sg.sparse_matrix(np.array([1, n + 1], np.int32), np.array([1, n + 1], np.int32))
    comp.set_submatrix(1, 1, Ad)
    _refused(mk(Pd), comp, 8, "level 0")
    n1 = Ps[1][0]
    ell1 = sg.ellpack_matrix(n1, n1, np.arange(1, n1 + 1, dtype=np.int32).reshape(n1, 1), np.ones((n1, 1)))
    _refused(mk([Pd[0], ell1]), Ad, 8, "level 1")
    # SGM_ERR_BAD_ARG = 1: parameters outside their limits
    for kw in (dict(nu_pre=0), dict(nu_post=-1), dict(coarse_sweeps=0)):
        with pytest.raises(sg.SigmaError) as e:
            sg.multigrid(Pd, omega=OMEGA, **kw)
        assert e.value.code == 1
    with pytest.raises(sg.SigmaError) as e:                      # the factory has no P
        sg._ck(sg.lib().sgm_pc_create(sg.C.byref(sg.C.c_void_p()), sg.C.c_int32(3)))
    assert e.value.code == 1
    # a handle that was refused once can be set up again with a matrix that fits
    pc = mk(Pd)
    with pytest.raises(sg.SigmaError):
        pc.setup(Bd)
    pc.setup(Ad)
    z = np.zeros(n)
    pc.solve(Ad, z, PB.test_vector(n))
    assert np.isfinite(z).all()


# ------------------------------------------------------------------ 7. the Fortran host layer
def test_fortran_program_solves_with_the_same_iteration_count():
    exe = os.path.join(ROOT, "sigma_amd", "fortran", "mg_test_hip")
    if not os.path.exists(exe):
        pytest.skip("sigma_amd/fortran/mg_test_hip was not built (no amdflang at build time)")
    A, Ps, b, _ = _restated_pcg(63)
    _, it = _device_solve(sg.cg(1e-10), A, Ps, b)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout.replace("\n ", "")
    assert "mg_test_hip: ok" in out, r.stdout
    found = re.search(r"V\(1,1\)-PCG iterations\s+(\d+)", out)
    assert found and int(found.group(1)) == it, (r.stdout, it)
