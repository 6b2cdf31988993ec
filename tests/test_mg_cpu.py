"""CPU-side checks of the multigrid preconditioner's contract (tests/mg_restated.py): the two restatements agree bit for
bit, the restated V(1,1)-PCG needs a grid-independent handful of iterations where plain CG needs hundreds, and without a GPU
sgm_mg_create fails loudly like every other create."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import algebra_restated as R      # noqa: E402
import mg_restated as MG          # noqa: E402
import sigma_amd as sg            # noqa: E402
from sigma_amd import problems as P   # noqa: E402


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


PARAMS = [(1, 1, 8), (2, 2, 1), (3, 0, 2)]


@pytest.mark.parametrize("case", ["poisson31", "random_spd"])
def test_literal_and_vectorised_restatements_agree_bit_for_bit(case):
    A, Ps = MG.poisson_case(31, 31) if case == "poisson31" else MG.random_spd_case(300)
    lev = MG.levels(A, Ps)
    assert [m[0] for m in lev] == ([961, 256, 64, 16] if case == "poisson31" else [300, 75, 19])
    n = A[0]
    rs = np.random.RandomState(7)
    for nu_pre, nu_post, coarse in PARAMS:
        lit = MG.Literal(A, Ps, 0.8, nu_pre, nu_post, coarse, lev=lev)
        vec = MG.Vectorised(A, Ps, 0.8, nu_pre, nu_post, coarse, lev=lev)
        for l in range(len(lev)):
            assert np.array_equal(R.bits(lit.idiag[l]), R.bits(vec.idiag[l]))
        for r in (P.test_vector(n), rs.standard_normal(n)):
            assert np.array_equal(R.bits(lit.apply(r)), R.bits(vec.apply(r))), (case, nu_pre, nu_post, coarse)


def test_galerkin_levels_of_the_poisson_hierarchy_are_nine_point():
    A, Ps = MG.poisson_case(100, 70)
    lev = MG.levels(A, Ps)
    assert [m[0] for m in lev] == [7000, 1750, 450, 117, 35, 12]
    for m in lev:
        assert np.diff(m[2]).max() <= 9


def test_interp2d_hierarchy_level_counts():
    for (nx, ny), nlev in (((31, 31), 4), ((63, 63), 5), ((127, 127), 6), ((255, 255), 7), ((100, 70), 6)):
        h = P.interp2d_hierarchy(nx, ny)
        assert len(h) + 1 == nlev
        assert h[0][3] == nx * ny
        for a, b in zip(h, h[1:]):
            assert a[4] == b[3]                      # the column count of one level is the row count of the next


@pytest.mark.parametrize("nx,ny", [(63, 63), (127, 127), (100, 70)])
def test_restated_vcycle_pcg_needs_ten_times_fewer_iterations_than_plain_cg(nx, ny):
    A, Ps = MG.poisson_case(nx, ny)
    n = A[0]
    rows = MG._Rows(A)
    xs = P.test_vector(n)
    b = rows.matvec(xs)
    vc = MG.Vectorised(A, Ps, 0.8, 1, 1, 8)
    x, it, res2 = MG.pcg(rows, b, vc.apply, tol=1e-10)
    _, it_plain, _ = MG.pcg(rows, b, None, tol=1e-10)
    print(f"{nx}x{ny}: V(1,1)-PCG {it} iterations, plain CG {it_plain}, max error {np.abs(x - xs).max():.3e}")
    assert np.sqrt(res2) <= 1e-10
    assert it <= 14
    assert it_plain >= 10 * it
    assert np.abs(x - xs).max() <= 1e-9


@pytest.mark.skipif(_has_gpu(), reason="GPU present: the loud-failure path cannot be seen")
def test_mg_create_fails_loudly_without_gpu():
    L = sg.lib()
    h = C.c_void_p()
    rc = L.sgm_mg_create(C.byref(h), C.c_int32(0), None, C.c_double(0.8), C.c_int32(1), C.c_int32(1), C.c_int32(8))
    assert rc == 6 and not h.value
    assert "no CPU path" in L.sgm_last_error().decode()
    with pytest.raises(sg.SigmaError) as e:
        sg.multigrid([], omega=0.8)
    assert e.value.code == 6


def test_sgm_pc_create_keeps_refusing_the_multigrid_kind():
    h = C.c_void_p()
    assert sg.lib().sgm_pc_create(C.byref(h), C.c_int32(3)) == 1 and not h.value
