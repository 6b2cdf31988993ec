"""Value edits on the device (sgm_mat_set_entries / add_entries / get_entries / zero / scalar_multiply / add_matrix and the
plans): bit for bit against the reference's results (tests/golden/edit) and the restated contract (tests/edit_restated.py)."""
import glob
import os
import re

import numpy as np
import pytest

import edit_restated as R
import sigma_amd as sg
from sigma_amd import problems as PB
from test_edit_cpu import ADD, ADD_MATRIX, ADD_MULT, GET, SCALE, SET, SET_MULT, ZERO, bits, same, structure

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "edit", "*.npz")))


@pytest.fixture(scope="module", autouse=True)
def _init():
    sg.init(0)


def dev(S, val):
    """a device handle of a restated structure"""
    if S["fmt"] == "csr":
        return sg.csr_matrix(S["nrow"], S["ncol"], S["ptr"], S["node"], np.ascontiguousarray(val, np.float64))
    return sg.ellpack_matrix(S["nrow"], S["ncol"], S["node"], np.ascontiguousarray(val, np.float64).reshape(S["node"].shape))


def read(A):
    return A.get("val", np.float64)


@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: os.path.basename(p)[:-4])
def test_every_fixture_is_reproduced_bit_for_bit(path):
    d = np.load(path)
    S = structure(d)
    A = dev(S, np.zeros(R.nslots(S)))
    if S["fmt"] == "ell":
        assert np.array_equal(A.get("degrees", np.int32), S["degrees"])
    for k in range(int(d["nops"])):
        t = f"op{k}_"
        code = int(d[t + "code"])
        if code == SET:
            A.set_value(d[t + "i"], d[t + "j"], d[t + "z"])
        elif code == ADD:
            A.add_value(d[t + "i"], d[t + "j"], d[t + "z"])
        elif code == ADD_MULT:
            A.add_multiple_values(d[t + "is"], d[t + "js"], d[t + "B"])
        elif code == SET_MULT:
            A.set_multiple_values(d[t + "is"], d[t + "js"], d[t + "B"])
        elif code == ADD_MATRIX:
            B = dev(structure(d, t + "b_"), d[t + "b_val"])
            A.add_sparse_matrix(B, float(d[t + "alpha"][0]) if len(d[t + "alpha"]) else None)
        elif code == SCALE:
            A.scalar_multiply(float(d[t + "alpha"][0]))
        elif code == ZERO:
            A.zero()
        if code == GET:
            got = A.get_value(d[t + "i"], d[t + "j"])
            print(path, k, "get", int((bits(got) != bits(d[t + "zout"])).sum()), "of", len(got), "differ")
            assert np.array_equal(bits(got), bits(d[t + "zout"])), k
        else:
            got = read(A)
            print(path, k, code, int((bits(got) != bits(d[t + "val"])).sum()), "of", len(got), "slots differ")
            assert np.array_equal(bits(got), bits(d[t + "val"])), (k, code)


def _long_row_csr(rs):
    """unsorted rows, stored duplicates, and a 3000-entry row"""
    S = R.random_csr(rs, 300, 4000, 5.0, dup_frac=0.25, empty_rows=(3, 100))
    ptr, node = S["ptr"].astype(np.int64), S["node"]
    long_cols = (rs.permutation(4000)[:3000] + 1).astype(np.int32)
    r = 41
    lo, hi = ptr[r] - 1, ptr[r + 1] - 1
    node = np.concatenate([node[:lo], long_cols, node[hi:]])
    ptr[r + 1:] += 3000 - (hi - lo)
    return R.csr(300, 4000, ptr, node)


@pytest.mark.parametrize("which", ["csr", "ell"])
def test_random_batches_one_shot_and_plan_against_the_restatement(which):
    rs = np.random.RandomState(11 if which == "csr" else 12)
    S = _long_row_csr(rs) if which == "csr" else R.random_ell(rs, 700, 500, 9)
    val = rs.standard_normal(R.nslots(S))
    if which == "ell":
        val = (val.reshape(S["node"].shape) * (np.arange(S["node"].shape[1])[None, :] < S["degrees"][:, None])).reshape(-1)
    A, Bp = dev(S, val), dev(S, val)
    want = val
    for step, mode in enumerate(("add", "set", "add")):
        i, j, z = R.random_batch(rs, S, 6000, nan=False)
        if which == "csr":                       # a long chain on one entry of the 3000-entry row, and hits all over that row
            c = S["node"][S["ptr"][41] - 1 + 1234]
            i[1000:1700], j[1000:1700] = 42, c
            i[3000:3400] = 42
            j[3000:3400] = S["node"][S["ptr"][41] - 1 + rs.randint(0, 3000, 400)]
        want = R.apply_vectorised(S, want, i, j, z, mode)
        (A.add_value if mode == "add" else A.set_value)(i, j, z)
        got = read(A)
        print(which, step, mode, int((bits(got) != bits(want)).sum()), "of", len(got), "slots differ from the restatement")
        assert np.array_equal(bits(got), bits(want))
        plan = sg.edit_plan(Bp, i, j)
        info = plan.info()
        assert info["m"] == 6000 and info["slots"] == R.chain_stats(S, i, j)[0] and info["longest_chain"] == R.chain_stats(S, i, j)[1]
        assert info["stored_sources"] >= np.diff(R.locate_vectorised(S, i, j)[0]).sum()
        (plan.add if mode == "add" else plan.set)(z)
        assert np.array_equal(bits(read(Bp)), bits(want))                  # one-shot and plan + apply: identical bits
        gi, gj = rs.randint(1, S["nrow"] + 1, 500).astype(np.int32), rs.randint(1, S["ncol"] + 1, 500).astype(np.int32)
        gi[:250], gj[:250] = i[:250], j[:250]
        assert np.array_equal(bits(A.get_value(gi, gj)), bits(R.get_vectorised(S, want, gi, gj)))
    # apply twice with zero_first: the same matrix twice; without: on top
    z2 = R.special_values(rs, 6000, nan=False)
    once = R.apply_vectorised(S, np.zeros(R.nslots(S)), i, j, z2, "add")
    plan.add(z2, zero_first=True)
    first = read(Bp)
    plan.add(z2, zero_first=True)
    assert np.array_equal(bits(first), bits(once)) and np.array_equal(bits(read(Bp)), bits(once))
    plan.add(z2)
    assert np.array_equal(bits(read(Bp)), bits(R.apply_vectorised(S, once, i, j, z2, "add")))
    # device tensors as arguments; m = 0
    import torch
    ti, tj = torch.from_numpy(i).cuda(), torch.from_numpy(j).cuda()
    tz = torch.from_numpy(z2).cuda()
    A.zero()
    A.add_value(ti, tj, tz)
    assert np.array_equal(bits(read(A)), bits(once))
    assert np.array_equal(bits(A.get_value(ti, tj).cpu().numpy()), bits(R.get_vectorised(S, once, i, j)))
    A.add_value(np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0))
    assert np.array_equal(bits(read(A)), bits(once))
    A.scalar_multiply(-0.3)
    assert same(read(A), np.float64(-0.3) * once)
    A.add_sparse_matrix(Bp, 1.0 / 3.0)
    bi, bj, bz = R.matrix_triples(S, read(Bp), 1.0 / 3.0)
    assert same(read(A), R.apply_vectorised(S, np.float64(-0.3) * once, bi, bj, bz, "add"))
    assert same([A.get_value(1, 1)], R.get_literal(S, read(A), [1], [1]))


def _families():
    rs = np.random.RandomState(5)
    n = 60 * 50
    ptr, node, _ = PB.poisson2d_csr(60, 50)
    grid = R.csr(n, n, ptr, node)
    rnd = R.random_csr(rs, 1500, 1500, 6.0, dup_frac=0.0)
    rows = [(rs.permutation(1200)[:rs.randint(50, 91)] + 1).astype(np.int32) for _ in range(1200)]      # long rows of uneven length
    uneven = R.csr(1200, 1200, np.concatenate([[1], 1 + np.cumsum([len(c) for c in rows])]), np.concatenate(rows))
    el = R.random_ell(rs, 2000, 2000, 12)
    return [("sliced stencil", grid, {}, "k_csr_sl<"), ("dictionary", grid, {"csr_sliced": 0}, "k_csr_do"),
            ("row-owner", rnd, {"csr_sliced": 0}, "CW=4"), ("SELL", uneven, {}, "k_csr_sell"),
            ("ELLPACK", el, {"ell_colblock": 0}, "k_ell"), ("column-blocked ELLPACK", el, {"ell_colblock": 2}, "k_ellcb")]


@pytest.mark.parametrize("lean", [1, 0])
def test_after_an_edit_the_handle_is_whole_for_every_kernel_family(lean):
    defaults = {"csr_sliced": 1, "csr_sell": 1, "ell_colblock": 1, "csr_lean": 1}
    seen = []
    for name, S, opts, expect in _families():
        rs = np.random.RandomState(len(name))
        val0 = rs.standard_normal(R.nslots(S))
        if S["fmt"] == "ell":
            val0 = (val0.reshape(S["node"].shape) * (np.arange(S["node"].shape[1])[None, :] < S["degrees"][:, None])).reshape(-1)
        i, j, _ = R.random_batch(rs, S, 5000)
        z = rs.standard_normal(5000)
        want = R.apply_vectorised(S, R.apply_vectorised(S, val0, i, j, z, "add"), i[:900], j[:900], z[:900], "set")
        try:
            for k, v in dict(opts, csr_lean=lean).items():
                sg.set_option(k, v)
            H, F = dev(S, val0), dev(S, want)
        finally:
            for k, v in defaults.items():
                sg.set_option(k, v)
        seen.append((name, H.kernel))
        assert expect in H.kernel and H.kernel == F.kernel, (name, H.kernel, F.kernel)
        x = rs.standard_normal(S["ncol"])
        xt = rs.standard_normal(S["nrow"])
        y0, t0 = np.zeros(S["nrow"]), np.zeros(S["ncol"])
        H.matvec(x, y0)
        H.matvec_t(xt, t0)                           # the transpose exists before the edit: it must be refreshed
        H.add_value(i, j, z)
        H.set_value(i[:900], j[:900], z[:900])
        assert np.array_equal(bits(read(H)), bits(want)), name
        for _ in range(2):
            y, yf, t, tf = np.zeros(S["nrow"]), np.zeros(S["nrow"]), np.zeros(S["ncol"]), np.zeros(S["ncol"])
            H.matvec(x, y); F.matvec(x, yf)
            H.matvec_t(xt, t); F.matvec_t(xt, tf)
            assert np.array_equal(bits(y), bits(yf)) and not np.array_equal(y, y0), name
            assert np.array_equal(bits(t), bits(tf)), name
            plan = sg.edit_plan(H, i, j)             # second round: through a plan, zero_first
            plan.add(z, zero_first=True)
            F.set_values(R.apply_vectorised(S, np.zeros(R.nslots(S)), i, j, z, "add").reshape(-1))
    print(seen)


def test_a_jacobi_preconditioner_set_up_again_sees_the_new_diagonal():
    n = 40 * 30
    ptr, node, val = PB.poisson2d_csr(40, 30)
    S = R.csr(n, n, ptr, node)
    A = sg.csr_matrix(n, n, ptr, node, val)
    pc = sg.jacobi()
    pc.setup(A)
    d0 = pc.idiag.copy()
    rows = np.arange(1, n + 1, dtype=np.int32)
    z = np.random.RandomState(2).uniform(0.5, 1.5, n)
    A.add_value(rows, rows, z)
    pc.setup(A)
    want = R.apply_vectorised(S, val, rows, rows, z, "add")
    diag = R.get_vectorised(S, want, rows, rows)
    assert np.array_equal(bits(pc.idiag), bits(1.0 / diag)) and not np.array_equal(pc.idiag, d0)


def test_an_algebra_result_refilled_after_its_operand_was_edited():
    rs = np.random.RandomState(9)
    S = R.random_csr(rs, 80, 80, 4.0, dup_frac=0.0)
    v = rs.standard_normal(R.nslots(S))
    X, Y = dev(S, v), dev(S, v)
    M = sg.sparse_matrix_product(X, Y)
    i, j, z = R.random_batch(rs, S, 400, nan=False)
    X.add_value(i, j, z)
    M.refill(X, Y)
    fresh = sg.sparse_matrix_product(dev(S, R.apply_vectorised(S, v, i, j, z, "add")), Y)
    assert np.array_equal(M.get("node", np.int32), fresh.get("node", np.int32))
    assert same(read(M), read(fresh))


def test_refusals_leave_the_matrix_unchanged():
    rs = np.random.RandomState(21)
    for S in (R.random_csr(rs, 50, 60, 4.0, empty_rows=(7,)), R.random_ell(rs, 50, 60, 5)):
        val = rs.standard_normal(R.nslots(S))
        if S["fmt"] == "ell":
            val = (val.reshape(S["node"].shape) * (np.arange(S["node"].shape[1])[None, :] < S["degrees"][:, None])).reshape(-1)
        A = dev(S, val)
        before = read(A)
        i, j, z = R.random_batch(rs, S, 200, nan=False)
        # a missing entry at t = 150 and another, later one: the smaller t is named
        for t in (149, 180):
            free = sorted(set(range(1, 61)) - set(R.row_slots(S, int(i[t]))[1].tolist()))
            j[t] = free[0]
        for call in (A.add_value, A.set_value, lambda a, b, c: sg.edit_plan(A, a, b)):
            with pytest.raises(sg.SigmaError) as e:
                call(i, j, z)
            assert e.value.code == 8 and "t = 150 " in str(e.value) and f"({i[149]}, {j[149]})" in str(e.value), str(e.value)
            assert np.array_equal(bits(read(A)), bits(before))
        assert A.get_value(int(i[149]), int(j[149])) == 0.0          # never an error for an absent entry
        i2 = i.copy()
        i2[30] = 51
        with pytest.raises(sg.SigmaError) as e:
            A.add_value(i2, j, z)
        assert e.value.code == 2 and "t = 31 " in str(e.value), str(e.value)
        j2 = j.copy()
        j2[12] = 0
        with pytest.raises(sg.SigmaError) as e:
            A.set_value(i, j2, z)
        assert e.value.code == 2 and "t = 13 " in str(e.value)
        assert np.array_equal(bits(read(A)), bits(before))
        # a plan belongs to its matrix
        i, j, z = R.random_batch(rs, S, 100, nan=False)
        plan = sg.edit_plan(A, i, j)
        other = dev(S, val)
        with pytest.raises(sg.SigmaError) as e:
            plan.add(z, A=other)
        assert e.value.code == 1
        assert np.array_equal(bits(read(other)), bits(before))
        if S["fmt"] == "csr":
            A.left_permute(np.arange(50, 0, -1, dtype=np.int32))
            moved = read(A)
            with pytest.raises(sg.SigmaError) as e:
                plan.add(z)
            assert e.value.code == 1 and "pattern" in str(e.value)
            assert np.array_equal(bits(read(A)), bits(moved))
    n = 16
    ptr, node, val = PB.poisson2d_csr(4, 4)
    part = sg.partitioned_csr_matrix(n, n, ptr, node, val, np.array([0, 8, 16], np.int64))
    one = np.ones(1, np.int32)
    L = sg.lib()
    import ctypes as C
    for rc in (L.sgm_mat_add_entries(part._h, C.c_int64(1), C.c_void_p(one.ctypes.data), C.c_void_p(one.ctypes.data),
                                     C.c_void_p(np.ones(1).ctypes.data), C.c_int(0)),
               L.sgm_mat_zero(part._h), L.sgm_mat_scalar_multiply(part._h, C.c_double(2.0))):
        assert rc == 8
    x, y = np.ones(n), np.zeros(n)
    part.matvec(x, y)
    ref = sg.csr_matrix(n, n, ptr, node, val)
    yr = np.zeros(n)
    ref.matvec(x, yr)
    assert np.array_equal(y, yr)


def test_the_fem_flow_end_to_end_on_a_512_grid():
    """pattern by from_edges, a plan, apply(zero_first) with the element matrices in a device tensor, CG to a fixed count"""
    import torch
    nx = 512
    nn = nx * nx
    x, ele = R.fem_grid(nx, nx, seed=4)
    ti, tj, zk = R.fem_triples(x, ele, "stiffness")
    _, _, zm = R.fem_triples(x, ele, "mass")
    z = zk + zm                                           # K + M: positive definite
    di, dj = torch.from_numpy(ti).cuda(), torch.from_numpy(tj).cuda()
    dz = torch.from_numpy(z).cuda()
    A = sg.csr_matrix.from_edges(nn, nn, di, dj, torch.zeros_like(dz))
    S = R.csr(nn, nn, A.get("ptr", np.int32), A.get("node", np.int32))
    plan = sg.edit_plan(A, di, dj)
    info = plan.info()
    assert info["m"] == 18 * (nx - 1) ** 2 and info["slots"] == R.nslots(S) and info["longest_chain"] == 6
    print("plan info", info, "padding", info["stored_sources"] / info["m"])
    plan.add(dz, zero_first=True)
    want = R.apply_vectorised(S, np.zeros(R.nslots(S)), ti, tj, z, "add")
    got = read(A)
    print("fem 512:", int((bits(got) != bits(want)).sum()), "of", len(got), "entries differ from the restatement")
    assert np.array_equal(bits(got), bits(want))
    plan.add(2.0 * dz, zero_first=True)                   # the next time step's matrices ...
    plan.add(dz, zero_first=True)                         # ... and back
    assert np.array_equal(bits(read(A)), bits(want))
    F = sg.csr_matrix(nn, nn, S["ptr"], S["node"], want)
    b = np.full(nn, 1.0 / nn)
    us = []
    for M in (A, F):
        s = sg.cg(1e-30)
        s.set_max_iter(60)
        s.setup(M)
        u = np.zeros(nn)
        s.solve(M, u, b, check=False)
        assert s.iterations == 60
        us.append(u)
    assert np.array_equal(bits(us[0]), bits(us[1])) and np.isfinite(us[0]).all() and us[0].max() > 0
