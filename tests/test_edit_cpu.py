"""Value edits (sgm_mat_set_entries / add_entries / get_entries / zero / scalar_multiply / add_matrix, sgm_edit_plan_*): the
two numpy restatements of the contract (tests/edit_restated.py) against the reference's own results (tests/golden/edit, made
by tools/edit_golden), the host locate step through the C ABI, and the loud failures without a GPU."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import edit_restated as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "edit", "*.npz")))
SET, ADD, ADD_MULT, SET_MULT, ADD_MATRIX, SCALE, ZERO, GET = 1, 2, 3, 4, 5, 6, 7, 8


def bits(a):
    return np.ascontiguousarray(a, np.float64).reshape(-1).view(np.int64)


def same(a, b):
    """the same bits, NaNs in the same positions (which operand's payload a NaN + NaN keeps is the adder's choice, scalar and
    SIMD additions of one CPU already differ in it; the fixtures hold no NaN and are compared bit for bit)"""
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb])


def structure(d, tag=""):
    nrow, ncol = (int(v) for v in d["shape"])
    if int(d["fmt"]) == 0:
        return R.csr(nrow, ncol, d[tag + "ptr"], d[tag + "node"])
    return R.ell(nrow, ncol, d[tag + "node"], d[tag + "degrees"])


def replay(d, apply, get):
    """every operation of a fixture through one restatement; yields (k, got, want)"""
    S = structure(d)
    val = np.zeros(R.nslots(S))
    for k in range(int(d["nops"])):
        t = f"op{k}_"
        code = int(d[t + "code"])
        if code in (SET, ADD):
            val = apply(S, val, d[t + "i"], d[t + "j"], d[t + "z"], "set" if code == SET else "add")
        elif code in (ADD_MULT, SET_MULT):
            i, j, z = R.expand_multiple(d[t + "is"], d[t + "js"], d[t + "B"])
            val = apply(S, val, i, j, z, "add" if code == ADD_MULT else "set")
        elif code == ADD_MATRIX:
            alpha = float(d[t + "alpha"][0]) if len(d[t + "alpha"]) else None
            i, j, z = R.matrix_triples(structure(d, t + "b_"), d[t + "b_val"], alpha)
            val = apply(S, val, i, j, z, "add")
        elif code == SCALE:
            val = np.float64(d[t + "alpha"][0]) * val
        elif code == ZERO:
            val = np.zeros_like(val)
        if code == GET:
            yield k, get(S, val, d[t + "i"], d[t + "j"]), d[t + "zout"]
        else:
            yield k, val, d[t + "val"]


def test_the_fixtures_are_there():
    names = {os.path.basename(f)[:-4] for f in FIXTURES}
    for case in ("fem_stiffness", "fem_mass", "set_then_add", "add_multiple", "add_matrix", "scale_zero_get", "padding_column"):
        assert case + "_csr" in names and case + "_ell" in names, case
    biggest = max(os.path.getsize(f) for f in glob.glob(os.path.join(ROOT, "tests", "golden", "*.npz")))
    assert all(os.path.getsize(f) <= biggest for f in FIXTURES)


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(f)[:-4] for f in FIXTURES])
def test_both_restatements_reproduce_the_reference_bit_for_bit(path):
    d = np.load(path)
    for apply, get in ((R.apply_literal, R.get_literal), (R.apply_vectorised, R.get_vectorised)):
        n = 0
        for k, got, want in replay(d, apply, get):
            assert np.array_equal(bits(got), bits(want)), (apply.__name__, k)
            n += 1
        assert n == int(d["nops"])


@pytest.mark.parametrize("seed", range(6))
def test_the_restatements_agree_on_random_batches_with_stored_duplicates(seed):
    rs = np.random.RandomState(100 + seed)
    S = R.random_csr(rs, 60, 50, 4.0, dup_frac=0.3, empty_rows=(5, 17)) if seed % 2 == 0 else R.random_ell(rs, 50, 40, 6)
    val = rs.standard_normal(R.nslots(S))
    if S["fmt"] == "ell":                      # padding holds 0.0
        val = val.reshape(S["node"].shape) * (np.arange(S["node"].shape[1])[None, :] < S["degrees"][:, None])
        val = val.reshape(-1)
    for mode in ("set", "add", "add"):
        i, j, z = R.random_batch(rs, S, 500)
        a, b = R.apply_literal(S, val, i, j, z, mode), R.apply_vectorised(S, val, i, j, z, mode)
        assert same(a, b)
        assert np.array_equal(R.locate_literal(S, i, j)[0], R.locate_vectorised(S, i, j)[0])
        assert np.array_equal(R.locate_literal(S, i, j)[1], R.locate_vectorised(S, i, j)[1])
        val = a
    gi, gj = rs.randint(1, S["nrow"] + 1, 300), rs.randint(1, S["ncol"] + 1, 300)
    assert same(R.get_literal(S, val, gi, gj), R.get_vectorised(S, val, gi, gj))
    if S["fmt"] == "csr":                      # a stored duplicate is edited in both copies
        slots, rows, cols = R._stored(S)
        key = rows * 1000 + cols
        u, c = np.unique(key, return_counts=True)
        assert (c > 1).any()
        r, cc = divmod(int(u[c > 1][0]), 1000)
        out = R.apply_literal(S, np.zeros(R.nslots(S)), [r], [cc], [2.5], "add")
        assert (out == 2.5).sum() == int(c[c > 1][0])


@pytest.mark.parametrize("kind", ["stiffness", "mass"])
@pytest.mark.parametrize("fmt", ["csr", "ell"])
def test_the_fem_fixtures_see_the_order_of_the_additions(kind, fmt):
    """accumulating the same triples in REVERSED order changes the bits of at least one entry: a restatement (or a kernel)
    that re-associated the sums would not reproduce these fixtures"""
    d = np.load(os.path.join(ROOT, "tests", "golden", "edit", f"fem_{kind}_{fmt}.npz"))
    S = structure(d)
    i, j, z = d["op0_i"], d["op0_j"], d["op0_z"]
    assert len(i) == 864 and R.chain_stats(S, i, j) == (379, 6)
    rev = R.apply_vectorised(S, np.zeros(R.nslots(S)), i[::-1], j[::-1], z[::-1], "add")
    changed = int((bits(rev) != bits(d["op0_val"])).sum())
    assert np.allclose(rev, d["op0_val"], rtol=1e-12, atol=1e-15)
    assert changed >= 1, changed
    # the generator is the one the fixtures were made with
    x, ele = R.fem_grid(9, 7, seed=1, jitter=0.1)
    ti, tj, tz = R.fem_triples(x, ele, kind)
    assert np.array_equal(ti, i) and np.array_equal(tj, j) and np.array_equal(bits(tz), bits(z))
    if fmt == "csr":
        P = R.pattern_csr(63, 63, ti, tj)
        assert np.array_equal(P["ptr"], S["ptr"]) and np.array_equal(P["node"], S["node"])


def test_the_fem_stream_is_a_stiffness_matrix():
    x, ele = R.fem_grid(12, 10, seed=3)
    i, j, z = R.fem_triples(x, ele, "stiffness")
    S = R.pattern_csr(120, 120, i, j)
    val = R.apply_vectorised(S, np.zeros(R.nslots(S)), i, j, z, "add")
    rows = np.repeat(np.arange(120), np.diff(S["ptr"]))
    dense = np.zeros((120, 120))
    dense[rows, S["node"] - 1] = val
    assert np.allclose(dense, dense.T, atol=1e-12) and np.allclose(dense.sum(1), 0.0, atol=1e-12)
    mi, mj, mz = R.fem_triples(x, ele, "mass")
    assert np.isclose(mz.sum(), 11 * 9, rtol=0.05)                 # the area of the (jittered) domain


def test_host_locate_returns_the_restatements_hits():
    import sigma_amd as sg
    rs = np.random.RandomState(7)
    S = R.random_csr(rs, 80, 70, 5.0, dup_frac=0.3, empty_rows=(0, 33, 79))
    i, j, _ = R.random_batch(rs, S, 700)
    off, slot, miss = sg.edit_locate_host(80, 70, S["ptr"], S["node"], i, j)
    roff, rslot, rmiss = R.locate_literal(S, i, j)
    assert np.array_equal(off, roff) and np.array_equal(slot, rslot + 1) and miss == rmiss == 0
    assert off[-1] > 700                                            # stored duplicates were hit
    # absent entries: the smallest t, hits of the others unchanged
    i2, j2 = i.copy(), j.copy()
    absent = []
    for t in (500, 123, 640):
        r = int(i2[t])
        free = sorted(set(range(1, 71)) - set(R.row_slots(S, r)[1].tolist()))
        j2[t] = free[0]
        absent.append(t + 1)
    i2[300] = 34                                                    # an empty row
    off2, slot2, miss2 = sg.edit_locate_host(80, 70, S["ptr"], S["node"], i2, j2)
    roff2, rslot2, rmiss2 = R.locate_vectorised(S, i2, j2)
    assert miss2 == rmiss2 == min(absent) == 124
    assert np.array_equal(off2, roff2) and np.array_equal(slot2, rslot2 + 1)
    # sizing call, m = 0, capacity too small, indices out of range
    L = sg.lib()
    needed, fm = C.c_int64(-1), C.c_int64(-1)
    o = np.zeros(len(i) + 1, np.int64)
    args = (C.c_int32(80), C.c_int32(70), C.c_void_p(S["ptr"].ctypes.data), C.c_void_p(S["node"].ctypes.data))
    assert L.sgm_edit_locate_host(*args, C.c_int64(len(i)), C.c_void_p(i.ctypes.data), C.c_void_p(j.ctypes.data),
                                  C.c_void_p(o.ctypes.data), None, C.c_int64(0), C.byref(needed), C.byref(fm)) == 0
    assert needed.value == off[-1] and fm.value == 0 and np.array_equal(o, off)
    small = np.zeros(4, np.int32)
    assert L.sgm_edit_locate_host(*args, C.c_int64(len(i)), C.c_void_p(i.ctypes.data), C.c_void_p(j.ctypes.data),
                                  C.c_void_p(o.ctypes.data), C.c_void_p(small.ctypes.data), C.c_int64(4), C.byref(needed), C.byref(fm)) == 1
    assert L.sgm_edit_locate_host(*args, C.c_int64(0), None, None, C.c_void_p(o.ctypes.data), None, C.c_int64(0),
                                  C.byref(needed), C.byref(fm)) == 0
    assert needed.value == 0 and fm.value == 0 and o[0] == 0
    off0, slot0, miss0 = sg.edit_locate_host(80, 70, S["ptr"], S["node"], [], [])
    assert len(off0) == 1 and len(slot0) == 0 and miss0 == 0
    i3 = i.copy()
    i3[41] = 81
    with pytest.raises(sg.SigmaError) as e:
        sg.edit_locate_host(80, 70, S["ptr"], S["node"], i3, j)
    assert e.value.code == 2 and "triple 42" in str(e.value)


def test_every_edit_entry_point_refuses_null_handles_without_crashing():
    import sigma_amd as sg
    L = sg.lib()
    one_i, one_z = np.ones(1, np.int32), np.ones(1)
    pi, pz = C.c_void_p(one_i.ctypes.data), C.c_void_p(one_z.ctypes.data)
    h = C.c_void_p()
    out4 = (C.c_int64 * 4)()
    calls = {
        "sgm_mat_set_entries": lambda: L.sgm_mat_set_entries(None, C.c_int64(1), pi, pi, pz, C.c_int(0)),
        "sgm_mat_add_entries": lambda: L.sgm_mat_add_entries(None, C.c_int64(1), pi, pi, pz, C.c_int(0)),
        "sgm_mat_get_entries": lambda: L.sgm_mat_get_entries(None, C.c_int64(1), pi, pi, pz, C.c_int(0)),
        "sgm_mat_zero": lambda: L.sgm_mat_zero(None),
        "sgm_mat_scalar_multiply": lambda: L.sgm_mat_scalar_multiply(None, C.c_double(2.0)),
        "sgm_mat_add_matrix": lambda: L.sgm_mat_add_matrix(None, None, None),
        "sgm_edit_plan_create": lambda: L.sgm_edit_plan_create(C.byref(h), None, C.c_int64(1), pi, pi, C.c_int(0)),
        "sgm_edit_plan_apply": lambda: L.sgm_edit_plan_apply(None, None, pz, C.c_int(1), C.c_int(0), C.c_int(0)),
        "sgm_edit_plan_info": lambda: L.sgm_edit_plan_info(None, out4),
        "sgm_edit_plan_destroy": lambda: L.sgm_edit_plan_destroy(None),
    }
    for name, call in calls.items():
        rc = call()
        assert rc in (6, 1), (name, rc)            # SGM_ERR_NO_DEVICE without a GPU, SGM_ERR_BAD_ARG with one
        assert L.sgm_last_error(), name
        assert not h.value


def test_the_python_names_are_the_references():
    import sigma_amd as sg
    for cls in (sg.csr_matrix, sg.ellpack_matrix):
        for name in ("set_value", "add_value", "get_value", "set_multiple_values", "add_multiple_values", "add_sparse_matrix", "zero",
                     "scalar_multiply"):
            assert callable(getattr(cls, name)), (cls, name)
    for name in ("add", "set", "info", "destroy"):
        assert callable(getattr(sg.edit_plan, name))
    assert callable(sg.edit_locate_host)
