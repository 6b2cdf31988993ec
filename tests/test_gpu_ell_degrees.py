"""ELLPACK rows the padding cannot describe, on the device: every reader of degrees(i) -- read-back, Jacobi, ILDU(0), PCG,
get / set / add_value, plans, add_sparse_matrix, the permutations, the text dump, a composite -- on every row shape of
tests/ell_degree_cases.py, against the oracle (oracle.EllMatrix takes degrees explicitly) or tests/edit_restated.py.  Every
comparison is np.array_equal, values by their bits: there is no tolerance in this file.

Handles are built WITH degrees (sg.ellpack_matrix(..., degrees=)) for every shape, and WITHOUT for the shapes whose degrees the
padding tells (1, 2, 3, 7, 8, 10); shape 9 without degrees must refuse every reader and still multiply; shapes 4 to 6 without
degrees are only characterised (the documented limit of the recovery).

The products of a row with node = 0 slots: the reference reads x(0) there (README: an empty row); the library multiplies the
slot's value by x(1).  The oracle is handed node = 1 in those slots, which is the same arithmetic without the read out of
bounds; the value in such a slot is +0.0 in every case here."""
import functools
import os
import sys

import numpy as np
import pytest

import sigma_amd as sg
from sigma_amd import problems as P

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edit_restated as R  # noqa: E402
import ell_degree_cases as K  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = K.cases()
GRID = [("given", n) for n in K.NAMES] + [("recovered", n) for n in K.RECOVERABLE]
IDS = [f"{how}-{n}" for how, n in GRID]
SPD = [(how, n) for how, n in GRID if CASES[n].spd]


@pytest.fixture(scope="module", autouse=True)
def _init():
    sg.init(0)


@pytest.fixture
def dot_order_1():
    sg.set_option("dot_order", 1)
    yield
    sg.set_option("dot_order", 0)


def bits(a):
    return np.ascontiguousarray(a, np.float64).reshape(-1).view(np.int64)


def handle(name, how="given", val=None):
    c = CASES[name]
    return sg.ellpack_matrix(c.n, c.m, c.node, c.val if val is None else val, degrees=c.degrees if how == "given" else None)


@functools.lru_cache(maxsize=None)
def oracle(name):
    """(orc, E as the reference holds it, E with node 0 -> 1 for the products): built once per case, never changed"""
    import oracle as orc
    c = CASES[name]
    return orc, orc.EllMatrix(*c[:6]), orc.EllMatrix(c.n, c.m, c.max_d, np.where(c.node == 0, 1, c.node), c.val, c.degrees)


@functools.lru_cache(maxsize=None)
def product_refs(name):
    orc, _, Es = oracle(name)
    c = CASES[name]
    x, w = P.test_vector(c.m), np.cos(0.37 * np.arange(c.n))
    y0, t0 = np.sin(0.11 * np.arange(c.n)), np.sin(0.23 * np.arange(c.m))
    return x, w, y0, t0, {"matvec": Es.matvec(x), "matvec_add": Es.matvec_add(x, y0.copy()), "matvec_t": Es.matvec_t(w),
                          "matvec_t_add": Es.matvec_t_add(w, t0.copy())}


def products(H, name):
    c = CASES[name]
    x, w, y0, t0, _ = product_refs(name)
    return {"matvec": H.matvec(x, np.full(c.n, -7.0)), "matvec_add": H.matvec_add(x, y0.copy()),
            "matvec_t": H.matvec_t(w, np.full(c.m, -7.0)), "matvec_t_add": H.matvec_t_add(w, t0.copy())}


def versions(H):
    return tuple(int(v) for v in H.get("versions", np.int64))


# ------------------------------------------------------------------------------------------------ shape x reader
@pytest.mark.parametrize("how,name", GRID, ids=IDS)
def test_read_back(how, name):
    c = CASES[name]
    H = handle(name, how)
    assert np.array_equal(H.get("degrees", np.int32), c.degrees)
    assert np.array_equal(H.get("node", np.int32).reshape(c.n, c.max_d), c.node)          # the 0 slots read back as 0
    assert np.array_equal(bits(H.get("val", np.float64)), bits(c.val))


@pytest.mark.parametrize("colblock", [0, 1])
@pytest.mark.parametrize("offset_dict", [0, 1])
@pytest.mark.parametrize("how,name", GRID, ids=IDS)
def test_products_under_every_ellpack_kernel_option(how, name, offset_dict, colblock):
    """matvec, matvec_add, matvec_t, matvec_t_add = the oracle's, whichever ELLPACK kernel the options select; and the same bits
    from a handle that was given no degrees (the products never read them)."""
    want = product_refs(name)[4]
    H = handle(name, how)
    H0 = handle(name, "recovered")
    for A in (H, H0):
        A.set_option("ell_offset_dict", offset_dict)
        A.set_option("ell_colblock", colblock)
    got, got0 = products(H, name), products(H0, name)
    for k in want:
        assert np.array_equal(bits(got[k]), bits(want[k])), (k, H.kernel)
        assert np.array_equal(bits(got0[k]), bits(got[k])), (k, H0.kernel)


@pytest.mark.parametrize("how,name", GRID, ids=IDS)
def test_jacobi_idiag(how, name):
    """1 / get_value(i, i): the first degrees(i) slots, the last hit -- Inf where the diagonal is no real entry, whatever the
    padding holds (shape 6 keeps the deleted diagonal's column in its padding)"""
    orc, E, _ = oracle(name)
    c = CASES[name]
    pc = sg.jacobi()
    pc.setup(handle(name, how))
    want = orc.Jacobi(E).idiag
    assert np.array_equal(bits(pc.idiag), bits(want))
    D, present = K.dense_real(c)
    assert np.array_equal(np.isinf(pc.idiag), ~np.diag(present) | (np.diag(D) == 0.0))


@pytest.mark.parametrize("how,name", GRID, ids=IDS)
def test_ildu_factors_and_apply(how, name):
    orc, E, _ = oracle(name)
    c = CASES[name]
    ref = orc.Ildu(E)
    H = handle(name, how)
    pc = sg.ldu()
    pc.setup(H)
    for nm, want in (("Lptr", ref.Lptr), ("Uptr", ref.Uptr), ("Lnode", ref.Lnode[:ref.Lptr[-1] - 1]), ("Unode", ref.Unode[:ref.Uptr[-1] - 1])):
        assert np.array_equal(pc.get(nm, np.int32)[:len(want)], want), nm
    for nm, want in (("Lval", ref.Lval[:ref.Lptr[-1] - 1]), ("Uval", ref.Uval[:ref.Uptr[-1] - 1]), ("D", ref.D)):
        got = pc.get(nm, np.float64)[:len(want)]
        nan = np.isnan(want)                                  # (0 / 0 in a row without a pivot: NaN by position)
        assert np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got[~nan]), bits(want[~nan])), nm
    b = P.test_vector(c.n)
    z, zr = pc.solve(H, np.zeros(c.n), b), ref.solve(b)
    nan = np.isnan(zr)
    assert np.array_equal(np.isnan(z), nan) and np.array_equal(bits(z[~nan]), bits(zr[~nan]))


@pytest.mark.parametrize("how,name", SPD, ids=[f"{h}-{n}" for h, n in SPD])
def test_pcg_in_the_reference_dot_order(how, name, dot_order_1):
    """CG preconditioned by ILDU(0) of the matrix, dot_order = 1: the oracle's iteration count and every bit of x"""
    orc, E, Es = oracle(name)
    c = CASES[name]
    b = P.test_vector(c.n)
    xr, itr = orc.cg(Es, b, tol=1e-12, pc=orc.Ildu(E))[:2]
    H = handle(name, how)
    pc = sg.ldu()
    pc.setup(H)
    s = sg.cg(1e-12)
    s.setup(H)
    x = np.zeros(c.n)
    s.solve(H, x, b, pc)
    assert s.iterations == itr and itr > 1
    assert np.array_equal(bits(x), bits(xr))


@pytest.mark.parametrize("how,name", GRID, ids=IDS)
def test_get_value_real_padding_absent(how, name):
    c = CASES[name]
    real, pad, absent = K.probes(c)
    ij = np.array(real + pad + absent, np.int32)
    S = R.ell(c.n, c.m, c.node, c.degrees)
    want = R.get_literal(S, c.val, ij[:, 0], ij[:, 1])
    assert np.all(want[len(real):] == 0.0)
    got = handle(name, how).get_value(ij[:, 0], ij[:, 1])
    assert np.array_equal(bits(got), bits(want))


@pytest.mark.parametrize("how,name", GRID, ids=IDS)
def test_set_and_add_batches(how, name):
    c = CASES[name]
    S = R.ell(c.n, c.m, c.node, c.degrees)
    rs = np.random.RandomState(11)
    H = handle(name, how)
    val = c.val
    for mode in ("set", "add", "add"):
        i, j, z = R.random_batch(rs, S, 700, nan=False)
        (H.set_value if mode == "set" else H.add_value)(i, j, z)
        val = R.apply_vectorised(S, val, i, j, z, mode)
        assert np.array_equal(bits(H.get("val", np.float64)), bits(val)), mode


@pytest.mark.parametrize("how,name", GRID, ids=IDS)
def test_edit_of_a_column_that_is_no_entry_is_refused(how, name):
    """a column that stands only in a row's padding (what delete_edge leaves behind), or nowhere in the row: set_value and
    add_value refuse the whole batch, the values and the versions stay"""
    c = CASES[name]
    real, pad, absent = K.probes(c)
    H = handle(name, how)
    before = versions(H)
    for i, j in pad[:2] + absent[:2]:
        for edit in (H.set_value, H.add_value):
            with pytest.raises(sg.SigmaError) as e:
                edit(np.array([real[0][0], i, real[-1][0]], np.int32), np.array([real[0][1], j, real[-1][1]], np.int32), np.ones(3))
            assert e.value.code == 8
    assert np.array_equal(bits(H.get("val", np.float64)), bits(c.val)) and versions(H) == before


@pytest.mark.parametrize("how,name", GRID, ids=IDS)
def test_plan_made_before_set_degrees_is_refused_afterwards(how, name):
    c = CASES[name]
    real = K.probes(c)[0]
    i, j = np.array([r[0] for r in real], np.int32), np.array([r[1] for r in real], np.int32)
    H = handle(name, how)
    plan = sg.edit_plan(H, i, j)
    z = np.arange(len(i), dtype=np.float64)
    plan.add(z)
    v0 = versions(H)
    H.set_degrees(c.degrees)
    v1 = versions(H)
    assert v1[0] == v0[0] and v1[1] > v0[1] and v1[2] > v0[2]
    with pytest.raises(sg.SigmaError) as e:
        plan.add(z)
    assert e.value.code == 1 and "pattern changed" in str(e.value)
    S = R.ell(c.n, c.m, c.node, c.degrees)
    assert np.array_equal(bits(H.get("val", np.float64)), bits(R.apply_vectorised(S, c.val, i, j, z, "add")))
    sg.edit_plan(H, i, j).add(z)                       # a plan made afterwards works


@pytest.mark.parametrize("how,name", GRID, ids=IDS)
def test_add_sparse_matrix_with_the_matrix_as_the_added_operand(how, name):
    c = CASES[name]
    S = R.ell(c.n, c.m, c.node, c.degrees)
    v0 = np.cos(np.arange(c.val.size)).reshape(c.val.shape)
    A, B = handle(name, "given", val=v0), handle(name, how)
    A.add_sparse_matrix(B, alpha=0.375)
    i, j, z = R.matrix_triples(S, c.val, 0.375)
    assert len(i) == int(c.degrees.sum())
    assert np.array_equal(bits(A.get("val", np.float64)), bits(R.apply_vectorised(S, v0, i, j, z, "add")))


@pytest.mark.parametrize("how,name", GRID, ids=IDS)
def test_left_then_right_permute(how, name):
    orc, E, _ = oracle(name)
    c = CASES[name]
    rs = np.random.RandomState(17)
    p, q = (rs.permutation(c.n) + 1).astype(np.int32), (rs.permutation(c.m) + 1).astype(np.int32)
    node, val, deg = orc.ell_permuted(E, p, q)
    H = handle(name, how)
    H.left_permute(p)
    H.right_permute(q)
    assert np.array_equal(H.get("degrees", np.int32), deg)
    assert np.array_equal(H.get("node", np.int32).reshape(c.n, c.max_d), node)            # zeros kept
    assert np.array_equal(bits(H.get("val", np.float64)), bits(val))
    # ... and the permuted handle still multiplies like the oracle's permuted matrix
    Ep = orc.EllMatrix(c.n, c.m, c.max_d, np.where(node == 0, 1, node), val, deg)
    x = P.test_vector(c.m)
    assert np.array_equal(bits(H.matvec(x, np.zeros(c.n))), bits(Ep.matvec(x)))


@pytest.mark.parametrize("how,name", GRID, ids=IDS)
def test_text_dump(how, name, tmp_path):
    """A%to_file (sparse_matrix_interfaces.f90:601-653): `nrow ncol nnz`, then the cursor's entries -- row after row the first
    degrees(i) slots (ellpack_graphs.f90:310-369) -- one `i j value` line each; the values read back bit for bit"""
    c = CASES[name]
    f = tmp_path / "a.txt"
    handle(name, how).to_file(str(f))
    lines = open(f).read().split("\n")
    assert [int(t) for t in lines[0].split()] == [c.n, c.m, int(c.degrees.sum())]
    want = [(i + 1, int(c.node[i, k]), c.val[i, k]) for i in range(c.n) for k in range(int(c.degrees[i]))]
    got = [(int(a), int(b), float(v)) for a, b, v in (ln.split() for ln in lines[1:] if ln)]
    assert [(a, b) for a, b, _ in got] == [(a, b) for a, b, _ in want]
    assert np.array_equal(bits([v for _, _, v in got]), bits([v for _, _, v in want]))


@pytest.mark.parametrize("how,name", GRID, ids=IDS)
def test_jacobi_of_a_composite_with_such_a_leaf(how, name):
    orc, E, _ = oracle(name)
    c = CASES[name]
    ptr, node, val = P.poisson2d_csr(10, 7)
    S = sg.sparse_matrix([1, c.n + 1, c.n + 71], [1, c.n + 1, c.n + 71])
    S.set_submatrix(1, 1, handle(name, how))
    S.set_submatrix(2, 2, sg.csr_matrix(70, 70, ptr, node, val))
    pc = sg.jacobi()
    pc.setup(S)
    want = np.concatenate([orc.Jacobi(E).idiag, orc.Jacobi(orc.CsrMatrix(70, 70, ptr, node, val)).idiag])
    assert np.array_equal(bits(pc.idiag), bits(want))


# ------------------------------------------------------------------------------------------------ no degrees at all (shape 9)
def _readers(H, c, tmp_path):
    real = K.probes(c)[0]
    i, j = np.array([real[0][0]], np.int32), np.array([real[0][1]], np.int32)
    p = np.arange(1, c.n + 1, dtype=np.int32)

    def composite():
        S = sg.sparse_matrix([1, c.n + 1], [1, c.n + 1])
        S.set_submatrix(1, 1, H)
        sg.jacobi().setup(S)
    other = handle("1_add_edge_padding")
    return {"ildu": lambda: sg.ldu().setup(H), "jacobi": lambda: sg.jacobi().setup(H), "composite jacobi": composite,
            "get_value": lambda: H.get_value(i, j), "set_value": lambda: H.set_value(i, j, np.ones(1)),
            "add_value": lambda: H.add_value(i, j, np.ones(1)), "edit_plan": lambda: sg.edit_plan(H, i, j),
            "add_sparse_matrix (target)": lambda: H.add_sparse_matrix(other), "add_sparse_matrix (operand)": lambda: other.add_sparse_matrix(H),
            "left_permute": lambda: H.left_permute(p), "right_permute": lambda: H.right_permute(p),
            "get degrees": lambda: H.get("degrees", np.int32), "to_file": lambda: H.to_file(str(tmp_path / "x.txt"))}


@pytest.mark.parametrize("name", K.UNKNOWN)
def test_without_degrees_every_reader_refuses_and_the_products_stay(name, tmp_path):
    c = CASES[name]
    H = handle(name, "recovered")
    before = versions(H)
    for what, call in _readers(H, c, tmp_path).items():
        with pytest.raises(sg.SigmaError) as e:
            call()
        assert e.value.code == 8 and "sgm_ell_set_degrees" in str(e.value), what
    assert versions(H) == before
    assert np.array_equal(H.get("node", np.int32).reshape(c.n, c.max_d), c.node) and np.array_equal(bits(H.get("val", np.float64)), bits(c.val))
    want = product_refs(name)[4]
    got = products(H, name)
    for k in want:
        assert np.array_equal(bits(got[k]), bits(want[k])), k
    # handing the degrees in afterwards opens every reader
    H.set_degrees(c.degrees)
    for what, call in _readers(H, c, tmp_path).items():
        if what not in ("left_permute", "right_permute", "set_value", "add_value", "add_sparse_matrix (target)"):      # (these change H)
            call()
    assert np.array_equal(H.get("degrees", np.int32), c.degrees)


@pytest.mark.parametrize("name", K.DELETED)
def test_documented_limit_rows_delete_edge_left_behind(name):
    """CHARACTERISATION of the limit stated in include/sigma_hip.h, not a parity test: a row delete_edge has worked on can be
    slot for slot an add_edge row with one more neighbour, so WITHOUT the degrees argument the handle recovers one too many on
    those rows.  No reader is compared with the oracle in this state: whoever holds such arrays must pass degrees."""
    c = CASES[name]
    got = handle(name, "recovered").get("degrees", np.int32)
    sp = np.array(c.special) - 1
    assert np.array_equal(got, c.recovered) and np.all(got[sp] == c.degrees[sp] + 1)


# ------------------------------------------------------------------------------------------------ validation
def _bad_degrees(name):
    c = CASES[name]
    s = c.special[0] - 1
    out = {}
    for what, d in (("negative", -1), ("beyond max_d", c.max_d + 1)):
        out[what] = c.degrees.copy()
        out[what][s] = d
    zero_rows = np.nonzero((c.node == 0).any(axis=1))[0]
    if len(zero_rows):                                  # a degree that takes a 0 slot for a column
        r = int(zero_rows[0])
        out["covers a 0 slot"] = c.degrees.copy()
        out["covers a 0 slot"][r] = int(np.nonzero(c.node[r] == 0)[0][0]) + 1
    return out


@pytest.mark.parametrize("name", ["1_add_edge_padding", "3_empty_row", "8_zero_tail", "4_last_neighbour_deleted", "max_d_one"])
def test_bad_degrees_are_refused_and_the_handle_keeps_its_own(name):
    orc, E, _ = oracle(name)
    c = CASES[name]
    H = handle(name, "given")
    before = versions(H)
    bad = _bad_degrees(name)
    assert name not in ("3_empty_row", "8_zero_tail", "max_d_one") or "covers a 0 slot" in bad
    for what, deg in bad.items():
        with pytest.raises(sg.SigmaError) as e:
            H.set_degrees(deg)
        assert e.value.code == 2, what
        with pytest.raises(sg.SigmaError) as e:         # ... and at create: no handle is left behind
            sg.ellpack_matrix(c.n, c.m, c.node, c.val, degrees=deg)
        assert e.value.code == 2, what
    with pytest.raises(sg.SigmaError) as e:
        H.set_degrees(c.degrees[:-1])
    assert e.value.code == 2
    assert versions(H) == before and np.array_equal(H.get("degrees", np.int32), c.degrees)
    pc = sg.jacobi()
    pc.setup(H)
    assert np.array_equal(bits(pc.idiag), bits(orc.Jacobi(E).idiag))
