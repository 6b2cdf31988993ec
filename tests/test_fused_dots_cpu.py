"""The reference of tests/test_gpu_fused_dots.py checked on its own, without a GPU: exact_dot against rational arithmetic, the
conditions that make `==` the right comparison on the `int` data, the bars of the `real` data met by the oracle's own dot in
more than one order, and the case list against the table of kernel families."""
import ctypes as C

import numpy as np
import pytest

import fused_dot_cases as F

SMALL = [c.name for c in F.CASES if F.structure(c.name)["n"] <= 5000]


def _oracle_dot(a, b):
    """The oracle's left-to-right double dot."""
    import oracle as orc
    orc.set_dot_mode(0)
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return float(orc.lib().orc_dot(C.c_int32(a.size), a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p)))


def test_two_product_is_error_free():
    rs = np.random.RandomState(1)
    a = np.concatenate([rs.standard_normal(300), rs.standard_normal(100) * 1e150, rs.standard_normal(100) * 1e-140, [3.0, -2.0, 0.0]])
    b = np.concatenate([rs.standard_normal(300), rs.standard_normal(100) * 1e-150, rs.standard_normal(100) * 1e140, [3.0, 1.0, 5.0]])
    p, e = F.two_product(a, b)
    for k in range(a.size):
        assert F.Fraction(p[k]) + F.Fraction(e[k]) == F.Fraction(a[k]) * F.Fraction(b[k]), k


@pytest.mark.parametrize("name", SMALL)
def test_exact_dot_is_the_correctly_rounded_rational_sum(name):
    """exact_dot == the Fraction sum rounded once, on both data sets of every case of at most 5000 rows, y = A x and y0 + A x,
    and whatever the order of the operands."""
    rs = np.random.RandomState(len(name))
    for data in F.DATASETS:
        R = F.reference(name, data)
        perm = rs.permutation(R.n)
        for add in (0, 1):
            y = R.y[add]
            for a, b in ((R.w, y), (y, y)):
                d = F.exact_dot(a, b)
                assert d == float(F.fraction_dot(a, b)), (name, data, add)      # (Fraction -> float rounds to nearest even)
                assert F.exact_dot(a[perm], b[perm]) == d, (name, data, add)


def test_exact_dot_at_the_largest_case_is_permutation_invariant():
    R = F.reference("sl_banded_1048573_w3", "real")
    perm = np.random.RandomState(2).permutation(R.n)
    assert F.exact_dot(R.w[perm], R.y[0][perm]) == R.wy[0][0]
    assert F.exact_dot(R.y[0][perm], R.y[0][perm]) == R.yy[0][0]


@pytest.mark.parametrize("name", [c.name for c in F.CASES])
def test_int_cases_meet_the_conditions_for_exact_equality(name):
    """Every product and partial sum an integer below 2^53 in any order (sum |w y| and sum y^2 below 2^53, integer operands),
    y_i >= 1 on every non-empty row, and the oracle's own dot -- left to right, and over a random permutation -- == exact_dot."""
    R = F.reference(name, "int")
    st = F.structure(name)
    for v in (R.x, R.w, R.y0, R.y[0], R.y[1]):
        assert np.array_equal(v, np.rint(v))
    assert set(np.unique(R.x)) <= {1.0, 2.0, 3.0} and set(np.unique(np.abs(R.w))) <= {1.0, 2.0, 3.0}
    assert np.abs(R.y0).max() <= 3.0
    assert (R.y[0][R.nonempty] >= 1.0).all() and (R.y[0][~R.nonempty] == 0.0).all()
    perm = np.random.RandomState(3).permutation(R.n)
    for add in (0, 1):
        y = R.y[add]
        assert sum(R.abs_wy[add]) < F.TWO53 and sum(R.abs_yy[add]) < F.TWO53
        assert _oracle_dot(R.w, y) == sum(R.wy[add]) == _oracle_dot(R.w[perm], y[perm])
        assert _oracle_dot(y, y) == sum(R.yy[add]) == _oracle_dot(y[perm], y[perm])
        for ip, (a, b) in enumerate(R.parts):
            assert _oracle_dot(R.w[a:b], y[a:b]) == R.wy[add][ip] and _oracle_dot(y[a:b], y[a:b]) == R.yy[add][ip]
    assert len(R.parts) == max(1, R.case.nparts) and R.parts[0][0] == 0 and R.parts[-1][1] == st["n"]


@pytest.mark.parametrize("name", [c.name for c in F.CASES])
def test_real_cases_the_oracles_dot_meets_the_bar_in_two_orders(name):
    """|dot - exact| <= gamma_n * sum |w y| (resp. gamma_n * sum y^2) for the oracle's left-to-right dot and for the same over a
    random permutation: the bar holds for the reference alone, whatever the order."""
    R = F.reference(name, "real")
    perm = np.random.RandomState(4).permutation(R.n)
    for add in (0, 1):
        y = R.y[add]
        g = F.gamma(R.n)
        for a, b, ex, bar in ((R.w, y, F.exact_dot(R.w, y), g * np.abs(R.w * y).sum()), (y, y, F.exact_dot(y, y), g * (y * y).sum())):
            for d in (_oracle_dot(a, b), _oracle_dot(a[perm], b[perm]), float(np.dot(a, b))):
                assert abs(d - ex) <= bar, (name, add, d, ex, bar)


def test_every_family_of_the_table_has_its_cases():
    """The case list names every family of the table; every kernel family among them is reached by a case of its own name; each
    family has a case at the smallest count its launch geometry allows (1, or 8 for a CSR row range) and one above it; one part's
    sum y^2 passes 2^24 (a float accumulator would not be exact there); the partitions cut an inner part into two ranges or more."""
    fams = {}
    for c in F.CASES:
        fams.setdefault(c.family, []).append(c)
    assert tuple(sorted(fams)) == tuple(sorted(F.FAMILIES))
    assert {c.key for c in F.CASES} == set(F.KERNEL_KEYS)
    for fam, cases in fams.items():
        if fam in F.KERNEL_KEYS:
            assert all(c.key == fam for c in cases), fam
        counts = [cnt for c in cases for cnt in F.reference(c.name, "int").count]
        lo = min(c.min_grid for c in cases)
        assert min(counts) == lo and max(counts) > lo, (fam, counts)
        assert max(counts) <= 8192
        assert any(v > F.TWO24 for c in cases for v in F.reference(c.name, "int").abs_yy[0]), fam
    for c in F.CASES:           # the long-row cases are regular enough for the SELL form (the library builds it up to 30 % padding)
        if c.key.startswith("k_csr_sell"):
            assert F.sell_padding(F.structure(c.name)) <= 1.25, c.name
    for c in fams["partition"]:
        R = F.reference(c.name, "int")
        assert len(R.parts) == c.nparts and all(b > a for a, b in R.parts)
        if c.nparts == 3:
            assert len(R.ranges[1]) >= 2 and R.count[1] == sum(F.range_grid(b - a, 512, 8) for a, b in R.ranges[1])


def test_kernel_key_reads_the_names_the_library_reports():
    for kernel, fmt, key in (("k_csr_sl<W=5>", "csr", "k_csr_sl"), ("k_csr_sl<W=5>", "ell", "sliced ellpack"), ("k_csr_slb<W=27>", "csr", "k_csr_slb"),
                             ("k_csr_sl32<W=16>", "csr", "k_csr_sl32"), ("k_csr_do<256,1536,CW=1>", "csr", "k_csr_do CW=1"),
                             ("k_csr_do<256,4096,CW=4>", "csr", "k_csr_do CW=4"), ("k_csr_sell<pad=1.043,xw=1114x1>", "csr", "k_csr_sell xw"),
                             ("k_csr_sell<pad=1.043>", "csr", "k_csr_sell"), ("k_csr_rl", "csr", "k_csr_rl"), ("k_csr_spmv", "csr", "k_csr_spmv"),
                             ("k_ellcb<cols=256,R=256>", "ell", "k_ellcb ell"), ("k_ellcb<cols=256,R=256,csr>", "csr", "k_ellcb csr"),
                             ("k_ell_spmv", "ell", "k_ell_spmv"), ("k_ell_do<MDP=16>", "ell", "k_ell_do<16>"), ("composite", "composite", "composite")):
        assert F.kernel_key(kernel, fmt) == key
