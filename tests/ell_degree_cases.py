"""ELLPACK rows whose degrees the padding cannot tell -- host only, numpy only.

An ellpack_graph keeps node(max_d, n) and degrees(n) (ellpack_graphs.f90:14-21): the first degrees(i) slots of row i are its
neighbours, the rest is padding.  Here:

  * EllGraph: what add_edge (ellpack_graphs.f90:379-413), add_edge_with_reallocation (:600-639) and delete_edge (:418-481) do to
    node(:, i) and degrees(i), statement for statement (node is kept as a C array (n, max_d) = the Fortran (max_d, n));
  * the two recovery rules restated: old_rule_degrees (first occurrence of the last slot's column; a last slot of 0 means 0 -- what
    sgm_ell_create did for every handle) and recovered_degrees (the rule of include/sigma_hip.h: three row shapes, -1 otherwise);
  * builders: one matrix per row shape (CASES), each a Case whose first six fields are (n, m, max_d, node, val, degrees) -- the
    arguments of oracle.EllMatrix -- with the special rows mixed among ordinary ones;
  * dense_real: the dense, plain-Python statement every reader of degrees is held to: the real entries of row i are its first
    degrees(i) slots, and of a column stored twice the last one answers (ellpack_matrix_get_value, ellpack_matrices.f90:232-235).
"""
from collections import namedtuple

import numpy as np

N = 300
BAND = (0, -1, 1, -9, 9)          # insertion order of an ordinary row: the diagonal first

Case = namedtuple("Case", "n m max_d node val degrees name spd special recovered")
# spd: symmetric, strictly diagonally dominant with a positive diagonal and no value outside the real entries -> PCG is meaningful
# special: the 1-based rows that carry the shape; recovered: what recovered_degrees must answer (None: -1 somewhere = no degrees)


class EllGraph:
    def __init__(self, n, max_d=0):
        self.n, self.max_d = int(n), int(max_d)
        self.node = np.zeros((self.n, self.max_d), np.int32)
        self.degrees = np.zeros(self.n, np.int32)
        self.ne = 0

    def connected(self, i, j):                          # ellpack_graphs.f90:236-255: the first degrees(i) slots
        return bool(np.any(self.node[i - 1, :self.degrees[i - 1]] == j))

    def add_edge(self, i, j):                           # :379-413
        if self.connected(i, j):
            return
        k = int(self.degrees[i - 1])
        if k < self.max_d:
            self.node[i - 1, k:] = j                    # :397 the whole rest of the row
            self.degrees[i - 1] += 1
            self.ne += 1
        else:
            self._add_edge_with_reallocation(i, j)

    def _add_edge_with_reallocation(self, i, j):        # :600-639
        node = np.zeros((self.n, self.max_d + 1), np.int32)
        node[:, :self.max_d] = self.node
        if self.max_d > 0:
            node[:, self.max_d] = node[:, self.max_d - 1]           # :618-622 every row repeats its last slot
        node[i - 1, self.max_d] = j
        self.node = node
        self.ne += 1
        self.degrees[i - 1] += 1
        self.max_d += 1

    def delete_edge(self, i, j):                        # :418-481
        if not self.connected(i, j):
            return
        d = self.max_d
        if d < 2:
            raise ValueError("delete_edge with max_d = 1 reads node(0, i) in the reference (:450): not restated")
        max_degree_decrease = self.degrees[i - 1] == d
        row = self.node[i - 1]
        indx = int(np.nonzero(row == j)[0][0])          # :439-441 the first slot holding j, of all max_d
        row[indx:d - 1] = row[indx + 1:d].copy()        # :444 shift left
        row[d - 1] = row[d - 2]                         # :449-451 the last slot copies its left neighbour
        self.ne -= 1
        self.degrees[i - 1] -= 1
        if max_degree_decrease:                         # :461-477 the array shrinks with the largest degree
            self.max_d = int(self.degrees.max())
            if self.max_d < d:
                self.node = np.ascontiguousarray(self.node[:, :self.max_d])


def old_rule_degrees(node):
    """The rule sgm_ell_create used for every handle: degrees(i) = first occurrence of the last slot's column, 0 when it is 0."""
    node = np.asarray(node, np.int32)
    n, md = node.shape
    deg = np.zeros(n, np.int32)
    for i in range(n):
        last = node[i, md - 1] if md else 0
        if last != 0:
            d = 1
            while d < md and node[i, d - 1] != last:
                d += 1
            deg[i] = d
    return deg


def recovered_degrees(node):
    """The rule of include/sigma_hip.h (sgm_ell_set_degrees): d distinct nonzero columns followed by copies of the d-th (add_edge),
    all zero, or d distinct nonzero columns followed by zeros; -1 for every other row."""
    node = np.asarray(node, np.int32)
    n, md = node.shape
    deg = np.zeros(n, np.int32)
    for i in range(n):
        row = [int(c) for c in node[i]]
        z = next((k for k, c in enumerate(row) if c == 0), md)
        if z < md:
            d = z if all(c == 0 for c in row[z:]) else -1
        elif md == 0:
            d = 0
        else:
            d = row.index(row[-1]) + 1
            if any(c != row[-1] for c in row[d:]):
                d = -1
        if d > 0 and len(set(row[:d])) != d:
            d = -1
        deg[i] = d
    return deg


# ------------------------------------------------------------------------------------------------ values
def _offdiag(i, j):
    a, b = min(i, j), max(i, j)
    return -(1.0 + (a * 31 + b * 17) % 7) / 8.0          # symmetric in (i, j), exact in binary


def real_values(node, degrees):
    """Values on the real entries only: a symmetric off-diagonal function, the diagonal (where it is a real entry) strictly
    dominant; +0.0 in every padding slot."""
    n, md = node.shape
    val = np.zeros((n, md))
    for i in range(n):
        s = 0.0
        for k in range(int(degrees[i])):
            j = int(node[i, k])
            if j != i + 1:
                val[i, k] = _offdiag(i + 1, j)
                s += abs(val[i, k])
        for k in range(int(degrees[i])):
            if node[i, k] == i + 1:
                val[i, k] = 1.0 + s
    return val


def dense_real(case):
    """(D, present): D[i, j] = the value of the LAST of the first degrees(i) slots of row i holding column j + 1, present[i, j]
    whether there is one.  Plain loops on purpose."""
    D = np.zeros((case.n, case.m))
    present = np.zeros((case.n, case.m), bool)
    for i in range(case.n):
        for k in range(int(case.degrees[i])):
            j = int(case.node[i, k]) - 1
            D[i, j] = case.val[i, k]
            present[i, j] = True
    return D, present


def probes(c):
    """(real (i, j) pairs, padding-only (i, j) pairs, absent (i, j) pairs), 1-based: a padding-only column stands in a slot of
    the row past degrees(i) and in none of the first degrees(i)"""
    D, present = dense_real(c)
    real = [(i + 1, int(j) + 1) for i in range(c.n) for j in np.nonzero(present[i])[0]]
    pad = sorted({(i + 1, int(col)) for i in range(c.n) for col in c.node[i, c.degrees[i]:] if col != 0 and not present[i, col - 1]})
    absent = []
    for i in list(np.array(c.special) - 1) + [0, c.n - 1]:
        j = next(j for j in range(c.m) if not present[i, j] and (i + 1, j + 1) not in pad)
        absent.append((int(i) + 1, j + 1))
    return real, pad, absent


# ------------------------------------------------------------------------------------------------ builders
def _band_rows(n):
    return {i: [i + o for o in BAND if 1 <= i + o <= n] for i in range(1, n + 1)}


def _random_rows(n, seed, per_row=2):
    """a symmetric pattern with scattered columns: the diagonal, then every pair (i, j) in both rows"""
    rs = np.random.RandomState(seed)
    rows = {i: [i] for i in range(1, n + 1)}
    for i in range(1, n + 1):
        for j in rs.randint(1, n + 1, size=per_row):
            j = int(j)
            if j != i and j not in rows[i]:
                rows[i].append(j)
                rows[j].append(i)
    return rows


def _drop(rows, i, j):
    """edge (i, j) and (j, i) never inserted"""
    if j in rows[i]:
        rows[i].remove(j)
    if i != j and i in rows[j]:
        rows[j].remove(i)


def _graph(n, rows, max_d=0):
    g = EllGraph(n, max_d)
    for i in range(1, n + 1):
        for j in rows[i]:
            g.add_edge(i, j)
    return g


def _case(name, g, spd, special, recovered, node=None, val=None, degrees=None):
    node = np.ascontiguousarray(g.node if node is None else node, np.int32)
    degrees = np.ascontiguousarray(g.degrees if degrees is None else degrees, np.int32)
    val = real_values(node, degrees) if val is None else val
    rec = None if recovered is None else np.ascontiguousarray(recovered, np.int32)
    return Case(g.n, g.n, node.shape[1], node, np.ascontiguousarray(val), degrees, name, spd, tuple(special), rec)


SPECIAL = (12, 64, 129, 200, 256, 288)              # interior rows of the band (full rows of five), far enough apart


def shape1_add_edge_padding():
    """control: rows as add_edge leaves them, the ones near the ends of the band padded with their last neighbour"""
    g = _graph(N, _band_rows(N))
    return _case("1_add_edge_padding", g, True, (1, 2, 9, N - 8, N), g.degrees)


def shape2_full_row():
    """scattered columns; the special rows alone fill all max_d slots with distinct columns"""
    rows = _random_rows(N, 11)
    md = max(len(r) for r in rows.values())
    for s in SPECIAL:
        j = 1
        while len(rows[s]) < md + 2:
            if j != s and j not in rows[s] and len(rows[j]) < md:
                rows[s].append(j)
                rows[j].append(s)
            j += 7
    g = _graph(N, rows)
    assert all(g.degrees[s - 1] == g.max_d for s in SPECIAL)
    return _case("2_full_row", g, True, SPECIAL, g.degrees)


def shape3_empty_row():
    """rows without any edge keep node(:, i) = 0, degree 0 (and nobody points at them)"""
    rows = _band_rows(N)
    for s in SPECIAL:
        for j in list(rows[s]):
            _drop(rows, s, j)
    g = _graph(N, rows)
    assert all(np.all(g.node[s - 1] == 0) for s in SPECIAL)
    return _case("3_empty_row", g, False, SPECIAL, g.degrees)


def shape4_last_neighbour_deleted():
    """[s, s-1, s+1, s+1, s+1] with degree 3, delete_edge(s, s+1): the row keeps its slots and has degree 2 -- the padding says 3"""
    rows = _band_rows(N)
    for s in SPECIAL:
        _drop(rows, s, s - 9)
        _drop(rows, s, s + 9)
    g = _graph(N, rows)
    for s in SPECIAL:
        before = g.node[s - 1].copy()
        g.delete_edge(s, s + 1)
        g.delete_edge(s + 1, s)                     # (a middle neighbour there: the matrix stays symmetric)
        assert np.array_equal(g.node[s - 1], before) and g.degrees[s - 1] == 2
    rec = g.degrees.copy()
    rec[[s - 1 for s in SPECIAL]] = 3
    return _case("4_last_neighbour_deleted", g, True, SPECIAL, rec)


def shape5_only_neighbour_deleted():
    """[s, s, s, s, s] with degree 1, delete_edge(s, s): the same slots, degree 0 -- the padding says 1"""
    rows = _band_rows(N)
    for s in SPECIAL:
        for j in list(rows[s]):
            if j != s:
                _drop(rows, s, j)
    g = _graph(N, rows)
    for s in SPECIAL:
        g.delete_edge(s, s)
        assert np.all(g.node[s - 1] == s) and g.degrees[s - 1] == 0
    rec = g.degrees.copy()
    rec[[s - 1 for s in SPECIAL]] = 1
    return _case("5_only_neighbour_deleted", g, False, SPECIAL, rec)


def shape6_diagonal_deleted_last():
    """[s-1, s+1, s, s, s] with degree 3, delete_edge(s, s): the diagonal stays in the slots and is no entry any more"""
    rows = _band_rows(N)
    for s in SPECIAL:
        _drop(rows, s, s - 9)
        _drop(rows, s, s + 9)
        rows[s] = [s - 1, s + 1, s]
    g = _graph(N, rows)
    for s in SPECIAL:
        g.delete_edge(s, s)
        assert list(g.node[s - 1]) == [s - 1, s + 1, s, s, s] and g.degrees[s - 1] == 2
    rec = g.degrees.copy()
    rec[[s - 1 for s in SPECIAL]] = 3
    return _case("6_diagonal_deleted_last", g, False, SPECIAL, rec)


def shape7_middle_neighbour_deleted():
    """second control: delete_edge of a middle neighbour shifts the row left and leaves an add_edge-shaped row"""
    g = _graph(N, _band_rows(N))
    for s in SPECIAL:
        g.delete_edge(s, s + 1)
        g.delete_edge(s + 1, s)
        assert list(g.node[s - 1]) == [s, s - 1, s - 9, s + 9, s + 9] and g.degrees[s - 1] == 4
    return _case("7_middle_neighbour_deleted", g, True, SPECIAL, g.degrees)


def shape8_zero_tail():
    """a caller's padding: [s, s-1, 0, 0, 0] with degree 2 (the old rule reads the last slot, 0, as an empty row)"""
    rows = _band_rows(N)
    for s in SPECIAL:
        for j in (s + 1, s - 9, s + 9):
            _drop(rows, s, j)
    g = _graph(N, rows)
    node = g.node.copy()
    for s in SPECIAL:
        node[s - 1, 2:] = 0
    return _case("8_zero_tail", g, True, SPECIAL, g.degrees, node=node)


def shape9_repeated_column():
    """a caller's full row that stores a column twice, with different values, degree max_d: [s, s-1, s+1, s-9, s-1] on every
    second special row, and on the others [s, s-1, s+1, s-9, s] -- the DIAGONAL twice, so that get_value(s, s), and with it
    Jacobi's idiag, is the later slot's value and not the first one's.  The product counts both slots."""
    g = _graph(N, _band_rows(N))
    node = g.node.copy()
    val = real_values(node, g.degrees)
    for t, s in enumerate(SPECIAL):
        assert g.degrees[s - 1] == g.max_d and node[s - 1, 0] == s
        node[s - 1, g.max_d - 1] = node[s - 1, t % 2]
        val[s - 1, g.max_d - 1] = 0.25 * val[s - 1, t % 2]
    return _case("9_repeated_column", g, False, SPECIAL, None, node=node, val=val)


def shape10_values_in_padding():
    """add_edge-shaped rows with nonzero values in their padding slots: the product counts them, readers of degrees do not"""
    rows = _band_rows(N)
    for s in SPECIAL:
        _drop(rows, s, s - 9)
        _drop(rows, s, s + 9)
    g = _graph(N, rows)
    val = real_values(g.node, g.degrees)
    for s in SPECIAL:
        val[s - 1, 3:] = (0.5, -0.25)
    return _case("10_values_in_padding", g, False, SPECIAL, g.degrees, val=val)


def max_d_one():
    """max_d = 1: a diagonal matrix, some rows empty"""
    rows = {i: ([] if i % 50 == 7 else [i]) for i in range(1, N + 1)}
    g = _graph(N, rows)
    assert g.max_d == 1
    return _case("max_d_one", g, False, tuple(i for i in range(1, N + 1) if i % 50 == 7), g.degrees)


def one_row_only():
    """empty apart from one row"""
    rows = {i: [] for i in range(1, N + 1)}
    rows[150] = [150, 3, 299]
    g = _graph(N, rows)
    return _case("one_row_only", g, False, (150,), g.degrees)


BUILDERS = (shape1_add_edge_padding, shape2_full_row, shape3_empty_row, shape4_last_neighbour_deleted,
            shape5_only_neighbour_deleted, shape6_diagonal_deleted_last, shape7_middle_neighbour_deleted, shape8_zero_tail,
            shape9_repeated_column, shape10_values_in_padding, max_d_one, one_row_only)
_CACHE = {}


def cases():
    """every Case, built once (read-only: copy before changing)"""
    if not _CACHE:
        for b in BUILDERS:
            c = b()
            for a in (c.node, c.val, c.degrees):
                a.setflags(write=False)
            _CACHE[c.name] = c
    return _CACHE


NAMES = ("1_add_edge_padding", "2_full_row", "3_empty_row", "4_last_neighbour_deleted", "5_only_neighbour_deleted",
         "6_diagonal_deleted_last", "7_middle_neighbour_deleted", "8_zero_tail", "9_repeated_column", "10_values_in_padding",
         "max_d_one", "one_row_only")
DELETED = ("4_last_neighbour_deleted", "5_only_neighbour_deleted", "6_diagonal_deleted_last")     # recovered, and wrong (documented)
UNKNOWN = ("9_repeated_column",)                                                                   # no degrees without the argument
RECOVERABLE = tuple(n for n in NAMES if n not in DELETED + UNKNOWN)                                # recovered, and right
