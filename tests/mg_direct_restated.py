"""The contract of multigrid's direct coarse solve (option "mg_coarse_direct"), restated twice.

Setup, on the coarsest level A_L of n rows:

    D(i,j) = +0.0 plus the stored copies of (i,j) in stored order (duplicates summed, absent entries +0.0)
    W = [D | I];  for k = 0 .. n-1:
        p = the smallest i >= k that maximises fabs(W(i,k)), a NaN larger than everything (np.argmax of the absolute values)
        W(p,k) is 0, NaN or +-Inf: refused (Refused.step = k + 1)
        piv(k) = p + 1 ; rows k and p swapped
        W(k,j) = W(k,j) / W(k,k) for every j, the divisor taken before the row is scaled
        every i != k: f = W(i,k) read before the update, W(i,j) = W(i,j) - (f * W(k,j)) for every j
    Ainv = the right block

Apply: columns in chunks of 256; s_c(i) = +0.0 plus the individually rounded products Ainv(i,j) * b(j) in ascending j;
x(i) = +0.0 plus s_0(i), s_1(i), ... in ascending c.  vcycle(L, b) returns that x; the levels above are mg_restated's.

* `invert_literal` / `apply_literal` / `Literal` transcribe this element by element: slow, for small n.
* `invert_vectorised` / `apply_vectorised` / `Vectorised` do one elimination step (one column of the product) at a time."""
import numpy as np

import mg_restated as MG

CHUNK = 256
MAX_ROWS = 4096


class Refused(Exception):
    def __init__(self, step, n):
        super().__init__(f"singular or non-finite coarse level ({n} rows) at elimination step {step}")
        self.step = step


def dense(M):
    """D of step 1, entry by entry in stored order"""
    n, _, ptr, node, val = MG._csr0(M)
    D = np.zeros((n, n))
    for i in range(n):
        for e in range(ptr[i], ptr[i + 1]):
            D[i, node[e]] = D[i, node[e]] + val[e]
    return D


def _bad(v):
    return v == 0.0 or not np.isfinite(v)


# ------------------------------------------------------------------------------------ literal
def invert_literal(D):
    n = D.shape[0]
    W = [[np.float64(D[i, j]) for j in range(n)] + [np.float64(1.0 if i == j else 0.0) for j in range(n)] for i in range(n)]
    piv = np.zeros(n, np.int32)
    with np.errstate(all="ignore"):
        for k in range(n):
            p = k
            for i in range(k, n):
                a, best = abs(W[i][k]), abs(W[p][k])
                if (np.isnan(a) and not np.isnan(best)) or a > best:          # strictly larger: the smallest index stays
                    p = i
            if _bad(W[p][k]):
                raise Refused(k + 1, n)
            piv[k] = p + 1
            W[k], W[p] = W[p], W[k]
            d = W[k][k]
            for j in range(2 * n):
                W[k][j] = W[k][j] / d
            for i in range(n):
                if i == k:
                    continue
                f = W[i][k]
                for j in range(2 * n):
                    W[i][j] = W[i][j] - (f * W[k][j])
    return np.array([[W[i][n + j] for j in range(n)] for i in range(n)], np.float64).reshape(n, n), piv


def apply_literal(Ainv, b):
    n = Ainv.shape[0]
    x = np.empty(n)
    with np.errstate(all="ignore"):
        for i in range(n):
            z = np.float64(0.0)
            for c0 in range(0, n, CHUNK):
                s = np.float64(0.0)
                for j in range(c0, min(c0 + CHUNK, n)):
                    s = s + np.float64(Ainv[i, j]) * np.float64(b[j])
                z = z + s
            x[i] = z
    return x


# ------------------------------------------------------------------------------------ vectorised per elimination step
def invert_vectorised(D):
    n = D.shape[0]
    W = np.hstack([np.asarray(D, np.float64), np.eye(n)])
    piv = np.zeros(n, np.int32)
    with np.errstate(all="ignore"):
        for k in range(n):
            p = k + int(np.argmax(np.abs(W[k:, k])))
            if _bad(W[p, k]):
                raise Refused(k + 1, n)
            piv[k] = p + 1
            if p != k:
                W[[k, p]] = W[[p, k]]
            W[k] = W[k] / W[k, k]
            f = W[:, k].copy()
            row = W[k].copy()
            W -= f[:, None] * row[None, :]
            W[k] = row
    return W[:, n:].copy(), piv


def apply_vectorised(Ainv, b):
    n = Ainv.shape[0]
    x = np.zeros(n)
    with np.errstate(all="ignore"):
        for c0 in range(0, n, CHUNK):
            s = np.zeros(n)
            for j in range(c0, min(c0 + CHUNK, n)):
                s = s + Ainv[:, j] * b[j]
            x = x + s
    return x


# ------------------------------------------------------------------------------------ the V-cycle with that coarse level
class _Direct:
    """replaces the l == L branch of a mg_restated class"""
    _invert = _apply = None

    def _setup_direct(self):
        M = self.lev[-1]
        if M[0] > MAX_ROWS:
            raise ValueError(f"the coarsest level has {M[0]} rows, the limit is {MAX_ROWS}")
        self.D = dense(M)
        self.Ainv, self.piv = type(self)._invert(self.D)

    def vcycle(self, l, b):
        if l == len(self.lev) - 1:
            return type(self)._apply(self.Ainv, np.asarray(b, np.float64))
        return super().vcycle(l, b)


class Literal(_Direct, MG.Literal):
    _invert, _apply = staticmethod(invert_literal), staticmethod(apply_literal)

    def __init__(self, A, Ps, omega, nu_pre, nu_post, coarse_sweeps=8, lev=None):
        MG.Literal.__init__(self, A, Ps, omega, nu_pre, nu_post, coarse_sweeps, lev=lev)
        self._setup_direct()


class Vectorised(_Direct, MG.Vectorised):
    _invert, _apply = staticmethod(invert_vectorised), staticmethod(apply_vectorised)

    def __init__(self, A, Ps, omega, nu_pre, nu_post, coarse_sweeps=8, lev=None):
        MG.Vectorised.__init__(self, A, Ps, omega, nu_pre, nu_post, coarse_sweeps, lev=lev)
        self._setup_direct()


# ------------------------------------------------------------------------------------ the test problems
def golden_csr(name):
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".npz"))
    ptr, node, val = g["ref_ptr"], g["ref_node"], g["ref_val"]
    n = len(ptr) - 1
    return n, n, np.asarray(ptr, np.int32), np.asarray(node, np.int32), np.asarray(val, np.float64)


def from_rows(rows, ncol=None):
    """rows: list of lists of (column (0-based), value), in stored order"""
    ptr = np.cumsum([0] + [len(r) for r in rows]) + 1
    node = np.array([c + 1 for r in rows for c, _ in r], np.int32)
    val = np.array([v for r in rows for _, v in r], np.float64)
    return len(rows), len(rows) if ncol is None else ncol, ptr.astype(np.int32), node, val


def poisson(nx, ny):
    from sigma_amd import problems as Pr
    ptr, node, val = Pr.poisson2d_csr(nx, ny)
    return nx * ny, nx * ny, ptr, node, val


def pivoting_case():
    """A 6 x 6 symmetric fine matrix with a unit-ish diagonal and the piecewise-constant P over pairs of rows, made by hand so
    that the Galerkin level is [[0, 2, 1], [2, 0, 0], [1, 0, 3]] (the pairs (0,1) and (2,3) are [[1, -1], [-1, 1]] blocks,
    which sum to an exact zero): a zero on the diagonal at step 1, rows 1 and 2 are swapped, piv = [2, 2, 3]."""
    rows = [[(0, 1.0), (1, -1.0), (2, 2.0)],
            [(0, -1.0), (1, 1.0), (4, 1.0)],
            [(0, 2.0), (2, 1.0), (3, -1.0)],
            [(2, -1.0), (3, 1.0)],
            [(1, 1.0), (4, 1.5)],
            [(5, 1.5)]]
    return from_rows(rows), [MG.piecewise_constant(6, width=2)]


def tie_case():
    """no P: column 1 holds 1, -3, 3 -- rows 2 and 3 tie in absolute value and the smaller index wins: piv[0] = 2"""
    return from_rows([[(0, 1.0), (1, 1.0)], [(0, -3.0), (1, 2.0), (2, 1.0)], [(0, 3.0), (1, -4.0), (2, 5.0)]]), []


def zero_row_case(n=7, zero=4):
    """a tridiagonal matrix whose row AND column `zero` (0-based) hold nothing but a stored 0.0 (what an empty column of P
    leaves in P^T A P).  The rows before it are diagonally dominant and keep nonzero pivots, so column `zero` is all zero when
    its step comes: refused at step zero + 1 exactly."""
    rows = [[(j, 4.0 if j == i else -1.0) for j in (i - 1, i, i + 1) if 0 <= j < n and j != zero] for i in range(n)]
    rows[zero] = [(zero, 0.0)]
    return from_rows(rows), []


def cases():
    """name -> (A, [P ...]): the coarse levels of the tests, smallest first by what they exercise"""
    A, Ps = MG.random_spd_case()
    adv = golden_csr("advdiff1d_csr_1024")
    return {
        "spd19": (A, Ps),                                                       # less than one wave and one chunk
        "spd75": (A, Ps[:1]),
        "spd128_L0": (golden_csr("random_spd_128"), []),                        # L = 0: exactly two 64-row blocks
        "advdiff256": (adv, [MG.piecewise_constant(adv[0], width=4)]),          # non-symmetric, exactly one chunk
        "dup16_L0": (golden_csr("duplicates_csr_16"), []),                      # duplicate stored entries in step 1
        "one_row": (poisson(5, 5), [MG.piecewise_constant(25, width=25)]),
        "pivoting": pivoting_case(),
        "tie_L0": tie_case(),
    }


SPD = ("spd19", "spd75", "spd128_L0", "one_row")
LITERAL = ("spd19", "spd75", "spd128_L0", "dup16_L0", "one_row", "pivoting", "tie_L0")      # small enough for the literal form
