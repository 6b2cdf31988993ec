"""Cases and the exact reference for the dot products fused into the SpMV kernels (tests/test_gpu_fused_dots.py on the GPU,
tests/test_fused_dots_cpu.py for the reference itself).  Host only: nothing here touches a GPU.

Every SpMV kernel family carries two optional epilogues -- partial sums of w.y and of y.y (SpmvDots, sgm_internal.hpp) -- that CG,
BiCGStab and Lanczos consume in the default dot order.  sgm_mat_matvec_dots makes the scalars themselves observable; this module
says what they must be:

  exact_dot(a, b)   the correctly rounded sum of a_i * b_i (error-free products, then math.fsum)
  `int` data        matrix values, x in {1, 2, 3}, w in +-{1, 2, 3}, y0 in {-3 .. 3}: every product, row sum and partial sum in
                    every order is an integer below 2^53, so the device scalar must == the reference whatever the summation tree;
                    y_i >= 1 on every non-empty row, so a dropped, doubled or mis-indexed row cannot hide
  `real` data       standard normal; |device - exact| <= gamma_n * sum|w_i y_i| (resp. gamma_n * sum y_i^2), gamma_n = n u / (1 - n u),
                    u = 2^-53, n = the part's rows: the a-priori bound for n rounded products added in any order

The structures are the smallest at which each family can still go wrong (see CASES); each case names the kernel it means to
reach (`key`, compared with kernel_key(H.kernel)) and the number of partial sums its product leaves (`count`, from the launch
geometry of sgm_spmv_select.hpp: a CSR row range never runs on fewer than 8 workgroups, so 8 is the smallest count of a CSR
family; ELLPACK kernels and the composite's separate dot kernel go down to 1).
"""
import functools
import math
from collections import namedtuple
from fractions import Fraction

import numpy as np

from sigma_amd import problems as P

U = 2.0 ** -53
TWO53 = 2.0 ** 53
TWO24 = 2.0 ** 24


def gamma(n):
    return n * U / (1.0 - n * U)


# ------------------------------------------------------------------------------------ the exact reference
def _split(a):
    """Veltkamp: a = hi + lo with 26-bit halves."""
    c = 134217729.0 * a                    # 2^27 + 1
    hi = c - (c - a)
    return hi, a - hi


def two_product(a, b):
    """Dekker: p = fl(a * b) and e with p + e == a * b exactly (no FMA needed)."""
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    return p, e


def exact_dot(a, b):
    """The correctly rounded value of sum a_i * b_i (finite operands)."""
    a = np.ascontiguousarray(a, np.float64)
    b = np.ascontiguousarray(b, np.float64)
    p, e = two_product(a, b)
    return math.fsum(np.concatenate([p, e]).tolist())


def fraction_dot(a, b):
    s = Fraction(0)
    for u, v in zip(a.tolist(), b.tolist()):
        s += Fraction(u) * Fraction(v)
    return s


def nonfinite_class(a, b):
    """What a sum of the products a_i * b_i is in ANY order once one of them is not finite: 'nan', '+inf' or '-inf'
    (None: all finite)."""
    with np.errstate(invalid="ignore", over="ignore"):
        p = np.asarray(a, np.float64) * np.asarray(b, np.float64)
    if np.isnan(p).any() or (np.isposinf(p).any() and np.isneginf(p).any()):
        return "nan"
    if np.isposinf(p).any():
        return "+inf"
    if np.isneginf(p).any():
        return "-inf"
    return None


# ------------------------------------------------------------------------------------ structures (patterns only)
def _csr(n, m, deg, cols):
    ptr = np.concatenate([[1], 1 + np.cumsum(deg)]).astype(np.int32)
    return {"fmt": "csr", "n": int(n), "m": int(m), "ptr": ptr, "node": (np.asarray(cols) + 1).astype(np.int32)}


def banded_short_rows(n, seed, wmax=8, noffs=15):
    """tests/test_gpu_parity.py's _banded_short_rows made square (columns clipped to n - 1, which keeps the offsets inside
    0 .. noffs - 1): mostly full rows of wmax entries, some shorter, some empty; duplicates inside a row allowed."""
    rs = np.random.RandomState(seed)
    deg = np.full(n, wmax)
    short = rs.rand(n) < 0.10
    deg[short] = rs.randint(0, wmax, size=int(short.sum()))
    deg[[0, n // 2, n - 1]] = [0, 1, wmax]
    rows = np.repeat(np.arange(n), deg)
    return _csr(n, n, deg, np.minimum(rows + rs.randint(0, noffs, size=rows.size), n - 1))


def grid5(nx, ny):
    ptr, node, _ = P.poisson2d_csr(nx, ny)
    return {"fmt": "csr", "n": nx * ny, "m": nx * ny, "ptr": ptr, "node": node}


def stencil3d(nx, ny, nz):
    """27-point stencil (nz = 1: the 2-D 9-point one), columns ascending."""
    n = nx * ny * nz
    idx = np.arange(n)
    i, j, k = idx % nx, (idx // nx) % ny, idx // (nx * ny)
    cols, oks = [], []
    for dk in (-1, 0, 1):
        for dj in (-1, 0, 1):
            for di in (-1, 0, 1):
                oks.append((i + di >= 0) & (i + di < nx) & (j + dj >= 0) & (j + dj < ny) & (k + dk >= 0) & (k + dk < nz))
                cols.append(idx + di + dj * nx + dk * nx * ny)
    C, M = np.stack(cols, 1), np.stack(oks, 1)
    return _csr(n, n, M.sum(1), C[M])


def short_random(n, w, seed):
    """Rows of <= w entries at arbitrary columns: no dictionary (forced off for the one-row matrix)."""
    rs = np.random.RandomState(seed)
    deg = np.where(rs.rand(n) < 0.9, w, rs.randint(0, w + 1, size=n))
    deg[-1] = w
    return _csr(n, n, deg, rs.randint(0, n, size=int(deg.sum())))


def many_offsets(n, seed):
    """Rows of 0 .. 11 entries within +-60 of the diagonal: more than 15 offsets, fewer than 256."""
    rs = np.random.RandomState(seed)
    deg = rs.randint(0, 12, size=n)
    rows = np.repeat(np.arange(n), deg)
    return _csr(n, n, deg, np.clip(rows + rs.randint(-60, 61, size=rows.size), 0, n - 1))


def long_banded(n, lo, hi, seed, band=0):
    """tests/test_gpu_parity.py's long-row matrices: lo .. hi arbitrary columns inside a band, symmetrised, sorted columns.
    (700 rows with that test's band of 300 are nearly all boundary: rows too uneven for SELL, sell_padding 1.56; +-130 gives 1.21)"""
    import scipy.sparse as sp
    rs = np.random.RandomState(seed)
    band = band or max(2 * hi, 300)
    deg = rs.randint(lo, hi + 1, size=n)
    deg[rs.randint(0, n, size=5)] = 0
    rows = np.repeat(np.arange(n), deg)
    cols = np.clip(rows + rs.randint(-band, band + 1, size=rows.size), 0, n - 1)
    B = sp.csr_matrix((np.ones(rows.size), (rows, cols)), shape=(n, n))
    S = (B + B.T + sp.identity(n)).tocsr()
    S.sum_duplicates()
    S.sort_indices()
    return {"fmt": "csr", "n": n, "m": n, "ptr": (S.indptr + 1).astype(np.int32), "node": (S.indices + 1).astype(np.int32)}


def sell_padding(st):
    """Stored slots over entries of the SELL-128-512 form (rows of every 512-row window sorted by length, chunks of 128 of their
    own even width): the library builds the form up to 1.30."""
    lens = np.diff(st["ptr"])
    slots = 0
    for w0 in range(0, st["n"], 512):
        srt = np.sort(lens[w0:w0 + 512])[::-1]
        for c in range(0, len(srt), 128):
            slots += (int(srt[c]) + 1) // 2 * 2 * 128
    return slots / float(lens.sum())


def ragged(n, seed):
    """Rows of 0 .. 5 entries, empty rows, and every fiftieth-or-so row 5000 entries long (beyond the line-staged kernel)."""
    rs = np.random.RandomState(seed)
    deg = rs.randint(0, 6, size=n)
    deg[rs.randint(0, n, size=n // 50)] = 5000
    deg[[0, 1, 2]] = [0, 0, 1]
    return _csr(n, n, deg, rs.randint(0, n, size=int(deg.sum())))


def scattered_csr(n, dmin, dmax, seed):
    """Rows of dmin .. dmax DISTINCT columns anywhere: what the column-blocked form is for."""
    rs = np.random.RandomState(seed)
    deg = rs.randint(dmin, dmax + 1, size=n)
    key = rs.rand(n, n) if n <= 512 else None
    if key is not None:
        order = np.argsort(key, axis=1)
        cols = np.concatenate([order[r, :deg[r]] for r in range(n)])
    else:
        cols = np.concatenate([rs.choice(n, d, replace=False) for d in deg])
    return _csr(n, n, deg, cols)


def _ell(n, ei, ej):
    return {"fmt": "ell", "n": int(n), "m": int(n), "ei": np.asarray(ei, np.int32), "ej": np.asarray(ej, np.int32)}


def random_ell(n, d, seed):
    """problems.random_regular_ell: the diagonal and d - 1 distinct random columns, rows of d // 2 .. d entries (padding)."""
    ei, ej, _ = P.random_regular_ell(n, d, seed, dmin=max(1, d // 2) if d > 1 else None)
    return _ell(n, ei, ej)


def banded_ell(n, max_d, seed, reach=12):
    """Rows of 1 .. max_d distinct columns within +-reach: 2 reach + 1 > 15 offsets, so the 1-byte-code kernel, not the slices."""
    rs = np.random.RandomState(seed)
    deg = np.where(rs.rand(n) < 0.8, max_d, rs.randint(1, max_d + 1, size=n))
    deg[rs.randint(0, n)] = max_d
    cols = np.arange(n)[:, None] + np.arange(-reach, reach + 1)[None, :]
    key = rs.rand(n, 2 * reach + 1)
    key[(cols < 0) | (cols >= n)] = 2.0                   # columns outside the matrix sort last and are never taken
    order = np.argsort(key, axis=1)
    take = (np.arange(2 * reach + 1)[None, :] < deg[:, None]) & (np.take_along_axis(key, order, 1) < 2.0)
    ej = np.take_along_axis(cols, order, 1)[take]         # row by row, in the order drawn
    ei = np.repeat(np.arange(n), take.sum(1))
    return _ell(n, ei + 1, ej + 1)


def structured_ell(n, offs=(-7, -2, -1, 0, 1, 2, 7)):
    """A seven-offset stencil in ELLPACK shape (boundary rows padded): the sliced route."""
    idx = np.arange(n)
    ei, ej = [], []
    for o in offs:
        ok = (idx + o >= 0) & (idx + o < n)
        ei.append(idx[ok] + 1)
        ej.append(idx[ok] + o + 1)
    ei, ej = np.concatenate(ei), np.concatenate(ej)
    order = np.argsort(ei, kind="stable")
    return _ell(n, ei[order], ej[order])


def composite(n, cut, deg_):
    """2 x 2 CSR leaves, n rows cut at `cut`; rows of deg_ entries per leaf (duplicates allowed), a few of them empty."""
    cuts = [0, cut, n]
    leaves = {}
    for it in range(2):
        for jt in range(2):
            nr, nc = cuts[it + 1] - cuts[it], cuts[jt + 1] - cuts[jt]
            rs = np.random.RandomState(40 + 2 * it + jt + n)
            deg = np.full(nr, deg_)
            deg[rs.randint(0, nr, 3)] = 0
            leaves[(it, jt)] = _csr(nr, nc, deg, rs.randint(0, nc, size=int(deg.sum())))
    return {"fmt": "composite", "n": n, "m": n, "cuts": cuts, "leaves": leaves}


# ------------------------------------------------------------------------------------ the cases
# name, family (a row of the issue's table), struct (a thunk), create (the defaults set around the handle's creation), handle (options
# set on the handle afterwards), key (kernel_key of H.kernel), wg_rows (rows per workgroup of the launch geometry: 512 for the
# sliced / SELL forms, 256 for the other CSR kernels and the plain ELLPACK ones, the tile height for the column-blocked form, 1024
# for the composite's dot kernel), min_grid (8: CSR row ranges), nparts / align (in-process partitions)
Case = namedtuple("Case", "name family struct create handle key wg_rows min_grid nparts align")


def _c(name, family, struct, key, wg_rows, create=None, handle=None, min_grid=8, nparts=0, align=0):
    return Case(name, family, struct, dict(create or {}), dict(handle or {}), key, wg_rows, min_grid, nparts, align)


FAMILIES = ("k_csr_sl", "k_csr_slb", "k_csr_sl32", "k_csr_do CW=1", "k_csr_do CW=4", "k_csr_sell xw", "k_csr_sell", "k_csr_rl",
            "k_csr_spmv", "k_ellcb ell", "k_ellcb csr", "k_ell_spmv", "k_ell_do<4>", "k_ell_do<8>", "k_ell_do<16>", "sliced ellpack",
            "partition", "composite", "lean parts")
# what kernel_key may return: the kernel families of the table (partitions and lean parts run kernels of these)
KERNEL_KEYS = tuple(f for f in FAMILIES if f not in ("partition", "lean parts"))

_P = functools.partial
_NO_SLICES = {"csr_sliced": 0}
_INT32_OWNER = {"csr_sliced": 0, "csr_offset_dict": 0}
_ROW_LINES = {"csr_sell": 0, "csr_row_owner": 0}
_ELLCB = lambda cols: {"ell_colblock": 2, "ell_colblock_cols": cols}       # noqa: E731

CASES = tuple(
    [_c(f"sl_banded_{n}_w{w}", "k_csr_sl", _P(banded_short_rows, n, 100 + n, w), "k_csr_sl", 512)
     for n, w in ((1, 3), (255, 3), (256, 5), (257, 7), (511, 8), (512, 5), (513, 8), (70001, 8), (1048573, 3))] +
    [_c("sl_grid5_301x233", "k_csr_sl", _P(grid5, 301, 233), "k_csr_sl", 512),
     # one slice (a 9-point grid of 506 rows), and 8 slices + a tail of 205 rows (27 points)
     _c("slb_9pt_22x23", "k_csr_slb", _P(stencil3d, 22, 23, 1), "k_csr_slb", 512),
     _c("slb_27pt_23x17x11", "k_csr_slb", _P(stencil3d, 23, 17, 11), "k_csr_slb", 512),
     _c("slb_9pt_70x51", "k_csr_slb", _P(stencil3d, 70, 51, 1), "k_csr_slb", 512),
     _c("sl32_1_w16", "k_csr_sl32", _P(short_random, 1, 16, 7), "k_csr_sl32", 512, create={"csr_offset_dict": 0}),
     _c("sl32_513_w16", "k_csr_sl32", _P(short_random, 513, 16, 8), "k_csr_sl32", 512),
     _c("sl32_40001_w12", "k_csr_sl32", _P(short_random, 40001, 12, 9), "k_csr_sl32", 512)] +
    [_c(f"do1_{n}", "k_csr_do CW=1", _P(many_offsets, n, 20 + n), "k_csr_do CW=1", 256, create=_NO_SLICES) for n in (65, 2049, 3001, 40001)] +
    [_c(f"do4_{n}", "k_csr_do CW=4", _P(many_offsets, n, 20 + n), "k_csr_do CW=4", 256, create=_INT32_OWNER) for n in (65, 2049, 3001, 40001)] +
    [_c("sell_xw_700", "k_csr_sell xw", _P(long_banded, 700, 70, 120, 1, 130), "k_csr_sell xw", 512),
     _c("sell_xw_5000", "k_csr_sell xw", _P(long_banded, 5000, 66, 90, 2), "k_csr_sell xw", 512),
     _c("sell_700", "k_csr_sell", _P(long_banded, 700, 70, 120, 1, 130), "k_csr_sell", 512, handle={"csr_xwindow": 0}),
     _c("sell_5000", "k_csr_sell", _P(long_banded, 5000, 66, 90, 2), "k_csr_sell", 512, handle={"csr_xwindow": 0}),
     _c("rl_700", "k_csr_rl", _P(long_banded, 700, 70, 120, 1, 130), "k_csr_rl", 256, create=_ROW_LINES),
     _c("rl_5000", "k_csr_rl", _P(long_banded, 5000, 66, 90, 2), "k_csr_rl", 256, create=_ROW_LINES),
     _c("spmv_ragged_3001", "k_csr_spmv", _P(ragged, 3001, 4), "k_csr_spmv", 256),
     _c("spmv_ragged_200", "k_csr_spmv", _P(ragged, 200, 5), "k_csr_spmv", 256),
     _c("ellcb_ell_130_d6", "k_ellcb ell", _P(random_ell, 130, 6, 31), "k_ellcb ell", 256, create=_ELLCB(64), min_grid=1),
     _c("ellcb_ell_3001_d12", "k_ellcb ell", _P(random_ell, 3001, 12, 32), "k_ellcb ell", 256, create=_ELLCB(256), min_grid=1),
     _c("ellcb_ell_5000_d32", "k_ellcb ell", _P(random_ell, 5000, 32, 33), "k_ellcb ell", 512, create=_ELLCB(512), min_grid=1),
     _c("ellcb_csr_200", "k_ellcb csr", _P(scattered_csr, 200, 1, 12, 34), "k_ellcb csr", 256,
        create=dict(_ELLCB(64), csr_offset_dict=0), min_grid=1),
     _c("ellcb_csr_3001", "k_ellcb csr", _P(scattered_csr, 3001, 1, 12, 35), "k_ellcb csr", 256, create=_ELLCB(256), min_grid=1),
     _c("ellcb_csr_5000", "k_ellcb csr", _P(scattered_csr, 5000, 8, 32, 36), "k_ellcb csr", 512, create=_ELLCB(512), min_grid=1)] +
    [_c(f"ell_spmv_{n}_d{d}", "k_ell_spmv", _P(random_ell, n, d, 50 + d), "k_ell_spmv", 256, create={"ell_offset_dict": 0}, min_grid=1)
     for n, d in ((200, 5), (257, 1), (4097, 5), (257, 9), (4097, 20), (40001, 9))] +
    [_c(f"ell_do{mdp}_{n}_d{d}", f"k_ell_do<{mdp}>", _P(banded_ell, n, d, 60 + d + n), f"k_ell_do<{mdp}>", 256, min_grid=1)
     for mdp, d, big in ((4, 3, 150001), (8, 8, 40001), (16, 16, 40001)) for n in (200, big)] +
    [_c(f"ell_sliced_{n}", "sliced ellpack", _P(structured_ell, n), "sliced ellpack", 512, min_grid=1) for n in (300, 513, 40001)] +
    [_c(f"part{k}_grid5_450x450", "partition", _P(grid5, 450, 450), "k_csr_sl", 512, nparts=k, align=512) for k in (3, 5)] +
    [_c(f"part{k}_long_5000", "partition", _P(long_banded, 5000, 66, 90, 2), "k_csr_sell", 512, nparts=k, align=2) for k in (3, 5)] +
    # (480 rows of 2 x 30 entries: one workgroup of the separate dot kernel, and sum y^2 past 2^24; 2500 rows: three workgroups)
    [_c("composite_480", "composite", _P(composite, 480, 201, 30), "composite", 1024, min_grid=1),
     _c("composite_2500", "composite", _P(composite, 2500, 1201, 8), "composite", 1024, min_grid=1),
     # csr_lean (on by default: the cases above already run on lean parts) named, and switched off
     _c("lean_on_sl_5121", "lean parts", _P(banded_short_rows, 5121, 77, 8), "k_csr_sl", 512, create={"csr_lean": 1}),
     _c("lean_off_sl_5121", "lean parts", _P(banded_short_rows, 5121, 77, 8), "k_csr_sl", 512, create={"csr_lean": 0}),
     _c("lean_on_sell_700", "lean parts", _P(long_banded, 700, 70, 120, 1, 130), "k_csr_sell xw", 512, create={"csr_lean": 1}),
     _c("lean_off_sell_700", "lean parts", _P(long_banded, 700, 70, 120, 1, 130), "k_csr_sell xw", 512, create={"csr_lean": 0})])
CASE_BY_NAME = {c.name: c for c in CASES}
DATASETS = ("int", "real")
# every option a case may set, with the default it is put back to
OPTION_DEFAULTS = {"csr_sliced": 1, "csr_offset_dict": 1, "csr_row_owner": 1, "csr_row_lines": 1, "csr_sell": 1, "csr_xwindow": 1,
                   "csr_lean": 1, "ell_offset_dict": 1, "ell_colblock": 1, "ell_colblock_cols": 16384}


def kernel_key(kernel, fmt):
    """H.kernel -> the family of KERNEL_KEYS it belongs to."""
    if kernel == "composite":
        return "composite"
    if kernel.startswith("k_ellcb"):
        return "k_ellcb csr" if kernel.endswith(",csr>") else "k_ellcb ell"
    if fmt == "ell" and kernel.startswith("k_csr_sl<"):
        return "sliced ellpack"
    if kernel.startswith("k_ell_do<MDP="):
        return "k_ell_do<%s>" % kernel[len("k_ell_do<MDP="):-1]
    if kernel.startswith("k_csr_sell"):
        return "k_csr_sell xw" if "xw=" in kernel else "k_csr_sell"
    if kernel.startswith("k_csr_do"):
        return "k_csr_do CW=1" if "CW=1" in kernel else "k_csr_do CW=4"
    return kernel.split("<")[0]


# ------------------------------------------------------------------------------------ partitions: rows, ranges, counts
def part_starts(n, nparts, align):
    s = [(n * k // nparts) // align * align for k in range(nparts)] + [n]
    return np.asarray(s, np.int64)


def part_ranges(ptr, node, r0, r1, block=512):
    """set_interior_range + spmv_ranges restated: the interior (the first longest run of `block`-row blocks of the part whose rows
    reference owned columns only) first, then the rows before it and the rows after it; one range when there is no interior."""
    n = r1 - r0
    lo, hi = ptr[r0:r1] - 1, ptr[r0 + 1:r1 + 1] - 1
    c = node[lo[0]:hi[-1]].astype(np.int64) - 1
    out = ((c < r0) | (c >= r1)).astype(np.int64)
    cs = np.concatenate([[0], np.cumsum(out)])
    halo_row = (cs[hi - lo[0]] - cs[lo - lo[0]]) > 0
    if not halo_row.any():
        return [(0, n)]
    nb = (n + block - 1) // block
    best_lo = best_len = run_lo = run_len = 0
    for b in range(nb):
        if halo_row[b * block:min((b + 1) * block, n)].any():
            run_len, run_lo = 0, b + 1
            continue
        run_len += 1
        if run_len > best_len:
            best_len, best_lo = run_len, run_lo
    int_lo, int_hi = best_lo * block, min((best_lo + best_len) * block, n)
    if int_hi <= int_lo:
        return [(0, n)]
    return [r for r in ((int_lo, int_hi), (0, int_lo), (int_hi, n)) if r[1] > r[0]]


def range_grid(rows, wg_rows, min_grid):
    """Workgroups (= partial sums per dot) of one launch over `rows` rows: grid_for_rows for CSR ranges (a multiple of 8; its
    caps lie far above these sizes), one workgroup per wg_rows rows for the ELLPACK kernels and the composite's dot kernel."""
    g = (max(rows, 1) + wg_rows - 1) // wg_rows
    return max(8, (g + 7) // 8 * 8) if min_grid == 8 else max(1, g)


# ------------------------------------------------------------------------------------ data and reference, once per (case, data set)
def _values(rs, data, size):
    return rs.randint(1, 4, size=size).astype(np.float64) if data == "int" else rs.standard_normal(size)


def _oracle_matrix(orc, st, rs, data):
    if st["fmt"] == "csr":
        return orc.CsrMatrix(st["n"], st["m"], st["ptr"], st["node"], _values(rs, data, st["node"].size))
    return orc.EllMatrix.from_edges(st["n"], st["m"], st["ei"], st["ej"], _values(rs, data, st["ei"].size))


class Ref:
    """Everything a test needs of one (case, data set): the oracle's matrix (or the composite's leaves), x, w, y0, the oracle's
    y = A x and y0 + A x, the parts' rows and ranges, and per part the exact scalars and the bars."""


@functools.lru_cache(maxsize=None)
def structure(name):
    return CASE_BY_NAME[name].struct()


@functools.lru_cache(maxsize=None)
def reference(name, data):
    import oracle as orc
    case = CASE_BY_NAME[name]
    st = structure(name)
    rs = np.random.RandomState(sum(map(ord, name)) * 2 + (data == "int"))
    n, m = st["n"], st["m"]
    R = Ref()
    R.case, R.data, R.n, R.m, R.fmt = case, data, n, m, st["fmt"]
    if st["fmt"] == "composite":
        R.leaves = {k: _oracle_matrix(orc, s, rs, data) for k, s in sorted(st["leaves"].items())}
        R.cuts = st["cuts"]
        R.A = None
    else:
        R.A = _oracle_matrix(orc, st, rs, data)
    if data == "int":
        R.x = rs.randint(1, 4, size=m).astype(np.float64)
        R.w = (rs.randint(1, 4, size=n) * rs.choice([-1, 1], size=n)).astype(np.float64)
        R.y0 = rs.randint(-3, 4, size=n).astype(np.float64)
    else:
        R.x, R.w, R.y0 = rs.standard_normal(m), rs.standard_normal(n), rs.standard_normal(n)
    R.y = (oracle_matvec(R, R.x, None), oracle_matvec(R, R.x, R.y0))
    if case.nparts:
        starts = part_starts(n, case.nparts, case.align)
        R.starts = starts
        R.parts = [(int(starts[k]), int(starts[k + 1])) for k in range(case.nparts)]
        R.ranges = [part_ranges(st["ptr"], st["node"], r0, r1) for r0, r1 in R.parts]
    else:
        R.starts = None
        R.parts = [(0, n)]
        R.ranges = [[(0, n)]]
    R.count = [sum(range_grid(b - a, case.wg_rows, case.min_grid) for a, b in rg) for rg in R.ranges]
    R.nonempty = nonempty_rows(st)
    # per add in (0, 1) and part: exact w.y, exact y.y, sum |w y|, sum y^2
    R.wy, R.yy, R.abs_wy, R.abs_yy = [], [], [], []
    for add in (0, 1):
        y = R.y[add]
        R.wy.append([exact_dot(R.w[a:b], y[a:b]) for a, b in R.parts])
        R.yy.append([exact_dot(y[a:b], y[a:b]) for a, b in R.parts])
        R.abs_wy.append([float(np.abs(R.w[a:b] * y[a:b]).sum()) for a, b in R.parts])
        R.abs_yy.append([float((y[a:b] * y[a:b]).sum()) for a, b in R.parts])
    if data == "int":
        # the conditions that make `==` the right comparison, asserted where the data are made
        for add in (0, 1):
            assert max(R.abs_wy[add]) < TWO53 and max(R.abs_yy[add]) < TWO53, name
            assert all(float(v).is_integer() for v in R.wy[add] + R.yy[add]), name
        assert (R.y[0][R.nonempty] >= 1.0).all(), name
    return R


def nonempty_rows(st):
    if st["fmt"] == "csr":
        return np.diff(st["ptr"]) > 0
    if st["fmt"] == "ell":
        return np.bincount(st["ei"] - 1, minlength=st["n"]) > 0
    out = np.zeros(st["n"], bool)
    for (it, _jt), s in st["leaves"].items():
        out[st["cuts"][it]:st["cuts"][it + 1]] |= np.diff(s["ptr"]) > 0
    return out


def oracle_matvec(R, x, y0):
    """The oracle's y = A x (y0 None) or y0 + A x; a composite as composite_matvec_add's block loop over the oracle's leaves."""
    x = np.ascontiguousarray(x, np.float64)
    if R.A is not None:
        return R.A.matvec(x) if y0 is None else R.A.matvec_add(x, y0.copy())
    y = np.zeros(R.n) if y0 is None else y0.copy()
    for (it, jt), L in R.leaves.items():
        L.matvec_add(x[R.cuts[jt]:R.cuts[jt + 1]].copy(), y[R.cuts[it]:R.cuts[it + 1]])
    return y
