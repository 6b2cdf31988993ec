"""Sparse matrix algebra on the device at C2 size: build (symbolic + numeric) and refill times of A*A, A+A, P^T A P
(P the 2:1 linear interpolation) and R A R^T (R = P^T) on a 5-point Poisson grid, with the compulsory bytes of each
counted here and the fraction of 8 TB/s they reach.  One JSON line per case.

    python tools/algebra_bench.py [--nx 3162] [--warmup 1] [--reps 5] [--out FILE]

The library calls end in a stream synchronisation, so host wall clock around a call is its device time plus launch
overhead.  Compulsory bytes: build = operands read once (ptr, node, val) + output written once; refill = operand values
and the index arrays the numeric walk reads + the plan (term offsets, term slots, row pointers) + output values written
once."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sigma_amd as sg  # noqa: E402
from sigma_amd import problems as PB  # noqa: E402

PEAK = 8.0e12


def csr_bytes(n, nnz):
    return 4 * (n + 1) + 12 * nnz


def timed(f, reps, destroy=False):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = f()
        ts.append(time.perf_counter() - t0)
        if destroy:
            r.destroy()
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=3162)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", default="product,sum,ptap,rart")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sg.init(0)
    nx = a.nx
    n = nx * nx
    ptr, node, val = PB.poisson2d_csr(nx, nx)
    A = sg.csr_matrix(n, n, ptr, node, val)
    pp, pn, pv, nc = PB.interp2d_csr(nx, nx)
    P = sg.csr_matrix(n, nc, pp, pn, pv)
    R = sg.csr_matrix(nc, n, *_transpose(n, nc, pp, pn, pv))
    nnzA, nnzP = len(val), len(pv)
    ops = {"product": (sg.sparse_matrix_product, A, A), "sum": (sg.sparse_matrix_sum, A, A), "ptap": (sg.PtAP, A, P),
           "rart": (sg.RARt, A, R)}
    lines = []
    for case in a.cases.split(","):
        f, X, Y = ops[case]
        for _ in range(a.warmup):
            f(X, Y).destroy()
        t_build = timed(lambda: f(X, Y), a.reps, destroy=True)
        M = f(X, Y)
        for _ in range(a.warmup):
            M.refill(X, Y)
        t_refill = timed(lambda: M.refill(X, Y), a.reps)
        nout, nnz = M.nrow, M.nnz
        short, long_ = M.algebra_rows()
        # operands: the distinct handles read once
        if case in ("product", "sum"):
            operands = csr_bytes(n, nnzA)
            nterms = 25 * n if case == "product" else 2 * nnzA
            walk_idx = 4 * (n + 1) + 4 * nnzA + (4 * nnzA if case == "product" else 0)
            vals = 8 * nnzA
        else:
            operands = csr_bytes(n, nnzA) + csr_bytes(X.nrow if case == "ptap" else nc, nnzP)
            nterms = None
            walk_idx = 4 * (n + 1) + 4 * nnzA + 2 * (4 * (n + 1) + 4 * nnzP) + 8 * nnzP  # A, P and P^T's rows, tperm
            vals = 8 * nnzA + 8 * nnzP
        if nterms is None:
            pdeg = np.diff(pp)
            adeg_rows = np.repeat(np.arange(n), np.diff(ptr))
            nterms = int((pdeg[adeg_rows] * pdeg[node - 1]).sum())
        plan = 8 * (nout + 1) + 4 * nterms + 4 * (nout + 1)
        build_bytes = operands + csr_bytes(nout, nnz)
        refill_bytes = vals + walk_idx + plan + 8 * nnz
        rec = {"case": case, "nx": nx, "rows": nout, "nnz_out": nnz, "terms": nterms, "rows_lds": short, "rows_long": long_,
               "build_s": t_build, "refill_s": t_refill, "build_over_refill": t_build / t_refill,
               "build_bytes": build_bytes, "refill_bytes": refill_bytes,
               "build_frac_8TBs": build_bytes / t_build / PEAK, "refill_frac_8TBs": refill_bytes / t_refill / PEAK}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        M.destroy()
    if a.out:
        with open(a.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


def _transpose(n, nc, pp, pn, pv):
    """R = P^T as 1-based CSR arrays (rows of R = columns of P, entries by P's row ascending)"""
    rows = np.repeat(np.arange(n), np.diff(pp))
    cols = pn - 1
    order = np.argsort(cols, kind="stable")
    rptr = np.ones(nc + 1, np.int64)
    rptr[1:] += np.cumsum(np.bincount(cols, minlength=nc))
    return rptr.astype(np.int32), (rows[order] + 1).astype(np.int32), np.ascontiguousarray(pv[order])


if __name__ == "__main__":
    main()
