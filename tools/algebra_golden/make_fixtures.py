"""Fixtures of tests/golden/algebra: the reference's sparse_matrix_sum / sparse_matrix_product / PtAP / RARt on seeded
inputs.  Compiles algebra_golden.f90 against the objects and .mod files `bash oracle/build_ref.sh` leaves in
oracle/_ref/obj, runs it once per case and stores the operands as the reference holds them and its result (1-based CSR
arrays).  Not part of the build or of any test: the fixtures are data.

    python tools/algebra_golden/make_fixtures.py
"""
import glob
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from sigma_amd import problems as PB  # noqa: E402

OBJ = os.path.join(ROOT, "oracle", "_ref", "obj")
OUT = os.path.join(ROOT, "tests", "golden", "algebra")
FC = os.environ.get("FC", "/opt/rocm/bin/amdflang")
OPS = {"sum": 0, "product": 1, "ptap": 2, "rart": 3}


def build_driver(tmp):
    objs = [o for o in sorted(glob.glob(os.path.join(OBJ, "*.o")))
            if not os.path.basename(o).startswith(("ref_driver", "hip_"))]
    exe = os.path.join(tmp, "algebra_golden")
    subprocess.check_call([FC, "-O2", "-J", tmp, "-I", OBJ, "-c", os.path.join(HERE, "algebra_golden.f90"),
                           "-o", os.path.join(tmp, "algebra_golden.o")])
    subprocess.check_call([FC, "-O2", "-o", exe, os.path.join(tmp, "algebra_golden.o")] + objs +
                          ["-Wl,-z,execstack", "-Wl,--unresolved-symbols=ignore-all"])
    return exe


def edges_of(nrow, ncol, ptr, node, val):
    """insertion-order edge list of 1-based CSR arrays (rows ascending, stored order inside a row)"""
    ptr = np.asarray(ptr, np.int64)
    ei = np.repeat(np.arange(1, nrow + 1, dtype=np.int32), np.diff(ptr))
    return (nrow, ncol, ei, np.asarray(node, np.int32), np.asarray(val, np.float64))


def random_matrix(rs, nrow, ncol, density, empty_rows=(), signed_zeros=False):
    ei, ej = [], []
    for i in range(nrow):
        if i in empty_rows:
            continue
        d = rs.binomial(ncol, density)
        cols = rs.permutation(ncol)[:d]         # unshuffled order = insertion order, not sorted
        ei += [i + 1] * d
        ej += list(cols + 1)
    ev = rs.standard_normal(len(ei))
    if signed_zeros and len(ev):
        k = rs.choice(len(ev), size=max(1, len(ev) // 5), replace=False)
        ev[k] = np.where(rs.rand(len(k)) < 0.5, -0.0, 0.0)
    return (nrow, ncol, np.array(ei, np.int32), np.array(ej, np.int32), ev)


def laplacian_graph(rs, n, p):
    """a random graph Laplacian (the shape of the reference's test/matrix_test_ptap.f90)"""
    up = np.triu(rs.rand(n, n) < p, 1)
    adj = up | up.T
    ei, ej, ev = [], [], []
    for i in range(n):
        nb = np.nonzero(adj[i])[0]
        ei += [i + 1] * (len(nb) + 1)
        ej += [i + 1] + list(nb + 1)
        ev += [float(len(nb))] + [-1.0] * len(nb)
    return (n, n, np.array(ei, np.int32), np.array(ej, np.int32), np.array(ev))


def cases():
    rs = np.random.RandomState(20261016)
    p = PB.poisson2d_csr(12, 10)
    A = edges_of(120, 120, *p)
    yield "poisson_times_itself", "product", A, A
    S = random_matrix(rs, 60, 60, 0.08)
    St = (60, 60, S[3], S[2], S[4])                 # its transpose as an edge list (same entries)
    order = np.lexsort((np.arange(len(St[2])), St[2]))
    St = (60, 60, St[2][order], St[3][order], St[4][order])
    yield "skew_plus_transpose", "sum", S, St
    B = random_matrix(rs, 40, 30, 0.1, empty_rows=(0, 7, 19))
    Cm = random_matrix(rs, 30, 50, 0.1, empty_rows=(3, 4, 5))
    yield "rectangular_product", "product", B, Cm
    # a row of B whose entries all hit empty rows of C: an empty result row
    Bz = (5, 30, np.array([1, 1, 2, 3, 5], np.int32), np.array([4, 5, 1, 2, 6], np.int32), np.array([1.0, 2.0, 3.0, 4.0, 5.0]))
    Cz = (30, 8, np.array([1, 2, 6], np.int32), np.array([3, 1, 8], np.int32), np.array([1.5, -2.0, 0.5]))
    yield "empty_result_row", "product", Bz, Cz
    nx, ny = 9, 7
    pa = PB.poisson2d_csr(nx, ny)
    pp = PB.interp2d_csr(nx, ny)
    yield "ptap_interp_poisson", "ptap", edges_of(nx * ny, nx * ny, *pa), edges_of(nx * ny, pp[3], *pp[:3])
    L = laplacian_graph(rs, 256, 0.02)
    P = random_matrix(rs, 256, 128, 0.03)
    yield "ptap_laplacian_256", "ptap", L, P
    Pt = (128, 256, P[3], P[2], P[4])
    order = np.lexsort((np.arange(len(Pt[2])), Pt[2]))
    Pt = (128, 256, Pt[2][order], Pt[3][order], Pt[4][order])
    yield "rart_laplacian_256", "rart", L, Pt
    Z1 = random_matrix(rs, 30, 30, 0.15, signed_zeros=True)
    Z2 = random_matrix(rs, 30, 30, 0.15, signed_zeros=True)
    yield "signed_zeros_sum", "sum", Z1, Z2
    yield "signed_zeros_product", "product", Z1, Z2
    Rz = random_matrix(rs, 12, 30, 0.2, signed_zeros=True)
    yield "signed_zeros_rart", "rart", Z1, Rz


def write_matrix(f, m):
    nrow, ncol, ei, ej, ev = m
    np.array([nrow, ncol, len(ei)], np.int32).tofile(f)
    if len(ei):
        np.asarray(ei, np.int32).tofile(f)
        np.asarray(ej, np.int32).tofile(f)
        np.asarray(ev, np.float64).tofile(f)


def read_matrix(buf, off):
    nrow, ncol, nnz = np.frombuffer(buf, np.int32, 3, off)
    off += 12
    ri = np.frombuffer(buf, np.int32, nnz, off); off += 4 * nnz
    ci = np.frombuffer(buf, np.int32, nnz, off); off += 4 * nnz
    rv = np.frombuffer(buf, np.float64, nnz, off); off += 8 * nnz
    assert np.all(np.diff(ri) >= 0)
    ptr = np.ones(nrow + 1, np.int32)
    np.cumsum(np.bincount(ri - 1, minlength=nrow), out=ptr[1:])
    ptr[1:] += 1
    return int(nrow), int(ncol), ptr, ci.astype(np.int32), rv.copy(), off


def main():
    os.makedirs(OUT, exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_driver(tmp)
        for name, op, X, Y in cases():
            fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
            with open(fin, "wb") as f:
                np.array([OPS[op]], np.int32).tofile(f)
                write_matrix(f, X)
                write_matrix(f, Y)
            subprocess.check_call([exe, fin, fout])
            buf = open(fout, "rb").read()
            d = {"op": np.array(OPS[op], np.int32)}
            off = 0
            for tag in ("x", "y", "z"):
                nrow, ncol, ptr, node, val, off = read_matrix(buf, off)
                d[tag + "_shape"] = np.array([nrow, ncol], np.int32)
                d[tag + "_ptr"], d[tag + "_node"], d[tag + "_val"] = ptr, node, val
            np.savez_compressed(os.path.join(OUT, name + ".npz"), **d)
            print(f"{name}: {op}, result {d['z_shape'][0]} x {d['z_shape'][1]}, nnz {len(d['z_val'])}")


if __name__ == "__main__":
    main()
