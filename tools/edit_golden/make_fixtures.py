"""Fixtures of tests/golden/edit: the reference's set_value / add_value / get_value / add_multiple_values /
add_sparse_matrix / scalar_multiply / zero on seeded inputs, CSR and ELLPACK.  Compiles edit_golden.f90 against the objects
and .mod files `bash oracle/build_ref.sh` leaves in oracle/_ref/obj, runs it once per case and stores the structure as the
reference holds it, every operation's inputs and the reference's value array after it.  Not part of the build or of any test:
the fixtures are data.

    python tools/edit_golden/make_fixtures.py
"""
import glob
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import edit_restated as R  # noqa: E402

OBJ = os.path.join(ROOT, "oracle", "_ref", "obj")
OUT = os.path.join(ROOT, "tests", "golden", "edit")
FC = os.environ.get("FC", "/opt/rocm/bin/amdflang")
SET, ADD, ADD_MULT, SET_MULT, ADD_MATRIX, SCALE, ZERO, GET = 1, 2, 3, 4, 5, 6, 7, 8


def build_driver(tmp):
    objs = [o for o in sorted(glob.glob(os.path.join(OBJ, "*.o")))
            if not os.path.basename(o).startswith(("ref_driver", "hip_"))]
    exe = os.path.join(tmp, "edit_golden")
    subprocess.check_call([FC, "-O2", "-J", tmp, "-I", OBJ, "-c", os.path.join(HERE, "edit_golden.f90"),
                           "-o", os.path.join(tmp, "edit_golden.o")])
    subprocess.check_call([FC, "-O2", "-o", exe, os.path.join(tmp, "edit_golden.o")] + objs +
                          ["-Wl,-z,execstack", "-Wl,--unresolved-symbols=ignore-all"])
    return exe


def random_edges(rs, nrow, ncol, max_d):
    ei, ej = [], []
    for r in range(nrow):
        d = rs.randint(1, max_d + 1)
        ei += [r + 1] * d
        ej += list(rs.permutation(ncol)[:d] + 1)
    return np.array(ei, np.int32), np.array(ej, np.int32)


def values(rs, m):
    """normal values with +0.0 / -0.0 and Inf among them (no NaN is made: +Inf only)"""
    z = rs.standard_normal(m)
    pick = rs.rand(m)
    z[pick < 0.06] = 0.0
    z[(pick >= 0.06) & (pick < 0.12)] = -0.0
    z[(pick >= 0.12) & (pick < 0.15)] = np.inf
    return z


def batch(rs, ei, ej, m, z=None):
    """m triples on pattern entries, half of them repeating one of the first few"""
    pick = rs.randint(len(ei), size=m)
    rep = rs.rand(m) < 0.5
    pick[rep] = pick[rs.randint(max(1, m // 8), size=int(rep.sum()))]
    return ei[pick], ej[pick], values(rs, m) if z is None else z


def cases():
    rs = np.random.RandomState(20261016)
    # P1 stiffness and mass assembly of fem.f90's triple stream, jittered coordinates
    x, ele = R.fem_grid(9, 7, seed=1, jitter=0.1)
    nn = x.shape[1]
    for kind in ("stiffness", "mass"):
        ti, tj, tz = R.fem_triples(x, ele, kind)
        yield "fem_" + kind, nn, nn, ti, tj, [(ADD, ti, tj, tz)]
    ei, ej = random_edges(rs, 40, 40, 7)
    yield "set_then_add", 40, 40, ei, ej, [(SET,) + batch(rs, ei, ej, 300), (ADD,) + batch(rs, ei, ej, 400),
                                           (ADD,) + batch(rs, ei, ej, 200, rs.standard_normal(200))]
    # add_multiple_values with an index repeated in `is` and in `js`: a full 6 x 6 block pattern inside a larger matrix
    blk = np.array([3, 9, 4, 17, 11, 20], np.int32)
    bi, bj = np.repeat(blk, 6), np.tile(blk, 6)
    e2i, e2j = random_edges(rs, 24, 24, 4)
    pi, pj = np.concatenate([e2i, bi]), np.concatenate([e2j, bj])
    is_ = np.array([3, 9, 3, 17, 9], np.int32)
    js = np.array([4, 11, 11, 20, 4, 3], np.int32)
    yield "add_multiple", 24, 24, pi, pj, [(ADD_MULT, is_, js, rs.standard_normal((5, 6))),
                                           (ADD_MULT, js, is_, rs.standard_normal((6, 5)))]
    # add_sparse_matrix: B's pattern inside A's
    ei, ej = random_edges(rs, 30, 30, 6)
    sub = np.sort(rs.choice(len(ei), size=len(ei) // 2, replace=False))
    sub = sub[rs.permutation(len(sub))]
    bv = values(rs, len(sub))
    yield "add_matrix", 30, 30, ei, ej, [(SET,) + batch(rs, ei, ej, 150), (ADD_MATRIX, 1.0 / 3.0, ei[sub], ej[sub], bv),
                                         (ADD_MATRIX, None, ei[sub], ej[sub], bv)]
    ei, ej = random_edges(rs, 25, 31, 5)
    gi = np.concatenate([ei[::3], rs.randint(1, 26, size=40).astype(np.int32)])
    gj = np.concatenate([ej[::3], rs.randint(1, 32, size=40).astype(np.int32)])
    yield "scale_zero_get", 25, 31, ei, ej, [(SET, ei, ej, rs.standard_normal(len(ei))), (GET, gi, gj), (SCALE, -1.7),
                                             (GET, gi, gj), (ZERO,), (GET, gi, gj)]
    # an ELLPACK row whose padding repeats the very column being added to (rows shorter than max_d, their last neighbour)
    ei = np.array([1, 1, 1, 1, 2, 2, 3, 4, 4, 4], np.int32)
    ej = np.array([2, 5, 1, 4, 3, 2, 3, 4, 1, 5], np.int32)
    ti = np.array([2, 3, 2, 4, 3, 2], np.int32)
    tj = np.array([2, 3, 2, 5, 3, 3], np.int32)
    yield "padding_column", 5, 5, ei, ej, [(ADD, ti, tj, rs.standard_normal(6)), (SET, ti[:3], tj[:3], rs.standard_normal(3)),
                                           (ADD, ti, tj, rs.standard_normal(6))]


def write_ops(f, fmt, ops):
    for op in ops:
        code = op[0]
        np.array([code], np.int32).tofile(f)
        if code in (SET, ADD, GET):
            np.array([len(op[1])], np.int32).tofile(f)
            np.asarray(op[1], np.int32).tofile(f)
            np.asarray(op[2], np.int32).tofile(f)
            if code != GET:
                np.asarray(op[3], np.float64).tofile(f)
        elif code in (ADD_MULT, SET_MULT):
            np.array([len(op[1]), len(op[2])], np.int32).tofile(f)
            np.asarray(op[1], np.int32).tofile(f)
            np.asarray(op[2], np.int32).tofile(f)
            np.asarray(op[3], np.float64).flatten("F").tofile(f)
        elif code == ADD_MATRIX:
            np.array([0 if op[1] is None else 1], np.int32).tofile(f)
            np.array([0.0 if op[1] is None else op[1]], np.float64).tofile(f)
            np.array([fmt, len(op[2])], np.int32).tofile(f)
            np.asarray(op[2], np.int32).tofile(f)
            np.asarray(op[3], np.int32).tofile(f)
            np.asarray(op[4], np.float64).tofile(f)
        elif code == SCALE:
            np.array([op[1]], np.float64).tofile(f)
    np.array([0], np.int32).tofile(f)


class Reader:
    def __init__(self, buf):
        self.buf, self.off = buf, 0

    def take(self, dtype, n):
        a = np.frombuffer(self.buf, dtype, n, self.off).copy()
        self.off += a.nbytes
        return a


def read_structure(r, fmt, nrow, d, tag):
    if fmt == 0:
        nnz = int(r.take(np.int32, 1)[0])
        d[tag + "ptr"], d[tag + "node"] = r.take(np.int32, nrow + 1), r.take(np.int32, nnz)
        return nnz
    md = int(r.take(np.int32, 1)[0])
    d[tag + "node"] = r.take(np.int32, md * nrow).reshape(nrow, md)          # (max_d, n) Fortran order = (n, max_d) C order
    d[tag + "degrees"] = r.take(np.int32, nrow)
    return md * nrow


def main():
    os.makedirs(OUT, exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_driver(tmp)
        for name, nrow, ncol, ei, ej, ops in cases():
            for fmt, fname in ((0, "csr"), (1, "ell")):
                fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
                with open(fin, "wb") as f:
                    np.array([fmt, nrow, ncol, len(ei)], np.int32).tofile(f)
                    np.asarray(ei, np.int32).tofile(f)
                    np.asarray(ej, np.int32).tofile(f)
                    write_ops(f, fmt, ops)
                subprocess.check_call([exe, fin, fout])
                r = Reader(open(fout, "rb").read())
                d = {"fmt": np.array(fmt, np.int32), "shape": np.array([nrow, ncol], np.int32), "nops": np.array(len(ops), np.int32)}
                slots = read_structure(r, fmt, nrow, d, "")
                for k, op in enumerate(ops):
                    t = f"op{k}_"
                    d[t + "code"] = np.array(op[0], np.int32)
                    if op[0] in (SET, ADD, GET):
                        d[t + "i"], d[t + "j"] = np.asarray(op[1], np.int32), np.asarray(op[2], np.int32)
                        if op[0] != GET:
                            d[t + "z"] = np.asarray(op[3], np.float64)
                    elif op[0] in (ADD_MULT, SET_MULT):
                        d[t + "is"], d[t + "js"], d[t + "B"] = np.asarray(op[1], np.int32), np.asarray(op[2], np.int32), np.asarray(op[3], np.float64)
                    elif op[0] == ADD_MATRIX:
                        d[t + "alpha"] = np.array([] if op[1] is None else [op[1]], np.float64)
                        nb = read_structure(r, fmt, nrow, d, t + "b_")
                        d[t + "b_val"] = r.take(np.float64, nb)
                    elif op[0] == SCALE:
                        d[t + "alpha"] = np.array([op[1]], np.float64)
                    if op[0] == GET:
                        d[t + "zout"] = r.take(np.float64, len(op[1]))
                    else:
                        d[t + "val"] = r.take(np.float64, slots)
                assert r.off == len(r.buf), (name, fname, r.off, len(r.buf))
                path = os.path.join(OUT, f"{name}_{fname}.npz")
                np.savez_compressed(path, **d)
                print(f"{name}_{fname}: {nrow} x {ncol}, {slots} slots, {len(ops)} operations, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
