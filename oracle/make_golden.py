#!/usr/bin/env python3
"""Generate tests/golden/*.npz by running the REAL reference (oracle/_ref/sigma_ref_driver,
built by oracle/build_ref.sh from /root/reference with amdflang).  TEST INFRASTRUCTURE.

Run in the build container only (the reference does not exist on the GPU box):

    bash oracle/build_ref.sh && python oracle/make_golden.py

A fixture is data: the inputs (edge list in insertion order, x, b, solver settings) and
the arrays the reference produced (index arrays, values, y = A x, preconditioner
factors, solver solutions and iteration counts).  No reference source is stored.
"""
from __future__ import annotations

import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

from sigma_amd import problems as P  # noqa: E402

DRIVER = os.path.join(HERE, "_ref", "sigma_ref_driver")
GOLDEN = os.path.join(ROOT, "tests", "golden")

CG, BICGSTAB = 1, 2
NOPC, JACOBI, LDU = 0, 1, 2
CSR, ELL = 1, 2


def run_reference(n, m, fmt, edges, x, b, solves, mode=None):
    ei, ej, ev = edges
    with tempfile.TemporaryDirectory() as td:
        inp = os.path.join(td, "in.bin")
        with open(inp, "wb") as f:
            f.write(struct.pack("<5i", n, m, len(ei), fmt, len(solves)))
            f.write(np.asarray(ei, "<i4").tobytes())
            f.write(np.asarray(ej, "<i4").tobytes())
            f.write(np.asarray(ev, "<f8").tobytes())
            f.write(np.asarray(x, "<f8").tobytes())
            f.write(np.asarray(b, "<f8").tobytes())
            for (s, pc, tol) in solves:
                f.write(struct.pack("<iid", s, pc, tol))
        out = subprocess.run([DRIVER, inp, os.path.join(td, "o")] + ([mode] if mode else []), check=True,
                             capture_output=True, text=True, timeout=600)
        sys.stdout.write(out.stdout)
        res = {}
        for fn in sorted(os.listdir(td)):
            if not fn.startswith("o."):
                continue
            if fn == "o.matrix.txt":        # A%to_file output, kept byte for byte
                res["ref_matrix_txt"] = np.frombuffer(open(os.path.join(td, fn), "rb").read(), dtype=np.uint8)
                continue
            _, name, ext = fn.split(".")
            res["ref_" + name] = np.fromfile(os.path.join(td, fn),
                                             dtype="<i4" if ext == "i4" else "<f8")
    return res


ONLY = sys.argv[1] if len(sys.argv) > 1 else None      # name prefix filter, e.g. `make_golden.py perm_`


def case(name, n, m, fmt, edges, x, b, solves, extra=None, mode=None):
    if ONLY and not name.startswith(ONLY):
        return
    print(f"== {name}: n={n} ne={len(edges[0])} fmt={'csr' if fmt == CSR else 'ell'}")
    res = run_reference(n, m, fmt, edges, x, b, solves, mode)
    res.update(n=np.int32(n), m=np.int32(m), fmt=np.int32(fmt),
               ei=np.asarray(edges[0], np.int32), ej=np.asarray(edges[1], np.int32),
               ev=np.asarray(edges[2], np.float64), x=np.asarray(x, np.float64),
               b=np.asarray(b, np.float64),
               solves=np.array([(s, pc, tol) for s, pc, tol in solves], np.float64))
    if extra:
        res.update(extra)
    np.savez_compressed(os.path.join(GOLDEN, name + ".npz"), **res)


def main():
    os.makedirs(GOLDEN, exist_ok=True)
    if not os.path.exists(DRIVER):
        sys.exit("oracle/_ref/sigma_ref_driver missing: run oracle/build_ref.sh first")

    # -- the reference's own deterministic tests --------------------------------
    # test/solver_test_diffusion_1d.f90: ELLPACK n=127, CG tol 1e-16 (64 its, error 0)
    for fmt, tag in ((ELL, "ell"), (CSR, "csr")):
        edges, f, v = P.diffusion_1d(127)
        case(f"diffusion1d_{tag}_127", 127, 127, fmt, edges, P.test_vector(127), f,
             [(CG, NOPC, 1e-16), (CG, JACOBI, 1e-16)], extra=dict(analytic=v))
    # test/solver_test_advection_diffusion_1d.f90: ELLPACK n=1024, BiCGStab tol 1e-12
    for fmt, tag in ((ELL, "ell"), (CSR, "csr")):
        edges, f, v = P.advection_diffusion_1d(1024)
        case(f"advdiff1d_{tag}_1024", 1024, 1024, fmt, edges, P.test_vector(1024), f,
             [(BICGSTAB, NOPC, 1e-12), (BICGSTAB, JACOBI, 1e-12)], extra=dict(analytic=v))

    # -- config C1 at n=1e4 is too slow to converge at 1e-16 in a fixture; a 2000-row CSR
    #    version pins CG on a longer recurrence ---------------------------------
    edges, f, v = P.diffusion_1d(2000)
    case("diffusion1d_csr_2000", 2000, 2000, CSR, edges, P.test_vector(2000), f,
         [(CG, NOPC, 1e-14)], extra=dict(analytic=v))

    # -- BASELINE config C1 at its stated size: tridiag(-1,2,-1), n = 10,000, f = 2 dx^2, CG from 0 to an absolute
    #    1e-16.  The reference needs 9388 iterations (its sequential dot_product loses the recurrence's
    #    orthogonality later than n/2 = 5000, where exact arithmetic -- and a tree-order dot -- stops).
    edges, f, v = P.diffusion_1d(10000)
    case("diffusion1d_csr_10000", 10000, 10000, CSR, edges, P.test_vector(10000), f,
         [(CG, NOPC, 1e-16)], extra=dict(analytic=v))

    # -- C2 mini: 5-point Poisson 32x24 (non-square on purpose) ------------------
    nx, ny = 32, 24
    n = nx * ny
    edges = P.poisson2d_edges(nx, ny)
    b = np.full(n, 1.0 / n)
    case("poisson2d_32x24", n, n, CSR, edges, P.test_vector(n), b,
         [(CG, NOPC, 1e-12), (CG, JACOBI, 1e-12), (CG, LDU, 1e-12),
          (BICGSTAB, NOPC, 1e-12), (BICGSTAB, JACOBI, 1e-12), (BICGSTAB, LDU, 1e-12)])
    # (CG / BiCGStab + LDU on the ELLPACK operand: sparse_ldu_setup takes any sparse_matrix_interface, ldu_solvers.f90:95-130,
    #  and reads it through the get_edges cursor -- the rows' real entries, never the padding)
    case("poisson2d_ell_32x24", n, n, ELL, edges, P.test_vector(n), b,
         [(CG, NOPC, 1e-12), (CG, LDU, 1e-12), (BICGSTAB, LDU, 1e-12)])

    # -- C5 mini: 7-point Laplacian 8x7x6 ---------------------------------------
    nx, ny, nz = 8, 7, 6
    n = nx * ny * nz
    edges = P.laplace3d_edges(nx, ny, nz)
    b = np.full(n, 1.0 / n)
    case("laplace3d_8x7x6", n, n, CSR, edges, P.test_vector(n), b,
         [(CG, NOPC, 1e-13), (CG, LDU, 1e-13)])

    # -- C4 mini: random 32-regular digraph in ELLPACK, and a padded variant -----
    n = 512
    for dmin, tag in ((None, "full"), (24, "padded")):
        edges = P.random_regular_ell(n, 32, 12345, dmin=dmin)
        case(f"random_ell32_{tag}_512", n, n, ELL, edges, P.test_vector(n),
             np.ones(n), [])
        case(f"random_csr32_{tag}_512", n, n, CSR, edges, P.test_vector(n),
             np.ones(n), [])

    # -- the matrix family of solver_test_jacobi / solver_test_incomplete_cholesky
    n = 128
    rs = np.random.RandomState(7)
    for skew, tag in ((False, "spd"), (True, "skew")):
        edges = P.random_spd_edges(n, seed=3, skew=skew)
        xs = rs.random_sample(n)
        b = rs.random_sample(n)
        solves = ([(CG, NOPC, 1e-14), (CG, JACOBI, 1e-14), (CG, LDU, 1e-14)] if not skew
                  else [(BICGSTAB, NOPC, 1e-13), (BICGSTAB, JACOBI, 1e-13),
                        (BICGSTAB, LDU, 1e-13)])
        case(f"random_{tag}_128", n, n, CSR, edges, xs, b, solves)

    # ... and the SPD member of that family held in ELLPACK: rows of 3..13 entries in max_d = 13 slots, so most rows carry padding
    #     (the last neighbour repeated, value 0) that the LDU pattern and fill must not see
    edges = P.random_spd_edges(n, seed=3, skew=False)
    case("random_spd_ell_padded_128", n, n, ELL, edges, rs.random_sample(n), rs.random_sample(n),
         [(CG, NOPC, 1e-14), (CG, JACOBI, 1e-14), (CG, LDU, 1e-14), (BICGSTAB, LDU, 1e-13)])

    # duplicate edges in the insertion list (ll_graph%add_edge skips them; the second
    # set_value wins): exercises the de-duplication of the graph build
    edges, f, _ = P.diffusion_1d(16)
    ei = np.concatenate([edges[0], edges[0][::3]])
    ej = np.concatenate([edges[1], edges[1][::3]])
    ev = np.concatenate([edges[2], 2.5 + 0 * edges[2][::3]])
    for fmt, tag in ((CSR, "csr"), (ELL, "ell")):
        case(f"duplicates_{tag}_16", 16, 16, fmt, (ei, ej, ev), P.test_vector(16), f, [])


def perm_cases():
    """Reorderings (permutations.f90) + symmetric permutation by the colour ordering; the
    solves run on the PERMUTED matrix (ref_driver mode `perm`)."""
    nx, ny = 32, 24
    n = nx * ny
    case("perm_poisson2d_32x24", n, n, CSR, P.poisson2d_edges(nx, ny), P.test_vector(n), np.full(n, 1.0 / n),
         [(CG, NOPC, 1e-12), (CG, LDU, 1e-12), (BICGSTAB, LDU, 1e-12)], mode="perm")
    nx, ny, nz = 8, 7, 6
    n = nx * ny * nz
    case("perm_laplace3d_8x7x6", n, n, CSR, P.laplace3d_edges(nx, ny, nz), P.test_vector(n), np.full(n, 1.0 / n),
         [(CG, LDU, 1e-13)], mode="perm")
    nx, ny = 32, 24
    n = nx * ny
    case("perm_poisson2d_ell_32x24", n, n, ELL, P.poisson2d_edges(nx, ny), P.test_vector(n), np.full(n, 1.0 / n),
         [(CG, NOPC, 1e-12), (CG, JACOBI, 1e-12)], mode="perm")
    n = 128
    rs = np.random.RandomState(17)
    case("perm_random_spd_128", n, n, CSR, P.random_spd_edges(n, seed=3, skew=False), rs.random_sample(n),
         rs.random_sample(n), [(CG, LDU, 1e-14)], mode="perm")


def eig_cases():
    """lanczos / generalized_lanczos (src/eigensolver.f90:27-155, ref_driver mode `eig:<nsteps>`).
    The reference draws its start vector from a TIME-SEEDED generator (util.f90:72-102), so these
    two fixtures hold a different Q(:,1) every time they are regenerated; the tests feed the
    fixture's own Q(:,1) back as the start vector and compare T and Q from there."""
    nx, ny = 16, 12
    n = nx * ny
    case("eig_poisson2d_16x12", n, n, CSR, P.poisson2d_edges(nx, ny), P.test_vector(n), np.full(n, 1.0 / n), [],
         mode="eig:12", extra=dict(nsteps=np.int32(12), time_seeded_start_vector=np.int32(1)))
    nx, ny, nz = 6, 5, 4
    n = nx * ny * nz
    case("eig_laplace3d_6x5x4", n, n, CSR, P.laplace3d_edges(nx, ny, nz), P.test_vector(n), np.full(n, 1.0 / n), [],
         mode="eig:10", extra=dict(nsteps=np.int32(10), time_seeded_start_vector=np.int32(1)))


def comp_cases():
    """The composite `sparse_matrix` (sparse_matrix_composites.f90): the same entries split into a
    2 x 2 block matrix at row/column nb1 (ref_driver mode `comp:<nb1>`); y, y_add, yt, yt_add and
    the solves (CG, CG + Jacobi: jacobi_setup reads the composite through get_value) are the
    composite's.  The blocks' own ptr/node/val are in the fixture as ref_blk<it><jt>_*."""
    nx, ny = 32, 24
    n = nx * ny
    case("comp_poisson2d_32x24", n, n, CSR, P.poisson2d_edges(nx, ny), P.test_vector(n), np.full(n, 1.0 / n),
         [(CG, NOPC, 1e-12), (CG, JACOBI, 1e-12), (BICGSTAB, JACOBI, 1e-12)], mode="comp:401",
         extra=dict(nb1=np.int32(401)))
    n = 128
    rs = np.random.RandomState(27)
    case("comp_random_spd_128", n, n, CSR, P.random_spd_edges(n, seed=3, skew=False), rs.random_sample(n),
         rs.random_sample(n), [(CG, NOPC, 1e-14), (CG, JACOBI, 1e-14)], mode="comp:50", extra=dict(nb1=np.int32(50)))


def ell_delete_case():
    """ellpack_delete_edge (ellpack_graphs.f90:418-481, ref_driver mode `del:<file>`): a 12-vertex graph, then a list of
    delete_edge calls -- a last neighbour, an only neighbour, a diagonal stored last, middle neighbours, an edge that is not
    there, and the deletions that take the widest rows down so that the array shrinks.  The fixture holds the edge list, the
    delete list and node / degrees / max_d as the reference leaves them; tests/test_ell_degrees_cpu.py holds the numpy
    restatement (tests/ell_degree_cases.py) to it."""
    name = "ell_delete_edge_12"
    if ONLY and not name.startswith(ONLY):
        return
    n = 12
    rows = {1: [1, 2, 3], 2: [2], 3: [2, 4, 3], 4: [4, 3, 5, 9, 1], 5: [5, 4, 6, 10, 12], 6: [6, 5, 7], 7: [], 8: [8, 7, 9, 1],
            9: [9, 8, 10, 4], 10: [10, 9], 11: [3, 11], 12: [12, 5, 1, 2, 7]}
    ei = np.array([i for i in sorted(rows) for _ in rows[i]], np.int32)
    ej = np.array([j for i in sorted(rows) for j in rows[i]], np.int32)
    dele = [(1, 3), (2, 2), (3, 3), (4, 3), (6, 6), (6, 12), (9, 10), (9, 4), (11, 3), (11, 11), (7, 1),
            (4, 1), (5, 6), (12, 7), (12, 12), (8, 8)]
    di, dj = np.array([d[0] for d in dele], np.int32), np.array([d[1] for d in dele], np.int32)
    with tempfile.TemporaryDirectory() as td:
        df = os.path.join(td, "del.bin")
        with open(df, "wb") as f:
            f.write(struct.pack("<i", len(di)) + di.astype("<i4").tobytes() + dj.astype("<i4").tobytes())
        res = run_reference(n, n, ELL, (ei, ej, np.ones(len(ei))), np.zeros(n), np.zeros(n), [], mode="del:" + df)
    res.update(n=np.int32(n), ei=ei, ej=ej, di=di, dj=dj)
    os.makedirs(os.path.join(GOLDEN, "ell_degrees"), exist_ok=True)      # (a folder of its own: tests/golden/*.npz are matrix fixtures)
    np.savez_compressed(os.path.join(GOLDEN, "ell_degrees", name + ".npz"), **res)


if __name__ == "__main__":
    ell_delete_case()
    if ONLY and "ell_delete_edge_12".startswith(ONLY):
        sys.exit(0)
    main()
    perm_cases()
    eig_cases()
    comp_cases()
