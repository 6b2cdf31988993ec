"""Multi-vector products Y = A X against k single products, on the four layouts that have native kernels.  Device blocks
(k, n) on the stream the library launches on, HIP events, the library asynchronous while a sample is taken (no host wait between
the k single products), one warm-up, medians of --reps samples taken ALTERNATING (matmat, column loop, k x matvec, ...).
Recorded, not gated.

  operands   c2        problems.poisson2d_csr(3162, 3162)       the 4-bit sliced form, W = 5
             grid7     the 7-point 300^3 grid                    the 4-bit sliced form, W = 7
             grid27    a 27-point 160^3 grid                     the 1-byte sliced form
             interp    problems.interp2d_csr(3162, 3162)         rows of <= 4 entries: the library gives it k_csr_do, so the column loop
             band12    4 M rows of 12 entries within +-4096      the int32-column sliced form
  per k      matmat_us, loop_us (the column loop: sgm_mat_matmat_probe with block_cap = 1), matvec_us (k calls of matvec),
             ratio = matmat / (k x matvec) beside `model`, the byte model of the layout per row:
                 4-bit (8W + 4 + 16k) / k(8W + 20)     1-byte (9W + 16k) / k(9W + 16)     int32 (12W + 16k) / k(12W + 16)
             spread = the larger (max - min) / median of the matmat and the k x matvec samples; `wins` (k = a block width
             only): matmat faster by more than twice that spread -- the test a (form, KB) pair stays selected by
             gbps = the bytes the product moves by construction (the matrix stream of sgm_mat_footprint once, k x the vectors)
             over matmat's time, beside copy_gbps: a device copy of 2^27 bytes measured in the same run

    python tools/matmat_bench.py [--scale 1.0] [--reps 7] [--operands c2,grid7,grid27,interp,band12] [--out FILE]     one JSON line
    python tools/matmat_bench.py --trace       a few calls of every product per operand, for a kernel trace of its own
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KS = (2, 4, 8, 16)


def stencil27(nx, ny, nz):
    """27-point stencil, columns ascending, values that differ from entry to entry (1-based ptr / node)."""
    n = nx * ny * nz
    idx = np.arange(n, dtype=np.int64)
    i, j, k = idx % nx, (idx // nx) % ny, idx // (nx * ny)
    cols = np.empty((n, 27), np.int32)
    ok = np.empty((n, 27), bool)
    q = 0
    for dk in (-1, 0, 1):
        for dj in (-1, 0, 1):
            for di in (-1, 0, 1):
                ok[:, q] = (i + di >= 0) & (i + di < nx) & (j + dj >= 0) & (j + dj < ny) & (k + dk >= 0) & (k + dk < nz)
                cols[:, q] = idx + di + dj * nx + dk * nx * ny + 1
                q += 1
    ptr = np.concatenate([[1], 1 + np.cumsum(ok.sum(1))]).astype(np.int32)
    node = cols[ok]
    val = -1.0 - 1e-3 * (np.arange(node.size) % 13)
    return ptr, node, val


def operands(scale):
    from sigma_amd import problems as P
    e2, e7, e27 = max(16, int(3162 * scale ** 0.5)), max(8, int(300 * scale ** (1 / 3))), max(8, int(160 * scale ** (1 / 3)))
    e2 += e2 % 2                                                       # (even edges: even vector lengths, blocks used in place)
    e7 += e7 % 2
    e27 += e27 % 2

    def c2():
        ptr, node, val = P.poisson2d_csr(e2, e2)
        return e2 * e2, e2 * e2, ptr, node, val

    def grid7():
        ptr, node, val = P.laplace3d_csr(e7, e7, e7)
        return e7 ** 3, e7 ** 3, ptr, node, val

    def grid27():
        ptr, node, val = stencil27(e27, e27, e27)
        return e27 ** 3, e27 ** 3, ptr, node, val

    def interp():
        ptr, node, val, nc = P.interp2d_csr(e2, e2)
        return e2 * e2, nc, ptr, node, val

    def band12():
        # rows of 12 entries at random columns within +-4096 of the diagonal: more than 255 offsets, so no dictionary
        n = 4 * e2 * e2 // 10
        n += n % 2
        rs = np.random.RandomState(12)
        rows = np.repeat(np.arange(n, dtype=np.int64), 12)
        node = (np.clip(rows + rs.randint(-4096, 4097, size=rows.size), 0, n - 1) + 1).astype(np.int32)
        return n, n, (1 + 12 * np.arange(n + 1, dtype=np.int64)).astype(np.int32), node, rs.standard_normal(rows.size)

    return {"c2": (c2, "sl"), "grid7": (grid7, "sl"), "grid27": (grid27, "slb"), "interp": (interp, "sl32"), "band12": (band12, "sl32")}


def model(form, W, k):
    a, b = {"sl": (8 * W + 4, 16), "slb": (9 * W, 16), "sl32": (12 * W, 16)}[form]
    return (a + b * k) / (k * (a + b))


def timed(torch, f, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        f()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / inner


def spread(ts):
    return (max(ts) - min(ts)) / float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0, help="rows of every operand, as a fraction of the documented sizes")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3, help="calls per sample")
    ap.add_argument("--operands", default="c2,grid7,grid27,interp,band12")
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    import re
    import torch
    import sigma_amd as sg
    sg.init(0)
    torch.cuda.set_stream(torch.cuda.Stream())          # a stream of its own: the events and the library's launches share it
    sg.use_torch_stream()
    src = torch.ones(1 << 23, dtype=torch.float64, device="cuda")
    dst = torch.zeros_like(src)
    dst.copy_(src)
    copy_gbps = 2 * src.numel() * 8 / float(np.median([timed(torch, lambda: dst.copy_(src), 5) for _ in range(a.reps)])) * 1e-9
    rec = {"scale": a.scale, "reps": a.reps, "inner": a.inner, "copy_gbps": copy_gbps, "operands": {}}
    ops = operands(a.scale)
    for name in a.operands.split(","):
        make, form = ops[name]
        n, m, ptr, node, val = make()
        A = sg.csr_matrix(n, m, ptr, node, val)
        del ptr, node, val
        W = int(re.search(r"W=(\d+)", A.kernel).group(1)) if "W=" in A.kernel else 0
        mv_bytes = A.footprint()[1]
        ld_x, ld_y = m + m % 2, n + n % 2                             # even leading dimensions: the blocks are used in place
        kmax = max(KS)
        X = torch.randn((kmax, ld_x), dtype=torch.float64, device="cuda")
        Y = torch.zeros((kmax, ld_y), dtype=torch.float64, device="cuda")
        out = {"rows": n, "cols": m, "kernel": A.kernel, "form": form, "W": W, "matvec_bytes": mv_bytes, "k": {}}
        sg.set_async(True)
        try:
            for k in ((4,) if a.trace else KS):
                Xk, Yk = X[:k], Y[:k]
                f_mm = lambda: A.matmat(Xk, Yk)                                               # noqa: E731
                f_loop = lambda: sg.matmat_probe(A, Xk, Yk, block_cap=1)                      # noqa: E731
                f_mv = lambda: [A.matvec(X[j], Y[j]) for j in range(k)]                       # noqa: E731
                for f in (f_mm, f_loop, f_mv):
                    f()
                if a.trace:
                    continue
                t = {"mm": [], "loop": [], "mv": []}
                for _ in range(a.reps):
                    t["mm"].append(timed(torch, f_mm, a.inner))
                    t["loop"].append(timed(torch, f_loop, a.inner))
                    t["mv"].append(timed(torch, f_mv, a.inner))
                mm, loop, mv = (float(np.median(t[q])) for q in ("mm", "loop", "mv"))
                sp = max(spread(t["mm"]), spread(t["mv"]))
                moved = mv_bytes - 8 * (n + m) + k * 8 * (n + m)
                r = {"kernel": A.matmat_kernel(k), "matmat_us": mm * 1e6, "loop_us": loop * 1e6, "matvec_us": mv * 1e6,
                     "ratio": mm / mv, "model": model(form, W, k) if W and A.matmat_kernel(k).startswith("k_mm_") else None, "spread": sp,
                     "gbps": moved / mm * 1e-9, "matvec_gbps": k * mv_bytes / mv * 1e-9}
                if A.matmat_kernel(k).endswith(f"KB={k}> x1"):
                    r["wins"] = bool(mm < mv * (1.0 - 2.0 * sp))
                out["k"][str(k)] = r
        finally:
            sg.set_async(False)
            sg.synchronize()
        rec["operands"][name] = out
        A.destroy()
        del A, X, Y
        torch.cuda.empty_cache()
    print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
