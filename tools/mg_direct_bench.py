"""Multigrid's direct coarse solve (option "mg_coarse_direct") against the coarse sweeps it replaces.  The 5-point Poisson
matrix of an nx x nx grid, V(1,1), omega = 0.8, b = A * test_vector, CG to 1e-10.  Whole calls (hierarchy build, setup) are timed
with a host clock around a call that ends in a synchronisation; the inversion with the library's own clock
(sgm_pc_get "mg_coarse_invert_ms"); applies (a V-cycle: one synchronous apply; a coarse level alone: 20 queued back to back in asynchronous mode) and solves with HIP events on the stream the library launches on.  Medians of
--reps after a warm-up; the two coarse treatments ALTERNATE inside every repetition.

  c2            the smoothed aggregation hierarchy cut at --min-coarse (default 2000: the fill-in levels are not built and the
                last level fits the direct solve): hierarchy build, setup (+ the inversion alone), one apply (+ the coarse
                product / the eight coarse sweeps alone, as a one-level preconditioner on the coarsest matrix), CG
  geometric     interp2d_hierarchy cut at the first level of at most 4096 rows with the direct solve, against all levels
                with 8 sweeps: setup, apply, CG
  sizes         coarsest levels of 512, 1024, 2048 and 4096 rows (one 2:1 interpolation under a 63x31 .. 127x127 grid): the
                inversion against the setup with sweeps on the same hierarchy (= that level's Galerkin product + the inverse
                diagonals); the coarse product against the eight sweeps, and as a fraction of 8 TB/s on 8 n^2 + 16 n bytes -- back to
                back (the inverse stays in the 256 MiB last-level cache) and "cold", one apply after a 1 GiB fill

    python tools/mg_direct_bench.py [--nx 3162] [--reps 5] [--min-coarse 2000] [--out FILE] [--only c2,geometric,sizes]
    python tools/mg_direct_bench.py --invert-only 4096          one setup with the inversion (for a kernel trace)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK = 8.0e12
OMEGA, NU, COARSE, TOL = 0.8, 1, 8, 1e-10
SIZES = {512: (63, 31), 1024: (63, 63), 2048: (127, 63), 4096: (127, 127)}


def wall(f):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = f()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def poisson(sg, nx, ny):
    from sigma_amd import problems as P
    ptr, node, val = P.poisson2d_csr(nx, ny)
    return sg.csr_matrix(nx * ny, nx * ny, ptr, node, val), P.test_vector(nx * ny)


def geometric(sg, nx, ny, count=None):
    from sigma_amd import problems as P
    hs = P.interp2d_hierarchy(nx, ny)
    return [sg.csr_matrix(nf, nc, p, nd, v) for p, nd, v, nf, nc in (hs if count is None else hs[:count])]


def make(sg, Ps, coarse):
    return sg.multigrid(Ps, omega=OMEGA, nu_pre=NU, nu_post=NU, coarse_sweeps=COARSE, coarse=coarse)


def med(v):
    return float(np.median(v))


def setups(sg, A, variants, reps):
    """variants: {name: (Ps, coarse)}; fresh preconditioners, alternated; -> {name: (seconds, all, invert_ms or None)}"""
    ts = {k: [] for k in variants}
    inv = {k: [] for k in variants}
    for _ in range(1 + reps):
        for k, (Ps, coarse) in variants.items():
            pc = make(sg, Ps, coarse)
            ts[k].append(wall(lambda: pc.setup(A))[0])
            if coarse == "direct":
                inv[k].append(float(pc.get("mg_coarse_invert_ms", np.float64)[0]))
            pc.destroy()
    return {k: (med(ts[k][1:]), ts[k], med(inv[k][1:]) if inv[k] else None) for k in variants}


def applies(A, pcs, r, reps, inner=20):
    """pcs: {name: (pc, matrix)}; one apply on device vectors, HIP events around `inner` of them; alternated.  inner = 1: a
    single synchronous apply between the events, as tools/mg_bench.py times its V-cycle"""
    import torch
    import sigma_amd as sg
    ts = {k: [] for k in pcs}
    zs = {k: torch.zeros(M.nrow, dtype=torch.float64, device="cuda") for k, (_, M) in pcs.items()}
    rs = {k: r[:M.nrow].contiguous() for k, (_, M) in pcs.items()}
    for _ in range(1 + reps):
        for k, (pc, M) in pcs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            sg.set_async(inner > 1)                         # the applies queue back to back: no synchronisation between them
            e0.record()
            for _i in range(inner):
                pc.solve(M, zs[k], rs[k])
            e1.record()
            e1.synchronize()
            sg.set_async(False)
            ts[k].append(e0.elapsed_time(e1) * 1e-3 / inner)
    return {k: (med(ts[k][1:]), ts[k]) for k in pcs}


def cold_applies(pcs, r, reps):
    """one apply at a time, after a 1 GiB fill has pushed everything out of the caches: what a V-cycle at C2 size sees"""
    import torch
    flush = torch.empty(1 << 27, dtype=torch.float64, device="cuda")
    ts = {k: [] for k in pcs}
    zs = {k: torch.zeros(M.nrow, dtype=torch.float64, device="cuda") for k, (_, M) in pcs.items()}
    rs = {k: r[:M.nrow].contiguous() for k, (_, M) in pcs.items()}
    for i in range(1 + reps):
        for k, (pc, M) in pcs.items():
            flush.fill_(float(i))
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            pc.solve(M, zs[k], rs[k])
            e1.record()
            e1.synchronize()
            ts[k].append(e0.elapsed_time(e1) * 1e-3)
    return {k: (med(ts[k][1:]), ts[k]) for k in pcs}, zs, rs


def solves(sg, A, pcs, b, xs, reps):
    import torch
    out = {}
    ts = {k: [] for k in pcs}
    its, err = {}, {}
    solver = sg.cg(TOL)
    solver.setup(A)
    x = torch.zeros_like(b)
    for _ in range(1 + reps):
        for k, pc in pcs.items():
            x.zero_()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            solver.solve(A, x, b, pc)
            e1.record()
            e1.synchronize()
            ts[k].append(e0.elapsed_time(e1) * 1e-3)
            its[k] = solver.last_iterations
            err[k] = float((x - xs).abs().max())
    for k in pcs:
        out[k] = {"iterations": its[k], "seconds": med(ts[k][1:]), "seconds_all": ts[k], "max_error": err[k]}
    return out


def compare(sg, emit, tag, A, xs, variants, reps, coarse_alone):
    """setup, apply, CG for every variant of one matrix; coarse_alone: also the coarsest level's treatment on its own"""
    import torch
    r = torch.from_numpy(xs).cuda()
    b = torch.zeros_like(r)
    A.matvec(r, b)
    for k, (t, all_, inv) in setups(sg, A, variants, reps).items():
        emit({"figure": "setup", "case": tag, "variant": k, "seconds": t, "seconds_all": all_, "inversion_ms": inv})
    pcs = {}
    for k, (Ps, coarse) in variants.items():
        pcs[k] = make(sg, Ps, coarse)
        pcs[k].setup(A)
    ap = {k: (pc, A) for k, pc in pcs.items()}
    keep = []
    if coarse_alone:
        k0 = next(iter(variants))
        ML = pcs[k0].level_handle(len(variants[k0][0]))
        for coarse in ("direct", "sweeps"):
            pcl = make(sg, [], coarse)
            pcl.setup(ML)
            ap["coarse_alone_" + coarse] = (pcl, ML)
            keep.append(pcl)
    timed = applies(A, {k: v for k, v in ap.items() if not k.startswith("coarse_alone_")}, r, reps, inner=1)
    timed.update(applies(A, {k: v for k, v in ap.items() if k.startswith("coarse_alone_")}, r, reps))
    for k, (t, all_) in timed.items():
        pc, M = ap[k]
        emit({"figure": "apply", "case": tag, "variant": k, "rows": M.nrow, "seconds": t, "seconds_all": all_,
              "info": pc.info()["name"], "est_us": pc.info()["est_us"]})
    for k, rec in solves(sg, A, pcs, b, r, reps).items():
        emit({"figure": "solve", "case": tag, "variant": k, **rec, "info": pcs[k].info()["name"]})
    for pc in keep + list(pcs.values()):
        pc.destroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=3162)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--min-coarse", type=int, default=2000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default="c2,geometric,sizes")
    ap.add_argument("--invert-only", type=int, default=0, help="one setup with the inversion at this coarse size: the run a kernel trace is taken of")
    a = ap.parse_args()
    import torch
    import sigma_amd as sg
    sg.init(0)
    sg.use_torch_stream()

    def emit(rec):
        rec = {"nx": a.nx, **rec}
        print(json.dumps(rec), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(json.dumps(rec) + "\n")

    if a.invert_only:
        gx, gy = SIZES[a.invert_only]
        A, _ = poisson(sg, gx, gy)
        pc = make(sg, geometric(sg, gx, gy, 1), "direct")
        t, _ = wall(lambda: pc.setup(A))
        emit({"figure": "invert_only", "rows": a.invert_only, "setup_seconds": t, "inversion_ms": float(pc.get("mg_coarse_invert_ms", np.float64)[0])})
        return
    only = a.only.split(",")
    if "sizes" in only:
        for n, (gx, gy) in SIZES.items():
            A, xs = poisson(sg, gx, gy)
            Ps = geometric(sg, gx, gy, 1)
            assert Ps[0].ncol == n
            st = setups(sg, A, {"direct": (Ps, "direct"), "sweeps": (Ps, "sweeps")}, a.reps)
            pcs = {}
            ML = None
            for coarse in ("direct", "sweeps"):
                full = make(sg, Ps, coarse)
                full.setup(A)
                ML = full.level_handle(1)
                pcs[coarse] = (make(sg, [], coarse), ML)
                pcs[coarse][0].setup(ML)
                pcs["_keep_" + coarse] = full
            keep = [pcs.pop("_keep_direct"), pcs.pop("_keep_sweeps")]
            r = torch.from_numpy(xs).cuda()
            at = applies(A, pcs, r, a.reps)
            ct, zs, rs = cold_applies(pcs, r, a.reps)
            inv = keep[0].coarse_inverse()                  # the product against numpy's, on the inverse the device holds
            want = inv @ rs["direct"].cpu().numpy()
            perr = float(np.abs(zs["direct"].cpu().numpy() - want).max() / np.abs(want).max())
            nbytes = 8.0 * n * n + 16.0 * n
            emit({"figure": "size", "rows": n, "fine_rows": A.nrow, "coarse_nnz": ML.nnz,
                  "inversion_ms": st["direct"][2], "setup_with_sweeps_ms": st["sweeps"][0] * 1e3, "setup_with_direct_ms": st["direct"][0] * 1e3,
                  "product_us": at["direct"][0] * 1e6, "eight_sweeps_us": at["sweeps"][0] * 1e6,
                  "product_cold_us": ct["direct"][0] * 1e6, "eight_sweeps_cold_us": ct["sweeps"][0] * 1e6,
                  "product_bytes": nbytes, "product_frac_8TBs": nbytes / at["direct"][0] / PEAK,
                  "product_cold_frac_8TBs": nbytes / ct["direct"][0] / PEAK, "product_rel_diff_to_numpy": perr,
                  "product_us_all": [t * 1e6 for t in at["direct"][1]], "eight_sweeps_us_all": [t * 1e6 for t in at["sweeps"][1]]})
            del keep
    nx = a.nx
    if "c2" in only or "geometric" in only:
        A, xs = poisson(sg, nx, nx)
    if "c2" in only:
        ts, Ps = [], []
        for _ in range(1 + min(a.reps, 3)):
            for M in Ps:
                M.destroy()
            t, Ps = wall(lambda: sg.aggregation_hierarchy(A, theta=0.08, smooth_omega=2.0 / 3.0, max_levels=25, min_coarse=a.min_coarse))
            ts.append(t)
        emit({"figure": "hierarchy_build", "case": "aggregation", "min_coarse": a.min_coarse, "seconds": med(ts[1:]), "seconds_all": ts,
              "sizes": [A.nrow] + [M.ncol for M in Ps]})
        compare(sg, emit, "aggregation", A, xs, {"direct": (Ps, "direct"), "sweeps": (Ps, "sweeps")}, a.reps, True)
    if "geometric" in only:
        full = geometric(sg, nx, nx)
        sizes = [nx * nx] + [M.ncol for M in full]
        cut = next(i for i, s in enumerate(sizes) if s <= 4096)
        emit({"figure": "hierarchy", "case": "geometric", "sizes": sizes, "cut_levels": cut + 1, "cut_rows": sizes[cut]})
        compare(sg, emit, "geometric", A, xs, {"cut_direct": (full[:cut], "direct"), "full_sweeps": (full, "sweeps"),
                                               "cut_sweeps": (full[:cut], "sweeps")}, a.reps, False)


if __name__ == "__main__":
    main()
