"""The algebraic coarsening at C2 size: the 5-point Poisson matrix of an nx x nx grid, sg.aggregation_hierarchy (theta 0.08,
smooth_omega 2/3 and 0, at most 25 levels, down to 64 rows), V(1,1) with omega = 0.8 and 8 coarse sweeps on it, b = A *
test_vector.  Whole calls are timed with a host clock around a call that ends in a synchronisation, solves with HIP events on
the stream the library launches on; medians of --reps after a warm-up.

  level            per level and variant: rows, aggregates, strong adjacency entries, rounds, and the library's own HIP-event
                   times of the adjacency build, the rounds (their per-round readback included), numbering + phases, the
                   smoothing (tentative P, product, row scale, sum) and the Galerkin product -- taken from the SGM_TRACE lines
                   of a child process, medians over its builds
                   rounds_frac_8TBs: the rounds' compulsory bytes over their time, as a fraction of 8 TB/s.  Compulsory
                   bytes per round and pass: 4 B per strong adjacency entry (the int32 list) + one 8-byte gather per entry +
                   16 B per vertex (its own word read, the max written)
  hierarchy_build  the whole sg.aggregation_hierarchy call
  geometric_setup  the first sgm_pc_setup with problems.interp2d_hierarchy (what tools/mg_bench.py calls setup_first_s), in
                   the same process and visit; aggregation_setup: the same call on the aggregation hierarchy
  solve            CG to 1e-10: iterations and time with the aggregation hierarchy (smoothed, unsmoothed), the geometric one,
                   and plain CG

    python tools/aggregate_bench.py [--nx 3162] [--reps 5] [--min-coarse 64] [--out FILE]     one JSON line per figure
    python tools/aggregate_bench.py --build-only                             one hierarchy build (for a kernel trace)
"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK = 8.0e12
THETA, MAX_LEVELS = 0.08, 25
MIN_COARSE = 64                                              # (--min-coarse sets it)
OMEGA, NU, COARSE, TOL = 0.8, 1, 8, 1e-10
LINE = re.compile(r"aggregation level (\d+): rows (\d+), aggregates (\d+), strong (\d+), rounds (\d+), long rows (\d+), "
                  r"adjacency ([\d.]+) ms, rounds ([\d.]+) ms, phases ([\d.]+) ms, smoothing ([\d.]+) ms, galerkin ([\d.]+) ms")


def matrix(sg, nx):
    from sigma_amd import problems as P
    ptr, node, val = P.poisson2d_csr(nx, nx)
    return sg.csr_matrix(nx * nx, nx * nx, ptr, node, val), P.test_vector(nx * nx)


def build(sg, A, smooth):
    return sg.aggregation_hierarchy(A, theta=THETA, smooth_omega=smooth, max_levels=MAX_LEVELS, min_coarse=MIN_COARSE)


def wall(f):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = f()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def child(a):
    """the hierarchy built 1 + reps times with SGM_TRACE set by the parent: its stderr carries one line per level and build"""
    import sigma_amd as sg
    sg.init(0)
    A, _ = matrix(sg, a.nx)
    for _ in range(1 + a.reps):
        for P in build(sg, A, a.smooth):
            P.destroy()
        print("[bench] build done", file=sys.stderr, flush=True)


def level_figures(a, smooth):
    env = dict(os.environ, SGM_TRACE="1")
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--nx", str(a.nx), "--reps", str(a.reps), "--smooth", repr(smooth),
           "--min-coarse", str(a.min_coarse)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise SystemExit(f"the traced child failed ({r.returncode}):\n{r.stderr[-2000:]}")
    builds, cur = [], []
    for line in r.stderr.splitlines():
        m = LINE.search(line)
        if m:
            cur.append([int(v) for v in m.groups()[:6]] + [float(v) for v in m.groups()[6:]])
        elif "[bench] build done" in line:
            builds.append(cur)
            cur = []
    builds = builds[1:]                                     # the first build warms up
    out = []
    for l in range(len(builds[0])):
        rows = [b[l] for b in builds]
        lev, n, nagg, strong, rounds, nlong = rows[0][:6]
        t = {k: float(np.median([r_[6 + i] for r_ in rows])) * 1e-3
             for i, k in enumerate(("adjacency_s", "rounds_s", "phases_s", "smoothing_s", "galerkin_s"))}
        nbytes = rounds * 2 * (12 * strong + 16 * n)
        rec = {"figure": "level", "smooth_omega": smooth, "level": lev, "rows": n, "aggregates": nagg, "strong_entries": strong,
               "rounds": rounds, "long_rows": nlong, **t, "coarsening_s": t["adjacency_s"] + t["rounds_s"] + t["phases_s"],
               "rounds_bytes": nbytes, "rounds_frac_8TBs": nbytes / t["rounds_s"] / PEAK if t["rounds_s"] > 0 else None,
               "builds": len(rows)}
        out.append(rec)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=3162)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--smooth", type=float, default=2.0 / 3.0)
    ap.add_argument("--min-coarse", type=int, default=64, help="rows at which the descent stops (the library's default: 64)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--build-only", action="store_true", help="one hierarchy build: the run a kernel trace is taken of")
    a = ap.parse_args()
    global MIN_COARSE
    MIN_COARSE = a.min_coarse
    if a.child:
        return child(a)
    recs = []

    def emit(rec):
        rec = {"nx": a.nx, "min_coarse": a.min_coarse, **rec}
        recs.append(rec)
        print(json.dumps(rec), flush=True)
        if a.out:                                           # as it goes: a later stage that fails loses nothing
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(json.dumps(rec) + "\n")

    if a.build_only:
        import sigma_amd as sg
        sg.init(0)
        A, _ = matrix(sg, a.nx)
        Ps = build(sg, A, a.smooth)
        sg.synchronize()
        emit({"figure": "build_only", "smooth_omega": a.smooth, "sizes": [A.nrow] + [P.ncol for P in Ps]})
        return
    smooths = (2.0 / 3.0, 0.0)
    for s in smooths:                                       # one traced child at a time, before this process takes its memory
        for rec in level_figures(a, s):
            emit(rec)

    import torch
    import sigma_amd as sg
    from sigma_amd import problems as P
    sg.init(0)
    sg.use_torch_stream()
    nx, n = a.nx, a.nx * a.nx
    A, xs = matrix(sg, nx)
    hier = {}
    for s in smooths:
        ts = []
        for k in range(1 + a.reps):
            for M in hier.get(s, []):
                M.destroy()
            t, hier[s] = wall(lambda: build(sg, A, s))
            ts.append(t)
        emit({"figure": "hierarchy_build", "smooth_omega": s, "seconds": float(np.median(ts[1:])), "seconds_all": ts,
              "sizes": [n] + [M.ncol for M in hier[s]], "nnz_of_P": [M.nnz for M in hier[s]]})
    geo = [sg.csr_matrix(nf, nc, p, nd, v) for p, nd, v, nf, nc in P.interp2d_hierarchy(nx, nx)]

    def first_setup(Ps):
        ts = []
        for _ in range(4):                                  # a fresh preconditioner each time: levels built by sgm_mat_ptap
            pc = sg.multigrid(Ps, omega=OMEGA, nu_pre=NU, nu_post=NU, coarse_sweeps=COARSE)
            ts.append(wall(lambda: pc.setup(A))[0])
            pc.destroy()
        return float(np.median(ts[1:])), ts
    t, ts = first_setup(geo)
    emit({"figure": "geometric_setup", "seconds": t, "seconds_all": ts, "levels": len(geo) + 1})
    for s in smooths:
        t, ts = first_setup(hier[s])
        emit({"figure": "aggregation_setup", "smooth_omega": s, "seconds": t, "seconds_all": ts, "levels": len(hier[s]) + 1})

    r = torch.from_numpy(xs).cuda()
    b = torch.zeros_like(r)
    A.matvec(r, b)

    def solve(case, Ps):
        pc = None
        if Ps is not None:
            pc = sg.multigrid(Ps, omega=OMEGA, nu_pre=NU, nu_post=NU, coarse_sweeps=COARSE)
            pc.setup(A)
        solver = sg.cg(TOL)
        solver.setup(A)
        x = torch.zeros_like(b)
        ts = []
        for k in range(1 + 3):
            x.zero_()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            solver.solve(A, x, b, pc)
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e-3)
        emit({"figure": "solve", "case": case, "iterations": solver.last_iterations, "seconds": float(np.median(ts[1:])),
              "seconds_all": ts, "max_error": float((x - r).abs().max()), "info": pc.info()["name"] if pc else "plain CG"})
        if pc:
            pc.destroy()
    solve("aggregation_smoothed", hier[smooths[0]])
    solve("aggregation_unsmoothed", hier[smooths[1]])
    solve("geometric", geo)
    solve("plain_cg", None)


if __name__ == "__main__":
    main()
