"""CPU-side checks of the drop-in boundary: the C-ABI library loads, exports every symbol
include/sigma_hip.h declares, fails loudly without a GPU, and its host-only index work
(halo planning) is bit-exact against a numpy restatement."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sigma_amd as sg
from sigma_amd import problems as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    txt = open(os.path.join(ROOT, "include", "sigma_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(sgm_[a-z0-9_]+)\s*\(", txt)))


def test_library_builds_and_exports_every_declared_symbol():
    sg.build()
    L = sg.lib()
    names = declared_symbols()
    assert len(names) >= 40
    for nm in names:
        assert hasattr(L, nm), f"{nm} declared in include/sigma_hip.h but not exported"


def test_no_torch_types_in_the_abi():
    txt = open(os.path.join(ROOT, "include", "sigma_hip.h")).read()
    assert "torch" not in re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert 'extern "C"' in txt


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


@pytest.mark.skipif(_has_gpu(), reason="GPU present: the loud-failure path cannot be seen")
def test_product_fails_loudly_without_gpu():
    ptr, node, val = P.poisson2d_csr(4, 4)
    with pytest.raises(sg.SigmaError) as e:
        sg.csr_matrix(16, 16, ptr, node, val)
    assert e.value.code == 6 and "no CPU path" in str(e.value)


@pytest.mark.skipif(_has_gpu(), reason="GPU present: the loud-failure path cannot be seen")
def test_bench_gpus_2_spawns_ranks_that_fail_at_no_device():
    """`python bench.py --gpus 2` typed plainly: the parent spawns the two rank processes itself
    (no torch.distributed.run, no exec) and on a CPU-only box they fail only at SGM_ERR_NO_DEVICE."""
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1"], env=env,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode != 0
    assert "sigma_hip status 6" in p.stderr and "no CPU path" in p.stderr
    assert "rank exit codes: [1, 1]" in p.stderr
    assert p.stdout.strip() == ""


def test_product_never_imports_the_oracle():
    import sys
    for fn in os.listdir(os.path.join(ROOT, "sigma_amd")):
        if fn.endswith(".py"):
            src = open(os.path.join(ROOT, "sigma_amd", fn)).read()
            assert "import oracle" not in src and "from oracle" not in src and "liborc" not in src
    for fn in os.listdir(os.path.join(ROOT, "sigma_amd", "csrc")):
        if not fn.endswith((".hip", ".hpp", ".cpp", ".h", "Makefile")):
            continue
        src = open(os.path.join(ROOT, "sigma_amd", "csrc", fn)).read()
        assert "oracle/" not in src.replace("links oracle/", "") and "liborc" not in src


def numpy_halo_plan(n_own, col_begin, node):
    node = node.astype(np.int64)
    own = (node > col_begin) & (node <= col_begin + n_own)
    halo = np.unique(node[~own])
    local = np.where(own, node - col_begin, n_own + 1 + np.searchsorted(halo, node))
    return local.astype(np.int32), halo.astype(np.int32)


@pytest.mark.parametrize("nparts", [2, 3, 4, 8])
def test_halo_plan_bit_exact(nparts):
    for (ptr, node, val), n in ((P.poisson2d_csr(37, 29), 37 * 29), (P.laplace3d_csr(9, 8, 11), 9 * 8 * 11)):
        starts = (np.arange(nparts + 1) * n // nparts) // 2 * 2
        starts[-1] = n
        for p in range(nparts):
            r0, r1 = starts[p], starts[p + 1]
            seg = node[ptr[r0] - 1: ptr[r1] - 1]
            loc, halo = sg.halo_plan_host(r1 - r0, r0, seg)
            loc_np, halo_np = numpy_halo_plan(r1 - r0, r0, seg)
            assert np.array_equal(loc, loc_np)
            assert np.array_equal(halo, halo_np)
    # random columns, including none outside the owned range
    rs = np.random.RandomState(0)
    node = rs.randint(1, 1001, size=5000).astype(np.int32)
    loc, halo = sg.halo_plan_host(1000, 0, node)
    assert len(halo) == 0 and np.array_equal(loc, node)
    loc, halo = sg.halo_plan_host(100, 450, node)
    loc_np, halo_np = numpy_halo_plan(100, 450, node)
    assert np.array_equal(loc, loc_np) and np.array_equal(halo, halo_np)


def test_fortran_shim_binds_only_declared_symbols():
    """Every bind(c) name in the Fortran host layer is declared in include/sigma_hip.h."""
    src = open(os.path.join(ROOT, "sigma_amd", "fortran", "sigma_hip.f90")).read()
    names = set(re.findall(r"bind\(c,\s*name='(sgm_[a-z0-9_]+)'\)", src))
    assert len(names) >= 20
    assert names <= set(declared_symbols())


# exports no Fortran layer binds, by name and with the reason ("every export bound by at least one
# Fortran layer or lists the exceptions by name")
NOT_FOR_A_FORTRAN_HOST = {
    "sgm_halo_plan_host": "host-only index work, exported so that tests can check it bit for bit without a GPU",
    "sgm_dist_plan_host": "same",
    "sgm_dist_neighbors_host": "same",
    "sgm_partition_links_host": "same",
    "sgm_mat_halo_nbr": "reads the exchange plan of a built matrix back for the parity tests",
    "sgm_mat_matvec_dots": "reads the fused partial sums of a product back for the parity tests",
    "sgm_slice_sched_host": "the slice schedule as a host table, so that a CPU test can check it is a permutation",
    "sgm_ell_degrees_host": "host-only index work (the degrees of an ELLPACK graph from its padding), exported for the CPU tests",
    "sgm_left_permute_rows_host": "host-only index work (a rank's rows of a permuted matrix), exported for the CPU tests",
    "sgm_comm_group_ok": "reads back what sgm_comm_init's probe of the transport found, for the GPU tests and bench.py",
    "sgm_comm_group_selftest": "a transport probe (does this RCCL take a group of send / recv + all-reduce?) for the GPU tests",
}


def test_every_export_is_bound_by_a_fortran_layer_or_listed_as_an_exception():
    """The Fortran host reaches the whole C ABI: every entry point of include/sigma_hip.h has a bind(c) interface in
    sigma_amd/fortran/sigma_hip.f90 (stand-alone) or oracle/hip_binding.f90 (reference-side), except the test-introspection
    helpers named above -- and those two lists are disjoint and complete."""
    decl = set(declared_symbols())
    bound = set()
    for f in (os.path.join(ROOT, "sigma_amd", "fortran", "sigma_hip.f90"), os.path.join(ROOT, "oracle", "hip_binding.f90")):
        bound |= set(re.findall(r"bind\(c,\s*name='(sgm_[a-z0-9_]+)'\)", open(f).read()))
    assert bound <= decl, bound - decl
    assert not (bound & set(NOT_FOR_A_FORTRAN_HOST))
    assert decl - bound == set(NOT_FOR_A_FORTRAN_HOST), (sorted(decl - bound - set(NOT_FOR_A_FORTRAN_HOST)),
                                                         sorted(set(NOT_FOR_A_FORTRAN_HOST) - (decl - bound)))
    # the surface VERDICT r03 named as unreachable from Fortran is bound by BOTH layers now
    ref = set(re.findall(r"name='(sgm_[a-z0-9_]+)'", open(os.path.join(ROOT, "oracle", "hip_binding.f90")).read()))
    for nm in ("sgm_comm_unique_id", "sgm_comm_init", "sgm_csr_create_dist", "sgm_partition_rows_by_nnz", "sgm_composite_create",
               "sgm_lanczos", "sgm_generalized_lanczos", "sgm_csr_from_edges"):
        assert nm in ref, nm


REF_BINDING_TEST = os.path.join(ROOT, "oracle", "_ref", "hip_binding_test")


@pytest.mark.skipif(not os.path.exists(REF_BINDING_TEST), reason="oracle/_ref not built (no reference sources / compiler here)")
@pytest.mark.skipif(_has_gpu(), reason="GPU present: the loud-failure path cannot be seen")
def test_reference_side_binding_links_and_dies_like_the_reference_without_a_gpu():
    """oracle/hip_binding.f90 -- types that EXTEND the reference's csr_matrix / ellpack_matrix /
    linear_solver -- compiled against the reference's own modules and linked with libsigma_hip.so
    (oracle/build_ref.sh).  Without a GPU its first product ends the program the way the
    reference ends on errors: a message and exit(1) (cg_solvers.f90:61-65)."""
    import subprocess
    p = subprocess.run([REF_BINDING_TEST], capture_output=True, text=True, timeout=120)
    assert p.returncode == 1
    assert "sigma_hip status" in p.stdout and "Terminating." in p.stdout and "no HIP device" in p.stdout


def test_integration_md_quotes_the_compiled_binding_verbatim():
    """INTEGRATION.md shows excerpts of the compiled binding (tools/sync_integration_md.py refreshes them): every fenced
    Fortran block of the document is verbatim text of oracle/hip_binding.f90, and the document stays a document."""
    src = open(os.path.join(ROOT, "oracle", "hip_binding.f90")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    blocks = re.findall(r"```fortran\n(.*?)\n```", doc, flags=re.S)
    assert len(blocks) >= 4
    for b in blocks:
        assert b in src, "an excerpt in INTEGRATION.md is not verbatim text of oracle/hip_binding.f90:\n" + b[:200]
    assert len(doc.splitlines()) <= 400, "INTEGRATION.md is the flows + excerpts, not a copy of the binding"
    assert "Which parity gate each dot order meets" in doc and "9388" in doc and "sgm_pc_info" in doc


def test_one_hip_runtime_per_process_whichever_side_loads_first():
    """Loading libsigma_hip.so before `import torch` must not leave two HIP/HSA runtimes mapped
    (the second one finds no GPU: torch then reports "No HIP GPUs are available")."""
    import subprocess
    import sys
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import sigma_amd as sg; sg.lib(); import torch\n"
            "libs = sorted(set(l.split()[-1] for l in open('/proc/self/maps')\n"
            "              if 'libamdhip64' in l or 'libhsa-runtime64' in l))\n"
            "print('\\n'.join(libs))\n" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-400:]
    libs = out.stdout.split()
    assert sum("libamdhip64" in l for l in libs) == 1, libs
    assert sum("libhsa-runtime64" in l for l in libs) == 1, libs


@pytest.mark.parametrize("nsl,period,grid,band", [(195112, 215296, 8192, 64), (24389, 215296, 4096, 64), (19411, 46225, 4096, 32),
                                                   (1000, 20000, 64, 16), (17, 999999, 8, 64), (4096, 16384, 2048, 8)])
def test_slice_schedule_is_a_permutation(nsl, period, grid, band):
    """sgm_slice_sched_host (host-only; the table the sliced kernels walk when "slice_sched" is on): every slice
    exactly once, a workgroup's empty entries only at its tail, slices one period apart on the same XCD
    (workgroup % 8) and about one band apart in its sequence."""
    t = sg.slice_sched_host(nsl, period, grid, band)
    assert t.shape[1] == grid
    v = t[t >= 0]
    assert np.array_equal(np.sort(v), np.arange(nsl))
    filled = (t >= 0)
    assert np.all(filled[:-1] | ~filled[1:])          # once a column is empty it stays empty
    xcd_of = np.empty(nsl, np.int64)
    pos_of = np.empty(nsl, np.int64)
    it, b = np.nonzero(filled)
    xcd_of[t[it, b]] = b % 8
    pos_of[t[it, b]] = it * (grid // 8) + b // 8
    step = period / 512.0
    if step >= 32 and nsl > 4 * step:
        s0 = np.arange(0, int(nsl - step - 1))
        s1 = np.round(s0 + step).astype(np.int64)
        same = xcd_of[s0] == xcd_of[s1]
        assert same.mean() > 0.9                       # (band edges: the neighbour one plane up may sit in the next band)
        d = (pos_of[s1] - pos_of[s0])[same]
        assert np.median(np.abs(d)) <= 2 * band + 2


def test_every_documented_option_is_accepted_and_unknown_names_are_refused():
    """The option names in the header's comment and the ones the library knows are the same set, group by group (no GPU
    needed: options are plain settings); the process-wide defaults stay at most 20 entries."""
    hdr = open(os.path.join(ROOT, "include", "sigma_hip.h")).read()
    start = hdr.index("/* ---- options")
    block = hdr[start:hdr.index("int sgm_set_option", start)]
    names = set(re.findall(r'^ \*   "([a-z_0-9]+)" \(', block, flags=re.M))
    assert {"csr_offset_dict", "csr_row_owner", "csr_row_lines", "csr_sliced", "cg_small", "slice_sched", "dot_order",
            "ildu_rows"} <= names, names
    src = open(os.path.join(ROOT, "sigma_amd", "csrc", "sgm_runtime.hip")).read()
    known = set(re.findall(r"SGM_OPT\((?:mat|solver|pc), ([a-z_0-9]+)\)", src)) | {"dist_force_collectives"}
    assert names == known, (names - known, known - names)
    assert len(known) <= 27            # 26 per-handle options + the one process-wide switch
    # ... and nothing else selects a kernel or an arithmetic order: the library reads three environment variables, none of which
    # changes a result -- SGM_TRACE (which path ran, on stderr), SGM_PC_TIMING (setup phase times on stderr),
    # SGM_RCCL_LIB (which RCCL build to dlopen)
    envs = set()
    for fn in os.listdir(os.path.join(ROOT, "sigma_amd", "csrc")):
        if fn.endswith((".hip", ".hpp")):
            envs |= set(re.findall(r'getenv\("([A-Z_0-9]+)"\)', open(os.path.join(ROOT, "sigma_amd", "csrc", fn)).read()))
    assert envs == {"SGM_TRACE", "SGM_PC_TIMING", "SGM_RCCL_LIB"}, envs
    nsites = sum(open(os.path.join(ROOT, "sigma_amd", "csrc", fn)).read().count("getenv(") for fn in os.listdir(os.path.join(ROOT, "sigma_amd", "csrc"))
                 if fn.endswith((".hip", ".hpp")))
    assert nsites <= 5, nsites
    # the measured-slower paths of round 3 are gone
    for gone in ("ell_colblock_band", "ell_colblock_pieces", "ell_colblock_nt", "slice_sched_band", "cg_small_chunk",
                 "krylov_graph_after", "ell_colblock_chunks"):
        assert gone not in known and sg.lib().sgm_set_option(gone.encode(), 1) != 0
    lib = sg.lib()
    defaults = {"ell_colblock_cols": 16384, "ell_colblock_rows": 0, "slice_sched": 0, "dot_order": 0, "ildu_reorder": 0,
                "pipeline_spin_limit": 0, "dist_force_collectives": 0, "dist_halo_fused": 1, "coop_spin_limit": 0,
                "cg_coop_variant": 0, "reorder_solve": 2, "coloring_pass": 0}
    for nm in sorted(known):
        assert lib.sgm_set_option(nm.encode(), defaults.get(nm, 1)) == 0, nm          # (set to its default: nothing changes)
    assert lib.sgm_set_option(b"no_such_option", 1) != 0
    assert lib.sgm_set_option(b"dot_order", 2) != 0
    # the per-handle setters refuse a null handle instead of dereferencing it
    assert lib.sgm_solver_set_option(None, b"dot_order", 1) != 0 and lib.sgm_pc_set_option(None, b"ildu_rows", 1) != 0


def test_device_side_generators_reproduce_the_numpy_ones():
    """bench.py generates C3 / C4 / C5 on the device with torch (sigma_amd.problems.*_torch); here the same functions on
    the CPU against the numpy generators the golden fixtures and the oracle tests use -- entry for entry."""
    import torch
    dev = torch.device("cpu")
    for a, b in ((P.tridiag_csr(257, 2.0, -0.9, -1.1), P.tridiag_csr_torch(257, 2.0, -0.9, -1.1, dev)),
                 (P.laplace3d_csr(7, 5, 4), P.laplace3d_rows_torch(7, 5, 4, dev))):
        for x, y in zip(a, b):
            assert np.array_equal(x, y.numpy())
    # a z-slab of the 3-D grid = the same rows of the whole matrix (local ptr, global columns)
    ptr, node, val = P.laplace3d_csr(6, 5, 7)
    p2, n2, v2 = (t.numpy() for t in P.laplace3d_rows_torch(6, 5, 7, dev, z0=2, z1=5))
    r0, r1 = 2 * 30, 5 * 30
    assert np.array_equal(p2, ptr[r0:r1 + 1] - ptr[r0] + 1)
    assert np.array_equal(n2, node[ptr[r0] - 1:ptr[r1] - 1]) and np.array_equal(v2, val[ptr[r0] - 1:ptr[r1] - 1])
    n = 3000
    ei, ej, ev = P.random_regular_ell(n, 32, 12345)
    node, val = P.random_regular_ell_torch(n, 32, 12345, dev, chunk=1000)
    assert np.array_equal(node.numpy(), ej.reshape(n, 32)) and np.array_equal(val.numpy(), ev.reshape(n, 32))


def test_heartbeat_is_readable_without_a_gpu_and_from_any_thread():
    hb = sg.heartbeat()
    assert hb["phase_code"] == 0 and hb["phase"].startswith("idle") and hb["halo_posts"] == 0


def test_bench_watchdog_ends_a_process_that_stops_making_progress(tmp_path):
    """bench.Heartbeat: a rank whose phase does not change for --stall-s prints where it is and exits 86 (here a process that
    simply sleeps; on the GPU box tests/test_gpu_multirank.py stalls a rank inside a halo exchange)."""
    import subprocess
    import sys
    import time
    code = ("import sys, time; sys.path.insert(0, %r)\n"
            "import bench\n"
            "hb = bench.Heartbeat(3, 1.5, 100.0)\n"
            "hb.phase('c2: timed steps (test)')\n"
            "time.sleep(60)\n" % ROOT)
    env = dict(os.environ, SGM_BENCH_HB_DIR=str(tmp_path))
    t0 = time.time()
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, env=env)
    assert p.returncode == 86 and time.time() - t0 < 30
    assert "rank 3 STALLED" in p.stderr and "c2: timed steps (test)" in p.stderr
    import json
    st = json.load(open(tmp_path / "rank3.hb"))
    assert st["phase"] == "c2: timed steps (test)" and "no heartbeat" in st["stalled"]
    # ... and the deadline on a process that keeps beating
    code2 = code.replace("1.5, 100.0", "50.0, 2.0").replace("time.sleep(60)", "\nfor i in range(600):\n    hb.phase(f'step {i}'); time.sleep(0.1)")
    p = subprocess.run([sys.executable, "-c", code2], capture_output=True, text=True, timeout=120, env=env)
    assert p.returncode == 86 and "past --deadline-s" in p.stderr


def test_header_is_c99_and_a_plain_c_program_links_and_fails_loudly_without_a_gpu(tmp_path):
    """include/sigma_hip.h is a C header: tools/c_driver.c (BASELINE C1 through the C ABI, no C++ and no Python in the
    process) compiles as strict C99 against it, links with libsigma_hip.so alone, and -- here, without a GPU -- stops at
    sgm_init with the library's own message instead of computing anything on the host."""
    import subprocess
    exe = str(tmp_path / "c_driver")
    so_dir = os.path.join(ROOT, "sigma_amd")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tools", "c_driver.c"), "-L", so_dir, "-lsigma_hip", "-Wl,-rpath," + so_dir, "-lm", "-o", exe],
                   check=True, capture_output=True, text=True)
    p = subprocess.run([exe, "100"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 2, (p.returncode, p.stdout, p.stderr)
    assert "sgm_init" in p.stderr and "no CPU path" in p.stderr, p.stderr


def _bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_bench_refuses_zero_timed_steps():
    """`--steps` is the number of timed steps and `ms_per_step` is divided by it: 0 is refused before anything starts."""
    import subprocess
    import sys
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 2 and "--steps must be at least 1" in p.stderr, (p.returncode, p.stderr)
    assert p.stdout.strip() == ""


def test_bench_dump_outputs_are_the_same_rows_on_every_run(tmp_path):
    """--dump-outputs: y as float64; above DUMP_MAX_ROWS rows a fixed, ascending sample of rows, the same on every run."""
    import torch
    bench = _bench_module()
    small = torch.arange(1000, dtype=torch.float64)
    bench.dump_outputs(str(tmp_path / "s"), small, 1000)
    got = np.load(str(tmp_path / "s" / "y.npy"))
    assert got.dtype == np.float64 and np.array_equal(got, small.numpy())
    n = bench.DUMP_MAX_ROWS + 12345
    y = torch.arange(n, dtype=torch.float64) * 0.5
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), y, n)
    a, b = np.load(str(tmp_path / "a" / "y.npy")), np.load(str(tmp_path / "b" / "y.npy"))
    assert a.dtype == np.float64 and a.shape == (bench.DUMP_MAX_ROWS,) and a.nbytes <= 64 << 20
    assert np.array_equal(a, b)
    rows = a / 0.5
    assert np.all(np.diff(rows) > 0) and rows[0] >= 0 and rows[-1] < n


def test_bench_flat_keys_fit_the_drivers_record():
    """The driver keeps the first 24 scalars of `roofline` (6 are bound..traffic): the 18 after them must be the one-per-graded-
    thing list of VERDICT r05 item 1, whatever else the legs emit (r05's record lost C3 / C4 / cold / in-solver to new keys)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    wanted = ["cold_frac", "in_solver_frac", "c2_cg_iters_per_s", "c2_cg_frac_moved", "c3_spmv_frac_moved",
              "c3_bicgstab_iters_per_s", "c3_gmres30_iters_per_s", "c4_spmv_ms", "c4_spmv_frac_survey_bytes",
              "c4_product_bit_exact", "c5_1gpu_spmv_frac_moved", "c5_1gpu_cg_iters_per_s",
              "c5_8parts_cg_ms_per_iter_per_part", "c5_allreduce_1rank_ms", "c5_model_8gpu_speedup",
              "ceiling_copy_600MiB_GBs", "ceiling_copy_7600MiB_GBs", "pcg3162_ildu_reorder_over_cg"]
    assert list(bench.FLAT_HEAD) == wanted
    assert 6 + len(wanted) == bench.DRIVER_KEEPS_ROOFLINE_SCALARS
    assert all(len(k) <= 40 for k in wanted)
    # a dry line: every leg present, with more keys than the record holds
    cg = {"iters_per_s": 1.0, "ms_per_iter": 1.0, "frac_of_hbm_peak": 0.5, "effective_GBs_on_survey_floor": 1.0}
    c5 = {"spmv_ms": 1.0, "spmv_frac_of_hbm_peak": 0.5, "cg_iters_per_s": 1.0, "cg_frac_of_hbm_peak": 0.5, "spmv_GB/s_moved": 1.0}
    c5p = {f"c5_8parts_{k}": 1.0 for k in ("spmv_ms", "cg_ms_per_iter", "cg_ms_per_iter_per_part", "cg_ms_per_iter_mode0",
                                           "products_ms_per_part", "halo_ms_per_part", "dot_reduce_ms_per_part")}
    c5p.update({"c5_1part_cg_ms_per_iter": 1.0, "c5_allreduce_1rank_ms": 0.005, "c5_model_8gpu_speedup": 7.0,
                "c5_model_8gpu_cg_iters_per_s": 1.0, "c5_model_8gpu_speedup_ar30us": 6.6, "model_note": "x", "parts": 8})
    ceil = {"flat": {f"ceiling_{k}_{m}MiB_GBs": 1.0 for k in ("copy", "read", "mix8r1w") for m in (600, 7600)}}
    c3 = {"spmv_ms": 1.0, "frac_moved": 0.5, "layout_compression": 1.0, "bicgstab": {"iters_per_s": 1.0, "frac_moved": 0.5},
          "gmres30": {"iters_per_s": 1.0, "frac_moved": 0.5}}
    c4 = {"spmv_ms": 1.0, "frac_moved": 0.5, "frac_survey_bytes": 0.2, "product_bit_exact": True}
    leg = {"cg": {"setup_s": 0.0, "solve_s": 1.0}, "ildu0_natural_order": {"setup_s": 0.0, "solve_s": 1.0},
           "ildu0_colour_order": {"ordering_s": 0.0, "permutation_s": 0.0, "setup_s": 0.0, "solve_s": 1.0},
           "ildu0_reorder_inside_the_preconditioner": {"setup_s": 0.0, "solve_s": 1.0, "total_s_over_plain_cg_s": 0.8}}
    flat = bench.flat_roofline_keys(1, cg=cg, c5=c5, c5p=c5p, ceilings=ceil, c3=c3, c4=c4,
                                    pcg={"grid_1000": leg, "grid_3162": leg}, achieved=6000.0, moved_rank=6e8, k_cold=1e-4,
                                    in_solver_ms=0.1)
    assert list(flat)[:18] == wanted, list(flat)[:18]
    assert len(flat) > 18 and "c5_model_8gpu_speedup_ar30us" in flat and "model_note" not in flat
    assert all(isinstance(v, (int, float, bool)) for v in flat.values())
    # N = 8: what the 8 ranks measured leads the line
    flat8 = bench.flat_roofline_keys(8, cg=cg, c5=c5, moved_rank=6e8, k_cold=1e-4)
    assert list(flat8)[:4] == ["c5_8gpu_spmv_ms", "c5_8gpu_spmv_frac_moved", "c5_8gpu_cg_iters_per_s", "c5_8gpu_cg_frac_moved"]
    assert "c2_cg_iters_per_s" in list(flat8)[:8]


def test_every_test_name_quoted_in_the_docs_exists():
    """DESIGN.md / INTEGRATION.md / README.md / CHANGELOG.md / profiles/*/README.md cite tests by name as evidence (r05's
    INTEGRATION.md cited one that did not exist): every `test_*` word in them is a test function or a test file of tests/."""
    import glob
    funcs, files = set(), set()
    for f in glob.glob(os.path.join(ROOT, "tests", "*.py")):
        files.add(os.path.basename(f)[:-3])
        funcs |= set(re.findall(r"^\s*def (test_[A-Za-z0-9_]+)", open(f).read(), flags=re.M))
    docs = [os.path.join(ROOT, n) for n in ("DESIGN.md", "INTEGRATION.md", "README.md", "CHANGELOG.md")]
    docs += glob.glob(os.path.join(ROOT, "profiles", "*", "README.md")) + [os.path.join(ROOT, "include", "sigma_hip.h")]
    missing = {}
    for d in docs:
        if not os.path.exists(d):
            continue
        quoted = set(re.findall(r"\b(test_[a-z0-9_]+)\b", open(d).read()))
        bad = sorted(q for q in quoted if q not in funcs and q not in files)
        if bad:
            missing[os.path.relpath(d, ROOT)] = bad
    assert not missing, missing
