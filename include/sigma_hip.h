/*
 * sigma_hip.h -- C ABI of the MI355X-native SpMV + Krylov path for SiGMA.
 *
 * This is the drop-in boundary.  The reference (danshapero/sigma) has
 * no usable FFI for this path: src/wrapper.f90 is dead code that wraps graph edits only
 * (src/wrapper.f90:100-303, excluded at src/CMakeLists.txt:39-40).  What the Fortran
 * host binds with ISO_C_BINDING is therefore the set of type-bound procedures that make
 * up the path; every entry point below names the one it replaces.  Conventions follow
 * src/wrapper.f90: opaque handles (type(c_ptr)), `integer(c_int), value` scalars, and
 * index arrays are handed over EXACTLY as the Fortran holds them -- 1-based int32
 * (src/graph/formats/cs_graphs.f90:16, src/graph/formats/ellpack_graphs.f90:14) --
 * conversion to the device layout is this library's job.
 *
 * Errors: the reference prints and calls exit(1) (src/solver/cg_solvers.f90:61-65).
 * Here every function returns an int status (0 = ok) and sgm_last_error() holds the
 * message; sigma_amd/fortran/sigma_hip.f90 turns nonzero into print + exit(1).
 *
 * `where` arguments say where the caller's arrays live: SGM_HOST (copied across PCIe
 * inside the call) or SGM_DEVICE (HBM pointers, e.g. from sgm_malloc or a torch tensor).
 * All calls are synchronous on return unless sgm_set_async(1) was called.
 * Not thread-safe (the reference is single-threaded); one process drives one GPU.
 */
#ifndef SIGMA_HIP_H
#define SIGMA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sgm_mat_s *sgm_mat;       /* class(sparse_matrix_interface) leaf: csr_matrix / ellpack_matrix */
typedef struct sgm_pc_s *sgm_pc;         /* class(linear_solver) used as preconditioner: jacobi / ldu      */
typedef struct sgm_solver_s *sgm_solver; /* class(linear_solver): cg / bicgstab / gmres                    */
typedef struct sgm_comm_s *sgm_comm;     /* row-partition communicator (RCCL over xGMI); no reference analogue */

enum {
    SGM_OK = 0,
    SGM_ERR_BAD_ARG = 1,
    SGM_ERR_DIMS = 2,          /* non-square matrix handed to a solver: cg_solvers.f90:61-65 */
    SGM_ERR_HIP = 3,
    SGM_ERR_RCCL = 4,
    SGM_ERR_NOT_CONVERGED = 5, /* only when a max_iter extension is set and hit */
    SGM_ERR_NO_DEVICE = 6,
    SGM_ERR_ALLOC = 7,
    SGM_ERR_UNSUPPORTED = 8
};
enum { SGM_HOST = 0, SGM_DEVICE = 1 };
enum { SGM_FMT_CSR = 1, SGM_FMT_ELL = 2, SGM_FMT_COMPOSITE = 3 };
enum { SGM_SOLVER_CG = 1, SGM_SOLVER_BICGSTAB = 2, SGM_SOLVER_GMRES = 3, SGM_SOLVER_MINRES = 4, SGM_SOLVER_LSQR = 5 };
/* why an LSQR solve ended (sgm_lsqr_info): the iteration cap, rnorm <= tolerance, arnorm <= normal_tolerance, a NaN */
enum { SGM_LSQR_STOP_CAP = 0, SGM_LSQR_STOP_RESIDUAL = 1, SGM_LSQR_STOP_NORMAL = 2, SGM_LSQR_STOP_NAN = 3 };
enum { SGM_PC_JACOBI = 1, SGM_PC_ILDU0 = 2 };
#define SGM_PC_MG 3        /* multigrid V-cycle: made by sgm_mg_create (it needs its prolongations), not by sgm_pc_create */

/* ---- runtime -------------------------------------------------------------------- */
int sgm_init(int device);                 /* hipSetDevice + stream; fails loudly without a GPU */
int sgm_finalize(void);
const char *sgm_last_error(void);
int sgm_set_stream(void *hip_stream);     /* adopt the caller's hipStream_t (NULL = library stream) */
int sgm_set_async(int on);                /* 1: calls return without hipStreamSynchronize */
int sgm_synchronize(void);
/* ---- options ------------------------------------------------------------------------- *
 * Options choose among device formats / kernels / loop structures that all give the SAME bits (the one exception,
 * "dot_order", is spelled out below).  They are PER HANDLE: a matrix, solver or preconditioner copies the process-wide
 * defaults when it is created and keeps its own copy from then on --
 *     sgm_set_option(name, v)            the default that handles created LATER start with (touches no existing handle)
 *     sgm_mat_set_option(A, name, v)     this matrix      (composite: every block; A^T follows A)
 *     sgm_solver_set_option(s, name, v)  this solver      (read at the next solve)
 *     sgm_pc_set_option(pc, name, v)     this preconditioner
 * -- so two handles of one process may run different kernels, and no caller can change another caller's solver.
 * Unknown names, or a name of the wrong group, are SGM_ERR_BAD_ARG.
 *
 * Matrix options
 *   "csr_offset_dict" (1)  CSR matrices whose column-minus-row offsets take <= 255 distinct values (every stencil / banded
 *                          matrix) hold their columns as 1-byte dictionary codes: 9 instead of 12 bytes per entry; 0 = int32 kernels
 *   "ell_offset_dict" (1)  the same for ELLPACK matrices with max_d <= 16
 *   "csr_sliced" (1)       rows of <= 8 entries from <= 15 offsets (1-D / 2-D / 3-D stencils): values in slices of 512 rows,
 *                          slot-major, one 32-bit word of 4-bit codes per row, a lane owns two adjacent rows, no row pointers
 *                          read (8 W + 4 bytes per row of width W; k_csr_sl).  Its siblings for rows of 9..32 entries with a
 *                          dictionary (k_csr_slb) and for <= 32 similar-length entries at arbitrary columns (k_csr_sl32)
 *   "csr_row_owner" (1)    int32-column matrices with rows <= 64 entries: row-owner gather kernel; 0 = kernels for longer rows
 *   "csr_row_lines" (1)    longer rows of similar length (mean >= 16, none beyond 4096 or 4 x the mean): line-staged row-owner
 *                          kernel; 0 = the balanced streaming-gather kernel (any row length)
 *   "csr_sell" (1)         general matrices whose rows are too long / uneven for the uniform sliced form: SELL-128-512 (rows of
 *                          every 512-row window sorted by length, chunks of 128 rows slot-major with the chunk's own width),
 *                          taken from a longest row of 49 entries on; 2 = whenever the padding allows; 0 = the CSR kernels
 *   "csr_xwindow" (1)      the SELL form of a BANDED matrix (every 512-row slice gathers from a window of x that fits 144 KiB of
 *                          LDS, and re-uses it): the slice's window is staged in LDS with coalesced loads and every gather is an
 *                          LDS read, instead of one 128-byte line moved L2 -> L1 per 8-byte gather; 0 = gathers from L2
 *   "csr_lean" (1)         a matrix served by the sliced / SELL form keeps ONLY that form (+ row pointers) in HBM (C2: 0.48
 *                          instead of 1.13 GB); its CSR-order arrays are rebuilt on the device for whoever reads them
 *   "ell_colblock" (1)     ELLPACK matrices -- and CSR matrices with rows of similar length -- whose columns have no locality
 *                          (x >= 7 MiB, >= 8 slots per row, no offset dictionary): column-blocked two-phase product (products
 *                          through LDS-resident x blocks, then ordered row sums); 0 never, 2 always
 *   "ell_colblock_cols" (16384 = 128 KiB of LDS, the maximum)  x entries per block
 *   "ell_colblock_rows" (0 = automatic; 256 or 512)  rows per tile of the second phase
 *   "coloring_pass" (0)    sgm_graph_greedy_coloring / _greedy_color_order on this matrix's graph: 0 = the fastest pass that
 *                          applies (parities by union-find on the device, level sweep on the device, the reference's sequential
 *                          pass on the host), 1 = from the level sweep on, 2 = the host pass; the same colours whichever
 *   "slice_sched" (0)      sliced matrices most of whose rows carry a far offset (the plane stride of a 3-D grid): the slices
 *                          are handed to the XCDs tile by tile -- the plane is cut into bands (1 = of 64 slices, n > 1 = of n
 *                          slices), XCD x sweeps bands x, x + 8, ... plane after plane, so that the three planes a band reads
 *                          share ONE XCD's L2.  464^3: fabric reads 9.9 -> 8.6 GB per product with bands of 64, 7.1 GB
 *                          with bands of 8 -- and the time stays within run-to-run noise (the re-fetched planes were
 *                          Infinity-Cache hits; profiles/r04/c5_slice_sched_sweep.txt), hence off; only the ORDER of whole slices changes
 * Solver options
 *   "cg_small" (1)         CG (plain / Jacobi) with the WHOLE SOLVE in one launch: on a single-GPU matrix of <= 10240 rows
 *                          (stencil; 4096 otherwise) and <= 49k stored slots as ONE workgroup -- p in LDS, x and r in
 *                          registers --; on a larger stencil matrix, up to 256 x 4096 rows, as up to 256 co-resident workgroups
 *                          (one per CU) that own 1024..4096 rows each and meet twice per iteration through sc1 stores / polls
 *                          (k_cg_coop: n = 1e6 17.7 instead of 36 us per iteration, n = 1e5 10.7 instead of 13.0); every wait
 *                          is bounded, a hand-off that gives up hands the solve to the launch loop.  A launch runs at most
 *                          50000 iterations (n > 1: at most n) and the solve continues in the next one from parked r, p,
 *                          res2, bit-identical to the uncut solve; 0 = the launch loop (three kernels per iteration)
 *   "bicgstab_small" (1)   the same for BiCGStab (one workgroup <= 4096 rows; the cooperative kernel k_bicg_coop beyond, for
 *                          the systems the cooperative CG kernel takes)
 *   "krylov_graph" (1)     the CG / BiCGStab launch loops on one GPU (plain / Jacobi) go on as replays of ONE captured group
 *                          of 16 iterations (a hipGraph) once a solve has run 64 iterations (n > 1: n, rounded up to a
 *                          multiple of 16); 0 = launch every kernel
 *   "gmres_cgs2" (1)       how GMRES orthogonalises: 1 = classical Gram-Schmidt applied twice in its low-synchronisation form --
 *                          the stored basis vector is the ONCE-projected one and the second projection lives in the Cholesky
 *                          factor R of the stored columns' Gram matrix (V = S R^-1 never formed; H = R Gs R^-1): the basis is
 *                          read twice per step and two reductions (all-reduces) are taken, 2 k + 3 vector passes at basis
 *                          size k; 0 = modified Gram-Schmidt (k + 2 dependent passes and reductions, 4 k + 8 vector passes),
 *                          the checker.  (Round 4's blocked CGS-2 with the second projection applied -- three passes, three
 *                          reductions -- was 1265 it/s on C3 against 1644 and is gone.)
 *   "dot_order" (0)        how CG / BiCGStab / MINRES / LSQR add up their dot products.  0 = tree order (per-workgroup partial sums,
 *                          re-reduced in a fixed order): a legal order for the Fortran intrinsic, deterministic, the fast one.
 *                          1 = the order the reference build uses (amdflang -O2 turns dot_product into ONE accumulator fed
 *                          first element to last, cg_solvers.f90:131,135,140): every iterate, iteration count and residual is
 *                          then BIT-IDENTICAL to the reference's, also on row partitions and across ranks; about 4 ns per
 *                          element -- a VALIDATION mode for n up to ~1e5.  MINRES (no reference counterpart) takes the same
 *                          one-accumulator order with 1, which makes its whole solve deterministic down to the bit
 *                          (sgm_minres_create states every operation).  GMRES (no reference counterpart) keeps the tree order
 *   "coop_spin_limit" (0 = built-in, 2^19 polls)  how often a hand-off of the cooperative CG / BiCGStab kernels polls before
 *                          it gives up (the launch loop then takes the solve from the caller's x); tests set 1 to force that path
 *   "cg_coop_variant" (0)  which cooperative kernel serves a system, all the same statements: low four bits = rows per thread
 *                          pinned (1, 2, 4 or 8; 0 = by size), + 16 = never the variant that keeps a small system on one XCD
 *   "reorder_solve" (2)    with a preconditioner that factorised the colour-ordered matrix ("ildu_reorder"): 2 = the whole solve
 *                          runs in that order (x, b permuted once each way, products on P A P^T) and CG folds its r update and
 *                          r.z into the two sweeps; 1 = that order, separate steps; 0 = r and z permuted around every apply
 *   "dist_halo_fused" (1)  CG on a row partition (ranks or in-process parts): the boundary rows of r (z with a preconditioner)
 *                          travel in the same step as the all-reduce of r.r (r.z) -- over RCCL ONE ncclGroup holding the
 *                          send / recv pairs and the all-reduce -- and every part forms its halo copy of p itself by the owner's
 *                          statement p = r + beta p (cg_solvers.f90:142): the product starts without an exchange and without a
 *                          wait for one.  Same operands, same statement: the same bits as exchanging p.  2 = the send / recv
 *                          group on its own just before the all-reduce; 0 = p's halo exchanged in front of every product
 *                          (on the communication stream, overlapped with the interior rows)
 * Preconditioner options
 *   "ildu_strips" (1)      ILDU(0) factors of grid-like matrices use the strip- / slab-pipelined triangular solves; 0 = the
 *                          level-scheduled walkers
 *   "ildu_rows" (1)        ILDU(0) factors of <= 32 levels (what a colour ordering leaves) are swept in row space, one launch
 *                          per level on the vectors themselves; 2 = every level launched (1 skips two); 0 = the walkers
 *   "pipeline_spin_limit" (0 = built-in, 2^22 polls)  how often a wait inside the pipelined sweeps polls before it gives up
 *                          (a sweep that gives up is redone with the walkers and the pipeline retired for that handle:
 *                          sgm_pc_get "pipeline_retired"); tests set 1 to force that path
 *   "ildu_reorder" (0)     1 = the preconditioner is ILDU(0) of the COLOUR-ORDERED matrix P A P^T (P = the reference's
 *                          greedy_color_ordering of A's graph, permutations.f90:162-205; on the device for bipartite graphs such
 *                          as the 5- / 7-point grids); sgm_pc_apply is z = P^T M^-1 P r.  Its factors have one dependency level per
 *                          colour whatever order A is in, so an apply is a few bandwidth-bound launches instead of a
 *                          dependency chain of nx + ny levels.  The caller keeps A, b, x as they are; the preconditioner keeps
 *                          P A P^T, and sgm_solver_solve -- handed the matrix the preconditioner was set up with, unchanged
 *                          since -- runs the whole solve in that order (x, b permuted once each way).  A different
 *                          (equally valid) preconditioner than ILDU(0) in A's own order: iteration counts are those of the
 *                          permuted system -- off by default because the reference's `ldu()` factors A in the given order
 * Multigrid preconditioners take one more name, through sgm_pc_set_option only (SGM_ERR_BAD_ARG on another kind; it is no
 * process-wide default): "mg_coarse_direct", default 0; 1 = the coarsest level is inverted at the next sgm_pc_setup and every
 * V-cycle applies the inverse in place of the coarse sweeps (at most SGM_MG_DIRECT_MAX_ROWS rows; see sgm_mg_create below).
 * Like "ildu_reorder" it selects a different preconditioner, not another kernel for the same bits.
 * Process-wide (sgm_set_option only)
 *   "dist_force_collectives" (0)  1 = a matrix distributed over ONE rank still issues its all-reduces (the fixed cost of the
 *                          RCCL code path, measurable on a single-GPU box: bench.py's `dist_overhead_1rank`)          */
int sgm_set_option(const char *name, int value);
int sgm_mat_set_option(sgm_mat A, const char *name, int value);
int sgm_solver_set_option(sgm_solver s, const char *name, int value);
int sgm_pc_set_option(sgm_pc pc, const char *name, int value);
/* The schedule itself, host-only (no HIP call; what the library uploads for a row range of n_slices
 * 512-row slices): tab_out[it * grid + workgroup] = slice or -1, iters_out = entries per workgroup.
 * tab_out may be NULL to ask for iters_out only; capacity in entries (>= iters * grid).          */
int sgm_slice_sched_host(int64_t n_slices, int64_t period_rows, int32_t grid, int32_t band_slices,
                         int32_t *tab_out, int64_t capacity, int32_t *iters_out);
/* sgm_heartbeat: where the thread that drives the library is right now -- callable from ANOTHER host thread while that one
 * is blocked in a synchronisation or a collective (bench.py's watchdog: a multi-GPU run that hangs says where).
 * out6 = {phase code, beats (bumped at every phase change and solver batch), iterations the running solve has queued,
 * halo exchanges posted, all-reduces posted, solver calls entered}; phase_name (optional) receives the phase in words.
 * Two ranks stuck with different post counts name the rank that fell behind.  No HIP call; never blocks.              */
int sgm_heartbeat(int64_t *out6, char *phase_name, int len);
int sgm_malloc(void **p, size_t bytes);   /* HBM buffer for hosts without a device allocator */
int sgm_free(void *p);
int sgm_memcpy(void *dst, const void *src, size_t bytes, int kind); /* 0 h2d, 1 d2h, 2 d2d */

/* ---- matrices -------------------------------------------------------------------- *
 * sgm_csr_create    <- csr_matrix: g%ptr(n+1), g%node(nnz), val(nnz)
 *                      src/matrix/formats/cs_matrices.f90:32-38,112-151; cs_graphs.f90:16
 * sgm_ell_create    <- ellpack_matrix: g%node(max_d,n), val(max_d,n) column-major,
 *                      padding = last neighbour / 0.0
 *                      src/matrix/formats/ellpack_matrices.f90:28-33; ellpack_graphs.f90:14,164
 * sgm_*_set_values  <- re-upload after host-side set_value/add_value
 *                      (test/solver_test_jacobi.f90:240-274 edits A, then re-runs setup)
 * sgm_mat_matvec    <- A%matvec(x,y): y = 0 ; matvec_add
 *                      src/linear_operator/linear_operator_interface.f90:185-194
 * sgm_mat_matvec_add<- csr_matvec_add cs_matrices.f90:600-622 /
 *                      ellpack_matvec_add ellpack_matrices.f90:640-665
 * sgm_mat_destroy   <- A%destroy()
 * Results are bit-identical to the reference loops: per row, products are rounded
 * individually and added left to right in stored order (no FMA, no reassociation).   */
int sgm_csr_create(sgm_mat *out, int32_t nrow, int32_t ncol, int64_t nnz,
                   const int32_t *ptr_1based, const int32_t *node_1based,
                   const double *val, int where);
int sgm_csr_set_values(sgm_mat A, const double *val, int where);
int sgm_ell_create(sgm_mat *out, int32_t nrow, int32_t ncol, int32_t max_d,
                   const int32_t *node_1based_colmajor, const double *val_colmajor,
                   int where);
int sgm_ell_set_values(sgm_mat A, const double *val_colmajor, int where);
/* ELLPACK degrees.  The reference keeps degrees(n) beside node(max_d,n): the first degrees(i) slots of row i are its entries,
 * the rest is padding.  The products never read it (all max_d slots are summed); everything else does -- get_value / set_value /
 * add_value and edit plans, add_sparse_matrix, the permutations, ILDU(0) and Jacobi setup (get_value scans the first degrees(i)
 * slots and keeps the LAST hit, ellpack_matrices.f90:232-235), sgm_mat_get("degrees").
 *
 * sgm_ell_set_degrees hands the graph's own degrees in (host or device).  Checked before anything reads through them:
 * 0 <= degrees(i) <= max_d and the first degrees(i) slots of row i hold columns of 1..ncol; a violation is SGM_ERR_DIMS and the
 * handle keeps its previous degrees.  On success version and pattern_version move (which slots are entries has changed): an
 * edit plan made before is refused, derived matrices and multigrid levels are rebuilt.
 *
 * Without that call sgm_ell_create recovers degrees from the padding, for three row shapes only:
 *   d distinct nonzero columns, every later slot equal to slot d      (what add_edge / graph_build leave: ellpack_graphs.f90:164,394-397)
 *   all slots 0                                                       (a row without edges; sgm_mat_get("node") gives the 0 back)
 *   d distinct nonzero columns, every later slot 0                    (a caller's zero padding)
 * If any row has another shape (say a column stored twice among a full row's slots) the handle holds NO degrees: the products
 * work as ever, and every reader of degrees named above returns SGM_ERR_UNSUPPORTED with a message that names
 * sgm_ell_set_degrees.
 * LIMIT: the recovered degrees are right only for arrays no delete_edge has touched.  ellpack_delete_edge (ellpack_graphs.f90:
 * 418-481) shifts the row left and copies the second-to-last slot into the last, so deleting the last neighbour of [a,b,c,c,c]
 * (degree 3) leaves [a,b,c,c,c] with degree 2, and deleting the only neighbour of [a,a,a] leaves [a,a,a] with degree 0: rows
 * that no rule can tell from add_edge rows of degree 3 and 1.  Graphs that have seen delete_edge must hand their degrees in. */
int sgm_ell_set_degrees(sgm_mat A, const int32_t *degrees, int where);
int sgm_mat_matvec(sgm_mat A, const double *x, double *y, int where);
int sgm_mat_matvec_add(sgm_mat A, const double *x, double *y, int where);
/* sgm_mat_matvec_dots: test introspection -- y = A x (add = 1: y += A x, not chained, like sgm_mat_matvec_add) launched with
 * the fused dot epilogues exactly as the solvers launch it (CG's p.Ap, BiCGStab's r0.v / t.s / t.t, Lanczos's q.Aq in the
 * default dot order), and the scalars those epilogues leave, per part, as a consumer would see them: every part's partial
 * sums collapsed by the solvers' own reducer (k_reduce = load_scalar: same sum, same order).
 *   w and yy_out: both dots; w (and wy_out) only: w.y; yy_out only (w null): y.y; neither: SGM_ERR_BAD_ARG.
 *   wy_out / yy_out / count_out: HOST arrays, one entry per part (one entry for a single matrix or a composite);
 *   count_out[ip] = the number of partial sums part ip's product leaves per dot.
 * Vectors as for sgm_mat_matvec (w laid out like y), `where` holds for x, y and w.  Single-GPU CSR / ELLPACK matrices,
 * in-process partitions and composites of single-GPU leaves; a matrix on a communicator is SGM_ERR_UNSUPPORTED, and so
 * is w on a non-square matrix (y.y alone is fine there).  The partial arrays are allocated per call and start as NaN.   */
int sgm_mat_matvec_dots(sgm_mat A, const double *x, double *y, const double *w_or_null, int add,
                        double *wy_out_or_null, double *yy_out_or_null, int32_t *count_out_or_null, int where);
/* sgm_mat_matvec_t     <- A%matvec_t(x,y): y = 0 ; matvec_t_add
 *                         src/linear_operator/linear_operator_interface.f90:199-208
 * sgm_mat_matvec_t_add <- csc_matvec_add (the csr transpose kernel) cs_matrices.f90:627-647 /
 *                         ellpack_matvec_t_add ellpack_matrices.f90:670-693
 * x has nrow entries, y has ncol.  The reference scatters y(node(k)) += val(k)*x(j); here an
 * explicit transpose is built on first use so that every y(i) is summed in that same order
 * (bit-identical, no atomics).  On a matrix distributed over processes (sgm_csr_create_dist) the call is
 * collective: A^T is built once as another distributed matrix (every entry travels to the rank owning its
 * column), x = this rank's owned rows, y = its owned columns.  Not available on in-process partitions.   */
int sgm_mat_matvec_t(sgm_mat A, const double *x, double *y, int where);
int sgm_mat_matvec_t_add(sgm_mat A, const double *x, double *y, int where);
/* sgm_mat_matmat: Y = [Y +] op(A) X for a block of k vectors (an extension).
 * Contract -- for every column j < k:
 *   op = 0                          Y(:,j) holds exactly the bits sgm_mat_matvec would leave for x = X(:,j);
 *   op = SGM_OP_ADD                 the bits of sgm_mat_matvec_add;
 *   op = SGM_OP_TRANS [| SGM_OP_ADD] the bits of sgm_mat_matvec_t / sgm_mat_matvec_t_add, i.e. the chained sum over the cached
 *                                   transpose (x length nrow, y length ncol).
 * This holds for every matrix format, every kernel family and every setting of the matrix options; nothing else is promised
 * about order.  X and Y are column-major with leading dimensions ldx and ldy (the layout of the eigensolvers' bases): column
 * j starts at X + j * ldx / Y + j * ldy.  ldx must be at least the product's x length and ldy at least its y length.  Entries
 * of Y between a column's last row and ldy are never written; without the add bit Y is never read; a NaN or Inf in one
 * column of X reaches that column of Y only.
 *   k == 0 is a no-op; k == 1 is the existing single-vector call; k < 0, bits of op other than the two above, a null pointer,
 *   a short leading dimension, or overlapping address ranges of X and Y are SGM_ERR_BAD_ARG (Y untouched).
 *   Host operands are staged as sgm_mat_matvec stages them; a device operand whose columns are not all 16-byte aligned (odd
 *   leading dimension, odd base) is copied to an aligned block first, the rule a single vector is staged by.
 *   Single-GPU CSR and ELLPACK matrices and composites of them are served; in-process partitions and matrices on a
 *   communicator are SGM_ERR_UNSUPPORTED.
 * What runs: the three sliced forms (k_csr_sl's 4-bit codes -- sliced ELLPACK included --, k_csr_slb's 1-byte codes,
 * k_csr_sl32's int32 columns) have native multi-vector kernels (k_mm_sl / k_mm_slb / k_mm_sl32) that read the resident
 * layout once per block of KB columns.  A call is cut, left to right, into blocks of the largest selected width that fits;
 * a last single column goes through the existing product.  With the widths 8, 4 and 2 selected:
 *   k = 2: 2    3: 2 + 1    4: 4    5: 4 + 1    6: 4 + 2    7: 4 + 2 + 1    8: 8    9: 8 + 1    15: 8 + 4 + 2 + 1
 *   16: 8 + 8   17: 8 + 8 + 1   20: 8 + 8 + 4
 * (which widths a form has is a measured decision, profiles/matmat/README.md; sgm_mat_matmat_kernel tells).  Every other
 * layout (k_csr_do, k_csr_rl, k_csr_spmv, SELL, plain ELLPACK, k_ell_do, the column-blocked forms, composites) and a matrix
 * whose slice_sched option is on run the column loop: one existing product per column.
 *
 * sgm_mat_matmat_kernel: what a call would run, without running it (like sgm_mat_kernel), e.g.
 *   "k_mm_sl<W=5,KB=4> x1 + k_mm_sl<W=5,KB=2> x1 + k_csr_sl<W=5> x1", or "columns: k_csr_sell<...>" for the column loop.
 *   (With SGM_OP_TRANS the cached transpose is built if it is not there yet.)
 * sgm_mat_matmat_probe: test introspection -- the same product with the block width capped (block_cap = 1: the column loop;
 *   0 = no cap) and the native kernels' grid capped at grid_cap workgroups (rounded down to a multiple of 8, at least 8;
 *   0 = automatic).  Same bits whatever the caps.                                                                          */
#define SGM_OP_ADD 1
#define SGM_OP_TRANS 2
int sgm_mat_matmat(sgm_mat A, int32_t op, int32_t k, const double *X, int64_t ldx, double *Y, int64_t ldy, int where);
int sgm_mat_matmat_kernel(sgm_mat A, int32_t op, int32_t k, char *buf, int len);
int sgm_mat_matmat_probe(sgm_mat A, int32_t op, int32_t k, const double *X, int64_t ldx, double *Y, int64_t ldy,
                         int32_t block_cap, int32_t grid_cap, int where);
/* sgm_csr_from_edges / sgm_ell_from_edges <- the assembly sequence of the reference's tests
 *   g%add_edge(i,j)... ; convert_graph_type(g, "compressed sparse" | "ellpack") ; A%set_graph(g) ;
 *   A%set_value(i,j,z)...        (test/solver_test_jacobi.f90:73-128)
 * i.e. ll_graphs.f90:355-370 (repeated edges ignored) + cs_graphs.f90:109-197 /
 * ellpack_graphs.f90:105-170 + cs_matrices.f90:840-863 (the last value written wins).
 * The edge list (1-based, INSERTION order) is turned into the same ptr/node/val (or
 * node(max_d,n)/val/degrees) arrays on the device -- bit-identical index work.
 * sgm_mat_get reads a leaf matrix back in the reference's layout: "ptr","node","val" (CSR),
 * "max_d","degrees","node","val" (ELLPACK, (max_d,n) Fortran order); "versions" (either
 * format): three int64 -- the handle's serial number, its version (bumped by every change of
 * its entries or their order) and its pattern_version (bumped by the permutations).      */
int sgm_csr_from_edges(sgm_mat *out, int32_t nrow, int32_t ncol, int64_t ne, const int32_t *ei_1based,
                       const int32_t *ej_1based, const double *ev, int where);
int sgm_ell_from_edges(sgm_mat *out, int32_t nrow, int32_t ncol, int64_t ne, const int32_t *ei_1based,
                       const int32_t *ej_1based, const double *ev, int where);
int sgm_mat_get(sgm_mat A, const char *name, void *out_host, size_t bytes, size_t *needed);
/* ---- sparse matrix algebra (src/matrix/sparse_matrix_algebra.f90:13) ------------------ *
 * sgm_mat_sum     <- sparse_matrix_sum      sparse_matrix_algebra.f90:25-145   A = B + C
 * sgm_mat_product <- sparse_matrix_product  :154-189 -> sparse_matrix_product_C :310-420   A = B * C
 * sgm_mat_ptap    <- PtAP                   :425-538   B = P^T A P
 * sgm_mat_rart    <- RARt                   :543-655   B = R A R^T
 * The result is a new single-GPU CSR leaf (*out), bit-identical to the reference's: the columns of every
 * row in the order of their first contribution (ll_graphs.f90:355-370, cs_graphs.f90:109-197), every
 * value +0.0 plus its terms in contribution order (cs_matrices.f90:868-891), each term a product rounded
 * on its own.  Operands are single-GPU CSR leaves; composite, distributed / partitioned and ELLPACK
 * operands are SGM_ERR_UNSUPPORTED; shapes that do not fit are SGM_ERR_DIMS (the reference exits).
 * The result keeps its symbolic plan (freed by sgm_mat_destroy).  sgm_mat_get(out, "algebra_rows")
 * reads {rows its symbolic pass ran in LDS, rows that took the long-row path}.
 * sgm_mat_algebra_refill(out, X, Y): only the values again, from the operands' current values (the
 * same handles in the same order as at creation, none of the three permuted since; else
 * SGM_ERR_BAD_ARG); bumps out's version like sgm_csr_set_values.                            */
int sgm_mat_sum(sgm_mat *out, sgm_mat B, sgm_mat C);       /* A = B + C   */
int sgm_mat_product(sgm_mat *out, sgm_mat B, sgm_mat C);   /* A = B * C   */
int sgm_mat_ptap(sgm_mat *out, sgm_mat A, sgm_mat P);      /* B = P^T A P */
int sgm_mat_rart(sgm_mat *out, sgm_mat A, sgm_mat R);      /* B = R A R^T */
int sgm_mat_algebra_refill(sgm_mat out, sgm_mat X, sgm_mat Y);
/* ---- editing values on the device (src/matrix/sparse_matrix_interfaces.f90:106-128,378-460) ------ *
 * A batch is m triples (i_t, j_t, z_t), 1-based, processed as if the reference's scalar call were made for t = 1..m:
 * sgm_mat_set_entries     <- A%set_value(i,j,z)   cs_matrices.f90:840-863 / ellpack_matrices.f90:444-470
 * sgm_mat_add_entries     <- A%add_value(i,j,z)   cs_matrices.f90:868-891 / ellpack_matrices.f90:475-500; also
 *                            set / add_multiple_values(is, js, B) (cs_matrices.f90:934-966, ellpack_matrices.f90:538-573)
 *                            as the batch `for k: for l: (is(k), js(l), B(k,l))`, rows outer
 * sgm_mat_get_entries     <- A%get_value(i,j)     cs_matrices.f90:709-724 / ellpack_matrices.f90:220-237: the LAST stored slot
 *                            of row i holding j, +0.0 if there is none (never an error for an absent entry)
 * sgm_mat_zero            <- A%zero()             val = 0.0 over every stored slot, ELLPACK padding included
 * sgm_mat_scalar_multiply <- A%scalar_multiply(alpha)  ellpack_matrices.f90:578-596  val = alpha * val
 * sgm_mat_add_matrix      <- A%add_sparse_matrix(B [, alpha])  sparse_matrix_interfaces.f90:430-460: B's stored entries in
 *                            cursor order (rows ascending, stored order, ELLPACK padding skipped), z = alpha * B_ij rounded
 *                            (alpha NULL: as they are), then added
 * Triple t addresses EVERY stored slot k of row i_t with node(k) == j_t (a row that stores a column twice has both copies
 * edited); an ELLPACK row is scanned over its first degrees(i) slots only, padding keeps its column and stays 0.0.  set: the z
 * of the last triple addressing the slot.  add: ((v + z_a) + z_b) + ... in ascending t, every addition rounded on its own --
 * the reference's bits, signed zeros / Inf / NaN included.  A triple that addresses no stored slot is SGM_ERR_UNSUPPORTED
 * (the pattern is not grown, unlike default_sparse_matrix_kernels.f90:176-229), an index outside the matrix SGM_ERR_DIMS;
 * the message names the smallest such t and its (i, j), and the matrix is unchanged.  `where` covers i, j and z together;
 * m <= INT32_MAX - 4; m = 0 succeeds.  Every edit ends like sgm_csr_set_values (version bumped, kernel layouts refreshed,
 * transpose stale; pattern_version stays).  Single-GPU CSR / ELLPACK leaves; composite, partitioned and distributed handles
 * are SGM_ERR_UNSUPPORTED.
 * sgm_edit_plan_create locates and orders a batch once; sgm_edit_plan_apply takes only new z (the same m values in the same
 * order), mode SGM_EDIT_SET / SGM_EDIT_ADD, optionally after A%zero() (zero_first) -- the re-assembly of a fixed mesh as one
 * pass over the values.  A plan belongs to its matrix: another handle, or the same one after a permutation, is
 * SGM_ERR_BAD_ARG.  sgm_edit_plan_info: out4 = {m, slots addressed, longest chain, stored source indices incl. padding}.
 * sgm_edit_locate_host: the locate step as host-only index work on the reference's CSR arrays (no HIP call): hit_off (m+1
 * offsets), hit_slot (ascending 1-based positions k per triple; NULL = sizing call), needed = hit_off[m], first_missing = the
 * smallest t without a slot or 0.                                                                                          */
typedef struct sgm_edit_plan_s *sgm_edit_plan;
enum { SGM_EDIT_SET = 0, SGM_EDIT_ADD = 1 };
int sgm_mat_set_entries(sgm_mat A, int64_t m, const int32_t *i, const int32_t *j, const double *z, int where);
int sgm_mat_add_entries(sgm_mat A, int64_t m, const int32_t *i, const int32_t *j, const double *z, int where);
int sgm_mat_get_entries(sgm_mat A, int64_t m, const int32_t *i, const int32_t *j, double *z_out, int where);
int sgm_mat_zero(sgm_mat A);
int sgm_mat_scalar_multiply(sgm_mat A, double alpha);
int sgm_mat_add_matrix(sgm_mat A, sgm_mat B, const double *alpha_or_null);
int sgm_edit_plan_create(sgm_edit_plan *out, sgm_mat A, int64_t m, const int32_t *i, const int32_t *j, int where);
int sgm_edit_plan_apply(sgm_edit_plan plan, sgm_mat A, const double *z, int mode, int zero_first, int where);
int sgm_edit_plan_info(sgm_edit_plan plan, int64_t *out4);
int sgm_edit_plan_destroy(sgm_edit_plan plan);
int sgm_edit_locate_host(int32_t nrow, int32_t ncol, const int32_t *ptr_1based, const int32_t *node_1based, int64_t m,
                         const int32_t *i, const int32_t *j, int64_t *hit_off, int32_t *hit_slot, int64_t capacity,
                         int64_t *needed, int64_t *first_missing);
/* sgm_composite_create <- type(sparse_matrix), the block "matrix of matrices"
 *                         src/matrix/sparse_matrix_composites.f90:41-162; matvec_add = loop over
 *                         the blocks `C%matvec_add(x(j1:j2), y(i1:i2))`, :1076-1099 (row blocks
 *                         outer, column blocks inner), matvec_t_add :1104-1127 (column blocks
 *                         outer).  row_ptr/col_ptr are the 1-based block offsets (nrb+1 / ncb+1
 *                         entries); blocks[it*ncb + jt] are leaf handles (NULL = empty block) that
 *                         stay owned by the caller.  The handle works with matvec(_t)(_add) and
 *                         with the unpreconditioned solvers.                               */
int sgm_composite_create(sgm_mat *out, int32_t nrb, int32_t ncb, const int32_t *row_ptr_1based,
                         const int32_t *col_ptr_1based, const sgm_mat *blocks);
int sgm_mat_info(sgm_mat A, int32_t *nrow, int32_t *ncol, int64_t *nnz, int32_t *fmt,
                 int64_t *x_len /* entries matvec reads from x: ncol, or owned+halo when distributed */);
/* ---- re-orderings ------------------------------------------------- *
 * Graph = the matrix's own cs_graph (neighbours of i = the columns of row i in stored order).
 * sgm_graph_bfs_order          breadth_first_search(p, g)   src/graph/permutations.f90:22-78
 *                              p(i) = visiting number from vertex 1, -1 if never reached
 * sgm_graph_greedy_coloring    greedy_coloring(colors, g)   permutations.f90:83-157
 * sgm_graph_greedy_color_order greedy_color_ordering(p, ptrs, num_colors, g)  :162-205
 *                              p(i) = new index when vertices are sorted by colour; ptrs
 *                              (num_colors+1 entries, may be NULL) = first index per colour;
 *                              fails where the reference would index out of bounds (a vertex
 *                              not reachable from vertex 1)
 * Outputs are HOST arrays of nrow int32 (1-based values, like the reference's).  The
 * breadth-first numbering runs on the device (level-synchronous, same FIFO order); so does the
 * colouring (option "coloring_pass": parities by union-find for a bipartite graph, else a level sweep
 * that reproduces the sequential pass's order- and tally-dependent choices; the reference's own
 * sequential pass on the host is the last resort and the checker) -- the same colours whichever.
 * On a CSR matrix DISTRIBUTED OVER RANKS (sgm_csr_create_dist; round 6) the three orderings and the two permutations below are
 * collective: the whole index structure is gathered onto every rank once (one grouped exchange, host memory for the length of the
 * call), the orderings run by the single-GPU passes on every rank (the same p / colours everywhere, arrays of the GLOBAL nrow),
 * left_permute cuts this rank's NEW rows out of the gathered matrix and rebuilds the handle's row block (same row partition, new halo
 * plan), right_permute renames this rank's columns without any exchange; p is the global permutation, the same on every rank.  A
 * setup path for matrices one rank can hold; in-process partitions are refused.
 * sgm_mat_left_permute(A, p)   A%left_permute(p)   cs_matrices.f90:471-478: row i -> row p(i)
 * sgm_mat_right_permute(A, p)  A%right_permute(p)  cs_matrices.f90:483-490: column j -> p(j)
 *                              (ELLPACK handles too: ellpack_matrices.f90:601-632)
 *                              device kernels; entries keep their stored order inside a row, so
 *                              row sums are bit-identical to the reference's permuted matrix.
 *                              Preconditioners set up before a permutation must be set up again. */
int sgm_graph_bfs_order(sgm_mat A, int32_t *p_out);
int sgm_graph_greedy_coloring(sgm_mat A, int32_t *colors_out, int32_t *num_colors);
int sgm_graph_greedy_color_order(sgm_mat A, int32_t *p_out, int32_t *ptrs_out, int32_t ptrs_len,
                                 int32_t *num_colors);
int sgm_mat_left_permute(sgm_mat A, const int32_t *p, int where);
int sgm_mat_right_permute(sgm_mat A, const int32_t *p, int where);
/* name of the SpMV kernel variant the matrix runs with under the current options
 * (diagnostics for benches and tests; e.g. "k_csr_sl<W=5>", "k_csr_do<256,1536,CW=1>") */
int sgm_mat_kernel(sgm_mat A, char *buf, int len);
/* bytes by construction: what the handle keeps in HBM (every layout it holds), and what ONE
 * y = A x moves with the kernel the current options select: that kernel's stored format as it
 * reads it (padded slices, codes, row pointers) + every x entry once + every y entry once.
 * bench.py grades the roofline fraction on matvec_bytes, not on the reference layout's bytes. */
int sgm_mat_footprint(sgm_mat A, int64_t *resident_bytes, int64_t *matvec_bytes);
int sgm_mat_destroy(sgm_mat A);

/* ---- vector statements inline in the solvers (SURVEY §2a "dot", "axpy family") ---- *
 * dot_product(a,b)  cg_solvers.f90:131,135,140 ; y = y + alpha*x  cg_solvers.f90:137-138 */
int sgm_dot(int64_t n, const double *a, const double *b, double *result, int where);
int sgm_axpy(int64_t n, double alpha, const double *x, double *y, int where);

/* ---- preconditioners --------------------------------------------------------------- *
 * sgm_jacobi_create <- jacobi() + jacobi_setup      src/solver/jacobi_solvers.f90:23-63
 * sgm_ildu0_create  <- ldu(incomplete,level=0) + sparse_ldu_setup
 *                      src/solver/ldu_solvers.f90:73-130 (pattern :397-440 and factorization
 *                      :275-387 run on the device -- the reference's statements per row, rows
 *                      of one dependency level side by side --; the factors live in HBM, host
 *                      copies of their values are made for sgm_pc_get only);
 *                      on a row-partitioned matrix: ILDU(0) of each part's diagonal block
 *                      (block-Jacobi, no exchange in the apply; iteration counts differ
 *                      from the one-part factorisation)
 * sgm_pc_create     <- jacobi() / ldu(...) as factories: the object before it has seen a matrix (set options, then setup)
 * sgm_pc_setup      <- pc%setup(A): the first one, or again after the values changed
 * sgm_pc_apply      <- pc%solve(A, z, r): jacobi_solve :68-81 / ldu_solve :160-176
 * sgm_pc_get        <- read back idiag / L,D,U for parity checks ("idiag","Lptr","Lnode",
 *                      "Lval","Uptr","Unode","Uval","D"; 1-based like the reference; with "ildu_reorder" they are
 *                      the factors of P A P^T and "perm" is p, row i of A = row p(i) of that matrix)          */
int sgm_pc_create(sgm_pc *out, int32_t kind /* SGM_PC_JACOBI | SGM_PC_ILDU0 */);   /* the factory alone: no matrix seen yet */
int sgm_jacobi_create(sgm_pc *out, sgm_mat A);
int sgm_ildu0_create(sgm_pc *out, sgm_mat A);
int sgm_pc_setup(sgm_pc pc, sgm_mat A);
int sgm_pc_apply(sgm_pc pc, const double *r, double *z, int where);
int sgm_pc_get(sgm_pc pc, const char *name, void *out_host, size_t bytes, size_t *needed);
/* sgm_pc_info: which sweeps serve part `part` (0 on one GPU) of a preconditioner that has been set up, and what an apply
 * costs -- the reference's `ldu()` (ldu_solvers.f90:73-86) factors A in the order it is given, and on a naturally ordered grid
 * the triangular solves of ldu_solve (:160-176, row recurrences :227-236, :254-263) are a dependency chain of nx + ny levels:
 * correct, the reference's semantics, and 50-100 x below the HBM roofline.  This says so BEFORE the solve:
 *   out4[0], out4[1]  dependency levels of L, of U        out4[2]  path: 0 diagonal scaling, 1 row-space sweeps (bandwidth-
 *   bound), 2 strip pipeline, 3 slab pipeline, 4 level walkers        out4[3]  colours of the ordering (0 = A's own order)
 *   est_us  estimated microseconds per apply               path_name  e.g. "strip pipeline, 6323 levels", "row space, 2 levels";
 *   with a colour ordering, followed by "; product of the ordered part: k_csr_sl<W=5>" -- the SpMV kernel of the permuted copy
 * With SGM_TRACE set every sgm_pc_setup prints the same line on stderr.  The remedy for a chain: ldu(reorder = "colour")
 * (option "ildu_reorder"), INTEGRATION.md. */
int sgm_pc_info(sgm_pc pc, int32_t part, int32_t *out4, double *est_us, char *path_name, int len);
int sgm_pc_destroy(sgm_pc pc);

/* ---- multigrid preconditioner (an extension: the reference has PtAP / RARt "for multigrid setup" and no multigrid) ---- *
 * sgm_mg_create: one V-cycle on Galerkin levels with damped Jacobi sweeps.  P[l] (l = 0 .. ncoarse-1, borrowed: they must
 * outlive the preconditioner) is the n_l x n_{l+1} CSR prolongation of level l; ncoarse = 0 is the coarse sweeps on A alone.
 * sgm_pc_setup(pc, A) builds A_{l+1} = P_l^T A_l P_l with sgm_mat_ptap (owned by the preconditioner), the inverse diagonals
 * (the Jacobi setup's rule) and the work vectors; a second setup with the same handles and unchanged patterns refills the
 * levels through sgm_mat_algebra_refill, anything else rebuilds them.  z = M^-1 r is vcycle(0, r), every operation rounded
 * on its own, row sums as sgm_mat_matvec forms them:
 *   first sweep of a level (zero start)   x(i) = omega * (idiag(i) * b(i))
 *   further sweeps, out of place          q = A_l x ; t(i) = b(i) - q(i) ; x'(i) = x(i) + omega * (idiag(i) * t(i))
 *   coarsest level                        coarse_sweeps sweeps
 *   other levels                          nu_pre sweeps ; r = b - A_l x ; b_c = sgm_mat_matvec_t(P_l, r) ; x_c = vcycle(l+1, b_c) ;
 *                                         sgm_mat_matvec_add(P_l, x_c, x) ; nu_post sweeps
 * nu_pre >= 1, nu_post >= 0, coarse_sweeps >= 1 (SGM_ERR_BAD_ARG otherwise).  With nu_pre == nu_post, A symmetric positive
 * definite and 0 < omega * lambda_max(D^-1 A) < 2 the operator is symmetric positive definite (usable inside CG); the
 * library does not check this.  Setup refuses with SGM_ERR_DIMS when A is not square or the row counts of the P_l do not
 * chain, with SGM_ERR_UNSUPPORTED (naming the level) for ELLPACK, composite, partitioned or distributed A or P; after a
 * refused setup the handle can only be set up again or destroyed.
 * sgm_pc_info: out4 = {levels, levels, 5, 0}, path_name e.g. "V(1,1) omega 0.8, 7 levels, 8 coarse sweeps".
 * sgm_pc_get: "mg_paths" (int32 per level: 1 = sweeps fused on the 4-bit sliced form, 2 = fused on the 1-byte sliced form (rows of up to 9 or 27 entries),
 * 0 = product + elementwise pass), "mg_idiag_<l>" (the inverse diagonal of level l).
 * sgm_mg_level_matrix: A_level after setup (level 0 = the caller's A), borrowed: do not destroy it.
 *
 * Direct coarse solve: sgm_pc_set_option(pc, "mg_coarse_direct", 1) -- default 0, read at the next
 * sgm_pc_setup, SGM_ERR_BAD_ARG on a preconditioner of another kind.  Setup then inverts the coarsest level A_L on the
 * device by dense Gauss-Jordan elimination with partial pivoting, and every V-cycle replaces the coarse sweeps by the one
 * dense product x = Ainv b (with no prolongation at all the preconditioner is A^-1 itself):
 *   D(i,j) = +0.0 plus the stored copies of (i,j) in stored order; W = [D | I]; for k = 0 .. n-1:
 *     p = the smallest i >= k that maximises fabs(W(i,k)) (a NaN counts as the largest); piv(k) = p + 1; rows k and p swapped;
 *     W(k,j) = W(k,j) / W(k,k) (the divisor taken first); every i != k: f = W(i,k), W(i,j) = W(i,j) - (f * W(k,j))
 *   Ainv = the right block.  x(i) = +0.0 plus s_0(i), s_1(i), ... where s_c(i) = +0.0 plus the individually rounded products
 *   Ainv(i,j) * b(j) of the columns 256c .. 256c+255 in ascending j.
 * Setup refuses with SGM_ERR_UNSUPPORTED when A_L has more than SGM_MG_DIRECT_MAX_ROWS rows (the message gives both numbers)
 * and when a pivot W(p,k) is 0, NaN or +-Inf ("singular or non-finite coarse level", the message names the 1-based step).
 * sgm_pc_get: "mg_coarse_inverse" (n * n doubles, row-major), "mg_coarse_pivots" (n int32, 1-based); both SGM_ERR_BAD_ARG
 * when the last successful setup ran without the option ("mg_coarse_invert_ms": one double, the time of the last inversion).  sgm_pc_info: path_name ends with "direct coarse solve (1297 rows)"
 * in place of "8 coarse sweeps".  A second setup inverts again; the option may change between setups.                      */
#define SGM_MG_DIRECT_MAX_ROWS 4096   /* a 128 MiB inverse, plus twice that as elimination workspace during setup */
int sgm_mg_create(sgm_pc *out, int32_t ncoarse, const sgm_mat *P /* ncoarse handles, borrowed */,
                  double omega, int32_t nu_pre, int32_t nu_post, int32_t coarse_sweeps);
int sgm_mg_level_matrix(sgm_pc pc, int32_t level, sgm_mat *borrowed);   /* A_level after setup; level 0 = the caller's A */

/* ---- algebraic coarsening: the prolongations of sgm_mg_create from A alone (an extension, as the multigrid is) ---------- *
 * Smoothed aggregation on a distance-2 maximal independent set, a contract with one right answer (DESIGN.md section 9d;
 * restated in tests/aggregate_restated.py).  Indices below are 0-based; the arrays at the boundary are 1-based.
 *   diagonal     d(i) = the LAST stored copy of a_ii (the Jacobi setup's rule), 0.0 when absent
 *   strength     a stored entry a of row i in column j != i is strong when a*a >= (theta*theta) * (fabs(d(i)) * fabs(d(j))),
 *                every product rounded on its own; a NaN on either side: not strong.  N(i) = the set of j with a strong
 *                stored copy of (i,j) or of (j,i)
 *   keys         h = (uint32)i * 0x9E3779B1; h ^= h >> 15; h *= 0x85EBCA6B; h ^= h >> 13; h *= 0xC2B2AE35; h ^= h >> 16;
 *                key(i) = ((uint64)h << 32) | (i + 1)
 *   roots        the set R with: i in R <=> no j at distance 1 or 2 from i (in N) with key(j) > key(i) is in R -- the
 *                greedy maximal independent set of the squared graph in descending key order.  Empty N(i): a root
 *   numbering    roots are numbered 1..nagg in ascending row index
 *   membership   a root is its own aggregate; phase 1: a non-root with a root in N(i) joins the root of largest key;
 *                phase 2: every other vertex joins the aggregate of the largest-key member of N(i) that is a root or was
 *                placed in phase 1
 *   T            n x nagg, row i holds the one entry (agg(i), 1.0)
 *   P            smooth_omega == 0: T.  Otherwise W = sgm_mat_product(A, T), every stored value w of W's row i replaced
 *                by (-(smooth_omega * idiag(i))) * w with idiag(i) = 1.0 / d(i), or 0.0 when d(i) == 0, and
 *                P = sgm_mat_sum(T, W): T's entry first in every row
 *   hierarchy    A_0 = A; while levels < max_levels and n_l > min_coarse: aggregate A_l; stop without adding a level when
 *                nagg >= n_l; otherwise emit P_l and form A_{l+1} = sgm_mat_ptap(A_l, P_l).  *ncoarse = 0 is a valid result
 * sgm_mat_aggregate writes agg_out[i] in 1..*nagg for every row (n entries, host or device by `where`).
 * sgm_mg_aggregation_hierarchy returns P_0 .. P_{*ncoarse-1}, new single-GPU CSR matrices the caller owns (sgm_mat_destroy;
 * they do not depend on A's lifetime); P_out has max_levels-1 slots.  The intermediate A_l are destroyed inside the call
 * (sgm_pc_setup builds them again).
 * Refusals: SGM_ERR_DIMS when A is not square; SGM_ERR_UNSUPPORTED for ELLPACK, composite, partitioned or distributed A;
 * SGM_ERR_BAD_ARG for theta negative or NaN, smooth_omega negative, NaN or infinite, max_levels < 1, min_coarse < 1, null
 * outputs.  A refused call creates nothing.  A is never modified (its cached transpose may be built).
 * With SGM_TRACE set the hierarchy prints one line per level on stderr: sizes, rounds and the time of every stage.        */
int sgm_mat_aggregate(sgm_mat A, double theta, int32_t *agg_out, int32_t *nagg, int where);
int sgm_mg_aggregation_hierarchy(sgm_mat A, double theta, double smooth_omega, int32_t max_levels, int32_t min_coarse,
                                 sgm_mat *P_out, int32_t *ncoarse);

/* ---- solvers ------------------------------------------------------------------------ *
 * sgm_cg_create       <- cg(tolerance)            src/solver/cg_solvers.f90:36-47
 * sgm_bicgstab_create <- bicgstab(tolerance)      src/solver/bicgstab_solvers.f90:37-48
 * sgm_gmres_create    <- NO reference counterpart; GMRES(restart), Arnoldi by low-synchronisation
 *                        classical Gram-Schmidt with re-orthogonalisation (CGS-2: the basis read twice, two
 *                        reductions per step; option "gmres_cgs2" = 0: modified Gram-Schmidt), Givens
 *                        rotations; same tolerance / iterations conventions as cg
 * sgm_minres_create   <- NO reference counterpart; preconditioned MINRES (Paige-Saunders) for SYMMETRIC A, definite or not,
 *                        and a symmetric positive definite preconditioner M (neither property is checked): one product per
 *                        step, seven work vectors whatever the step count, a residual norm that never increases.  Single-GPU
 *                        CSR, ELLPACK and composite matrices, every preconditioner kind or none; sgm_solver_setup refuses
 *                        row-partitioned and distributed matrices with SGM_ERR_UNSUPPORTED.  The contract (DESIGN.md 9f;
 *                        tests/minres_restated.py restates it) -- every operation rounded on its own, `A u` the library's
 *                        product (0.0 + row sum in stored order), `a.b` the solver's dot product (tree order; ONE accumulator
 *                        fed first element to last with option "dot_order" = 1, and then every bit of the solve is pinned),
 *                        `M^-1 u` a copy without a preconditioner:
 *                            r1 = b - A x ; y = M^-1 r1 ; beta1 = sqrt(r1.y)
 *                            beta1 == 0: return (0 iterations, res2 = 0, converged)
 *                            oldb = 0 ; beta = beta1 ; dbar = 0 ; epsln = 0 ; phibar = beta1 ; cs = -1 ; sn = 0
 *                            w = w2 = 0 ; r2 = r1
 *                            while fabs(phibar) > tolerance (and the max_iter cap allows), k = 1, 2, ...:
 *                                s = 1.0/beta ; v(i) = s*y(i)
 *                                y = A v
 *                                k >= 2:  t = beta/oldb ; y(i) = y(i) - t*r1(i)
 *                                alfa = v.y
 *                                t = alfa/beta ; y(i) = y(i) - t*r2(i)
 *                                r1 = r2 ; r2 = y ; y = M^-1 r2
 *                                oldb = beta ; bb = r2.y ; beta = sqrt(bb)
 *                                oldeps = epsln ; delta = cs*dbar + sn*alfa ; gbar = sn*dbar - cs*alfa
 *                                epsln = sn*beta ; dbar = -(cs*beta)
 *                                gamma = sqrt(gbar*gbar + beta*beta) ; gi = 1.0/gamma ; cs = gbar*gi ; sn = beta*gi
 *                                phi = cs*phibar ; phibar = sn*phibar
 *                                w1 = w2 ; w2 = w ; w(i) = ((v(i) - oldeps*w1(i)) - delta*w2(i)) * gi ; x(i) = x(i) + phi*w(i)
 *                                iterations += 1 ; history gets fabs(phibar)
 *                            res2 = phibar*phibar
 *                        Tolerance (ABSOLUTE, on sqrt(res2) = |phibar|, the M^-1-norm of the residual as in cg_solve_pc),
 *                        max_iter, `iterations`, `converged` as for cg; the history holds fabs(phibar), not its square.  beta == 0
 *                        after a step is convergence (sn = 0, phibar = 0).  Ends that are NOT convergence: bb < 0 (M is not
 *                        positive definite) or bb not a number -- at the start or in a step --, gamma == 0, gamma or phibar not
 *                        a number.  The solve stops AT that step: the step is not counted, x keeps the value it had before it,
 *                        the call returns SGM_OK (with or without a cap) and converged = 0; res2 is NaN, or the last
 *                        phibar*phibar for gamma == 0.
 * sgm_lsqr_create     <- NO reference counterpart; LSQR (Paige-Saunders, Golub-Kahan bidiagonalisation): min |A x - b|_2 for a
 *                        RECTANGULAR A (nrow = m, ncol = n, any shape and rank; x has n entries, b has m), optionally damped.
 *                        One product with A and one with A^T per step, four work vectors (u^ of m, v^ and w of n entries, one of
 *                        max(m, n)) beside x, a residual norm that never increases.  Single-GPU CSR and ELLPACK matrices, no
 *                        preconditioner: sgm_solver_setup refuses composite, row-partitioned and distributed matrices and
 *                        sgm_solver_solve a non-null pc (a right preconditioner needs M^-T), both with SGM_ERR_UNSUPPORTED.
 *                        A^T is the cached explicit transpose of sgm_mat_matvec_t -- a SECOND COPY of the matrix in device
 *                        memory, counted by sgm_mat_footprint's resident bytes -- built at setup and given A's current values
 *                        at the start of every solve.  The contract (tests/lsqr_restated.py restates it) --
 *                        every operation rounded on its own, every sqrt(a*a + b*b) exactly that expression (never hypot),
 *                        `A u` the library's product, `A^T u` sgm_mat_matvec_t's (every entry summed in the scatter's order:
 *                        source row ascending, then slot), `a.a` the solver's dot product (tree order; ONE accumulator fed
 *                        first element to last with option "dot_order" = 1, and then every bit of the solve is pinned).
 *                        Neither bidiagonalisation vector is normalised in memory (u^ = beta u, v^ = alpha v):
 *                            u^ = b - A x ; beta = sqrt(u^.u^)              beta == 0: return (0 iterations, stop 1)
 *                            z = A^T u^ ; v^(i) = (1.0/beta)*z(i) ; alpha = sqrt(v^.v^)      alpha == 0: return (0 iterations, stop 2)
 *                            w(i) = (1.0/alpha)*v^(i) ; phibar = beta ; rhobar = alpha ; Psi = 0
 *                            rnorm = beta ; arnorm = alpha*beta ; the two tests below
 *                            step k = 1, 2, ... (while the max_iter cap allows):
 *                                y = A v^ ; u^(i) = (1.0/alpha)*y(i) - (alpha/beta)*u^(i) ; beta' = sqrt(u^.u^)
 *                                beta' != 0:  z = A^T u^ ; v^(i) = (1.0/beta')*z(i) - (beta'/alpha)*v^(i) ; alpha' = sqrt(v^.v^)
 *                                beta' == 0:  alpha' = 0
 *                                damp != 0:   rhobar1 = sqrt(rhobar*rhobar + damp*damp) ; c1 = rhobar/rhobar1 ; s1 = damp/rhobar1
 *                                             psi = s1*phibar ; phibar = c1*phibar ; Psi = Psi + psi*psi
 *                                otherwise    rhobar1 = rhobar
 *                                rho = sqrt(rhobar1*rhobar1 + beta'*beta') ; c = rhobar1/rho ; s = beta'/rho ; theta = s*alpha'
 *                                rhobar = -(c*alpha') ; phi = c*phibar ; phibar = s*phibar
 *                                rnorm = sqrt(phibar*phibar + Psi) (fabs(phibar) with damp == 0)
 *                                arnorm = (fabs(phibar)*alpha')*fabs(c)
 *                                x(i) = x(i) + (phi/rho)*w(i)
 *                                beta' != 0 and alpha' != 0:  w(i) = (1.0/alpha')*v^(i) - (theta/rho)*w(i)
 *                                alpha = alpha' ; beta = beta' ; iterations += 1 ; history gets rnorm ; res2 = rnorm*rnorm
 *                                stop 1 if beta' == 0 ; else stop 2 if alpha' == 0 ; else the two tests:
 *                            tests:  stop 1 if not rnorm > tolerance ; else stop 2 if not arnorm > normal_tolerance
 *                        Both tolerances are ABSOLUTE.  A solve always returns SGM_OK with a stop value (sgm_lsqr_info), except
 *                        at the cap: stop 1 = rnorm <= tolerance, the system is solved as a compatible one; stop 2 = arnorm
 *                        <= normal_tolerance, the least-squares solution (arnorm estimates |A^T r - damp^2 (x - x0)|_2); stop 0
 *                        = the max_iter cap (SGM_ERR_NOT_CONVERGED, as for cg); stop 3 = u^.u^ or v^.v^ negative or not a number,
 *                        or rho or the new phibar not a number -- that step stores nothing: it is not counted and x keeps the
 *                        last finished iterate (res2 is NaN).  `converged` = stop 1 or 2.  1.0/beta' and 1.0/alpha' are never
 *                        formed from a zero.  With an initial guess the damped problem is the one for the CORRECTION:
 *                        min |A d - (b - A x0)|^2 + damp^2 |d|^2, x = x0 + d.  normal_tolerance and damp are creation
 *                        parameters (NaN or negative: SGM_ERR_BAD_ARG), live through sgm_lsqr_set_params like the tolerance.
 * sgm_solver_setup    <- solver%setup(A): square check, work vectors, iterations = 0
 *                        cg_solvers.f90:52-90
 * sgm_solver_solve    <- solver%solve(A,x,b[,pc]): cg_solve :116-150, cg_solve_pc :155-194,
 *                        bicgstab_solve :124-177, bicgstab_solve_pc :182-237.
 *                        ABSOLUTE tolerance on sqrt(res2), initial guess from x, no
 *                        iteration cap unless sgm_solver_set_max_iter (an extension) is
 *                        called; `iterations` accumulates across solves like the reference.
 *                        The whole loop is device-resident: x and b cross the boundary once.
 *                        A breakdown (NaN res2) ends the loop as it ends the reference's; `converged` is then 0
 *                        (and the call returns SGM_ERR_NOT_CONVERGED when an iteration cap is set).
 * sgm_solver_set_tolerance <- solver%set_params(tolerance) cg_solvers.f90:95-111, bicgstab_solvers.f90:103-119, and any
 *                        later edit of the public field solver%tolerance, which the reference's loops read at every solve
 *                        (cg_solvers.f90:133,175): the next solve on this handle stops at the new ABSOLUTE tolerance;
 *                        work vectors, options and the accumulated `iterations` are kept.  Both Fortran layers and
 *                        sigma_amd push the host object's tolerance in front of every solve.
 * sgm_solver_destroy  <- solver%destroy()          cg_solvers.f90:199-212                 */
int sgm_cg_create(sgm_solver *out, double tolerance);
int sgm_bicgstab_create(sgm_solver *out, double tolerance);
int sgm_gmres_create(sgm_solver *out, double tolerance, int32_t restart);
int sgm_minres_create(sgm_solver *out, double tolerance);
int sgm_lsqr_create(sgm_solver *out, double tolerance, double normal_tolerance, double damp);
int sgm_lsqr_set_params(sgm_solver s, double normal_tolerance, double damp);
int sgm_lsqr_info(sgm_solver s, int32_t *stop, double *rnorm, double *arnorm);
int sgm_solver_setup(sgm_solver s, sgm_mat A);
int sgm_solver_set_max_iter(sgm_solver s, int64_t max_iter /* <= 0: unbounded */);
int sgm_solver_set_tolerance(sgm_solver s, double tolerance);
int sgm_solver_set_history(sgm_solver s, int64_t capacity); /* record res2 per iteration */
int sgm_solver_solve(sgm_solver s, sgm_mat A, double *x, const double *b, sgm_pc pc_or_null,
                     int where);
int sgm_solver_info(sgm_solver s, int64_t *iterations, double *res2, int32_t *converged,
                    int64_t *last_solve_iterations);
int sgm_solver_get_history(sgm_solver s, double *out_host, int64_t capacity, int64_t *count);
int sgm_solver_destroy(sgm_solver s);

/* ---- Lanczos ------------------------------------------------------------------------- *
 * sgm_lanczos <- lanczos(A, T, Q)  src/eigensolver.f90:27-90 (what eigensolve :160-208 feeds to
 * LAPACK dstev): nsteps Lanczos steps with full re-orthogonalisation.  T_host: 3 x nsteps,
 * column-major (T(2,:) diagonal, T(1,:) = T(3,:) off-diagonal); Q_out (optional): n x nsteps
 * column-major Lanczos vectors.  q1 is the start vector (the reference draws it from a
 * time-seeded RNG); it is normalised inside.  A may be row-partitioned: an in-process partition takes and
 * returns global vectors, a rank of a matrix distributed over processes its owned slice of q1 and Q (n_local x nsteps);
 * the dots are all-reduced, T is the same on every rank.
 * Every sum of both routines is taken in the device's defined order, a function of n alone (sgm_eigsh below, "Dot products"),
 * with one exception: on a leaf matrix (one CSR or ELLPACK part) the alpha of sgm_lanczos comes out of the product kernel's
 * epilogue, in that kernel's own order (what sgm_mat_matvec_dots reports).  On composites and in-process partitions alpha is a
 * sum in the device's order like every other; over ranks each sum is reduced to a slot and all-reduced.
 * (tests/lanczos_restated.py restates both loops; tests/test_gpu_lanczos.py holds T and Q to it bit for bit.) */
int sgm_lanczos(sgm_mat A, int32_t nsteps, const double *q1, double *T_host, double *Q_out, int where);

/* sgm_generalized_lanczos <- generalized_lanczos(A, B, T, Q)  src/eigensolver.f90:95-155: Lanczos for
 * A x = lambda B x.  Every step solves B w = v with `solver_for_B` (set up for B by the caller, like
 * B%set_solver; optional preconditioner), started from w = A q_i as the reference's
 * `call B%solve(w, v)` does (:140).  No re-orthogonalisation (the reference has none here); q1 is
 * normalised in the B-norm (:123-124).  T_host / Q_out as in sgm_lanczos; A and B may be row-partitioned (the same way). */
int sgm_generalized_lanczos(sgm_mat A, sgm_mat B, sgm_solver solver_for_B, sgm_pc pc_or_null, int32_t nsteps,
                            const double *q1, double *T_host, double *Q_out, int where);

/* ---- extreme eigenpairs: thick-restart Lanczos ------------------------------------------ *
 * sgm_eigsh <- NO reference counterpart: the k smallest (which = 0, "SA") or largest (which = 1, "LA") algebraic eigenvalues
 * of a SYMMETRIC matrix and their eigenvectors, to a residual tolerance, by thick-restart Lanczos (Wu-Simon).  Symmetry is NOT
 * checked.  The basis (ncv + 1 columns and one work vector, 8 (ncv + 2) n bytes) never leaves HBM, Ritz vectors are formed in
 * place on the device (sgm_basis_rotate) and the TRUE residual norms are computed and returned.  Single-GPU CSR, ELLPACK and
 * composite matrices; row-partitioned and distributed ones are SGM_ERR_UNSUPPORTED, a non-square one SGM_ERR_DIMS;
 * k < 1, ncv <= k, ncv > 64, ncv >= n, tol < 2^-40 (or not a number), max_restarts < 0, which not 0 or 1: SGM_ERR_BAD_ARG.
 *
 * The contract (this comment is its one statement: DESIGN.md 9g points here, tests/eigsh_restated.py restates it).  Every
 * operation is rounded on its own (no FMA); `A u` is the library's product (0.0 + row sum in stored order); m = ncv; Q holds
 * m + 1 columns q_0 .. q_m with an even leading dimension; H is the m x m projected matrix, on the host;
 * keep = min(k + (m - k)/2, m - 1) with integer division.
 *     q_0(i) = q1(i) / sqrt(q1.q1) ;  l = 0 ;  anorm = 0 ;  H = 0
 *     cycle c = 0, 1, ...:
 *       for j = l .. m-1:
 *          w = A q_j
 *          h_i = q_i.w, i = 0..j ;  w(:) = (..(w(:) - h_0 q_0(:)) - ..) - h_j q_j(:)    (columns ascending, every subtraction rounded)
 *          g_i = q_i.w, i = 0..j ;  w(:) = (..(w(:) - g_0 q_0(:)) - ..) - g_j q_j(:)    (second classical Gram-Schmidt pass)
 *          H(j,j) = h_j + g_j ;  beta_j = sqrt(w.w)
 *          s = (j == l ? anorm : s) ; |H(j,j)| > s: s = |H(j,j)| ; beta_j > s: s = beta_j
 *          not (beta_j > 2^-40 * s):  the cycle ends here with nc = j + 1 columns ("closed": an invariant subspace, or a NaN)
 *          j < m-1:  H(j+1,j) = H(j,j+1) = beta_j
 *          t = 1.0/beta_j ;  q_{j+1}(:) = w(:) * t
 *       nc = m unless closed.  A NaN among the H(j,j), beta_j of this cycle: leave with found = 0, converged = 0
 *       (theta, Z) = symeig(leading nc x nc block of H)    (sgm_symeig_host) ;  anorm = max(anorm, max_i |theta_i|)
 *       order the Ritz values: ascending for SA, descending for LA, ties by index
 *       closed:  leave with found = min(k, nc), converged = (nc >= k)            (every rho is 0)
 *       rho_i = |beta_{m-1} * Z(m-1, i)|
 *       rho_i <= tol * anorm for the first k in that order:  leave with found = k, converged = 1
 *       c == max_restarts:  leave with found = k, converged = 0
 *       Q[:, 0..keep-1] = Q[:, 0..m-1] * Z[:, first keep in that order]          (sgm_basis_rotate)
 *       q_keep = q_m
 *       H = 0 ;  H(i,i) = theta_i, H(keep,i) = H(i,keep) = beta_{m-1} * Z(m-1, i)   for the kept i = 0..keep-1 in that order
 *       l = keep ;  restarts += 1
 *     end:
 *       V = Q[:, 0..nc-1] * Z[:, first `found` in that order]                     (sgm_basis_rotate)
 *       lambda_i = theta_i
 *       resid_i = sqrt(r.r), r(:) = y(:) - lambda_i * v_i(:), y = A v_i           (on the device, one product per pair)
 * Convergence is decided by rho, the Lanczos ESTIMATE of the residual, against tol * anorm (anorm: the largest |Ritz value|
 * seen, a lower bound of |A|_2).  resid_out is always the TRUE residual norm |A v - lambda v|_2 of the returned pair; the two
 * are different numbers, and only rho is compared with tol.  2^-40 is a contract constant: a beta_j that small against the
 * scale of H means the Krylov space has closed, which is why a smaller tol is refused.  A closed space with at least k Ritz
 * pairs is convergence; with fewer, found = what there is and converged = 0.  A NaN anywhere (the matrix, q1 -- a zero q1
 * gives 0/0 --) ends with converged = 0 and found = 0, never "converged"; the call still returns SGM_OK.
 * Dot products: the order of every sum is a function of n alone, never of the CU count.  With G = min(1024, max(1,
 * ceil(n / 1024))) workgroups of 256 threads, thread t of the 256 G adds the products of elements 2i, 2i+1 for i = t, t + 256 G,
 * ... to its own accumulator, which starts at 0.0 (thread 0 then the last element of an odd n); each wave of 64 threads sums
 * its accumulators by the butterfly v += v[lane ^ 32], ^ 16, ... ^ 1; a workgroup adds its four wave sums left to right; for
 * G > 1 the G workgroup sums are re-reduced the same way by one workgroup: thread t adds sums t, t + 256, ... to 0.0, then the
 * butterfly and the four wave sums.  (G = 1: MINRES's default order, minres_restated.tree_dot.)
 * Host-device traffic: the cycle's new H(j,j) and beta_j come to the host in ONE copy per cycle -- its one synchronisation --
 * and the selected columns of Z go back in one; within a cycle nothing waits for the host: a closed cycle raises a device
 * flag and its remaining kernels return at once.
 * q1: n entries (host or device per `where`).  lambda_out, resid_out: k entries on the HOST; entries from `found` on are NaN.
 * V_out (may be NULL): n x k column-major, host or device per `where`; only the first `found` columns are written.
 * info (host): {restarts, products with A (the residual ones included), found, converged}.
 *
 * sgm_symeig_host: all eigenpairs of a small dense symmetric matrix by cyclic Jacobi, HOST ONLY (no HIP call, usable without a
 * GPU; m <= 64 takes microseconds there).  H: m x m column-major, both triangles read; theta: m eigenvalues in the order Jacobi
 * leaves them (NOT sorted); Z: m x m column-major, H Z = Z diag(theta); sweeps (may be NULL): the sweeps taken.  The contract:
 *     A = H ; Z = I ; sweeps = 0
 *     repeat at most 64 times:
 *         every A(p,q), p < q, is exactly 0:  stop
 *         sweeps += 1
 *         for p = 0 .. m-2, for q = p+1 .. m-1 (row-major over p < q), where apq = A(p,q) != 0:
 *             tau = (A(q,q) - A(p,p)) / (2.0*apq) ;  r = sqrt(1.0 + tau*tau)
 *             t = tau >= 0 ? 1.0/(tau + r) : -1.0/(r - tau)
 *             c = 1.0/sqrt(1.0 + t*t) ;  s = t*c
 *             A(p,p) = A(p,p) - t*apq ;  A(q,q) = A(q,q) + t*apq ;  A(p,q) = A(q,p) = 0
 *             i != p, q:  x = A(i,p) ; y = A(i,q) ;  A(i,p) = A(p,i) = c*x - s*y ;  A(i,q) = A(q,i) = s*x + c*y
 *             every i:    x = Z(i,p) ; y = Z(i,q) ;  Z(i,p) = c*x - s*y ;  Z(i,q) = s*x + c*y
 *     theta(i) = A(i,i)
 *
 * sgm_basis_rotate: Q[:, 0:kk] <- Q[:, 0:m] Z in place, 1 <= kk <= m <= 64, ldq >= n.  Q: n x m column-major with leading
 * dimension ldq, on the device (where = SGM_DEVICE; SGM_HOST: copied there and back); Z: m x kk column-major on the HOST.
 * Entry (i, c) of the result is ((0.0 + Q(i,0) Z(0,c)) + Q(i,1) Z(1,c)) + ... ascending, formed from the row as it was before
 * the call.  One row per lane, Z in LDS; compulsory traffic 8 n (m + kk) bytes.                                            */
int sgm_eigsh(sgm_mat A, int32_t k, int32_t ncv, int32_t which /* 0 = smallest algebraic, 1 = largest */, double tol,
              int32_t max_restarts, const double *q1, double *lambda_out /* k, host */,
              double *V_out /* n x k column-major, may be NULL */, double *resid_out /* k, host: the TRUE residual norms */,
              int64_t *info /* restarts, products, found, converged */, int where);
int sgm_symeig_host(int32_t m, const double *H /* m x m column-major, symmetric */, double *theta, double *Z, int32_t *sweeps);
int sgm_basis_rotate(int64_t n, int32_t m, int32_t kk, double *Q, int64_t ldq, const double *Z /* m x kk column-major, host */,
                     int where);

/* ---- smallest eigenpairs with a preconditioner: generalized Davidson ------------------- *
 * sgm_davidson <- NO reference counterpart: the k smallest algebraic eigenvalues of a SYMMETRIC matrix and their
 * eigenvectors by the generalized Davidson method with thick restart.  The search space is expanded by M^-1 r, r the residual
 * of the first Ritz pair that has not converged and M a preconditioner the caller has set up on A (Jacobi, ILDU(0), the
 * multigrid V-cycle -- whatever sgm_pc_setup accepts for A; NULL: M = I): with a V-cycle the number of steps does not grow with
 * the grid, where sgm_eigsh "SA" needs a number of products that does.  Symmetry of A and definiteness of M are NOT checked.
 * The search space V and its image W = A V (ncv columns each, and two work vectors: 8 (2 ncv + 2) n bytes) never leave HBM.
 * Single-GPU CSR, ELLPACK and composite matrices; row-partitioned and distributed ones are SGM_ERR_UNSUPPORTED, a non-square
 * one SGM_ERR_DIMS; k < 1, ncv <= k, ncv > 64, ncv >= n, tol < 2^-40 (or not a number), max_steps < 0, a null pointer, a
 * preconditioner of any kind whose last setup was not on a matrix of A's size (none at all included): SGM_ERR_BAD_ARG, before
 * anything is launched -- its apply would read and write vectors of another length; a multigrid preconditioner whose last
 * setup on such a matrix failed: the error of its apply.  The call after a refusal works.
 *
 * The contract (this comment is its one statement: DESIGN.md 9h points here, tests/davidson_restated.py restates it).  Every
 * operation is rounded on its own (no FMA); `A u` is the library's product; `a.b` is sgm_eigsh's dot product (above: its order
 * is a function of n alone); `M^-1 u` is the preconditioner's apply, a copy when pc is NULL; V and W hold ncv columns with an
 * even leading dimension; H is the projected matrix, on the host; keep = min(k + (ncv - k)/2, ncv - 1) with integer division.
 *     t = 1.0/sqrt(q1.q1) ;  V_0(:) = q1(:) * t ;  W_0 = A V_0 ;  H(0,0) = V_0.W_0
 *     m = 1 ;  locked = 0 ;  anorm = 0 ;  steps = restarts = 0
 *     loop:
 *       a NaN in H[0:m, 0:m]:  leave with found = 0, converged = 0
 *       (theta, Z) = symeig(H[0:m, 0:m])    (sgm_symeig_host) ;  a NaN in theta:  leave with found = 0, converged = 0
 *       anorm = max(anorm, max_i |theta_i|) ;  order the Ritz values ascending, ties by index
 *       while locked < min(k, m):
 *           c = order[locked] ;  z = Z[:, c]
 *           u(i) = ((0.0 + V(i,0) z_0) + V(i,1) z_1) + ...  ascending over the m columns ;  y(i) the same over W
 *           r(i) = y(i) - theta_c * u(i) ;  rn = sqrt(r.r)
 *           rn <= tol * anorm:  locked += 1      otherwise: leave the while (r is the residual the step expands with)
 *       locked == k:          for j = 0 .. (locked at the start of this pass of the loop) - 1, ascending:
 *                                 c = order[j] ;  u, y, r, rn as above ;  not (rn <= tol * anorm):  locked = j, stop looking
 *       locked == k:          leave with found = k, converged = 1
 *       locked == m:          leave with found = m, converged = 0       (every Ritz pair of a space smaller than k has
 *                                                                         converged: nothing to expand from)
 *       steps == max_steps:   leave with found = min(k, m), converged = 0
 *       m == ncv:   V[:, 0..keep-1] = V[:, 0..m-1] * Z[:, first keep in that order]   (sgm_basis_rotate's sums) ;  W the same
 *                   H = 0 ;  H(i,i) = theta of the kept i ;  theta = those, Z = I, the order 0, 1, .. ;  m = keep ;
 *                   restarts += 1                                                     (r stays as computed)
 *       t = M^-1 r ;  tau = sqrt(t.t)
 *       h_i = V_i.t, i = 0..m-1 ;  t(:) = (..(t(:) - h_0 V_0(:)) - ..) - h_{m-1} V_{m-1}(:)   (columns ascending, every subtraction rounded)
 *       g_i = V_i.t, i = 0..m-1 ;  t(:) = (..(t(:) - g_0 V_0(:)) - ..) - g_{m-1} V_{m-1}(:)   (second classical Gram-Schmidt pass)
 *       beta = sqrt(t.t)
 *       a NaN in tau or beta:      leave with found = 0, converged = 0
 *       not (beta > 2^-40 * tau):  leave with found = min(k, locked), converged = 0   (the preconditioned residual lies in the space)
 *       s = 1.0/beta ;  V_m(:) = t(:) * s ;  W_m = A V_m ;  H(i,m) = H(m,i) = V_i.W_m for i = 0..m ;  m += 1 ;  steps += 1
 *     end:
 *       Vout = V[:, 0..m-1] * Z[:, first `found` in that order]                      (sgm_basis_rotate)
 *       lambda_i = theta_i
 *       resid_i = sqrt(r.r), r(:) = y(:) - lambda_i * v_i(:), y = A v_i               (on the device, one product per pair)
 * rn is the residual of the Ritz pair AS THE TWO BASES GIVE IT (W z - theta V z; W = A V holds up to the roundings of the
 * rotations); it is the number compared with tol * anorm (anorm: the largest |Ritz value| seen, a lower bound of |A|_2), and it
 * is not what is returned: resid_out is always the TRUE residual norm |A v - lambda v|_2 of the returned pair, from a product of
 * its own, as in sgm_eigsh.  Locked pairs are NOT frozen: no column is deflated, every Rayleigh-Ritz step derives them again
 * from the grown space (which can only lower a Ritz value), and `locked` is a COUNT: while the space grows they are not tested
 * again.  A Ritz value that comes down between two locked ones -- the second copy of a double eigenvalue that the space met late
 * -- moves the later ones on by one and takes a locked place without having been tested; that is why the pairs locked in
 * earlier passes are looked at once more before the call says "converged" (k - 1 passes over the bases at most, at the end),
 * and the first one that fails becomes the pair to expand with.  resid_out reports what came of them all.
 * 2^-40 is the contract constant of sgm_eigsh.  A NaN anywhere (the matrix, the preconditioner, q1 -- a zero q1 gives 0 * inf --)
 * ends with converged = 0 and found = 0, never "converged"; the call still returns SGM_OK.
 * Host-device traffic: two synchronisations per step.  H's new column (with tau, beta and the flag of the test on them) comes
 * to the host for the Jacobi sweeps, and z goes back; then r.r comes to the host, once more for every pair that is locked in
 * that step.  Within a step nothing else waits for the host: a failed test raises a device flag and the step's remaining
 * kernels return at once.  Against a V-cycle of tens of launches these two are not what a step costs.
 * One pass per step reads both bases (u, y, r and the partial sums of r.r in one kernel; compulsory traffic 8 n (2m + 1) bytes);
 * the orthogonalisation reads V three times, the new column of H reads it once more; a restart reads and writes V and W once.
 * q1: n entries (host or device per `where`).  lambda_out, resid_out: k entries on the HOST; entries from `found` on are NaN.
 * V_out (may be NULL): n x k column-major, host or device per `where`; only the first `found` columns are written.
 * info (host, 6 entries): {steps, products with A (W_0, one per step, the residual ones), applies of the preconditioner (0
 * without one), restarts, found, converged}.                                                                              */
int sgm_davidson(sgm_mat A, sgm_pc pc_or_null, int32_t k, int32_t ncv, double tol, int32_t max_steps, const double *q1,
                 double *lambda_out /* k, host */, double *V_out /* n x k column-major, may be NULL */,
                 double *resid_out /* k, host: the TRUE residual norms */,
                 int64_t *info /* steps, products, applies, restarts, found, converged */, int where);

/* ---- smallest eigenpairs of A x = lambda B x: Davidson in the B-inner product ---------- *
 * sgm_davidson_gen <- NO reference counterpart (the reference states this problem for generalized_lanczos only, with a solve
 * with B in every step): the k smallest eigenvalues of A x = lambda B x, A SYMMETRIC, B SYMMETRIC POSITIVE DEFINITE, and their
 * B-orthonormal eigenvectors (V^T B V = I) by sgm_davidson's method carried out in the B-inner product.  No system with B is
 * solved: a step costs one product with B, one with A and one apply of the preconditioner, which the caller has set up on A
 * exactly as for sgm_davidson (NULL: M = I).  Symmetry of A and B is NOT checked; definiteness of B is checked where the loop
 * meets it (d below).  The search space V and its images W = A V and U = B V (ncv columns each, and three work vectors:
 * 8 (3 ncv + 3) n bytes) never leave HBM.
 * A: single-GPU CSR, ELLPACK or composite; B: the same; they may differ in format.  Before anything is launched: a
 * row-partitioned or distributed A or B is SGM_ERR_UNSUPPORTED; a non-square A or B, or sizes that differ, SGM_ERR_DIMS; a null
 * pointer (B included) and sgm_davidson's argument limits (k < 1, ncv <= k, ncv > 64, ncv >= n, tol < 2^-40 or not a number,
 * max_steps < 0, a preconditioner that does not serve A) SGM_ERR_BAD_ARG.  The call after a refusal works.
 *
 * The contract (this comment is its one statement: DESIGN.md 9i points here, tests/davidson_gen_restated.py restates it).
 * Every operation is rounded on its own (no FMA); `A u` and `B u` are the library's products; `a.b` is sgm_eigsh's dot product
 * (its order is a function of n alone); rotations use sgm_basis_rotate's sums; V, W and U hold ncv columns with an even leading
 * dimension; H is the projected matrix, on the host; keep = min(k + (ncv - k)/2, ncv - 1) as in sgm_davidson.
 *     p = B q1 ;  d = q1.p ;  not (d > 0):  leave with found = 0, converged = 0            (a NaN compares false)
 *     t = 1.0/sqrt(d) ;  V_0(:) = q1(:) * t ;  U_0(:) = p(:) * t ;  W_0 = A V_0 ;  H(0,0) = V_0.W_0
 *     m = 1 ;  locked = 0 ;  anorm = 0 ;  steps = restarts = 0
 *     loop:
 *       the NaN tests of H and theta, (theta, Z) = symeig(H[0:m, 0:m]), anorm, the ascending order:  as sgm_davidson
 *       the residual of the pair c = order[j], z = Z[:, c]:
 *           y(i) = ((0.0 + W(i,0) z_0) + W(i,1) z_1) + ...  ascending over the m columns ;  p(i) the same over U
 *           r(i) = y(i) - theta_c * p(i) ;  rn = sqrt(r.r) ;  pn = sqrt(p.p)
 *           it meets the test when  rn <= (tol * anorm) * pn
 *       the while that locks, the second look at the pairs locked earlier, the three ways out (locked == k, locked == m,
 *       steps == max_steps):  as sgm_davidson, with that test
 *       m == ncv:   the thick restart of sgm_davidson with Zk in place of Z[:, first keep in that order], Zk = those columns,
 *                   each z divided by sqrt(((0.0 + z_0 z_0) + z_1 z_1) + ...) (ascending, on the host) ;  the rotation by Zk
 *                   applied to V, to W and to U
 *       t = M^-1 r ;  tau = sqrt(t.t)
 *       h_i = U_i.t, i = 0..m-1 ;  t(:) = (..(t(:) - h_0 V_0(:)) - ..) - h_{m-1} V_{m-1}(:)   (columns ascending, every subtraction rounded)
 *       g_i = U_i.t, i = 0..m-1 ;  t(:) = (..(t(:) - g_0 V_0(:)) - ..) - g_{m-1} V_{m-1}(:) ;  nu = sqrt(t.t)
 *       a NaN in tau or nu:       leave with found = 0, converged = 0
 *       not (nu > 2^-40 * tau):   leave with found = min(k, locked), converged = 0
 *       p = B t ;  d = t.p ;  not (d > 0):  leave with found = 0, converged = 0     (B is not positive definite, or a NaN)
 *       s = 1.0/sqrt(d) ;  V_m(:) = t(:) * s ;  U_m(:) = p(:) * s ;  W_m = A V_m
 *       H(i,m) = H(m,i) = V_i.W_m for i = 0..m ;  m += 1 ;  steps += 1
 *     end:
 *       Vout = V[:, 0..m-1] * Zf, Zf = Z[:, first `found` in that order], every column divided the same way   (sgm_basis_rotate)
 *       lambda_i = theta_i
 *       resid_i = sqrt(r.r), r(:) = y(:) - lambda_i * p(:), y = A v_i, p = B v_i      (on the device, two products per pair)
 * Correction and dots use different bases: the Gram-Schmidt correction subtracts columns of V, the dots are taken against
 * columns of U = B V.  h_i = U_i.t is the B-inner product of V_i and t, so this IS classical Gram-Schmidt, twice, in the
 * B-inner product -- with no product with B inside it.  The one product with B of a step is p = B t, which gives the B-norm
 * of the new direction and the new column of U at once.
 * The test is relative to |B v|_2: p = U z is B times the Ritz vector as the bases give it, and a pair meets the test when
 * |W z - theta U z|_2 <= tol * anorm * |U z|_2.  With B = I that is sgm_davidson's test up to the rounding of |v|_2 (there
 * the vector has norm 1 by construction and is not measured).  The test does not change when A is scaled (r and anorm scale
 * alike) or when B is (theta U z and U z do): it needs no norm of B.
 * The columns of Z are normalised before a rotation, which sgm_davidson does not do: cyclic Jacobi leaves |z|_2 = 1 only to
 * a few tens of eps (8e-15 at m = 20), a rotation by such a z multiplies the B-norm of a kept column by |z|_2, and the factors
 * of the restarts accumulate in the columns that stay -- after 18 restarts V^T B V had 1 + 1e-13 on its diagonal.  With the
 * division a restart costs the kept columns one rounding of their norm, and V^T B V = I holds to a few eps whatever the number
 * of restarts.  The Ritz vector of the residual test is not normalised: rn / pn does not depend on |z|_2.
 * U is a rotated copy, not a recomputation: U = B V holds only up to the roundings of the scalings and the rotations, as
 * W = A V does in sgm_davidson, and rn is the residual AS THE BASES GIVE IT.  resid_out is always the TRUE residual norm
 * |A v - lambda B v|_2 of the returned pair, from two products of its own.
 * Locked pairs are not frozen; 2^-40, the NaN rule (found = 0, converged = 0, the call returns SGM_OK) and the two
 * synchronisations per step are sgm_davidson's: H's new column comes to the host with tau, nu and the flag, then r.r and p.p in
 * one copy.  A failed test (nu, or d) raises a device flag and the step's remaining kernels return at once.
 * Counts: a step that ends at one of its tests counts none of that step's products.  Products with A: W_0, one per step, one
 * per returned pair.  Products with B: the first (p = B q1, counted even when its d fails), one per step, one per returned pair.
 * One pass per step reads W and U (y, p, r and the partial sums of r.r and p.p in one kernel; compulsory traffic 8 n (2m + 1)
 * bytes, as sgm_davidson's); the orthogonalisation reads U twice and V twice, H's new column reads V once more; a restart reads
 * and writes V, W and U once.
 * q1, lambda_out, resid_out, V_out: as sgm_davidson.  info (host, 7 entries): {steps, products with A, products with B, applies
 * of the preconditioner (0 without one), restarts, found, converged}.                                                     */
int sgm_davidson_gen(sgm_mat A, sgm_mat B, sgm_pc pc_or_null, int32_t k, int32_t ncv, double tol, int32_t max_steps,
                     const double *q1, double *lambda_out /* k, host */, double *V_out /* n x k column-major, may be NULL */,
                     double *resid_out /* k, host: the TRUE |A v - lambda B v|_2 */,
                     int64_t *info /* steps, products with A, products with B, applies, restarts, found, converged */, int where);

/* ---- row-partitioned multi-GPU (nothing in the reference) ---------------- *
 * One process per GPU.  Rank r owns the contiguous global rows
 * [row_starts[r], row_starts[r+1]) of A and the same slice of every vector.
 * sgm_comm_unique_id / sgm_comm_init: RCCL bootstrap (the 128-byte id is broadcast by the
 * host, e.g. over torch.distributed/gloo or MPI).
 * sgm_csr_create_dist: this rank's rows with GLOBAL 1-based column ids; builds the sorted
 * unique halo list, renumbers columns to [owned | halo] and exchanges the send lists.
 * A distributed matrix reads x of length x_len = owned + halo (sgm_mat_info): the owned
 * part is the caller's, the halo part is filled by the library (ncclSend/ncclRecv with
 * the neighbour ranks) in every matvec.  Dots inside the solvers become
 * ncclAllReduce(sum, fp64); row sums stay bit-identical to the 1-GPU result.
 * sgm_csr_create_partitioned: the same partition / halo / reduction machinery with all P
 * row blocks inside ONE process on ONE GPU (exchanges are device gathers): x, y, b are
 * plain global-length vectors.  It exists so that the multi-GPU logic is exercised by
 * `pytest -m gpu` on a single-GPU box.
 * sgm_halo_plan_host: the host-only index work of the two calls above (no HIP call), so it
 * can be checked bit-for-bit without a GPU: sorted unique halo list (global, 1-based) and
 * the renumbered node array (1-based: 1..n_own owned, n_own+1.. halo, in halo-list order). */
int sgm_comm_unique_id(void *id128);
int sgm_comm_init(sgm_comm *out, int rank, int nranks, const void *id128);
int sgm_comm_destroy(sgm_comm c);
/* sgm_comm_attach_halo_comm: a SECOND communicator (its own 128-byte id, broadcast like the first) for the halo send / recv
 * pairs, so that they do not share a queue with the dots' all-reduces -- an A/B switch for the overlap of halo traffic
 * with interior rows on a multi-GPU node.  Optional; without it one communicator carries both.
 * sgm_dist_profile(on) / sgm_dist_profile_read: HIP-event timers around the phases of the row-partitioned path, summed
 * since the last read: ms_out[6] / count_out[6] = { halo gather + send/recv on the communication stream (post -> done),
 * interior-rows kernel(s), what the launch stream then still waits for the halo, boundary-rows kernel(s),
 * per-dot partial -> slot reduction kernels, all-reduces }.  Reading synchronises the library's streams.           */
int sgm_comm_attach_halo_comm(sgm_comm c, const void *id128);
/* sgm_comm_group_selftest: one ncclGroup holding a send / recv pair (rank to itself) and an in-place all-reduce of one double
 * -- the group CG posts per iteration with "dist_halo_fused" = 1 -- on this communicator's transport.  out3 = { the double
 * the pair delivered (42 + rank), the all-reduced 1.0 (= nranks), microseconds of the second such group }.  No reference
 * counterpart (the reference has no communication); a probe that lets a one-GPU box show that the real
 * librccl accepts the mixed group. */
int sgm_comm_group_selftest(sgm_comm c, double *out3);
/* sgm_comm_group_ok: what sgm_comm_init's own probe found (1 / 0).  With more than one rank sgm_comm_init posts, once and
 * collectively, the group CG depends on with "dist_halo_fused" = 1 -- one double to the right neighbour, one from the left and
 * an all-reduce in ONE ncclGroup -- and the ranks agree on the outcome with a plain all-reduce.  0 = some rank's transport
 * refused the group or delivered wrong values: every solve on this communicator then posts the pairs and the all-reduce one
 * after the other (the order "dist_halo_fused" = 2 uses) instead of failing in its first iteration.  No reference counterpart (the reference has no communication). */
int sgm_comm_group_ok(sgm_comm c);
int sgm_dist_profile(int on);
int sgm_dist_profile_read(double *ms_out /* 6 */, int64_t *count_out /* 6 */);
int sgm_csr_create_dist(sgm_mat *out, sgm_comm comm, const int64_t *row_starts /* nranks+1, 0-based */,
                        int64_t nnz_local, const int32_t *ptr_1based_local,
                        const int32_t *node_1based_global, const double *val, int where);
/* sgm_csr_create_dist_rect: rows partitioned by row_starts, x (the columns) by col_starts -- an off-diagonal block
 * of a composite (sparse_matrix_composites.f90:41-162) whose block rows / columns have partitions of their own.
 * matvec reads x as [this rank's col_starts slice | halo].  A composite of such leaves (every leaf on the same
 * communicator, block row i partitioned like block column i) is itself a distributed operator: its vectors are
 * the concatenation of this rank's slices of the block vectors.                                               */
int sgm_csr_create_dist_rect(sgm_mat *out, sgm_comm comm, const int64_t *row_starts, const int64_t *col_starts,
                             int64_t nnz_local, const int32_t *ptr_1based_local,
                             const int32_t *node_1based_global, const double *val, int where);
/* sgm_ell_create_dist: this rank's rows of an ELLPACK matrix (node / val as (max_d, n_local) column-major,
 * GLOBAL 1-based columns, padding as the reference keeps it).  Held as fixed-length CSR rows whose padding
 * slots are stored entries, so the row sums equal ellpack_matvec_add's (ellpack_matrices.f90:640-665).
 * degrees_or_null: this rank's degrees(n_local), where node / val live; checked like sgm_ell_set_degrees' (SGM_ERR_DIMS).
 * NULL: recovered from the padding by the rule stated at sgm_ell_set_degrees, or absent when a row has another shape
 * (ILDU(0) setup on the matrix then refuses). */
int sgm_ell_create_dist(sgm_mat *out, sgm_comm comm, const int64_t *row_starts, int32_t max_d,
                        const int32_t *node_1based_global_colmajor, const double *val_colmajor,
                        const int32_t *degrees_or_null, int where);
int sgm_csr_create_partitioned(sgm_mat *out, int32_t nparts, const int64_t *row_starts /* nparts+1 */,
                               int32_t nrow, int32_t ncol, int64_t nnz,
                               const int32_t *ptr_1based, const int32_t *node_1based,
                               const double *val /* host arrays */);
/* sgm_csr_create_partitioned_parts: the same in-process partition handed over PART BY PART: for every part its rows as
 * sgm_csr_create_dist takes a rank's (local 1-based row pointers, GLOBAL 1-based columns, values), all host or all device
 * arrays -- for matrices too large to assemble whole on the host (the 7-point 464^3 grid of BASELINE config 5: 8.8 GB).  Same
 * planners and parts as sgm_csr_create_partitioned; no reference counterpart (the reference has one address space:
 * cs_matrices.f90:32-107). */
int sgm_csr_create_partitioned_parts(sgm_mat *out, int32_t nparts, const int64_t *row_starts /* nparts+1 */,
                                     const int64_t *nnz_of_part, const int32_t *const *ptr_1based_local_of_part,
                                     const int32_t *const *node_1based_global_of_part, const double *const *val_of_part,
                                     int where);
int sgm_halo_plan_host(int32_t n_own, int64_t col_begin /* first owned global column, 0-based */,
                       int64_t nnz, const int32_t *node_1based_global,
                       int32_t *node_1based_local_out, int32_t *halo_cols_out /* capacity nnz */,
                       int32_t *n_halo_out);
/* The rest of the host-only planning that sgm_csr_create_dist / _partitioned run (no HIP call; the
 * world_size-2 gloo test drives exactly these, exchanging the lists over gloo instead of RCCL):
 * sgm_dist_plan_host       one rank's requests: want[q] = entries of its (sorted) halo list that
 *                          rank q owns, want_off = their prefix sum (nranks+1: the run of halo
 *                          entries owned by q), req[t] = index of halo entry t in ITS OWNER's local
 *                          numbering (0-based) -- the list that owner gathers from when it sends.
 * sgm_dist_neighbors_host  one rank's neighbour table from the all-gathered want matrix
 *                          (want_all[q*nranks + r] = rank q's want[r]): per neighbour its rank,
 *                          how many entries go to it / come from it, and where the received run
 *                          starts inside this rank's halo region.  Arrays hold up to nranks-1.
 * sgm_partition_links_host every (sender, receiver) link of an in-process partition, as
 *                          sgm_csr_create_partitioned builds them: first call with sender = NULL
 *                          for the sizes (n_links, idx_needed), then with arrays; idx_concat holds
 *                          the senders' gather lists end to end (0-based local indices).
 * sgm_partition_rows_by_nnz contiguous row blocks balanced by the bytes of B_csr they carry
 *                          (12 per stored entry + 20 per row, SURVEY 8d/8e "balanced by nnz"),
 *                          boundaries rounded to multiples of `align` rows (even; 512 keeps the
 *                          sliced kernel's slices whole).  row_starts_out: nparts+1 entries.
 * sgm_mat_halo_nbr         reads the exchange plan of a built matrix back (k < 0: only n_nbrs). */
int sgm_dist_plan_host(int32_t rank, int32_t nranks, const int64_t *row_starts, int32_t n_halo,
                       const int32_t *halo_cols_1based, int32_t *want, int32_t *want_off, int32_t *req);
int sgm_dist_neighbors_host(int32_t rank, int32_t nranks, const int32_t *want_all, int32_t *peer,
                            int32_t *send_count, int32_t *recv_count, int32_t *recv_offset, int32_t *n_nbrs);
int sgm_partition_links_host(int32_t nparts, const int64_t *row_starts, const int32_t *ptr_1based,
                             const int32_t *node_1based, int32_t *n_links, int32_t *sender, int32_t *receiver,
                             int32_t *recv_offset, int32_t *count, int32_t *idx_concat, int64_t idx_capacity,
                             int64_t *idx_needed);
int sgm_partition_rows_by_nnz(int32_t nrow, const int32_t *ptr_1based, int32_t nparts, int32_t align,
                              int64_t *row_starts_out);
/* Two more pieces of host-only index work, exported like the planners above so that the CPU suite (and the sanitizer build,
 * tools/asan) drives the statements the library runs:
 * sgm_ell_degrees_host        degrees(n) of an ELLPACK graph recovered from the padding the reference keeps (ellpack_graphs.f90:164,
 *                             :394-397: the rest of a row repeats the neighbour just added; a row of zeros is empty) -- what
 *                             sgm_ell_create / sgm_ell_create_dist do when no degrees are handed in; -1 for a row the padding
 *                             does not describe (the rule and its limit: at sgm_ell_set_degrees above)
 * sgm_left_permute_rows_host  rows [r0, r1) (0-based) of A%left_permute(p) (cs_matrices.f90:471-478) cut out of the whole matrix:
 *                             what a rank keeps of a permuted matrix distributed over ranks.  lnode == NULL: sizing call. */
int sgm_ell_degrees_host(int32_t n, int32_t max_d, const int32_t *node_1based_colmajor, int32_t *degrees_out);
int sgm_left_permute_rows_host(int32_t n, const int32_t *p_1based, const int32_t *ptr_1based, const int32_t *node_1based,
                               const double *val, int64_t r0, int64_t r1, int32_t *lptr_out, int32_t *lnode_out,
                               double *lval_out, int64_t capacity, int64_t *needed);
int sgm_mat_halo_nbr(sgm_mat A, int32_t part, int32_t k, int32_t *n_nbrs, int32_t *peer, int32_t *send_count,
                     int32_t *recv_count, int32_t *recv_offset, int32_t *send_idx_host, int32_t capacity);

#ifdef __cplusplus
}
#endif
#endif /* SIGMA_HIP_H */
