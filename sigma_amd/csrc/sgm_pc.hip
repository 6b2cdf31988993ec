// Preconditioners for gfx950: the object behind sgm_pc, its C ABI, and the pc_* functions the Krylov loops call.
//
// Jacobi (jacobi_solvers.f90:37-81): idiag(i) = 1/A(i,i) is extracted on the DEVICE by a row scan (the reference calls
// A%get_value(i,i) per row, cs_matrices.f90:709-724); apply is one elementwise pass (scale_by, sgm_trsv.hip).
// ILDU(0) (ldu_solvers.f90:95-176, :208-265, :275-440): one IlduState per part; sgm_ildu.hip sets a block up, sgm_trsv.hip /
// sgm_trsv3.hip sweep it; which sweep serves an apply is decided here (pc_apply_parts).
// Option ildu_reorder: the factors are those of the colour-ordered matrix P A P^T.  The ordering (device, sgm_order.hip) is
// found once per pattern, the permuted copy of A is rebuilt at every setup and kept for the solvers; the HOST only orders
// the halo slots and maps the neighbours' request lists.
// Multigrid (SGM_PC_MG) lives in sgm_mg.hip behind the mg_* hooks.
#include "sgm_pc_internal.hpp"

#include <algorithm>
#include <chrono>
#include <cstring>

using namespace sgm;

namespace {

// ------------------------------------------------------------------------------ kernels
// rows [row0, row0 + count) of a leaf; the diagonal of global row i sits at local column
// (local row) + dcol of this leaf (dcol = 0 for a plain matrix; row-block minus column-block
// offset for a block of a composite, composite_mat_get_value sparse_matrix_composites.f90:465-485)
__global__ void k_jacobi_setup_csr(int32_t count, int32_t row0, int32_t dcol, const int32_t *__restrict__ rowptr,
                                   const int32_t *__restrict__ col, const double *__restrict__ val,
                                   double *__restrict__ idiag)
{
    int32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    const int32_t i = row0 + t, want = i + dcol;
    double z = 0.0;                                   // get_value: 0 when the entry is absent
    for (int32_t k = rowptr[i]; k < rowptr[i + 1]; ++k)
        if (col[k] == want) z = val[k];
    idiag[t] = 1.0 / z;
}
__global__ void k_jacobi_setup_ell(int32_t count, int32_t row0, int32_t dcol, int32_t n, int32_t max_d,
                                   const int32_t *__restrict__ ecol, const double *__restrict__ eval,
                                   const int32_t *__restrict__ edeg, double *__restrict__ idiag)
{
    int32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    const int32_t i = row0 + t, want = i + dcol;
    // ellpack get_value scans the first degrees(i) slots and keeps the LAST hit (ellpack_matrices.f90:232-235): the padding,
    // whatever it holds, is no entry, and of a column stored twice among the real slots the later one answers
    // (edeg: validated against max_d when it came in, sgm_ell_set_degrees; null only when there is no slot at all)
    const int32_t d = edeg ? min(edeg[i], max_d) : 0;
    double z = 0.0;
    for (int32_t k = 0; k < d; ++k)
        if (ecol[(int64_t)k * n + i] == want) z = eval[(int64_t)k * n + i];
    idiag[t] = 1.0 / z;
}
__global__ void k_fill_inf(int32_t count, double *idiag)
{
    int32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < count) idiag[t] = 1.0 / 0.0;
}

}  // namespace

namespace sgm {

int pc_kind(sgm_pc pc) { return pc ? pc->kind : 0; }
sgm_pc pc_adopt_mg(MgState *S)
{
    sgm_pc pc = new sgm_pc_s;
    pc->kind = SGM_PC_MG;
    pc->mg = S;
    return pc;
}
MgState *pc_mg(sgm_pc pc) { return pc && pc->kind == SGM_PC_MG ? pc->mg : nullptr; }
// an apply that is a handful of launches (Jacobi; ILDU through the strip / slab pipeline or over a few wide levels) lets the
// solvers queue a whole batch of iterations between two looks at the stop flag; thousands of level launches per apply do not
bool pc_apply_is_short(sgm_pc pc)
{
    if (!pc || pc->kind == SGM_PC_JACOBI) return true;
    if (pc->kind == SGM_PC_MG) return false;      // a V-cycle is tens of launches: the solvers look at the stop flag after each iteration
    // (a colour-ordered matrix has two or three levels per factor: its level-scheduled apply is seven to nine launches)
    for (const auto &S : pc->ild) {
        if (pc->opt.ildu_strips && (S.grid_ok || S.slab_ok)) continue;
        if (!S.levels_ready) return false;
        if (pc->opt.ildu_rows && S.L.rows_on && S.U.rows_on) continue;         // at most 2 * kRowLevels launches
        if (!S.walk_ready || 3 + S.L.schedule.size() + S.U.schedule.size() > 35) return false;
    }
    return true;
}
const double *pc_idiag(sgm_pc pc, size_t part) { return pc->parts[part].idiag; }
// pc_apply_parts(pc, A, ..) finds what it reads and stays inside vectors of A's length: the preconditioner's last setup was
// on a matrix of A's size (pc->n: 0 before any setup) and, for Jacobi and ILDU(0), of A's parts.  (A multigrid preconditioner
// whose last setup FAILED on a matrix of that size passes here and is refused by mg_apply.)
bool pc_serves(sgm_pc pc, sgm_mat A)
{
    if (!pc || !A) return false;
    if (pc->n != A->nrow) return false;
    if (pc->kind == SGM_PC_MG) return true;
    if (pc->kind == SGM_PC_JACOBI) return !pc->parts.empty() && pc->parts.size() >= A->parts.size() && pc->parts[0].idiag;
    return !pc->ild.empty() && pc->ild.size() == A->parts.size();
}

// ILDU(0) of the colour-ordered matrix (option ildu_reorder): the permuted matrix the factors belong to (null: none / natural
// order).  A solver that finds one runs in the permuted order: x and b through pc_permute_vec once each way, the products on
// this matrix, and pc_in_permuted(pc, true) around the solve so that the applies skip their own two permutations.
// Only for the very matrix it was made from, unchanged since (the reference lets any matrix be solved with any preconditioner:
// for another one the applies permute r and z themselves).
sgm_mat pc_permuted_matrix(sgm_pc pc, sgm_mat A)
{
    if (!pc || pc->kind != SGM_PC_ILDU0 || pc->ro.empty() || !pc->Ap || !A) return nullptr;
    return pc->Ap_serial == A->serial && pc->Ap_version == A->version ? pc->Ap : nullptr;
}
void pc_in_permuted(sgm_pc pc, bool on) { if (pc) pc->in_permuted = on; }

// The sticky abort word of a preconditioner whose apply runs through a pipelined triangular solve right now (null otherwise:
// nothing to watch).  Whoever synchronises after such applies copies it back; nonzero = some sweep gave up and its result --
// and everything computed from it -- is not to be used.
int32_t *pc_abort_word(sgm_pc pc)
{
    if (!pc || pc->kind != SGM_PC_ILDU0 || !pc->opt.ildu_strips || !pc->abort_sticky) return nullptr;
    for (const auto &S : pc->ild)
        if (S.grid_ok || S.slab_ok) return pc->abort_sticky;
    return nullptr;
}
// After an abort: the pipelines of this handle are retired (every later apply takes the level walkers, built here if they
// were never needed) and the word is cleared.  Loud on stderr: it should not happen on a GPU this process owns.
int pc_retire_pipelines(sgm_pc pc)
{
    fprintf(stderr, "[sigma_hip] ILDU pipelined triangular solve gave up waiting (preempted / shared GPU?): result discarded, "
                    "redone with the level-scheduled solves; the pipeline is retired for this preconditioner\n");
    for (auto &S : pc->ild) {
        S.grid_ok = false;
        S.slab_ok = false;
        SGM_TRY(ensure_levels(&S));
        if (!rows_serve(&S)) SGM_TRY(ensure_walkers(&S));
    }
    pc->retired += 1;
    SGM_HIP(hipMemsetAsync(pc->abort_sticky, 0, sizeof(int32_t), g_rt.stream));
    return SGM_OK;
}

// dst[p(i) - 1] = src[i]  /  dst[i] = src[p(i) - 1]
__global__ void k_perm_to(int32_t n, const int32_t *__restrict__ p1, const double *__restrict__ src, double *__restrict__ dst,
                          const int *__restrict__ flag)
{
    if (flag && *flag) return;
    int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const int32_t stride = gridDim.x * blockDim.x;
    for (; i < n; i += stride) dst[p1[i] - 1] = src[i];
}
__global__ void k_perm_from(int32_t n, const int32_t *__restrict__ p1, const double *__restrict__ src, double *__restrict__ dst,
                            const int *__restrict__ flag)
{
    if (flag && *flag) return;
    int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const int32_t stride = gridDim.x * blockDim.x;
    for (; i < n; i += stride) dst[i] = src[p1[i] - 1];
}

static int pc_apply_parts_ordered(sgm_pc pc, sgm_mat A, const double *const *r, double *const *z, const int *const *flags);

// part ip's slice: dst = P src (to_permuted) or dst = P^T src
void pc_permute_vec(sgm_pc pc, size_t ip, const double *src, double *dst, bool to_permuted)
{
    const int32_t n = pc->ro[ip].n;
    if (!n) return;
    if (to_permuted) hipLaunchKernelGGL(k_perm_to, dim3(vec_grid(n)), dim3(kBlock), 0, g_rt.stream, n, (const int32_t *)pc->ro[ip].perm, src, dst, (const int *)nullptr);
    else hipLaunchKernelGGL(k_perm_from, dim3(vec_grid(n)), dim3(kBlock), 0, g_rt.stream, n, (const int32_t *)pc->ro[ip].perm, src, dst, (const int *)nullptr);
}

// CG's "r -= alpha q; z = M^-1 r; partial sums of r.z" as the two launches of a two-level row-space factorisation
// (k_trsv_rows_cg).  false: this preconditioner is not of that kind here -- the caller launches the three steps itself.
// *count = partial sums left in `part`.
// pc_cg_fused_rows: 0 = not that kind, else n0 -- the caller first updates r(0 .. n0-1) -= alpha q (the rows without L
// entries: nobody else writes them), then calls pc_cg_fused, which updates the others as its first sweep reaches them
int32_t pc_cg_fused_rows(sgm_pc pc, size_t ip)
{
    if (!pc || pc->kind != SGM_PC_ILDU0 || ip >= pc->ild.size() || (!pc->ro.empty() && !pc->in_permuted)) return 0;
    const IlduState *S = &pc->ild[ip];
    if ((S->opt.ildu_strips && (S->grid_ok || S->slab_ok)) || !S->levels_ready || !rows_two_level(S)) return 0;
    return S->rows_n0;
}
bool pc_cg_fused(sgm_pc pc, size_t ip, ScalarRef res2, ScalarRef dpr, const double *q, double *r, double *z, double *part, int *count, const int *flag, int gen)
{
    if (!pc_cg_fused_rows(pc, ip)) return false;
    rows_cg_fused(&pc->ild[ip], res2, dpr, q, r, z, part, count, flag, gen);
    return true;
}

int pc_apply_parts(sgm_pc pc, sgm_mat A, const double *const *r, double *const *z, const int *const *flags)
{
    if (pc->kind == SGM_PC_ILDU0 && !pc->ro.empty() && !pc->in_permuted) {
        // z = P^T M^-1 P r, part by part: into the colour order, the sweeps there, back
        hipStream_t st = g_rt.stream;
        const size_t P = pc->ro.size();
        std::vector<const double *> rr(P);
        std::vector<double *> zz(P);
        for (size_t ip = 0; ip < P; ++ip) {
            const auto &R = pc->ro[ip];
            if (R.n) hipLaunchKernelGGL(k_perm_to, dim3(vec_grid(R.n)), dim3(kBlock), 0, st, R.n, (const int32_t *)R.perm, r[ip], R.rp, flags ? flags[ip] : nullptr);
            rr[ip] = R.rp; zz[ip] = R.zp;
        }
        SGM_TRY(pc_apply_parts_ordered(pc, A, rr.data(), zz.data(), flags));
        for (size_t ip = 0; ip < P; ++ip) {
            const auto &R = pc->ro[ip];
            if (R.n) hipLaunchKernelGGL(k_perm_from, dim3(vec_grid(R.n)), dim3(kBlock), 0, st, R.n, (const int32_t *)R.perm, (const double *)R.zp, z[ip], flags ? flags[ip] : nullptr);
        }
        SGM_HIP(hipGetLastError());
        return SGM_OK;
    }
    return pc_apply_parts_ordered(pc, A, r, z, flags);
}

static int pc_apply_parts_ordered(sgm_pc pc, sgm_mat A, const double *const *r, double *const *z, const int *const *flags)
{
    if (pc->kind == SGM_PC_MG) {
        if (A->parts.size() != 1) return fail(SGM_ERR_UNSUPPORTED, "multigrid: single-GPU matrices only");
        return mg_apply(pc->mg, r[0], z[0], flags ? flags[0] : nullptr);
    }
    if (pc->kind == SGM_PC_JACOBI) {
        for (size_t ip = 0; ip < A->parts.size(); ++ip)
            scale_by(A->parts[ip].n, pc->parts[ip].idiag, r[ip], z[ip], flags ? flags[ip] : nullptr);
    } else {
        for (size_t ip = 0; ip < pc->ild.size(); ++ip) {      // block-Jacobi over the parts: no exchange
            const IlduState *S = &pc->ild[ip];
            const int *flag = flags ? flags[ip] : nullptr;
            const int spin = pc->opt.pipeline_spin_limit > 0 ? pc->opt.pipeline_spin_limit : kStripSpinLimit;
            if (S->grid_ok && S->opt.ildu_strips) {                 // grid-like factors: one strip-pipelined launch per sweep
                apply_grid(S, r[ip], z[ip], flag, spin, pc->abort_sticky);
                continue;
            }
            if (S->slab_ok && S->opt.ildu_strips) {                 // 3-D grid factors: one slab-pipelined launch per sweep
                slab3_apply(S->slab, r[ip], z[ip], flag, spin, pc->abort_sticky);
                continue;
            }
            SGM_TRY(ensure_levels(&pc->ild[ip]));              // (built on first need when a pipelined path served the pattern so far)
            if (rows_serve(S)) { apply_rows(S, r[ip], z[ip], flag); continue; }
            SGM_TRY(ensure_walkers(&pc->ild[ip]));
            apply_levels(S, r[ip], z[ip], flag);
        }
    }
    SGM_HIP(hipGetLastError());
    return SGM_OK;
}

}  // namespace sgm

extern "C" {

static int pc_setup_ordered(sgm_pc pc, sgm_mat A);
int sgm_pc_info(sgm_pc pc, int32_t part, int32_t *out4, double *est_us, char *path_name, int len);

// SGM_TRACE: one line per setup naming the sweeps that will serve the applies (sgm_pc_info) -- a chain-bound `ldu()` says so
static void trace_setup(sgm_pc pc)
{
    if (!trace_on()) return;
    const size_t P = pc->kind == SGM_PC_JACOBI ? 1 : pc->ild.size();
    for (size_t ip = 0; ip < P && ip < 2; ++ip) {
        int32_t o[4]; double us = 0.0; char nm[160];
        if (sgm_pc_info(pc, (int32_t)ip, o, &us, nm, (int)sizeof nm) != SGM_OK) return;
        fprintf(stderr, "[sigma_hip] %s setup%s: %s, about %.0f us per apply%s%s\n", pc->kind == SGM_PC_JACOBI ? "jacobi" : "ildu",
                P > 1 ? (ip == 0 ? " (part 0)" : " (part 1)") : "", nm, us, o[3] ? ", colour-ordered" : "",
                o[2] >= 2 && !o[3] ? " -- a dependency chain: ldu(reorder=\"colour\") / option ildu_reorder makes it two bandwidth-bound sweeps" : "");
    }
}

static void free_reorder(sgm_pc pc)
{
    for (auto &R : pc->ro) { dfree(R.perm); dfree(R.rp); dfree(R.zp); dfree(R.hmap); for (int32_t *q : R.send_order) dfree(q); }
    pc->ro.clear();
}

// ILDU(0) of the colour-ordered matrix (option ildu_reorder): the ordering once per pattern (ldu_solvers.f90:117-125 builds the
// pattern once), a permuted copy of A per setup (the values may have changed), the regular device-side setup on that copy.
// On a row partition every part orders its own DIAGONAL block (greedy_color_ordering of A_kk's graph, permutations.f90:83-205;
// no communication) and the copy's part k is P_k A_k [P_k^T (+) I]: rows and owned columns renumbered, halo columns and
// the neighbours' request lists' meaning kept (the lists are mapped through P_k) -- block-Jacobi ILDU(0) of the ordered
// blocks, SURVEY 8e.
static double ms_since(std::chrono::steady_clock::time_point t)
{
    (void)hipStreamSynchronize(g_rt.stream);
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
}

static int halo_orders(sgm_pc pc, sgm_mat A);
// the orderings and the halo orders, found for this matrix's pattern and kept until it changes
static int find_orderings(sgm_pc pc, sgm_mat A)
{
    const auto t0 = std::chrono::steady_clock::now();
    const size_t P = A->parts.size();
    bool same = pc->ro.size() == P && pc->ro_serial == A->serial && pc->ro_pattern == A->pattern_version;
    for (size_t ip = 0; same && ip < P; ++ip) same = pc->ro[ip].n == A->parts[ip].n && pc->ro[ip].perm && pc->ro[ip].rp && pc->ro[ip].zp;
    if (same) return SGM_OK;
    free_reorder(pc);
    for (auto &S : pc->ild) free_ildu(S);
    pc->ild.clear();
    pc->ro.resize(P);
    struct Undo { sgm_pc pc; bool armed = true; ~Undo() { if (armed) free_reorder(pc); } } undo{pc};      // (a failure below leaves no half-made ordering behind)
    for (size_t ip = 0; ip < P; ++ip) {
        sgm_mat B = nullptr;
        SGM_TRY(diag_block_plain(A->parts[ip], &B));
        std::vector<int32_t> ptrs;
        const int rc = color_order_device(B, &pc->ro[ip].perm, ptrs);
        sgm_mat_destroy(B);
        if (rc != SGM_OK) return rc;
        pc->ro[ip].n = A->parts[ip].n;
        pc->ro[ip].colors = (int32_t)ptrs.size() - 1;
        SGM_TRY(dalloc(&pc->ro[ip].rp, (size_t)pc->ro[ip].n + 2));
        SGM_TRY(dalloc(&pc->ro[ip].zp, (size_t)pc->ro[ip].n + 2));
    }
    SGM_TRY(halo_orders(pc, A));
    undo.armed = false;
    pc->ro_serial = A->serial;
    pc->ro_pattern = A->pattern_version;
    pc->reorder_ms[0] = ms_since(t0);
    return SGM_OK;
}

static int halo_orders(sgm_pc pc, sgm_mat A)
{
    const size_t P = A->parts.size();
    // Halo slots in the order of the permuted rows they attach to (index work, once per pattern): in the colour order a
    // grid part's halo columns would otherwise sit at a different offset from every row -- the 15-entry offset dictionary
    // overflows and the product falls from k_csr_sl (8.5 B per slot) to k_csr_sl32 (12 B).  Every receiver orders the
    // slots of each neighbour's segment and the senders permute their lists to match (ranks: one exchange of int32 lists).
    for (size_t ip = 0; ip < P; ++ip) {
        std::vector<std::pair<int32_t, int32_t>> seg;
        if (A->comm) {
            for (const HaloNbr &nb : A->parts[ip].nbrs)
                if (nb.recv_count) seg.emplace_back(nb.recv_offset, nb.recv_count);
        } else {
            for (size_t is = 0; is < P; ++is)
                for (const HaloNbr &nb : A->parts[is].nbrs)
                    if ((size_t)nb.peer == ip && nb.send_count) seg.emplace_back(nb.recv_offset, nb.send_count);
        }
        auto &R = pc->ro[ip];
        SGM_TRY(halo_attach_order(A->parts[ip], R.perm, seg, R.hmap_host));
        if (!R.hmap_host.empty()) {
            SGM_TRY(dalloc(&R.hmap, R.hmap_host.size()));
            SGM_HIP(hipMemcpyAsync(R.hmap, R.hmap_host.data(), R.hmap_host.size() * 4, hipMemcpyHostToDevice, g_rt.stream));
            SGM_HIP(hipStreamSynchronize(g_rt.stream));
        }
    }
    if (A->comm) SGM_TRY(exchange_halo_orders(A, pc->ro[0].hmap_host, pc->ro[0].send_order));
    else
        for (size_t is = 0; is < P; ++is) {
            auto &S = pc->ro[is];
            S.send_order.assign(A->parts[is].nbrs.size(), nullptr);
            for (size_t k = 0; k < A->parts[is].nbrs.size(); ++k) {
                const HaloNbr &nb = A->parts[is].nbrs[k];
                if (!nb.send_count) continue;
                const std::vector<int32_t> &hm = pc->ro[(size_t)nb.peer].hmap_host;
                std::vector<int32_t> rel((size_t)nb.send_count);
                for (int32_t t = 0; t < nb.send_count; ++t) rel[(size_t)t] = hm[(size_t)nb.recv_offset + t] - nb.recv_offset;
                SGM_TRY(dalloc(&S.send_order[k], (size_t)nb.send_count));
                SGM_HIP(hipMemcpyAsync(S.send_order[k], rel.data(), (size_t)nb.send_count * 4, hipMemcpyHostToDevice, g_rt.stream));
                SGM_HIP(hipStreamSynchronize(g_rt.stream));
            }
        }
    return SGM_OK;
}

// the permuted copy of A (kept, with A's kernel forms, for the solvers) and the regular setup on it
static int setup_on_permuted_copy(sgm_pc pc, sgm_mat A)
{
    const size_t P = A->parts.size();
    auto t0 = std::chrono::steady_clock::now();
    if (pc->Ap) { sgm_mat_destroy(pc->Ap); pc->Ap = nullptr; }
    sgm_mat Ap = new sgm_mat_s;
    Ap->fmt = SGM_FMT_CSR; Ap->nrow = A->nrow; Ap->ncol = A->ncol; Ap->nnz = A->nnz;
    Ap->comm = A->comm; Ap->row_starts = A->row_starts; Ap->col_starts = A->col_starts; Ap->halo_cols = A->halo_cols;
    Ap->parts.resize(P);
    int rc = SGM_OK;
    for (size_t ip = 0; rc == SGM_OK && ip < P; ++ip)
        rc = permuted_part(A->parts[ip], pc->ro[ip].perm, Ap->parts[ip], pc->ro[ip].hmap, &pc->ro[ip].send_order);
    if (A->comm && !Ap->halo_cols.empty() && pc->ro[0].hmap_host.size() == Ap->halo_cols.size())      // (global column of every halo slot, in the new order)
        for (size_t h = 0; h < pc->ro[0].hmap_host.size(); ++h) Ap->halo_cols[(size_t)pc->ro[0].hmap_host[h]] = A->halo_cols[h];
    pc->reorder_ms[1] = ms_since(t0);
    t0 = std::chrono::steady_clock::now();
    if (rc == SGM_OK) rc = pc_setup_ordered(pc, Ap);
    pc->reorder_ms[2] = ms_since(t0);
    if (rc == SGM_OK) { pc->Ap = Ap; pc->Ap_serial = A->serial; pc->Ap_version = A->version; }
    else sgm_mat_destroy(Ap);
    return rc;
}

int sgm_pc_setup(sgm_pc pc, sgm_mat A)
{
    SGM_TRY(require_init());
    if (!pc || !A) return fail(SGM_ERR_BAD_ARG, "sgm_pc_setup: null argument");
    if (pc->kind == SGM_PC_MG) {
        SGM_TRY(mg_setup(pc->mg, A));
        pc->n = A->nrow;
        return SGM_OK;
    }
    const bool reorder = pc->kind == SGM_PC_ILDU0 && pc->opt.ildu_reorder && A->fmt == SGM_FMT_CSR && A->nrow == A->ncol && A->nrow > 0;
    if (reorder) {
        SGM_TRY(find_orderings(pc, A));
        SGM_TRY(setup_on_permuted_copy(pc, A));
    } else {
        if (!pc->ro.empty()) { free_reorder(pc); for (auto &S : pc->ild) free_ildu(S); pc->ild.clear(); }
        if (pc->Ap) { sgm_mat_destroy(pc->Ap); pc->Ap = nullptr; }
        SGM_TRY(pc_setup_ordered(pc, A));
    }
    trace_setup(pc);
    return SGM_OK;
}

// out[t] = 1 / A(row0 + t, row0 + t + dcol) for `count` rows of the leaf part p (see k_jacobi_setup_csr)
static int jacobi_rows(const Part &p, int32_t fmt, int32_t row0, int32_t count, int32_t dcol, double *out)
{
    hipStream_t st = g_rt.stream;
    const int grid = (count + kBlock - 1) / kBlock;
    if (fmt == SGM_FMT_ELL) SGM_TRY(ell_need_degrees("Jacobi setup", p));
    if (!grid) return SGM_OK;
    if (fmt == SGM_FMT_CSR) {
        SGM_TRY(csr_need_arrays(p));
        hipLaunchKernelGGL(k_jacobi_setup_csr, dim3(grid), dim3(kBlock), 0, st, count, row0, dcol, p.rowptr, p.col, p.val, out);
        csr_release_arrays(p);
    } else
        hipLaunchKernelGGL(k_jacobi_setup_ell, dim3(grid), dim3(kBlock), 0, st, count, row0, dcol, p.n, p.max_d, p.ecol,
                           p.eval, (const int32_t *)p.edeg, out);
    return SGM_OK;
}

// jacobi_setup only needs A%get_value(i,i) (jacobi_solvers.f90:59-61), which a composite answers from the block that
// owns (i,i) (sparse_matrix_composites.f90:465-485)
static int jacobi_setup_composite(sgm_pc pc, sgm_mat A)
{
    hipStream_t st = g_rt.stream;
    if (pc->parts.size() != 1) {
        for (auto &pp : pc->parts) dfree(pp.idiag);
        pc->parts.assign(1, PartPC());
    }
    pc->n = A->nrow;
    pc->parts[0].n = A->nrow;
    if (!pc->parts[0].idiag) SGM_TRY(dalloc(&pc->parts[0].idiag, (size_t)A->nrow + 2));
    const int nrb = (int)A->blk_row_ptr.size() - 1, ncb = (int)A->blk_col_ptr.size() - 1;
    for (int it = 0; it < nrb; ++it)
        for (int jt = 0; jt < ncb; ++jt) {
            const int32_t lo = std::max(A->blk_row_ptr[it], A->blk_col_ptr[jt]);
            const int32_t hi = std::min(A->blk_row_ptr[it + 1], A->blk_col_ptr[jt + 1]);
            if (hi <= lo) continue;               // this block holds no diagonal entry
            sgm_mat C = A->blocks[(size_t)it * ncb + jt];
            double *out = pc->parts[0].idiag + lo;
            if (!C) {
                hipLaunchKernelGGL(k_fill_inf, dim3((hi - lo + kBlock - 1) / kBlock), dim3(kBlock), 0, st, hi - lo, out);
                continue;
            }
            SGM_TRY(jacobi_rows(C->parts[0], C->fmt, lo - A->blk_row_ptr[it], hi - lo, A->blk_row_ptr[it] - A->blk_col_ptr[jt], out));
        }
    SGM_HIP(hipGetLastError());
    return finish();
}

static int jacobi_setup_parts(sgm_pc pc, sgm_mat A)
{
    if (pc->parts.size() != A->parts.size()) {
        for (auto &pp : pc->parts) dfree(pp.idiag);
        pc->parts.assign(A->parts.size(), PartPC());
    }
    pc->n = A->nrow;
    for (size_t ip = 0; ip < A->parts.size(); ++ip) {
        const Part &p = A->parts[ip];
        if (!pc->parts[ip].idiag) SGM_TRY(dalloc(&pc->parts[ip].idiag, (size_t)p.n + 2));
        pc->parts[ip].n = p.n;
        SGM_TRY(jacobi_rows(p, A->fmt, 0, p.n, 0, pc->parts[ip].idiag));
    }
    SGM_HIP(hipGetLastError());
    return finish();
}

// ILDU(0); on a row partition: of every part's diagonal block (block-Jacobi ILDU -- exact parity with the reference holds
// for one part, more parts change the iteration counts).  An ELLPACK operand is factorised through its real entries
// (ell_view, sgm_ildu.hip).
static int ildu_setup(sgm_pc pc, sgm_mat A)
{
    if (A->fmt != SGM_FMT_CSR && A->fmt != SGM_FMT_ELL)
        return fail(SGM_ERR_UNSUPPORTED, "ILDU(0) needs a CSR or ELLPACK matrix");
    if (!pc->abort_sticky) SGM_TRY(dalloc(&pc->abort_sticky, 1));
    SGM_HIP(hipMemsetAsync(pc->abort_sticky, 0, sizeof(int32_t), g_rt.stream));
    if (pc->ild.size() != A->parts.size()) {
        for (auto &S : pc->ild) free_ildu(S);
        pc->ild.assign(A->parts.size(), IlduState());
        for (auto &S0 : pc->ild) S0.opt = pc->opt;
    }
    pc->n = A->nrow;
    for (size_t ip = 0; ip < A->parts.size(); ++ip) SGM_TRY(ildu_setup_part(pc->ild[ip], A->parts[ip], A->fmt));
    return SGM_OK;
}

// the setup proper, on the matrix the factors belong to (A itself, or its colour-ordered copy)
static int pc_setup_ordered(sgm_pc pc, sgm_mat A)
{
    if (A->nrow != A->ncol)      // jacobi_solvers.f90:46-50, ldu_solvers.f90:104-108
        return fail(SGM_ERR_DIMS, "Cannot make a %s solver for a non-square matrix",
                    pc->kind == SGM_PC_JACOBI ? "Jacobi" : "LDU");
    // ILDU on a composite has no reference behaviour to match: its pattern pass walks the composite's get_edges cursor, whose
    // block advance skips block (2,1) and runs past the last column block (sparse_matrix_composites.f90:724-727)
    if (A->fmt == SGM_FMT_COMPOSITE && pc->kind != SGM_PC_JACOBI)
        return fail(SGM_ERR_UNSUPPORTED, "ILDU(0) needs a leaf CSR matrix, not a composite (the reference's own "
                                         "pattern pass is broken on composites)");
    if (A->fmt == SGM_FMT_COMPOSITE) return jacobi_setup_composite(pc, A);
    return pc->kind == SGM_PC_JACOBI ? jacobi_setup_parts(pc, A) : ildu_setup(pc, A);
}

/* sgm_pc_create: the factory alone -- jacobi() / ldu() (jacobi_solvers.f90:23-31, ldu_solvers.f90:73-86) return an object
 * that has seen no matrix yet; options can be set on it before the first sgm_pc_setup builds its sweeps. */
int sgm_pc_create(sgm_pc *out, int32_t kind)
{
    if (!out || (kind != SGM_PC_JACOBI && kind != SGM_PC_ILDU0))      // (SGM_PC_MG needs its prolongations: sgm_mg_create)
        return fail(SGM_ERR_BAD_ARG, "sgm_pc_create: kind is SGM_PC_JACOBI or SGM_PC_ILDU0");
    sgm_pc pc = new sgm_pc_s;
    pc->kind = kind;
    *out = pc;
    return SGM_OK;
}

int sgm_jacobi_create(sgm_pc *out, sgm_mat A)
{
    if (!out) return fail(SGM_ERR_BAD_ARG, "sgm_jacobi_create: null out pointer");
    sgm_pc pc = new sgm_pc_s;
    pc->kind = SGM_PC_JACOBI;
    int rc = sgm_pc_setup(pc, A);
    if (rc != SGM_OK) { sgm_pc_destroy(pc); return rc; }
    *out = pc;
    return SGM_OK;
}

int sgm_ildu0_create(sgm_pc *out, sgm_mat A)
{
    if (!out) return fail(SGM_ERR_BAD_ARG, "sgm_ildu0_create: null out pointer");
    sgm_pc pc = new sgm_pc_s;
    pc->kind = SGM_PC_ILDU0;
    int rc = sgm_pc_setup(pc, A);
    if (rc != SGM_OK) { sgm_pc_destroy(pc); return rc; }
    *out = pc;
    return SGM_OK;
}

/* sgm_pc_set_option: this preconditioner's own copy of "ildu_strips", "ildu_rows", "pipeline_spin_limit" (sgm_set_option
 * only changes what preconditioners created LATER start with).  Which sweeps exist is decided at setup: switching a path
 * off acts from the next apply on, switching one on that was off at setup takes effect at the next sgm_pc_setup. */
int sgm_pc_set_option(sgm_pc pc, const char *name, int value)
{
    if (!pc || !name) return fail(SGM_ERR_BAD_ARG, "sgm_pc_set_option: null argument");
    if (!strcmp(name, "mg_coarse_direct")) {            // the multigrid group: one name, kept by the hierarchy's state
        if (pc->kind != SGM_PC_MG) return fail(SGM_ERR_BAD_ARG, "sgm_pc_set_option: '%s' is an option of multigrid preconditioners", name);
        return mg_set_option(pc->mg, name, value);
    }
    int v = 0;
    SGM_TRY(normalise_option(name, value, &v));
    int *f = pc_option_field(pc->opt, name);
    if (!f) return fail(SGM_ERR_BAD_ARG, "sgm_pc_set_option: '%s' is not a preconditioner option", name);
    *f = v;
    for (auto &S : pc->ild) S.opt = pc->opt;
    return SGM_OK;
}

int sgm_pc_apply(sgm_pc pc, const double *r, double *z, int where)
{
    SGM_TRY(require_init());
    if (!pc || !r || !z) return fail(SGM_ERR_BAD_ARG, "sgm_pc_apply: null argument");
    if (pc->kind == SGM_PC_MG) return mg_apply_vectors(pc->mg, r, z, where);
    if (pc->kind == SGM_PC_JACOBI && pc->parts.size() != 1)
        return fail(SGM_ERR_UNSUPPORTED, "sgm_pc_apply: stand-alone apply needs a single-part matrix");
    // the vectors hold THIS process's rows: all of them on one GPU or an in-process partition, this rank's block when the
    // matrix is distributed over ranks (pc->n is the global count there)
    int64_t nloc = 0;
    if (pc->kind == SGM_PC_ILDU0) for (const auto &S : pc->ild) nloc += S.n;
    else nloc = pc->parts.empty() ? 0 : pc->parts[0].n;
    Staged sr, sz;
    SGM_TRY(stage_in(sr, r, nloc, where, true));
    SGM_TRY(stage_in(sz, z, nloc, where, false));
    // a throw-away matrix view with the right part count for pc_apply_parts (block-Jacobi ILDU on an in-process partition:
    // the caller's vectors are global, part k's slice starts where the rows of the parts before it end)
    const size_t NP = pc->kind == SGM_PC_ILDU0 ? std::max<size_t>(pc->ild.size(), 1) : 1;
    sgm_mat_s view;
    view.parts.resize(NP);
    if (NP == 1) view.parts[0].n = (int32_t)nloc;
    else
        for (size_t ip = 0; ip < NP; ++ip) view.parts[ip].n = pc->ild[ip].n;
    // in-place apply (r == z on the device) through a pipelined sweep: a sweep that gives up has scattered its "not yet
    // written" patterns over z = r by the time anyone notices, so the redo below needs a right-hand side of its own
    Staged rkeep;
    if (sr.dev == sz.dev && pc_abort_word(pc)) {
        SGM_TRY(dalloc(&rkeep.dev, (size_t)nloc));
        rkeep.owned = true;
        SGM_HIP(hipMemcpyAsync(rkeep.dev, sr.dev, (size_t)nloc * sizeof(double), hipMemcpyDeviceToDevice, g_rt.stream));
    }
    std::vector<const double *> rsv(NP);
    std::vector<double *> zsv(NP);
    { int64_t off = 0; for (size_t ip = 0; ip < NP; ++ip) { rsv[ip] = (rkeep.dev ? rkeep.dev : sr.dev) + off; zsv[ip] = sz.dev + off; off += view.parts[ip].n; } }
    const double *const *rs = rsv.data();
    double *const *zs = zsv.data();
    SGM_TRY(pc_apply_parts(pc, &view, rs, zs, nullptr));
    if (int32_t *ab = pc_abort_word(pc)) {
        // a pipelined sweep may give up (bounded waits): look before the result leaves -- one 4-byte copy and a
        // synchronisation against an apply of a millisecond, also in async mode -- and redo it with the level walkers
        int32_t aborted = 0;
        SGM_HIP(hipMemcpyAsync(&aborted, ab, sizeof(int32_t), hipMemcpyDeviceToHost, g_rt.stream));
        SGM_HIP(hipStreamSynchronize(g_rt.stream));
        if (aborted) {
            SGM_TRY(pc_retire_pipelines(pc));
            SGM_TRY(pc_apply_parts(pc, &view, rs, zs, nullptr));
        }
    }
    SGM_TRY(stage_out(sz, z, nloc, where));
    return finish();
}

int sgm_pc_get(sgm_pc pc, const char *name, void *out, size_t bytes, size_t *needed)
{
    if (!pc || !name) return fail(SGM_ERR_BAD_ARG, "sgm_pc_get: null argument");
    const void *src = nullptr;
    size_t sz = 0;
    std::string nm(name);
    static const char kEmpty = 0;
    if (pc->kind == SGM_PC_MG) {
        SGM_TRY(mg_get(pc->mg, name, &src, &sz));
        if (needed) *needed = sz;
        if (out && sz) {
            if (bytes < sz) return fail(SGM_ERR_BAD_ARG, "sgm_pc_get: buffer too small (%zu < %zu)", bytes, sz);
            memcpy(out, src, sz);
        }
        return SGM_OK;
    }
    if (pc->kind == SGM_PC_JACOBI && nm == "idiag") {
        if (pc->parts.size() != 1) return fail(SGM_ERR_UNSUPPORTED, "sgm_pc_get(idiag): single-part only");
        pc->hidiag.resize((size_t)pc->n);
        SGM_HIP(hipStreamSynchronize(g_rt.stream));
        if (pc->n) SGM_HIP(hipMemcpy(pc->hidiag.data(), pc->parts[0].idiag, (size_t)pc->n * 8, hipMemcpyDeviceToHost));
        src = pc->hidiag.data(); sz = pc->hidiag.size() * 8;
    } else if (pc->kind == SGM_PC_ILDU0) {
        if (pc->ild.size() != 1) return fail(SGM_ERR_UNSUPPORTED, "sgm_pc_get: single-part ILDU only");
        IlduState *S = &pc->ild[0];
        if (nm == "Lval" || nm == "Uval" || nm == "D") SGM_TRY(ensure_host_values(S));
        if (nm == "Lptr" || nm == "Lnode" || nm == "Uptr" || nm == "Unode") SGM_TRY(ensure_host_pattern(S));
        if (nm == "Lptr") { src = S->hLptr.data(); sz = S->hLptr.size() * 4; }
        else if (nm == "Lnode") { src = S->hLnode.data(); sz = S->hLnode.size() * 4; }
        else if (nm == "Lval") { src = S->hLval.data(); sz = S->hLval.size() * 8; }
        else if (nm == "Uptr") { src = S->hUptr.data(); sz = S->hUptr.size() * 4; }
        else if (nm == "Unode") { src = S->hUnode.data(); sz = S->hUnode.size() * 4; }
        else if (nm == "Uval") { src = S->hUval.data(); sz = S->hUval.size() * 8; }
        else if (nm == "D") { src = S->hD.data(); sz = S->hD.size() * 8; }
        else if (nm == "strips") {          // strip pipeline in use: {strips per sweep, steps per strip, order variant of L, of U}; zeros = off
            static int32_t sv[4];
            const bool on = S->grid_ok && S->opt.ildu_strips;
            sv[0] = on ? S->gL.NI : 0; sv[1] = on ? S->gL.S : 0; sv[2] = on ? S->gL.order : 0; sv[3] = on ? S->gU.order : 0;
            src = sv; sz = sizeof sv;
        }
        else if (nm == "strip_clocks" && S->grid_ok) {     // per strip of the L sweep: chain start, end (100 MHz ticks)
            static std::vector<long long> ck;
            ck.assign((size_t)2 * S->gL.NI, 0);
            SGM_HIP(hipStreamSynchronize(g_rt.stream));
            for (int32_t i = 0; i < S->gL.NI; ++i)
                SGM_HIP(hipMemcpy(&ck[2 * i], S->gL.edge + (int64_t)i * (S->gL.S + kEdgePad) + S->gL.S + 64, 16, hipMemcpyDeviceToHost));
            src = ck.data(); sz = ck.size() * 8;
        }
        else if (nm == "slabs") {           // slab pipeline in use: {strips, line groups, lines per group, steps, order of L, of U}; zeros = off
            static int32_t sv[6];
            memset(sv, 0, sizeof sv);
            if (S->slab_ok && S->opt.ildu_strips) slab3_info(S->slab, sv);
            src = sv; sz = sizeof sv;
        }
        else if (nm == "slab_clocks" && S->slab_ok) {
            static std::vector<long long> ck;
            SGM_HIP(hipStreamSynchronize(g_rt.stream));
            SGM_TRY(slab3_clocks(S->slab, ck));
            src = ck.data(); sz = ck.size() * 8;
        }
        else if (nm == "perm") {                 // option ildu_reorder: p (1-based; row i of A = row p(i) of the factorised matrix); empty = natural order
            static std::vector<int32_t> hp;
            hp.assign((size_t)(!pc->ro.empty() ? pc->n : 0), 0);
            if (!pc->ro.empty() && pc->n) { SGM_HIP(hipStreamSynchronize(g_rt.stream)); SGM_HIP(hipMemcpy(hp.data(), pc->ro[0].perm, hp.size() * 4, hipMemcpyDeviceToHost)); }
            src = hp.data(); sz = hp.size() * 4;
            if (!sz) src = &kEmpty;
        }
        else if (nm == "reorder_ms") {           // last setup with ildu_reorder: {ordering, permuted copy, setup on the copy, colours}
            static double rm[4];
            rm[0] = pc->reorder_ms[0]; rm[1] = pc->reorder_ms[1]; rm[2] = pc->reorder_ms[2]; rm[3] = !pc->ro.empty() ? pc->ro[0].colors : 0;
            src = rm; sz = sizeof rm;
        }
        else if (nm == "pipeline_retired") {     // how often a pipelined sweep gave up and the pipelines were retired (0 = never)
            static int32_t rv[1];
            rv[0] = pc->retired;
            src = rv; sz = sizeof rv;
        }
        else if (nm == "row_levels") {           // row-space level path in use: {1, launches of the L sweep, of the U sweep}; zeros = off
            static int32_t rl[3];
            const bool on = !(S->opt.ildu_strips && (S->grid_ok || S->slab_ok)) && rows_serve(S);
            const bool fu = S->opt.ildu_rows == 1;
            rl[0] = on;
            rl[1] = on ? (int32_t)S->L.row_levels.size() - (fu && S->rows_n0 > 0 ? 1 : 0) : 0;
            rl[2] = on ? (int32_t)S->U.row_levels.size() - (fu && S->rows_fin ? 1 : 0) : 0;
            src = rl; sz = sizeof rl;
        }
        else if (nm == "levels") {
            SGM_TRY(ensure_levels(&pc->ild[0]));
            static int32_t lv[2];
            lv[0] = (int32_t)S->L.level_ptr.size() - 1;
            lv[1] = (int32_t)S->U.level_ptr.size() - 1;
            src = lv; sz = sizeof lv;
        }
    }
    const bool known = nm == "strips" || nm == "strip_clocks" || nm == "slabs" || nm == "slab_clocks" || nm == "pipeline_retired" || nm == "idiag" || nm == "Lptr" || nm == "Lnode" || nm == "Lval" || nm == "Uptr" ||
                       nm == "Unode" || nm == "Uval" || nm == "D" || nm == "levels" || nm == "row_levels" || nm == "perm" || nm == "reorder_ms";
    if (!known || (!src && sz)) return fail(SGM_ERR_BAD_ARG, "sgm_pc_get: unknown array '%s'", name);
    if (!src) src = &kEmpty;
    if (needed) *needed = sz;
    if (out && sz) {
        if (bytes < sz) return fail(SGM_ERR_BAD_ARG, "sgm_pc_get: buffer too small (%zu < %zu)", bytes, sz);
        memcpy(out, src, sz);
    }
    return SGM_OK;
}

/* sgm_pc_info: which sweeps serve part `part` of this preconditioner and what an apply costs -- so that a caller who builds
 * `ldu()` the way the reference's tests do (solver_test_incomplete_cholesky.f90:137-141) can SEE that the factors of a
 * naturally ordered grid are a dependency chain before paying for it.
 *   out[0], out[1]  dependency levels of L and of U (the row recurrences of ldu_solvers.f90:227-236, :254-263 can start a level
 *                   only when the one before it is done); 1 for a diagonal preconditioner
 *   out[2]          path: 0 diagonal scaling (Jacobi), 1 row-space sweeps (one launch per level, bandwidth-bound), 2 strip
 *                   pipeline (2-D grid factors), 3 slab pipeline (3-D grid factors), 4 level walkers
 *   out[3]          colours of the ordering the factors belong to (option ildu_reorder); 0 = the matrix's own order
 *   est_us          estimated microseconds per apply on this GPU (from the path's measured constants)
 *   path_name       the same in words */
int sgm_pc_info(sgm_pc pc, int32_t part, int32_t *out4, double *est_us, char *path_name, int len)
{
    if (!pc) return fail(SGM_ERR_BAD_ARG, "sgm_pc_info: null preconditioner");
    if (pc->kind == SGM_PC_MG) {
        if (part != 0) return fail(SGM_ERR_BAD_ARG, "sgm_pc_info: part %d", part);
        return mg_info(pc->mg, out4, est_us, path_name, len > 0 ? (size_t)len : 0);
    }
    int32_t o[4] = {1, 1, 0, 0};
    double us = 0.0;
    char nm[160] = "";
    if (pc->kind == SGM_PC_JACOBI) {
        if (part < 0 || (size_t)part >= std::max<size_t>(pc->parts.size(), 1)) return fail(SGM_ERR_BAD_ARG, "sgm_pc_info: part %d", part);
        us = 24.0 * pc->n / 5.5e6;
        snprintf(nm, sizeof nm, "diagonal scaling, 1 level");
    } else {
        if (part < 0 || (size_t)part >= pc->ild.size()) return fail(SGM_ERR_BAD_ARG, "sgm_pc_info: part %d of %zu (set the preconditioner up first)", part, pc->ild.size());
        IlduState *S = &pc->ild[(size_t)part];
        o[3] = (size_t)part < pc->ro.size() ? pc->ro[(size_t)part].colors : 0;
        if (S->grid_ok && S->opt.ildu_strips) {
            // a w x nj grid in natural order: rows (i, j) with i + j equal form a level
            o[0] = o[1] = S->gL.w + S->gL.nj - 1;
            o[2] = 2;
            us = 2.0 * (0.075 * S->gL.S + 9.9 * std::max(0, S->gL.NI - 1)) + 3.0 * 16.0 * S->gL.NP / 5.5e6;
            snprintf(nm, sizeof nm, "strip pipeline, %d levels", o[0]);
        } else if (S->slab_ok && S->opt.ildu_strips) {
            int32_t w = 0, h = 0, sv[6] = {0, 0, 0, 0, 0, 0};
            slab3_dims(S->slab, &w, &h);
            slab3_info(S->slab, sv);
            const int32_t nk = (int32_t)((S->n + (int64_t)w * h - 1) / ((int64_t)w * h));
            o[0] = o[1] = w + h + nk - 2;
            o[2] = 3;
            us = 2.0 * (0.135 * sv[3] + 6.5 * std::max(0, sv[1] - 1)) + 3.0 * 16.0 * S->n / 5.5e6;
            snprintf(nm, sizeof nm, "slab pipeline, %d levels", o[0]);
        } else {
            SGM_TRY(ensure_levels(S));
            o[0] = (int32_t)S->L.level_ptr.size() - 1;
            o[1] = (int32_t)S->U.level_ptr.size() - 1;
            if (rows_serve(S)) {
                o[2] = 1;
                // one launch per level and sweep (+ the two permutations of a stand-alone apply in a colour order), about 4.5 us each
                // when the levels are small: a 2-level apply of 1e5 rows is 32 us of launches around 2 us of traffic
                us = (12.0 * ((double)S->nnzL + S->nnzU) + 56.0 * S->n) / 5.5e6 + 4.5 * ((double)o[0] + o[1] + (o[3] ? 2 : 0));
                snprintf(nm, sizeof nm, "row space, %d levels", std::max(o[0], o[1]));
            } else {
                o[2] = 4;
                // (0.3 us per level and sweep, 0.16 where the levels are a wave wide at most -- chains --, measured on factors of
                //  1e3 ... 4e5 levels: tools/pc_survey.py)
                const double per_level = (int64_t)std::max(o[0], 1) * 64 >= (int64_t)S->n ? 0.16 : 0.30;
                us = per_level * ((double)o[0] + o[1]) + (12.0 * ((double)S->nnzL + S->nnzU) + 56.0 * S->n) / 5.5e6;
                snprintf(nm, sizeof nm, "level walkers, %d levels", std::max(o[0], o[1]));
            }
        }
    }
    // a colour-ordered part: the kernel the PRODUCT on the permuted copy runs with (the solvers iterate on that copy)
    if (pc->kind == SGM_PC_ILDU0 && pc->Ap && (size_t)part < pc->Ap->parts.size() && (size_t)part < pc->ro.size() && pc->ro[(size_t)part].colors) {
        char kn[64];
        part_kernel_name(pc->Ap->parts[(size_t)part], pc->Ap->fmt, kn, sizeof kn);
        const size_t used = strlen(nm);
        snprintf(nm + used, sizeof nm - used, "; product of the ordered part: %s", kn);
    }
    if (out4) memcpy(out4, o, sizeof o);
    if (est_us) *est_us = us;
    if (path_name && len > 0) snprintf(path_name, (size_t)len, "%s", nm);
    return SGM_OK;
}

int sgm_pc_destroy(sgm_pc pc)
{
    if (!pc) return SGM_OK;
    for (auto &pp : pc->parts) dfree(pp.idiag);
    for (auto &S : pc->ild) free_ildu(S);
    dfree(pc->abort_sticky);
    free_reorder(pc);
    if (pc->Ap) sgm_mat_destroy(pc->Ap);
    mg_free(pc->mg);
    delete pc;
    return SGM_OK;
}

}  // extern "C"
