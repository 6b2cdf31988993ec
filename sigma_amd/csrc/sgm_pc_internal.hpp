// Private to the preconditioner family: sgm_pc.hip (the object, Jacobi, the colour re-ordering, the pc_* functions of the
// Krylov loops, the C ABI), sgm_ildu.hip (ILDU(0) setup) and sgm_trsv.hip (the triangular sweeps).  The state of an ILDU(0)
// preconditioner and the host functions the three call across; sgm_trsv3.hip (the slab pipeline) keeps its own state behind
// the slab3_* functions of sgm_internal.hpp; sgm_mg.hip and sgm_mg_direct.hip share the mg_direct_* functions at the end.
// The library is built without relocatable device code: a kernel is launched
// only from the file that defines it, so everything declared here is a host function.  (The device pieces the strip and the
// slab pipeline have in common -- abort, empty marker, DPP shift, the scatter out of position space -- are inline / static in
// sgm_trsv_device.hpp, which those two files include: one definition, a copy per file.)
#pragma once
#include "sgm_internal.hpp"

namespace sgm {

constexpr int kTrsvBlock = 1024;
constexpr int kNarrow = 4096;        // levels with <= this many rows are walked by one workgroup (4 rows per lane)
constexpr int kRing = 8192;          // LDS ring of recent results (64 KiB): covers two narrow levels
constexpr int kInline = 4;           // dependencies stored inside the row record
constexpr int kRowLevels = 32;       // factors of at most this many levels are swept in row space, one launch per level
constexpr int kStripSpinLimit = 1 << 22;   // strip / slab sweeps: polls before a wait gives up (option pipeline_spin_limit = 0)
constexpr int kEdgePad = 72;         // an edge row of a strip: S + 64 values (a strip reads its left neighbour's step t + 63), 2 clocks

struct TrsvRec {                     // one row of a triangular factor, in level order (64 bytes)
    int32_t cnt, k0;                 // entries of the row; offset of its entries in pq / pv
    int32_t q[kInline];              // position (in level order) of the first dependencies
    double v[kInline];               // their values
    int32_t pad[2];
};
static_assert(sizeof(TrsvRec) == 64, "TrsvRec is one 64-byte record");

struct TriFactor {                   // strictly triangular factor on the device, level order
    int32_t *order = nullptr;        // device: pos -> row
    TrsvRec *recs = nullptr;         // device: n records
    int32_t *pq = nullptr;           // device: dependency positions of ALL entries, rows in level order
    double *pv = nullptr;            // device: their values
    int32_t *level_ptr_dev = nullptr;
    int32_t *wq = nullptr;           // device: dependency POSITIONS, kInline slots, slot-major (-1 = none): wide levels
    uint32_t *dq32 = nullptr;        // device: low halves of dq, contiguous (runs with <= 2 dependencies per row)
    uint64_t *dq = nullptr;          // device: ring-walker copy, 4 x 16-bit position deltas per row (0 = none)
    double *dv = nullptr;            // device: ring-walker copy, kInline value slots, slot-major (slot*n + pos)
    std::vector<uint64_t> h_dq;
    size_t nstride = 0;              // entries per value slot of dv (n + padding)
    std::vector<int32_t> level_ptr;  // host: offsets into the level order per level
    std::vector<int32_t> h_order, h_pos;             // host: pos -> row, row -> pos
    int32_t *src = nullptr;                          // device: level-order entry -> entry of the factor's val array
    std::vector<TrsvRec> h_recs;
    std::vector<int32_t> h_pq;
    // cls: -1 = one wave (levels of <= 64 rows), 0..2 = 256/512/1024 threads (one row per lane), 3/4 = 2/4 rows per lane; ring: k_trsv_walk_ring
    // applies; c: most dependencies of a row in the run
    struct Launch { int32_t l0, l1; bool narrow; int cls; bool ring; int c; };
    std::vector<Launch> schedule;
    // row-space copy for factors of a few levels (colour orderings: one per colour): dependency ROWS and values, rc slots,
    // slot-major over the level order -- the sweeps then run on the vectors themselves, one launch per level (k_trsv_rows)
    struct RowLevel { int32_t b, e, c, row0; };      // positions [b, e); most entries of a row; row0 >= 0: rows row0, row0+1, ...
    std::vector<RowLevel> row_levels;
    bool rows_on = false;
    bool have_levels = false, have_walkers = false;   // index work done: levels (+ row-space copy) / the walkers' structures
    int rc = 0;
    int32_t *rq = nullptr;
    double *rv = nullptr;
    // the dependency rows once more as 4-bit codes (rc <= 8 and at most 15 distinct offsets "dependency row - own row" in the
    // whole factor -- any stencil matrix in any of the reference's orderings): rcode[p] = eight codes of position p (15 =
    // no entry), rdict = the offsets.  4 bytes per row where rq holds 4 * rc: the fused PCG sweeps read these.
    uint32_t *rcode = nullptr;
    int32_t *rdict = nullptr;
    int nrdict = 0;
};

// A strictly triangular factor whose rows depend only on the previous row (r-1) and on the row one grid
// line back (r-w): ILDU(0) factors of 5-point / banded matrices in natural order.  The grid is cut into
// STRIPS of 64 columns; a strip's rows are re-laid in a skewed order: lane l of the strip's chain wave handles
// column i0+l and, at step t, grid line t-l, so that the (i-1, j) neighbour is lane l-1's result of the previous
// step (one DPP shift), the (i, j-1) neighbour the lane's own, and every access of a step is one coalesced
// line of the skewed layout (position = strip base + step * 64 + lane).  See k_trsv_strip.
struct StripRec { double cS, cW, rhs; uint64_t code; };    // 32 bytes per (step, lane): coefficients of the r-w / r-1
                                                           // dependency, right-hand side, bit0 has r-w, bit1 has r-1,
                                                           // bit2 r-1 comes FIRST in the row's stored order
struct GridTri {
    bool on = false;
    int32_t w = 0, nj = 0, NI = 0, S = 0;                       // grid width / lines, strips, steps per strip
    int order = 2;                                              // 0 / 1: every two-term row has its r-w / r-1 term first; 2: mixed
    int64_t NP = 0;                                             // positions (incl. padding) = NI * S * 64
    StripRec *rec = nullptr;                                    // device
    int32_t *row = nullptr;                                     // device: position -> row (-1 = padding)
    double *edge = nullptr;                                     // device: NI x (S + 72): lane 63's result of every step (kEdgeEmpty = not yet), 2 clocks
    int32_t *progress = nullptr;                                // device: NI + 1: steps whose edge values are published; [NI] = abort
    int32_t *pos = nullptr;                                     // device: row -> position (index work only; freed after it)
    int32_t *srcS = nullptr, *srcW = nullptr;                   // device: position -> entry of the factor's val array (-1 = none)
    uint8_t *code = nullptr;                                    // device: presence / order bits per position
};

struct PartPC {
    double *idiag = nullptr;
    int32_t n = 0;                   // rows of the part (on a matrix distributed over ranks: this rank's, not the global count)
};

// ILDU(0) of one diagonal block (the whole matrix on one GPU; with a row partition, the owned
// rows x owned columns of each part: block-Jacobi ILDU)
struct IlduState {
    PcOptions opt = g_opt.pc;        // the owning preconditioner's options (kept equal to sgm_pc_s::opt)
    int32_t n = 0;
    TriFactor L, U;
    double *D = nullptr;
    double *xpL = nullptr, *xpU = nullptr, *Dp = nullptr;   // level-order work vectors, D in U's level order
    int32_t *mapLU = nullptr;                                // U position -> L position of the same row
    std::vector<int32_t> hLptr, hLnode, hUptr, hUnode;      // 1-based, as the reference holds them
    // the factors live on the device (0-based pattern copies, values in the pattern's order; D = the array above): the
    // factorisation runs there, level by level of L's dependency graph (L.order / L.level_ptr), and every structure the
    // applies read is filled from these by kernels.  Host copies of the VALUES only on request (sgm_pc_get, self-check).
    int32_t *dLptr = nullptr, *dLnode = nullptr, *dUptr = nullptr, *dUnode = nullptr;
    double *dLval = nullptr, *dUval = nullptr;
    std::vector<double> hLval, hUval, hD;
    bool host_vals = false;
    int32_t maxL = 0, maxU = 0;                              // longest row of each factor
    int32_t nnzL = 0, nnzU = 0;
    // grid-like factors (found on the device, grid_detect_device): the factorisation walks the anti-diagonals of the grid;
    // L's true dependency levels are then only built if something asks for them
    int32_t *forder = nullptr;
    std::vector<int32_t> flevel_ptr;
    int32_t dev_wl = 0, dev_wu = 0;                          // grid widths found on the device (0: not grid-like / not looked)
    bool dev_slab = false;                                   // a 3-D grid's factors, found on the device
    // strip-pipeline path (both factors grid-like, see GridTri): results in position space and the L -> U hand-over
    GridTri gL, gU;
    double *gxL = nullptr, *gxU = nullptr, *gDp = nullptr;
    int32_t *gmapLU = nullptr;
    bool grid_ok = false;                                   // the strip path reproduced the level-scheduled apply at setup
    // slab-pipeline path (3-D grid factors, sgm_trsv3.hip); slab_ok: it reproduced the level-scheduled apply at setup
    Slab3 *slab = nullptr;
    bool slab_ok = false;
    // the level-scheduled structures are built on first need when a pipelined path serves the pattern
    bool levels_ready = false, levels_pattern = false;
    bool walk_ready = false, walk_pattern = false;          // the same for the level walkers' structures (ensure_walkers)
    // row-space sweeps (apply_rows): L's level 0 is the entry-less run of rows 0 .. rows_n0-1 (0: it is not); L's last level
    // and U's level 0 are the same entry-less run of rows
    int32_t rows_n0 = 0;
    bool rows_fin = false;
};

}  // namespace sgm

struct sgm_pc_s {
    int kind = 0;
    int32_t n = 0;
    std::vector<sgm::PartPC> parts;  // jacobi
    std::vector<sgm::IlduState> ild; // ildu: one block per part
    std::vector<double> hidiag;
    int32_t *abort_sticky = nullptr; // device: set by a pipelined triangular sweep that gave up; cleared by the host only
    int retired = 0;                 // pipelines switched off after an abort (diagnostics: sgm_pc_get "pipeline_retired")
    sgm::PcOptions opt = sgm::g_opt.pc;   // this preconditioner's options: the defaults at its creation, then sgm_pc_set_option
    // option "ildu_reorder": the factors are those of P A P^T -- on a row partition of P_k A_kk P_k^T for every part k, each
    // part ordering its own diagonal block (no communication; halo columns keep their numbers).  perm = p (1-based, local:
    // row i of the part is row p(i) of the permuted part), rp / zp = right-hand side and result in the permuted order
    // hmap (device, n_halo entries; null: the halo keeps its order) = the part's halo slots re-ordered by the permuted rows they
    // attach to; send_order[k] (device) = where entry j this part sends over its k-th link goes in the RECEIVER's re-ordered halo
    struct Reorder {
        int32_t *perm = nullptr; double *rp = nullptr, *zp = nullptr; int32_t n = 0, colors = 0;
        int32_t *hmap = nullptr; std::vector<int32_t> hmap_host; std::vector<int32_t *> send_order;
    };
    std::vector<Reorder> ro;            // one per part; empty = natural order
    uint64_t ro_serial = 0, ro_pattern = 0;     // the matrix (serial number, pattern version) the orderings were found for
    double reorder_ms[3] = {0, 0, 0};  // last setup: ordering, permuted copy, (factorisation is in the regular phases)
    // the permuted matrix itself, kept (with A's kernel forms) for the Krylov solvers: they run the whole solve in the
    // permuted order -- b and x permuted once each way -- instead of permuting r and z in every apply (in_permuted: vectors
    // handed to pc_apply_parts are in that order already)
    sgm_mat Ap = nullptr;
    uint64_t Ap_serial = 0, Ap_version = 0;            // ... of the matrix it is the permutation of
    bool in_permuted = false;
    sgm::MgState *mg = nullptr;        // SGM_PC_MG: the hierarchy and its work vectors (sgm_mg.hip)
};

namespace sgm {

// Row-space tables rq / rv, slice-major: the rc slots of 512 consecutive positions lie side by side, so a sweep's tile reads ONE
// contiguous run (rc * 6 KiB for both tables) instead of 2 * rc streams a whole vector apart.  (Measured in round 4 against
// the slot-major layout it replaced: the same time -- the sweeps are not bound by the number of open streams.)  Size <=
// (n + 511) * rc entries.
__host__ __device__ inline size_t rs_at(int c, uint32_t p, int rc) { return ((size_t)(p >> 9) * rc + c) * 512 + (p & 511u); }

// which sweeps serve a block (the selection rules, shared by the applies, the setup and the getters)
inline bool rows_serve(const IlduState *S) { return S->opt.ildu_rows && S->levels_ready && S->L.rows_on && S->U.rows_on; }
// both factors exactly two row-space levels, the outer ones entry-less (a two-colour ordering): k_trsv_rows_cg's case
inline bool rows_two_level(const IlduState *S)
{
    return rows_serve(S) && S->opt.ildu_rows == 1 && S->rows_n0 > 0 && S->rows_fin && S->L.row_levels.size() == 2 && S->U.row_levels.size() == 2;
}

// ---- sgm_ildu.hip: setup of one block, and what is built from its factors on first need
// fmt: the matrix's format (SGM_FMT_CSR / SGM_FMT_ELL); P: the part whose diagonal block is factorised
int ildu_setup_part(IlduState &S, const Part &P, int32_t fmt);
void free_ildu(IlduState &S);
int ensure_levels(IlduState *S);         // dependency levels, row-space copies, the row-space work vector
int ensure_walkers(IlduState *S);        // the level walkers' structures (ensure_levels included)
int ensure_host_pattern(IlduState *S);   // hLptr .. hUnode (1-based)
int ensure_host_values(IlduState *S);    // hLval, hUval, hD

// ---- sgm_trsv.hip: z = (I+U)^-1 D^-1 (I+L)^-1 r on device vectors, stream-ordered -- the caller has chosen the path and
// built its structures (the interface of a pipeline towards setup mirrors slab3_* in sgm_internal.hpp)
void apply_grid(const IlduState *S, const double *r, double *z, const int *flag, int spin_limit, int32_t *sticky);   // strip pipeline
void grid_lower_result(const IlduState *S, double *dst);        // (I+L)^-1 r of the last apply_grid, in row order (self-check)
void apply_levels(const IlduState *S, const double *r, double *z, const int *flag);     // level walkers
void apply_rows(const IlduState *S, const double *r, double *z, const int *flag);       // row-space levels
// PCG's r -= alpha q ; z = M^-1 r ; partial sums of r.z in the two launches of a two-level factorisation (rows_two_level)
void rows_cg_fused(const IlduState *S, ScalarRef res2, ScalarRef dpr, const double *q, double *r, double *z, double *part, int *count,
                   const int *flag, int gen);
void scale_by(int64_t n, const double *d, const double *r, double *z, const int *flag);      // z = d * r: the Jacobi apply

// ---- sgm_mg_direct.hip: the dense inverse of multigrid's coarsest level, used by sgm_mg.hip
struct MgDirect;
int mg_direct_setup(MgDirect **out, sgm_mat A);      // Gauss-Jordan with partial pivoting; a refusal leaves *out null
int mg_direct_apply(const MgDirect *D, const double *b, double *x, const int *flag);      // x = Ainv b, b != x, stream-ordered
int mg_direct_get(MgDirect *D, const char *name, const void **src, size_t *sz);           // "mg_coarse_inverse" / "mg_coarse_pivots"
int mg_direct_rows(const MgDirect *D);
double mg_direct_invert_ms(const MgDirect *D);
void mg_direct_free(MgDirect *D);

}  // namespace sgm
