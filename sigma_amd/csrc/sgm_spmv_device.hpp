// Device pieces every product kernel shares (sgm_spmv.hip, sgm_mg.hip, sgm_ellcb.hip): the stop test, the workgroup ->
// slice / row-block maps, the start and finish of a row under the numerics contract of sgm_spmv.hip, the fused-dot
// partials, and the row sums of the two dictionary-coded sliced layouts.  Each is defined here once; all are inlined.
#pragma once
#include "sgm_spmv_select.hpp"

namespace sgm {

// ---- stop flag: a product launched for generation `gen` does nothing once the flag holds a generation <= gen.
// stop_flag only REQUESTS the flag; kernels that start other loads before they wait for it test stop_hit later.
__device__ __forceinline__ int stop_flag(const int *__restrict__ flag_done) { return flag_done ? *flag_done : 0; }
__device__ __forceinline__ bool stop_hit(int st, int gen) { return st && gen >= st; }
__device__ __forceinline__ bool stopped(const int *__restrict__ flag_done, int gen)
{
    if (flag_done) {
        const int st = *flag_done;
        if (stop_hit(st, gen)) return true;
    }
    return false;
}

// ---- work-group -> row-block map.  Blocks b and b+8 share an XCD (round-robin dispatch), so
// the blocks of one XCD take CONSECUTIVE row blocks inside each sweep of the grid: the x
// entries they gather (own rows +- the stencil reach) stay in that XCD's 4 MiB L2.
// Bijective because the grid is a multiple of 8.  Placement only changes speed.
__device__ __forceinline__ int64_t rowblock_of(int it, int b, int grid)
{
    const int per = grid >> 3;
    return (int64_t)it * grid + (int64_t)(b & 7) * per + (b >> 3);
}

// ---- the slice a workgroup of a sliced kernel starts with (it then strides by the grid).  mode 0: round-robin.
// mode 1 (slice_map_mode): XCD-block-cyclic -- inside every window of 8 G consecutive slices the workgroups of one XCD
// (blockIdx % 8) take G = 32 consecutive slices, so the x entries a slice shares with its neighbours (2-D stencils:
// +-nx rows = a few slices away) are fetched into ONE XCD's L2 instead of several (C2: 103.8 -> 99-100 us).  The
// launcher only asks for it when the grid is a multiple of 8 G (the map is then a permutation).
__device__ __forceinline__ int64_t first_slice(int mode)
{
    if (!mode) return blockIdx.x;
    constexpr int G = kSliceMapGroup;
    const int xcd = blockIdx.x & 7, loc = blockIdx.x >> 3;
    return (int64_t)(loc / G) * (8 * G) + xcd * G + loc % G;
}

// ---- a row under the numerics contract: the sum starts at 0.0 and y(i) = 0.0 + z (matvec), y(i) = y0 + z (matvec_add),
// or -- chain -- the sum continues from y0 and is y(i) itself (transpose products).  Where y0 and w(i) are loaded and
// how y(i) is stored stays with each kernel: that placement is tuned per kernel (registers, see k_csr_do).
template <bool ADD>
__device__ __forceinline__ double row_start(double y0, bool chain) { return (ADD && chain) ? y0 : 0.0; }
template <bool ADD>
__device__ __forceinline__ double row_value(double y0, double z, bool chain) { return ADD ? (chain ? z : y0 + z) : 0.0 + z; }
template <bool DOT_W, bool DOT_YY>
__device__ __forceinline__ void dots_add(double wv, double yi, double &dwy, double &dyy)
{
    if (DOT_W) dwy += wv * yi;
    if (DOT_YY) dyy += yi * yi;
}
// the workgroup's partial sums of w.y and y.y, one slot per workgroup; red: BLOCK / 64 doubles of LDS
template <int BLOCK, bool DOT_W, bool DOT_YY>
__device__ __forceinline__ void dots_write(double dwy, double dyy, double *red, double *__restrict__ part_wy, double *__restrict__ part_yy)
{
    if (DOT_W) {
        const double t = block_sum<BLOCK>(dwy, red);
        if (threadIdx.x == 0) part_wy[blockIdx.x] = t;
    }
    if (DOT_YY) {
        const double t = block_sum<BLOCK>(dyy, red);
        if (threadIdx.x == 0) part_yy[blockIdx.x] = t;
    }
}

// ---- the two adjacent rows row, row + 1 of a lane of a sliced kernel (row even: 16-byte accesses; the last row of an
// odd n stands alone)
template <bool ADD>
__device__ __forceinline__ f64x2 pair_load_y0(const double *__restrict__ y, int32_t row, int32_t n)
{
    f64x2 y0 = {0.0, 0.0};
    if (ADD) {
        if (row + 1 < n) y0 = *reinterpret_cast<const f64x2 *>(y + row);
        else if (row < n) y0.x = y[row];
    }
    return y0;
}
template <bool ADD>
__device__ __forceinline__ f64x2 pair_start(f64x2 y0, bool chain)
{
    f64x2 z;
    z.x = row_start<ADD>(y0.x, chain);
    z.y = row_start<ADD>(y0.y, chain);
    return z;
}
template <bool ADD, bool DOT_W, bool DOT_YY>
__device__ __forceinline__ void pair_finish(double *__restrict__ y, const double *__restrict__ w, int32_t row, int32_t n, f64x2 y0, f64x2 z,
                                            bool chain, double &dwy, double &dyy)
{
    f64x2 yi;
    yi.x = row_value<ADD>(y0.x, z.x, chain);
    yi.y = row_value<ADD>(y0.y, z.y, chain);
    if (row + 1 < n) {
        __builtin_nontemporal_store(yi, reinterpret_cast<f64x2 *>(y + row));
        if (DOT_W) { const f64x2 wv = *reinterpret_cast<const f64x2 *>(w + row); dwy += wv.x * yi.x; dwy += wv.y * yi.y; }
        if (DOT_YY) { dyy += yi.x * yi.x; dyy += yi.y * yi.y; }
    } else if (row < n) {
        __builtin_nontemporal_store(yi.x, y + row);
        dots_add<DOT_W, DOT_YY>(DOT_W ? w[row] : 0.0, yi.x, dwy, dyy);
    }
}

// ---- row sums of the 4-bit sliced form (k_csr_sl, k_mg_sl): cw = the code words of rows row, row + 1 (eight 4-bit
// dictionary codes each, 15 = no entry), v = their W value pairs, dl = the dictionary in LDS.  All 2 W gathers of x are
// requested first; then the products are rounded one by one and added to z in stored order.
template <int W>
__device__ __forceinline__ f64x2 sl_row_sums(f64x2 z, u32x2 cw, const f64x2 (&v)[W], const double *__restrict__ x, int32_t row,
                                             const int32_t *dl)
{
    double xa[W], xb[W];
#pragma unroll
    for (int u = 0; u < W; ++u) {
        const uint32_t ca = (cw.x >> (4 * u)) & 15u, cb = (cw.y >> (4 * u)) & 15u;
        xa[u] = ca != 15u ? x[row + dl[ca]] : 0.0;
        xb[u] = cb != 15u ? x[row + 1 + dl[cb]] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < W; ++u) {
        if (((cw.x >> (4 * u)) & 15u) != 15u) z.x = z.x + v[u].x * xa[u];
        if (((cw.y >> (4 * u)) & 15u) != 15u) z.y = z.y + v[u].y * xb[u];
    }
    return z;
}

// ---- row sums of the 1-byte sliced form (k_csr_slb, k_mg_slb) for the lane's rows row, row + 1 of slice sl: values
// slot-major, W per row; per chunk of 8 slots the 8 code bytes of a row sit together (255 = no entry), so one 16-byte load
// brings the codes of both rows.  Slots are walked in stored order.
template <int W>
__device__ __forceinline__ f64x2 slb_row_sums(f64x2 z, const double *__restrict__ sval, const uint8_t *__restrict__ sbcode, int64_t sl, int tid,
                                              const double *__restrict__ x, int32_t row, const int32_t *dl)
{
    constexpr int BLOCK = kSlRows / 2;
    constexpr int NCH = (W + 7) / 8;
    const f64x2 *vb = reinterpret_cast<const f64x2 *>(sval + sl * (int64_t)W * kSlRows) + tid;
    const u32x4s *cb = reinterpret_cast<const u32x4s *>(sbcode + sl * (int64_t)(NCH * 8 * kSlRows)) + tid;      // 16 bytes: rows 2t, 2t+1
    // chunks of 8 slots.  Unrolled over all chunks the compiler keeps every slot live (237 VGPRs at W = 27, two waves
    // per SIMD) -- which still wins up to W = 28: all of a wave's loads are in flight at once; beyond that a rolled loop
    auto chunk = [&](int c, auto cnt_tag) {
        constexpr int CNT = decltype(cnt_tag)::value;
        f64x2 v[CNT];
        double xa[CNT], xb[CNT];
        const u32x4s cw = __builtin_nontemporal_load(cb + c * BLOCK);
#pragma unroll
        for (int u = 0; u < CNT; ++u) v[u] = __builtin_nontemporal_load(vb + (c * 8 + u) * BLOCK);
#pragma unroll
        for (int u = 0; u < CNT; ++u) {
            const uint32_t ca = ((u < 4 ? cw.x : cw.y) >> (8 * (u & 3))) & 255u;
            const uint32_t cbv = ((u < 4 ? cw.z : cw.w) >> (8 * (u & 3))) & 255u;
            xa[u] = ca != 255u ? x[row + dl[ca]] : 0.0;
            xb[u] = cbv != 255u ? x[row + 1 + dl[cbv]] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < CNT; ++u) {
            const uint32_t ca = ((u < 4 ? cw.x : cw.y) >> (8 * (u & 3))) & 255u;
            const uint32_t cbv = ((u < 4 ? cw.z : cw.w) >> (8 * (u & 3))) & 255u;
            if (ca != 255u) z.x = z.x + v[u].x * xa[u];
            if (cbv != 255u) z.y = z.y + v[u].y * xb[u];
        }
    };
    if (W > 28) {       // (measured on the 160^3 27-point matrix, rolled vs unrolled: W = 32: 249 vs 281 us; 28: 237 vs 224; 27: 229 vs 218)
#pragma unroll 1
        for (int c = 0; c < W / 8; ++c) chunk(c, std::integral_constant<int, 8>{});
    } else {
#pragma unroll
        for (int c = 0; c < W / 8; ++c) chunk(c, std::integral_constant<int, 8>{});
    }
    if (W % 8) chunk(W / 8, std::integral_constant<int, (W % 8 ? W % 8 : 8)>{});
    return z;
}

}  // namespace sgm
