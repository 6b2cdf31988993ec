// Device pieces the two pipelined triangular sweeps share: the strip pipeline (k_trsv_strip, sgm_trsv.hip) and the slab
// pipeline (k_trsv_slab, sgm_trsv3.hip).  The library is built without relocatable device code, so everything here is
// inline or static: each of the two files gets its own copy.
#pragma once
#include "sgm_internal.hpp"

namespace sgm {

typedef double f64x2s __attribute__((ext_vector_type(2)));

// "not yet written": a SIGNALLING NaN no subtraction can produce (arithmetic quiets NaNs), so the values a sweep hands to its
// neighbour -- a strip's edge values, a slab's results -- are their own flags
constexpr unsigned long long kEdgeEmpty = 0x7FF4A5A5A5A5A5A5ull;

// A wait that gives up marks the sweep (abort_word: cleared by the next sweep's gather, read by the setup self-check) AND the
// preconditioner's sticky word, which only the host clears: the solvers and sgm_pc_apply read it whenever they synchronise
// anyway, redo the work with the level walkers and retire the pipeline for this handle -- a result the library itself
// spoiled never reaches the caller (sgm::pc_abort_word / pc_retire_pipelines).
__device__ inline void raise_abort(int32_t *abort_word, int32_t *sticky)
{
    __hip_atomic_store(abort_word, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (sticky) __hip_atomic_store(sticky, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ inline double dpp_shift_up(double v, double lane0)
{
    // lane l receives lane l-1's v (wave_shr:1 crosses the 16-lane DPP rows on gfx9); lane 0 receives lane0
    const int lo = __double2loint(v), hi = __double2hiint(v);
    const int slo = __builtin_amdgcn_update_dpp(__double2loint(lane0), lo, 0x138, 0xf, 0xf, false);
    const int shi = __builtin_amdgcn_update_dpp(__double2hiint(lane0), hi, 0x138, 0xf, 0xf, false);
    return __hiloint2double(shi, slo);
}

// out of position space: dst[row of position p] = xp[p] (padding positions have no row)
static __global__ void k_pos_scatter(int64_t np, double *__restrict__ dst, const double *__restrict__ xp,
                                     const int32_t *__restrict__ row, const int *flag)
{
    if (flag && *flag) return;
    int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; p < np; p += stride) { const int32_t r = row[p]; if (r >= 0) dst[r] = xp[p]; }
}

}  // namespace sgm
