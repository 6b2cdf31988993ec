// LSQR (Paige-Saunders, Golub-Kahan bidiagonalisation) on the device: min |A x - b|_2 for a RECTANGULAR A, optionally damped.  No
// reference counterpart; the contract is the loop in include/sigma_hip.h (sgm_lsqr_create) and DESIGN.md section 9j, restated by
// tests/lsqr_restated.py.  A launch loop in the style of run_minres (sgm_minres.hip): no cooperative kernel, no graph replay.
// Compiled with -ffp-contract=off.
//
// Neither bidiagonalisation vector is normalised in memory: u^ = beta u and v^ = alpha v are what is stored, and the scale factors
// ride in the scalars (as MINRES's beta / oldb does), which saves two vector passes per step.  The recurrence's scalars (alpha,
// beta, phibar, rhobar, Psi) live in device memory TWICE: the kernels of step k read copy k & 1, and the one thread that commits
// step k (FLsqrWX) writes copy (k + 1) & 1 -- every workgroup of that kernel forms the same new values from the same partial sums
// in its prepare().  A step is two products and three fused passes:
//     y = A v^                                                                 spmv_parts(A)        m rows
//     u^ = (1.0/alpha) y - (alpha/beta) u^ ; partial u^.u^                     FLsqrU               reads 2, writes 1 of length m
//     z = A^T u^                                                               spmv_parts(A->T)     n rows
//     v^ = (1.0/beta') z - (beta'/alpha) v^ ; partial v^.v^                    FLsqrV               reads 2, writes 1 of length n
//     rotation ; x += (phi/rho) w ; w = (1.0/alpha') v^ - (theta/rho) w ; bookkeeping    FLsqrWX    reads 3, writes 2 of length n
// (y and z share one buffer: y has been read by FLsqrU before z is formed.)
#include "sgm_krylov.hpp"

namespace sgm {

enum { L_UU = 0, L_VV = 1 };                                         // partial arrays
enum { LV_U = 0, LV_V = 1, LV_W = 2, LV_T = 3 };                     // work vectors: u^ (m), v^ (n), w (n), y / z (max(m, n))
enum { LS_ALPHA = 0, LS_BETA, LS_PHIBAR, LS_RHOBAR, LS_PSI, LS_COUNT };

__device__ inline double lsqr_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// after u^ = b - A x0 and the partial sums of u^.u^: beta, and the ends that need nothing else
__global__ __launch_bounds__(kBlock) void k_lsqr_start_u(ScalarRef uu, LsqrDev *S, int *flag, double *res_out)
{
    __shared__ double red[kBlock / 64];
    const double d = load_scalar<kBlock>(uu, red);
    if (threadIdx.x != 0) return;
    S->stop = 0;
    if (d < 0.0 || d != d) {
        S->stop = SGM_LSQR_STOP_NAN; S->rnorm = S->arnorm = lsqr_nan();
        *res_out = lsqr_nan();
        *flag = 1;
        return;
    }
    const double beta = sqrt(d);
    S->st[0][LS_BETA] = beta;
    S->rnorm = beta; S->arnorm = 0.0;
    *res_out = beta * beta;
    if (beta == 0.0) { S->stop = SGM_LSQR_STOP_RESIDUAL; *flag = 1; }
}
// after v^ = (1.0/beta) A^T u^ and the partial sums of v^.v^: alpha, the scalars of step 1 and the loop tests before it
__global__ __launch_bounds__(kBlock) void k_lsqr_start_v(ScalarRef vv, LsqrDev *S, double tol, double ntol, int *flag, double *res_out)
{
    __shared__ double red[kBlock / 64];
    if (*flag) return;
    const double d = load_scalar<kBlock>(vv, red);
    if (threadIdx.x != 0) return;
    if (d < 0.0 || d != d) {
        S->stop = SGM_LSQR_STOP_NAN; S->rnorm = S->arnorm = lsqr_nan();
        *res_out = lsqr_nan();
        *flag = 1;
        return;
    }
    double *st = S->st[0];
    const double alpha = sqrt(d), beta = st[LS_BETA];
    st[LS_ALPHA] = alpha; st[LS_PHIBAR] = beta; st[LS_RHOBAR] = alpha; st[LS_PSI] = 0.0;
    const double arnorm = alpha * beta;
    S->arnorm = arnorm;
    int stop = 0;
    if (alpha == 0.0) stop = SGM_LSQR_STOP_NORMAL;
    else if (!(beta > tol)) stop = SGM_LSQR_STOP_RESIDUAL;
    else if (!(arnorm > ntol)) stop = SGM_LSQR_STOP_NORMAL;
    if (stop) { S->stop = stop; *flag = 1; }
}

// w = (1.0/alpha) * v^      (the w of step 1)
struct FLsqrW0 {
    static constexpr bool kDot = false;
    const double *st; const double *v; double *w; double a = 0.0;
    __device__ bool prepare(double *) { a = 1.0 / st[LS_ALPHA]; return true; }
    template <bool NT> __device__ void pair(int64_t i)
    {
        double2 q = ld2<NT>(v, i); q.x = a * q.x; q.y = a * q.y; st2<NT>(w, i, q);
    }
    __device__ void single(int64_t i) { w[i] = a * v[i]; }
    __device__ void finish(double *) {}
};

// a = 1.0/alpha ; t = alpha/beta ; u^ = a*y - t*u^ ; partial u^.u^
struct FLsqrU {
    const double *st; const double *y; double *u; double *part;
    double a = 0.0, t = 0.0, s = 0.0;
    __device__ bool prepare(double *) { a = 1.0 / st[LS_ALPHA]; t = st[LS_ALPHA] / st[LS_BETA]; return true; }
    __device__ double one(double yv, double uv) { const double r = a * yv - t * uv; s += r * r; return r; }
    template <bool NT> __device__ void pair(int64_t i)
    {
        const double2 yy = ld2<NT>(y, i); double2 uu = ld2<NT>(u, i);
        uu.x = one(yy.x, uu.x); uu.y = one(yy.y, uu.y);
        st2<NT>(u, i, uu);
    }
    __device__ void single(int64_t i) { u[i] = one(y[i], u[i]); }
    __device__ void finish(double *red) { put_partial(s, part, red); }
};

// beta' = sqrt(u^.u^) ; a = 1.0/beta' ; t = beta'/alpha ; v^ = a*z - t*v^ ; partial v^.v^
// FIRST (the start): beta' is the stored beta and v^ = a*z.  Nothing is done where beta' is zero, negative or not a number:
// 1.0/beta' is never formed, and FLsqrWX ends the solve.
template <bool FIRST>
struct FLsqrV {
    ScalarRef uu; const double *st; const double *z; double *v; double *part;
    double a = 0.0, t = 0.0, s = 0.0;
    __device__ bool prepare(double *red)
    {
        if (FIRST) { a = 1.0 / st[LS_BETA]; return true; }
        const double d = load_scalar<kBlock>(uu, red);
        if (!(d > 0.0)) return false;
        const double beta = sqrt(d);
        a = 1.0 / beta;
        t = beta / st[LS_ALPHA];
        return true;
    }
    __device__ double one(double zv, double vv)
    {
        const double r = FIRST ? a * zv : a * zv - t * vv;
        s += r * r;
        return r;
    }
    template <bool NT> __device__ void pair(int64_t i)
    {
        const double2 zz = ld2<NT>(z, i);
        double2 q = make_double2(0, 0);
        if (!FIRST) q = ld2<NT>(v, i);
        q.x = one(zz.x, q.x); q.y = one(zz.y, q.y);
        st2<NT>(v, i, q);
    }
    __device__ void single(int64_t i) { v[i] = one(z[i], FIRST ? 0.0 : v[i]); }
    __device__ void finish(double *red) { put_partial(s, part, red); }
};

// The rest of a step.  prepare(): every workgroup forms the step's scalars from u^.u^, v^.v^ and the scalars of the step before;
// commit(): one thread stores them for the next step, counts the step and raises the stop flag; then
//     x = x + (phi/rho)*w ; w = (1.0/alpha')*v^ - (theta/rho)*w      (w is left alone where beta' or alpha' is zero)
// A step that cannot be finished (u^.u^ or v^.v^ negative or not a number; rho or phibar' not a number) stores nothing but the
// stop: x keeps its last value, the step is not counted.
struct FLsqrWX {
    static constexpr bool kDot = false;
    ScalarRef uu, vv; const double *st_in; LsqrDev *S; int nxt;
    const double *v; double *w; double *x;
    double tol, ntol, damp; int *flag; int stop_value; int64_t *iters; double *history; int64_t hist_cap; double *res_out;
    double n_[LS_COUNT] = {0}, t1 = 0.0, t2 = 0.0, a = 0.0, rnorm = 0.0, arnorm = 0.0;
    int stop = 0; bool with_w = false;
    __device__ bool prepare(double *red)
    {
        const ScalarRef rs[2] = {uu, vv};
        double sc[2];
        load_scalars<kBlock, 2>(rs, sc, red);
        const double u2 = sc[0], v2 = sc[1];
        double phibar = st_in[LS_PHIBAR], psi = st_in[LS_PSI];
        const double rhobar = st_in[LS_RHOBAR];
        if (u2 < 0.0 || u2 != u2) { stop = SGM_LSQR_STOP_NAN; return false; }
        const double beta = sqrt(u2);
        double alpha = 0.0;                          // (beta' == 0: v^ was not formed; the rotation ends with s = theta = 0)
        if (beta != 0.0) {
            if (v2 < 0.0 || v2 != v2) { stop = SGM_LSQR_STOP_NAN; return false; }
            alpha = sqrt(v2);
        }
        double rhobar1 = rhobar;
        if (damp != 0.0) {
            rhobar1 = sqrt(rhobar * rhobar + damp * damp);
            const double c1 = rhobar / rhobar1, s1 = damp / rhobar1;
            const double ps = s1 * phibar;
            phibar = c1 * phibar;
            psi = psi + ps * ps;
        }
        const double rho = sqrt(rhobar1 * rhobar1 + beta * beta);
        const double c = rhobar1 / rho, s = beta / rho;
        const double theta = s * alpha;
        const double phi = c * phibar;
        n_[LS_ALPHA] = alpha;
        n_[LS_BETA] = beta;
        n_[LS_RHOBAR] = -(c * alpha);
        n_[LS_PHIBAR] = s * phibar;
        n_[LS_PSI] = psi;
        if (rho != rho || n_[LS_PHIBAR] != n_[LS_PHIBAR]) { stop = SGM_LSQR_STOP_NAN; return false; }
        const double ap = fabs(n_[LS_PHIBAR]);
        rnorm = damp != 0.0 ? sqrt(n_[LS_PHIBAR] * n_[LS_PHIBAR] + psi) : ap;
        arnorm = ap * alpha * fabs(c);
        t1 = phi / rho;
        t2 = theta / rho;
        with_w = beta != 0.0 && alpha != 0.0;
        if (with_w) a = 1.0 / alpha;
        if (beta == 0.0) stop = SGM_LSQR_STOP_RESIDUAL;
        else if (alpha == 0.0) stop = SGM_LSQR_STOP_NORMAL;
        else if (!(rnorm > tol)) stop = SGM_LSQR_STOP_RESIDUAL;
        else if (!(arnorm > ntol)) stop = SGM_LSQR_STOP_NORMAL;
        return true;
    }
    __device__ void commit()
    {
        if (blockIdx.x != 0 || threadIdx.x != 0) return;
        if (stop == SGM_LSQR_STOP_NAN) {
            S->stop = stop;
            *res_out = lsqr_nan();
            *flag = stop_value;
            return;
        }
        double *st = S->st[nxt];
#pragma unroll
        for (int k = 0; k < LS_COUNT; ++k) st[k] = n_[k];
        S->rnorm = rnorm; S->arnorm = arnorm;
        const int64_t it = *iters;
        if (history && it < hist_cap) history[it] = rnorm;
        *iters = it + 1;
        *res_out = rnorm * rnorm;
        if (stop) { S->stop = stop; *flag = stop_value; }
    }
    __device__ void one(double vv_, double &wv, double &xv)
    {
        xv = xv + t1 * wv;
        if (with_w) wv = a * vv_ - t2 * wv;
    }
    template <bool NT> __device__ void pair(int64_t i)
    {
        const double2 q = ld2<NT>(v, i); double2 ww = ld2<NT>(w, i), xx = ld2<NT>(x, i);
        one(q.x, ww.x, xx.x);
        one(q.y, ww.y, xx.y);
        st2<NT>(x, i, xx);
        if (with_w) st2<NT>(w, i, ww);
    }
    __device__ void single(int64_t i)
    {
        double ww = w[i], xx = x[i];
        one(v[i], ww, xx);
        x[i] = xx;
        if (with_w) w[i] = ww;
    }
    __device__ void finish(double *) {}
};

int run_lsqr(sgm_solver s, sgm_mat A, double *const *x, const double *const *b)
{
    PartWork &w = s->work[0];                       // (sgm_solver_setup refuses composite, partitioned and distributed matrices)
    const int64_t m = A->nrow, n = A->ncol;
    SGM_TRY(ensure_transpose(A));                   // (A's values may have changed since setup: the cached A^T takes them again)
    auto W = [&](int k) { return w.vec[k]; };
    int grid = 0;
    const double *cx[1]; double *yy[1];
    auto product = [&](sgm_mat M, const double *src, double *dst, const int *flag, int gen) -> int {
        cx[0] = src; yy[0] = dst;
        return spmv_parts(M, cx, yy, false, nullptr, flag, &grid, gen);
    };
    auto dot = [&](int k, int vec, int64_t len, bool use_flag, int gen) -> int {
        const int ks[1] = {k}; const int vecs[1][2] = {{vec, vec}};
        return finish_dots(s, A, ks, 1, vecs, use_flag, gen, nullptr, len);
    };
    LsqrDev *S = w.lsqr;
    const double tol = s->tolerance, ntol = s->normal_tolerance, damp = s->damp;
    s->breakdown = 0;
    w.count[L_UU] = dot_grid(m);
    w.count[L_VV] = dot_grid(n);

    // u^ = b - A x0 ; beta = sqrt(u^.u^) ; v^ = (1.0/beta) A^T u^ ; alpha = sqrt(v^.v^) ; w = (1.0/alpha) v^
    launch_elem(n, FCopy{W(LV_W), x[0]}, nullptr);                     // (x staged in w's buffer, which the start fills last)
    SGM_TRY(product(A, W(LV_W), W(LV_T), nullptr, INT32_MAX));
    launch_elem(m, FCgInit{b[0], W(LV_T), W(LV_U), nullptr, nullptr, false}, nullptr);
    launch_elem(m, FDot2{W(LV_U), W(LV_U), nullptr, nullptr, part(s, 0, L_UU), nullptr}, nullptr);
    SGM_TRY(dot(L_UU, LV_U, m, false, INT32_MAX));
    hipLaunchKernelGGL(k_lsqr_start_u, dim3(1), dim3(kBlock), 0, g_rt.stream, ref(s, 0, L_UU), S, w.flag, w.res);
    SGM_TRY(product(A->T, W(LV_U), W(LV_T), w.flag, INT32_MAX));
    launch_elem(n, FLsqrV<true>{ref(s, 0, L_UU), S->st[0], W(LV_T), W(LV_V), part(s, 0, L_VV)}, w.flag);
    SGM_TRY(dot(L_VV, LV_V, n, true, INT32_MAX));
    hipLaunchKernelGGL(k_lsqr_start_v, dim3(1), dim3(kBlock), 0, g_rt.stream, ref(s, 0, L_VV), S, tol, ntol, w.flag, w.res);
    launch_elem(n, FLsqrW0{S->st[0], W(LV_V), W(LV_W)}, w.flag);

    int64_t k = 0;
    int flag = 0; int64_t iters = 0; double res = 0.0;
    // step k + 1 of the solve with generation `gen`, relative to its batch
    auto enqueue_iter = [&](int64_t k, int gen) -> int {
        const int cur = (int)(k & 1), nxt = cur ^ 1;
        const double *st = S->st[cur];
        SGM_TRY(product(A, W(LV_V), W(LV_T), w.flag, gen));
        launch_elem(m, FLsqrU{st, W(LV_T), W(LV_U), part(s, 0, L_UU)}, w.flag, gen);
        SGM_TRY(dot(L_UU, LV_U, m, true, gen));
        SGM_TRY(product(A->T, W(LV_U), W(LV_T), w.flag, gen));
        launch_elem(n, FLsqrV<false>{ref(s, 0, L_UU), st, W(LV_T), W(LV_V), part(s, 0, L_VV)}, w.flag, gen);
        SGM_TRY(dot(L_VV, LV_V, n, true, gen));
        launch_elem(n, FLsqrWX{ref(s, 0, L_UU), ref(s, 0, L_VV), st, S, nxt, W(LV_V), W(LV_W), x[0], tol, ntol, damp,
                               w.flag, gen + 1, w.iters, w.history, s->hist_cap, w.res}, w.flag, gen);
        return SGM_OK;
    };
    for (;;) {
        // the host looks at the stop flag once per batch; batches grow with the steps already done (run_cg)
        const int64_t batch = next_batch(s, k, 16, false);
        if (batch > 0) hipLaunchKernelGGL(k_flag_norm, dim3(1), dim3(64), 0, g_rt.stream, w.flag);
        for (int64_t j = 0; j < batch; ++j) SGM_TRY(enqueue_iter(k + j, (int)j + 1));
        k += batch;
        SGM_HIP(hipGetLastError());
        SGM_TRY(read_state(s, &flag, &iters, &res));
        if (flag || (s->max_iter > 0 && k >= s->max_iter)) break;
    }
    LsqrDev end;
    SGM_HIP(hipMemcpy(&end, S, sizeof(LsqrDev), hipMemcpyDeviceToHost));
    s->lsqr_stop = flag ? end.stop : 0;
    s->lsqr_rnorm = end.rnorm;
    s->lsqr_arnorm = end.arnorm;
    s->breakdown = s->lsqr_stop == SGM_LSQR_STOP_NAN;
    store_result(s, s->lsqr_stop == SGM_LSQR_STOP_RESIDUAL || s->lsqr_stop == SGM_LSQR_STOP_NORMAL, iters, res);
    return SGM_OK;
}

}  // namespace sgm
