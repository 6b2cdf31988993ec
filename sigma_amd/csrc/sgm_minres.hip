// Preconditioned MINRES (Paige-Saunders) on the device, for symmetric A and a symmetric positive definite M: no reference
// counterpart; the contract is the loop in include/sigma_hip.h (sgm_minres_create) and DESIGN.md section 9f, restated by
// tests/minres_restated.py.  A launch loop in the style of run_cg (sgm_cg.hip): no one-workgroup or cooperative kernel, no
// graph replay.  Compiled with -ffp-contract=off.
//
// The recurrence's scalars (oldb, beta, dbar, epsln, phibar, cs, sn) live in device memory, TWICE: the kernels of step k read
// copy k & 1, and the one thread that commits step k (FMinresWX) writes copy (k + 1) & 1 -- every workgroup of that kernel
// forms the same new values from the same partial sums in its prepare(), so none of them waits for the thread that stores them.
// A step is the product and three fused passes:
//     y = A v                                                                  spmv_parts
//     y -= (beta / oldb) r1 (from step 2 on) ; partial v.y                     FMinresY1
//     y -= (alfa / beta) r2 ; [z = idiag * y] ; partial y.y [y.z]              FMinresY2    (r1 <- r2 <- y: the buffers rotate)
//     [z = M^-1 y ; partial y.z]                                               any other preconditioner
//     rotation ; w = ((v - oldeps w1) - delta w2) gi ; x += phi w ; v = y / beta (the NEXT step's v) ; bookkeeping    FMinresWX
#include "sgm_krylov.hpp"

namespace sgm {

enum { M_ALFA = 0, M_BB = 1 };                                       // partial arrays
enum { MV_V = 0, MV_W0 = 1, MV_W1 = 2, MV_X = 3, MV_R0 = 4 };        // work vectors: v, w / w2 (alternating), x staging, r1 / r2 / y (rotating)
enum { MS_OLDB = 0, MS_BETA, MS_DBAR, MS_EPSLN, MS_PHIBAR, MS_CS, MS_SN, MS_COUNT };
enum { MINRES_FAIL_NAN = 1, MINRES_FAIL_GAMMA = 2 };

// after r1 = b - A x, y = M^-1 r1 and the partial sums of r1.y: the scalars of step 1 and the loop test before it
__global__ __launch_bounds__(kBlock) void k_minres_start(ScalarRef bb, MinresDev *S, double tol, int *flag, double *res_out)
{
    __shared__ double red[kBlock / 64];
    const double d = load_scalar<kBlock>(bb, red);
    if (threadIdx.x != 0) return;
    S->fail = 0;
    if (d < 0.0 || d != d) {                 // M is not positive definite, or a NaN came in
        S->fail = MINRES_FAIL_NAN;
        *res_out = __longlong_as_double(0x7ff8000000000000ll);
        *flag = 1;
        return;
    }
    const double beta1 = sqrt(d);
    double *st = S->st[0];
    st[MS_OLDB] = 0.0; st[MS_BETA] = beta1; st[MS_DBAR] = 0.0; st[MS_EPSLN] = 0.0; st[MS_PHIBAR] = beta1;
    st[MS_CS] = -1.0; st[MS_SN] = 0.0;
    *res_out = beta1 * beta1;
    if (!(fabs(beta1) > tol)) *flag = 1;
}

// v = (1.0 / beta) * y      (the v of step 1)
struct FMinresV {
    static constexpr bool kDot = false;
    const double *st; const double *y; double *v; double s = 0.0;
    __device__ bool prepare(double *) { s = 1.0 / st[MS_BETA]; return true; }
    template <bool NT> __device__ void pair(int64_t i)
    {
        double2 a = ld2<NT>(y, i); a.x = s * a.x; a.y = s * a.y; st2<NT>(v, i, a);
    }
    __device__ void single(int64_t i) { v[i] = s * y[i]; }
    __device__ void finish(double *) {}
};

// t = beta / oldb ; y = y - t * r1 (not in step 1) ; partial v.y
struct FMinresY1 {
    const double *st; double *y; const double *r1, *v; double *part; bool first;
    double t = 0.0, s = 0.0;
    __device__ bool prepare(double *) { if (!first) t = st[MS_BETA] / st[MS_OLDB]; return true; }
    template <bool NT> __device__ void pair(int64_t i)
    {
        double2 yy = ld2<NT>(y, i); const double2 vv = ld2<NT>(v, i);
        if (!first) {
            const double2 rr = ld2<NT>(r1, i);
            yy.x = yy.x - t * rr.x; yy.y = yy.y - t * rr.y;
            st2<NT>(y, i, yy);
        }
        s += vv.x * yy.x; s += vv.y * yy.y;
    }
    __device__ void single(int64_t i)
    {
        double yv = y[i];
        if (!first) { yv = yv - t * r1[i]; y[i] = yv; }
        s += v[i] * yv;
    }
    __device__ void finish(double *red) { put_partial(s, part, red); }
};

// t = alfa / beta ; y = y - t * r2 ; then
//   MODE 0: partial y.y   MODE 1: z = idiag * y, partial y.z   MODE 2: nothing (another preconditioner follows)
template <int MODE>
struct FMinresY2 {
    static constexpr bool kDot = MODE != 2;
    ScalarRef alfa; const double *st; double *y; const double *r2, *idiag; double *z; double *part;
    double t = 0.0, s = 0.0;
    __device__ bool prepare(double *red) { t = load_scalar<kBlock>(alfa, red) / st[MS_BETA]; return true; }
    __device__ void one(double rv, double &yv, double idv, double &zv)
    {
        yv = yv - t * rv;
        if (MODE == 0) s += yv * yv;
        if (MODE == 1) { zv = idv * yv; s += yv * zv; }
    }
    template <bool NT> __device__ void pair(int64_t i)
    {
        const double2 rr = ld2<NT>(r2, i);
        double2 yy = ld2<NT>(y, i), zz = make_double2(0, 0), dd = make_double2(0, 0);
        if (MODE == 1) dd = ld2<NT>(idiag, i);
        one(rr.x, yy.x, dd.x, zz.x);
        one(rr.y, yy.y, dd.y, zz.y);
        st2<NT>(y, i, yy);
        if (MODE == 1) st2<NT>(z, i, zz);
    }
    __device__ void single(int64_t i)
    {
        double yv = y[i], zv = 0.0;
        one(r2[i], yv, MODE == 1 ? idiag[i] : 0.0, zv);
        y[i] = yv;
        if (MODE == 1) z[i] = zv;
    }
    __device__ void finish(double *red) { if (MODE != 2) put_partial(s, part, red); }
};

// The rest of a step.  prepare(): every workgroup forms the step's scalars from alfa, bb and the scalars of the step before;
// commit(): one thread stores them for the next step, counts the step and raises the stop flag; then
//     w1 = w2 ; w2 = w ; w = ((v - oldeps*w1) - delta*w2) * gi ; x = x + phi*w      (the new w takes w1's place)
//     v = (1.0 / beta) * z                                                           (z = M^-1 r2: the next step's v)
// A step that cannot be finished (bb < 0 or not a number; gamma == 0; gamma or phibar not a number) stores nothing but the
// stop: x keeps its last value, the step is not counted.
struct FMinresWX {
    static constexpr bool kDot = false;
    ScalarRef alfa, bb; const double *st_in; MinresDev *S; int nxt;
    double *v; const double *z; double *w1; const double *w2; double *x;
    double tol; int *flag; int stop_value; int64_t *iters; double *history; int64_t hist_cap; double *res_out;
    double n_[MS_COUNT] = {0}, oldeps = 0.0, delta = 0.0, gi = 0.0, phi = 0.0, s = 0.0, fail_res = 0.0;
    int fail = 0;
    __device__ bool prepare(double *red)
    {
        const ScalarRef rs[2] = {alfa, bb};
        double sc[2];
        load_scalars<kBlock, 2>(rs, sc, red);
        const double al = sc[0], b2 = sc[1];
        const double beta0 = st_in[MS_BETA], dbar = st_in[MS_DBAR], epsln = st_in[MS_EPSLN], phibar = st_in[MS_PHIBAR],
                     cs = st_in[MS_CS], sn = st_in[MS_SN];
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        if (b2 < 0.0 || b2 != b2) { fail = MINRES_FAIL_NAN; fail_res = nan; return false; }
        const double beta = sqrt(b2);
        oldeps = epsln;
        delta = cs * dbar + sn * al;
        const double gbar = sn * dbar - cs * al;
        const double gamma = sqrt(gbar * gbar + beta * beta);
        if (gamma == 0.0) { fail = MINRES_FAIL_GAMMA; fail_res = phibar * phibar; return false; }
        gi = 1.0 / gamma;
        n_[MS_OLDB] = beta0;
        n_[MS_BETA] = beta;
        n_[MS_EPSLN] = sn * beta;
        n_[MS_DBAR] = -(cs * beta);
        n_[MS_CS] = gbar * gi;
        n_[MS_SN] = beta * gi;
        phi = n_[MS_CS] * phibar;
        n_[MS_PHIBAR] = n_[MS_SN] * phibar;
        if (gamma != gamma || n_[MS_PHIBAR] != n_[MS_PHIBAR]) { fail = MINRES_FAIL_NAN; fail_res = nan; return false; }
        s = 1.0 / beta;
        return true;
    }
    __device__ void commit()
    {
        if (blockIdx.x != 0 || threadIdx.x != 0) return;
        if (fail) {
            S->fail = fail;
            *res_out = fail_res;
            *flag = stop_value;
            return;
        }
        double *st = S->st[nxt];
#pragma unroll
        for (int k = 0; k < MS_COUNT; ++k) st[k] = n_[k];
        const double a = fabs(n_[MS_PHIBAR]);
        const int64_t it = *iters;
        if (history && it < hist_cap) history[it] = a;
        *iters = it + 1;
        *res_out = n_[MS_PHIBAR] * n_[MS_PHIBAR];
        if (!(a > tol)) *flag = stop_value;
    }
    __device__ void one(double &vv, double zv, double &w1v, double w2v, double &xv)
    {
        const double wn = ((vv - oldeps * w1v) - delta * w2v) * gi;
        xv = xv + phi * wn;
        w1v = wn;
        vv = s * zv;
    }
    template <bool NT> __device__ void pair(int64_t i)
    {
        double2 vv = ld2<NT>(v, i), ww = ld2<NT>(w1, i), xx = ld2<NT>(x, i);
        const double2 zz = ld2<NT>(z, i), w2v = ld2<NT>(w2, i);
        one(vv.x, zz.x, ww.x, w2v.x, xx.x);
        one(vv.y, zz.y, ww.y, w2v.y, xx.y);
        st2<NT>(w1, i, ww); st2<NT>(x, i, xx); st2<NT>(v, i, vv);
    }
    __device__ void single(int64_t i)
    {
        double vv = v[i], ww = w1[i], xx = x[i];
        one(vv, z[i], ww, w2[i], xx);
        w1[i] = ww; x[i] = xx; v[i] = vv;
    }
    __device__ void finish(double *) {}
};

int run_minres(sgm_solver s, sgm_mat A, double *const *x, const double *const *b, sgm_pc pc)
{
    PartWork &w = s->work[0];                       // (sgm_solver_setup refuses partitioned and distributed matrices)
    const int64_t n = w.n;
    const int pk = pc ? pc_kind(pc) : 0;
    auto W = [&](int k) { return w.vec[k]; };
    int grid = 0;
    const int *flags[1] = {w.flag};
    const double *cx[1]; double *yy[1];
    auto product = [&](const double *src, double *dst, const int *flag, int gen) -> int {
        cx[0] = src; yy[0] = dst;
        return spmv_parts(A, cx, yy, false, nullptr, flag, &grid, gen);
    };
    auto apply_pc = [&](const double *r, double *z, bool use_flag) -> int {
        const double *rr[1] = {r}; double *zz[1] = {z};
        return pc_apply_parts(pc, A, rr, zz, use_flag ? flags : nullptr);
    };
    s->breakdown = 0;
    w.count[M_ALFA] = w.count[M_BB] = dot_grid(n);
    SGM_HIP(hipMemsetAsync(W(MV_W0), 0, ((size_t)w.next + 2) * 8, g_rt.stream));
    SGM_HIP(hipMemsetAsync(W(MV_W1), 0, ((size_t)w.next + 2) * 8, g_rt.stream));

    // r1 = b - A x ; y = M^-1 r1 ; beta1 = sqrt(r1.y) ; v = y / beta1.   r[c2] holds r2 (= r1 at the start), r[c1] r1, r[c0] is free
    int c0 = 0, c1 = 1, c2 = 2;
    auto R = [&](int c) { return W(MV_R0 + c); };
    launch_elem(n, FCopy{W(MV_X), x[0]}, nullptr);
    SGM_TRY(product(W(MV_X), R(c1), nullptr, INT32_MAX));
    launch_elem(n, FCgInit{b[0], R(c1), R(c2), nullptr, nullptr, false}, nullptr);
    if (pk != 0) SGM_TRY(apply_pc(R(c2), R(c0), false));
    int zc = pk != 0 ? c0 : c2;                      // where z = M^-1 r2 stands (without a preconditioner: r2 itself)
    launch_elem(n, FDot2{R(c2), R(zc), nullptr, nullptr, part(s, 0, M_BB), nullptr}, nullptr);
    { const int ks[1] = {M_BB}; const int vecs[1][2] = {{MV_R0 + c2, MV_R0 + zc}}; SGM_TRY(finish_dots(s, A, ks, 1, vecs)); }
    hipLaunchKernelGGL(k_minres_start, dim3(1), dim3(kBlock), 0, g_rt.stream, ref(s, 0, M_BB), w.minres, s->tolerance, w.flag, w.res);
    launch_elem(n, FMinresV{w.minres->st[0], R(zc), W(MV_V)}, w.flag);

    int64_t k = 0;
    int flag = 0; int64_t iters = 0; double res = 0.0;
    const int64_t batch_max = pc_apply_is_short(pc) ? 16 : 1;
    // step k + 1 of the solve with generation `gen`, relative to its batch
    auto enqueue_iter = [&](int64_t k, int gen) -> int {
        const int cur = (int)(k & 1), nxt = cur ^ 1;
        const double *st = w.minres->st[cur];
        double *y = R(c0);
        SGM_TRY(product(W(MV_V), y, w.flag, gen));
        launch_elem(n, FMinresY1{st, y, R(c1), W(MV_V), part(s, 0, M_ALFA), k == 0}, w.flag, gen);
        { const int ks[1] = {M_ALFA}; const int vecs[1][2] = {{MV_V, MV_R0 + c0}}; SGM_TRY(finish_dots(s, A, ks, 1, vecs, true, gen)); }
        double *z = pk != 0 ? R(c1) : y;             // (r1's buffer is free once FMinresY1 has read it)
        if (pk == 0)
            launch_elem(n, FMinresY2<0>{ref(s, 0, M_ALFA), st, y, R(c2), nullptr, nullptr, part(s, 0, M_BB)}, w.flag, gen);
        else if (pk == SGM_PC_JACOBI)
            launch_elem(n, FMinresY2<1>{ref(s, 0, M_ALFA), st, y, R(c2), pc_idiag(pc, 0), z, part(s, 0, M_BB)}, w.flag, gen);
        else {
            launch_elem(n, FMinresY2<2>{ref(s, 0, M_ALFA), st, y, R(c2), nullptr, nullptr, nullptr}, w.flag, gen);
            SGM_TRY(apply_pc(y, z, true));
            launch_elem(n, FDot2{y, z, nullptr, nullptr, part(s, 0, M_BB), nullptr}, w.flag, gen);
        }
        // r1 = r2 ; r2 = y: the buffers change roles
        { const int t = c1; c1 = c2; c2 = c0; c0 = t; }
        { const int ks[1] = {M_BB}; const int vecs[1][2] = {{MV_R0 + c2, MV_R0 + (pk != 0 ? c0 : c2)}}; SGM_TRY(finish_dots(s, A, ks, 1, vecs, true, gen)); }
        // w stands in W0 after an even number of steps, in W1 after an odd one; the new w takes the place of w1
        double *wcur = W(cur ? MV_W1 : MV_W0), *wold = W(cur ? MV_W0 : MV_W1);
        launch_elem(n, FMinresWX{ref(s, 0, M_ALFA), ref(s, 0, M_BB), st, w.minres, nxt, W(MV_V), z, wold, wcur, x[0], s->tolerance,
                                 w.flag, gen + 1, w.iters, w.history, s->hist_cap, w.res}, w.flag, gen);
        return SGM_OK;
    };
    for (;;) {
        // the host looks at the stop flag once per batch; batches grow with the steps already done (run_cg)
        const int64_t batch = next_batch(s, k, batch_max, false);
        if (batch > 0) hipLaunchKernelGGL(k_flag_norm, dim3(1), dim3(64), 0, g_rt.stream, w.flag);
        for (int64_t j = 0; j < batch; ++j) SGM_TRY(enqueue_iter(k + j, (int)j + 1));
        k += batch;
        SGM_HIP(hipGetLastError());
        SGM_TRY(read_state(s, &flag, &iters, &res));
        if (flag || s->aborted || (s->max_iter > 0 && k >= s->max_iter)) break;
    }
    int32_t failed = 0;
    SGM_HIP(hipMemcpy(&failed, &w.minres->fail, sizeof(int32_t), hipMemcpyDeviceToHost));
    s->breakdown = failed;
    store_result(s, flag && !failed, iters, res);
    return SGM_OK;
}

}  // namespace sgm
