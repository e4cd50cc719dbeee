// solver_multi.hip — spmv_cg_multi: k independent conjugate-gradient solves A x_c = b_c in one loop, on CDNA4 (gfx950).
//
// B, X and every work vector are ROW-MAJOR (n x k), entry (i, c) at i*k + c, as in spmv_apply_multi (kernels_spmm.hip), and the
// product W = A U of every iteration IS that entry point with overwrite: the matrix is read once per iteration for all k systems,
// and column c of W has the SCALAR kernel's order of additions, bit for bit.  Nothing couples the columns (this is not block CG):
// each has its own alpha, beta, gamma, delta and follows the Chronopoulos-Gear recurrence of cg_fused_kernel (solver.hip).
//
// Three launches per iteration:
//   1  spmm_apply           W = A U (U = D^-1 R with Jacobi, else U is R itself)
//   2  cgm_dots_kernel      delta_c = u_c . w_c
//   3  cgm_fused_kernel     beta = gamma / gamma_old;  alpha = gamma / (delta - beta gamma / alpha_old);
//                           p = u + beta p;  s = w + beta s;  x += alpha p;  r -= alpha s;  u = D^-1 r;  r.r and r.u
//
// Shape of the vector kernels: a group of KP lanes owns a row, lane t of it the column t (narrow path: 8-byte accesses; KP = the
// next power of two >= k) or the columns 2t and 2t + 1 (wide path: 16-byte accesses; k even and B, X 16-byte aligned; KP = the next
// power of two >= k / 2).  The kBlock / KP rows of a workgroup are consecutive, so a wavefront reads one contiguous stretch, and
// the rows are dealt over the workgroups in a grid-stride loop.  alpha_c and beta_c are formed once per workgroup and sit in the
// lane's registers for all of its rows.
//
// The dot products are DETERMINISTIC: no atomic adds in arrival order.  A workgroup reduces its lanes' sums per column in a fixed
// order (an xor butterfly over the row groups of a wavefront, then the four wavefronts in order) and stores the result in a
// [workgroups][k] buffer; the workgroup that takes the last ticket of the launch (took_last_ticket, solver_common.hpp: the pattern
// spmv_cgls runs too, with the one fencing thread per workgroup it needs) adds the buffer up per column - again in an order fixed
// by (n, k) alone - and writes the column's scalars, which the next launch reads.  Which workgroup comes last changes nothing: the
// order of the additions belongs to the buffer, not to the adder.  So two calls give the same bits, and column c depends on column
// c of B and X alone at a given (n, k, c).  The buffer's layout, part[workgroup][column], and with it the order of the additions
// are this file's own (column_sum, store_partials, column_total): grid_totals' part[quantity][workgroup] adds in another order.
//
// Per-column state on the device (CgmScalars): `frozen` is written by the host when a column has converged (or b_c = 0) - the
// kernels then neither read nor write that column of X, R, U, P, S; a column whose r.r is at or below 1e-28 b.b passes quietly as
// in cg_fused_kernel; a column without a descent direction raises ITS status word.  A frozen or quiet column's scalars are never
// looked at, so its 0/0 stays where it is.  Frozen columns still ride through the product (their column of W is rewritten with
// the same bits): compacting them is not done.
#include <cmath>
#include <vector>

#include "common.hpp"
#include "solver_common.hpp"
#include "solver_host.hpp"
#include "wave.hpp"

namespace spmv
{
namespace
{
constexpr int kCgmMaxK    = 64;    // columns per call (spmv_apply_multi's limit)
constexpr int kCgmMaxGrid = 1024;  // workgroups per launch (4 per CU): what the last workgroup adds up per column

struct CgmScalars
{
    double   gamma[kCgmMaxK];      // r_j . u_j (without a preconditioner: r_j . r_j)
    double   gamma_old[kCgmMaxK];  // gamma of the iteration before (0 before the first: beta_0 = 0)
    double   alpha_old[kCgmMaxK];  // alpha of the iteration before
    double   delta[kCgmMaxK];      // u_j . A u_j
    double   rr[kCgmMaxK];         // r_j . r_j: what the host looks at
    double   bb[kCgmMaxK];         // b . b
    double   floor_rr[kCgmMaxK];   // 1e-28 b.b: at or below it r.r is rounding noise and the column passes quietly
    int32_t  frozen[kCgmMaxK];     // written by the host: the column has converged (or b_c = 0) and is left alone
    int32_t  status[kCgmMaxK];     // 1: no descent direction (p.Ap <= 0 or r.M^-1 r <= 0), 2: r.r is NaN
    uint32_t ticket;               // workgroups of the current launch that have stored their partial sums
    uint32_t pad;
};

template <int V>
__device__ __forceinline__ void load_cols(const double* p, double (&v)[V])
{
    if constexpr (V == 2)
    {
        const f64x2 t = *(const f64x2*)p;
        v[0]            = t[0];
        v[1]            = t[1];
    }
    else
        v[0] = *p;
}
template <int V>
__device__ __forceinline__ void store_cols(double* p, const double (&v)[V])
{
    if constexpr (V == 2)
        *(f64x2*)p = f64x2{v[0], v[1]};
    else
        *p = v[0];
}

// Sum of v over the lanes of the workgroup whose lane index agrees in its low bits (lane & (KP - 1): the lanes of one column), in a
// fixed order: xor butterfly over the row groups of a wavefront, then the four wavefronts in order.  Valid in threads 0 .. KP-1.
__device__ __forceinline__ double column_sum(double v, int KP, double (*s_part)[kWave])
{
    const int lane = lane_id();
    for (int off = KP; off < kWave; off <<= 1) v += bpermute(v, lane ^ off);
    __syncthreads();  // the previous call's readers are done with s_part
    if (lane < KP) s_part[threadIdx.x >> 6][lane] = v;
    __syncthreads();
    double t = 0.0;
    if ((int)threadIdx.x < KP)
        for (int w = 0; w < kBlock / kWave; ++w) t += s_part[w][threadIdx.x];
    return t;
}

// the workgroup's sums of `val` per column into part[blockIdx.x][0..k)
template <int V>
__device__ __forceinline__ void store_partials(const double (&val)[V], int KP, int k, double* __restrict__ part, double (*s_part)[kWave])
{
#pragma unroll
    for (int e = 0; e < V; ++e)
    {
        const double t = column_sum(val[e], KP, s_part);
        const int    c = (int)threadIdx.x * V + e;
        if ((int)threadIdx.x < KP && c < k) part[(int64_t)blockIdx.x * k + c] = t;
    }
}

// column (threadIdx.x)'s total of part[0 .. gridDim.x)[c], for threads < KC (KC: the next power of two >= k): the 256 / KC
// slices of workgroups g = slice, slice + slices, ... are added up by one lane each, then column_sum over the slices
__device__ __forceinline__ double column_total(const double* part, int k, int kc_log2, double (*s_part)[kWave])
{
    const int KC = 1 << kc_log2, c = threadIdx.x & (KC - 1), slice = threadIdx.x >> kc_log2, slices = kBlock >> kc_log2;
    double    acc = 0.0;
    if (c < k)
        for (int g = slice; g < (int)gridDim.x; g += slices) acc += partial_sum_load(part + (int64_t)g * k + c);
    return column_sum(acc, KC, s_part);
}

// R = B - Q (Q = A X0), U = D^-1 R (PRE), P = S = 0; the last workgroup writes every scalar of every column
template <bool PRE, int V>
__global__ __launch_bounds__(kBlock) void cgm_init_kernel(int64_t n, int k, int kp_log2, int kc_log2, const double* __restrict__ B,
                                                          const double* __restrict__ Q, double* __restrict__ R, double* __restrict__ U,
                                                          double* __restrict__ P, double* __restrict__ S, const double* __restrict__ dinv,
                                                          double* __restrict__ part, CgmScalars* __restrict__ s)
{
    __shared__ double s_part[kBlock / kWave][kWave];
    const int  KP = 1 << kp_log2, t = threadIdx.x & (KP - 1), grp = threadIdx.x >> kp_log2, rpb = kBlock >> kp_log2;
    const int  c  = t * V;
    double     rr[V] = {}, bb[V] = {}, ru[V] = {};
    const double zero[V] = {};
    if (c < k)
        for (int64_t row = (int64_t)blockIdx.x * rpb + grp; row < n; row += (int64_t)gridDim.x * rpb)
        {
            const int64_t at = row * k + c;
            const double  d  = PRE ? dinv[row] : 1.0;
            double        bv[V], qv[V], rv[V], uv[V];
            load_cols<V>(B + at, bv);
            load_cols<V>(Q + at, qv);
#pragma unroll
            for (int e = 0; e < V; ++e)
            {
                rv[e] = bv[e] - qv[e];
                uv[e] = PRE ? rv[e] * d : rv[e];
                rr[e] = fma(rv[e], rv[e], rr[e]);
                bb[e] = fma(bv[e], bv[e], bb[e]);
                if (PRE) ru[e] = fma(rv[e], uv[e], ru[e]);
            }
            store_cols<V>(R + at, rv);
            if (PRE) store_cols<V>(U + at, uv);
            store_cols<V>(P + at, zero);
            store_cols<V>(S + at, zero);
        }
    const int64_t plane = (int64_t)gridDim.x * k;  // one [workgroups][k] buffer per quantity
    store_partials<V>(rr, KP, k, part, s_part);
    store_partials<V>(bb, KP, k, part + plane, s_part);
    if (PRE) store_partials<V>(ru, KP, k, part + 2 * plane, s_part);
    if (!took_last_ticket(&s->ticket)) return;
    const double t_rr = column_total(part, k, kc_log2, s_part);
    const double t_bb = column_total(part + plane, k, kc_log2, s_part);
    const double t_ru = PRE ? column_total(part + 2 * plane, k, kc_log2, s_part) : t_rr;
    if ((int)threadIdx.x < k)
    {
        const int cc      = threadIdx.x;
        s->gamma[cc]      = t_ru;
        s->gamma_old[cc]  = 0.0;
        s->alpha_old[cc]  = 0.0;
        s->delta[cc]      = 0.0;
        s->rr[cc]         = t_rr;
        s->bb[cc]         = t_bb;
        s->floor_rr[cc]   = 1e-28 * t_bb;
        s->frozen[cc]     = 0;
        s->status[cc]     = 0;
    }
    if (threadIdx.x == 0) s->ticket = 0;
}

// delta_c = u_c . w_c for the columns that are not frozen
template <int V>
__global__ __launch_bounds__(kBlock) void cgm_dots_kernel(int64_t n, int k, int kp_log2, int kc_log2, const double* __restrict__ U,
                                                          const double* __restrict__ W, double* __restrict__ part,
                                                          CgmScalars* __restrict__ s)
{
    __shared__ double s_part[kBlock / kWave][kWave];
    const int KP = 1 << kp_log2, t = threadIdx.x & (KP - 1), grp = threadIdx.x >> kp_log2, rpb = kBlock >> kp_log2;
    const int c  = t * V;
    bool      on[V];
#pragma unroll
    for (int e = 0; e < V; ++e) on[e] = c + e < k && s->frozen[c + e] == 0;
    bool any = false, all = true;
#pragma unroll
    for (int e = 0; e < V; ++e)
    {
        any = any || on[e];
        all = all && on[e];
    }
    double acc[V] = {};
    if (any)
        for (int64_t row = (int64_t)blockIdx.x * rpb + grp; row < n; row += (int64_t)gridDim.x * rpb)
        {
            const int64_t at = row * k + c;
            if (V == 2 && all)
            {
                double uv[V], wv[V];
                load_cols<V>(U + at, uv);
                load_cols<V>(W + at, wv);
#pragma unroll
                for (int e = 0; e < V; ++e) acc[e] = fma(uv[e], wv[e], acc[e]);
            }
            else
            {
#pragma unroll
                for (int e = 0; e < V; ++e)
                    if (on[e]) acc[e] = fma(U[at + e], W[at + e], acc[e]);
            }
        }
    store_partials<V>(acc, KP, k, part, s_part);
    if (!took_last_ticket(&s->ticket)) return;
    const double total = column_total(part, k, kc_log2, s_part);
    if ((int)threadIdx.x < k && s->frozen[threadIdx.x] == 0) s->delta[threadIdx.x] = total;
    if (threadIdx.x == 0) s->ticket = 0;
}

// The fused update of one iteration, the counterpart of cg_fused_kernel for k columns in one pass.  Without a preconditioner
// (PRE false) u IS r: U is not touched and W = A R.
template <bool PRE, int V>
__global__ __launch_bounds__(kBlock) void cgm_fused_kernel(int64_t n, int k, int kp_log2, int kc_log2, const double* __restrict__ W,
                                                           double* __restrict__ U, double* __restrict__ P, double* __restrict__ S,
                                                           double* __restrict__ X, double* __restrict__ R, const double* __restrict__ dinv,
                                                           double* __restrict__ part, CgmScalars* __restrict__ s)
{
    __shared__ double s_part[kBlock / kWave][kWave];
    __shared__ double s_alpha[kCgmMaxK], s_beta[kCgmMaxK], s_gamma[kCgmMaxK];
    __shared__ int    s_live[kCgmMaxK];
    if (threadIdx.x < kCgmMaxK)
    {
        const int cc = threadIdx.x;
        double    alpha = 0.0, beta = 0.0, gamma = 0.0;
        int       live = 0;
        if (cc < k && s->frozen[cc] == 0)
        {
            const double rr_c = s->rr[cc];
            gamma             = s->gamma[cc];
            if (rr_c != rr_c)
            {
                if (blockIdx.x == 0) s->status[cc] = 2;  // r.r is NaN: b, x0 or the matrix hold non-finite numbers
            }
            else if (rr_c > s->floor_rr[cc])  // at or below the floor: rounding noise, the column passes quietly
            {
                const double gamma_old = s->gamma_old[cc], delta = s->delta[cc];
                beta               = gamma_old > 0.0 ? gamma / gamma_old : 0.0;
                const double denom = beta != 0.0 ? delta - beta * gamma / s->alpha_old[cc] : delta;
                if (!(denom > 0.0) || !(gamma > 0.0))
                {
                    // a residual to speak of and no descent direction: p.Ap <= 0 or r.M^-1 r <= 0 (or one of them NaN)
                    if (blockIdx.x == 0) s->status[cc] = 1;
                }
                else
                {
                    alpha = gamma / denom;
                    live  = 1;
                }
            }
        }
        s_alpha[cc] = alpha;
        s_beta[cc]  = beta;
        s_gamma[cc] = gamma;
        s_live[cc]  = live;
    }
    __syncthreads();
    const int KP = 1 << kp_log2, t = threadIdx.x & (KP - 1), grp = threadIdx.x >> kp_log2, rpb = kBlock >> kp_log2;
    const int c  = t * V;
    double    alpha[V], beta[V];
    bool      on[V];
    bool      any = false, all = true;
#pragma unroll
    for (int e = 0; e < V; ++e)
    {
        const int cc = min(c + e, kCgmMaxK - 1);
        on[e]        = c + e < k && s_live[cc] != 0;
        alpha[e]     = s_alpha[cc];
        beta[e]      = s_beta[cc];
        any          = any || on[e];
        all          = all && on[e];
    }
    double rr[V] = {}, rz[V] = {};
    // the same fma forms as cg_fused_kernel's
    auto one = [&](int e, double wi, double ui, double& pi, double& si, double& xi, double& ri, double di, double& u_out) {
        pi    = fma(beta[e], pi, ui);
        si    = fma(beta[e], si, wi);
        xi    = fma(alpha[e], pi, xi);
        ri    = fma(-alpha[e], si, ri);
        u_out = PRE ? ri * di : ri;
        rr[e] = fma(ri, ri, rr[e]);
        if (PRE) rz[e] = fma(ri, u_out, rz[e]);
    };
    if (any)
        for (int64_t row = (int64_t)blockIdx.x * rpb + grp; row < n; row += (int64_t)gridDim.x * rpb)
        {
            const int64_t at = row * k + c;
            const double  d  = PRE ? dinv[row] : 1.0;
            if (V == 2 && all)
            {
                double wv[V], uv[V], pv[V], sv[V], xv[V], rv[V], uo[V];
                load_cols<V>(W + at, wv);
                load_cols<V>(R + at, rv);
                if (PRE) load_cols<V>(U + at, uv);
                load_cols<V>(P + at, pv);
                load_cols<V>(S + at, sv);
                load_cols<V>(X + at, xv);
#pragma unroll
                for (int e = 0; e < V; ++e) one(e, wv[e], PRE ? uv[e] : rv[e], pv[e], sv[e], xv[e], rv[e], d, uo[e]);
                store_cols<V>(P + at, pv);
                store_cols<V>(S + at, sv);
                store_cols<V>(X + at, xv);
                store_cols<V>(R + at, rv);
                if (PRE) store_cols<V>(U + at, uo);
            }
            else
            {
#pragma unroll
                for (int e = 0; e < V; ++e)
                    if (on[e])
                    {
                        const int64_t i  = at + e;
                        double        pi = P[i], si = S[i], xi = X[i], ri = R[i], uo;
                        one(e, W[i], PRE ? U[i] : ri, pi, si, xi, ri, d, uo);
                        P[i] = pi;
                        S[i] = si;
                        X[i] = xi;
                        R[i] = ri;
                        if (PRE) U[i] = uo;
                    }
            }
        }
    const int64_t plane = (int64_t)gridDim.x * k;
    store_partials<V>(rr, KP, k, part, s_part);
    if (PRE) store_partials<V>(rz, KP, k, part + plane, s_part);
    if (!took_last_ticket(&s->ticket)) return;
    const double t_rr = column_total(part, k, kc_log2, s_part);
    const double t_rz = PRE ? column_total(part + plane, k, kc_log2, s_part) : t_rr;
    if ((int)threadIdx.x < k && s_live[threadIdx.x] != 0)
    {
        const int cc     = threadIdx.x;
        s->gamma_old[cc] = s_gamma[cc];
        s->alpha_old[cc] = s_alpha[cc];
        s->gamma[cc]     = t_rz;
        s->rr[cc]        = t_rr;
    }
    if (threadIdx.x == 0) s->ticket = 0;
}

int log2_pow2_at_least(int v)
{
    int l = 0;
    while ((1 << l) < v) ++l;
    return l;
}
}  // namespace

int cg_multi_solve(spmv_ctx* ctx, const spmv_mat* A, int32_t k, const double* B, double* X, int max_iter, double rel_tol,
                   int check_every, int precond, int32_t* iters, double* rel_resid)
{
    const char* const who = "spmv_cg_multi";
    const int64_t     n   = A->nrow;
    for (int c = 0; c < k; ++c)
    {
        iters[c]     = 0;
        rel_resid[c] = 0.0;
    }
    if (n == 0) return SPMV_OK;
    hipStream_t  st = ctx->stream;
    const size_t nk = (size_t)n * (size_t)k;
    const bool   pre = precond == SPMV_PRECOND_JACOBI;
    // wide: 16-byte accesses, two columns per lane - every row then starts on a 16-byte boundary (k even) of 16-byte aligned arrays
    const bool wide    = (k % 2) == 0 && aligned16(X) && aligned16(B);
    const int  kp_log2 = log2_pow2_at_least(wide ? k / 2 : k);
    const int  kc_log2 = log2_pow2_at_least(k);
    const int  rpb     = kBlock >> kp_log2;
    const int  grid    = (int)std::max<int64_t>(1, std::min<int64_t>(kCgmMaxGrid, ceil_div(n, rpb)));
    // R, P, S, W, (Jacobi) U and dinv, and the partial sums of three quantities per column
    double *       R, *P, *S, *W, *U = nullptr, *dinv = nullptr, *part;
    CgmScalars*    s = nullptr;
    SolveWorkspace ws(ctx, who);
    for (double** piece : {&R, &P, &S, &W}) ws.piece(*piece, nk);
    if (pre) ws.piece(U, nk);
    if (pre) ws.piece(dinv, n);
    ws.piece(part, 3 * (size_t)grid * k);
    SPMV_TRY(ws.allocate((void**)&s, sizeof(CgmScalars)));
    SPMV_TRY(setup_preconditioner(ctx, A, precond, dinv, who));
    if (!U) U = R;  // M = I: the preconditioned residual is the residual itself
    CgmScalars           h;
    std::vector<int32_t> frozen(kCgmMaxK, 0);
    std::vector<double>  limit(k), rr(k);
    auto fetch = [&]() { return read_scalars(ctx, &h, s, sizeof(CgmScalars), who); };
    // the host's flags to the device, before the next iteration is queued
    auto freeze = [&]() { return write_scalars(ctx, s->frozen, frozen.data(), sizeof(int32_t) * kCgmMaxK, who, "writing the column flags"); };
#define SPMV_CGM_LAUNCH(KERNEL, ...)                                                                                      \
    do                                                                                                                    \
    {                                                                                                                     \
        if (wide)                                                                                                         \
            hipLaunchKernelGGL((KERNEL<2>), dim3(grid), dim3(kBlock), 0, st, n, (int)k, kp_log2, kc_log2, __VA_ARGS__);    \
        else                                                                                                              \
            hipLaunchKernelGGL((KERNEL<1>), dim3(grid), dim3(kBlock), 0, st, n, (int)k, kp_log2, kc_log2, __VA_ARGS__);    \
    } while (0)
#define SPMV_CGM_LAUNCH_PRE(KERNEL, ...)                                                                                      \
    do                                                                                                                        \
    {                                                                                                                         \
        if (pre && wide)                                                                                                      \
            hipLaunchKernelGGL((KERNEL<true, 2>), dim3(grid), dim3(kBlock), 0, st, n, (int)k, kp_log2, kc_log2, __VA_ARGS__);  \
        else if (pre)                                                                                                         \
            hipLaunchKernelGGL((KERNEL<true, 1>), dim3(grid), dim3(kBlock), 0, st, n, (int)k, kp_log2, kc_log2, __VA_ARGS__);  \
        else if (wide)                                                                                                        \
            hipLaunchKernelGGL((KERNEL<false, 2>), dim3(grid), dim3(kBlock), 0, st, n, (int)k, kp_log2, kc_log2, __VA_ARGS__); \
        else                                                                                                                  \
            hipLaunchKernelGGL((KERNEL<false, 1>), dim3(grid), dim3(kBlock), 0, st, n, (int)k, kp_log2, kc_log2, __VA_ARGS__); \
    } while (0)
    SPMV_TRY(spmm_apply(ctx, A, k, X, W, true));  // W = A X0
    SPMV_CGM_LAUNCH_PRE(cgm_init_kernel, B, (const double*)W, R, U, P, S, (const double*)dinv, part, s);
    SPMV_TRY(fetch());
    int live = 0;
    for (int c = 0; c < k; ++c)
    {
        const double bb = h.bb[c];
        rr[c]           = h.rr[c];
        limit[c]        = rel_tol * rel_tol * bb;  // squared norms are compared
        if (!std::isfinite(bb) || !std::isfinite(rr[c]))
            SPMV_FAIL(SPMV_ERR_INVALID, "spmv_cg_multi: column %d: b.b = %g, r0.r0 = %g: b, x0 or the matrix hold non-finite numbers", c, bb, rr[c]);
        if (!(bb > 0.0) || rr[c] <= limit[c])
        {
            // b_c = 0: x0 stays (spmv_cg's rule); else x0 already solves the system to rel_tol
            frozen[c]    = 1;
            rel_resid[c] = bb > 0.0 ? sqrt(rr[c] / bb) : 0.0;
        }
        else
            ++live;
    }
    if (live == 0) return SPMV_OK;
    if (live < k) SPMV_TRY(freeze());
    const int     every = std::max(1, check_every);
    const double* in    = U;  // the product runs on the (preconditioned) residual
    int           j = 0, rc = SPMV_OK;
    while (j < max_iter && live > 0)
    {
        if ((rc = spmm_apply(ctx, A, k, in, W, true)) != SPMV_OK) break;  // W = A U
        SPMV_CGM_LAUNCH(cgm_dots_kernel, in, (const double*)W, part, s);
        SPMV_CGM_LAUNCH_PRE(cgm_fused_kernel, (const double*)W, U, P, S, X, R, (const double*)dinv, part, s);
        ++j;
        if (j % every != 0 && j != max_iter) continue;
        if ((rc = fetch()) != SPMV_OK) break;
        bool changed = false;
        for (int c = 0; c < k; ++c)
        {
            if (frozen[c]) continue;
            rr[c] = h.rr[c];
            // the status word is set only with a residual to speak of; it is looked at first
            if (h.status[c] == 2 || !std::isfinite(rr[c]))
            {
                set_error("spmv_cg_multi: column %d: the residual is not finite at or before iteration %d (non-finite numbers in b, x0 or the matrix, or overflow)", c, j);
                rc = SPMV_ERR_INVALID;
                break;
            }
            if (h.status[c] != 0)
            {
                set_error("spmv_cg_multi: column %d: p.Ap <= 0 (or r.M^-1 r <= 0) at or before iteration %d: the matrix is not positive definite", c, j);
                rc = SPMV_ERR_INVALID;
                break;
            }
            if (rr[c] <= limit[c])
            {
                frozen[c]    = 1;
                iters[c]     = j;
                rel_resid[c] = sqrt(rr[c] / h.bb[c]);
                changed      = true;
                --live;
            }
        }
        if (rc != SPMV_OK) break;
        if (changed && live > 0 && (rc = freeze()) != SPMV_OK) break;
    }
    if (rc == SPMV_OK) rc = hip_step(hipGetLastError(), who, "a launch of the iteration");
    for (int c = 0; c < k; ++c)
        if (!frozen[c])
        {
            iters[c]     = j;
            rel_resid[c] = sqrt(rr[c] / h.bb[c]);
        }
#undef SPMV_CGM_LAUNCH
#undef SPMV_CGM_LAUNCH_PRE
    return rc;  // (the workspace waits for the stream and frees)
}
}  // namespace spmv
