// solver_bicgstab.hip — spmv_bicgstab: A x = b for a square, not necessarily symmetric A by BiCGSTAB, device-resident, on CDNA4 (gfx950).
//
// A is any handle the forward product (mat_apply_ex) takes: every format; a shard where it holds a square matrix.  The product is
// not changed and gets no kernel here; both products of an iteration are forward ones and run whatever kernel the handle runs.  No
// transposed state is built.  The recurrence is right-preconditioned BiCGSTAB, exactly as it runs (every vector has nrow entries):
//
//   r = b - A x;  rhat = r;  p = r;  rho = rhat.r
//   loop:
//     phat = M^-1 p;   v = A phat;   alpha = rho / (rhat.v)
//     s = r - alpha v; shat = M^-1 s; t = A shat
//     omega = (t.s) / (t.t)
//     x += alpha phat + omega shat;   r = s - omega t
//     rho' = rhat.r;  beta = (rho' / rho) * (alpha / omega)
//     p = r + beta (p - omega v);  rho = rho'
//
// M = I for SPMV_PRECOND_NONE: phat and shat are p and s themselves, no copies.  M = diag(A) of a CSR handle for
// SPMV_PRECOND_JACOBI.  M = L U, the ILU(0) factors of a CSR handle (ilu0.hip), for SPMV_PRECOND_ILU0: phat = M^-1 p and
// shat = M^-1 s are two applications (ilu0_apply: the level launches of two triangular solves each) in front of the two products,
// behind the plain flavours of the direction and half-step kernels; eight work vectors.  Right preconditioning: r is the
// residual of A x = b itself, so the stopping rule is on the true system.
//
// Seven launches per iteration:
//   1  mat_apply_ex              v = A phat (overwrite)
//   2  bicg_dot_kernel<false>    rhat.v
//   3  bicg_half_kernel          alpha = rho / rhat.v;  s = r - alpha v;  shat = dinv s (Jacobi)
//   4  mat_apply_ex              t = A shat (overwrite)
//   5  bicg_dot_kernel<true>     t.s and t.t (grid_totals<2>)
//   6  bicg_update_kernel        omega = t.s / t.t;  x += alpha phat + omega shat;  r = s - omega t;  rhat.r and r.r
//                                (grid_totals<2>); the workgroup with the last ticket forms beta from them and moves rho' into rho
//   7  bicg_direction_kernel     p = r + beta (p - omega v);  phat = dinv p (Jacobi)
// beta is formed behind launch 6's sums rather than in front of launch 7's loop: the same expression from the same numbers, and
// launch 7 then writes no scalar and needs no ticket.  The set-up is one product (v = A x0) and bicg_init_kernel: r, rhat, p (phat),
// b.b, r.r and rho = r.r.
//
// Every scalar stays in one device struct (BicgScalars); the host reads it every check_every iterations and after the last one.
// An iteration that starts with r.r at or below 1e-28 b.b (rounding noise of the recurrence; 0 ends the solve) passes quietly: its
// vector kernels leave x and every work vector they write alone.  t.t = 0 (s = 0: the half step landed) gives omega = 0,
// x += alpha phat, r = s; if the new r.r is above the floor that is a breakdown.  Breakdowns - rho = 0, rhat.v = 0 or omega = 0 with
// r.r above the floor, or one of them not finite - raise the status word, and the kernel that sees one leaves x and r alone, as do
// the launches behind it.
//
// Every dot product is DETERMINISTIC, by the last-ticket pattern of solver_common.hpp (grid_totals): no atomic adds in arrival
// order, no slotted accumulators.  A solve is exactly as reproducible as the product its handle runs.
//
// Vector kernels: kBlock threads, grid-stride loops, 64-bit indices, no scratch.  The work vectors are fresh 256-byte aligned pieces
// of one allocation and go in 16-byte accesses (two elements per lane, an odd last element by one extra lane); the caller's x
// (update) and b (init) go in 16-byte accesses where they are 16-byte aligned and have two entries or more, in 8-byte accesses
// otherwise (WIDE).  Work memory: r, rhat, p, v, s, t (Jacobi: dinv, phat, shat as well) and the partial sums of two quantities.
//
// Not part of the reference's API, so there is no reference output.  What pins it: every iterate x_k and the residual against
// BiCGSTAB in extended precision (tests/bicgstab_ref.py, tests/test_gpu_bicgstab.py).
#include <cmath>

#include "common.hpp"
#include "solver_common.hpp"
#include "solver_host.hpp"
#include "wave.hpp"

namespace spmv
{
namespace
{
enum : int32_t
{
    kBicgRho   = 1,  // rho = rhat.r is 0 or not finite at the start of an iteration
    kBicgRhatV = 2,  // rhat.v is 0, or alpha not finite
    kBicgOmega = 3   // omega is 0 with r.r above the floor, or not finite
};

struct BicgScalars
{
    double   alpha;     // rho / rhat.v, by launch 3
    double   omega;     // t.s / t.t, by launch 6
    double   beta;      // (rho' / rho) * (alpha / omega), by launch 6's last workgroup
    double   rho;       // rhat.r of the current r
    double   rho_new;   // rhat.r behind the update (kept beside rho for the host's look)
    double   rhv;       // rhat.v
    double   ts;        // t.s
    double   tt;        // t.t (directly behind ts: launch 5 writes both)
    double   rr;        // r.r: what the host looks at
    double   bb;        // b.b
    double   floor_rr;  // 1e-28 b.b, written by the host once b.b is known: at or below it r.r is rounding noise
    int32_t  status;    // 0, or the first breakdown (kBicg*)
    uint32_t ticket;    // workgroups of the current launch that have stored their partial sums
};

// an iteration takes its steps only from a residual above the floor and with no breakdown behind it
static __device__ __forceinline__ bool bicg_live(const BicgScalars* s) { return s->rr > s->floor_rr && s->status == 0; }

// r = b - q (q = A x0);  rhat = r;  p = r;  phat = dinv p (PRE);  b.b, r.r and rho = rhat.r = r.r.  WIDE: b is 16-byte aligned
template <bool WIDE, bool PRE>
__global__ __launch_bounds__(kBlock) void bicg_init_kernel(int64_t n, const double* __restrict__ b, const double* __restrict__ q,
                                                           const double* __restrict__ dinv, double* __restrict__ r,
                                                           double* __restrict__ rhat, double* __restrict__ p, double* __restrict__ phat,
                                                           double* __restrict__ part, BicgScalars* __restrict__ s)
{
    double acc[2] = {0.0, 0.0};  // b.b, r.r
    if constexpr (WIDE)
    {
        const int64_t npairs = n / 2;
        for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < npairs; i += (int64_t)gridDim.x * kBlock)
        {
            const f64x2 bv = ((const f64x2*)b)[i], qv = ((const f64x2*)q)[i];
            f64x2       rv;
#pragma unroll
            for (int e = 0; e < 2; ++e)
            {
                rv[e]  = bv[e] - qv[e];
                acc[0] = fma(bv[e], bv[e], acc[0]);
                acc[1] = fma(rv[e], rv[e], acc[1]);
            }
            ((f64x2*)r)[i]    = rv;
            ((f64x2*)rhat)[i] = rv;
            ((f64x2*)p)[i]    = rv;
            if constexpr (PRE)
            {
                const f64x2 dv       = ((const f64x2*)dinv)[i];
                ((f64x2*)phat)[i] = f64x2{dv[0] * rv[0], dv[1] * rv[1]};
            }
        }
    }
    // WIDE: the odd last element, by one lane;  otherwise every element, one per lane
    const bool    lead  = blockIdx.x == 0 && threadIdx.x == 0;
    const int64_t first = WIDE ? (((n & 1) && lead) ? n - 1 : n) : (int64_t)blockIdx.x * kBlock + threadIdx.x;
    for (int64_t i = first; i < n; i += (int64_t)gridDim.x * kBlock)
    {
        const double bi = b[i], ri = bi - q[i];
        r[i] = rhat[i] = p[i] = ri;
        if constexpr (PRE) phat[i] = dinv[i] * ri;
        acc[0] = fma(bi, bi, acc[0]);
        acc[1] = fma(ri, ri, acc[1]);
    }
    double total[2];
    if (!grid_totals<2>(acc, part, &s->ticket, total)) return;
    if (threadIdx.x == 0)
    {
        s->bb     = total[0];
        s->rr     = total[1];
        s->rho    = total[1];
        s->ticket = 0;
    }
}

// out[0] = a.c;  SELF: out[1] = a.a as well.  Complete work vectors: 16-byte accesses
template <bool SELF>
__global__ __launch_bounds__(kBlock) void bicg_dot_kernel(int64_t n, const double* __restrict__ a, const double* __restrict__ c,
                                                          double* __restrict__ out, double* __restrict__ part, BicgScalars* __restrict__ s)
{
    constexpr int NQ      = SELF ? 2 : 1;
    double        acc[NQ] = {};
    const int64_t npairs  = n / 2;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < npairs; i += (int64_t)gridDim.x * kBlock)
    {
        const f64x2 av = ((const f64x2*)a)[i], cv = ((const f64x2*)c)[i];
#pragma unroll
        for (int e = 0; e < 2; ++e)
        {
            acc[0] = fma(av[e], cv[e], acc[0]);
            if constexpr (SELF) acc[NQ - 1] = fma(av[e], av[e], acc[NQ - 1]);
        }
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0)
    {
        const double ai = a[n - 1];
        acc[0]          = fma(ai, c[n - 1], acc[0]);
        if constexpr (SELF) acc[NQ - 1] = fma(ai, ai, acc[NQ - 1]);
    }
    double total[NQ];
    if (!grid_totals<NQ>(acc, part, &s->ticket, total)) return;
    if (threadIdx.x == 0)
    {
#pragma unroll
        for (int q = 0; q < NQ; ++q) out[q] = total[q];
        s->ticket = 0;
    }
}

// alpha = rho / rhat.v;  sv = r - alpha v;  shat = dinv sv (PRE).  No sum and no scalar that this launch reads is written: no ticket
template <bool PRE>
__global__ __launch_bounds__(kBlock) void bicg_half_kernel(int64_t n, const double* __restrict__ r, const double* __restrict__ v,
                                                           const double* __restrict__ dinv, double* __restrict__ sv,
                                                           double* __restrict__ shat, BicgScalars* __restrict__ s)
{
    // (uniform over the grid: every thread reads the same scalars; the status word is raised only where every thread sees why)
    if (!bicg_live(s)) return;
    const double rho = s->rho, alpha = rho / s->rhv;
    const bool   lead = blockIdx.x == 0 && threadIdx.x == 0;
    if (!(rho != 0.0) || !isfinite(rho))
    {
        if (lead) s->status = kBicgRho;
        return;
    }
    if (!(s->rhv != 0.0) || !isfinite(alpha))
    {
        if (lead) s->status = kBicgRhatV;
        return;
    }
    if (lead) s->alpha = alpha;
    const int64_t npairs = n / 2;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < npairs; i += (int64_t)gridDim.x * kBlock)
    {
        const f64x2 rv = ((const f64x2*)r)[i], vv = ((const f64x2*)v)[i];
        const f64x2 t  = f64x2{fma(-alpha, vv[0], rv[0]), fma(-alpha, vv[1], rv[1])};
        ((f64x2*)sv)[i] = t;
        if constexpr (PRE)
        {
            const f64x2 dv       = ((const f64x2*)dinv)[i];
            ((f64x2*)shat)[i] = f64x2{dv[0] * t[0], dv[1] * t[1]};
        }
    }
    if ((n & 1) && lead)
    {
        const int64_t i = n - 1;
        const double  t = fma(-alpha, v[i], r[i]);
        sv[i]           = t;
        if constexpr (PRE) shat[i] = dinv[i] * t;
    }
}

// omega = t.s / t.t (0 where t.t = 0);  x += alpha phat + omega shat;  r = sv - omega t;  rhat.r and r.r.  The workgroup with the
// last ticket writes r.r, forms beta = (rho' / rho) * (alpha / omega) and moves rho' into rho.  WIDE: x is 16-byte aligned.
// (without Jacobi phat and shat are p and sv: read only here)
template <bool WIDE>
__global__ __launch_bounds__(kBlock) void bicg_update_kernel(int64_t n, const double* __restrict__ phat, const double* __restrict__ shat,
                                                             const double* __restrict__ sv, const double* __restrict__ t,
                                                             const double* __restrict__ rhat, double* __restrict__ x,
                                                             double* __restrict__ r, double* __restrict__ part, BicgScalars* __restrict__ s)
{
    const double alpha = s->alpha, ts = s->ts, tt = s->tt, rho = s->rho, floor_rr = s->floor_rr;
    bool         live  = bicg_live(s);
    const bool   landed = tt == 0.0;  // s = 0 (or A shat = 0): the half step is the whole step
    const double omega  = landed ? 0.0 : ts / tt;
    if (live && !landed && (!(omega != 0.0) || !isfinite(omega)))
    {
        if (blockIdx.x == 0 && threadIdx.x == 0) s->status = kBicgOmega;
        live = false;
    }
    const int64_t stride = (int64_t)gridDim.x * kBlock, first = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t npairs = n / 2;
    double        acc[2] = {0.0, 0.0};  // rhat.r, r.r
    if (live)
    {
        if constexpr (WIDE)
        {
            for (int64_t i = first; i < npairs; i += stride)
            {
                const f64x2 pv = ((const f64x2*)phat)[i], hv = ((const f64x2*)shat)[i];
                f64x2       xv = ((f64x2*)x)[i];
                xv[0]          = fma(omega, hv[0], fma(alpha, pv[0], xv[0]));
                xv[1]          = fma(omega, hv[1], fma(alpha, pv[1], xv[1]));
                ((f64x2*)x)[i] = xv;
            }
            if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) x[n - 1] = fma(omega, shat[n - 1], fma(alpha, phat[n - 1], x[n - 1]));
        }
        else
            for (int64_t i = first; i < n; i += stride) x[i] = fma(omega, shat[i], fma(alpha, phat[i], x[i]));
        for (int64_t i = first; i < npairs; i += stride)
        {
            const f64x2 s2 = ((const f64x2*)sv)[i], tv = ((const f64x2*)t)[i], hv = ((const f64x2*)rhat)[i];
            const f64x2 rv = f64x2{fma(-omega, tv[0], s2[0]), fma(-omega, tv[1], s2[1])};
            ((f64x2*)r)[i] = rv;
#pragma unroll
            for (int e = 0; e < 2; ++e)
            {
                acc[0] = fma(hv[e], rv[e], acc[0]);
                acc[1] = fma(rv[e], rv[e], acc[1]);
            }
        }
        if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0)
        {
            const int64_t i  = n - 1;
            const double  ri = fma(-omega, t[i], sv[i]);
            r[i]             = ri;
            acc[0]           = fma(rhat[i], ri, acc[0]);
            acc[1]           = fma(ri, ri, acc[1]);
        }
    }
    double total[2];
    if (!grid_totals<2>(acc, part, &s->ticket, total)) return;
    if (threadIdx.x == 0)
    {
        if (live)
        {
            const double rho_new = total[0], rr = total[1];
            const bool   go_on   = rr > floor_rr;
            if (landed && go_on) s->status = kBicgOmega;  // omega = 0 and a residual to speak of: no next direction
            s->omega   = omega;
            s->rho_new = rho_new;
            s->rr      = rr;
            s->beta    = go_on && !landed ? (rho_new / rho) * (alpha / omega) : 0.0;
            s->rho     = rho_new;
        }
        s->ticket = 0;
    }
}

// p = r + beta (p - omega v);  phat = dinv p (PRE).  Reads the scalars launch 6 left, writes none
template <bool PRE>
__global__ __launch_bounds__(kBlock) void bicg_direction_kernel(int64_t n, const double* __restrict__ r, const double* __restrict__ v,
                                                                const double* __restrict__ dinv, double* __restrict__ p,
                                                                double* __restrict__ phat, const BicgScalars* __restrict__ s)
{
    if (!bicg_live(s)) return;  // (r.r is the new one: at or below the floor no later iteration reads p)
    const double  beta = s->beta, omega = s->omega;
    const int64_t npairs = n / 2;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < npairs; i += (int64_t)gridDim.x * kBlock)
    {
        const f64x2 rv = ((const f64x2*)r)[i], vv = ((const f64x2*)v)[i];
        f64x2       pv = ((const f64x2*)p)[i];
        pv[0]          = fma(beta, fma(-omega, vv[0], pv[0]), rv[0]);
        pv[1]          = fma(beta, fma(-omega, vv[1], pv[1]), rv[1]);
        ((f64x2*)p)[i] = pv;
        if constexpr (PRE)
        {
            const f64x2 dv       = ((const f64x2*)dinv)[i];
            ((f64x2*)phat)[i] = f64x2{dv[0] * pv[0], dv[1] * pv[1]};
        }
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0)
    {
        const int64_t i  = n - 1;
        const double  pi = fma(beta, fma(-omega, v[i], p[i]), r[i]);
        p[i]             = pi;
        if constexpr (PRE) phat[i] = dinv[i] * pi;
    }
}
}  // namespace

int bicgstab_solve(spmv_ctx* ctx, const spmv_mat* A, const double* b, double* x, int max_iter, double rel_tol, int check_every,
                   int precond, int* iters, double* rel_resid)
{
    const char* const who = "spmv_bicgstab";
    const int64_t     n   = A->nrow;
    *iters                = 0;
    *rel_resid            = 0.0;
    if (n == 0) return SPMV_OK;
    hipStream_t st  = ctx->stream;
    const bool  jacobi = precond == SPMV_PRECOND_JACOBI, by_launches = applied_by_launches(precond);  // (by_launches: the column of precond.hpp's table)
    // r, rhat, p, v, s, t (Jacobi: dinv, phat, shat; ILU(0): phat, shat) and the partial sums of two quantities
    double *r, *rhat, *p, *v, *sv, *t, *dinv = nullptr, *phat = nullptr, *shat = nullptr, *part;
    BicgScalars*   s = nullptr;
    SolveWorkspace ws(ctx, who);
    for (double** piece : {&r, &rhat, &p, &v, &sv, &t}) ws.piece(*piece, n);
    if (jacobi) ws.piece(dinv, n);
    if (jacobi || by_launches) ws.piece(phat, n);
    if (jacobi || by_launches) ws.piece(shat, n);
    ws.piece(part, 2 * (size_t)kMaxGrid);
    SPMV_TRY(ws.allocate((void**)&s, sizeof(BicgScalars)));
    SPMV_TRY(setup_preconditioner(ctx, A, precond, dinv, who));
    if (!phat) phat = p, shat = sv;  // M = I: phat and shat are p and s themselves
    const bool  wide_x = wide_ok(x, n), wide_b = wide_ok(b, n);
    const int   grid   = pair_grid(n);
    const int   grid_x = wide_x ? grid : stream_grid(n), grid_b = wide_b ? grid : stream_grid(n);
    apply_extra over;
    over.overwrite = true;
    // the seven launches of an iteration (ILU(0): and the two applications phat = M^-1 p, shat = M^-1 s; in a quiet iteration they
    // run on the p and s that stand, which the update kernel then does not read)
    auto iteration = [&]() -> int {
        if (by_launches) SPMV_TRY(apply_preconditioner(ctx, A, precond, p, phat));
        SPMV_TRY(mat_apply_ex(ctx, A, phat, v, over));
        hipLaunchKernelGGL(bicg_dot_kernel<false>, dim3(grid), dim3(kBlock), 0, st, n, (const double*)rhat, (const double*)v, &s->rhv, part, s);
        if (jacobi)
            hipLaunchKernelGGL(bicg_half_kernel<true>, dim3(grid), dim3(kBlock), 0, st, n, (const double*)r, (const double*)v, (const double*)dinv, sv, shat, s);
        else
            hipLaunchKernelGGL(bicg_half_kernel<false>, dim3(grid), dim3(kBlock), 0, st, n, (const double*)r, (const double*)v, (const double*)dinv, sv, shat, s);
        if (by_launches) SPMV_TRY(apply_preconditioner(ctx, A, precond, sv, shat));
        SPMV_TRY(mat_apply_ex(ctx, A, shat, t, over));
        hipLaunchKernelGGL(bicg_dot_kernel<true>, dim3(grid), dim3(kBlock), 0, st, n, (const double*)t, (const double*)sv, &s->ts, part, s);
        if (wide_x)
            hipLaunchKernelGGL(bicg_update_kernel<true>, dim3(grid_x), dim3(kBlock), 0, st, n, (const double*)phat, (const double*)shat, (const double*)sv,
                               (const double*)t, (const double*)rhat, x, r, part, s);
        else
            hipLaunchKernelGGL(bicg_update_kernel<false>, dim3(grid_x), dim3(kBlock), 0, st, n, (const double*)phat, (const double*)shat, (const double*)sv,
                               (const double*)t, (const double*)rhat, x, r, part, s);
        if (jacobi)
            hipLaunchKernelGGL(bicg_direction_kernel<true>, dim3(grid), dim3(kBlock), 0, st, n, (const double*)r, (const double*)v, (const double*)dinv, p, phat,
                               (const BicgScalars*)s);
        else
            hipLaunchKernelGGL(bicg_direction_kernel<false>, dim3(grid), dim3(kBlock), 0, st, n, (const double*)r, (const double*)v, (const double*)dinv, p, phat,
                               (const BicgScalars*)s);
        return SPMV_OK;
    };
    BicgScalars h;
    auto        fetch = [&]() { return read_scalars(ctx, &h, s, sizeof(BicgScalars), who); };
    // s (and shat) are read by the second product of a quiet iteration that never wrote them
    SPMV_TRY(hip_step(hipMemsetAsync(sv, 0, sizeof(double) * (size_t)n, st), who, "clearing s"));
    if (jacobi) SPMV_TRY(hip_step(hipMemsetAsync(shat, 0, sizeof(double) * (size_t)n, st), who, "clearing shat"));
    SPMV_TRY(mat_apply_ex(ctx, A, x, v, over));  // v = A x0
#define SPMV_BICG_INIT(WIDE, PRE)                                                                                                                  \
    hipLaunchKernelGGL((bicg_init_kernel<WIDE, PRE>), dim3(grid_b), dim3(kBlock), 0, st, n, b, (const double*)v, (const double*)dinv, r, rhat, p, phat, \
                       part, s)
    if (wide_b)
    {
        if (jacobi) SPMV_BICG_INIT(true, true); else SPMV_BICG_INIT(true, false);
    }
    else
    {
        if (jacobi) SPMV_BICG_INIT(false, true); else SPMV_BICG_INIT(false, false);
    }
#undef SPMV_BICG_INIT
    SPMV_TRY(fetch());
    const double bb = h.bb;
    double       rr = h.rr;
    if (!std::isfinite(bb) || !std::isfinite(rr))
        SPMV_FAIL(SPMV_ERR_INVALID, "spmv_bicgstab: b.b = %g, r0.r0 = %g: b, x0 or the matrix hold non-finite numbers", bb, rr);
    if (!(bb > 0.0)) return SPMV_OK;  // b = 0: x0 stays, as spmv_cg leaves it
    const double limit = rel_tol * rel_tol * bb;  // squared norms are compared
    int          k = 0, rc = SPMV_OK;
    if (rr > limit && rr > 0.0 && max_iter > 0)
    {
        const double floor_rr = 1e-28 * bb;
        SPMV_TRY(write_scalars(ctx, &s->floor_rr, &floor_rr, sizeof(double), who, "writing the noise floor"));
        const int every = std::max(1, check_every);
        while (k < max_iter)
        {
            if ((rc = iteration()) != SPMV_OK) break;
            ++k;
            if (k % every != 0 && k != max_iter) continue;
            if ((rc = fetch()) != SPMV_OK) break;
            rr = h.rr;
            if (!std::isfinite(rr))
            {
                set_error("spmv_bicgstab: r.r is not finite at or before iteration %d (non-finite numbers in the matrix, or overflow)", k);
                rc = SPMV_ERR_INVALID;
                break;
            }
            // (a breakdown behind an iterate that is within the tolerance is no error: x holds that iterate)
            if (rr <= limit || rr == 0.0) break;
            if (h.status != 0)
            {
                const char* what = h.status == kBicgRho ? "rho = rhat.r" : h.status == kBicgRhatV ? "rhat.v" : "omega = t.s / t.t";
                set_error("spmv_bicgstab: breakdown: %s is zero (or not finite) at or before iteration %d with a residual to speak of", what, k);
                rc = SPMV_ERR_INVALID;
                break;
            }
            if (!std::isfinite(h.rho))
            {
                set_error("spmv_bicgstab: rho = rhat.r is not finite at or before iteration %d (overflow)", k);
                rc = SPMV_ERR_INVALID;
                break;
            }
        }
        if (rc == SPMV_OK) rc = hip_step(hipGetLastError(), who, "a launch of the iteration");
    }
    *iters     = k;
    *rel_resid = sqrt(rr / bb);
    return rc;  // (the workspace waits for the stream and frees)
}
}  // namespace spmv
