// solver_minres.hip — spmv_minres: (A - shift I) x = b for a square SYMMETRIC A that need not be definite, by Paige and Saunders'
// preconditioned MINRES, device-resident, on CDNA4 (gfx950).
//
// A is any handle the forward product (mat_apply_ex) takes: every format; a shard where it holds a square matrix.  The product is
// not changed and gets no kernel here; no transposed state is built; nothing checks the symmetry.  The shift is applied in the
// vector kernel behind the product, so it costs nothing and works for every format.  M is the preconditioner `precond` of the handle
// P (A itself where P is null): it must be symmetric positive definite, which one built from an indefinite A is not - hence P.
// The recurrence, exactly as it runs (every vector has nrow entries):
//
//   r1 = b - (A - shift I) x0;  y = M^-1 r1;  beta1 = sqrt(r1.y);  r2 = r1;  beta = beta1;  oldb = 0;  dbar = epsln = 0;
//   phibar = beta1;  cs = -1;  sn = 0;  w = w2 = 0
//   loop:
//     v = y / beta;   y = A v - shift v;   from the second iteration on  y -= (beta / oldb) r1
//     alfa = v.y;     y -= (alfa / beta) r2;   r1 = r2;  r2 = y;  y = M^-1 r2;   oldb = beta;  beta = sqrt(r2.y)
//     oldeps = epsln;  delta = cs dbar + sn alfa;  gbar = sn dbar - cs alfa;  epsln = sn beta;  dbar = -cs beta
//     gamma = sqrt(gbar^2 + beta^2);  cs = gbar / gamma;  sn = beta / gamma;  phi = cs phibar;  phibar = sn phibar
//     w1 = w2;  w2 = w;  w = (v - oldeps w1 - delta w2) / gamma;   x += phi w
//
// phibar is ||r_k|| in the M^-1 norm: the 2-norm for SPMV_PRECOND_NONE.  The stopping rule compares it with beta_b = sqrt(b.M^-1 b),
// which does not depend on x0 and costs one more preconditioner application at the set-up.
//
// FOUR launches per iteration without a preconditioner and with Jacobi:
//   1  mat_apply_ex              q = A v (overwrite), into the buffer that is free
//   2  minres_lanczos_kernel     q = q - shift v - (beta / oldb) r1, and alfa = v.q (grid_totals<1>)
//   3  minres_resid_kernel       q -= (alfa / beta) r2: the new r2;  y = dinv r2 (Jacobi);  r2.y (grid_totals<1>); the workgroup with
//                                the last ticket does the rotation arithmetic (minres_rotate: beta .. phibar, the iteration count)
//   4  minres_update_kernel      w1's buffer takes w = (v - oldeps w1 - delta w2) / gamma;  x += phi w;  v = y / beta for the next product
// A preconditioner applied by launches (Chebyshev, AMG, FSAI) adds its own sequence and one dot kernel: launch 3 forms r2 alone,
// apply_preconditioner writes y, and minres_dot_kernel takes r2.y and carries the rotation.  The vector kernels of the four-launch
// shape read or write 15 doubles per row (launch 2: q, v, r1 in, q out; launch 3: q, r2 in, q out; launch 4: v, w1, w2, y, x in,
// w, x, v out); Jacobi adds dinv in and y out.
//
// Vectors rotate by pointer on the host, no copies: the old r1 is dead behind launch 2 and is the next product's output, the new w
// overwrites w1 in place.  Work memory, all of one SolveWorkspace for the duration of the call: SIX vectors without a preconditioner
// (r1, r2, the product's output, v, w, w2: y is r2), SEVEN with one (y), EIGHT with Jacobi (dinv), the partial sums of three
// quantities and the scalar block (MinresScalars).
//
// Every scalar stays in MinresScalars on the device; the host reads it every check_every iterations and after the last one.  An
// iteration that starts with phibar at or below the floor 1e-14 beta_b passes quietly: its kernels write nothing (this recurrence
// divides a vector by a norm, as spmv_gmres does).  beta = 0 - the Krylov space is exhausted, the iterate exact - gives sn = 0 and
// phibar = 0 and is such a case: launch 4 still takes the step into x and forms no next v.  r2.y below zero BEYOND ROUNDING - below
// -(4 floor)^2 = -16 * (1e-14 beta_b)^2 - says that M is not positive definite and raises the status word; between that and zero it
// is rounding and counts as 0.  A non-finite alfa, beta or phibar raises it too.  The kernel that raises it leaves x alone, as do
// the launches behind it.  gamma = 0 cannot happen while beta > 0 and has no clamp.
//
// Every dot product is DETERMINISTIC, by the last-ticket pattern of solver_common.hpp (grid_totals).  Vector kernels: kBlock threads,
// grid-stride loops, 64-bit indices, no scratch; the work vectors go in 16-byte accesses (two elements per lane, an odd last
// element by one extra lane), the caller's x (launch 4) and b and x (set-up) in 16-byte accesses where they are 16-byte aligned and
// have two entries or more, in 8-byte accesses otherwise (WIDE).
//
// Not part of the reference's API.  What pins it: every iterate x_k and phibar against the recurrence in extended precision
// (tests/minres_ref.py, tests/test_gpu_minres.py).
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
    kMinresNotSpd = 1,  // r2.y = r.M^-1 r below zero beyond rounding
    kMinresAlfa   = 2,  // alfa = v.y not finite
    kMinresBeta   = 3,  // beta not finite
    kMinresPhibar = 4   // gamma, and with it phibar, not finite
};
enum : int
{
    kDotBetaB  = 0,  // minres_dot_kernel: b.M^-1 b
    kDotStart  = 1,  //   r1.y of the set-up
    kDotRotate = 2   //   r2.y of an iteration
};
constexpr double kFloorRel    = 1e-14;  // the floor on phibar, in units of beta_b
constexpr double kNegMultiple = 4.0;    // r.M^-1 r below -(kNegMultiple floor)^2 is not rounding

struct MinresScalars
{
    double   alfa;      // v.y, by launch 2
    double   beta;      // sqrt(r2.y) of the current r2
    double   oldb;      // the beta before it
    double   dbar, epsln, oldeps, delta, gamma, cs, sn, phi;
    double   phibar;    // ||r_k|| in the M^-1 norm: what the host looks at
    double   ry;        // the last r2.y as it was summed (the host's message where it is negative)
    double   bb;        // b.b
    double   bmb;       // b.M^-1 b = beta_b^2
    double   floor;     // 1e-14 beta_b, written by the host once beta_b is known
    int32_t  status;    // 0, or the first trouble (kMinres*)
    int32_t  it;        // iterations that took their step
    int32_t  stepped;   // the iteration in flight took its step: launch 4 writes w and x
    uint32_t ticket;    // workgroups of the current launch that have stored their partial sums
};

// an iteration takes its step only from a residual above the floor and with no trouble behind it
static __device__ __forceinline__ bool minres_live(const MinresScalars* s) { return s->phibar > s->floor && s->status == 0; }

// the set-up's last word: beta1 = sqrt(r1.y) and the scalars of iteration 0 (one thread; the host judges the sign of r1.y)
static __device__ __forceinline__ void minres_start(MinresScalars* s, double ry)
{
    const double beta1 = sqrt(fmax(ry, 0.0));
    s->ry              = ry;
    s->beta            = !(ry == ry) ? ry : beta1;  // (a NaN stays one for the host to see)
    s->phibar          = s->beta;
    s->oldb = s->dbar = s->epsln = s->sn = 0.0;
    s->cs                                = -1.0;
}

// the rotation arithmetic behind r2.y (one thread of the workgroup with the last ticket): oldb, beta, the plane rotation, phi, phibar
static __device__ __forceinline__ void minres_rotate(MinresScalars* s, double ry, bool live)
{
    s->stepped = 0;
    if (!live) return;
    const double alfa = s->alfa, fl = kNegMultiple * s->floor;
    s->ry = ry;
    if (!isfinite(alfa))
    {
        s->status = kMinresAlfa;
        return;
    }
    if (!isfinite(ry))
    {
        s->beta   = ry;
        s->status = kMinresBeta;
        return;
    }
    if (ry < -(fl * fl))
    {
        s->status = kMinresNotSpd;
        return;
    }
    const double beta = sqrt(fmax(ry, 0.0)), cs = s->cs, sn = s->sn, dbar = s->dbar;
    const double delta = cs * dbar + sn * alfa, gbar = sn * dbar - cs * alfa;
    const double gamma = sqrt(gbar * gbar + beta * beta);
    const double cs1 = gbar / gamma, sn1 = beta / gamma, phibar = sn1 * s->phibar;
    if (!isfinite(phibar) || !isfinite(cs1))
    {
        s->gamma  = gamma;
        s->status = kMinresPhibar;
        return;
    }
    s->oldb   = s->beta;
    s->beta   = beta;
    s->oldeps = s->epsln;
    s->delta  = delta;
    s->epsln  = sn * beta;
    s->dbar   = -cs * beta;
    s->gamma  = gamma;
    s->cs     = cs1;
    s->sn     = sn1;
    s->phi    = cs1 * s->phibar;
    s->phibar = phibar;
    s->it += 1;
    s->stepped = 1;
}

// set-up: r2 = b - q + shift x0 (q = A x0);  y = dinv r2 (PRE);  b.b, b.M^-1 b and r2.y (PRE: with dinv; else M = I, which the
// by-launches preconditioners put right with two dot kernels).  WIDE: b and x0 are 16-byte aligned
template <bool WIDE, bool PRE>
__global__ __launch_bounds__(kBlock) void minres_init_kernel(int64_t n, const double* __restrict__ b, const double* __restrict__ x0,
                                                             const double* __restrict__ q, double shift, const double* __restrict__ dinv,
                                                             double* __restrict__ r2, double* __restrict__ y, double* __restrict__ part,
                                                             MinresScalars* __restrict__ s)
{
    double acc[3] = {0.0, 0.0, 0.0};  // b.b, b.M^-1 b, r2.y
    if constexpr (WIDE)
    {
        const int64_t npairs = n / 2;
        for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < npairs; i += (int64_t)gridDim.x * kBlock)
        {
            const f64x2 bv = ((const f64x2*)b)[i], xv = ((const f64x2*)x0)[i], qv = ((const f64x2*)q)[i];
            f64x2       dv = f64x2{1.0, 1.0}, rv, yv;
            if constexpr (PRE) dv = ((const f64x2*)dinv)[i];
#pragma unroll
            for (int e = 0; e < 2; ++e)
            {
                rv[e]  = fma(shift, xv[e], bv[e] - qv[e]);
                yv[e]  = PRE ? dv[e] * rv[e] : rv[e];
                acc[0] = fma(bv[e], bv[e], acc[0]);
                acc[1] = fma(PRE ? dv[e] * bv[e] : bv[e], bv[e], acc[1]);
                acc[2] = fma(rv[e], yv[e], acc[2]);
            }
            ((f64x2*)r2)[i] = rv;
            if constexpr (PRE) ((f64x2*)y)[i] = yv;
        }
    }
    // WIDE: the odd last element, by one lane;  otherwise every element, one per lane
    const bool    lead  = blockIdx.x == 0 && threadIdx.x == 0;
    const int64_t first = WIDE ? (((n & 1) && lead) ? n - 1 : n) : (int64_t)blockIdx.x * kBlock + threadIdx.x;
    for (int64_t i = first; i < n; i += (int64_t)gridDim.x * kBlock)
    {
        const double bi = b[i], ri = fma(shift, x0[i], bi - q[i]), di = PRE ? dinv[i] : 1.0, yi = PRE ? di * ri : ri;
        r2[i] = ri;
        if constexpr (PRE) y[i] = yi;
        acc[0] = fma(bi, bi, acc[0]);
        acc[1] = fma(PRE ? di * bi : bi, bi, acc[1]);
        acc[2] = fma(ri, yi, acc[2]);
    }
    double total[3];
    if (!grid_totals<3>(acc, part, &s->ticket, total)) return;
    if (threadIdx.x == 0)
    {
        s->bb  = total[0];
        s->bmb = total[1];
        minres_start(s, total[2]);
        s->ticket = 0;
    }
}

// a.c of two complete work vectors, and what hangs on it (what): b.M^-1 b, the set-up's r1.y, or an iteration's r2.y with the rotation
__global__ __launch_bounds__(kBlock) void minres_dot_kernel(int64_t n, const double* __restrict__ a, const double* __restrict__ c, int what,
                                                            double* __restrict__ part, MinresScalars* __restrict__ s)
{
    const bool    live   = what != kDotRotate || minres_live(s);
    double        acc[1] = {0.0};
    const int64_t npairs = n / 2;
    if (live)
    {
        for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < npairs; i += (int64_t)gridDim.x * kBlock)
        {
            const f64x2 av = ((const f64x2*)a)[i], cv = ((const f64x2*)c)[i];
            acc[0]         = fma(av[1], cv[1], fma(av[0], cv[0], acc[0]));
        }
        if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) acc[0] = fma(a[n - 1], c[n - 1], acc[0]);
    }
    double total[1];
    if (!grid_totals<1>(acc, part, &s->ticket, total)) return;
    if (threadIdx.x == 0)
    {
        if (what == kDotBetaB)
            s->bmb = total[0];
        else if (what == kDotStart)
            minres_start(s, total[0]);
        else
            minres_rotate(s, total[0], live);
        s->ticket = 0;
    }
}

// v = y / beta: the first Lanczos vector (the later ones are launch 4's).  Reads the scalars, writes none
__global__ __launch_bounds__(kBlock) void minres_first_kernel(int64_t n, const double* __restrict__ y, double* __restrict__ v,
                                                              const MinresScalars* __restrict__ s)
{
    if (!minres_live(s)) return;
    const double  beta   = s->beta;
    const int64_t npairs = n / 2;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < npairs; i += (int64_t)gridDim.x * kBlock)
    {
        const f64x2 yv = ((const f64x2*)y)[i];
        ((f64x2*)v)[i] = f64x2{yv[0] / beta, yv[1] / beta};
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) v[n - 1] = y[n - 1] / beta;
}

// launch 2: q = q - shift v - (beta / oldb) r1 (the last term from the second iteration on), and alfa = v.q
__global__ __launch_bounds__(kBlock) void minres_lanczos_kernel(int64_t n, double shift, const double* __restrict__ v, const double* __restrict__ r1,
                                                                double* __restrict__ q, double* __restrict__ part, MinresScalars* __restrict__ s)
{
    // (uniform over the grid: every thread reads the same scalars, ahead of the ticket that lets the last workgroup write alfa)
    const bool    live   = minres_live(s), second = s->it > 0;
    const double  c1     = second ? s->beta / s->oldb : 0.0;
    double        acc[1] = {0.0};
    const int64_t npairs = n / 2;
    if (live)
    {
        for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < npairs; i += (int64_t)gridDim.x * kBlock)
        {
            const f64x2 vv = ((const f64x2*)v)[i];
            f64x2       qv = ((f64x2*)q)[i];
            qv[0]          = fma(-shift, vv[0], qv[0]);
            qv[1]          = fma(-shift, vv[1], qv[1]);
            if (second)
            {
                const f64x2 rv = ((const f64x2*)r1)[i];
                qv[0]          = fma(-c1, rv[0], qv[0]);
                qv[1]          = fma(-c1, rv[1], qv[1]);
            }
            ((f64x2*)q)[i] = qv;
            acc[0]         = fma(vv[1], qv[1], fma(vv[0], qv[0], acc[0]));
        }
        if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0)
        {
            const int64_t i  = n - 1;
            double        qi = fma(-shift, v[i], q[i]);
            if (second) qi = fma(-c1, r1[i], qi);
            q[i]   = qi;
            acc[0] = fma(v[i], qi, acc[0]);
        }
    }
    double total[1];
    if (!grid_totals<1>(acc, part, &s->ticket, total)) return;
    if (threadIdx.x == 0)
    {
        if (live) s->alfa = total[0];
        s->ticket = 0;
    }
}

// launch 3: q -= (alfa / beta) r2, which makes q the new r2;  PRE: y = dinv q;  DOT: r2.y (PRE: q.y, else q.q) and the rotation.
// Without DOT (a preconditioner applied by launches forms y next) no sum is taken and no scalar written: no ticket
template <bool PRE, bool DOT>
__global__ __launch_bounds__(kBlock) void minres_resid_kernel(int64_t n, const double* __restrict__ r2, const double* __restrict__ dinv,
                                                              double* __restrict__ q, double* __restrict__ y, double* __restrict__ part,
                                                              MinresScalars* __restrict__ s)
{
    const bool    live   = minres_live(s);
    const double  c2     = s->alfa / s->beta;
    double        acc[1] = {0.0};
    const int64_t npairs = n / 2;
    if (live)
    {
        for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < npairs; i += (int64_t)gridDim.x * kBlock)
        {
            const f64x2 rv = ((const f64x2*)r2)[i];
            f64x2       qv = ((f64x2*)q)[i], yv;
            qv[0]          = fma(-c2, rv[0], qv[0]);
            qv[1]          = fma(-c2, rv[1], qv[1]);
            ((f64x2*)q)[i] = qv;
            yv             = qv;
            if constexpr (PRE)
            {
                const f64x2 dv = ((const f64x2*)dinv)[i];
                yv             = f64x2{dv[0] * qv[0], dv[1] * qv[1]};
                ((f64x2*)y)[i] = yv;
            }
            if constexpr (DOT) acc[0] = fma(qv[1], yv[1], fma(qv[0], yv[0], acc[0]));
        }
        if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0)
        {
            const int64_t i  = n - 1;
            const double  qi = fma(-c2, r2[i], q[i]);
            double        yi = qi;
            q[i]             = qi;
            if constexpr (PRE) y[i] = yi = dinv[i] * qi;
            if constexpr (DOT) acc[0] = fma(qi, yi, acc[0]);
        }
    }
    if constexpr (DOT)
    {
        double total[1];
        if (!grid_totals<1>(acc, part, &s->ticket, total)) return;
        if (threadIdx.x == 0)
        {
            minres_rotate(s, total[0], live);
            s->ticket = 0;
        }
    }
}

// launch 4: w = (v - oldeps w1 - delta w2) / gamma into w1's place;  x += phi w;  and, where the solve goes on, v = y / beta for the
// next product.  Reads the scalars the rotation left, writes none.  WIDE: x is 16-byte aligned
template <bool WIDE>
__global__ __launch_bounds__(kBlock) void minres_update_kernel(int64_t n, const double* __restrict__ y, const double* __restrict__ w2,
                                                               double* __restrict__ w1, double* __restrict__ v, double* __restrict__ x,
                                                               const MinresScalars* __restrict__ s)
{
    if (!s->stepped) return;
    const bool    next = minres_live(s);  // (phibar is the new one: at or below the floor no later iteration reads v)
    const double  oldeps = s->oldeps, delta = s->delta, gamma = s->gamma, phi = s->phi, beta = s->beta;
    const int64_t npairs = n / 2;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < npairs; i += (int64_t)gridDim.x * kBlock)
    {
        const f64x2 vv = ((const f64x2*)v)[i], av = ((const f64x2*)w1)[i], cv = ((const f64x2*)w2)[i];
        f64x2       wv;
        wv[0]           = fma(-delta, cv[0], fma(-oldeps, av[0], vv[0])) / gamma;
        wv[1]           = fma(-delta, cv[1], fma(-oldeps, av[1], vv[1])) / gamma;
        ((f64x2*)w1)[i] = wv;
        if constexpr (WIDE)
        {
            f64x2 xv       = ((f64x2*)x)[i];
            xv[0]          = fma(phi, wv[0], xv[0]);
            xv[1]          = fma(phi, wv[1], xv[1]);
            ((f64x2*)x)[i] = xv;
        }
        else
        {
            x[2 * i]     = fma(phi, wv[0], x[2 * i]);
            x[2 * i + 1] = fma(phi, wv[1], x[2 * i + 1]);
        }
        if (next)
        {
            const f64x2 yv = ((const f64x2*)y)[i];
            ((f64x2*)v)[i] = f64x2{yv[0] / beta, yv[1] / beta};
        }
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0)
    {
        const int64_t i  = n - 1;
        const double  wi = fma(-delta, w2[i], fma(-oldeps, w1[i], v[i])) / gamma;
        w1[i]            = wi;
        x[i]             = fma(phi, wi, x[i]);
        if (next) v[i] = y[i] / beta;
    }
}

// flag != 0: an entry of dinv that is not above zero
__global__ __launch_bounds__(kBlock) void minres_dinv_sign_kernel(int64_t n, const double* __restrict__ dinv, int* __restrict__ flag)
{
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) bad |= !(dinv[i] > 0.0);
    if (bad) atomicOr(flag, 1);
}

// Jacobi's 1 / p_ii must all be positive (the flag is the first word of the context's scratch; synchronous)
int check_positive_diagonal(spmv_ctx* ctx, const double* dinv, int64_t n, const char* who)
{
    SPMV_TRY(ensure_scratch(ctx, 64));
    int* flag   = (int*)ctx->scratch;
    int  h_flag = 0;
    SPMV_TRY(hip_step(hipMemsetAsync(flag, 0, sizeof(int), ctx->stream), who, "clearing the sign flag"));
    hipLaunchKernelGGL(minres_dinv_sign_kernel, dim3(stream_grid(n)), dim3(kBlock), 0, ctx->stream, n, dinv, flag);
    SPMV_TRY(read_scalars(ctx, &h_flag, flag, sizeof(int), who));
    SPMV_REQUIRE(h_flag == 0, "%s: the Jacobi preconditioner is not positive definite (a diagonal entry of its matrix is negative)", who);
    return SPMV_OK;
}
}  // namespace

int minres_solve(spmv_ctx* ctx, const spmv_mat* A, const spmv_mat* P, const double* b, double* x, double shift, int max_iter, double rel_tol,
                 int check_every, int precond, int* iters, double* rel_resid)
{
    const char* const who = "spmv_minres";
    const int64_t     n   = A->nrow;
    *iters                = 0;
    *rel_resid            = 0.0;
    if (n == 0) return SPMV_OK;
    if (!P) P = A;
    hipStream_t st     = ctx->stream;
    const bool  jacobi = precond == SPMV_PRECOND_JACOBI, by_launches = applied_by_launches(precond);  // (by_launches: the column of precond.hpp's table)
    // r1, r2, the product's output, v, w, w2 (a preconditioner: y as well; Jacobi: dinv) and the partial sums of three quantities
    double *r1, *r2, *q, *v, *w, *w2, *y = nullptr, *dinv = nullptr, *part;
    MinresScalars* s = nullptr;
    SolveWorkspace ws(ctx, who);
    for (double** piece : {&r1, &r2, &q, &v, &w, &w2}) ws.piece(*piece, n);
    if (jacobi || by_launches) ws.piece(y, n);
    if (jacobi) ws.piece(dinv, n);
    ws.piece(part, 3 * (size_t)kMaxGrid);
    SPMV_TRY(ws.allocate((void**)&s, sizeof(MinresScalars)));
    SPMV_TRY(setup_preconditioner(ctx, P, precond, dinv, who));
    if (jacobi) SPMV_TRY(check_positive_diagonal(ctx, dinv, n, who));
    const bool  wide_x = wide_ok(x, n), wide_bx = wide_x && wide_ok(b, n);
    const int   grid = pair_grid(n), grid_bx = wide_bx ? grid : stream_grid(n);
    const size_t bytes = sizeof(double) * (size_t)n;
    apply_extra over;
    over.overwrite = true;
    MinresScalars h;
    auto          fetch = [&]() { return read_scalars(ctx, &h, s, sizeof(MinresScalars), who); };
    auto          dot   = [&](const double* a, const double* c, int what) {
        hipLaunchKernelGGL(minres_dot_kernel, dim3(grid), dim3(kBlock), 0, st, n, a, c, what, part, s);
    };
    // ---- the set-up: r2 = b - (A - shift I) x0, y = M^-1 r2, beta1, beta_b ---------------------------------------------------------
    SPMV_TRY(hip_step(hipMemsetAsync(w, 0, bytes, st), who, "clearing w"));
    SPMV_TRY(hip_step(hipMemsetAsync(w2, 0, bytes, st), who, "clearing w2"));
    SPMV_TRY(mat_apply_ex(ctx, A, x, q, over));  // q = A x0
#define SPMV_MINRES_INIT(WIDE, PRE)                                                                                                                \
    hipLaunchKernelGGL((minres_init_kernel<WIDE, PRE>), dim3(grid_bx), dim3(kBlock), 0, st, n, b, (const double*)x, (const double*)q, shift, \
                       (const double*)dinv, r2, y, part, s)
    if (wide_bx)
    {
        if (jacobi) SPMV_MINRES_INIT(true, true); else SPMV_MINRES_INIT(true, false);
    }
    else
    {
        if (jacobi) SPMV_MINRES_INIT(false, true); else SPMV_MINRES_INIT(false, false);
    }
#undef SPMV_MINRES_INIT
    if (by_launches)
    {
        // b.M^-1 b over an aligned copy of b (r1's buffer is free until the second iteration), then r1.y
        SPMV_TRY(hip_step(hipMemcpyAsync(r1, b, bytes, hipMemcpyDeviceToDevice, st), who, "copying b"));
        SPMV_TRY(apply_preconditioner(ctx, P, precond, r1, y));
        dot(r1, y, kDotBetaB);
        SPMV_TRY(apply_preconditioner(ctx, P, precond, r2, y));
        dot(r2, y, kDotStart);
    }
    if (!y) y = r2;  // M = I: y is r2 itself
    SPMV_TRY(fetch());
    if (!std::isfinite(h.bb)) SPMV_FAIL(SPMV_ERR_INVALID, "spmv_minres: b.b = %g: b holds non-finite numbers", h.bb);
    if (!std::isfinite(h.bmb)) SPMV_FAIL(SPMV_ERR_INVALID, "spmv_minres: b.M^-1 b = %g is not finite (non-finite numbers in the preconditioner)", h.bmb);
    if (!std::isfinite(h.beta))
        SPMV_FAIL(SPMV_ERR_INVALID, "spmv_minres: beta1 = sqrt(r.M^-1 r) of x0 is not finite (r.M^-1 r = %g): x0, the matrix or the preconditioner hold non-finite numbers", h.ry);
    if (!(h.bb > 0.0)) return SPMV_OK;  // b = 0: x0 stays, as spmv_cg leaves it
    if (h.bmb < 0.0) SPMV_FAIL(SPMV_ERR_INVALID, "spmv_minres: preconditioner is not positive definite (b.M^-1 b = %g) at or before iteration 0", h.bmb);
    if (!(h.bmb > 0.0)) return SPMV_OK;  // (M^-1 b = 0: nothing to measure a residual against)
    const double beta_b = sqrt(h.bmb), floor_phi = kFloorRel * beta_b, limit = rel_tol * beta_b;
    if (h.ry < -(kNegMultiple * floor_phi) * (kNegMultiple * floor_phi))
        SPMV_FAIL(SPMV_ERR_INVALID, "spmv_minres: preconditioner is not positive definite (r.M^-1 r = %g) at or before iteration 0", h.ry);
    double phibar = h.phibar;
    int    k = 0, rc = SPMV_OK;
    if (phibar > limit && phibar > floor_phi && max_iter > 0)
    {
        SPMV_TRY(write_scalars(ctx, &s->floor, &floor_phi, sizeof(double), who, "writing the noise floor"));
        hipLaunchKernelGGL(minres_first_kernel, dim3(grid), dim3(kBlock), 0, st, n, (const double*)y, v, (const MinresScalars*)s);
        // the four launches of an iteration (a preconditioner applied by launches: and its application with the dot behind it; in a
        // quiet iteration the product and the application run on what stands, which no kernel then reads)
        auto iteration = [&]() -> int {
            SPMV_TRY(mat_apply_ex(ctx, A, v, q, over));
            hipLaunchKernelGGL(minres_lanczos_kernel, dim3(grid), dim3(kBlock), 0, st, n, shift, (const double*)v, (const double*)r1, q, part, s);
            if (jacobi)
                hipLaunchKernelGGL((minres_resid_kernel<true, true>), dim3(grid), dim3(kBlock), 0, st, n, (const double*)r2, (const double*)dinv, q, y, part, s);
            else if (by_launches)
            {
                hipLaunchKernelGGL((minres_resid_kernel<false, false>), dim3(grid), dim3(kBlock), 0, st, n, (const double*)r2, (const double*)dinv, q, y, part, s);
                SPMV_TRY(apply_preconditioner(ctx, P, precond, q, y));
                dot(q, y, kDotRotate);
            }
            else
                hipLaunchKernelGGL((minres_resid_kernel<false, true>), dim3(grid), dim3(kBlock), 0, st, n, (const double*)r2, (const double*)dinv, q, y, part, s);
            const double* ynew = (jacobi || by_launches) ? y : q;
            if (wide_x)
                hipLaunchKernelGGL(minres_update_kernel<true>, dim3(grid), dim3(kBlock), 0, st, n, ynew, (const double*)w, w2, v, x, (const MinresScalars*)s);
            else
                hipLaunchKernelGGL(minres_update_kernel<false>, dim3(grid), dim3(kBlock), 0, st, n, ynew, (const double*)w, w2, v, x, (const MinresScalars*)s);
            // by pointer: r1 = r2, r2 = q, the old r1 takes the next product;  w2 = w, w = what was written over the old w2
            double* const free_now = r1;
            r1 = r2, r2 = q, q = free_now;
            std::swap(w, w2);
            return SPMV_OK;
        };
        const int every = std::max(1, check_every);
        while (k < max_iter)
        {
            if ((rc = iteration()) != SPMV_OK) break;
            ++k;
            if (k % every != 0 && k != max_iter) continue;
            if ((rc = fetch()) != SPMV_OK) break;
            if (h.status != 0)
            {
                if (h.status == kMinresNotSpd)
                    set_error("spmv_minres: preconditioner is not positive definite (r.M^-1 r = %g) at or before iteration %d", h.ry, k);
                else
                    set_error("spmv_minres: %s is not finite at or before iteration %d (non-finite numbers in the matrix or the preconditioner, or overflow)",
                              h.status == kMinresAlfa ? "alfa = v.y" : h.status == kMinresBeta ? "beta = sqrt(r.M^-1 r)" : "phibar", k);
                rc = SPMV_ERR_INVALID;
                break;
            }
            phibar = h.phibar;
            if (phibar <= limit || phibar <= floor_phi) break;  // (at or below the floor every later iteration would pass quietly)
        }
        if (rc == SPMV_OK) rc = hip_step(hipGetLastError(), who, "a launch of the iteration");
        k = h.it;
    }
    *iters     = k;
    *rel_resid = phibar / beta_b;
    return rc;  // (the workspace waits for the stream and frees)
}
}  // namespace spmv
