// solver_cgls.hip — spmv_cgls: least squares min ||b - A x||^2 + damp^2 ||x||^2 by CGLS, device-resident, on CDNA4 (gfx950).
//
// A is any handle the forward product (mat_apply_ex) and the transposed product (transpose_apply) both take: every format, any
// shape; a shard is the rectangular matrix it holds.  Neither product is changed and neither gets a kernel here.  The recurrence,
// exactly as it runs (b, r, q have nrow entries; x, p, s have ncol):
//
//   r = b - A x;  s = A^T r - damp^2 x;  p = s;  gamma = s.s
//   loop:
//     q = A p;  delta = q.q + damp^2 p.p;  alpha = gamma / delta
//     x += alpha p;  r -= alpha q
//     s = A^T r - damp^2 x
//     gamma' = s.s;  beta = gamma' / gamma;  p = s + beta p;  gamma = gamma'
//
// Six launches per iteration, with and without damping:
//   1  mat_apply_ex             q = A p (overwrite)
//   2  cgls_dot_kernel          q.q
//   3  cgls_update_kernel       alpha = gamma / (q.q + damp^2 p.p);  x += alpha p;  r -= alpha q;  s = -damp^2 x_new (0 without
//                               damping);  r.r
//   4  transpose_apply          s += A^T r: it accumulates, which is why launch 3 leaves -damp^2 x in s (no memset per iteration)
//   5  cgls_dot_kernel          gamma' = s.s
//   6  cgls_direction_kernel    beta = gamma' / gamma;  p = s + beta p;  gamma = gamma';  p.p for the next delta (damp > 0 only)
// The set-up is the same kernels: s = A^T b and its dot give ||A^T b||^2 (the reference of the stopping rule, independent of x0);
// q = A x0 and cgls_init_kernel give r, b.b and r.r; then launches 3 to 6 run on zeroed scalars, where gamma = 0 makes launch 3
// leave x and r alone and write s = -damp^2 x0, and beta = 0 makes launch 6 copy p = s.
//
// alpha, beta, gamma, delta are formed on the device from scalars that never leave it (CglsScalars); the host reads gamma, r.r and
// the status word every check_every iterations and after the last one.  An iteration whose gamma is at or below 1e-28 ||A^T b||^2
// (rounding noise of the recurrence; 0 ends the solve) passes quietly: x and r stay, s is formed again from them, p restarts at s.
// delta <= 0 (or NaN) with gamma above that floor, or a NaN gamma, raises the status word and leaves x and r alone.
//
// Every dot product is DETERMINISTIC, by the last-ticket pattern of solver_common.hpp (grid_totals): a workgroup sums its lanes in
// a fixed order (xor butterfly inside a wavefront, then the four wavefronts in order) and stores the result in a [workgroups]
// buffer; the workgroup that takes the last ticket of the launch adds the buffer up in buffer order and writes the scalar the next
// launch reads.  No atomic adds in arrival order: a solve is exactly as reproducible as the two products its handle runs.
//
// Vector kernels: kBlock threads, grid-stride loops, 64-bit indices.  r, q, p, s are fresh 256-byte aligned allocations and go in
// 16-byte accesses (two elements per lane, an odd last element by one extra lane); the caller's x (update) and b (init) go in
// 16-byte accesses where they are 16-byte aligned and have two entries or more, in 8-byte accesses otherwise.
//
// Not part of the reference's API, so there is no reference output.  What pins it: every iterate x_k and both residuals against
// CGLS in extended precision (tests/cgls_ref.py, tests/test_gpu_cgls.py).
#include <cmath>

#include "common.hpp"
#include "solver_common.hpp"
#include "solver_host.hpp"
#include "wave.hpp"

namespace spmv
{
namespace
{
struct CglsScalars
{
    double   gamma;        // s.s of the current s (0 until the set-up's direction launch)
    double   gamma_new;    // s.s behind the transposed product, until the direction launch moves it into gamma
    double   qq;           // q.q
    double   pp;           // p.p (damp > 0 only)
    double   rr;           // r.r: what the host looks at, with gamma
    double   bb;           // b.b
    double   atb2;         // ||A^T b||^2
    double   floor_gamma;  // 1e-28 ||A^T b||^2, written by the host once it is known: at or below it gamma is rounding noise
    int32_t  status;       // 1: delta <= 0 (or NaN) with gamma above the floor, 2: gamma is NaN
    uint32_t ticket;       // workgroups of the current launch that have stored their partial sums
};

// r = b - q (q = A x0), b.b, r.r.  WIDE: b is 16-byte aligned (q and r always are)
template <bool WIDE>
__global__ __launch_bounds__(kBlock) void cgls_init_kernel(int64_t n, const double* __restrict__ b, const double* __restrict__ q,
                                                           double* __restrict__ r, double* __restrict__ part, CglsScalars* __restrict__ s)
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
            ((f64x2*)r)[i] = rv;
        }
        if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0)
        {
            const double bi = b[n - 1], ri = bi - q[n - 1];
            r[n - 1]        = ri;
            acc[0]          = fma(bi, bi, acc[0]);
            acc[1]          = fma(ri, ri, acc[1]);
        }
    }
    else
        for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock)
        {
            const double bi = b[i], ri = bi - q[i];
            r[i]            = ri;
            acc[0]          = fma(bi, bi, acc[0]);
            acc[1]          = fma(ri, ri, acc[1]);
        }
    double total[2];
    if (!grid_totals<2>(acc, part, &s->ticket, total)) return;
    if (threadIdx.x == 0)
    {
        s->bb     = total[0];
        s->rr     = total[1];
        s->ticket = 0;
    }
}

// *out = v.v of a complete work vector (s or q: fresh allocations, 16-byte accesses)
__global__ __launch_bounds__(kBlock) void cgls_dot_kernel(int64_t n, const double* __restrict__ v, double* __restrict__ out,
                                                          double* __restrict__ part, CglsScalars* __restrict__ s)
{
    double        acc[1] = {0.0};
    const int64_t npairs = n / 2;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < npairs; i += (int64_t)gridDim.x * kBlock)
    {
        const f64x2 t = ((const f64x2*)v)[i];
        acc[0]        = fma(t[0], t[0], acc[0]);
        acc[0]        = fma(t[1], t[1], acc[0]);
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) acc[0] = fma(v[n - 1], v[n - 1], acc[0]);
    double total[1];
    if (!grid_totals<1>(acc, part, &s->ticket, total)) return;
    if (threadIdx.x == 0)
    {
        *out      = total[0];
        s->ticket = 0;
    }
}

// alpha = gamma / (q.q + damp^2 p.p);  x += alpha p;  r -= alpha q;  s = -damp^2 x_new;  r.r.  Without a step to take (gamma at
// or below the floor, or no alpha to be had) x and r stay and s and r.r are formed from them as they are.
// WIDE: x is 16-byte aligned (p, s, q, r always are).  nc: entries of x, p, s;  nr: entries of r, q
template <bool WIDE, bool DAMP>
__global__ __launch_bounds__(kBlock) void cgls_update_kernel(int64_t nc, int64_t nr, double damp2, const double* __restrict__ p,
                                                             const double* __restrict__ q, double* __restrict__ x,
                                                             double* __restrict__ r, double* __restrict__ sv, double* __restrict__ part,
                                                             CglsScalars* __restrict__ s)
{
    // (uniform over the grid: every thread reads the same scalars, and nobody writes them before the last ticket is taken)
    const double gamma = s->gamma;
    double       alpha = 0.0;
    bool         live  = false;
    if (gamma != gamma)
    {
        if (blockIdx.x == 0 && threadIdx.x == 0) s->status = 2;  // b, x0 or the matrix hold non-finite numbers
    }
    else if (gamma > s->floor_gamma)
    {
        const double delta = DAMP ? s->qq + damp2 * s->pp : s->qq;
        if (!(delta > 0.0))
        {
            if (blockIdx.x == 0 && threadIdx.x == 0) s->status = 1;  // a gradient to speak of and no step along it
        }
        else
        {
            alpha = gamma / delta;
            live  = true;
        }
    }
    const int64_t stride = (int64_t)gridDim.x * kBlock, first = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if constexpr (WIDE)
    {
        const int64_t npairs = nc / 2;
        for (int64_t i = first; i < npairs; i += stride)
        {
            f64x2 xv = ((f64x2*)x)[i];
            if (live)
            {
                const f64x2 pv = ((const f64x2*)p)[i];
                xv[0]          = fma(alpha, pv[0], xv[0]);
                xv[1]          = fma(alpha, pv[1], xv[1]);
                ((f64x2*)x)[i] = xv;
            }
            ((f64x2*)sv)[i] = DAMP ? f64x2{-damp2 * xv[0], -damp2 * xv[1]} : f64x2{0.0, 0.0};
        }
        if ((nc & 1) && blockIdx.x == 0 && threadIdx.x == 0)
        {
            const int64_t i  = nc - 1;
            double        xi = x[i];
            if (live) x[i] = xi = fma(alpha, p[i], xi);
            sv[i] = DAMP ? -damp2 * xi : 0.0;
        }
    }
    else
        for (int64_t i = first; i < nc; i += stride)
        {
            double xi = x[i];
            if (live) x[i] = xi = fma(alpha, p[i], xi);
            sv[i] = DAMP ? -damp2 * xi : 0.0;
        }
    double        acc[1] = {0.0};
    const int64_t rpairs = nr / 2;
    for (int64_t i = first; i < rpairs; i += stride)
    {
        f64x2 rv = ((f64x2*)r)[i];
        if (live)
        {
            const f64x2 qv = ((const f64x2*)q)[i];
            rv[0]          = fma(-alpha, qv[0], rv[0]);
            rv[1]          = fma(-alpha, qv[1], rv[1]);
            ((f64x2*)r)[i] = rv;
        }
        acc[0] = fma(rv[0], rv[0], acc[0]);
        acc[0] = fma(rv[1], rv[1], acc[0]);
    }
    if ((nr & 1) && blockIdx.x == 0 && threadIdx.x == 0)
    {
        const int64_t i  = nr - 1;
        double        ri = r[i];
        if (live) r[i] = ri = fma(-alpha, q[i], ri);
        acc[0] = fma(ri, ri, acc[0]);
    }
    double total[1];
    if (!grid_totals<1>(acc, part, &s->ticket, total)) return;
    if (threadIdx.x == 0)
    {
        s->rr     = total[0];
        s->ticket = 0;
    }
}

// beta = gamma' / gamma;  p = s + beta p;  gamma = gamma';  p.p (DAMP).  Where the update took no step (gamma at or below the
// floor; at the set-up gamma = 0) beta = 0 and p restarts at s without being read.
template <bool DAMP>
__global__ __launch_bounds__(kBlock) void cgls_direction_kernel(int64_t n, const double* __restrict__ sv, double* __restrict__ p,
                                                                double* __restrict__ part, CglsScalars* __restrict__ s)
{
    const double gamma = s->gamma, gamma_new = s->gamma_new;
    if (gamma_new != gamma_new && blockIdx.x == 0 && threadIdx.x == 0) s->status = 2;
    const bool    live   = gamma > s->floor_gamma && gamma_new == gamma_new;
    const double  beta   = live ? gamma_new / gamma : 0.0;
    double        acc[1] = {0.0};
    const int64_t npairs = n / 2;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < npairs; i += (int64_t)gridDim.x * kBlock)
    {
        f64x2 pv = ((const f64x2*)sv)[i];
        if (live)
        {
            const f64x2 old = ((const f64x2*)p)[i];
            pv[0]           = fma(beta, old[0], pv[0]);
            pv[1]           = fma(beta, old[1], pv[1]);
        }
        ((f64x2*)p)[i] = pv;
        if (DAMP)
        {
            acc[0] = fma(pv[0], pv[0], acc[0]);
            acc[0] = fma(pv[1], pv[1], acc[0]);
        }
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0)
    {
        const int64_t i  = n - 1;
        double        pi = sv[i];
        if (live) pi = fma(beta, p[i], pi);
        p[i] = pi;
        if (DAMP) acc[0] = fma(pi, pi, acc[0]);
    }
    if constexpr (DAMP)
    {
        double total[1];
        if (!grid_totals<1>(acc, part, &s->ticket, total)) return;
        if (threadIdx.x == 0)
        {
            s->pp     = total[0];
            s->gamma  = gamma_new;
            s->ticket = 0;
        }
    }
    else
    {
        // no sum to wait for, but gamma may move only once every workgroup has read it: the last ticket again
        if (!took_last_ticket(&s->ticket)) return;
        if (threadIdx.x == 0)
        {
            s->gamma  = gamma_new;
            s->ticket = 0;
        }
    }
}
}  // namespace

int cgls_solve(spmv_ctx* ctx, const spmv_mat* A, const double* b, double* x, int max_iter, double rel_tol, int check_every,
               double damp, int* iters, double* rel_normal_resid, double* rel_resid)
{
    const char* const who = "spmv_cgls";
    const int64_t     nr = A->nrow, nc = A->ncol;
    *iters            = 0;
    *rel_normal_resid = 0.0;
    *rel_resid        = 0.0;
    if (nr == 0 || nc == 0) return SPMV_OK;
    SPMV_TRY(transpose_setup(const_cast<spmv_mat*>(A)));  // (once; the transposed state is no part of the forward one)
    hipStream_t st = ctx->stream;
    // r, q (nrow), p, s (ncol) and the partial sums of two quantities
    double *       r, *q, *p, *sv, *part;
    CglsScalars*   s = nullptr;
    SolveWorkspace ws(ctx, who);
    ws.piece(r, nr);
    ws.piece(q, nr);
    ws.piece(p, nc);
    ws.piece(sv, nc);
    ws.piece(part, 2 * (size_t)kMaxGrid);
    SPMV_TRY(ws.allocate((void**)&s, sizeof(CglsScalars)));
    const bool   wide_x = wide_ok(x, nc), wide_b = wide_ok(b, nr);
    const bool   damped = damp > 0.0;
    const double damp2  = damp * damp;
    const int    grid_r = pair_grid(nr), grid_c = pair_grid(nc);
    const int    grid_u = wide_x ? std::max(grid_r, grid_c) : std::max(grid_r, stream_grid(nc));
    apply_extra  over;
    over.overwrite = true;
    auto dot = [&](int64_t n, const double* v, double* out) {
        hipLaunchKernelGGL(cgls_dot_kernel, dim3(n == nr ? grid_r : grid_c), dim3(kBlock), 0, st, n, v, out, part, s);
    };
    // launches 3 to 6 of an iteration: the update, s += A^T r, gamma' = s.s, the direction
    auto behind_the_product = [&]() -> int {
#define SPMV_CGLS_UPDATE(WIDE, DAMP) \
    hipLaunchKernelGGL((cgls_update_kernel<WIDE, DAMP>), dim3(grid_u), dim3(kBlock), 0, st, nc, nr, damp2, p, q, x, r, sv, part, s)
        if (wide_x)
        {
            if (damped) SPMV_CGLS_UPDATE(true, true); else SPMV_CGLS_UPDATE(true, false);
        }
        else
        {
            if (damped) SPMV_CGLS_UPDATE(false, true); else SPMV_CGLS_UPDATE(false, false);
        }
#undef SPMV_CGLS_UPDATE
        SPMV_TRY(transpose_apply(ctx, A, r, sv));
        dot(nc, sv, &s->gamma_new);
        if (damped)
            hipLaunchKernelGGL(cgls_direction_kernel<true>, dim3(grid_c), dim3(kBlock), 0, st, nc, sv, p, part, s);
        else
            hipLaunchKernelGGL(cgls_direction_kernel<false>, dim3(grid_c), dim3(kBlock), 0, st, nc, sv, p, part, s);
        return SPMV_OK;
    };
    CglsScalars h;
    auto        fetch = [&]() { return read_scalars(ctx, &h, s, sizeof(CglsScalars), who); };
    SPMV_TRY(hip_step(hipMemsetAsync(sv, 0, sizeof(double) * (size_t)nc, st), who, "clearing s"));
    SPMV_TRY(transpose_apply(ctx, A, b, sv));  // s = A^T b
    dot(nc, sv, &s->atb2);
    SPMV_TRY(mat_apply_ex(ctx, A, x, q, over));  // q = A x0
    if (wide_b)
        hipLaunchKernelGGL(cgls_init_kernel<true>, dim3(grid_r), dim3(kBlock), 0, st, nr, b, (const double*)q, r, part, s);
    else
        hipLaunchKernelGGL(cgls_init_kernel<false>, dim3(stream_grid(nr)), dim3(kBlock), 0, st, nr, b, (const double*)q, r, part, s);
    SPMV_TRY(behind_the_product());  // gamma = 0: s = A^T r0 - damp^2 x0, p = s, x and r as they are
    SPMV_TRY(fetch());
    const double bb = h.bb, atb2 = h.atb2;
    double       gamma = h.gamma, rr = h.rr;
    if (!std::isfinite(bb) || !std::isfinite(atb2) || !std::isfinite(gamma) || !std::isfinite(rr))
        SPMV_FAIL(SPMV_ERR_INVALID, "spmv_cgls: b.b = %g, ||A^T b||^2 = %g, gamma_0 = %g, r0.r0 = %g: b, x0 or the matrix hold non-finite numbers", bb,
                  atb2, gamma, rr);
    if (!(atb2 > 0.0)) return SPMV_OK;  // A^T b = 0 (b = 0 among it): x0 stays, as spmv_cg leaves it at b.b = 0
    const double limit = rel_tol * rel_tol * atb2;  // squared norms are compared
    int          k = 0, rc = SPMV_OK;
    if (gamma > limit && gamma > 0.0 && max_iter > 0)
    {
        const double floor_gamma = 1e-28 * atb2;
        SPMV_TRY(write_scalars(ctx, &s->floor_gamma, &floor_gamma, sizeof(double), who, "writing the noise floor"));
        const int every = std::max(1, check_every);
        while (k < max_iter)
        {
            if ((rc = mat_apply_ex(ctx, A, p, q, over)) != SPMV_OK) break;  // q = A p
            dot(nr, q, &s->qq);
            if ((rc = behind_the_product()) != SPMV_OK) break;
            ++k;
            if (k % every != 0 && k != max_iter) continue;
            if ((rc = fetch()) != SPMV_OK) break;
            gamma = h.gamma;
            rr    = h.rr;
            // the status word is set only with a gradient above the floor; it is looked at first
            if (h.status == 2 || !std::isfinite(gamma))
            {
                set_error("spmv_cgls: gamma = s.s is not finite at or before iteration %d (non-finite numbers in b, x0 or the matrix, or overflow)", k);
                rc = SPMV_ERR_INVALID;
                break;
            }
            if (h.status != 0)
            {
                set_error("spmv_cgls: delta = q.q + damp^2 p.p <= 0 (or not finite) at or before iteration %d with a gradient to speak of", k);
                rc = SPMV_ERR_INVALID;
                break;
            }
            if (!std::isfinite(rr))
            {
                set_error("spmv_cgls: r.r is not finite at or before iteration %d (overflow)", k);
                rc = SPMV_ERR_INVALID;
                break;
            }
            if (gamma <= limit || gamma == 0.0) break;
        }
        if (rc == SPMV_OK) rc = hip_step(hipGetLastError(), who, "a launch of the iteration");
    }
    *iters            = k;
    *rel_normal_resid = sqrt(gamma / atb2);
    *rel_resid        = sqrt(rr / bb);
    return rc;  // (the workspace waits for the stream and frees)
}
}  // namespace spmv
