// solver_refine.hip - iterative refinement (spmv_refine): fp64 answers from a solver that runs on a cheaper handle.
//
// A defines the system; A_lo - the intended use: the SPMV_FMT_CSR_F32 copy of A, 8 bytes per entry instead of 12 - is what the inner
// solver multiplies by.  Per outer step: r = b - A x with A's forward product (overwrite) and one vector kernel, ||r|| by the
// deterministic dot (vec_dot: per-workgroup partial sums added in a fixed order), then A_lo d = r from d = 0 by spmv_cg's or
// spmv_bicgstab's driver to inner_tol, x += d.  The error of the rounded matrix enters d alone, never r: as long as the inner solve
// reduces the error by a factor below one the outer iteration converges to the solution of the fp64 system.
//
// It stops at ||r|| <= rel_tol ||b||, after max_outer steps, or when a step did not reduce ||r|| - x then goes back to the iterate
// with the smallest residual seen, which is the previous one (the residuals decreased up to there); that costs the third vector.
// Work memory: r, d and that copy of x, nrow doubles each, in one workspace for the duration of the call; the inner solver takes
// and releases its own per step.  No kernel of its own: the products, the vector kernels and the inner solvers are the library's.
#include <cmath>

#include "common.hpp"
#include "solver_host.hpp"

namespace spmv
{
int refine_solve(spmv_ctx* ctx, const spmv_mat* A, const spmv_mat* A_lo, const double* b, double* x, int solver, int precond, int max_outer,
                 int inner_max_iter, double inner_tol, double rel_tol, int* outer, int* inner_total, double* rel_resid)
{
    const char* const who = "spmv_refine";
    const int64_t     n   = A->nrow;
    *outer                = 0;
    *inner_total          = 0;
    *rel_resid            = 0.0;
    if (n == 0) return SPMV_OK;
    double bb = 0.0;
    SPMV_TRY(vec_dot(ctx, b, b, n, &bb));
    if (!std::isfinite(bb)) SPMV_FAIL(SPMV_ERR_INVALID, "%s: b.b = %g: b holds non-finite numbers", who, bb);
    if (!(bb > 0.0)) return SPMV_OK;  // b = 0: x is untouched (spmv_cg's rule)
    double *       r = nullptr, *d = nullptr, *xbest = nullptr;
    void*          unused = nullptr;
    SolveWorkspace ws(ctx, who);
    ws.piece(r, n);
    ws.piece(d, n);
    ws.piece(xbest, n);
    SPMV_TRY(ws.allocate(&unused, 64));
    hipStream_t st   = ctx->stream;
    double      best = 0.0;
    apply_extra over;
    over.overwrite = true;
    for (int k = 0;; ++k)
    {
        SPMV_TRY(mat_apply_ex(ctx, A, x, d, over));       // d = A x
        SPMV_TRY(vec_axpby(ctx, 1.0, b, -1.0, d, r, n));  // r = b - A x
        double rr = 0.0;
        SPMV_TRY(vec_dot(ctx, r, r, n, &rr));
        if (!std::isfinite(rr)) SPMV_FAIL(SPMV_ERR_INVALID, "%s: r.r = %g at outer step %d: x, the matrix or a correction hold non-finite numbers", who, rr, k);
        const double res = std::sqrt(rr / bb);
        if (k > 0 && !(res < best))
        {
            // the step did not reduce the residual: back to the iterate before it
            SPMV_TRY(hip_step(hipMemcpyAsync(x, xbest, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, st), who, "restoring the best iterate"));
            SPMV_TRY(hip_step(hipStreamSynchronize(st), who, "restoring the best iterate"));
            *rel_resid = best;
            return SPMV_OK;
        }
        best       = res;
        *rel_resid = res;
        if (res <= rel_tol || k >= max_outer) break;
        SPMV_TRY(hip_step(hipMemcpyAsync(xbest, x, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, st), who, "keeping the iterate"));
        SPMV_TRY(vec_fill(ctx, d, n, 0.0));
        int    it        = 0;
        double inner_res = 0.0;
        // an inner solve that runs out of iterations returns SPMV_OK with what it has; a breakdown is its error and this call's
        if (solver == SPMV_REFINE_CG)
            SPMV_TRY(cg_solve(ctx, A_lo, r, d, inner_max_iter, inner_tol, 1, precond, &it, &inner_res));
        else
            SPMV_TRY(bicgstab_solve(ctx, A_lo, r, d, inner_max_iter, inner_tol, 1, precond, &it, &inner_res));
        *inner_total += it;
        SPMV_TRY(vec_axpby(ctx, 1.0, xbest, 1.0, d, x, n));  // x = (the iterate kept above) + d
        ++*outer;
    }
    SPMV_TRY(hip_step(hipStreamSynchronize(st), who, "the last step"));
    return SPMV_OK;
}
}  // namespace spmv
