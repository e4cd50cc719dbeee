// solver_host.hip — the host side that the solves share (solver_host.hpp): argument checks, the workspace, the preconditioner's
// set-up and application through its row of the table (precond.hpp).  One kernel: the inverse diagonal of a CSR handle, for Jacobi
// and for Chebyshev's scaling.
#include "solver_host.hpp"

namespace spmv
{
namespace
{
// 1 / a_ii of a CSR handle (duplicates of the diagonal entry are summed, as the product would); flag != 0: a zero or
// missing diagonal entry
__global__ __launch_bounds__(kBlock) void csr_inv_diag_kernel(int nrow, int64_t row_begin, const int32_t* __restrict__ row_ptr,
                                                              const int32_t* __restrict__ col, const double* __restrict__ val,
                                                              double* __restrict__ dinv, int* __restrict__ flag)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= nrow) return;
    double    d   = 0.0;
    const int end = row_ptr[i + 1];
    for (int j = row_ptr[i]; j < end; ++j)
        if ((int64_t)col[j] == row_begin + i) d += val[j];
    if (d == 0.0)
    {
        atomicOr(flag, 1);
        d = 1.0;
    }
    dinv[i] = 1.0 / d;
}

}  // namespace

// dinv[i] = 1 / a_ii; the flag is the first word of the context's scratch
int jacobi_inverse_diagonal(spmv_ctx* ctx, const spmv_mat* A, double* dinv, const char* who, const char* what)
{
    SPMV_TRY(ensure_scratch(ctx, 64));
    int* flag   = (int*)ctx->scratch;
    int  h_flag = 0;
    (void)hipMemsetAsync(flag, 0, sizeof(int), ctx->stream);
    hipLaunchKernelGGL(csr_inv_diag_kernel, dim3((unsigned)ceil_div(A->nrow, kBlock)), dim3(kBlock), 0, ctx->stream, (int)A->nrow,
                       A->row_begin, A->a, A->b, A->v, dinv, flag);
    SPMV_HIP(hipGetLastError());
    if (hipMemcpyAsync(&h_flag, flag, sizeof(int), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
        hipStreamSynchronize(ctx->stream) != hipSuccess || h_flag != 0)
        SPMV_FAIL(SPMV_ERR_INVALID, "%s: the matrix has a zero or missing diagonal entry (%s)", who, what);
    return SPMV_OK;
}

// ---- argument checks -----------------------------------------------------------------------------------------------------------
bool vectors_disjoint(const spmv_vec* b, const spmv_vec* x)
{
    return b->n == 0 || x->n == 0 || b->d + b->n <= x->d || x->d + x->n <= b->d;
}

int check_limits(const char* who, int max_iter, double rel_tol)
{
    SPMV_REQUIRE(max_iter >= 0 && rel_tol >= 0.0, "%s: max_iter=%d rel_tol=%g", who, max_iter, rel_tol);
    return SPMV_OK;
}

int check_vector_lengths(const char* who, const spmv_mat* A, const char* name_b, const spmv_vec* b, const char* name_x, const spmv_vec* x)
{
    SPMV_REQUIRE(b->n == A->nrow && x->n == A->nrow, "%s: %s has %lld and %s %lld entries, the matrix %d rows", who, name_b, (long long)b->n, name_x,
                 (long long)x->n, A->nrow);
    return SPMV_OK;
}

int check_vector_pair(const char* who, const spmv_mat* A, const char* name_b, const spmv_vec* b, const char* name_x, const spmv_vec* x)
{
    SPMV_TRY(check_vector_lengths(who, A, name_b, b, name_x, x));
    SPMV_REQUIRE(vectors_disjoint(b, x), "%s: %s and %s must not overlap", who, name_b, name_x);
    return SPMV_OK;
}

int check_known_preconditioner(const char* who, int precond)
{
    SPMV_REQUIRE(precond_row_of(precond), "%s: unknown preconditioner %d", who, precond);
    return SPMV_OK;
}

int check_square_solve(const solver_rules& S, const spmv_ctx* ctx, const spmv_mat* A, const spmv_vec* b, const spmv_vec* x, int max_iter,
                       double rel_tol, int precond, const int32_t* iters, const double* rel_resid)
{
    SPMV_REQUIRE(ctx && A && b && x && iters && rel_resid, "%s: null argument", S.who);
    SPMV_REQUIRE(A->nrow == A->ncol, "%s: %s is %d x %d, not square", S.who, S.matrix, A->nrow, A->ncol);
    if (S.alias_only)
    {
        SPMV_TRY(check_vector_lengths(S.who, A, "b", b, "x", x));
        SPMV_REQUIRE(b->d != x->d || x->n == 0, "%s: b and x must not alias", S.who);
    }
    else
        SPMV_TRY(check_vector_pair(S.who, A, "b", b, "x", x));
    SPMV_TRY(check_limits(S.who, max_iter, rel_tol));
    return check_known_preconditioner(S.who, precond);
}

int check_shift_and_precond_handle(const solver_rules& S, const spmv_ctx* ctx, const spmv_mat* A, const spmv_mat* P, double shift, int precond)
{
    SPMV_REQUIRE(std::isfinite(shift), "%s: shift=%g, must be finite", S.who, shift);
    if (!P) return SPMV_OK;
    SPMV_REQUIRE(precond != SPMV_PRECOND_NONE, "%s: a preconditioner's handle P was given with SPMV_PRECOND_NONE: name the preconditioner, or pass P = NULL", S.who);
    SPMV_REQUIRE(P->nrow == A->nrow && P->ncol == A->nrow, "%s: P is %d x %d, A is %d x %d: the preconditioner's handle must be square and of A's size", S.who,
                 P->nrow, P->ncol, A->nrow, A->ncol);
    SPMV_REQUIRE(P->ctx == ctx, "%s: P belongs to another context", S.who);
    return SPMV_OK;
}

int check_refine(const spmv_ctx* ctx, const spmv_mat* A, const spmv_mat* A_lo, const spmv_vec* b, const spmv_vec* x, int solver, int precond,
                 int max_outer, int inner_max_iter, double inner_tol, double rel_tol, const int32_t* outer, const int32_t* inner_total,
                 const double* rel_resid)
{
    const char* const who = "spmv_refine";
    SPMV_REQUIRE(ctx && A && A_lo && b && x && outer && inner_total && rel_resid, "%s: null argument", who);
    SPMV_REQUIRE(A->nrow == A->ncol, "%s: the matrix is %d x %d, not square", who, A->nrow, A->ncol);
    SPMV_REQUIRE(A_lo->nrow == A->nrow && A_lo->ncol == A->ncol, "%s: A_lo is %d x %d, A is %d x %d: the shapes must match", who, A_lo->nrow, A_lo->ncol, A->nrow,
                 A->ncol);
    SPMV_REQUIRE(A->ctx == ctx && A_lo->ctx == ctx, "%s: %s belongs to another context", who, A->ctx != ctx ? "A" : "A_lo");
    SPMV_TRY(check_vector_pair(who, A, "b", b, "x", x));
    SPMV_REQUIRE(max_outer >= 0 && inner_max_iter >= 0 && inner_tol >= 0.0 && rel_tol >= 0.0, "%s: max_outer=%d inner_max_iter=%d inner_tol=%g rel_tol=%g", who,
                 max_outer, inner_max_iter, inner_tol, rel_tol);
    SPMV_REQUIRE(solver == SPMV_REFINE_CG || solver == SPMV_REFINE_BICGSTAB, "%s: unknown solver %d (0: CG, 1: BiCGSTAB)", who, solver);
    return check_known_preconditioner(who, precond);
}

int check_preconditioner(const solver_rules& S, const spmv_mat* A, int precond)
{
    SPMV_TRY(check_known_preconditioner(S.who, precond));
    const precond_row& P = kPreconds[precond];
    if (S.refused & (1u << precond)) SPMV_FAIL(SPMV_ERR_UNSUPPORTED, "%s: the %s preconditioner is not built for %s", S.who, P.name, S.not_built_for);
    if (P.check_handle) return P.check_handle(A, S.who);
    if (precond != SPMV_PRECOND_JACOBI) return SPMV_OK;
    // Jacobi reads the diagonal from the handle's own CSR arrays (the plain solve needs the product alone and takes a handle that
    // released them)
    const bool gone = !A->b || !A->v;
    if (A->format != SPMV_FMT_CSR || (S.jacobi_arrays == solver_rules::jacobi_arrays_unsupported && gone))
        SPMV_FAIL(SPMV_ERR_UNSUPPORTED, "%s: the Jacobi preconditioner reads the diagonal of a CSR handle", S.who);
    SPMV_REQUIRE(!(S.jacobi_arrays == solver_rules::jacobi_arrays_invalid && A->nnz > 0 && gone),
                 "%s: this handle gave up its CSR arrays (panel_keep_csr = 0): no diagonal for the Jacobi preconditioner", S.who);
    return SPMV_OK;
}

// ---- errors carry text ---------------------------------------------------------------------------------------------------------
int hip_step(hipError_t e, const char* who, const char* step)
{
    if (e == hipSuccess) return SPMV_OK;
    SPMV_FAIL(SPMV_ERR_HIP, "%s: %s failed: %s", who, step, hipGetErrorString(e));
}

int read_scalars(spmv_ctx* ctx, void* host, const void* dev, size_t bytes, const char* who)
{
    hipError_t e = hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    return hip_step(e, who, "reading the iteration scalars");
}

int write_scalars(spmv_ctx* ctx, void* dev, const void* host, size_t bytes, const char* who, const char* step)
{
    hipError_t e = hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    return hip_step(e, who, step);
}

// ---- the workspace -------------------------------------------------------------------------------------------------------------
void SolveWorkspace::piece(double*& p, size_t doubles)
{
    if (npieces_ < kMaxPieces)
    {
        where_[npieces_] = &p;
        at_[npieces_]    = doubles_;
    }
    ++npieces_;  // (one too many is allocate()'s error)
    doubles_ += padded(doubles);
}

int SolveWorkspace::allocate(void** scalars, size_t scalar_bytes)
{
    SPMV_REQUIRE(npieces_ <= kMaxPieces, "%s: %d pieces of work memory, the workspace holds %d", who_, npieces_, kMaxPieces);
    const size_t bytes = sizeof(double) * doubles_;
    if (hipMalloc(&slab_, bytes) != hipSuccess || hipMalloc(&scalars_, scalar_bytes) != hipSuccess)
    {
        (void)hipGetLastError();
        SPMV_FAIL(SPMV_ERR_ALLOC, "%s: out of device memory for the work vectors and scalars (%zu + %zu bytes)", who_, bytes, scalar_bytes);
    }
    for (int i = 0; i < npieces_; ++i) *where_[i] = slab_ + at_[i];
    *scalars = scalars_;
    return hip_step(hipMemsetAsync(scalars_, 0, scalar_bytes, ctx_->stream), who_, "clearing the iteration scalars");
}

SolveWorkspace::~SolveWorkspace()
{
    (void)hipStreamSynchronize(ctx_->stream);
    if (slab_) (void)hipFree(slab_);
    if (scalars_) (void)hipFree(scalars_);
}

// ---- the preconditioner --------------------------------------------------------------------------------------------------------
int setup_preconditioner(spmv_ctx* ctx, const spmv_mat* A, int precond, double* dinv, const char* who)
{
    if (precond == SPMV_PRECOND_JACOBI) return jacobi_inverse_diagonal(ctx, A, dinv, who);
    const precond_row* P = precond_row_of(precond);
    return P && P->ensure ? P->ensure(ctx, const_cast<spmv_mat*>(A)) : SPMV_OK;
}

int apply_preconditioner(spmv_ctx* ctx, const spmv_mat* A, int precond, const double* r, double* z)
{
    const precond_row* P = precond_row_of(precond);
    if (!P || !P->apply) SPMV_FAIL(SPMV_ERR_INVALID, "apply_preconditioner: preconditioner %d is not applied by launches", precond);
    return P->apply(ctx, A, r, z);
}
}  // namespace spmv
