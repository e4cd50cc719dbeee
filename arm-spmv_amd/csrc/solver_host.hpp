// solver_host.hpp — the host side that the solves share (spmv_cg, spmv_cg_multi, spmv_cgls, spmv_bicgstab, spmv_gmres, spmv_minres): the
// argument checks of their ABI entries, the owner of a solve's device memory, the preconditioner's set-up and application (a
// look-up in precond.hpp's table and a call), and the small questions every driver asks about a vector (may it go in 16-byte
// accesses, how many workgroups).  Defined in solver_host.hip; the device side of what the solvers share is solver_common.hpp.
#pragma once

#include "common.hpp"
#include "precond.hpp"

namespace spmv
{
// ---- argument checks: on the host, before the device is touched (abi.hip) ------------------------------------------------------
// (what a solver's refusals depend on: solver_rules, precond.hpp)
bool vectors_disjoint(const spmv_vec* b, const spmv_vec* x);  // an empty vector overlaps nothing
// two vectors of as many entries as A has rows: "<who>: <name_b> has %lld and <name_x> %lld entries, the matrix %d rows" ...
int check_vector_lengths(const char* who, const spmv_mat* A, const char* name_b, const spmv_vec* b, const char* name_x, const spmv_vec* x);
// ... whose ranges are apart: "<who>: <name_b> and <name_x> must not overlap"
int check_vector_pair(const char* who, const spmv_mat* A, const char* name_b, const spmv_vec* b, const char* name_x, const spmv_vec* x);
int  check_limits(const char* who, int max_iter, double rel_tol);
int  check_known_preconditioner(const char* who, int precond);
// the square single-vector solvers: null arguments, square, the lengths of b and x, alias / overlap, limits, a known preconditioner
int check_square_solve(const solver_rules& S, const spmv_ctx* ctx, const spmv_mat* A, const spmv_vec* b, const spmv_vec* x, int max_iter,
                       double rel_tol, int precond, const int32_t* iters, const double* rel_resid);
// beside it for spmv_minres: a finite shift, and a preconditioner's own handle P (null: A) - square, of A's size, in A's context, and
// not given where precond is SPMV_PRECOND_NONE
int check_shift_and_precond_handle(const solver_rules& S, const spmv_ctx* ctx, const spmv_mat* A, const spmv_mat* P, double shift, int precond);
// spmv_refine: null arguments, A square, A_lo of A's shape and context, the lengths of b and x, overlap, the four limits, a known inner
// solver and preconditioner
int check_refine(const spmv_ctx* ctx, const spmv_mat* A, const spmv_mat* A_lo, const spmv_vec* b, const spmv_vec* x, int solver, int precond,
                 int max_outer, int inner_max_iter, double inner_tol, double rel_tol, const int32_t* outer, const int32_t* inner_total,
                 const double* rel_resid);
// a known preconditioner that this solver does not take (S.refused), or not on this handle (the row's check_handle; Jacobi: S.jacobi_arrays)
int check_preconditioner(const solver_rules& S, const spmv_mat* A, int precond);

// ---- errors carry text ---------------------------------------------------------------------------------------------------------
// SPMV_OK, or SPMV_ERR_HIP with "<who>: <step> failed: <HIP's words>" as the last error
int hip_step(hipError_t e, const char* who, const char* step);
// the host's look at a solve's scalars on the device: copies `bytes` and waits for the stream
int read_scalars(spmv_ctx* ctx, void* host, const void* dev, size_t bytes, const char* who);
// the host's word to the device between two looks (`step` names it): copies `bytes` and waits for the stream
int write_scalars(spmv_ctx* ctx, void* dev, const void* host, size_t bytes, const char* who, const char* step);

// ---- the workspace: one owner of a solve's device memory -----------------------------------------------------------------------
// A driver names its pieces (piece), then allocate() makes one slab and the solver's scalars struct (cleared on the stream) and
// points every piece into the slab, in the order named, each on a 256-byte boundary.  However the solve returns, the destructor
// waits for the stream and frees both.  A piece that was never named stays the nullptr its pointer was.
struct SolveWorkspace
{
    SolveWorkspace(spmv_ctx* ctx, const char* who) : ctx_(ctx), who_(who) {}
    SolveWorkspace(const SolveWorkspace&)            = delete;
    SolveWorkspace& operator=(const SolveWorkspace&) = delete;
    ~SolveWorkspace();

    // doubles from one piece's start to the next one's: the stride of vectors that share a piece
    static size_t padded(size_t doubles) { return (doubles + 31) & ~(size_t)31; }
    void          piece(double*& p, size_t doubles);
    int           allocate(void** scalars, size_t scalar_bytes);

private:
    static constexpr int kMaxPieces = 12;
    spmv_ctx*   ctx_;
    const char* who_;
    double**    where_[kMaxPieces];
    size_t      at_[kMaxPieces];
    int         npieces_ = 0;
    size_t      doubles_ = 0;
    double*     slab_    = nullptr;
    void*       scalars_ = nullptr;
};

// ---- the preconditioner --------------------------------------------------------------------------------------------------------
// Before a solve's first launch: the state that stays in the handle (the row's ensure), or dinv[i] = 1 / a_ii of a CSR handle for
// Jacobi (synchronous; a zero or missing diagonal entry is `who`'s error).  SPMV_PRECOND_NONE: nothing.
int setup_preconditioner(spmv_ctx* ctx, const spmv_mat* A, int precond, double* dinv, const char* who);
// dinv[i] = 1 / a_ii of a CSR handle (duplicates summed; synchronous); a zero or missing entry: INVALID, "<who>: ... (<what>)"
int jacobi_inverse_diagonal(spmv_ctx* ctx, const spmv_mat* A, double* dinv, const char* who, const char* what = "Jacobi preconditioner");
// a preconditioner that is a launch sequence of its own (a work vector z between the product and the updates), not a diagonal: the
// table's by_launches column
inline bool applied_by_launches(int precond)
{
    const precond_row* P = precond_row_of(precond);
    return P && P->by_launches;
}
// z = M^-1 r: the row's apply (symmetric Gauss-Seidel: one sweep from z = 0).  A preconditioner without one: INVALID
int apply_preconditioner(spmv_ctx* ctx, const spmv_mat* A, int precond, const double* r, double* z);

// ---- width and grids -----------------------------------------------------------------------------------------------------------
inline bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }
// n doubles at p may go in 16-byte accesses, two elements per lane (an odd last element by one extra lane)
inline bool wide_ok(const double* p, int64_t n) { return aligned16(p) && n >= 2; }
// workgroups of a grid-stride kernel over n elements, two per lane
inline int pair_grid(int64_t n) { return stream_grid(std::max<int64_t>(1, n / 2)); }
}  // namespace spmv
