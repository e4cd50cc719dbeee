// precond.hip — the preconditioners' table (precond.hpp), the solvers' rows of refusals, and the pieces the units' handle checks are
// built from.  Host code only: the device pass sees an empty file (it would otherwise emit the table, a constant, for the device
// too, with its pointers to host functions).
#include "precond.hpp"

#ifndef __HIP_DEVICE_COMPILE__
namespace spmv
{
namespace
{
// before a solve's first launch.  Symmetric Gauss-Seidel and ILU(0) are built once per handle and order; a Chebyshev, AMG or FSAI
// handle that was set up explicitly is used as it stands, and else set up with the defaults
int symgs_ensure(spmv_ctx*, spmv_mat* m) { return symgs_setup(m); }
int ilu0_ensure(spmv_ctx*, spmv_mat* m) { return ilu0_setup(m); }
int cheby_ensure(spmv_ctx* ctx, spmv_mat* m) { return m->cheby ? SPMV_OK : cheby_setup(ctx, m, m->cheby_degree, /*scaled=*/1, 0.0, 0.0); }
int amg_ensure(spmv_ctx* ctx, spmv_mat* m) { return m->amg ? SPMV_OK : amg_setup(ctx, m, 0, 0, 0, 0.0, 0.0); }  // 0: every default
int fsai_ensure(spmv_ctx* ctx, spmv_mat* m) { return m->fsai ? SPMV_OK : fsai_setup(ctx, m, 0); }               // 0: the handle's "fsai_level"
// one sweep on A z = r from z = 0
int symgs_apply(spmv_ctx* ctx, const spmv_mat* A, const double* r, double* z) { return symgs_sweep(ctx, A, r, z, /*zero_guess=*/true); }

constexpr unsigned bit(int id) { return 1u << id; }
}  // namespace

// Jacobi has no row of functions: its 1 / a_ii is a piece of each solve's workspace (jacobi_inverse_diagonal, solver_host.hip), and
// what it refuses depends on the solver (check_preconditioner).
// (whether a Chebyshev handle is set up, and what its own set-up needs, is looked at on the device's side)
const precond_row kPreconds[kPrecondCount] = {
    // id                    name                      by_launches  check_handle        ensure        apply        free        set_param        get_param
    {SPMV_PRECOND_NONE,      "none",                   false,       nullptr,            nullptr,      nullptr,     nullptr,    nullptr,         nullptr},
    {SPMV_PRECOND_JACOBI,    "Jacobi",                 false,       nullptr,            nullptr,      nullptr,     nullptr,    nullptr,         nullptr},
    {SPMV_PRECOND_SYMGS,     "symmetric Gauss-Seidel", false,       nullptr,            symgs_ensure, symgs_apply, symgs_free, symgs_set_param, symgs_get_param},
    {SPMV_PRECOND_ILU0,      "ILU(0)",                 true,        ilu0_check_handle,  ilu0_ensure,  ilu0_apply,  ilu0_free,  ilu0_set_param,  ilu0_get_param},
    {SPMV_PRECOND_CHEBYSHEV, "Chebyshev",              true,        cheby_check_handle, cheby_ensure, cheby_apply, cheby_free, cheby_set_param, cheby_get_param},
    {SPMV_PRECOND_AMG,       "AMG",                    true,        amg_check_handle,   amg_ensure,   amg_apply,   amg_free,   amg_set_param,   amg_get_param},
    {SPMV_PRECOND_FSAI,      "FSAI",                   true,        fsai_check_handle,  fsai_ensure,  fsai_apply,  fsai_free,  fsai_set_param,  fsai_get_param},
};

// Which solver takes which preconditioner.  A row that is not refused here is refused or taken by its own check_handle; Jacobi by
// jacobi_arrays.
constexpr unsigned kNotOnKColumns = bit(SPMV_PRECOND_SYMGS) | bit(SPMV_PRECOND_ILU0) | bit(SPMV_PRECOND_CHEBYSHEV) | bit(SPMV_PRECOND_AMG) | bit(SPMV_PRECOND_FSAI);
//                                    who              matrix                alias_only  refused                  not_built_for  jacobi_arrays
const solver_rules kCgRules       = {"spmv_cg",       "the matrix",         true,       0,                       nullptr,       solver_rules::jacobi_arrays_unsupported};
const solver_rules kCgMultiRules  = {"spmv_cg_multi", "the matrix",         false,      kNotOnKColumns,          "k columns",   solver_rules::jacobi_arrays_elsewhere};
const solver_rules kBicgstabRules = {"spmv_bicgstab", "the matrix (shard)", false,      bit(SPMV_PRECOND_SYMGS), "this solver", solver_rules::jacobi_arrays_invalid};
const solver_rules kGmresRules    = {"spmv_gmres",    "the matrix (shard)", false,      bit(SPMV_PRECOND_SYMGS), "this solver", solver_rules::jacobi_arrays_invalid};
const solver_rules kLobpcgRules   = {"spmv_lobpcg",   "the matrix (shard)", false,      bit(SPMV_PRECOND_SYMGS), "this solver", solver_rules::jacobi_arrays_invalid};
// (spmv_minres needs a symmetric positive definite M: the sweep and the incomplete factors are neither symmetric nor sure to be definite)
const solver_rules kMinresRules   = {"spmv_minres",   "the matrix (shard)", false,      bit(SPMV_PRECOND_SYMGS) | bit(SPMV_PRECOND_ILU0), "this solver", solver_rules::jacobi_arrays_invalid};

// ---- the pieces of the units' handle checks (on the host; `noun` is the unit's name in its messages) -----------------------------
int check_whole_square(const spmv_mat* m, const char* who, const char* noun)
{
    SPMV_REQUIRE(m->nrow == m->ncol && m->row_begin == 0, "%s: %s needs the whole square matrix (%d x %d, first row %lld)", who, noun, m->nrow, m->ncol,
                 (long long)m->row_begin);
    return SPMV_OK;
}

int check_csr_arrays(const spmv_mat* m, const char* who, const char* what_for)
{
    SPMV_REQUIRE(m->nnz == 0 || (m->b && m->v), "%s: the CSR arrays are gone (panel_keep_csr = 0 released them)%s", who, what_for);
    return SPMV_OK;
}

int check_whole_square_csr(const spmv_mat* m, const char* who, const char* noun)
{
    if (m->format != SPMV_FMT_CSR) SPMV_FAIL(SPMV_ERR_UNSUPPORTED, "%s: %s needs a CSR handle (format %d)", who, noun, m->format);
    SPMV_TRY(check_whole_square(m, who, noun));
    return check_csr_arrays(m, who, "");
}
}  // namespace spmv
#endif
