// precond.hpp — one table for the host side of the preconditioners: a row per SPMV_PRECOND_* id with its name, its check of a
// handle, its set-up before a solve, its application, its release and its parameters.  The solvers' shared host side
// (solver_host.hip) and the handle's lifetime and parameters (abi.hip) go through the rows; which solver refuses which row stands
// beside them (solver_rules).  Defined in precond.hip.  A new preconditioner is one more row, and a bit in the rules of the solvers
// that do not take it.
#pragma once

#include "common.hpp"

namespace spmv
{
struct precond_row
{
    int         id;           // SPMV_PRECOND_*: the row's index in kPreconds
    const char* name;         // as in "the %s preconditioner is not built for %s"
    bool        by_launches;  // every driver arranges for it: a launch sequence of its own with a work vector z between the product and the
                              // updates (symmetric Gauss-Seidel is applied by launches too, but only inside spmv_cg's arrangement)
    int (*check_handle)(const spmv_mat* m, const char* who);  // on the host, before the device is touched; null: nothing to refuse here
    int (*ensure)(spmv_ctx* ctx, spmv_mat* m);                // before a solve's first launch: the state in the handle; null: none
    int (*apply)(spmv_ctx* ctx, const spmv_mat* A, const double* r, double* z);  // z = M^-1 r, asynchronous; null: not applied by launches
    void (*free)(spmv_mat* m);                                                   // the state in the handle; null: none
    bool (*set_param)(spmv_mat* m, const char* name, int64_t value, int* rc);    // false: not one of mine
    bool (*get_param)(const spmv_mat* m, const char* name, int64_t* value);      // false: not one of mine
};

constexpr int            kPrecondCount = 7;
extern const precond_row kPreconds[kPrecondCount];  // in id order

inline const precond_row* precond_row_of(int id) { return id >= 0 && id < kPrecondCount ? &kPreconds[id] : nullptr; }

// What a solver's refusals depend on.  Every message starts with `who`.  The rows of the solvers stand under the table.
struct solver_rules
{
    const char* who;
    const char* matrix;         // the noun of "is %d x %d, not square": "the matrix" or "the matrix (shard)"
    bool        alias_only;     // b and x are refused where they start at the same address (spmv_cg), not where their ranges overlap
    unsigned    refused;        // bit i: "the <kPreconds[i].name> preconditioner is not built for <not_built_for>", UNSUPPORTED
    const char* not_built_for;  // the end of that refusal: "k columns", "this solver"
    enum
    {
        jacobi_arrays_elsewhere,    // the entry checks the handle's arrays itself, for its product
        jacobi_arrays_unsupported,  // arrays gone: UNSUPPORTED, as a handle that is not CSR (spmv_cg)
        jacobi_arrays_invalid       // arrays gone: INVALID, "gave up its CSR arrays"
    } jacobi_arrays;
};
extern const solver_rules kCgRules, kCgMultiRules, kBicgstabRules, kGmresRules, kLobpcgRules, kMinresRules;
}  // namespace spmv
