// amg.hip — aggregation algebraic multigrid (SPMV_PRECOND_AMG, spmv_amg_*): a deterministic device set-up and one V(1,1) cycle
// z = B r, device-resident, on CDNA4 (gfx950).  tests/amg_ref.py is the NumPy twin of every line below.
//
// The method.  Level 0 is the handle's own CSR arrays; level l + 1 is built from level l until level l is the coarsest:
// n_l <= coarse_max, or l + 1 == max_levels, or the next level would hold more than 0.8 n_l rows (5 n_c > 4 n_l: stalled).
//
// Strength.  Every row needs a stored non-zero diagonal entry (duplicates summed, as Jacobi reads it).  theta <= 0: every stored
// entry a_ij with j != i makes j a neighbour of i.  theta > 0: j != i is a neighbour iff a_ij^2 >= theta^2 |a_ii a_jj|, per
// stored entry.  The graph is what the row lists give: nothing is symmetrised.
//
// Aggregation by MIS(2).  The priority of row i is the pair (h(i), i), compared as unsigned numbers, the hash first; h is the
// 32-bit finaliser h ^= h >> 16; h *= 0x85ebca6b; h ^= h >> 13; h *= 0xc2b2ae35; h ^= h >> 16 of i.  It travels as the 64-bit key
// (h << 32 | i) + 1, so that 0 is below every priority.  All rows start undecided.  One round: t_i = the priority of an
// undecided row, 0 otherwise; twice t_i <- max(t_i, max over the neighbours j of t_j), from one buffer into another; an
// undecided row whose t is its own priority becomes a root; the flag "is a root" is spread twice the same way; an undecided
// row that the flag reaches is removed.  Rounds run until no row is undecided (the host reads one counter per round; the
// largest undecided priority always becomes a root, so the loop ends).  Roots take the aggregate ids 0, 1, .. in ascending row
// order (an exclusive scan).  Pass 1: a row that is no root and has roots among its neighbours joins the one of smallest id.
// Pass 2: every row still free joins the smallest aggregate id among its neighbours as pass 1 left them.  A removed row has a
// root within two steps of its own row lists, so pass 2 leaves no row free.  Nothing depends on the order of the launches.
//
// Coarse operator.  A_c[I, J] = sum of a_ij over ALL stored entries with agg(i) = I and agg(j) = J.  This file writes the key
// (I, J) of every entry; sorted_runs.hip does the rest: entry ids ordered stably by (I, J), runs of equal keys marked and counted,
// and one lane per coarse entry adding its run from 0.0 left to right in that order - plain additions, so the sum is defined.  The result is
// CSR with ascending columns, in a handle of its own that goes through the engine's kernel selection ("amg_level_kernel" != 0
// forces that kernel id on every coarse handle; an id that a coarse operator cannot run - the LDS-window kernel where a block's
// window is wider than its tile - fails the set-up with SPMV_ERR_UNSUPPORTED, naming the level).  Beside agg every level keeps the member lists agg_ptr / agg_rows (rows
// ascending within an aggregate: one more stable sort).
//
// Smoother.  Every level holds the Chebyshev state of chebyshev.hip with degree smooth_degree, Jacobi scaling, lmax the row
// bound and lmin = lmax / 30; level 0's is the handle's own (spmv_amg_setup replaces it, as spmv_chebyshev_setup would).
//
// Coarsest solve.  n_L <= 1024: the host downloads the operator and inverts it densely by LU with partial pivoting, in double
// (a pivot below 2^-44 of the largest entry: SPMV_ERR_INVALID, "singular coarsest operator"); the inverse goes to the device
// row-major and x_L = inverse b_L is one launch, a wavefront per row.  n_L > 1024: one Chebyshev application of that level.
//
// Cycle.  On level l with right-hand side b_l (b_0 = r, x_0 = z; r is never written):
//   x_l = M_l^-1 b_l                              cheby_apply
//   w = A_l x_l;  b_{l+1}[I] = sum over the members i of I, ascending, of (b_l[i] - w[i]), from 0.0      amg_restrict_kernel
//   x_{l+1} = cycle(l + 1)
//   x_l[i] += omega x_{l+1}[agg(i)]               amg_prolong_add_kernel
//   x_l += M_l^-1 (b_l - A_l x_l)                 cheby_smooth
// 4 d + 7 launches a level (d = smooth_degree) and 1 (dense) or 2 d + 1 (Chebyshev) at the coarsest: "amg_launches".  The state
// owns b_l, x_l (l >= 1) and w_l; an application allocates nothing and reads nothing back.  Every sum of this
// file has a fixed order; the products A_l x are as reproducible as the kernel each level runs (include/spmv_abi.h, "Order of the
// additions"): the six ids that store every y_i once - VECTOR, LDSWIN, SCALAR, ELL (a fixed order per row), PANEL and TWOPHASE (row
// sums in LDS, which the tests see return equal bits on their small hierarchies) - give equal bits from call to call on a level 0
// that runs one of them; no such promise under SEGSCAN and SPLIT (atomic adds on y in arrival order) nor under AUTO, where every
// coarse handle selects for itself - from 64K entries on by a timed trial that may choose any of the eight.
//
// Smoothed aggregation (spmv_amg_setup_smoothed; tests/amg_sa_ref.py is its twin).  Aggregates, strength mask and stop rules are
// the ones above.  On level l:
//   A^F   theta <= 0: the level's own arrays, no copy.  theta > 0: row i holds, in stored order, every stored diagonal entry and
//         every entry the mask calls a neighbour; a row with a weak off-diagonal entry ends on one more entry (i, i), the sum of its
//         weak values from 0.0 left to right (count, exclusive_scan_i32, fill: a transient CSR handle).
//   d_i   the sum of the diagonal entries of row i of A^F in stored order (amg_diag_kernel); a zero d_i: SPMV_ERR_INVALID.
//   lam   the row bound of chebyshev.hip over A^F with s_i = 1 / d_i (for theta <= 0 the lmax of the level's smoother).
//   T     n x nc, one entry 1.0 at (i, agg(i)), row_ptr iota: a transient CSR handle.
//   P     AT = spgemm(A^F, T); g = prolong_damping / lam on the host; c_i = g / d_i; P[i, J] = e - c_i AT[i, J] with e = 1.0 where
//         J = agg(i) and 0.0 elsewhere: the product rounded once, then a plain subtraction (amg_smooth_prolongator_kernel, over
//         AT's own arrays: the handle becomes P).
//   R     csr_transpose(P);  A_{l+1} = spgemm(R, spgemm(A_l, P)) with the full A_l, under "amg_level_kernel" as above.
// spgemm.hip defines every sum and the row bound is a maximum: the hierarchy is defined bit for bit.  P and R stay with the level;
// T, A^F and A P are freed before the next level is built.  The cycle differs in two launches a level, so that it keeps 4 d + 7:
//   b_{l+1}[I] = sum_k R[I, k] (b_l[i_k] - w[i_k])        amg_restrict_csr_kernel
//   x_l[i] += omega sum_J P[i, J] x_{l+1}[J]              amg_prolong_csr_kernel
// A group of g = 2^k lanes serves a row: lane t takes the entries t, t + g, .. left to right (fma), then the xor butterfly of
// wave.hpp; no atomics, every result is stored once, equal bits from call to call for a given g.  g comes per level and per
// operator from the mean row length (amg_sa_settings.hpp).
#include <cmath>
#include <memory>

#include "amg_sa_settings.hpp"
#include "common.hpp"
#include "solver_host.hpp"
#include "sorted_runs.hpp"
#include "wave.hpp"

namespace spmv
{
struct amg_level
{
    int64_t   n = 0, nnz = 0;
    spmv_mat* A = nullptr;  // level 0: the handle itself (borrowed); else an internal CSR handle, owned
    int64_t   nc = 0;       // aggregates (0 on the coarsest level)
    int32_t * agg = nullptr, *agg_ptr = nullptr, *agg_rows = nullptr;  // [n], [nc + 1], [n]; null on the coarsest level
    double *  b = nullptr, *x = nullptr, *w = nullptr;                 // into the slab; b and x null on level 0
    spmv_mat *P = nullptr, *R = nullptr;  // smoothed aggregation: n x nc and its transpose, owned; null on the coarsest level and in a plain state
    int       lanes_p = 1, lanes_r = 1;   // the lanes a row of P / R takes in the cycle (amg_sa_settings.hpp)
};

struct amg_state
{
    std::vector<amg_level> lv;
    int32_t max_levels = 0, coarse_max = 0, degree = 0;
    double  strength = 0.0, omega = 0.0;
    double* inv  = nullptr;  // the coarsest operator's inverse, row-major (null: Chebyshev serves the coarsest level)
    double* slab = nullptr;  // the levels' vectors
    int64_t bytes = 0;
    int32_t mis_rounds = 0;
    bool    smoothed = false;  // built by spmv_amg_setup_smoothed
    double  damping  = 0.0;    // its prolong_damping
};

namespace
{
constexpr int     kAmgMaxLevels = 32, kAmgDenseMax = 1024, kAmgMaxDegree = 64, kAmgMaxRounds = 4096;
constexpr int32_t kUndecided = 0, kRoot = 1, kRemoved = 2;

// ---- set-up kernels --------------------------------------------------------------------------------------------------------------
static __host__ __device__ __forceinline__ uint32_t amg_hash(uint32_t h)
{
    h ^= h >> 16;
    h *= 0x85ebca6bu;
    h ^= h >> 13;
    h *= 0xc2b2ae35u;
    h ^= h >> 16;
    return h;
}
static __device__ __forceinline__ uint64_t amg_priority(int64_t i) { return (((uint64_t)amg_hash((uint32_t)i) << 32) | (uint32_t)i) + 1; }

template <bool STRONG>
static __device__ __forceinline__ bool amg_neighbour(int64_t i, int j, double a, const double* __restrict__ diag, double theta2)
{
    if (j == i) return false;
    if constexpr (STRONG)
        return a * a >= theta2 * fabs(diag[i] * diag[j]);
    else
        return true;
}

// diag[i] = a_ii, duplicates summed; a zero or missing entry is counted
__global__ __launch_bounds__(kBlock) void amg_diag_kernel(int64_t n, const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                          const double* __restrict__ val, double* __restrict__ diag, int32_t* __restrict__ zeros)
{
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock)
    {
        double    d   = 0.0;
        const int end = row_ptr[i + 1];
        for (int e = row_ptr[i]; e < end; ++e)
            if (col[e] == i) d += val[e];
        diag[i] = d;
        if (d == 0.0) atomicAdd(zeros, 1);
    }
}

// out_i = max(v_i, max over the neighbours j of v_j), one lane per row.  What v is:
enum : int
{
    kSrcPriority = 0,  // the priority of an undecided row, 0 otherwise (from state)
    kSrcBuffer   = 1,  // in[]
    kSrcRoot     = 2   // 1 for a root - of an earlier round (state) or of this one (undecided, in[] is its own priority) - 0 otherwise
};
template <int SRC>
static __device__ __forceinline__ uint64_t amg_source(int64_t j, const int32_t* __restrict__ state, const uint64_t* __restrict__ in)
{
    if constexpr (SRC == kSrcPriority)
        return state[j] == kUndecided ? amg_priority(j) : 0;
    else if constexpr (SRC == kSrcBuffer)
        return in[j];
    else
    {
        const int32_t s = state[j];
        return (s == kRoot || (s == kUndecided && in[j] == amg_priority(j))) ? 1 : 0;
    }
}
template <int SRC, bool STRONG>
__global__ __launch_bounds__(kBlock) void amg_propagate_kernel(int64_t n, const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                               const double* __restrict__ val, const double* __restrict__ diag, double theta2,
                                                               const int32_t* __restrict__ state, const uint64_t* __restrict__ in,
                                                               uint64_t* __restrict__ out)
{
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock)
    {
        uint64_t  t   = amg_source<SRC>(i, state, in);
        const int end = row_ptr[i + 1];
        for (int e = row_ptr[i]; e < end; ++e)
        {
            const int j = col[e];
            if (amg_neighbour<STRONG>(i, j, STRONG ? val[e] : 0.0, diag, theta2)) t = max(t, amg_source<SRC>(j, state, in));
        }
        out[i] = t;
    }
}

// the end of a round: an undecided row whose t is its own priority becomes a root, one that the root flag reached is removed,
// the others are counted
__global__ __launch_bounds__(kBlock) void amg_update_kernel(int64_t n, const uint64_t* __restrict__ t, const uint64_t* __restrict__ reached,
                                                            int32_t* __restrict__ state, int32_t* __restrict__ undecided)
{
    int left = 0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock)
    {
        if (state[i] != kUndecided) continue;
        if (t[i] == amg_priority(i))
            state[i] = kRoot;
        else if (reached[i])
            state[i] = kRemoved;
        else
            ++left;
    }
    if (left) atomicAdd(undecided, left);  // (an integer sum: the order does not matter)
}

// flag[i] = 1 for a root, i < n;  flag[n] = 0: the scan of n + 1 entries ends on the number of roots
__global__ __launch_bounds__(kBlock) void amg_root_flag_kernel(int64_t n, const int32_t* __restrict__ state, int32_t* __restrict__ flag)
{
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i <= n; i += (int64_t)gridDim.x * kBlock)
        flag[i] = (i < n && state[i] == kRoot) ? 1 : 0;
}

// pass 1: a root takes its id; another row the smallest id among the roots of its neighbours, or -1
template <bool STRONG>
__global__ __launch_bounds__(kBlock) void amg_pass1_kernel(int64_t n, const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                           const double* __restrict__ val, const double* __restrict__ diag, double theta2,
                                                           const int32_t* __restrict__ state, const int32_t* __restrict__ root_id,
                                                           int32_t* __restrict__ agg)
{
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock)
    {
        int32_t best = INT32_MAX;
        if (state[i] == kRoot)
            best = root_id[i];
        else
        {
            const int end = row_ptr[i + 1];
            for (int e = row_ptr[i]; e < end; ++e)
            {
                const int j = col[e];
                if (amg_neighbour<STRONG>(i, j, STRONG ? val[e] : 0.0, diag, theta2) && state[j] == kRoot) best = min(best, root_id[j]);
            }
        }
        agg[i] = best == INT32_MAX ? -1 : best;
    }
}

// pass 2: a row still free takes the smallest aggregate id among its neighbours as pass 1 left them; a row that stays free
// (there is none: see the header) is counted
template <bool STRONG>
__global__ __launch_bounds__(kBlock) void amg_pass2_kernel(int64_t n, const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                           const double* __restrict__ val, const double* __restrict__ diag, double theta2,
                                                           const int32_t* __restrict__ agg1, int32_t* __restrict__ agg, int32_t* __restrict__ count,
                                                           int32_t* __restrict__ free_rows)
{
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock)
    {
        int32_t mine = agg1[i];
        if (mine < 0)
        {
            int32_t   best = INT32_MAX;
            const int end  = row_ptr[i + 1];
            for (int e = row_ptr[i]; e < end; ++e)
            {
                const int j = col[e];
                if (!amg_neighbour<STRONG>(i, j, STRONG ? val[e] : 0.0, diag, theta2)) continue;
                const int32_t a = agg1[j];
                if (a >= 0) best = min(best, a);
            }
            mine = best == INT32_MAX ? -1 : best;
        }
        agg[i] = mine;
        if (mine < 0)
            atomicAdd(free_rows, 1);
        else
            atomicAdd(count + mine, 1);  // members per aggregate (an integer sum)
    }
}

// the key (I, J) of every stored entry
__global__ __launch_bounds__(kBlock) void amg_key_kernel(int64_t n, const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                         const int32_t* __restrict__ agg, int32_t* __restrict__ key_i, int32_t* __restrict__ key_j)
{
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock)
    {
        const int32_t I   = agg[i];
        const int     end = row_ptr[i + 1];
        for (int e = row_ptr[i]; e < end; ++e)
        {
            key_i[e] = I;
            key_j[e] = agg[col[e]];
        }
    }
}

// ---- cycle kernels ---------------------------------------------------------------------------------------------------------------
// b_c[I] = sum over the members i of I, ascending, of (b[i] - w[i]), from 0.0: one lane per aggregate, no atomics
__global__ __launch_bounds__(kBlock) void amg_restrict_kernel(int64_t nc, const int32_t* __restrict__ agg_ptr, const int32_t* __restrict__ agg_rows,
                                                              const double* __restrict__ b, const double* __restrict__ w, double* __restrict__ b_c)
{
    for (int64_t I = (int64_t)blockIdx.x * kBlock + threadIdx.x; I < nc; I += (int64_t)gridDim.x * kBlock)
    {
        double    acc = 0.0;
        const int end = agg_ptr[I + 1];
        for (int k = agg_ptr[I]; k < end; ++k)
        {
            const int i = agg_rows[k];
            acc += b[i] - w[i];
        }
        b_c[I] = acc;
    }
}

// x[i] += omega x_c[agg[i]].  WIDE: x is 16-byte aligned (agg always is): two elements per lane, an odd last one by one lane
template <bool WIDE>
__global__ __launch_bounds__(kBlock) void amg_prolong_add_kernel(int64_t n, double omega, const int32_t* __restrict__ agg,
                                                                 const double* __restrict__ x_c, double* __restrict__ x)
{
    const int64_t stride = (int64_t)gridDim.x * kBlock, first = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if constexpr (WIDE)
    {
        const int64_t npairs = n / 2;
        for (int64_t i = first; i < npairs; i += stride)
        {
            const i32x2 a  = ((const i32x2*)agg)[i];
            const f64x2 xv = ((const f64x2*)x)[i];
            ((f64x2*)x)[i] = f64x2{fma(omega, x_c[a[0]], xv[0]), fma(omega, x_c[a[1]], xv[1])};
        }
    }
    const bool    lead = blockIdx.x == 0 && threadIdx.x == 0;
    const int64_t from = WIDE ? (((n & 1) && lead) ? n - 1 : n) : first;
    for (int64_t i = from; i < n; i += stride) x[i] = fma(omega, x_c[agg[i]], x[i]);
}

// x = inverse b: one wavefront per row of the row-major inverse, lanes stride the columns, the fixed butterfly of wave.hpp
__global__ __launch_bounds__(kBlock) void amg_dense_apply_kernel(int n, const double* __restrict__ inv, const double* __restrict__ b,
                                                                 double* __restrict__ x)
{
    const int row = blockIdx.x * (kBlock / kWave) + (threadIdx.x >> 6);
    if (row >= n) return;  // (a whole wavefront: no lane of it takes part in the butterfly)
    const double* r   = inv + (size_t)row * n;
    double        acc = 0.0;
    for (int c = threadIdx.x & 63; c < n; c += kWave) acc = fma(r[c], b[c], acc);
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) x[row] = acc;
}

// ---- smoothed aggregation: set-up kernels, one lane per row -------------------------------------------------------------------------
// count[i] = entries of row i of A^F (the diagonal entries, the neighbours, and one more where a weak entry is lumped); count[n] = 0
__global__ __launch_bounds__(kBlock) void amg_filter_count_kernel(int64_t n, const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                                  const double* __restrict__ val, const double* __restrict__ diag, double theta2,
                                                                  int32_t* __restrict__ count)
{
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i <= n; i += (int64_t)gridDim.x * kBlock)
    {
        int kept = 0, weak = 0;
        if (i < n)
        {
            const int end = row_ptr[i + 1];
            for (int e = row_ptr[i]; e < end; ++e)
            {
                const int j = col[e];
                if (j == i || amg_neighbour<true>(i, j, val[e], diag, theta2))
                    ++kept;
                else
                    weak = 1;
            }
        }
        count[i] = kept + weak;
    }
}

// row i of A^F at f_rp[i]: the kept entries in stored order, then (i, i) with the sum of the weak values from 0.0, left to right
__global__ __launch_bounds__(kBlock) void amg_filter_fill_kernel(int64_t n, const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                                 const double* __restrict__ val, const double* __restrict__ diag, double theta2,
                                                                 const int32_t* __restrict__ f_rp, int32_t* __restrict__ f_col,
                                                                 double* __restrict__ f_val)
{
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock)
    {
        int       at   = f_rp[i];
        bool      weak = false;
        double    lump = 0.0;
        const int end  = row_ptr[i + 1];
        for (int e = row_ptr[i]; e < end; ++e)
        {
            const int    j = col[e];
            const double a = val[e];
            if (j == i || amg_neighbour<true>(i, j, a, diag, theta2))
            {
                f_col[at] = j;
                f_val[at] = a;
                ++at;
            }
            else
            {
                weak = true;
                lump = __dadd_rn(lump, a);
            }
        }
        if (weak)
        {
            f_col[at] = (int32_t)i;
            f_val[at] = lump;
        }
    }
}

// T: row_ptr[i] = i (i <= n), col[i] = agg[i], val[i] = 1.0
__global__ __launch_bounds__(kBlock) void amg_tentative_kernel(int64_t n, const int32_t* __restrict__ agg, int32_t* __restrict__ t_rp,
                                                               int32_t* __restrict__ t_col, double* __restrict__ t_val)
{
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i <= n; i += (int64_t)gridDim.x * kBlock)
    {
        t_rp[i] = (int32_t)i;
        if (i < n)
        {
            t_col[i] = agg[i];
            t_val[i] = 1.0;
        }
    }
}

// P[i, J] = e - (g / d_i) AT[i, J] over AT's own values; e = 1.0 where J = agg(i), else 0.0.  One product, one subtraction: no fma
__global__ __launch_bounds__(kBlock) void amg_smooth_prolongator_kernel(int64_t n, const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                                        const int32_t* __restrict__ agg, const double* __restrict__ d, double g,
                                                                        double* __restrict__ val)
{
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock)
    {
        const double  c    = g / d[i];
        const int32_t mine = agg[i];
        const int     end  = row_ptr[i + 1];
        for (int e = row_ptr[i]; e < end; ++e) val[e] = __dsub_rn(col[e] == mine ? 1.0 : 0.0, __dmul_rn(c, val[e]));
    }
}

// ---- smoothed aggregation: the cycle's two fused kernels ---------------------------------------------------------------------------
// b_c[I] = sum_k R[I, k] (b[i_k] - w[i_k]): G lanes a row of R, lane t the entries t, t + G, .. left to right, then the fixed
// butterfly inside the group.  The loop bound is the row's, so every lane of a group runs the same trips of the outer loop and
// the butterfly never reads a lane outside its group; groups do not straddle a wavefront (G divides 64).
template <int G>
__global__ __launch_bounds__(kBlock) void amg_restrict_csr_kernel(int64_t nc, const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                                  const double* __restrict__ val, const double* __restrict__ b,
                                                                  const double* __restrict__ w, double* __restrict__ b_c)
{
    constexpr int RPB = kBlock / G;
    const int     t   = threadIdx.x % G;
    for (int64_t I = (int64_t)blockIdx.x * RPB + threadIdx.x / G; I < nc; I += (int64_t)gridDim.x * RPB)
    {
        double        acc = 0.0;
        const int64_t end = row_ptr[I + 1];
        for (int64_t k = (int64_t)row_ptr[I] + t; k < end; k += G)
        {
            const int i = col[k];
            acc         = fma(val[k], b[i] - w[i], acc);
        }
        acc = group_sum_swizzle<G>(acc);
        if (t == 0) b_c[I] = acc;
    }
}

// x[i] += omega sum_J P[i, J] x_c[J], the same grouping
template <int G>
__global__ __launch_bounds__(kBlock) void amg_prolong_csr_kernel(int64_t n, double omega, const int32_t* __restrict__ row_ptr,
                                                                 const int32_t* __restrict__ col, const double* __restrict__ val,
                                                                 const double* __restrict__ x_c, double* __restrict__ x)
{
    constexpr int RPB = kBlock / G;
    const int     t   = threadIdx.x % G;
    for (int64_t i = (int64_t)blockIdx.x * RPB + threadIdx.x / G; i < n; i += (int64_t)gridDim.x * RPB)
    {
        double        acc = 0.0;
        const int64_t end = row_ptr[i + 1];
        for (int64_t k = (int64_t)row_ptr[i] + t; k < end; k += G) acc = fma(val[k], x_c[col[k]], acc);
        acc = group_sum_swizzle<G>(acc);
        if (t == 0) x[i] = fma(omega, acc, x[i]);
    }
}

// one instance per group size: G = 1, 2, 4, .., 64
#define SPMV_AMG_BY_LANES(lanes, KERNEL, grid, stream, ...)                                                                \
    switch (lanes)                                                                                                         \
    {                                                                                                                      \
        case 1: hipLaunchKernelGGL(KERNEL<1>, grid, dim3(kBlock), 0, stream, __VA_ARGS__); break;                          \
        case 2: hipLaunchKernelGGL(KERNEL<2>, grid, dim3(kBlock), 0, stream, __VA_ARGS__); break;                          \
        case 4: hipLaunchKernelGGL(KERNEL<4>, grid, dim3(kBlock), 0, stream, __VA_ARGS__); break;                          \
        case 8: hipLaunchKernelGGL(KERNEL<8>, grid, dim3(kBlock), 0, stream, __VA_ARGS__); break;                          \
        case 16: hipLaunchKernelGGL(KERNEL<16>, grid, dim3(kBlock), 0, stream, __VA_ARGS__); break;                        \
        case 32: hipLaunchKernelGGL(KERNEL<32>, grid, dim3(kBlock), 0, stream, __VA_ARGS__); break;                        \
        default: hipLaunchKernelGGL(KERNEL<64>, grid, dim3(kBlock), 0, stream, __VA_ARGS__); break;                        \
    }
// workgroups of a grid-stride kernel over `rows` rows, `lanes` lanes each
inline dim3 group_grid(int64_t rows, int lanes) { return dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>(kMaxGrid, ceil_div(rows, kBlock / lanes)))); }

// ---- host helpers ----------------------------------------------------------------------------------------------------------------
void free_state(amg_state* st)
{
    if (!st) return;
    for (size_t l = 0; l < st->lv.size(); ++l)
    {
        amg_level& L = st->lv[l];
        for (void* p : {(void*)L.agg, (void*)L.agg_ptr, (void*)L.agg_rows})
            if (p) (void)hipFree(p);
        if (l > 0 && L.A) mat_free(L.A);
        if (L.P) mat_free(L.P);
        if (L.R) mat_free(L.R);
    }
    if (st->inv) (void)hipFree(st->inv);
    if (st->slab) (void)hipFree(st->slab);
    delete st;
}

#define SPMV_AMG_BY_STRENGTH(strong, launch_true, launch_false) \
    do                                                          \
    {                                                           \
        if (strong) launch_true; else launch_false;             \
    } while (0)

// the aggregates of one level: agg[n] (the caller's from here on), their number, the members per aggregate, the rounds
int aggregate(spmv_ctx* ctx, const spmv_mat* A, int level, double theta, int32_t** agg_out, int32_t** count_out, int64_t* nc_out, int32_t* rounds_out)
{
    const char* const who = "spmv_amg_setup";
    const int64_t     n   = A->nrow;
    hipStream_t       s   = ctx->stream;
    const int         grid = stream_grid(n);
    const bool        strong = theta > 0.0;
    const double      theta2 = theta * theta;
    device_pool       pool(ctx, who);
    double*           diag;
    int32_t *         state, *counters, *flag, *root_id, *agg1, *agg, *count;
    uint64_t *        ta, *tb, *tc;
    SPMV_TRY(pool.get(diag, (size_t)n));
    SPMV_TRY(pool.get(state, (size_t)n));
    SPMV_TRY(pool.get(counters, 4));
    SPMV_TRY(pool.get(ta, (size_t)n));
    SPMV_TRY(pool.get(tb, (size_t)n));
    SPMV_TRY(pool.get(tc, (size_t)n));
    SPMV_TRY(hip_step(hipMemsetAsync(counters, 0, 4 * sizeof(int32_t), s), who, "clearing the counters"));
    SPMV_TRY(hip_step(hipMemsetAsync(state, 0, sizeof(int32_t) * (size_t)n, s), who, "clearing the states"));
    hipLaunchKernelGGL(amg_diag_kernel, dim3(grid), dim3(kBlock), 0, s, n, A->a, A->b, A->v, diag, counters);
    int32_t h[4] = {0, 0, 0, 0};
    SPMV_TRY(read_scalars(ctx, h, counters, sizeof(h), who));
    SPMV_REQUIRE(h[0] == 0, "%s: the operator of level %d has %d rows with a zero or missing diagonal entry", who, level, h[0]);
#define SPMV_AMG_PROPAGATE(SRC, in, out)                                                                                                         \
    SPMV_AMG_BY_STRENGTH(strong,                                                                                                                  \
                         hipLaunchKernelGGL((amg_propagate_kernel<SRC, true>), dim3(grid), dim3(kBlock), 0, s, n, A->a, A->b, A->v,              \
                                            (const double*)diag, theta2, (const int32_t*)state, (const uint64_t*)in, out),                        \
                         hipLaunchKernelGGL((amg_propagate_kernel<SRC, false>), dim3(grid), dim3(kBlock), 0, s, n, A->a, A->b, A->v,             \
                                            (const double*)diag, theta2, (const int32_t*)state, (const uint64_t*)in, out))
    int rounds = 0;
    for (;;)
    {
        SPMV_REQUIRE(rounds < kAmgMaxRounds, "%s: the aggregation of level %d did not end within %d rounds", who, level, kAmgMaxRounds);
        SPMV_TRY(hip_step(hipMemsetAsync(counters + 1, 0, sizeof(int32_t), s), who, "clearing the counter of undecided rows"));
        SPMV_AMG_PROPAGATE(kSrcPriority, tc, ta);  // (reads the states alone)
        SPMV_AMG_PROPAGATE(kSrcBuffer, ta, tb);
        SPMV_AMG_PROPAGATE(kSrcRoot, tb, ta);
        SPMV_AMG_PROPAGATE(kSrcBuffer, ta, tc);
        hipLaunchKernelGGL(amg_update_kernel, dim3(grid), dim3(kBlock), 0, s, n, (const uint64_t*)tb, (const uint64_t*)tc, state, counters + 1);
        SPMV_TRY(hip_step(hipGetLastError(), who, "a launch of an aggregation round"));
        ++rounds;
        SPMV_TRY(read_scalars(ctx, h, counters, sizeof(h), who));
        if (h[1] == 0) break;
    }
#undef SPMV_AMG_PROPAGATE
    SPMV_TRY(pool.get(flag, (size_t)n + 1));
    SPMV_TRY(pool.get(root_id, (size_t)n + 1));
    hipLaunchKernelGGL(amg_root_flag_kernel, dim3(stream_grid(n + 1)), dim3(kBlock), 0, s, n, (const int32_t*)state, flag);
    SPMV_TRY(exclusive_scan_i32(ctx, flag, root_id, n + 1));
    int32_t nc = 0;
    SPMV_TRY(read_scalars(ctx, &nc, root_id + n, sizeof(nc), who));
    SPMV_REQUIRE(nc >= 1 && nc <= n, "%s: level %d counts %d roots among %lld rows", who, level, nc, (long long)n);
    SPMV_TRY(pool.get(agg1, (size_t)n));
    SPMV_TRY(pool.get(agg, (size_t)n));
    SPMV_TRY(pool.get(count, (size_t)nc + 1));
    SPMV_TRY(hip_step(hipMemsetAsync(count, 0, sizeof(int32_t) * ((size_t)nc + 1), s), who, "clearing the member counts"));
    SPMV_AMG_BY_STRENGTH(strong,
                         hipLaunchKernelGGL(amg_pass1_kernel<true>, dim3(grid), dim3(kBlock), 0, s, n, A->a, A->b, A->v, (const double*)diag, theta2,
                                            (const int32_t*)state, (const int32_t*)root_id, agg1),
                         hipLaunchKernelGGL(amg_pass1_kernel<false>, dim3(grid), dim3(kBlock), 0, s, n, A->a, A->b, A->v, (const double*)diag, theta2,
                                            (const int32_t*)state, (const int32_t*)root_id, agg1));
    SPMV_AMG_BY_STRENGTH(strong,
                         hipLaunchKernelGGL(amg_pass2_kernel<true>, dim3(grid), dim3(kBlock), 0, s, n, A->a, A->b, A->v, (const double*)diag, theta2,
                                            (const int32_t*)agg1, agg, count, counters + 2),
                         hipLaunchKernelGGL(amg_pass2_kernel<false>, dim3(grid), dim3(kBlock), 0, s, n, A->a, A->b, A->v, (const double*)diag, theta2,
                                            (const int32_t*)agg1, agg, count, counters + 2));
    SPMV_TRY(hip_step(hipGetLastError(), who, "a launch of the aggregation passes"));
    SPMV_TRY(read_scalars(ctx, h, counters, sizeof(h), who));
    SPMV_REQUIRE(h[2] == 0, "%s: %d rows of level %d were left without an aggregate", who, h[2], level);
    pool.keep(agg);
    pool.keep(count);
    *agg_out    = agg;
    *count_out  = count;
    *nc_out     = nc;
    *rounds_out = rounds;
    return SPMV_OK;
}
#undef SPMV_AMG_BY_STRENGTH

// the member lists of a level: agg_ptr (the scan of the member counts) and agg_rows (rows by aggregate, ascending within one)
int member_lists(spmv_ctx* ctx, amg_level& L, const int32_t* count)
{
    const char* const who = "spmv_amg_setup";
    void *            p = nullptr, *q = nullptr;
    if (hipMalloc(&p, sizeof(int32_t) * ((size_t)L.nc + 1)) != hipSuccess || hipMalloc(&q, sizeof(int32_t) * (size_t)L.n) != hipSuccess)
    {
        (void)hipGetLastError();
        if (p) (void)hipFree(p);
        SPMV_FAIL(SPMV_ERR_ALLOC, "%s: out of device memory for the member lists of %lld rows", who, (long long)L.n);
    }
    L.agg_ptr  = (int32_t*)p;
    L.agg_rows = (int32_t*)q;
    SPMV_TRY(exclusive_scan_i32(ctx, count, L.agg_ptr, L.nc + 1));
    return sort_ids_by_key(ctx, L.agg, L.n, key_bits(L.nc), L.agg_rows);
}

// A_c = P^T A P over every stored entry, as a CSR handle of its own
// (`level`: the level the operator becomes, for messages).  A forced kernel id whose product cannot launch on this operator is
// refused here, once, and not by every product of every cycle; no other kernel takes its place.
int coarse_operator(spmv_ctx* ctx, const spmv_mat* A, const int32_t* agg, int64_t nc, int32_t level_kernel, int level, spmv_mat** out)
{
    const char* const who = "spmv_amg_setup";
    const int64_t     n = A->nrow, nnz = A->nnz;
    hipStream_t       s = ctx->stream;
    device_pool       pool(ctx, who);
    int32_t *         key_i, *key_j;
    key_runs          kr;
    SPMV_TRY(pool.get(key_i, (size_t)nnz));
    SPMV_TRY(pool.get(key_j, (size_t)nnz));
    hipLaunchKernelGGL(amg_key_kernel, dim3(stream_grid(n)), dim3(kBlock), 0, s, n, A->a, A->b, agg, key_i, key_j);
    SPMV_TRY(hip_step(hipGetLastError(), who, "the key map's launch"));
    SPMV_TRY(runs_by_key_pair(ctx, pool, who, key_i, nc, key_j, nc, nnz, &kr));
    spmv_mat* C = nullptr;
    SPMV_TRY(mat_alloc(ctx, SPMV_FMT_CSR, (int32_t)nc, (int32_t)nc, kr.runs, 0, (size_t)nc + 1, (size_t)kr.runs, (size_t)kr.runs, &C));
    int rc = exclusive_scan_i32(ctx, kr.count_i, const_cast<int32_t*>(C->a), nc + 1);
    // (row_ptr is also the first run of every row: run s lands at s)
    if (rc == SPMV_OK) rc = runs_sum_into_csr(ctx, who, kr, A->v, C->a, nullptr, C->a, const_cast<int32_t*>(C->b), const_cast<double*>(C->v));
    if (rc == SPMV_OK) rc = hip_step(hipStreamSynchronize(s), who, "waiting for the coarse operator");
    if (rc == SPMV_OK)
    {
        if (level_kernel != SPMV_CSR_AUTO)
        {
            C->kernel_forced = true;
            C->kernel        = level_kernel;
        }
        rc = csr_analyse(C);  // the engine's usual selection: the model and, where it pays, a trial
        if (rc == SPMV_OK && C->kernel_forced && C->kernel == SPMV_CSR_LDSWIN && !csr_ldswin_fits(C))
        {
            set_error("%s: amg_level_kernel=%d (the LDS-window kernel) cannot run the operator of level %d (%lld rows): its widest block window "
                      "is %d columns, the tile holds %d",
                      who, level_kernel, level, (long long)nc, C->win_max_span, csr_ldswin_capacity());
            rc = SPMV_ERR_UNSUPPORTED;
        }
    }
    if (rc != SPMV_OK)
    {
        mat_free(C);
        return rc;
    }
    *out = C;
    return SPMV_OK;
}

// a transient handle of a set-up step: freed when the step returns however it returns
struct mat_holder
{
    spmv_mat* m = nullptr;
    mat_holder() = default;
    mat_holder(const mat_holder&)            = delete;
    mat_holder& operator=(const mat_holder&) = delete;
    ~mat_holder() { reset(); }
    void reset()
    {
        if (m) mat_free(m);
        m = nullptr;
    }
    spmv_mat* release()
    {
        spmv_mat* p = m;
        m           = nullptr;
        return p;
    }
};

// A^F of a level under theta > 0, as a CSR handle of its own (not analysed: only spgemm and the set-up kernels read it)
int filtered_operator(spmv_ctx* ctx, const spmv_mat* A, double theta, int level, const char* who, spmv_mat** out)
{
    const int64_t n = A->nrow;
    hipStream_t   s = ctx->stream;
    const double  theta2 = theta * theta;
    device_pool   pool(ctx, who);
    double*       diag;
    int32_t *     count, *f_rp, *zeros;
    SPMV_TRY(pool.get(diag, (size_t)n));
    SPMV_TRY(pool.get(count, (size_t)n + 1));
    SPMV_TRY(pool.get(f_rp, (size_t)n + 1));
    SPMV_TRY(pool.get(zeros, 1));
    SPMV_TRY(hip_step(hipMemsetAsync(zeros, 0, sizeof(int32_t), s), who, "clearing the counter"));
    hipLaunchKernelGGL(amg_diag_kernel, dim3(stream_grid(n)), dim3(kBlock), 0, s, n, A->a, A->b, A->v, diag, zeros);  // (aggregate() saw no zero)
    hipLaunchKernelGGL(amg_filter_count_kernel, dim3(stream_grid(n + 1)), dim3(kBlock), 0, s, n, A->a, A->b, A->v, (const double*)diag, theta2, count);
    SPMV_TRY(hip_step(hipGetLastError(), who, "the filter's counting launch"));
    SPMV_TRY(exclusive_scan_i32(ctx, count, f_rp, n + 1));
    int32_t entries = 0;
    SPMV_TRY(read_scalars(ctx, &entries, f_rp + n, sizeof(entries), who));
    SPMV_REQUIRE(entries >= 0 && entries <= A->nnz + n, "%s: the filtered operator of level %d counts %d entries", who, level, entries);
    spmv_mat* F = nullptr;
    SPMV_TRY(mat_alloc(ctx, SPMV_FMT_CSR, (int32_t)n, (int32_t)n, entries, 0, (size_t)n + 1, (size_t)entries, (size_t)entries, &F));
    int rc = hip_step(hipMemcpyAsync(const_cast<int32_t*>(F->a), f_rp, sizeof(int32_t) * ((size_t)n + 1), hipMemcpyDeviceToDevice, s), who,
                      "copying the filtered row offsets");
    if (rc == SPMV_OK)
    {
        hipLaunchKernelGGL(amg_filter_fill_kernel, dim3(stream_grid(n)), dim3(kBlock), 0, s, n, A->a, A->b, A->v, (const double*)diag, theta2, F->a,
                           const_cast<int32_t*>(F->b), const_cast<double*>(F->v));
        rc = hip_step(hipGetLastError(), who, "the filter's filling launch");
    }
    if (rc == SPMV_OK) rc = hip_step(hipStreamSynchronize(s), who, "waiting for the filtered operator");
    if (rc != SPMV_OK)
    {
        mat_free(F);
        return rc;
    }
    *out = F;
    return SPMV_OK;
}

// One level of smoothed aggregation: P, R = P^T and A_c = R A P (`level`: the level of A).  The transients - A^F, T, A P - are gone
// when it returns; the set-up's own handles run the row-parallel kernel and take no trial: only A_c selects (or takes level_kernel)
int smoothed_level(spmv_ctx* ctx, const spmv_mat* A, const int32_t* agg, int64_t nc, double theta, double damping, int32_t level_kernel, int level,
                   spmv_mat** P_out, spmv_mat** R_out, spmv_mat** C_out)
{
#pragma clang fp contract(off)
    const char* const who = "spmv_amg_setup_smoothed";
    const int64_t     n   = A->nrow;
    hipStream_t       s   = ctx->stream;
    mat_holder        F, T, P, R, AP, C;
    const spmv_mat*   AF = A;
    if (theta > 0.0)
    {
        SPMV_TRY(filtered_operator(ctx, A, theta, level, who, &F.m));
        AF = F.m;
    }
    device_pool pool(ctx, who);
    double *    d, *sv;
    int32_t*    zeros;
    SPMV_TRY(pool.get(d, (size_t)n));
    SPMV_TRY(pool.get(sv, (size_t)n));
    SPMV_TRY(pool.get(zeros, 1));
    SPMV_TRY(hip_step(hipMemsetAsync(zeros, 0, sizeof(int32_t), s), who, "clearing the counter"));
    hipLaunchKernelGGL(amg_diag_kernel, dim3(stream_grid(n)), dim3(kBlock), 0, s, n, AF->a, AF->b, AF->v, d, zeros);
    SPMV_TRY(hip_step(hipGetLastError(), who, "the filtered diagonal's launch"));
    int32_t nzero = 0;
    SPMV_TRY(read_scalars(ctx, &nzero, zeros, sizeof(nzero), who));
    SPMV_REQUIRE(nzero == 0, "%s: the filtered operator of level %d has %d rows with a zero diagonal (the weak entries cancel it)", who, level, nzero);
    SPMV_TRY(jacobi_inverse_diagonal(ctx, AF, sv, who, "the prolongator's Jacobi scaling"));
    double lam = 0.0;
    SPMV_TRY(cheby_row_bound(ctx, AF, sv, &lam));
    SPMV_REQUIRE(std::isfinite(lam) && lam > 0.0, "%s: the row bound of level %d is %g: the operator is zero or not finite", who, level, lam);
    const double g = damping / lam;
    // T
    SPMV_TRY(mat_alloc(ctx, SPMV_FMT_CSR, (int32_t)n, (int32_t)nc, n, 0, (size_t)n + 1, (size_t)n, (size_t)n, &T.m));
    hipLaunchKernelGGL(amg_tentative_kernel, dim3(stream_grid(n + 1)), dim3(kBlock), 0, s, n, agg, const_cast<int32_t*>(T.m->a),
                       const_cast<int32_t*>(T.m->b), const_cast<double*>(T.m->v));
    SPMV_TRY(hip_step(hipGetLastError(), who, "the tentative prolongator's launch"));
    // P over the arrays of A^F T
    SPMV_TRY(spgemm(ctx, AF, T.m, SPMV_SPGEMM_AUTO, &P.m, SPMV_CSR_VECTOR));
    hipLaunchKernelGGL(amg_smooth_prolongator_kernel, dim3(stream_grid(n)), dim3(kBlock), 0, s, n, P.m->a, P.m->b, agg, (const double*)d, g,
                       const_cast<double*>(P.m->v));
    SPMV_TRY(hip_step(hipGetLastError(), who, "the prolongator's launch"));
    SPMV_TRY(hip_step(hipStreamSynchronize(s), who, "waiting for the prolongator"));
    T.reset();
    F.reset();
    SPMV_TRY(csr_transpose(ctx, P.m, &R.m, SPMV_CSR_VECTOR));
    SPMV_TRY(spgemm(ctx, A, P.m, SPMV_SPGEMM_AUTO, &AP.m, SPMV_CSR_VECTOR));
    SPMV_TRY(spgemm(ctx, R.m, AP.m, SPMV_SPGEMM_AUTO, &C.m, level_kernel));
    AP.reset();
    if (C.m->kernel_forced && C.m->kernel == SPMV_CSR_LDSWIN && !csr_ldswin_fits(C.m))
        SPMV_FAIL(SPMV_ERR_UNSUPPORTED,
                  "%s: amg_level_kernel=%d (the LDS-window kernel) cannot run the operator of level %d (%lld rows): its widest block window is %d "
                  "columns, the tile holds %d",
                  who, level_kernel, level + 1, (long long)nc, C.m->win_max_span, csr_ldswin_capacity());
    *P_out = P.release();
    *R_out = R.release();
    *C_out = C.release();
    return SPMV_OK;
}

// the inverse of the coarsest operator (n <= 1024): LU with partial pivoting on the host, in double
int dense_inverse(spmv_ctx* ctx, const spmv_mat* A, double** inv_out)
{
#pragma clang fp contract(off)
    const char* const who = "spmv_amg_setup";
    const int         n   = A->nrow;
    const size_t      nnz = (size_t)A->nnz;
    std::vector<int32_t> rp((size_t)n + 1), cc(nnz);
    std::vector<double>  cv(nnz), lu((size_t)n * n, 0.0), inv((size_t)n * n, 0.0);
    hipError_t e = hipMemcpyAsync(rp.data(), A->a, sizeof(int32_t) * ((size_t)n + 1), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && nnz) e = hipMemcpyAsync(cc.data(), A->b, sizeof(int32_t) * nnz, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && nnz) e = hipMemcpyAsync(cv.data(), A->v, sizeof(double) * nnz, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    SPMV_TRY(hip_step(e, who, "downloading the coarsest operator"));
    double largest = 0.0;
    for (int i = 0; i < n; ++i)
        for (int k = rp[(size_t)i]; k < rp[(size_t)i + 1]; ++k) lu[(size_t)i * n + cc[(size_t)k]] += cv[(size_t)k];
    for (double v : lu) largest = std::max(largest, std::fabs(v));
    std::vector<int> perm((size_t)n);
    for (int i = 0; i < n; ++i) perm[(size_t)i] = i;
    for (int k = 0; k < n; ++k)
    {
        int p = k;
        for (int i = k + 1; i < n; ++i)
            if (std::fabs(lu[(size_t)i * n + k]) > std::fabs(lu[(size_t)p * n + k])) p = i;  // the first of the largest
        const double pivot = lu[(size_t)p * n + k];
        if (!(std::fabs(pivot) >= 0x1p-44 * largest) || pivot == 0.0)
            SPMV_FAIL(SPMV_ERR_INVALID, "%s: singular coarsest operator (%d rows: pivot %g at step %d, largest entry %g)", who, n, pivot, k, largest);
        if (p != k)
        {
            std::swap(perm[(size_t)p], perm[(size_t)k]);
            for (int j = 0; j < n; ++j) std::swap(lu[(size_t)p * n + j], lu[(size_t)k * n + j]);
        }
        for (int i = k + 1; i < n; ++i)
        {
            const double m = lu[(size_t)i * n + k] / pivot;
            lu[(size_t)i * n + k] = m;
            if (m != 0.0)
                for (int j = k + 1; j < n; ++j) lu[(size_t)i * n + j] -= m * lu[(size_t)k * n + j];
        }
    }
    // inverse = U^-1 L^-1 P, every column of P at once: rows of `inv` are the right-hand sides' rows
    for (int i = 0; i < n; ++i) inv[(size_t)i * n + perm[(size_t)i]] = 1.0;
    for (int i = 0; i < n; ++i)
        for (int k = 0; k < i; ++k)
        {
            const double m = lu[(size_t)i * n + k];
            if (m != 0.0)
                for (int j = 0; j < n; ++j) inv[(size_t)i * n + j] -= m * inv[(size_t)k * n + j];
        }
    for (int i = n - 1; i >= 0; --i)
    {
        for (int k = i + 1; k < n; ++k)
        {
            const double u = lu[(size_t)i * n + k];
            if (u != 0.0)
                for (int j = 0; j < n; ++j) inv[(size_t)i * n + j] -= u * inv[(size_t)k * n + j];
        }
        const double d = lu[(size_t)i * n + i];
        for (int j = 0; j < n; ++j) inv[(size_t)i * n + j] /= d;
    }
    void* dev = nullptr;
    if (hipMalloc(&dev, sizeof(double) * (size_t)n * n) != hipSuccess)
    {
        (void)hipGetLastError();
        SPMV_FAIL(SPMV_ERR_ALLOC, "%s: out of device memory for the inverse of %d rows", who, n);
    }
    e = hipMemcpyAsync(dev, inv.data(), sizeof(double) * (size_t)n * n, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess)
    {
        (void)hipFree(dev);
        return hip_step(e, who, "uploading the inverse");
    }
    *inv_out = (double*)dev;
    return SPMV_OK;
}
}  // namespace

// ---- checks on the host: the leading fields of the handle alone ------------------------------------------------------------------
int amg_check_handle(const spmv_mat* m, const char* who) { return check_whole_square_csr(m, who, "AMG"); }

int amg_check_setup(const spmv_mat* m, int max_levels, int coarse_max, int smooth_degree, double strength, double overcorrection, const char* who)
{
    SPMV_REQUIRE(max_levels >= 0 && max_levels <= kAmgMaxLevels, "%s: max_levels=%d, must be 1 .. 32 (0: 16)", who, max_levels);
    SPMV_REQUIRE(coarse_max >= 0 && coarse_max <= kAmgDenseMax, "%s: coarse_max=%d, must be 1 .. 1024 (0: 256)", who, coarse_max);
    SPMV_REQUIRE(smooth_degree >= 0 && smooth_degree <= kAmgMaxDegree, "%s: smooth_degree=%d, must be 1 .. 64 (0: 2)", who, smooth_degree);
    SPMV_REQUIRE(std::isfinite(strength), "%s: strength=%g, must be finite (<= 0: every stored entry)", who, strength);
    SPMV_REQUIRE(overcorrection == 0.0 || (overcorrection > 0.0 && overcorrection < 2.0), "%s: overcorrection=%g, must be inside (0, 2) (0: 1.5)", who,
                 overcorrection);
    return amg_check_handle(m, who);
}

int amg_check_setup_smoothed(const spmv_mat* m, int max_levels, int coarse_max, int smooth_degree, double strength, double overcorrection,
                             double prolong_damping, const char* who)
{
    // (the words of amg_check_setup but for the two defaults that differ)
    SPMV_REQUIRE(overcorrection == 0.0 || (overcorrection > 0.0 && overcorrection < 2.0), "%s: overcorrection=%g, must be inside (0, 2) (0: 1)", who,
                 overcorrection);
    SPMV_REQUIRE(prolong_damping == 0.0 || (prolong_damping > 0.0 && prolong_damping < 2.0), "%s: prolong_damping=%g, must be inside (0, 2) (0: 4/3)",
                 who, prolong_damping);
    return amg_check_setup(m, max_levels, coarse_max, smooth_degree, strength, overcorrection, who);
}

// ---- the state in the handle -----------------------------------------------------------------------------------------------------
void amg_free(spmv_mat* m)
{
    if (!m->amg) return;
    m->device_bytes -= m->amg->bytes;
    free_state(m->amg);
    m->amg = nullptr;
}

// the set-up behind both entries (the arguments are checked); smoothed: P, R and A_c = R A P per level in place of the member lists
// and the sums over aggregates
static int amg_build(spmv_ctx* ctx, spmv_mat* m, int max_levels, int coarse_max, int smooth_degree, double strength, double omega, bool smoothed,
                     double damping)
{
    const char* const who = smoothed ? "spmv_amg_setup_smoothed" : "spmv_amg_setup";
    auto deleter = [](amg_state* p) { free_state(p); };
    std::unique_ptr<amg_state, decltype(deleter)> st(new amg_state(), deleter);
    st->max_levels = max_levels ? max_levels : 16;
    st->coarse_max = coarse_max ? coarse_max : 256;
    st->degree     = smooth_degree ? smooth_degree : 2;
    st->strength   = strength > 0.0 ? strength : 0.0;
    st->omega      = omega;
    st->smoothed   = smoothed;
    st->damping    = damping;
    st->lv.emplace_back();
    st->lv[0].A   = m;
    st->lv[0].n   = m->nrow;
    st->lv[0].nnz = m->nnz;
    if (m->nrow > 0)
    {
        // the hierarchy
        for (int l = 0;; ++l)
        {
            const int64_t n = st->lv[(size_t)l].n;
            if (n <= st->coarse_max || l + 1 == st->max_levels) break;
            int32_t *agg = nullptr, *count = nullptr;
            int64_t  nc = 0;
            int32_t  rounds = 0;
            SPMV_TRY(aggregate(ctx, st->lv[(size_t)l].A, l, st->strength, &agg, &count, &nc, &rounds));
            st->mis_rounds += rounds;
            if (5 * nc > 4 * n)  // stalled: this level is the coarsest
            {
                (void)hipFree(agg);
                (void)hipFree(count);
                break;
            }
            spmv_mat* C = nullptr;
            if (!smoothed)
            {
                amg_level& L = st->lv[(size_t)l];
                L.agg        = agg;
                L.nc         = nc;
                const int rc = member_lists(ctx, L, count);
                (void)hipStreamSynchronize(ctx->stream);
                (void)hipFree(count);
                SPMV_TRY(rc);
                st->bytes += (int64_t)sizeof(int32_t) * (2 * n + nc + 1);
                SPMV_TRY(coarse_operator(ctx, st->lv[(size_t)l].A, agg, nc, m->amg_level_kernel, l + 1, &C));
            }
            else  // (no member lists: the restriction runs over R)
            {
                amg_level& L = st->lv[(size_t)l];
                L.agg        = agg;
                L.nc         = nc;
                (void)hipStreamSynchronize(ctx->stream);
                (void)hipFree(count);
                st->bytes += (int64_t)sizeof(int32_t) * n;
                SPMV_TRY(smoothed_level(ctx, L.A, agg, nc, st->strength, damping, m->amg_level_kernel, l, &L.P, &L.R, &C));
                L.lanes_p = amg_sa_group_lanes(L.P->nnz, L.P->nrow);
                L.lanes_r = amg_sa_group_lanes(L.R->nnz, L.R->nrow);
                st->bytes += L.P->device_bytes + L.R->device_bytes;
            }
            st->lv.emplace_back();
            amg_level& N = st->lv.back();
            N.A          = C;
            N.n          = nc;
            N.nnz        = C->nnz;
            SPMV_TRY(cheby_setup(ctx, C, st->degree, /*scaled=*/1, 0.0, 0.0));
        }
        // the vectors: w on every level, b and x below level 0
        const size_t nlev = st->lv.size();
        size_t       doubles = 0;
        for (size_t l = 0; l < nlev; ++l) doubles += SolveWorkspace::padded((size_t)st->lv[l].n) * (l == 0 ? 1 : 3);
        if (hipMalloc(&st->slab, sizeof(double) * doubles) != hipSuccess)
        {
            (void)hipGetLastError();
            SPMV_FAIL(SPMV_ERR_ALLOC, "%s: out of device memory for the levels' vectors (%zu bytes)", who, sizeof(double) * doubles);
        }
        st->bytes += (int64_t)(sizeof(double) * doubles);
        double* at = st->slab;
        for (size_t l = 0; l < nlev; ++l)
        {
            const size_t sn = SolveWorkspace::padded((size_t)st->lv[l].n);
            st->lv[l].w     = at;
            at += sn;
            if (l > 0)
            {
                st->lv[l].b = at;
                st->lv[l].x = at + sn;
                at += 2 * sn;
            }
        }
        // the coarsest solve
        const amg_level& last = st->lv.back();
        if (last.n <= kAmgDenseMax)
        {
            SPMV_TRY(dense_inverse(ctx, last.A, &st->inv));
            st->bytes += (int64_t)sizeof(double) * last.n * last.n;
        }
        for (size_t l = 1; l < nlev; ++l) st->bytes += st->lv[l].A->device_bytes;
        // level 0's smoother is the handle's own Chebyshev state; it is replaced last, behind everything that can fail above
        if (nlev > 1 || !st->inv) SPMV_TRY(cheby_setup(ctx, m, st->degree, /*scaled=*/1, 0.0, 0.0));
    }
    SPMV_TRY(hip_step(hipStreamSynchronize(ctx->stream), who, "waiting for the stream"));  // (an application of the earlier state may be in flight)
    amg_free(m);
    m->amg = st.release();
    m->device_bytes += m->amg->bytes;
    return SPMV_OK;
}

int amg_setup(spmv_ctx* ctx, spmv_mat* m, int max_levels, int coarse_max, int smooth_degree, double strength, double overcorrection)
{
    SPMV_TRY(amg_check_setup(m, max_levels, coarse_max, smooth_degree, strength, overcorrection, "spmv_amg_setup"));
    return amg_build(ctx, m, max_levels, coarse_max, smooth_degree, strength, overcorrection != 0.0 ? overcorrection : 1.5, false, 0.0);
}

int amg_setup_smoothed(spmv_ctx* ctx, spmv_mat* m, int max_levels, int coarse_max, int smooth_degree, double strength, double overcorrection,
                       double prolong_damping)
{
    SPMV_TRY(amg_check_setup_smoothed(m, max_levels, coarse_max, smooth_degree, strength, overcorrection, prolong_damping, "spmv_amg_setup_smoothed"));
    return amg_build(ctx, m, max_levels, coarse_max, smooth_degree, strength, overcorrection != 0.0 ? overcorrection : 1.0, true,
                     prolong_damping != 0.0 ? prolong_damping : 4.0 / 3.0);
}

int amg_info(const spmv_mat* m, int32_t* levels, int64_t* rows, int64_t* nnz)
{
    const amg_state* st = m->amg;
    if (!st) SPMV_FAIL(SPMV_ERR_INVALID, "spmv_amg_info: the handle was not set up (spmv_amg_setup)");
    *levels = (int32_t)st->lv.size();
    for (size_t l = 0; l < st->lv.size(); ++l)
    {
        if (rows) rows[l] = st->lv[l].n;
        if (nnz) nnz[l] = st->lv[l].nnz;
    }
    return SPMV_OK;
}

int amg_level_download(spmv_ctx* ctx, const spmv_mat* m, int level, int32_t* agg_host, int32_t* row_ptr, int32_t* col, double* val)
{
    const char* const who = "spmv_amg_level";
    const amg_state*  st  = m->amg;
    if (!st) SPMV_FAIL(SPMV_ERR_INVALID, "%s: the handle was not set up (spmv_amg_setup)", who);
    SPMV_REQUIRE(level >= 0 && level < (int)st->lv.size(), "%s: level=%d, the hierarchy has %d", who, level, (int)st->lv.size());
    const amg_level& L = st->lv[(size_t)level];
    SPMV_REQUIRE(!agg_host || L.agg, "%s: level %d is the coarsest: it has no aggregates", who, level);
    hipStream_t s = ctx->stream;
    hipError_t  e = hipSuccess;
    if (agg_host && L.n) e = hipMemcpyAsync(agg_host, L.agg, sizeof(int32_t) * (size_t)L.n, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && row_ptr) e = hipMemcpyAsync(row_ptr, L.A->a, sizeof(int32_t) * ((size_t)L.n + 1), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && col && L.nnz) e = hipMemcpyAsync(col, L.A->b, sizeof(int32_t) * (size_t)L.nnz, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && val && L.nnz) e = hipMemcpyAsync(val, L.A->v, sizeof(double) * (size_t)L.nnz, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    return hip_step(e, who, "downloading the level");
}

int amg_prolongator_download(spmv_ctx* ctx, const spmv_mat* m, int level, int64_t* nnz, int32_t* row_ptr, int32_t* col, double* val)
{
    const char* const who = "spmv_amg_prolongator";
    const amg_state*  st  = m->amg;
    if (!st) SPMV_FAIL(SPMV_ERR_INVALID, "%s: the handle was not set up (spmv_amg_setup_smoothed)", who);
    SPMV_REQUIRE(st->smoothed, "%s: the hierarchy is plain aggregation (spmv_amg_setup): its prolongator is the aggregates of spmv_amg_level", who);
    SPMV_REQUIRE(level >= 0 && level < (int)st->lv.size(), "%s: level=%d, the hierarchy has %d", who, level, (int)st->lv.size());
    const amg_level& L = st->lv[(size_t)level];
    SPMV_REQUIRE(L.P, "%s: level %d is the coarsest: it has no prolongator", who, level);
    *nnz          = L.P->nnz;
    hipStream_t s = ctx->stream;
    hipError_t  e = hipSuccess;
    if (row_ptr) e = hipMemcpyAsync(row_ptr, L.P->a, sizeof(int32_t) * ((size_t)L.n + 1), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && col && L.P->nnz) e = hipMemcpyAsync(col, L.P->b, sizeof(int32_t) * (size_t)L.P->nnz, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && val && L.P->nnz) e = hipMemcpyAsync(val, L.P->v, sizeof(double) * (size_t)L.P->nnz, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    return hip_step(e, who, "downloading the prolongator");
}

// ---- one transfer of a smoothed level by itself, for measurements (spmv_amg_transfer_timed) -------------------------------------------
int amg_check_transfer(const spmv_mat* m, int level, int what, int lanes, int64_t v_entries, const char* who)
{
    const amg_state* st = m->amg;
    if (!st) SPMV_FAIL(SPMV_ERR_INVALID, "%s: the handle was not set up (spmv_amg_setup_smoothed)", who);
    SPMV_REQUIRE(st->smoothed, "%s: the hierarchy is plain aggregation (spmv_amg_setup): it has no P and R", who);
    SPMV_REQUIRE(level >= 0 && level + 1 < (int)st->lv.size(), "%s: level=%d, the hierarchy has %d and the coarsest has no P and R", who, level,
                 (int)st->lv.size());
    SPMV_REQUIRE(what >= SPMV_AMG_RESTRICT_FUSED && what <= SPMV_AMG_PROLONG_UNFUSED, "%s: what=%d, must be 0 .. 3", who, what);
    SPMV_REQUIRE(lanes == 0 || (lanes >= 1 && lanes <= kAmgSaMaxLanes && (lanes & (lanes - 1)) == 0),
                 "%s: lanes=%d, must be 0 (the level's own) or a power of two in 1 .. 64", who, lanes);
    SPMV_REQUIRE(v_entries == st->lv[(size_t)level].n, "%s: the vector has %lld entries, level %d has %lld rows", who, (long long)v_entries, level,
                 (long long)st->lv[(size_t)level].n);
    return SPMV_OK;
}

// One restriction (v is b; w and b_c are the level's own) or one prolongation (v is x; x_c is the next level's own) of `level`:
// the cycle's fused kernel with the level's lanes or `lanes`, or the same step as a vector pass and a product through the
// handle of R or P (t: a work vector of the level's rows).  Asynchronous.
int amg_transfer_launch(spmv_ctx* ctx, const spmv_mat* m, int level, int what, int lanes, double* v, double* t)
{
    const amg_state* st = m->amg;
    const amg_level& L  = st->lv[(size_t)level];
    const amg_level& N  = st->lv[(size_t)level + 1];
    hipStream_t      s  = ctx->stream;
    apply_extra      over;
    over.overwrite = true;
    switch (what)
    {
        case SPMV_AMG_RESTRICT_FUSED:
        {
            const int g = lanes ? lanes : L.lanes_r;
            SPMV_AMG_BY_LANES(g, amg_restrict_csr_kernel, group_grid(L.nc, g), s, L.nc, L.R->a, L.R->b, L.R->v, (const double*)v, (const double*)L.w, N.b);
            break;
        }
        case SPMV_AMG_RESTRICT_UNFUSED:
            SPMV_TRY(vec_axpby(ctx, 1.0, v, -1.0, L.w, t, L.n));
            SPMV_TRY(mat_apply_ex(ctx, L.R, t, N.b, over));
            break;
        case SPMV_AMG_PROLONG_FUSED:
        {
            const int g = lanes ? lanes : L.lanes_p;
            SPMV_AMG_BY_LANES(g, amg_prolong_csr_kernel, group_grid(L.n, g), s, L.n, st->omega, L.P->a, L.P->b, L.P->v, (const double*)N.x, v);
            break;
        }
        default:
            SPMV_TRY(mat_apply_ex(ctx, L.P, N.x, t, over));
            SPMV_TRY(vec_axpby(ctx, st->omega, t, 1.0, v, v, L.n));
            break;
    }
    return hip_step(hipGetLastError(), "spmv_amg_transfer_timed", "a launch of the transfer");
}

static int64_t amg_launches(const amg_state* st, const spmv_mat* m)
{
    if (!st || m->nrow == 0) return 0;
    int64_t total = 0;
    const size_t nlev = st->lv.size();
    for (size_t l = 0; l < nlev; ++l)
    {
        int64_t d = 0;
        (void)cheby_get_param(st->lv[l].A, "cheby_degree", &d);  // (of the level's state as it stands)
        total += l + 1 < nlev ? 4 * d + 7 : (st->inv ? 1 : 2 * d + 1);
    }
    return total;
}

bool amg_get_param(const spmv_mat* m, const char* name, int64_t* value)
{
    const amg_state* st = m->amg;
    if (!strcmp(name, "amg_ready"))
        *value = st ? 1 : 0;
    else if (!strcmp(name, "amg_levels"))
        *value = st ? (int64_t)st->lv.size() : 0;
    else if (!strcmp(name, "amg_bytes"))
        *value = st ? st->bytes : 0;
    else if (!strcmp(name, "amg_launches"))  // per application
        *value = amg_launches(st, m);
    else if (!strcmp(name, "amg_mis_rounds"))  // the sum over the levels
        *value = st ? st->mis_rounds : 0;
    else if (!strcmp(name, "amg_level_kernel"))
        *value = m->amg_level_kernel;
    else if (!strcmp(name, "amg_smoothed"))
        *value = st && st->smoothed ? 1 : 0;
    else if (!strncmp(name, "amg_lanes_p", 11) || !strncmp(name, "amg_lanes_r", 11))  // "amg_lanes_p<level>", "amg_lanes_r<level>"
    {
        char*      end   = nullptr;
        const long level = name[11] ? strtol(name + 11, &end, 10) : -1;
        if (level < 0 || (end && *end) || !st || !st->smoothed || level + 1 >= (long)st->lv.size()) return false;
        *value = name[10] == 'p' ? st->lv[(size_t)level].lanes_p : st->lv[(size_t)level].lanes_r;
    }
    else
        return false;
    return true;
}

bool amg_set_param(spmv_mat* m, const char* name, int64_t value, int* rc)
{
    *rc = SPMV_OK;
    if (strcmp(name, "amg_level_kernel")) return false;
    if (value < SPMV_CSR_AUTO || value > SPMV_CSR_ELL)
    {
        set_error("%s: a CSR kernel id 1 .. 8 for every coarse handle of the next set-up, or 0 (AUTO), got %lld", name, (long long)value);
        *rc = SPMV_ERR_INVALID;
    }
    else
        m->amg_level_kernel = (int32_t)value;
    return true;
}

// ---- the application: z = B r, one V(1,1) cycle; asynchronous ---------------------------------------------------------------------
int amg_apply(spmv_ctx* ctx, const spmv_mat* A, const double* r, double* z)
{
    const char* const who = "spmv_amg_solve";
    const amg_state*  st  = A->amg;
    if (!st) SPMV_FAIL(SPMV_ERR_INVALID, "%s: the handle was not set up (spmv_amg_setup)", who);
    if (A->nrow == 0) return SPMV_OK;
    hipStream_t  s    = ctx->stream;
    const size_t nlev = st->lv.size();
    apply_extra  over;
    over.overwrite = true;
    for (size_t l = 0; l < nlev; ++l)
    {
        const amg_level& L = st->lv[l];
        const double*    b = l == 0 ? r : L.b;
        double*          x = l == 0 ? z : L.x;
        if (l + 1 == nlev)
        {
            if (st->inv)
                hipLaunchKernelGGL(amg_dense_apply_kernel, dim3((unsigned)ceil_div(L.n, kBlock / kWave)), dim3(kBlock), 0, s, (int)L.n,
                                   (const double*)st->inv, b, x);
            else
                SPMV_TRY(cheby_apply(ctx, L.A, b, x));
            break;
        }
        SPMV_TRY(cheby_apply(ctx, L.A, b, x));
        SPMV_TRY(mat_apply_ex(ctx, L.A, x, L.w, over));
        if (st->smoothed)
        {
            SPMV_AMG_BY_LANES(L.lanes_r, amg_restrict_csr_kernel, group_grid(L.nc, L.lanes_r), s, L.nc, L.R->a, L.R->b, L.R->v, b, (const double*)L.w,
                              st->lv[l + 1].b);
            continue;
        }
        hipLaunchKernelGGL(amg_restrict_kernel, dim3(stream_grid(L.nc)), dim3(kBlock), 0, s, L.nc, (const int32_t*)L.agg_ptr, (const int32_t*)L.agg_rows,
                           b, (const double*)L.w, st->lv[l + 1].b);
    }
    for (size_t l = nlev - 1; l-- > 0;)
    {
        const amg_level& L = st->lv[l];
        const double*    b = l == 0 ? r : L.b;
        double*          x = l == 0 ? z : L.x;
        if (st->smoothed)
        {
            SPMV_AMG_BY_LANES(L.lanes_p, amg_prolong_csr_kernel, group_grid(L.n, L.lanes_p), s, L.n, st->omega, L.P->a, L.P->b, L.P->v,
                              (const double*)st->lv[l + 1].x, x);
        }
        else if (wide_ok(x, L.n))
            hipLaunchKernelGGL(amg_prolong_add_kernel<true>, dim3(pair_grid(L.n)), dim3(kBlock), 0, s, L.n, st->omega, (const int32_t*)L.agg,
                               (const double*)st->lv[l + 1].x, x);
        else
            hipLaunchKernelGGL(amg_prolong_add_kernel<false>, dim3(stream_grid(L.n)), dim3(kBlock), 0, s, L.n, st->omega, (const int32_t*)L.agg,
                               (const double*)st->lv[l + 1].x, x);
        SPMV_TRY(cheby_smooth(ctx, L.A, b, x));
    }
    return hip_step(hipGetLastError(), who, "a launch of the cycle");
}
}  // namespace spmv
