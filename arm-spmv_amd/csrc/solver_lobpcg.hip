// solver_lobpcg.hip — spmv_lobpcg: the nev smallest (or largest) eigenvalues of a symmetric A and their vectors by LOBPCG (Knyazev's
// locally optimal block preconditioned conjugate gradients), device-resident, on CDNA4 (gfx950).
//
// A is any handle the forward product (mat_apply_ex) takes; the product is not changed and gets no kernel here.  The block arithmetic
// - Gram matrices U^T V and recombinations S C of blocks with n rows and up to 3 k = 48 columns - is block_ops.hip's; the small dense
// problems are solved on the host by small_dense.hpp.  What is new here is the driver, the fused residual kernel and the Jacobi scaling.
//
// The workspace (SolveWorkspace; a column a padded vector apart, ld = padded(n)):
//   S  = [X | P | W]     3 k columns: X in columns 0 .. k-1, P (np columns: the active count of the iteration before) behind it, W (na
//   AS = [AX | AP | AW]  columns: this iteration's active count) behind P.  So [X P W] is ONE block of m = k + np + na columns, and
//                        the step's [X_new | P_new] = S [C | C0_active] is written IN PLACE over columns 0 .. k + na - 1: X_new lands
//                        in X's place and P_new where the next iteration looks for P.
//   R                    k columns: AX - X diag(theta)
//   dinv (Jacobi), the partial sums, two Gram results, theta and a coefficient matrix.
// Seven n x k blocks in all.  Dropping P (rank loss, or a basis too close to singular) is the host's business alone: P's rows and
// columns are left out of the small problem and its rows of C are zeros - fma(p, 0.0, acc) leaves acc as it is.
//
// ORTHONORMALISE(B, threshold): G = B^T B; d = diag(G)^-1/2; d G d = L L^T (a pivot - the diagonal entry before its square root -
// below the threshold, or a diagonal entry that is not positive: rank loss, B untouched); B <- B (d L^-T), and AB alike where given.
//
//   start      orthonormalise X (kLobpcgRankPivot; rank loss: INVALID, "start block");  AX = A X;  G = X^T AX symmetrised = Z diag Z^T;
//              X <- X Z, AX <- AX Z, theta = the values (largest: the order reversed)
//   iteration  1  R = AX - X diag(theta), ||R_j||^2: lobpcg_resid_kernel, one launch, last-ticket sums
//              2  the host looks: active = {j: resid_j > tol}; none among the first nev, or max_iter reached: stop
//              3  W_c = M^-1 R_j for the active j;  twice: H = X^T W, W <- W - X H (a combine of [X P W] with the rows (-H; 0; I));
//                 orthonormalise W (kLobpcgRankPivot; rank loss: the first column that depends on those before it is left out of this
//                 iteration - no W, no P from it -, and so on; none left: INVALID, the last iterate is returned);  AW = A W
//              4  P (if any): orthonormalise P, AP alike; rank loss drops P for this iteration
//              5  GB = S^T S, GA = S^T AS (symmetrised on the host), read together
//              6  GA c = theta GB c on the host (generalised_eigh); the smallest pivot of GB in unit-diagonal scaling below
//                 kLobpcgBasisPivot with P in use: once more without P;  the k lowest (largest: highest) pairs
//              7  [X | P] <- S [C | C0_active], [AX | AP] <- AS [C | C0_active], in place (C0: C with the rows of X cleared)
// Launches of an iteration with a active columns and P in use: a preconditioner applications and a products, the residual, 6 Gram
// launches (X^T W twice, W^T W, P^T P, S^T S, S^T AS) and 7 combines (W twice, W, P, AP, S, AS).  Six host looks: the residual norms
// and five Gram results (GB and GA come together).
//
// Every sum over the rows is deterministic (block_ops.hip; here the last-ticket pattern of solver_common.hpp): a solve is exactly as
// reproducible as the product its handle runs.
#include <cmath>
#include <vector>

#include "common.hpp"
#include "small_dense.hpp"
#include "solver_common.hpp"
#include "solver_host.hpp"
#include "wave.hpp"

namespace spmv
{
namespace
{
constexpr int    kLobpcgMaxK       = SPMV_LOBPCG_MAX_K;
constexpr int    kLobpcgMaxBasis   = 3 * kLobpcgMaxK;
constexpr double kLobpcgRankPivot  = 1e-6;  // orthonormalisation of X, W, P: a pivot below it is rank loss
constexpr double kLobpcgBasisPivot = 1e-4;  // GB = S^T S in unit-diagonal scaling: below it the step is redone without P
static_assert(kLobpcgMaxBasis <= kBlockMaxCols && kLobpcgMaxBasis <= dense::kMaxOrder, "the basis fits the block kernels and the small solver");

struct LobpcgState
{
    uint32_t ticket;
    uint32_t pad;
    double   norm2[kLobpcgMaxK];  // ||R_j||^2
};

// R_j = AX_j - theta_j X_j and ||R_j||^2 for every column, one launch: a column after the other, each a grid-stride sweep with its own
// per-workgroup partial sum; the workgroup with the last ticket adds every column's in buffer order
__global__ __launch_bounds__(kBlock) void lobpcg_resid_kernel(int64_t n, int k, int64_t ld, const double* __restrict__ X, const double* __restrict__ AX,
                                                              double* __restrict__ R, const double* __restrict__ theta, double* __restrict__ part,
                                                              LobpcgState* __restrict__ s)
{
    __shared__ double s_part[kBlock / kWave];
    const int64_t     stride = (int64_t)gridDim.x * kBlock;
    for (int j = 0; j < k; ++j)
    {
        const double  th  = theta[j];
        const int64_t at  = (int64_t)j * ld;
        double        acc = 0.0;
        for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride)
        {
            const double r = fma(-th, X[at + i], AX[at + i]);
            R[at + i]      = r;
            acc            = fma(r, r, acc);
        }
        const double t = block_sum_all(acc, s_part);
        if (threadIdx.x == 0) part[(int64_t)j * gridDim.x + blockIdx.x] = t;
    }
    if (!took_last_ticket(&s->ticket)) return;
    for (int j = 0; j < k; ++j)
    {
        double a = 0.0;
        for (int g = threadIdx.x; g < (int)gridDim.x; g += kBlock) a += partial_sum_load(part + (int64_t)j * gridDim.x + g);
        const double t = block_sum_all(a, s_part);
        if (threadIdx.x == 0) s->norm2[j] = t;
    }
    if (threadIdx.x == 0) s->ticket = 0;
}

// w = dinv .* r (Jacobi)
__global__ __launch_bounds__(kBlock) void lobpcg_scale_kernel(int64_t n, const double* __restrict__ dinv, const double* __restrict__ r, double* __restrict__ w)
{
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) w[i] = dinv[i] * r[i];
}
}  // namespace

int lobpcg_solve(spmv_ctx* ctx, const spmv_mat* A, int k, int nev, bool largest, double* X_user, int max_iter, double tol, int precond, double* theta,
                 double* resid, int* iters)
{
    const char* const who = "spmv_lobpcg";
    const int64_t     n   = A->nrow;
    hipStream_t       st  = ctx->stream;
    *iters                = 0;
    const size_t  sn = SolveWorkspace::padded((size_t)n);
    const int64_t ld = (int64_t)sn;
    const int     mb = 3 * k;  // columns of S at most
    const bool    jacobi = precond == SPMV_PRECOND_JACOBI;
    constexpr size_t kSlot = (size_t)kLobpcgMaxBasis * kLobpcgMaxBasis;  // doubles of a Gram result
    constexpr size_t kCoef = 32;                                        // doubles in front of the coefficient matrix: theta
    double *         S, *AS, *R, *dinv = nullptr, *part, *Gdev, *Cdev;
    LobpcgState*     s = nullptr;
    SolveWorkspace   ws(ctx, who);
    ws.piece(S, (size_t)mb * sn);
    ws.piece(AS, (size_t)mb * sn);
    ws.piece(R, (size_t)k * sn);
    if (jacobi) ws.piece(dinv, n);
    ws.piece(part, std::max(block_gram_part_bound(mb), (size_t)k * (size_t)kMaxGrid));
    ws.piece(Gdev, 2 * kSlot);
    ws.piece(Cdev, kCoef + (size_t)mb * 2 * k);
    SPMV_TRY(ws.allocate((void**)&s, sizeof(LobpcgState)));
    SPMV_TRY(setup_preconditioner(ctx, A, precond, dinv, who));
    const int   grid = stream_grid(n);
    apply_extra over;
    over.overwrite = true;
    // the padding rows of the blocks are never read; the columns are cleared once so that no launch ever reads an uninitialised P
    SPMV_TRY(hip_step(hipMemsetAsync(S, 0, sizeof(double) * (size_t)mb * sn, st), who, "clearing the basis"));
    SPMV_TRY(hip_step(hipMemsetAsync(AS, 0, sizeof(double) * (size_t)mb * sn, st), who, "clearing the basis"));
    for (int j = 0; j < k; ++j)
        SPMV_TRY(hip_step(hipMemcpyAsync(S + (size_t)j * sn, X_user + (size_t)j * n, sizeof(double) * n, hipMemcpyDeviceToDevice, st), who, "copying X in"));
    auto copy_out = [&]() -> int {
        for (int j = 0; j < k; ++j)
            SPMV_TRY(hip_step(hipMemcpyAsync(X_user + (size_t)j * n, S + (size_t)j * sn, sizeof(double) * n, hipMemcpyDeviceToDevice, st), who, "copying X out"));
        return SPMV_OK;
    };
    std::vector<double> G(2 * kSlot), coef(kCoef + (size_t)mb * 2 * k);
    auto gram = [&](int p, const double* U, int q, const double* V, int slot) {
        return block_gram_launch(ctx, n, p, U, ld, q, V, ld, Gdev + slot * kSlot, part, &s->ticket);
    };
    auto fetch = [&](size_t doubles) { return read_scalars(ctx, G.data(), Gdev, sizeof(double) * doubles, who); };
    // the coefficient matrix (p x q, row-major, in coef behind theta's place) to the device, then Out = B C
    auto combine = [&](int p, const double* B, int q, double* Out, bool upload) -> int {
        if (upload) SPMV_TRY(write_scalars(ctx, Cdev + kCoef, coef.data() + kCoef, sizeof(double) * (size_t)p * q, who, "writing the coefficients"));
        return block_combine_launch(ctx, n, p, B, ld, q, Cdev + kCoef, Out, ld);
    };
    double* const cm = coef.data() + kCoef;
    // 0: B (and AB) orthonormalised in place;  1: rank loss, nothing written;  < 0: an error code.  With `kept`: a column that depends on
    // those before it (a pivot below kLobpcgRankPivot in unit-diagonal scaling) is left out, and so on; the columns that stay are
    // orthonormalised into the first kept->size() columns of B and named in *kept; 1 only when none stays
    auto orthonormalise = [&](double* B, double* AB, int c, std::vector<int>* kept = nullptr) -> int {
        int rc = gram(c, B, c, B, 0);
        if (rc == SPMV_OK) rc = fetch((size_t)c * c);
        if (rc != SPMV_OK) return rc;
        std::vector<int>    keep(c);
        std::vector<double> d(c), L((size_t)c * c), Li((size_t)c * c);
        for (int i = 0; i < c; ++i) keep[i] = i;
        int r = c;
        for (;;)
        {
            int bad = -1;
            for (int i = 0; i < r && bad < 0; ++i)
            {
                const double g = G[(size_t)keep[i] * c + keep[i]];
                if (!(g > 0.0) || !std::isfinite(g)) bad = i;
                else d[i] = 1.0 / std::sqrt(g);
            }
            if (bad < 0)
            {
                for (int i = 0; i < r; ++i)
                    for (int j = 0; j < r; ++j) L[(size_t)i * r + j] = i == j ? 1.0 : d[i] * G[(size_t)keep[i] * c + keep[j]] * d[j];
                bad = dense::cholesky_first_pivot_below(r, L.data(), kLobpcgRankPivot);
            }
            if (bad < 0) break;
            if (!kept) return 1;
            keep.erase(keep.begin() + bad);
            if (--r == 0) return 1;
        }
        double pivot = 0.0;
        if (!dense::cholesky_lower(r, L.data(), &pivot)) return 1;
        dense::tri_inverse_lower(r, L.data(), Li.data());
        for (size_t e = 0; e < (size_t)c * r; ++e) cm[e] = 0.0;
        for (int i = 0; i < r; ++i)
            for (int j = i; j < r; ++j) cm[(size_t)keep[i] * r + j] = d[i] * Li[(size_t)j * r + i];
        rc = combine(c, B, r, B, true);
        if (rc == SPMV_OK && AB) rc = combine(c, AB, r, AB, false);
        if (kept) kept->swap(keep);
        return rc;
    };
    double* const Xd  = S;
    double* const AXd = AS;
    // ---- the start: orthonormal X, AX, Rayleigh-Ritz ---------------------------------------------------------------------------
    {
        const int rc = orthonormalise(Xd, nullptr, k);
        if (rc < 0) return rc;
        if (rc == 1)
            SPMV_FAIL(SPMV_ERR_INVALID, "%s: the start block has lost rank: its columns are linearly dependent to a pivot below %g (or not finite)", who,
                      kLobpcgRankPivot);
    }
    for (int j = 0; j < k; ++j) SPMV_TRY(mat_apply_ex(ctx, A, Xd + (size_t)j * sn, AXd + (size_t)j * sn, over));
    SPMV_TRY(gram(k, Xd, k, AXd, 0));
    SPMV_TRY(fetch((size_t)k * k));
    std::vector<double> th(mb), Z((size_t)mb * mb), GAc((size_t)mb * mb), GBc((size_t)mb * mb);
    {
        for (int i = 0; i < k; ++i)
            for (int j = 0; j < k; ++j) GAc[(size_t)i * k + j] = 0.5 * (G[(size_t)i * k + j] + G[(size_t)j * k + i]);
        if (!dense::jacobi_eigh(k, GAc.data(), Z.data(), th.data()))
            SPMV_FAIL(SPMV_ERR_INVALID, "%s: X^T A X of the start block is not finite (non-finite numbers in the matrix or in X)", who);
        for (int j = 0; j < k; ++j)
        {
            const int c = largest ? k - 1 - j : j;
            theta[j]    = th[c];
            for (int i = 0; i < k; ++i) cm[(size_t)i * k + j] = Z[(size_t)i * k + c];
        }
        SPMV_TRY(combine(k, Xd, k, Xd, true));
        SPMV_TRY(combine(k, AXd, k, AXd, false));
    }
    // ---- the iteration -----------------------------------------------------------------------------------------------------------
    int np = 0, it = 0, rc = SPMV_OK;
    std::vector<int> active;
    LobpcgState      h;
    for (;;)
    {
        // 1, 2: the residuals and the host's look
        for (int j = 0; j < k; ++j) coef[j] = theta[j];
        if ((rc = write_scalars(ctx, Cdev, coef.data(), sizeof(double) * k, who, "writing theta")) != SPMV_OK) break;
        hipLaunchKernelGGL(lobpcg_resid_kernel, dim3(grid), dim3(kBlock), 0, st, n, k, ld, (const double*)Xd, (const double*)AXd, R, (const double*)Cdev, part, s);
        if ((rc = read_scalars(ctx, &h, s, sizeof(LobpcgState), who)) != SPMV_OK) break;
        bool finite = true;
        for (int j = 0; j < k; ++j)
        {
            resid[j] = std::sqrt(h.norm2[j]);
            if (!std::isfinite(theta[j]))
            {
                set_error("%s: theta_%d is not finite at iteration %d (non-finite numbers in the matrix or in X, or overflow)", who, j, it);
                finite = false;
            }
            else if (!std::isfinite(resid[j]))
            {
                set_error("%s: the residual norm of column %d is not finite at iteration %d (non-finite numbers in the matrix, or overflow)", who, j, it);
                finite = false;
            }
        }
        if (!finite)
        {
            rc = SPMV_ERR_INVALID;
            break;
        }
        active.clear();
        bool wanted = false;
        for (int j = 0; j < k; ++j)
            if (resid[j] > tol)
            {
                active.push_back(j);
                wanted = wanted || j < nev;
            }
        if (!wanted || it >= max_iter) break;
        int           na = (int)active.size(), m = k + np + na;
        double* const Pd = S + (size_t)k * sn, * const APd = AS + (size_t)k * sn;
        double* const Wd = S + (size_t)(k + np) * sn, * const AWd = AS + (size_t)(k + np) * sn;
        // 3: W = M^-1 R_active, projected against X twice, orthonormalised; AW
        for (int c = 0; c < na && rc == SPMV_OK; ++c)
        {
            const double* r = R + (size_t)active[c] * sn;
            double*       w = Wd + (size_t)c * sn;
            if (precond == SPMV_PRECOND_NONE)
                rc = hip_step(hipMemcpyAsync(w, r, sizeof(double) * n, hipMemcpyDeviceToDevice, st), who, "copying a residual");
            else if (jacobi)
                hipLaunchKernelGGL(lobpcg_scale_kernel, dim3(grid), dim3(kBlock), 0, st, n, (const double*)dinv, r, w);
            else
                rc = apply_preconditioner(ctx, A, precond, r, w);
        }
        for (int pass = 0; pass < 2 && rc == SPMV_OK; ++pass)
        {
            if ((rc = gram(k, Xd, na, Wd, 0)) != SPMV_OK || (rc = fetch((size_t)k * na)) != SPMV_OK) break;
            for (int i = 0; i < m; ++i)
                for (int c = 0; c < na; ++c)
                    cm[(size_t)i * na + c] = i < k ? -G[(size_t)i * na + c] : (i == k + np + c ? 1.0 : 0.0);
            rc = combine(m, S, na, Wd, true);
        }
        if (rc != SPMV_OK) break;
        {
            // rank loss among the residuals: the first column that depends on those before it is left out of this iteration, and so on;
            // none left: INVALID
            std::vector<int> kept;
            const int        o = orthonormalise(Wd, nullptr, na, &kept);
            if (o < 0)
            {
                rc = o;
                break;
            }
            if (o == 1)
            {
                set_error("%s: the preconditioned residuals have lost rank at iteration %d (no column with a pivot of %g or more): X, theta and resid hold the last iterate",
                          who, it, kLobpcgRankPivot);
                rc = SPMV_ERR_INVALID;
                break;
            }
            for (size_t i = 0; i < kept.size(); ++i) active[i] = active[(size_t)kept[i]];
            active.resize(kept.size());
            na = (int)kept.size();
            m  = k + np + na;
        }
        for (int c = 0; c < na && rc == SPMV_OK; ++c) rc = mat_apply_ex(ctx, A, Wd + (size_t)c * sn, AWd + (size_t)c * sn, over);
        if (rc != SPMV_OK) break;
        // 4: P
        bool use_p = np > 0;
        if (use_p)
        {
            const int o = orthonormalise(Pd, APd, np);
            if (o < 0)
            {
                rc = o;
                break;
            }
            if (o == 1) use_p = false;
        }
        // 5: the Gram matrices of the basis, read together
        if ((rc = gram(m, S, m, S, 0)) != SPMV_OK || (rc = gram(m, S, m, AS, 1)) != SPMV_OK || (rc = fetch(kSlot + (size_t)m * m)) != SPMV_OK) break;
        const double* GB = G.data();
        const double* GA = G.data() + kSlot;
        // 6: the small problem over the columns in use
        int         mu = 0;
        int         at[kLobpcgMaxBasis];
        bool        solved = false;
        for (;;)
        {
            mu = 0;
            for (int i = 0; i < m; ++i)
                if (use_p || i < k || i >= k + np) at[mu++] = i;
            for (int i = 0; i < mu; ++i)
                for (int j = 0; j < mu; ++j)
                {
                    GBc[(size_t)i * mu + j] = GB[(size_t)at[i] * m + at[j]];
                    GAc[(size_t)i * mu + j] = 0.5 * (GA[(size_t)at[i] * m + at[j]] + GA[(size_t)at[j] * m + at[i]]);
                }
            double pivot = 0.0;
            solved       = dense::generalised_eigh(mu, GAc.data(), GBc.data(), th.data(), Z.data(), &pivot);
            if ((!solved || pivot < kLobpcgBasisPivot) && use_p)
            {
                use_p = false;
                continue;
            }
            break;
        }
        if (!solved)
        {
            set_error("%s: the basis [X W] has lost rank, or its Gram matrices are not finite, at iteration %d: X, theta and resid hold the last iterate", who, it);
            rc = SPMV_ERR_INVALID;
            break;
        }
        // 7: [X | P] <- S [C | C0_active], [AX | AP] alike
        const int q = k + na;
        for (size_t e = 0; e < (size_t)m * q; ++e) cm[e] = 0.0;
        for (int i = 0; i < mu; ++i)
        {
            double* row = cm + (size_t)at[i] * q;
            for (int j = 0; j < k; ++j) row[j] = Z[(size_t)i * mu + (largest ? mu - 1 - j : j)];
            if (at[i] >= k)
                for (int c = 0; c < na; ++c) row[k + c] = row[active[c]];
        }
        for (int j = 0; j < k; ++j) theta[j] = th[largest ? mu - 1 - j : j];
        if ((rc = combine(m, S, q, S, true)) != SPMV_OK || (rc = combine(m, AS, q, AS, false)) != SPMV_OK) break;
        np = na;
        ++it;
    }
    if (rc == SPMV_OK) rc = hip_step(hipGetLastError(), who, "a launch of the iteration");
    *iters = it;
    if (rc == SPMV_OK || rc == SPMV_ERR_INVALID)
    {
        const int out = copy_out();  // (an error's text stays: copy_out sets one only where it fails itself)
        if (rc == SPMV_OK) rc = out;
    }
    return rc;  // (the workspace waits for the stream and frees)
}
}  // namespace spmv
