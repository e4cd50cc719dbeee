// chebyshev.hip — the Chebyshev polynomial preconditioner / smoother (SPMV_PRECOND_CHEBYSHEV, spmv_chebyshev_*) and the Lanczos
// spectrum estimate that feeds it (spmv_lanczos), device-resident, on CDNA4 (gfx950).
//
// The operator.  s_i = 1 / a_ii (scaled; the diagonal as Jacobi reads it from a CSR handle) or 1; B = diag(s) A; 0 < lmin < lmax hold
// B's spectrum (lmax must, lmin need not).  With theta = (lmax + lmin) / 2, delta = (lmax - lmin) / 2, sigma = theta / delta and
//   rho_0 = 1 / sigma;  c0 = 1 / theta;  for k = 1..d:  rho_k = 1 / (2 sigma - rho_{k-1});  c1_k = rho_k rho_{k-1};  c2_k = 2 rho_k / delta
// (cheby_coefficients: on the host, in double, one rounded operation per line, nothing contracted) the application z = M^-1 r is
//   d = c0 (s .* r);  z = d;  t = r
//   for k = 1..d:  w = A d;  t = t - w;  d = c1_k d + c2_k (s .* t);  z = z + d
// that is z = p_d(B) diag(s) r: the start and the d terms are d + 1 corrections of the Chebyshev iteration, p_d has degree d, and
// 1 - lambda p_d(lambda) = T_{d+1}((theta - lambda) / delta) / T_{d+1}(sigma).  r is never written.
//
// Launches of one application, 2 d + 1: cheby_start_kernel, then per term the handle's own forward product (mat_apply_ex, overwrite:
// whatever kernel AUTO chose, any format) and cheby_step_kernel, the whole of the term behind its product in one pass: it reads w, t
// (r in the first term), d, z and s, writes t (not in the last term), d and z - seven vector passes a term (eight scaled), one fewer
// in the last.  c1_k and c2_k are kernel arguments: no device scalar, no dot product, no look by the host.  spmv_chebyshev, the
// smoother x += M^-1 (b - A x), is one product and cheby_resid_kernel (t = b - w) in front of the same launches with z += d.
//
// Width: 16-byte accesses, two elements per lane and an odd last element by one extra lane, where every vector of the launch may
// (solver_host.hpp: wide_ok; the handle's own d, t, w, s always may, the caller's r and z decide); 8-byte accesses otherwise.
// Grid-stride loops, 64-bit indices, no scratch.  From 8M rows on (the rule of vec_axpby: nothing of such vectors survives in a
// cache) w and t go in nontemporal accesses - each is touched once per launch and next by a launch behind a whole product; d and z,
// which the next launch reads back, stay plain.
//
// The bounds.  cheby_row_bound_kernel: max_i |s_i| sum_j |a_ij| over every stored entry of a CSR handle's arrays, the infinity
// norm of B and so a RIGOROUS upper bound of every |lambda|; the maximum over the grid by the last-ticket pattern (a maximum does
// not depend on the order).  Lanczos: m steps without reorthogonalisation on C = diag(sqrt s) A diag(sqrt s), which has B's
// spectrum, run on the vectors u_j = sqrt(s) .* v_j so that no second copy of a vector is needed:
//   u_0 = sqrt(s) .* g / ||g||, g = gen_vec_uniform(seed)
//   w = A u_j;  alpha_j = u_j . w;  y = s .* w - alpha_j u_j - beta_j u_{j-1};  beta_{j+1}^2 = sum y_i^2 / s_i;  u_{j+1} = y / beta_{j+1}
// One product and two launches per step: lanczos_alpha_kernel divides the new u_j and w = A y by beta_j (the normalisation of the
// previous step, folded in) and sums alpha_j; lanczos_update_kernel writes y over u_{j-1} and sums beta_{j+1}^2.  Both sums are
// deterministic (grid_totals).  alpha and beta stay on the device; beta_{j+1} at or below 2^-44 max(|alpha|, beta) seen so far is
// an invariant subspace and ends the run quietly: the kernels write nothing further.  The host reads the coefficients once and
// takes the extreme eigenvalues of the tridiagonal matrix by bisection on the Sturm count.  A Ritz value is a LOWER estimate of
// lmax; spmv_chebyshev_setup multiplies it by 1.05.
#include <cmath>
#include <memory>

#include "common.hpp"
#include "solver_common.hpp"
#include "solver_host.hpp"
#include "wave.hpp"

namespace spmv
{
struct cheby_state
{
    int32_t degree = 0, scaled = 0;
    double  lmin = 0.0, lmax = 0.0;
    int32_t lmin_from = 0, lmax_from = 0;  // kCheby*: where each bound came from
    double  c0 = 0.0;
    std::vector<double> c1, c2;  // [degree]
    double* slab = nullptr;      // d | t | w | s, a padded vector apart
    double *d = nullptr, *t = nullptr, *w = nullptr, *s = nullptr;
    int64_t bytes = 0;
};

namespace
{
enum : int32_t
{
    kChebyGiven    = 0,  // the caller's
    kChebyRowBound = 1,  // max_i |s_i| sum_j |a_ij|
    kChebyLanczos  = 2,  // 1.05 ritz_max
    kChebyRatio    = 3   // lmax / "cheby_ratio"
};
constexpr int     kChebyMaxDegree  = 64;
constexpr int     kLanczosMaxSteps = 64;
constexpr int64_t kChebyNtRows     = (int64_t)8 << 20;

// ---- the application -----------------------------------------------------------------------------------------------------------
template <bool NT, typename T>
static __device__ __forceinline__ T stream_load(const T* p)
{
    if constexpr (NT)
        return __builtin_nontemporal_load(p);
    else
        return *p;
}
template <bool NT, typename T>
static __device__ __forceinline__ void stream_store(T v, T* p)
{
    if constexpr (NT)
        __builtin_nontemporal_store(v, p);
    else
        *p = v;
}

// d = c0 (s .* r);  z = d (ADD: z += d).  WIDE: r and z are 16-byte aligned
template <bool SCALED, bool ADD, bool WIDE>
__global__ __launch_bounds__(kBlock) void cheby_start_kernel(int64_t n, double c0, const double* __restrict__ r, const double* __restrict__ s,
                                                             double* __restrict__ d, double* __restrict__ z)
{
    const int64_t stride = (int64_t)gridDim.x * kBlock, first = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if constexpr (WIDE)
    {
        const int64_t npairs = n / 2;
        for (int64_t i = first; i < npairs; i += stride)
        {
            f64x2 rv = ((const f64x2*)r)[i];
            if constexpr (SCALED)
            {
                const f64x2 sv = ((const f64x2*)s)[i];
                rv             = f64x2{sv[0] * rv[0], sv[1] * rv[1]};
            }
            const f64x2 dv = f64x2{c0 * rv[0], c0 * rv[1]};
            ((f64x2*)d)[i] = dv;
            if constexpr (ADD)
            {
                const f64x2 zv = ((const f64x2*)z)[i];
                ((f64x2*)z)[i] = f64x2{zv[0] + dv[0], zv[1] + dv[1]};
            }
            else
                ((f64x2*)z)[i] = dv;
        }
    }
    // WIDE: the odd last element, by one lane;  otherwise every element, one per lane
    const bool    lead = blockIdx.x == 0 && threadIdx.x == 0;
    const int64_t from = WIDE ? (((n & 1) && lead) ? n - 1 : n) : first;
    for (int64_t i = from; i < n; i += stride)
    {
        const double di = c0 * (SCALED ? s[i] * r[i] : r[i]);
        d[i]            = di;
        z[i]            = ADD ? z[i] + di : di;
    }
}

// one term behind its product w = A d:  t = t - w;  d = c1 d + c2 (s .* t);  z = z + d
static __device__ __forceinline__ void cheby_term(double w, double tin, double s, double c1, double c2, double& t, double& d, double& z)
{
    t = tin - w;
    d = fma(c1, d, c2 * (s * t));
    z = z + d;
}

// FIRST: t is read from tin = r (which is never written) and written to tout; else tin and tout are both t, updated in place.
// LAST: t is not written.  WIDE: tin and z are 16-byte aligned.  NT (WIDE only): w and t in nontemporal accesses
template <bool SCALED, bool FIRST, bool LAST, bool WIDE, bool NT>
__global__ __launch_bounds__(kBlock) void cheby_step_kernel(int64_t n, double c1, double c2, const double* __restrict__ w, const double* tin,
                                                            double* tout, const double* __restrict__ s, double* __restrict__ d,
                                                            double* __restrict__ z)
{
    static_assert(WIDE || !NT, "the nontemporal accesses are the wide path's");
    const int64_t stride = (int64_t)gridDim.x * kBlock, first = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if constexpr (WIDE)
    {
        const int64_t npairs = n / 2;
        for (int64_t i = first; i < npairs; i += stride)
        {
            const f64x2 wv = stream_load<NT>((const f64x2*)w + i);
            const f64x2 tv = FIRST ? ((const f64x2*)tin)[i] : stream_load<NT>((const f64x2*)tin + i);
            f64x2       sv = f64x2{1.0, 1.0};
            if constexpr (SCALED) sv = ((const f64x2*)s)[i];
            const f64x2 dv = ((const f64x2*)d)[i], zv = ((const f64x2*)z)[i];
            double      t0, t1, d0 = dv[0], d1 = dv[1], z0 = zv[0], z1 = zv[1];
            cheby_term(wv[0], tv[0], sv[0], c1, c2, t0, d0, z0);
            cheby_term(wv[1], tv[1], sv[1], c1, c2, t1, d1, z1);
            if constexpr (!LAST) stream_store<NT>(f64x2{t0, t1}, (f64x2*)tout + i);
            ((f64x2*)d)[i] = f64x2{d0, d1};
            ((f64x2*)z)[i] = f64x2{z0, z1};
        }
    }
    const bool    lead = blockIdx.x == 0 && threadIdx.x == 0;
    const int64_t from = WIDE ? (((n & 1) && lead) ? n - 1 : n) : first;
    for (int64_t i = from; i < n; i += stride)
    {
        double di = d[i], zi = z[i], tn;
        cheby_term(w[i], tin[i], SCALED ? s[i] : 1.0, c1, c2, tn, di, zi);
        if constexpr (!LAST) tout[i] = tn;
        d[i] = di;
        z[i] = zi;
    }
}

// t = b - w (w = A x on entry): the smoother's residual.  WIDE: b is 16-byte aligned
template <bool WIDE>
__global__ __launch_bounds__(kBlock) void cheby_resid_kernel(int64_t n, const double* __restrict__ b, const double* __restrict__ w,
                                                             double* __restrict__ t)
{
    const int64_t stride = (int64_t)gridDim.x * kBlock, first = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if constexpr (WIDE)
    {
        const int64_t npairs = n / 2;
        for (int64_t i = first; i < npairs; i += stride)
        {
            const f64x2 bv = ((const f64x2*)b)[i], wv = ((const f64x2*)w)[i];
            ((f64x2*)t)[i] = f64x2{bv[0] - wv[0], bv[1] - wv[1]};
        }
    }
    const bool    lead = blockIdx.x == 0 && threadIdx.x == 0;
    const int64_t from = WIDE ? (((n & 1) && lead) ? n - 1 : n) : first;
    for (int64_t i = from; i < n; i += stride) t[i] = b[i] - w[i];
}

// ---- the row bound -------------------------------------------------------------------------------------------------------------
// out[0] = max_i |s_i| sum_j |a_ij| over every stored entry (s null: 1).  A row per lane, grid-stride; part takes the workgroups'
// maxima, and the workgroup with the last ticket takes the maximum of those
__global__ __launch_bounds__(kBlock) void cheby_row_bound_kernel(int nrow, const int32_t* __restrict__ row_ptr, const double* __restrict__ val,
                                                                 const double* __restrict__ s, double* __restrict__ part, uint32_t* ticket,
                                                                 double* __restrict__ out)
{
    __shared__ double s_max[kBlock / kWave];
    auto block_max = [&](double m) {
#pragma unroll
        for (int off = kWave / 2; off > 0; off >>= 1) m = fmax(m, __shfl_xor(m, off));
        __syncthreads();  // the previous call's readers are done with s_max
        if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = m;
        __syncthreads();
        double t = s_max[0];
#pragma unroll
        for (int w = 1; w < kBlock / kWave; ++w) t = fmax(t, s_max[w]);
        return t;
    };
    double m = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < nrow; i += (int64_t)gridDim.x * kBlock)
    {
        double    sum = 0.0;
        const int end = row_ptr[i + 1];
        for (int j = row_ptr[i]; j < end; ++j) sum += fabs(val[j]);
        m = fmax(m, s ? fabs(s[i]) * sum : sum);
    }
    m = block_max(m);
    if (threadIdx.x == 0) part[blockIdx.x] = m;
    if (!took_last_ticket(ticket)) return;
    double a = 0.0;
    for (int g = threadIdx.x; g < (int)gridDim.x; g += kBlock) a = fmax(a, partial_sum_load(part + g));
    a = block_max(a);
    if (threadIdx.x == 0)
    {
        out[0]  = a;
        *ticket = 0;
    }
}

// ---- Lanczos -------------------------------------------------------------------------------------------------------------------
struct LanczosState
{
    double   alpha[kLanczosMaxSteps];
    double   beta[kLanczosMaxSteps];  // beta[j] = beta_{j+1}: the norm of the vector step j left
    double   nrm;                     // what the next lanczos_alpha_kernel divides by: ||g|| at the start, beta_j behind a step
    double   scale;                   // max(|alpha|, beta) seen so far
    int32_t  done;                    // steps completed
    int32_t  stop;                    // 1: an invariant subspace (or a sum that is not a number) ended the run
    int32_t  bad;                     // 1: scaled, and an s_i that is not positive
    uint32_t ticket;
};

// g.g of the start vector in q;  SCALED: q = sqrt(s) .* g, and s_i <= 0 (or not a number) is noted
template <bool SCALED>
__global__ __launch_bounds__(kBlock) void lanczos_start_kernel(int64_t n, double* __restrict__ q, const double* __restrict__ s,
                                                               double* __restrict__ part, LanczosState* __restrict__ st)
{
    double acc[1] = {0.0};
    bool   bad    = false;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock)
    {
        const double g = q[i];
        acc[0]         = fma(g, g, acc[0]);
        if constexpr (SCALED)
        {
            const double si = s[i];
            if (!(si > 0.0)) bad = true;
            q[i] = sqrt(si) * g;
        }
    }
    if (bad) st->bad = 1;  // (every writer stores the same word)
    double total[1];
    if (!grid_totals<1>(acc, part, &st->ticket, total)) return;
    if (threadIdx.x == 0)
    {
        st->nrm    = sqrt(total[0]);
        st->ticket = 0;
    }
}

// u_j = q / nrm and w = w / nrm in place (w = A q on entry: the normalisation of the previous step);  alpha_j = u_j . w
__global__ __launch_bounds__(kBlock) void lanczos_alpha_kernel(int64_t n, int j, double* __restrict__ q, double* __restrict__ w,
                                                               double* __restrict__ part, LanczosState* __restrict__ st)
{
    if (st->stop) return;
    const double  nrm    = st->nrm;
    const int64_t npairs = n / 2;
    double        acc[1] = {0.0};
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < npairs; i += (int64_t)gridDim.x * kBlock)
    {
        const f64x2 q0 = ((const f64x2*)q)[i], w0 = ((const f64x2*)w)[i];
        const f64x2 qv = f64x2{q0[0] / nrm, q0[1] / nrm}, wv = f64x2{w0[0] / nrm, w0[1] / nrm};
        ((f64x2*)q)[i] = qv;
        ((f64x2*)w)[i] = wv;
        acc[0]         = fma(qv[1], wv[1], fma(qv[0], wv[0], acc[0]));
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0)
    {
        const double qi = q[n - 1] / nrm, wi = w[n - 1] / nrm;
        q[n - 1]        = qi;
        w[n - 1]        = wi;
        acc[0]          = fma(qi, wi, acc[0]);
    }
    double total[1];
    if (!grid_totals<1>(acc, part, &st->ticket, total)) return;
    if (threadIdx.x == 0)
    {
        st->alpha[j] = total[0];
        st->ticket   = 0;
    }
}

// y = s .* w - alpha_j u_j - beta_j u_{j-1}, written over u_{j-1} (p);  beta_{j+1}^2 = sum y_i^2 / s_i;  the workgroup with the last
// ticket records beta_{j+1} and ends the run at an invariant subspace
template <bool SCALED>
__global__ __launch_bounds__(kBlock) void lanczos_update_kernel(int64_t n, int j, double* __restrict__ p, const double* __restrict__ q,
                                                                const double* __restrict__ w, const double* __restrict__ s,
                                                                double* __restrict__ part, LanczosState* __restrict__ st)
{
    if (st->stop) return;
    const double  alpha = st->alpha[j], beta = j > 0 ? st->beta[j - 1] : 0.0;
    const int64_t npairs = n / 2;
    double        acc[1] = {0.0};
    auto          term   = [&](double wi, double qi, double pi, double si) {
        const double y = fma(-beta, pi, fma(-alpha, qi, SCALED ? si * wi : wi));
        acc[0] += SCALED ? y * y / si : y * y;
        return y;
    };
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < npairs; i += (int64_t)gridDim.x * kBlock)
    {
        const f64x2 wv = ((const f64x2*)w)[i], qv = ((const f64x2*)q)[i], pv = ((const f64x2*)p)[i];
        f64x2       sv = f64x2{1.0, 1.0};
        if constexpr (SCALED) sv = ((const f64x2*)s)[i];
        const double y0 = term(wv[0], qv[0], pv[0], sv[0]), y1 = term(wv[1], qv[1], pv[1], sv[1]);
        ((f64x2*)p)[i]  = f64x2{y0, y1};
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) p[n - 1] = term(w[n - 1], q[n - 1], p[n - 1], SCALED ? s[n - 1] : 1.0);
    double total[1];
    if (!grid_totals<1>(acc, part, &st->ticket, total)) return;
    if (threadIdx.x == 0)
    {
        const double b     = sqrt(total[0]);
        const double scale = fmax(st->scale, fabs(alpha));
        st->beta[j]        = b;
        st->done           = j + 1;
        if (!(b > 0x1p-44 * scale))  // (a sum that is not a number ends here too)
            st->stop = 1;
        else
        {
            st->scale = fmax(scale, b);
            st->nrm   = b;
        }
        st->ticket = 0;
    }
}

// the number of eigenvalues below x of the symmetric tridiagonal matrix (a; b off the diagonal): the Sturm count
int sturm_count(const double* a, const double* b, int m, double x, double tiny)
{
    int    count = 0;
    double q     = 1.0;
    for (int i = 0; i < m; ++i)
    {
        const double off = i > 0 ? b[i - 1] : 0.0;
        q                = (a[i] - x) - (i > 0 ? off * off / q : 0.0);
        if (q == 0.0) q = -tiny;
        if (q < 0.0) ++count;
    }
    return count;
}

// the k-th eigenvalue from below (k = 0 .. m-1) by bisection, to 2 ulp of the largest |value| the Gershgorin discs allow
double tridiagonal_eigenvalue(const double* a, const double* b, int m, int k)
{
    if (m == 1) return a[0];
    double lo = a[0], hi = a[0];
    for (int i = 0; i < m; ++i)
    {
        const double r = (i > 0 ? fabs(b[i - 1]) : 0.0) + (i + 1 < m ? fabs(b[i]) : 0.0);
        lo             = std::min(lo, a[i] - r);
        hi             = std::max(hi, a[i] + r);
    }
    const double big = std::max(fabs(lo), fabs(hi)), tol = 2.0 * 0x1p-52 * big, tiny = 0x1p-52 * 0x1p-52 * std::max(big, 0x1p-900);
    for (int it = 0; it < 200 && hi - lo > tol; ++it)
    {
        const double mid = lo + 0.5 * (hi - lo);
        if (sturm_count(a, b, m, mid, tiny) > k)
            hi = mid;
        else
            lo = mid;
    }
    return lo + 0.5 * (hi - lo);
}

bool has_csr_arrays(const spmv_mat* m) { return m->format == SPMV_FMT_CSR && m->a && ((m->b && m->v) || m->nnz == 0); }

void free_state(cheby_state* st)
{
    if (!st) return;
    if (st->slab) (void)hipFree(st->slab);
    delete st;
}

// max_i |s_i| sum_j |a_ij| of a CSR handle's arrays (s null: unscaled), read by the host
int row_bound(spmv_ctx* ctx, const spmv_mat* m, const double* s, double* bound)
{
    const int    grid  = stream_grid(m->nrow);
    const size_t bytes = sizeof(double) * ((size_t)kMaxGrid + 2);
    SPMV_TRY(ensure_scratch(ctx, bytes));
    double*   part   = (double*)ctx->scratch;
    double*   out    = part + kMaxGrid;
    uint32_t* ticket = (uint32_t*)(part + kMaxGrid + 1);
    SPMV_TRY(hip_step(hipMemsetAsync(out, 0, 2 * sizeof(double), ctx->stream), "spmv_chebyshev_setup", "clearing the row bound"));
    hipLaunchKernelGGL(cheby_row_bound_kernel, dim3(grid), dim3(kBlock), 0, ctx->stream, (int)m->nrow, m->a, m->v, s, part, ticket, out);
    SPMV_TRY(hip_step(hipGetLastError(), "spmv_chebyshev_setup", "the row bound's launch"));
    return read_scalars(ctx, bound, out, sizeof(double), "spmv_chebyshev_setup");
}
}  // namespace

int cheby_row_bound(spmv_ctx* ctx, const spmv_mat* m, const double* s, double* bound) { return row_bound(ctx, m, s, bound); }

// ---- the coefficient table: host only ------------------------------------------------------------------------------------------
int cheby_coefficients(int degree, double lmin, double lmax, double* c0, double* c1, double* c2)
{
#pragma clang fp contract(off)  // one rounded operation per line: the table equals the NumPy twin's bit for bit
    SPMV_REQUIRE(c0 && c1 && c2, "spmv_chebyshev_coefficients: null argument");
    SPMV_REQUIRE(degree >= 1 && degree <= kChebyMaxDegree, "spmv_chebyshev_coefficients: degree=%d, must be 1 .. 64", degree);
    SPMV_REQUIRE(std::isfinite(lmin) && std::isfinite(lmax) && lmin > 0.0 && lmin < lmax,
                 "spmv_chebyshev_coefficients: lmin=%g lmax=%g, must be finite with 0 < lmin < lmax", lmin, lmax);
    const double sum   = lmax + lmin;
    const double theta = sum / 2.0;
    const double diff  = lmax - lmin;
    const double delta = diff / 2.0;
    const double sigma = theta / delta;
    double       rho   = 1.0 / sigma;
    *c0                = 1.0 / theta;
    for (int k = 0; k < degree; ++k)
    {
        const double twice = 2.0 * sigma;
        const double den   = twice - rho;
        const double next  = 1.0 / den;
        c1[k]              = next * rho;
        const double num   = 2.0 * next;
        c2[k]              = num / delta;
        rho                = next;
    }
    return SPMV_OK;
}

// ---- checks on the host: the leading fields of the handle alone ------------------------------------------------------------------
int cheby_check_handle(const spmv_mat* m, const char* who) { return check_whole_square(m, who, "Chebyshev"); }

int cheby_check_scaled(const spmv_mat* m, const char* who)
{
    SPMV_REQUIRE(m->format == SPMV_FMT_CSR, "%s: the Jacobi scaling reads the diagonal of a CSR handle (format %d)", who, m->format);
    return check_csr_arrays(m, who, ": no diagonal for the Jacobi scaling");
}

int cheby_check_setup(const spmv_mat* m, int degree, int scaled, double lmin, double lmax, const char* who)
{
    SPMV_REQUIRE(degree >= 1 && degree <= kChebyMaxDegree, "%s: degree=%d, must be 1 .. 64", who, degree);
    SPMV_REQUIRE(std::isfinite(lmin) && std::isfinite(lmax) && lmin >= 0.0 && lmax >= 0.0,
                 "%s: lmin=%g lmax=%g, must be finite and not negative (0: estimated)", who, lmin, lmax);
    SPMV_REQUIRE(lmax == 0.0 || lmin < lmax, "%s: lmin=%g lmax=%g, must be lmin < lmax", who, lmin, lmax);
    SPMV_TRY(cheby_check_handle(m, who));
    if (scaled) SPMV_TRY(cheby_check_scaled(m, who));
    return SPMV_OK;
}

// ---- the state in the handle -----------------------------------------------------------------------------------------------------
void cheby_free(spmv_mat* m)
{
    if (!m->cheby) return;
    m->device_bytes -= m->cheby->bytes;
    free_state(m->cheby);
    m->cheby = nullptr;
}

int cheby_setup(spmv_ctx* ctx, spmv_mat* m, int degree, int scaled, double lmin, double lmax)
{
    const char* const who = "spmv_chebyshev_setup";
    SPMV_TRY(cheby_check_setup(m, degree, scaled, lmin, lmax, who));
    const int64_t n = m->nrow;
    auto          deleter = [](cheby_state* p) { free_state(p); };
    std::unique_ptr<cheby_state, decltype(deleter)> st(new cheby_state(), deleter);
    st->degree = degree;
    st->scaled = scaled ? 1 : 0;
    if (n > 0)
    {
        const size_t sn = SolveWorkspace::padded((size_t)n), nvec = scaled ? 4 : 3;
        if (hipMalloc(&st->slab, sizeof(double) * sn * nvec) != hipSuccess)
        {
            (void)hipGetLastError();
            SPMV_FAIL(SPMV_ERR_ALLOC, "%s: out of device memory for %zu work vectors of %lld entries", who, nvec, (long long)n);
        }
        st->bytes = (int64_t)(sizeof(double) * sn * nvec);
        st->d     = st->slab;
        st->t     = st->slab + sn;
        st->w     = st->slab + 2 * sn;
        if (scaled)
        {
            st->s = st->slab + 3 * sn;
            SPMV_TRY(jacobi_inverse_diagonal(ctx, m, st->s, who, "Chebyshev's Jacobi scaling"));
        }
        st->lmax_from = kChebyGiven;
        if (lmax == 0.0)
        {
            // the rigorous row bound where the arrays are there, 1.05 times Lanczos' largest Ritz value where it was asked for, the
            // smaller of the two
            double best = 0.0;
            if (has_csr_arrays(m))
            {
                SPMV_TRY(row_bound(ctx, m, st->s, &best));
                st->lmax_from = kChebyRowBound;
            }
            if (m->cheby_lanczos_steps > 0)
            {
                double  rmin = 0.0, rmax = 0.0;
                int32_t done = 0;
                SPMV_TRY(cheby_lanczos(ctx, m, st->scaled, m->cheby_lanczos_steps, 1, &rmin, &rmax, nullptr, nullptr, &done));
                const double est = 1.05 * rmax;
                if (st->lmax_from != kChebyRowBound || est < best)
                {
                    best          = est;
                    st->lmax_from = kChebyLanczos;
                }
            }
            else if (st->lmax_from != kChebyRowBound)
                SPMV_FAIL(SPMV_ERR_UNSUPPORTED,
                          "%s: no source for lmax: the row bound needs a CSR handle with its arrays, the Lanczos estimate \"cheby_lanczos_steps\" > 0", who);
            SPMV_REQUIRE(std::isfinite(best) && best > 0.0, "%s: the estimate of lmax is %g: the matrix is zero, not definite or not finite", who, best);
            lmax = best;
        }
        st->lmin_from = kChebyGiven;
        if (lmin == 0.0)
        {
            lmin          = lmax / (double)m->cheby_ratio;
            st->lmin_from = kChebyRatio;
        }
        SPMV_REQUIRE(lmin > 0.0 && lmin < lmax, "%s: lmin=%g lmax=%g, must be 0 < lmin < lmax", who, lmin, lmax);
        st->lmin = lmin;
        st->lmax = lmax;
        st->c1.resize((size_t)degree);
        st->c2.resize((size_t)degree);
        SPMV_TRY(cheby_coefficients(degree, lmin, lmax, &st->c0, st->c1.data(), st->c2.data()));
    }
    SPMV_TRY(hip_step(hipStreamSynchronize(ctx->stream), who, "waiting for the stream"));  // (an application of the earlier state may be in flight)
    cheby_free(m);
    m->cheby = st.release();
    m->device_bytes += m->cheby->bytes;
    return SPMV_OK;
}

int cheby_info(const spmv_mat* m, int32_t* degree, int32_t* scaled, double* lmin, double* lmax)
{
    const cheby_state* st = m->cheby;
    *degree               = st ? st->degree : 0;
    *scaled               = st ? st->scaled : 0;
    *lmin                 = st ? st->lmin : 0.0;
    *lmax                 = st ? st->lmax : 0.0;
    return SPMV_OK;
}

bool cheby_get_param(const spmv_mat* m, const char* name, int64_t* value)
{
    const cheby_state* st = m->cheby;
    if (!strcmp(name, "cheby_ready"))
        *value = st ? 1 : 0;
    else if (!strcmp(name, "cheby_degree"))  // of the state; not set up: what the solvers' set-up would take
        *value = st ? st->degree : m->cheby_degree;
    else if (!strcmp(name, "cheby_bytes"))
        *value = st ? st->bytes : 0;
    else if (!strcmp(name, "cheby_launches"))  // per application: the start, and a product and a step per term
        *value = st ? 2 * st->degree + 1 : 0;
    else if (!strcmp(name, "cheby_lanczos_steps"))
        *value = m->cheby_lanczos_steps;
    else if (!strcmp(name, "cheby_ratio"))
        *value = m->cheby_ratio;
    else if (!strcmp(name, "cheby_lmax_source"))  // 0 the caller's, 1 the row bound, 2 Lanczos
        *value = st ? st->lmax_from : 0;
    else if (!strcmp(name, "cheby_lmin_source"))  // 0 the caller's, 3 lmax / "cheby_ratio"
        *value = st ? st->lmin_from : 0;
    else
        return false;
    return true;
}

bool cheby_set_param(spmv_mat* m, const char* name, int64_t value, int* rc)
{
    *rc = SPMV_OK;
    auto refuse = [&](const char* range) {
        set_error("%s: %s, got %lld", name, range, (long long)value);
        *rc = SPMV_ERR_INVALID;
    };
    if (!strcmp(name, "cheby_lanczos_steps"))
    {
        if (value < 0 || value > kLanczosMaxSteps) refuse("0 (no Lanczos estimate) .. 64 steps");
        else m->cheby_lanczos_steps = (int32_t)value;
    }
    else if (!strcmp(name, "cheby_ratio"))
    {
        if (value < 2 || value > 1000000) refuse("lmax / lmin in 2 .. 1000000");
        else m->cheby_ratio = (int32_t)value;
    }
    else if (!strcmp(name, "cheby_degree"))
    {
        if (value < 1 || value > kChebyMaxDegree) refuse("1 .. 64");
        else m->cheby_degree = (int32_t)value;
    }
    else
        return false;
    return true;
}

// ---- the application: z = M^-1 r (add: z += M^-1 r; r_is_t: r is the state's own t, as the smoother leaves it) ---------------------
static int cheby_run(spmv_ctx* ctx, const spmv_mat* A, const double* r, double* z, bool add, bool r_is_t)
{
    const cheby_state* st = A->cheby;
    const int64_t      n  = A->nrow;
    hipStream_t        s  = ctx->stream;
    const bool         scaled = st->scaled != 0;
    const bool         wide0 = wide_ok(r, n) && wide_ok(z, n), wide_z = wide_ok(z, n), nt = n >= kChebyNtRows;
    const int          grid_w = pair_grid(n), grid_n = stream_grid(n);
#define SPMV_CHEBY_START(SCALED, ADD, WIDE) \
    hipLaunchKernelGGL((cheby_start_kernel<SCALED, ADD, WIDE>), dim3(WIDE ? grid_w : grid_n), dim3(kBlock), 0, s, n, st->c0, r, (const double*)st->s, st->d, z)
#define SPMV_CHEBY_START_W(SCALED, ADD)                  \
    do                                                   \
    {                                                    \
        if (wide0) SPMV_CHEBY_START(SCALED, ADD, true);  \
        else SPMV_CHEBY_START(SCALED, ADD, false);       \
    } while (0)
    if (scaled)
    {
        if (add) SPMV_CHEBY_START_W(true, true); else SPMV_CHEBY_START_W(true, false);
    }
    else
    {
        if (add) SPMV_CHEBY_START_W(false, true); else SPMV_CHEBY_START_W(false, false);
    }
#undef SPMV_CHEBY_START_W
#undef SPMV_CHEBY_START
    apply_extra over;
    over.overwrite = true;
    for (int k = 0; k < st->degree; ++k)
    {
        SPMV_TRY(mat_apply_ex(ctx, A, st->d, st->w, over));
        const bool    first = k == 0 && !r_is_t, last = k + 1 == st->degree;
        const bool    wide  = wide_z && (!first || wide_ok(r, n));
        const double* tin   = first ? r : st->t;
        const double  c1 = st->c1[(size_t)k], c2 = st->c2[(size_t)k];
#define SPMV_CHEBY_STEP(SCALED, FIRST, LAST, WIDE, NT)                                                                                          \
    hipLaunchKernelGGL((cheby_step_kernel<SCALED, FIRST, LAST, WIDE, NT>), dim3(WIDE ? grid_w : grid_n), dim3(kBlock), 0, s, n, c1, c2, \
                       (const double*)st->w, tin, st->t, (const double*)st->s, st->d, z)
#define SPMV_CHEBY_STEP_W(SCALED, FIRST, LAST)                            \
    do                                                                    \
    {                                                                     \
        if (wide && nt) SPMV_CHEBY_STEP(SCALED, FIRST, LAST, true, true); \
        else if (wide) SPMV_CHEBY_STEP(SCALED, FIRST, LAST, true, false); \
        else SPMV_CHEBY_STEP(SCALED, FIRST, LAST, false, false);          \
    } while (0)
#define SPMV_CHEBY_STEP_FL(SCALED)                             \
    do                                                         \
    {                                                          \
        if (first && last) SPMV_CHEBY_STEP_W(SCALED, true, true);        \
        else if (first) SPMV_CHEBY_STEP_W(SCALED, true, false);          \
        else if (last) SPMV_CHEBY_STEP_W(SCALED, false, true);           \
        else SPMV_CHEBY_STEP_W(SCALED, false, false);                    \
    } while (0)
        if (scaled) SPMV_CHEBY_STEP_FL(true); else SPMV_CHEBY_STEP_FL(false);
#undef SPMV_CHEBY_STEP_FL
#undef SPMV_CHEBY_STEP_W
#undef SPMV_CHEBY_STEP
    }
    return hip_step(hipGetLastError(), "spmv_chebyshev_solve", "a launch of the application");
}

int cheby_apply(spmv_ctx* ctx, const spmv_mat* A, const double* r, double* z)
{
    if (!A->cheby) SPMV_FAIL(SPMV_ERR_INVALID, "spmv_chebyshev_solve: the handle was not set up (spmv_chebyshev_setup)");
    if (A->nrow == 0) return SPMV_OK;
    return cheby_run(ctx, A, r, z, /*add=*/false, /*r_is_t=*/false);
}

// x += M^-1 (b - A x)
int cheby_smooth(spmv_ctx* ctx, const spmv_mat* A, const double* b, double* x)
{
    const cheby_state* st = A->cheby;
    if (!st) SPMV_FAIL(SPMV_ERR_INVALID, "spmv_chebyshev: the handle was not set up (spmv_chebyshev_setup)");
    const int64_t n = A->nrow;
    if (n == 0) return SPMV_OK;
    apply_extra over;
    over.overwrite = true;
    SPMV_TRY(mat_apply_ex(ctx, A, x, st->w, over));
    if (wide_ok(b, n))
        hipLaunchKernelGGL(cheby_resid_kernel<true>, dim3(pair_grid(n)), dim3(kBlock), 0, ctx->stream, n, b, (const double*)st->w, st->t);
    else
        hipLaunchKernelGGL(cheby_resid_kernel<false>, dim3(stream_grid(n)), dim3(kBlock), 0, ctx->stream, n, b, (const double*)st->w, st->t);
    return cheby_run(ctx, A, st->t, x, /*add=*/true, /*r_is_t=*/true);
}

// ---- Lanczos: the host side ------------------------------------------------------------------------------------------------------
int cheby_lanczos(spmv_ctx* ctx, const spmv_mat* A, int scaled, int steps, uint64_t seed, double* ritz_min, double* ritz_max, double* alpha,
                  double* beta, int32_t* steps_done)
{
    const char* const who = "spmv_lanczos";
    const int64_t     n   = A->nrow;
    *ritz_min = *ritz_max = 0.0;
    *steps_done           = 0;
    if (n == 0) return SPMV_OK;
    hipStream_t    s = ctx->stream;
    double *       p, *q, *w, *sv = nullptr, *part;
    LanczosState*  st = nullptr;
    SolveWorkspace ws(ctx, who);
    ws.piece(p, n);
    ws.piece(q, n);
    ws.piece(w, n);
    if (scaled) ws.piece(sv, n);
    ws.piece(part, kMaxGrid);
    SPMV_TRY(ws.allocate((void**)&st, sizeof(LanczosState)));
    if (scaled) SPMV_TRY(jacobi_inverse_diagonal(ctx, A, sv, who, "the Jacobi scaling"));
    SPMV_TRY(hip_step(hipMemsetAsync(p, 0, sizeof(double) * (size_t)n, s), who, "clearing u_-1"));
    SPMV_TRY(gen_vec_uniform(ctx, q, n, 0, seed));
    const int grid = pair_grid(n), grid1 = stream_grid(n);
    if (scaled)
        hipLaunchKernelGGL(lanczos_start_kernel<true>, dim3(grid1), dim3(kBlock), 0, s, n, q, (const double*)sv, part, st);
    else
        hipLaunchKernelGGL(lanczos_start_kernel<false>, dim3(grid1), dim3(kBlock), 0, s, n, q, (const double*)sv, part, st);
    apply_extra over;
    over.overwrite = true;
    for (int j = 0; j < steps; ++j)
    {
        SPMV_TRY(mat_apply_ex(ctx, A, q, w, over));
        hipLaunchKernelGGL(lanczos_alpha_kernel, dim3(grid), dim3(kBlock), 0, s, n, j, q, w, part, st);
        if (scaled)
            hipLaunchKernelGGL(lanczos_update_kernel<true>, dim3(grid), dim3(kBlock), 0, s, n, j, p, (const double*)q, (const double*)w,
                               (const double*)sv, part, st);
        else
            hipLaunchKernelGGL(lanczos_update_kernel<false>, dim3(grid), dim3(kBlock), 0, s, n, j, p, (const double*)q, (const double*)w,
                               (const double*)sv, part, st);
        std::swap(p, q);  // y, the next u_j before its normalisation, lies where u_{j-1} was
    }
    SPMV_TRY(hip_step(hipGetLastError(), who, "a launch of the run"));
    LanczosState h;
    SPMV_TRY(read_scalars(ctx, &h, st, sizeof(LanczosState), who));
    SPMV_REQUIRE(!h.bad, "%s: a diagonal entry is not positive: the scaled operator diag(sqrt s) A diag(sqrt s) needs every a_ii > 0", who);
    const int m = h.done;
    bool      finite = m >= 1 && m <= steps;
    for (int j = 0; j < m && finite; ++j) finite = std::isfinite(h.alpha[j]) && std::isfinite(h.beta[j]);
    SPMV_REQUIRE(finite, "%s: the coefficients are not finite (non-finite numbers in the matrix, or a zero start vector)", who);
    *steps_done = m;
    for (int j = 0; j < m; ++j)
    {
        if (alpha) alpha[j] = h.alpha[j];
        if (beta) beta[j] = h.beta[j];
    }
    *ritz_min = tridiagonal_eigenvalue(h.alpha, h.beta, m, 0);
    *ritz_max = tridiagonal_eigenvalue(h.alpha, h.beta, m, m - 1);
    return SPMV_OK;  // (the workspace waits for the stream and frees)
}
}  // namespace spmv
