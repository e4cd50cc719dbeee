// solver_gmres.hip — spmv_gmres: A x = b for a square, not necessarily symmetric A by restarted GMRES(m), device-resident, on CDNA4 (gfx950).
//
// A is any handle the forward product (mat_apply_ex) takes: every format; a shard where it holds a square matrix.  The product is
// not changed and gets no kernel here.  One product and one preconditioner application per iteration (BiCGSTAB: two of each); what
// is new is the orthogonalisation of each product against the basis so far.  The recurrence is right-preconditioned GMRES with
// classical Gram-Schmidt run twice, exactly as it runs (every vector has nrow entries; m = restart):
//
//   r = b - A x;  beta = ||r||;                                   (a cycle starts)   v_0 = r / beta;  g = (beta, 0, ...)
//   for j = 0 .. m-1:
//       z = M^-1 v_j;  w = A z;  h = 0
//       twice:  c_i = v_i . w  for i = 0..j, all against the same w;   w -= sum_i c_i v_i (ascending i);   h_i += c_i
//       h_{j+1} = ||w||;  v_{j+1} = w / h_{j+1}
//       rotations 0..j-1 applied to h;  d = sqrt(h_j^2 + h_{j+1}^2);  (cs_j, sn_j) = (h_j, h_{j+1}) / d;  h_j = d
//       g_{j+1} = -sn_j g_j;  g_j = cs_j g_j;      the recurrence's residual is |g_{j+1}|
//   the cycle ends at j = m, at a stop, at max_iter or when it landed:
//       y = R^-1 g (back substitution, row i: t = g_i, t -= R_ik y_k for ascending k > i, y_i = t / R_ii);
//       x += M^-1 (sum_i y_i v_i) (ascending i);  and if the solve goes on, r = b - A x again
//
// M = I for SPMV_PRECOND_NONE: z is v_j itself, no copy.  M = diag(A) of a CSR handle for SPMV_PRECOND_JACOBI: z = dinv v_{j+1} is
// written by the launch that normalises v_{j+1}, and dinv is fused into the sweep that updates x.  M = L U, the ILU(0) factors of a
// CSR handle (ilu0.hip), for SPMV_PRECOND_ILU0: z = M^-1 v_j is one application (ilu0_apply) in front of the product, and the
// update of x goes through w: w = V y, z = M^-1 w, x += z.  Right preconditioning: r is the residual of A x = b itself.
//
// Why classical Gram-Schmidt twice: the j + 1 dots of one pass are independent of each other, so they are ONE sweep over the basis
// with one grid-wide sum behind it; modified Gram-Schmidt is j + 1 dependent sweeps of one vector with j + 1 grid-wide sums (and
// launches).  One classical pass loses orthogonality like kappa^2; the second brings it back to rounding (Giraud, Langou, Rozloznik
// and van den Eshof 2005: "twice is enough").
//
// Six launches per iteration (ILU(0): and the level launches of one application), column j of a cycle:
//   1  mat_apply_ex               w = A z (overwrite)
//   2  gmres_dots_kernel          c_i = v_i . w, i = 0..j: the basis in tiles of kGmresTile vectors, w read once per tile, the
//                                 tile's accumulators in registers; h_i = c_i
//   3  gmres_update_kernel<false> w -= sum_i c_i v_i
//   4  gmres_dots_kernel          c_i = v_i . w again;  h_i += c_i
//   5  gmres_update_kernel<true>  w -= sum_i c_i v_i;  w.w;  the workgroup with the last ticket does the small problem in one
//                                 thread: h_{j+1}, the j old rotations, the new one, g, the column of R
//   6  gmres_normalise_kernel     v_{j+1} = w / h_{j+1};  z = dinv v_{j+1} (Jacobi).  Not launched behind a cycle's last column.
// Four sweeps over the j + 1 basis vectors per iteration.  The second pass's dots are NOT fused into the first update: v_i . w'
// needs the finished w' of an element and every v_i of that element again, that is j + 1 <= 64 vector pairs held in registers
// across the update - past the tile at once, and a second code path below it.  The bytes per iteration (8-byte words per row):
// 4 (j + 1) basis reads, w read ceil((j + 1) / kGmresTile) times by each dots launch and read and written by each update, and the
// normalisation's 2 (Jacobi 4): 8 (4 (j + 1) + 2 ceil((j + 1) / 8) + 6) bytes per row, 592 at j = 15, on top of the product.
// A cycle's end: gmres_backsolve_kernel (one thread), gmres_xupdate_kernel (one sweep over the columns that stand), and where the
// solve goes on one product, gmres_resid_kernel (r = b - A x into w, r.r, beta, g_0) and the normalisation: v_0 = w / beta.
//
// The small problem stays on the device (GmresState): R, cs, sn, g, y, the column count, the floor, a status word and the ticket.
// The host reads the head of it every check_every iterations, after the last one and behind every restart, and nowhere else.  An
// iteration that starts with |g_j| at or below 1e-14 ||b|| (rounding noise of the recurrence; h_{j+1} = 0, the lucky breakdown,
// among it) or behind a raised status passes quietly: its kernels write nothing.  d at or below 2^-44 times the norm of the new
// column (d = 0 up to the rounding of the j + 1 dots that made the column) with a residual above the floor is the breakdown of a
// singular A whose Krylov space is exhausted; it and anything not finite raise the status word, and x stays the iterate of the
// last completed cycle.  Stagnation is no error.
//
// Every dot product is DETERMINISTIC, by the last-ticket pattern of solver_common.hpp: per-workgroup partial sums per dot in a
// buffer of (m + 2) x kMaxGrid doubles, added in buffer order by the workgroup that stores last.  No atomic adds in arrival order.
//
// Vector kernels: kBlock threads, grid-stride loops over at most kMaxGrid workgroups, 64-bit indices, no scratch.  The basis (m + 1
// vectors), w, z (Jacobi, ILU(0)) and dinv (Jacobi) are 256-byte aligned pieces of one allocation, (m + 2 .. m + 4) nrow doubles,
// and go in 16-byte accesses (two elements per lane, an odd last element by one extra lane); the caller's x (the update) and b (the
// residual) go in 16-byte accesses where they are 16-byte aligned and have two entries or more, in 8-byte accesses otherwise (WIDE).
//
// Not part of the reference's API, so there is no reference output.  What pins it: every iterate x_k and the residual against
// this recurrence in extended precision (tests/gmres_ref.py, tests/test_gpu_gmres.py).
#include <cmath>
#include <cstddef>

#include "common.hpp"
#include "solver_common.hpp"
#include "solver_host.hpp"
#include "wave.hpp"

namespace spmv
{
namespace
{
constexpr int kGmresMaxRestart = 64;  // m <= 64: the small problem's arrays are sized for it
constexpr int kGmresTile       = 8;   // basis vectors per tile of the dots kernel: 8 accumulators and 8 loaded pairs in registers

enum : int32_t
{
    kGmresD         = 1,  // d = sqrt(h_j^2 + h_{j+1}^2) is 0 (up to rounding) with a residual above the floor
    kGmresNotFinite = 2   // h or g is not finite
};

struct GmresState
{
    // the head: what the host reads at its looks
    double   res;     // |g_{ncols}|: the recurrence's residual norm; behind gmres_resid_kernel ||b - A x||
    double   bb;      // b.b
    double   floor;   // 1e-14 ||b||: at or below it the residual is rounding noise
    double   hnext;   // what the normalisation divides w by: beta at a cycle's start, h_{j+1} behind column j
    int32_t  ncols;   // columns of the current cycle that stand
    int32_t  status;  // 0, or the first breakdown (kGmres*)
    uint32_t ticket;  // workgroups of the current launch that have stored their partial sums
    int32_t  pad;
    // the small problem
    double c[kGmresMaxRestart];      // the dots of the current Gram-Schmidt pass
    double h[kGmresMaxRestart + 1];  // the new column of the Hessenberg matrix
    double cs[kGmresMaxRestart];
    double sn[kGmresMaxRestart];
    double g[kGmresMaxRestart + 1];
    double y[kGmresMaxRestart];
    double R[kGmresMaxRestart * kGmresMaxRestart];  // column j at R + j * kGmresMaxRestart, rows 0..j
};
constexpr size_t kGmresHeadBytes = offsetof(GmresState, c);

// an iteration takes its steps only from a residual above the floor and with no breakdown behind it (uniform over a grid: no
// launch that asks writes what it reads here before its last ticket)
static __device__ __forceinline__ bool gmres_live(const GmresState* s) { return s->status == 0 && s->res > s->floor; }

// w = b - w (w = A x on entry);  r.r, and b.b (INIT);  the workgroup with the last ticket starts the cycle: beta, g_0, no columns.
// WIDE: b is 16-byte aligned
template <bool WIDE, bool INIT>
__global__ __launch_bounds__(kBlock) void gmres_resid_kernel(int64_t n, const double* __restrict__ b, double* __restrict__ w,
                                                             double* __restrict__ part, GmresState* __restrict__ s)
{
    double acc[2] = {0.0, 0.0};  // r.r, b.b
    if constexpr (WIDE)
    {
        const int64_t npairs = n / 2;
        for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < npairs; i += (int64_t)gridDim.x * kBlock)
        {
            const f64x2 bv = ((const f64x2*)b)[i], qv = ((const f64x2*)w)[i];
            const f64x2 rv = f64x2{bv[0] - qv[0], bv[1] - qv[1]};
            ((f64x2*)w)[i] = rv;
#pragma unroll
            for (int e = 0; e < 2; ++e)
            {
                acc[0] = fma(rv[e], rv[e], acc[0]);
                if constexpr (INIT) acc[1] = fma(bv[e], bv[e], acc[1]);
            }
        }
    }
    // WIDE: the odd last element, by one lane;  otherwise every element, one per lane
    const bool    lead  = blockIdx.x == 0 && threadIdx.x == 0;
    const int64_t first = WIDE ? (((n & 1) && lead) ? n - 1 : n) : (int64_t)blockIdx.x * kBlock + threadIdx.x;
    for (int64_t i = first; i < n; i += (int64_t)gridDim.x * kBlock)
    {
        const double bi = b[i], ri = bi - w[i];
        w[i]   = ri;
        acc[0] = fma(ri, ri, acc[0]);
        if constexpr (INIT) acc[1] = fma(bi, bi, acc[1]);
    }
    double total[2];
    if (!grid_totals<2>(acc, part, &s->ticket, total)) return;
    if (threadIdx.x == 0)
    {
        const double beta = sqrt(total[0]);
        if constexpr (INIT)
        {
            s->bb    = total[1];
            s->floor = 1e-14 * sqrt(total[1]);
        }
        s->res    = beta;
        s->hnext  = beta;
        s->g[0]   = beta;
        s->ncols  = 0;
        s->ticket = 0;
    }
}

// v_j = w / hnext for j = the columns that stand (v_0 = r / beta behind gmres_resid_kernel, v_{j+1} = w / h_{j+1} behind a column);
// z = dinv v_j (PRE).  Nothing where the residual is at the floor: no vector is divided by a norm that is rounding noise
template <bool PRE>
__global__ __launch_bounds__(kBlock) void gmres_normalise_kernel(int64_t n, int64_t vstride, double* __restrict__ V, const double* __restrict__ w,
                                                                 const double* __restrict__ dinv, double* __restrict__ z,
                                                                 const GmresState* __restrict__ s)
{
    if (!gmres_live(s)) return;
    const double  hn = s->hnext;
    double*       v  = V + (int64_t)s->ncols * vstride;
    const int64_t npairs = n / 2;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < npairs; i += (int64_t)gridDim.x * kBlock)
    {
        const f64x2 wv = ((const f64x2*)w)[i];
        const f64x2 vv = f64x2{wv[0] / hn, wv[1] / hn};
        ((f64x2*)v)[i] = vv;
        if constexpr (PRE)
        {
            const f64x2 dv = ((const f64x2*)dinv)[i];
            ((f64x2*)z)[i] = f64x2{dv[0] * vv[0], dv[1] * vv[1]};
        }
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0)
    {
        const int64_t i  = n - 1;
        const double  vi = w[i] / hn;
        v[i]             = vi;
        if constexpr (PRE) z[i] = dinv[i] * vi;
    }
}

// c_i = v_i . w for i = 0 .. ncols, all against the same w: the basis in tiles of kGmresTile vectors, w read once per tile, the
// tile's accumulators in registers (every index into acc is a compile-time one).  The workgroup with the last ticket adds each
// dot's partial sums in buffer order and writes c_i and h_i = c_i (first) or h_i += c_i
__global__ __launch_bounds__(kBlock) void gmres_dots_kernel(int64_t n, int64_t vstride, const double* __restrict__ V, const double* __restrict__ w,
                                                            int first, double* __restrict__ part, GmresState* __restrict__ s)
{
    __shared__ double s_part[kBlock / kWave];
    if (!gmres_live(s)) return;
    const int     nv     = s->ncols + 1;
    const int64_t npairs = n / 2, stride = (int64_t)gridDim.x * kBlock;
    const bool    tail   = (n & 1) && blockIdx.x == 0 && threadIdx.x == 0;
    for (int t0 = 0; t0 < nv; t0 += kGmresTile)
    {
        const int     cnt = min(kGmresTile, nv - t0);
        const double* vt  = V + (int64_t)t0 * vstride;
        double        acc[kGmresTile];
#pragma unroll
        for (int q = 0; q < kGmresTile; ++q) acc[q] = 0.0;
        // (a ragged last tile reads its last vector again in the places past it - lines the same lanes have just loaded - and
        // stores no sum for them: one loop without a predicate around its loads)
        for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < npairs; i += stride)
        {
            const f64x2 wv = ((const f64x2*)w)[i];
            f64x2       vv[kGmresTile];
#pragma unroll
            for (int q = 0; q < kGmresTile; ++q) vv[q] = ((const f64x2*)(vt + (int64_t)min(q, cnt - 1) * vstride))[i];
#pragma unroll
            for (int q = 0; q < kGmresTile; ++q) acc[q] = fma(vv[q][1], wv[1], fma(vv[q][0], wv[0], acc[q]));
        }
        if (tail)
        {
            const double wi = w[n - 1];
#pragma unroll
            for (int q = 0; q < kGmresTile; ++q)
                acc[q] = fma(vt[(int64_t)min(q, cnt - 1) * vstride + n - 1], wi, acc[q]);
        }
#pragma unroll
        for (int q = 0; q < kGmresTile; ++q)
            if (q < cnt)  // (uniform over the workgroup)
            {
                const double t = block_sum_all(acc[q], s_part);
                if (threadIdx.x == 0) part[(int64_t)(t0 + q) * gridDim.x + blockIdx.x] = t;
            }
    }
    if (!took_last_ticket(&s->ticket)) return;
    for (int q = 0; q < nv; ++q)
    {
        double a = 0.0;
        for (int g = threadIdx.x; g < (int)gridDim.x; g += kBlock) a += partial_sum_load(part + (int64_t)q * gridDim.x + g);
        const double t = block_sum_all(a, s_part);
        if (threadIdx.x == 0)
        {
            s->c[q] = t;
            s->h[q] = first ? t : s->h[q] + t;
        }
    }
    if (threadIdx.x == 0) s->ticket = 0;
}

// w -= sum_i c_i v_i, ascending i = 0 .. ncols.  NORM: w.w of the new w as well, and the workgroup with the last ticket does the
// small problem in one thread: h_{j+1} = ||w||, the j old rotations applied to the new column, the new rotation, g, column j of R
template <bool NORM>
__global__ __launch_bounds__(kBlock) void gmres_update_kernel(int64_t n, int64_t vstride, const double* __restrict__ V, double* __restrict__ w,
                                                              double* __restrict__ part, GmresState* __restrict__ s)
{
    __shared__ double s_c[kGmresMaxRestart];
    if (!gmres_live(s)) return;
    const int nv = s->ncols + 1;
    if ((int)threadIdx.x < nv) s_c[threadIdx.x] = s->c[threadIdx.x];
    __syncthreads();
    const int64_t npairs = n / 2;
    double        acc[1] = {0.0};
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < npairs; i += (int64_t)gridDim.x * kBlock)
    {
        f64x2 wv = ((const f64x2*)w)[i];
#pragma unroll 4
        for (int q = 0; q < nv; ++q)
        {
            const f64x2  vv = ((const f64x2*)(V + (int64_t)q * vstride))[i];
            const double c  = s_c[q];
            wv[0]           = fma(-c, vv[0], wv[0]);
            wv[1]           = fma(-c, vv[1], wv[1]);
        }
        ((f64x2*)w)[i] = wv;
        if constexpr (NORM) acc[0] = fma(wv[1], wv[1], fma(wv[0], wv[0], acc[0]));
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0)
    {
        double wi = w[n - 1];
        for (int q = 0; q < nv; ++q) wi = fma(-s_c[q], V[(int64_t)q * vstride + n - 1], wi);
        w[n - 1] = wi;
        if constexpr (NORM) acc[0] = fma(wi, wi, acc[0]);
    }
    if constexpr (NORM)
    {
        double total[1];
        if (!grid_totals<1>(acc, part, &s->ticket, total)) return;
        if (threadIdx.x == 0)
        {
            const int    j   = nv - 1;
            const double hj1 = sqrt(total[0]);
            double       sq  = total[0];  // the squared norm of the new column: what "d = 0" is measured against
            for (int i = 0; i <= j; ++i) sq = fma(s->h[i], s->h[i], sq);
            for (int i = 0; i < j; ++i)
            {
                const double a = s->h[i], c = s->h[i + 1], cs = s->cs[i], sn = s->sn[i];
                s->h[i]     = cs * a + sn * c;
                s->h[i + 1] = cs * c - sn * a;
            }
            const double hj = s->h[j], d = sqrt(hj * hj + hj1 * hj1), gj = s->g[j];
            if (!isfinite(d) || !isfinite(sq))
                s->status = kGmresNotFinite;
            else if (!(d > 0x1p-44 * sqrt(sq)))
                s->status = kGmresD;
            else
            {
                const double cs = hj / d, sn = hj1 / d;
                double*      Rj = s->R + (int64_t)j * kGmresMaxRestart;
                for (int i = 0; i < j; ++i) Rj[i] = s->h[i];
                Rj[j]       = d;
                s->cs[j]    = cs;
                s->sn[j]    = sn;
                s->g[j + 1] = -sn * gj;
                s->g[j]     = cs * gj;
                s->hnext    = hj1;
                s->ncols    = j + 1;
                s->res      = fabs(sn * gj);
                if (!isfinite(s->res)) s->status = kGmresNotFinite;
            }
            s->ticket = 0;
        }
    }
}

// y = R^-1 g over the columns that stand, by one thread: row i from the last one up, t = g_i, t -= R_ik y_k for ascending k > i
__global__ void gmres_backsolve_kernel(GmresState* __restrict__ s)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const int nc = s->ncols;
    for (int i = nc - 1; i >= 0; --i)
    {
        double t = s->g[i];
        for (int k = i + 1; k < nc; ++k) t = fma(-s->R[(int64_t)k * kGmresMaxRestart + i], s->y[k], t);
        s->y[i] = t / s->R[(int64_t)i * kGmresMaxRestart + i];
    }
}

// u = sum_i y_i v_i over the columns that stand, ascending i.  MODE 0: x += u;  1: x += dinv u (Jacobi);  2: out = u (ILU(0): the
// work vector M^-1 is applied to; zeros where no column stands).  WIDE: out (x) is 16-byte aligned
template <bool WIDE, int MODE>
__global__ __launch_bounds__(kBlock) void gmres_xupdate_kernel(int64_t n, int64_t vstride, const double* __restrict__ V,
                                                               const double* __restrict__ dinv, double* __restrict__ out,
                                                               const GmresState* __restrict__ s)
{
    __shared__ double s_y[kGmresMaxRestart];
    const int nc = s->ncols;
    if (nc == 0 && MODE != 2) return;
    if ((int)threadIdx.x < nc) s_y[threadIdx.x] = s->y[threadIdx.x];
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * kBlock, first = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if constexpr (WIDE)
    {
        const int64_t npairs = n / 2;
        for (int64_t i = first; i < npairs; i += stride)
        {
            f64x2 u = f64x2{0.0, 0.0};
            if (nc > 0)
            {
                const f64x2 v0 = ((const f64x2*)V)[i];
                u              = f64x2{s_y[0] * v0[0], s_y[0] * v0[1]};
            }
#pragma unroll 4
            for (int q = 1; q < nc; ++q)
            {
                const f64x2  vv = ((const f64x2*)(V + (int64_t)q * vstride))[i];
                const double yq = s_y[q];
                u[0]            = fma(yq, vv[0], u[0]);
                u[1]            = fma(yq, vv[1], u[1]);
            }
            if constexpr (MODE == 2)
                ((f64x2*)out)[i] = u;
            else
            {
                f64x2 xv = ((const f64x2*)out)[i];
                if constexpr (MODE == 1)
                {
                    const f64x2 dv = ((const f64x2*)dinv)[i];
                    xv[0] += dv[0] * u[0];
                    xv[1] += dv[1] * u[1];
                }
                else
                {
                    xv[0] += u[0];
                    xv[1] += u[1];
                }
                ((f64x2*)out)[i] = xv;
            }
        }
    }
    // WIDE: the odd last element, by one lane;  otherwise every element, one per lane
    const bool    lead = blockIdx.x == 0 && threadIdx.x == 0;
    const int64_t from = WIDE ? (((n & 1) && lead) ? n - 1 : n) : first;
    for (int64_t i = from; i < n; i += stride)
    {
        double u = nc > 0 ? s_y[0] * V[i] : 0.0;
        for (int q = 1; q < nc; ++q) u = fma(s_y[q], V[(int64_t)q * vstride + i], u);
        if constexpr (MODE == 2)
            out[i] = u;
        else if constexpr (MODE == 1)
            out[i] += dinv[i] * u;
        else
            out[i] += u;
    }
}

// x += z (ILU(0): z = M^-1 (V y)).  WIDE: x is 16-byte aligned
template <bool WIDE>
__global__ __launch_bounds__(kBlock) void gmres_xadd_kernel(int64_t n, const double* __restrict__ z, double* __restrict__ x)
{
    const int64_t stride = (int64_t)gridDim.x * kBlock, first = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if constexpr (WIDE)
    {
        const int64_t npairs = n / 2;
        for (int64_t i = first; i < npairs; i += stride)
        {
            const f64x2 zv = ((const f64x2*)z)[i];
            f64x2       xv = ((const f64x2*)x)[i];
            xv[0] += zv[0];
            xv[1] += zv[1];
            ((f64x2*)x)[i] = xv;
        }
    }
    const bool    lead = blockIdx.x == 0 && threadIdx.x == 0;
    const int64_t from = WIDE ? (((n & 1) && lead) ? n - 1 : n) : first;
    for (int64_t i = from; i < n; i += stride) x[i] += z[i];
}
}  // namespace

int gmres_solve(spmv_ctx* ctx, const spmv_mat* A, const double* b, double* x, int restart, int max_iter, double rel_tol, int check_every,
                int precond, int* iters, double* rel_resid)
{
    const char* const who = "spmv_gmres";
    const int64_t     n   = A->nrow;
    *iters                = 0;
    *rel_resid            = 0.0;
    if (n == 0) return SPMV_OK;
    const int   m  = restart;
    hipStream_t st = ctx->stream;
    const bool  jacobi = precond == SPMV_PRECOND_JACOBI, by_launches = applied_by_launches(precond);  // (by_launches: the column of precond.hpp's table)
    // the basis (m + 1 vectors, a padded vector apart), w, z (Jacobi, ILU(0)), dinv (Jacobi) and the partial sums of m + 2 quantities
    const size_t   sn = SolveWorkspace::padded((size_t)n);
    double *       V, *w, *z = nullptr, *dinv = nullptr, *part;
    GmresState*    s = nullptr;
    SolveWorkspace ws(ctx, who);
    ws.piece(V, (size_t)(m + 1) * sn);
    ws.piece(w, n);
    if (jacobi || by_launches) ws.piece(z, n);
    if (jacobi) ws.piece(dinv, n);
    ws.piece(part, (size_t)(m + 2) * (size_t)kMaxGrid);
    SPMV_TRY(ws.allocate((void**)&s, sizeof(GmresState)));
    SPMV_TRY(setup_preconditioner(ctx, A, precond, dinv, who));
    const bool  wide_x = wide_ok(x, n), wide_b = wide_ok(b, n);
    const int   grid   = pair_grid(n);
    const int   grid_x = wide_x ? grid : stream_grid(n), grid_b = wide_b ? grid : stream_grid(n);
    const int64_t vs   = (int64_t)sn;
    apply_extra over;
    over.overwrite = true;
    auto normalise = [&]() {
        if (jacobi)
            hipLaunchKernelGGL(gmres_normalise_kernel<true>, dim3(grid), dim3(kBlock), 0, st, n, vs, V, (const double*)w, (const double*)dinv, z,
                               (const GmresState*)s);
        else
            hipLaunchKernelGGL(gmres_normalise_kernel<false>, dim3(grid), dim3(kBlock), 0, st, n, vs, V, (const double*)w, (const double*)dinv, z,
                               (const GmresState*)s);
    };
    // r = b - A x into w, beta, g_0 and v_0: a cycle starts
    auto start_cycle = [&](bool init) -> int {
        SPMV_TRY(mat_apply_ex(ctx, A, x, w, over));
#define SPMV_GMRES_RESID(WIDE, INIT) hipLaunchKernelGGL((gmres_resid_kernel<WIDE, INIT>), dim3(grid_b), dim3(kBlock), 0, st, n, b, w, part, s)
        if (wide_b)
        {
            if (init) SPMV_GMRES_RESID(true, true); else SPMV_GMRES_RESID(true, false);
        }
        else
        {
            if (init) SPMV_GMRES_RESID(false, true); else SPMV_GMRES_RESID(false, false);
        }
#undef SPMV_GMRES_RESID
        normalise();
        return SPMV_OK;
    };
    // column j of the cycle (the host's count: a quiet iteration leaves the device's behind, and every later one of the cycle is
    // quiet too).  last: no later column of this cycle reads v_{j+1}
    auto iteration = [&](int j, bool last) -> int {
        const double* vj = V + (size_t)j * sn;
        if (by_launches) SPMV_TRY(apply_preconditioner(ctx, A, precond, vj, z));
        SPMV_TRY(mat_apply_ex(ctx, A, (jacobi || by_launches) ? (const double*)z : vj, w, over));
        hipLaunchKernelGGL(gmres_dots_kernel, dim3(grid), dim3(kBlock), 0, st, n, vs, (const double*)V, (const double*)w, 1, part, s);
        hipLaunchKernelGGL(gmres_update_kernel<false>, dim3(grid), dim3(kBlock), 0, st, n, vs, (const double*)V, w, part, s);
        hipLaunchKernelGGL(gmres_dots_kernel, dim3(grid), dim3(kBlock), 0, st, n, vs, (const double*)V, (const double*)w, 0, part, s);
        hipLaunchKernelGGL(gmres_update_kernel<true>, dim3(grid), dim3(kBlock), 0, st, n, vs, (const double*)V, w, part, s);
        if (!last) normalise();
        return SPMV_OK;
    };
    // y = R^-1 g;  x += M^-1 (V y) over the columns that stand
    auto end_cycle = [&]() -> int {
        hipLaunchKernelGGL(gmres_backsolve_kernel, dim3(1), dim3(kWave), 0, st, s);
#define SPMV_GMRES_XUPDATE(WIDE, MODE, GRID, OUT) \
    hipLaunchKernelGGL((gmres_xupdate_kernel<WIDE, MODE>), dim3(GRID), dim3(kBlock), 0, st, n, vs, (const double*)V, (const double*)dinv, OUT, (const GmresState*)s)
        if (by_launches)
        {
            SPMV_GMRES_XUPDATE(true, 2, grid, w);
            SPMV_TRY(apply_preconditioner(ctx, A, precond, w, z));
            if (wide_x)
                hipLaunchKernelGGL(gmres_xadd_kernel<true>, dim3(grid_x), dim3(kBlock), 0, st, n, (const double*)z, x);
            else
                hipLaunchKernelGGL(gmres_xadd_kernel<false>, dim3(grid_x), dim3(kBlock), 0, st, n, (const double*)z, x);
        }
        else if (jacobi)
        {
            if (wide_x) SPMV_GMRES_XUPDATE(true, 1, grid_x, x); else SPMV_GMRES_XUPDATE(false, 1, grid_x, x);
        }
        else
        {
            if (wide_x) SPMV_GMRES_XUPDATE(true, 0, grid_x, x); else SPMV_GMRES_XUPDATE(false, 0, grid_x, x);
        }
#undef SPMV_GMRES_XUPDATE
        return SPMV_OK;
    };
    GmresState* h = nullptr;  // the head alone is read
    alignas(GmresState) unsigned char h_bytes[kGmresHeadBytes];
    h = reinterpret_cast<GmresState*>(h_bytes);
    auto fetch = [&]() { return read_scalars(ctx, h_bytes, s, kGmresHeadBytes, who); };
    // the basis, w and z lie behind one another from V on; the product of a quiet iteration reads a basis vector or z that no launch
    // of the cycle wrote
    SPMV_TRY(hip_step(hipMemsetAsync(V, 0, sizeof(double) * (size_t)(m + 2 + (jacobi || by_launches ? 1 : 0)) * sn, st), who, "clearing the basis"));
    SPMV_TRY(start_cycle(true));
    SPMV_TRY(fetch());
    const double bb = h->bb;
    double       res = h->res;
    if (!std::isfinite(bb) || !std::isfinite(res))
        SPMV_FAIL(SPMV_ERR_INVALID, "spmv_gmres: b.b = %g, beta = ||b - A x0|| = %g: b, x0 or the matrix hold non-finite numbers", bb, res);
    if (!(bb > 0.0)) return SPMV_OK;  // b = 0: x0 stays, as spmv_cg leaves it
    const double bnorm = sqrt(bb), limit = rel_tol * bnorm, floor_res = 1e-14 * bnorm;
    int          k = 0, rc = SPMV_OK;
    if (res > limit && res > 0.0 && max_iter > 0)
    {
        const int every = std::max(1, check_every);
        int       j     = 0;
        while (k < max_iter)
        {
            if ((rc = iteration(j, j + 1 == m || k + 1 == max_iter)) != SPMV_OK) break;
            ++k;
            ++j;
            bool stop = false, landed = false;
            if (k % every == 0 || k == max_iter)
            {
                if ((rc = fetch()) != SPMV_OK) break;
                res = h->res;
                if (h->status == kGmresNotFinite || !std::isfinite(res))
                {
                    set_error("spmv_gmres: h or g is not finite at or before iteration %d (non-finite numbers in the matrix, or overflow)", k);
                    rc = SPMV_ERR_INVALID;
                    break;
                }
                // (a breakdown behind an iterate that is within the tolerance is no error)
                if (res <= limit || res == 0.0)
                    stop = true;
                else if (h->status != 0)
                {
                    set_error("spmv_gmres: breakdown: d = sqrt(h_j^2 + h_{j+1}^2) is zero at or before iteration %d with a residual to speak of "
                              "(the Krylov space is exhausted and the matrix is singular)", k);
                    rc = SPMV_ERR_INVALID;
                    break;
                }
                else if (k == max_iter)
                    stop = true;
                else
                    landed = res <= floor_res;  // the cycle ends here with the columns that stand
            }
            if (stop)
            {
                rc = end_cycle();
                break;
            }
            if (j == m || landed)
            {
                // a restart: the recomputed ||r|| is what is compared
                if ((rc = end_cycle()) != SPMV_OK || (rc = start_cycle(false)) != SPMV_OK || (rc = fetch()) != SPMV_OK) break;
                j   = 0;
                res = h->res;
                if (!std::isfinite(res))
                {
                    set_error("spmv_gmres: beta = ||b - A x|| is not finite at the restart behind iteration %d (overflow)", k);
                    rc = SPMV_ERR_INVALID;
                    break;
                }
                if (res <= limit || res == 0.0) break;
            }
        }
        if (rc == SPMV_OK) rc = hip_step(hipGetLastError(), who, "a launch of the iteration");
    }
    *iters     = k;
    *rel_resid = res / bnorm;
    return rc;  // (the workspace waits for the stream and frees)
}
}  // namespace spmv
