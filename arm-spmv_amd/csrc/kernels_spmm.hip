// kernels_spmm.hip — Y += A*X for k vectors at once (spmv_apply_multi), CSR and ELL, on CDNA4 (gfx950).
//
// X (ncol x k) and Y (nrow x k) are ROW-MAJOR: entry (j, c) at j*k + c.  The gather of one matrix entry then fetches the 8*k
// contiguous bytes X[col, 0..k) instead of one 8-byte word, and the 12 bytes of the entry (value + column) are read once for
// all k columns.  Algorithmic bytes per product: 12*nnz + 4*(nrow+1) + 8*ncol*k + 16*nrow*k (8*nrow*k with overwrite).
//
// Order of the additions (the contract of spmv_apply_multi): column c of Y is bit-identical to the oracle's fma flavour on
// column c of X - CSR: a row's sum from 0.0, left to right with fma, then y += sum (y = sum with overwrite); ELL: the
// accumulator starts at y (0.0 with overwrite) and takes the slots in order, padding included (0.0 * X[0, c]).  So ONE lane
// holds one (row, column) chain, in entry order; what is parallel is the rows and the columns, never a row's entries.
//
// Shape: lane t of a row's group owns column c0 + t of the column tile [c0, c0 + T), T = 1, 2, 4, ..., 64 (the next power of two
// >= k, at most 16 by default).  k > T: ceil(k / T) column tiles, one workgroup per (row block, tile), the tiles of a row block in
// consecutive workgroup ids so that the re-reads of its entries come from the caches; lanes beyond k are masked.
//   csr_spmm_kernel<T, NT>   a group of G = max(T, 8) lanes owns one row (G - T lanes only load for k < 8): the group reads the
//                            row's entries coalesced, 32 or G per chunk (lane t entries j0 + t, j0 + t + G, ...), passes them along
//                            the group with ds_bpermute, and each lane issues the gathers X[col * k + c0 + t] of 32 entries (one
//                            contiguous 8*T-byte piece per group and entry) before their 32 fmas: 32 gathers per lane in flight,
//                            the order unchanged.  y is read ahead of the row's loads.
//   ell_spmm_kernel<T, NT>   T lanes per row over the column-major slots: the group reads a slot's (value, column) of its row at
//                            one address (a broadcast); the 64/T rows of a wavefront are consecutive, so its loads are coalesced;
//                            16 slots' loads, then their 16 gathers, then their fmas.
// NT: the matrix is read with non-temporal loads when it is read once (one tile); with several tiles plain loads, so that the
// other tiles' workgroups find the lines in the caches.
//
// The product reads only the handle's own arrays (a, b, v): not the copies, layouts or plan AUTO made for spmv_apply.
#include <cstdlib>

#include "common.hpp"
#include "wave.hpp"

namespace spmv
{
namespace
{
constexpr int kSpmmCsrBatch = 32;      // CSR: entries whose gathers are issued before their fmas
constexpr int kSpmmEllBatch = 16;      // ELL: slots whose loads and gathers are issued before their fmas
constexpr int kSpmmMaxGrid  = 1 << 20;  // workgroups per launch; larger products loop (nrow * T can pass 2^32 lanes)

template <typename V>
__device__ __forceinline__ V load_matrix(const V* p, bool nt)
{
    return nt ? load_stream(p) : *p;
}

// lanes per row of the CSR kernel: at least 8, so that a row's entries are loaded 64 contiguous bytes at a time also for k < 8
// (lanes t >= T then only load)
template <int T>
constexpr int csr_group() { return T > 8 ? T : 8; }

template <int T, bool NT>
__global__ __launch_bounds__(kBlock) void csr_spmm_kernel(int nrow, int k, int ntiles, int64_t nvblocks,
                                                          const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                          const double* __restrict__ val, const double* __restrict__ X,
                                                          double* __restrict__ Y, int overwrite)
{
    constexpr int G    = csr_group<T>();                // lanes per row
    constexpr int ROWS = kBlock / G;                    // rows per workgroup
    constexpr int B    = kSpmmCsrBatch;                 // entries whose gathers are in flight together
    constexpr int U    = G > B ? G : B;                 // entries per chunk
    constexpr int Q    = U / G;                         // entries each lane loads per chunk
    const int     t    = threadIdx.x % G;
    const int     base = lane_id() & ~(G - 1);          // the group's first lane in the wavefront
    for (int64_t vb = blockIdx.x; vb < nvblocks; vb += gridDim.x)
    {
        const int64_t tile = vb % ntiles;
        const int64_t row  = (vb / ntiles) * ROWS + threadIdx.x / G;
        if (row >= nrow) continue;  // a whole group leaves together: G divides the wavefront
        const int  c    = (int)(tile * T) + t;
        const bool live = t < T && c < k;
        double*    yp   = Y + row * (int64_t)k + c;
        const double y0 = (live && !overwrite) ? *yp : 0.0;  // issued ahead of the row's loads
        const int  beg  = row_ptr[row];
        const int  end  = row_ptr[row + 1];
        double     sum  = 0.0;
        for (int j0 = beg; j0 < end; j0 += U)
        {
            const int n = min(U, end - j0);  // uniform over the group
            int       cl[Q];
            double    vl[Q];
#pragma unroll
            for (int q = 0; q < Q; ++q)
            {
                const int j = j0 + q * G + t;
                cl[q]       = j < end ? load_matrix(col + j, NT) : 0;
                vl[q]       = j < end ? load_matrix(val + j, NT) : 0.0;
            }
#pragma unroll
            for (int b = 0; b < U; b += B)
            {
                if (b >= n) break;
                double xg[B];
#pragma unroll
                for (int u = 0; u < B; ++u)
                {
                    const int e  = b + u;  // entry j0 + e of the row: register e / G of lane e % G
                    const int cj = bpermute(cl[e / G], base + e % G);
                    xg[u]        = (live && e < n) ? X[(int64_t)cj * k + c] : 0.0;
                }
#pragma unroll
                for (int u = 0; u < B; ++u)
                {
                    const double v = bpermute(vl[(b + u) / G], base + (b + u) % G);
                    if (b + u < n) sum = fma(v, xg[u], sum);
                }
            }
        }
        if (live) *yp = overwrite ? sum : y0 + sum;
    }
}

template <int T, bool NT>
__global__ __launch_bounds__(kBlock) void ell_spmm_kernel(int nrow, int slots, int k, int ntiles, int64_t nvblocks,
                                                          const int32_t* __restrict__ col, const double* __restrict__ val,
                                                          const double* __restrict__ X, double* __restrict__ Y, int overwrite)
{
    constexpr int ROWS = kBlock / T;
    const int     t    = threadIdx.x % T;
    for (int64_t vb = blockIdx.x; vb < nvblocks; vb += gridDim.x)
    {
        const int64_t tile = vb % ntiles;
        const int64_t row  = (vb / ntiles) * ROWS + threadIdx.x / T;
        if (row >= nrow) continue;
        const int  c    = (int)(tile * T) + t;
        const bool live = c < k;
        double*    yp   = Y + row * (int64_t)k + c;
        double     acc  = (live && !overwrite) ? *yp : 0.0;
        const size_t stride = (size_t)nrow;
        size_t       at     = (size_t)row;  // (row, slot s) at row + s * nrow
        int          s      = 0;
        for (; s + kSpmmEllBatch <= slots; s += kSpmmEllBatch, at += kSpmmEllBatch * stride)
        {
            int    cj[kSpmmEllBatch];
            double v[kSpmmEllBatch], xg[kSpmmEllBatch];
#pragma unroll
            for (int u = 0; u < kSpmmEllBatch; ++u)
            {
                cj[u] = load_matrix(col + at + u * stride, NT);
                v[u]  = load_matrix(val + at + u * stride, NT);
            }
#pragma unroll
            for (int u = 0; u < kSpmmEllBatch; ++u) xg[u] = live ? X[(int64_t)cj[u] * k + c] : 0.0;
#pragma unroll
            for (int u = 0; u < kSpmmEllBatch; ++u) acc = fma(v[u], xg[u], acc);
        }
        for (; s < slots; ++s, at += stride)
        {
            const int    cj = load_matrix(col + at, NT);
            const double vj = load_matrix(val + at, NT);
            acc             = fma(vj, live ? X[(int64_t)cj * k + c] : 0.0, acc);
        }
        if (live) *yp = acc;
    }
}

// lanes per group: the next power of two >= k, at most 16; SPMV_SPMM_LANES=32 or 64 raises the cap so that one group of a row
// covers up to that many columns instead of a further column tile (an A/B switch for tools/bench_spmm.py).  Read once per process;
// any other value leaves the cap at 16.
int spmm_lane_cap()
{
    static const int cap = [] {
        const char* e = getenv("SPMV_SPMM_LANES");
        const int   v = e ? atoi(e) : 16;
        return v == 32 || v == 64 ? v : 16;
    }();
    return cap;
}

int spmm_lanes(int32_t k)
{
    const int cap = spmm_lane_cap();
    int       t   = 1;
    while (t < k && t < cap) t *= 2;
    return t;
}

struct spmm_grid
{
    int     ntiles;
    int64_t nvblocks;
    dim3    grid;
};
spmm_grid spmm_shape(int32_t nrow, int32_t k, int T, int rows_per_block)
{
    spmm_grid g;
    g.ntiles   = (int)ceil_div(k, T);
    g.nvblocks = ceil_div(nrow, rows_per_block) * g.ntiles;
    g.grid     = dim3((unsigned)std::min<int64_t>(g.nvblocks, kSpmmMaxGrid));
    return g;
}

template <int T>
int launch_csr(spmv_ctx* ctx, const spmv_mat* A, int32_t k, const double* X, double* Y, int overwrite)
{
    const spmm_grid g = spmm_shape(A->nrow, k, T, kBlock / csr_group<T>());
    if (g.ntiles == 1)
        hipLaunchKernelGGL((csr_spmm_kernel<T, true>), g.grid, dim3(kBlock), 0, ctx->stream, A->nrow, k, g.ntiles, g.nvblocks,
                           A->a, A->b, A->v, X, Y, overwrite);
    else
        hipLaunchKernelGGL((csr_spmm_kernel<T, false>), g.grid, dim3(kBlock), 0, ctx->stream, A->nrow, k, g.ntiles, g.nvblocks,
                           A->a, A->b, A->v, X, Y, overwrite);
    SPMV_HIP(hipGetLastError());
    return SPMV_OK;
}

template <int T>
int launch_ell(spmv_ctx* ctx, const spmv_mat* A, int32_t k, const double* X, double* Y, int overwrite)
{
    const spmm_grid g = spmm_shape(A->nrow, k, T, kBlock / T);
    if (g.ntiles == 1)
        hipLaunchKernelGGL((ell_spmm_kernel<T, true>), g.grid, dim3(kBlock), 0, ctx->stream, A->nrow, A->k, k, g.ntiles, g.nvblocks,
                           A->b, A->v, X, Y, overwrite);
    else
        hipLaunchKernelGGL((ell_spmm_kernel<T, false>), g.grid, dim3(kBlock), 0, ctx->stream, A->nrow, A->k, k, g.ntiles,
                           g.nvblocks, A->b, A->v, X, Y, overwrite);
    SPMV_HIP(hipGetLastError());
    return SPMV_OK;
}

}  // namespace

int spmm_apply(spmv_ctx* ctx, const spmv_mat* A, int32_t k, const double* X, double* Y, bool overwrite)
{
    if (A->nrow == 0) return SPMV_OK;
    const int  T   = spmm_lanes(k);
    const int  ow  = overwrite ? 1 : 0;
    const bool csr = A->format == SPMV_FMT_CSR;
    if (!csr && A->format != SPMV_FMT_ELL)
        SPMV_FAIL(SPMV_ERR_UNSUPPORTED, "spmv_apply_multi: CSR and ELL handles only (format %d)", A->format);
    switch (T)
    {
        case 1: return csr ? launch_csr<1>(ctx, A, k, X, Y, ow) : launch_ell<1>(ctx, A, k, X, Y, ow);
        case 2: return csr ? launch_csr<2>(ctx, A, k, X, Y, ow) : launch_ell<2>(ctx, A, k, X, Y, ow);
        case 4: return csr ? launch_csr<4>(ctx, A, k, X, Y, ow) : launch_ell<4>(ctx, A, k, X, Y, ow);
        case 8: return csr ? launch_csr<8>(ctx, A, k, X, Y, ow) : launch_ell<8>(ctx, A, k, X, Y, ow);
        case 16: return csr ? launch_csr<16>(ctx, A, k, X, Y, ow) : launch_ell<16>(ctx, A, k, X, Y, ow);
        case 32: return csr ? launch_csr<32>(ctx, A, k, X, Y, ow) : launch_ell<32>(ctx, A, k, X, Y, ow);
        default: return csr ? launch_csr<64>(ctx, A, k, X, Y, ow) : launch_ell<64>(ctx, A, k, X, Y, ow);
    }
}
}  // namespace spmv
