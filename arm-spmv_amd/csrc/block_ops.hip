// block_ops.hip — the dense tall-skinny arithmetic of a block method, on CDNA4 (gfx950): spmv_block_gram (G = U^T V) and
// spmv_block_combine (Out = S C).  A BLOCK is p columns of n doubles, column-major: column c starts at c * ld, ld >= n; rows n .. ld - 1
// of a column are padding that is never read or written.  1 <= p, q <= kBlockMaxCols = 96 in both.  spmv_lobpcg (solver_lobpcg.hip)
// spends its time outside the products here; every later block method (block CG, deflation, s-step bases) needs the same two.
//
// block_gram_kernel<TP, TQ, SAME>: one sweep over the rows, every column of U and of V read once (SAME: U is V - same start, same ld,
// p = q - and is read once altogether).  A workgroup of 256 threads takes row tiles of kGramRows = 32 rows, tiles blockIdx.x,
// blockIdx.x + gridDim.x, ...  A tile is staged in LDS by coalesced column reads (32 consecutive lanes read 32 consecutive rows of one
// column, 256 bytes) into row-major arrays whose row stride is odd (16 TP + 1 doubles), so that neither the staging stores nor the
// reads below meet a bank twice.  The threads form a 16 x 16 grid (ty, tx); thread (ty, tx) owns the outputs
// G[ty + 16 a][tx + 16 b], a < TP, b < TQ: a register tile of TP x TQ accumulators, every index a compile-time one.  Per staged row
// it reads TP + TQ doubles from LDS (the u's are 4 distinct addresses a wavefront, broadcasts; the v's 16 consecutive doubles) and
// does TP TQ fmas.  TP, TQ in {1, 2, 3, 6}: p <= 16, 32, 48, 96 (the COLUMN TILE is 16: 16, 32 and 48 are its edges and 96 the limit).
// Columns p .. 16 TP - 1 and rows past n are staged as zeros; their accumulators are never stored.  At 6 x 6 that is 36 accumulators
// and 12 operands in double registers, 114 VGPRs of the lane's 512: no scratch, and the 50 KB of LDS let three workgroups share a CU.
// No MFMA: the fp64 matrix rate of this part is its vector rate.
//
// Determinism.  No double is added in arrival order.  An accumulator is ONE chain of fmas over the rows its workgroup visits, in row
// order.  Every workgroup stores its p q sums in part[blockIdx.x * p q + i q + j] and takes a ticket; the workgroup with the last
// ticket (took_last_ticket, solver_common.hpp) adds the workgroups' sums of every output in buffer order and writes G.  The grid is
// min(kGramMaxGrid, tiles): a function of n alone.  Two calls on the same data give the same bits.
// Symmetry.  With U = V, G[i][j] and G[j][i] are the chains fma(u_i, u_j, .) and fma(u_j, u_i, .) over the same rows in the same order,
// and their partial sums are added in the same order: fma is commutative in its factors, so both triangles hold the same bits.
//
// block_combine_kernel<QT>: Out[i, :] = S[i, :] C for every row.  A workgroup takes tiles of 64 rows; wavefront w stages columns
// w, w + 4, ... of the tile in LDS (a lane a row: 512 contiguous bytes a column) and, behind a barrier, computes the output columns
// w QT .. w QT + QT - 1 of its 64 rows: QT accumulators a lane, each 0.0 and then fma(s_ik, c_kj, acc) for k = 0 .. p - 1 in that
// order - the contract: the result is a function of the row alone.  c_kj is uniform over the wavefront and comes through the scalar
// cache.  The barrier stands between the last read of a tile's rows and the first write to them, so Out may be S itself (same start,
// same ld), or more generally a block whose row i lies in S's row i.  QT in {2, 4, 8, 12, 24}: q <= 8, 16, 32, 48, 96.
//
// C reaches the device through the stream from pinned host memory of the context; the staging area is not overwritten before the
// previous copy out of it has completed (an event).  G comes back the same way and the call waits for it.
#include "common.hpp"
#include "solver_common.hpp"
#include "solver_host.hpp"

namespace spmv
{
namespace
{
constexpr int kGramRows    = 32;   // rows of a staged tile
constexpr int kGramSide    = 16;   // the thread grid is 16 x 16; the column tile
constexpr int kGramMaxGrid = 512;  // workgroups: two a CU; the last one adds kGramMaxGrid x p q partial sums
constexpr int kCombRows    = 64;   // rows of a combine tile: a lane a row

template <int TP, int TQ, bool SAME>
__global__ __launch_bounds__(kBlock) void block_gram_kernel(int64_t n, int p, int q, const double* __restrict__ U, int64_t ldu,
                                                            const double* __restrict__ V, int64_t ldv, double* __restrict__ part,
                                                            double* __restrict__ G, uint32_t* __restrict__ ticket)
{
    constexpr int CP = kGramSide * TP + 1, CQ = kGramSide * TQ + 1;
    __shared__ double sU[kGramRows * CP];
    __shared__ double sV[SAME ? 1 : kGramRows * CQ];
    const double* const sVr = SAME ? sU : sV;
    const int           tx = threadIdx.x & (kGramSide - 1), ty = threadIdx.x / kGramSide;
    const int           sr = threadIdx.x & (kGramRows - 1), sc = threadIdx.x / kGramRows;  // the staging role: row, first column
    double              acc[TP][TQ];
#pragma unroll
    for (int a = 0; a < TP; ++a)
#pragma unroll
        for (int b = 0; b < TQ; ++b) acc[a][b] = 0.0;
    const int64_t ntiles = (n + kGramRows - 1) / kGramRows;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x)
    {
        const int64_t row  = tile * kGramRows + sr;
        const bool    live = row < n;
#pragma unroll
        for (int c = sc; c < kGramSide * TP; c += kBlock / kGramRows) sU[sr * CP + c] = (live && c < p) ? U[(int64_t)c * ldu + row] : 0.0;
        if constexpr (!SAME)
        {
#pragma unroll
            for (int c = sc; c < kGramSide * TQ; c += kBlock / kGramRows) sV[sr * CQ + c] = (live && c < q) ? V[(int64_t)c * ldv + row] : 0.0;
        }
        __syncthreads();
#pragma unroll 4
        for (int r = 0; r < kGramRows; ++r)
        {
            double u[TP], v[TQ];
#pragma unroll
            for (int a = 0; a < TP; ++a) u[a] = sU[r * CP + ty + kGramSide * a];
#pragma unroll
            for (int b = 0; b < TQ; ++b) v[b] = sVr[r * CQ + tx + kGramSide * b];
#pragma unroll
            for (int a = 0; a < TP; ++a)
#pragma unroll
                for (int b = 0; b < TQ; ++b) acc[a][b] = fma(u[a], v[b], acc[a][b]);
        }
        __syncthreads();  // the tile has been read: the next one may be staged
    }
    const int pq = p * q;
    double*   mine = part + (int64_t)blockIdx.x * pq;
#pragma unroll
    for (int a = 0; a < TP; ++a)
#pragma unroll
        for (int b = 0; b < TQ; ++b)
        {
            const int i = ty + kGramSide * a, j = tx + kGramSide * b;
            if (i < p && j < q) mine[i * q + j] = acc[a][b];
        }
    __threadfence();  // every thread stored partial sums (took_last_ticket's one fence covers wavefront 0's alone)
    if (!took_last_ticket(ticket)) return;
    for (int e = threadIdx.x; e < pq; e += kBlock)
    {
        double t = 0.0;
        for (int g = 0; g < (int)gridDim.x; ++g) t += partial_sum_load(part + (int64_t)g * pq + e);
        G[e] = t;
    }
    if (threadIdx.x == 0) *ticket = 0;
}

template <int QT>
__global__ __launch_bounds__(kBlock) void block_combine_kernel(int64_t n, int p, int q, const double* S, int64_t lds, const double* C,
                                                               double* Out, int64_t ldo)
{
    __shared__ double sS[kBlockMaxCols * kCombRows];
    const int         lane = threadIdx.x & (kWave - 1);
    const int         w    = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    const int         j0   = w * QT;
    const int64_t     ntiles = (n + kCombRows - 1) / kCombRows;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x)
    {
        const int64_t row  = tile * kCombRows + lane;
        const bool    live = row < n;
        for (int k = w; k < p; k += kBlock / kWave) sS[k * kCombRows + lane] = live ? S[(int64_t)k * lds + row] : 0.0;
        __syncthreads();  // every read of the tile's rows is done: they may be written (Out may be S)
        double acc[QT];
#pragma unroll
        for (int jj = 0; jj < QT; ++jj) acc[jj] = 0.0;
        // (QT scalars of C a step: the wide instances keep one step's in SGPRs, the narrow ones a few steps')
#pragma unroll(QT >= 8 ? 1 : 4)
        for (int k = 0; k < p; ++k)
        {
            const double  s  = sS[k * kCombRows + lane];
            const double* ck = C + k * q;
#pragma unroll
            for (int jj = 0; jj < QT; ++jj) acc[jj] = fma(s, ck[min(j0 + jj, q - 1)], acc[jj]);
        }
        if (live)
        {
#pragma unroll
            for (int jj = 0; jj < QT; ++jj)
                if (j0 + jj < q) Out[(int64_t)(j0 + jj) * ldo + row] = acc[jj];
        }
        __syncthreads();  // the tile has been read: the next one may be staged
    }
}

// workgroups of a Gram launch: a function of n alone.  (A grid of 2^20 / (p q) workgroups held to 256 .. 2048, with the next tile
// prefetched through registers, was measured: faster at 48 columns, 2.2 against 3.4 ms on 4M rows, and slower at 8 to 24.)
int gram_grid(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>(kGramMaxGrid, ceil_div(n, kGramRows))); }
int gram_tile(int cols) { return cols <= 16 ? 1 : cols <= 32 ? 2 : cols <= 48 ? 3 : 6; }

struct gram_args
{
    int64_t       n;
    int           p, q;
    const double *U, *V;
    int64_t       ldu, ldv;
    double *      part, *G;
    uint32_t*     ticket;
    hipStream_t   st;
};

template <int TP, int TQ, bool SAME>
void gram_launch(const gram_args& a)
{
    hipLaunchKernelGGL((block_gram_kernel<TP, TQ, SAME>), dim3(gram_grid(a.n)), dim3(kBlock), 0, a.st, a.n, a.p, a.q, a.U, a.ldu, a.V, a.ldv, a.part, a.G,
                       a.ticket);
}

template <int TP>
void gram_launch_q(const gram_args& a)
{
    switch (gram_tile(a.q))
    {
        case 1: gram_launch<TP, 1, false>(a); break;
        case 2: gram_launch<TP, 2, false>(a); break;
        case 3: gram_launch<TP, 3, false>(a); break;
        default: gram_launch<TP, 6, false>(a); break;
    }
}

// the block's extent in doubles: (cols - 1) ld + n
int64_t block_extent(int64_t n, int cols, int64_t ld) { return (int64_t)(cols - 1) * ld + n; }

// the context's device area: a ticket, the small matrix (G out, C in), the partial sums;  and its pinned twin of the small matrix
constexpr size_t kSmallBytes = sizeof(double) * kBlockMaxCols * kBlockMaxCols;
constexpr size_t kAreaHead   = 256 + kSmallBytes;

int block_area(spmv_ctx* ctx, size_t part_doubles)
{
    const size_t want = kAreaHead + sizeof(double) * part_doubles;
    if (!ctx->block_pinned)
    {
        SPMV_HIP(hipHostMalloc((void**)&ctx->block_pinned, kSmallBytes, hipHostMallocDefault));
        SPMV_HIP(hipEventCreateWithFlags(&ctx->block_ev, hipEventDisableTiming));
    }
    if (ctx->block_dev_bytes >= want) return SPMV_OK;
    if (ctx->block_dev)
    {
        SPMV_HIP(hipStreamSynchronize(ctx->stream));
        SPMV_HIP(hipFree(ctx->block_dev));
        ctx->block_dev       = nullptr;
        ctx->block_dev_bytes = 0;
    }
    SPMV_HIP(hipMalloc(&ctx->block_dev, want));
    ctx->block_dev_bytes = want;
    SPMV_HIP(hipMemsetAsync(ctx->block_dev, 0, 256, ctx->stream));  // the ticket: every launch leaves it 0
    return SPMV_OK;
}
}  // namespace

void block_ops_free(spmv_ctx* ctx)
{
    if (ctx->block_dev) (void)hipFree(ctx->block_dev);
    if (ctx->block_pinned) (void)hipHostFree(ctx->block_pinned);
    if (ctx->block_ev) (void)hipEventDestroy(ctx->block_ev);
    ctx->block_dev    = nullptr;
    ctx->block_pinned = nullptr;
    ctx->block_ev     = nullptr;
}

size_t block_gram_part_doubles(int64_t n, int p, int q) { return (size_t)gram_grid(n) * (size_t)p * (size_t)q; }
size_t block_gram_part_bound(int cols) { return (size_t)kGramMaxGrid * cols * cols; }

int block_gram_launch(spmv_ctx* ctx, int64_t n, int p, const double* U, int64_t ldu, int q, const double* V, int64_t ldv, double* G, double* part,
                      uint32_t* ticket)
{
    if (n == 0) return hip_step(hipMemsetAsync(G, 0, sizeof(double) * (size_t)p * q, ctx->stream), "spmv_block_gram", "clearing G");
    const gram_args a = {n, p, q, U, V, ldu, ldv, part, G, ticket, ctx->stream};
    if (U == V && ldu == ldv && p == q)
        switch (gram_tile(p))
        {
            case 1: gram_launch<1, 1, true>(a); break;
            case 2: gram_launch<2, 2, true>(a); break;
            case 3: gram_launch<3, 3, true>(a); break;
            default: gram_launch<6, 6, true>(a); break;
        }
    else
        switch (gram_tile(p))
        {
            case 1: gram_launch_q<1>(a); break;
            case 2: gram_launch_q<2>(a); break;
            case 3: gram_launch_q<3>(a); break;
            default: gram_launch_q<6>(a); break;
        }
    return hip_step(hipGetLastError(), "spmv_block_gram", "the launch");
}

int block_combine_launch(spmv_ctx* ctx, int64_t n, int p, const double* S, int64_t lds, int q, const double* C, double* Out, int64_t ldo)
{
    if (n == 0) return SPMV_OK;
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(kMaxGrid, ceil_div(n, kCombRows)));
#define SPMV_COMBINE(QT) hipLaunchKernelGGL((block_combine_kernel<QT>), dim3(grid), dim3(kBlock), 0, ctx->stream, n, p, q, S, lds, C, Out, ldo)
    if (q <= 8)
        SPMV_COMBINE(2);
    else if (q <= 16)
        SPMV_COMBINE(4);
    else if (q <= 32)
        SPMV_COMBINE(8);
    else if (q <= 48)
        SPMV_COMBINE(12);
    else
        SPMV_COMBINE(24);
#undef SPMV_COMBINE
    return hip_step(hipGetLastError(), "spmv_block_combine", "the launch");
}

// ---- the checks of the two ABI entries: on the host, before the device is touched ------------------------------------------------
int block_gram_check(const spmv_ctx* ctx, int64_t n, int p, const spmv_vec* U, int64_t ldu, int q, const spmv_vec* V, int64_t ldv, const double* G_host)
{
    const char* const who = "spmv_block_gram";
    SPMV_REQUIRE(ctx && U && V && G_host, "%s: null argument", who);
    SPMV_REQUIRE(p >= 1 && p <= kBlockMaxCols && q >= 1 && q <= kBlockMaxCols, "%s: p = %d, q = %d columns, must be 1 .. %d", who, p, q, kBlockMaxCols);
    SPMV_REQUIRE(n >= 0, "%s: n = %lld rows", who, (long long)n);
    SPMV_REQUIRE(ldu >= n && ldv >= n, "%s: ldu = %lld, ldv = %lld, must be at least n = %lld", who, (long long)ldu, (long long)ldv, (long long)n);
    SPMV_REQUIRE(U->n >= block_extent(n, p, ldu) && V->n >= block_extent(n, q, ldv),
                 "%s: a vector is too short for its block: U has %lld entries and needs %lld, V has %lld and needs %lld", who, (long long)U->n,
                 (long long)block_extent(n, p, ldu), (long long)V->n, (long long)block_extent(n, q, ldv));
    return SPMV_OK;
}

int block_combine_check(const spmv_ctx* ctx, int64_t n, int p, const spmv_vec* S, int64_t lds, int q, const double* C_host, const spmv_vec* Out, int64_t ldo)
{
    const char* const who = "spmv_block_combine";
    SPMV_REQUIRE(ctx && S && Out && C_host, "%s: null argument", who);
    SPMV_REQUIRE(p >= 1 && p <= kBlockMaxCols && q >= 1 && q <= kBlockMaxCols, "%s: p = %d, q = %d columns, must be 1 .. %d", who, p, q, kBlockMaxCols);
    SPMV_REQUIRE(n >= 0, "%s: n = %lld rows", who, (long long)n);
    SPMV_REQUIRE(lds >= n && ldo >= n, "%s: lds = %lld, ldo = %lld, must be at least n = %lld", who, (long long)lds, (long long)ldo, (long long)n);
    const int64_t es = block_extent(n, p, lds), eo = block_extent(n, q, ldo);
    SPMV_REQUIRE(S->n >= es && Out->n >= eo, "%s: a vector is too short for its block: S has %lld entries and needs %lld, Out has %lld and needs %lld", who,
                 (long long)S->n, (long long)es, (long long)Out->n, (long long)eo);
    const bool in_place = S->d == Out->d && lds == ldo;
    const bool apart    = n == 0 || S->d + es <= Out->d || Out->d + eo <= S->d;
    SPMV_REQUIRE(in_place || apart, "%s: Out and S overlap: Out may be S itself (the same start and the same ld), or lie apart from it", who);
    return SPMV_OK;
}

// ---- the two entries behind their checks ---------------------------------------------------------------------------------------
int block_gram(spmv_ctx* ctx, int64_t n, int p, const double* U, int64_t ldu, int q, const double* V, int64_t ldv, double* G_host)
{
    const size_t pq = (size_t)p * q;
    if (n == 0)
    {
        for (size_t e = 0; e < pq; ++e) G_host[e] = 0.0;
        return SPMV_OK;
    }
    SPMV_TRY(block_area(ctx, block_gram_part_doubles(n, p, q)));
    unsigned char* area = (unsigned char*)ctx->block_dev;
    double*        G    = (double*)(area + 256);
    SPMV_TRY(block_gram_launch(ctx, n, p, U, ldu, q, V, ldv, G, (double*)(area + kAreaHead), (uint32_t*)area));
    hipError_t e = hipMemcpyAsync(ctx->block_pinned, G, sizeof(double) * pq, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    SPMV_TRY(hip_step(e, "spmv_block_gram", "reading G"));
    std::memcpy(G_host, ctx->block_pinned, sizeof(double) * pq);
    return SPMV_OK;
}

int block_combine(spmv_ctx* ctx, int64_t n, int p, const double* S, int64_t lds, int q, const double* C_host, double* Out, int64_t ldo)
{
    if (n == 0) return SPMV_OK;
    const char* const who = "spmv_block_combine";
    SPMV_TRY(block_area(ctx, 0));
    // the staging area still feeds the previous call's copy until that copy's event has passed (an event never recorded has passed)
    SPMV_TRY(hip_step(hipEventSynchronize(ctx->block_ev), who, "waiting for the previous copy of C"));
    const size_t bytes = sizeof(double) * (size_t)p * q;
    std::memcpy(ctx->block_pinned, C_host, bytes);
    double* C = (double*)((unsigned char*)ctx->block_dev + 256);
    SPMV_TRY(hip_step(hipMemcpyAsync(C, ctx->block_pinned, bytes, hipMemcpyHostToDevice, ctx->stream), who, "the copy of C"));
    SPMV_TRY(hip_step(hipEventRecord(ctx->block_ev, ctx->stream), who, "recording the copy of C"));
    return block_combine_launch(ctx, n, p, S, lds, q, C, Out, ldo);
}
}  // namespace spmv
