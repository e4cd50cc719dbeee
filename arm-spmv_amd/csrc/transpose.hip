// transpose.hip - the transposed product y += A^T x (spmv_apply_transpose) for every format.
//
// Most formats need no kernel of their own: A's arrays read the other way round ARE a handle of A^T.  A CSR handle's row_ptr /
// col_ind / values are the CSC arrays of A^T, a CSC handle's are the CSR arrays of A^T, and a COO handle with its row and column
// arrays swapped is A^T.  So the transposed state of such a handle is an internal companion handle that borrows A's arrays
// (owned = false: it never frees them) and picks its own kernel like any handle of its format - a CSC companion chooses between
// the scatter and the row-grouped copy (which is the CSR of A^T, and picks panel or another CSR kernel itself), a CSR companion
// runs all of CSR AUTO.  A BSR handle gets a BSR handle of A^T with arrays of its own (convert_bsr.hip: blocks in stable order by
// block column, each transposed as it is copied) and the forward kernel runs on that; a handle of format 6 (single-precision value
// storage) likewise gets a format-6 handle of A^T of its own (convert_f32.hip).  An ELL handle becomes a COO companion: its rows are ELL's col_ind (borrowed), its columns the row of every
// slot (an array made here, owned by the transposed state, not by the companion), its values ELL's.  Every slot counts, padding
// included (0.0 * x_i into y[pad column]), as the forward ELL product counts it.
//
// DIA has the one new kernel, dia_transpose_kernel: output j (j < the forward kernel's column bound) takes the diagonals in slot
// order from y_j, acc = fma(val[i * ndiags + d], x[i], acc) with i = j - off_d, 0 <= i < nrow.  It reads A's own row-major values.
//
// The transposed state is built once (spmv_mat_transpose_setup, synchronous; the first transposed product runs it) and is no part
// of the handle's forward state: not of its kernel, its copies, its device_bytes or its plan.
#include "common.hpp"
#include "wave.hpp"

namespace spmv
{
struct transpose_state
{
    spmv_mat* comp       = nullptr;  // CSR / CSC / COO / ELL: the companion handle of A^T (borrows A's arrays)
    int32_t*  slot_rows  = nullptr;  // ELL: the row of every slot, column-major like col_ind (the companion's column indices)
    int32_t*  dia_bounds = nullptr;  // DIA: per chunk of kTrChunk diagonals, its smallest and its largest offset
    int32_t   dia_chunks = 0;
    int32_t   dia_rows   = 0;        // DIA: rows of the LDS window of the tiled kernel (256 + widest chunk spread); 0: the general kernel
    int64_t   bytes      = 0;        // device memory held here (the companion's own counts on top)
    int64_t   counted_in_owner = 0;  // BSR: the companion's bytes as they were added to the owner's device_bytes
};

namespace
{

// ---- ELL: the row of every slot (slot s of row i sits at i + s * nrow) ---------------------------------------------------------
__global__ __launch_bounds__(kBlock) void ell_slot_rows_kernel(int nrow, int64_t total, int32_t* __restrict__ rows)
{
    for (int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x; t < total; t += (int64_t)gridDim.x * kBlock)
        rows[t] = (int32_t)(t % nrow);
}

// ---- DIA transposed ------------------------------------------------------------------------------------------------------------
// A workgroup owns kBlock consecutive outputs j0 .. j0 + 255.  Diagonal d of output j reads row i = j - off_d, so for a chunk of
// kTrChunk diagonals with offsets in [lo, hi] the workgroup needs rows [j0 - hi, j0 + 256 - lo) of them: those rows x the chunk's
// diagonals are copied into LDS (row stride kTrChunk + 1: conflict-free, as in dia_kernel), with the matching stretch of x, and
// every lane then walks its own output from there.  Each value comes from HBM about once (a window overlaps the next workgroup's
// by the chunk's spread).  WIDE: 16-byte loads of two adjacent diagonals (even ndiags, 16-byte aligned values), as dia_kernel.
// The next chunk's loads are in flight while the current one is consumed.  Chunks spread wider than kTrSpread take the general
// kernel below.
constexpr int kTrChunk   = 16;
constexpr int kTrSpread  = 64;
constexpr int kTrMaxRows = kBlock + kTrSpread;

template <bool WIDE>
__global__ __launch_bounds__(kBlock) void dia_transpose_kernel(int nrow, int jmax, int ndiags, const int32_t* __restrict__ offsets,
                                                               const int32_t* __restrict__ bounds, const double* __restrict__ val,
                                                               const double* __restrict__ x, double* __restrict__ y, int win_rows)
{
    extern __shared__ double lds[];
    double*       tile  = lds;                                 // win_rows x (kTrChunk + 1)
    double*       xs    = lds + (size_t)win_rows * (kTrChunk + 1);  // win_rows
    constexpr int PER   = WIDE ? 2 : 1;                        // diagonals per lane and load
    constexpr int LPR   = kTrChunk / PER;                      // lanes per row of the tile
    constexpr int RPP   = kBlock / LPR;                        // rows per pass of the workgroup
    constexpr int NPASS = kTrMaxRows / RPP;                    // passes for the widest window
    constexpr int XPASS = (kTrMaxRows + kBlock - 1) / kBlock;  // x entries per lane
    static_assert(kTrMaxRows % RPP == 0, "whole passes");
    const int  j0     = blockIdx.x * kBlock;
    const int  j      = j0 + threadIdx.x;
    const bool mine   = j < jmax;
    double     acc    = mine ? y[j] : 0.0;
    const int  d_mine = (threadIdx.x % LPR) * PER;
    const int  r_mine = threadIdx.x / LPR;
    double     stage[NPASS * PER];
    double     xstage[XPASS];
    auto fetch = [&](int c) {
        const int     d0   = c * kTrChunk;
        const int     lo   = bounds[2 * c], hi = bounds[2 * c + 1];
        const int     rows = kBlock + hi - lo;
        const int64_t base = (int64_t)j0 - hi;  // the window's first row
#pragma unroll
        for (int p = 0; p < NPASS; ++p)
        {
            const int     r  = r_mine + p * RPP;
            const int64_t i  = base + r;
            const bool    in = r < rows && i >= 0 && i < nrow && d0 + d_mine < ndiags;
            if constexpr (WIDE)
            {
                f64x2 v = {0.0, 0.0};
                if (in) v = __builtin_nontemporal_load((const f64x2*)(val + (size_t)i * ndiags + d0 + d_mine));
                stage[2 * p]     = v[0];
                stage[2 * p + 1] = v[1];
            }
            else
                stage[p] = in ? load_stream(val + (size_t)i * ndiags + d0 + d_mine) : 0.0;
        }
#pragma unroll
        for (int q = 0; q < XPASS; ++q)
        {
            const int     r = (int)threadIdx.x + q * kBlock;
            const int64_t i = base + r;
            xstage[q]       = (r < rows && i >= 0 && i < nrow) ? x[i] : 0.0;
        }
    };
    const int nchunks = (ndiags + kTrChunk - 1) / kTrChunk;
    fetch(0);
    for (int c = 0; c < nchunks; ++c)
    {
        const int d0 = c * kTrChunk;
        const int dn = min(kTrChunk, ndiags - d0);
        const int hi = bounds[2 * c + 1];
        __syncthreads();  // the previous chunk has been consumed
#pragma unroll
        for (int p = 0; p < NPASS; ++p)
        {
            const int r = r_mine + p * RPP;
            if (r < win_rows)
#pragma unroll
                for (int e = 0; e < PER; ++e) tile[r * (kTrChunk + 1) + d_mine + e] = stage[PER * p + e];
        }
#pragma unroll
        for (int q = 0; q < XPASS; ++q)
        {
            const int r = (int)threadIdx.x + q * kBlock;
            if (r < win_rows) xs[r] = xstage[q];
        }
        __syncthreads();
        if (c + 1 < nchunks) fetch(c + 1);  // in flight while this chunk is consumed
        if (mine)
            for (int d = 0; d < dn; ++d)
            {
                const int     off = offsets[d0 + d];  // wave-uniform address: scalar load
                const int64_t i   = (int64_t)j - off;
                if (i >= 0 && i < nrow)
                {
                    const int lr = (int)threadIdx.x + hi - off;  // i - (j0 - hi): inside [0, 256 + hi - lo)
                    acc          = fma(tile[lr * (kTrChunk + 1) + d], xs[lr], acc);
                }
            }
    }
    if (mine) y[j] = acc;
}

// any offsets: one lane per output, the values straight from global memory (8-byte loads, ndiags apart across lanes)
__global__ __launch_bounds__(kBlock) void dia_transpose_general_kernel(int nrow, int jmax, int ndiags, const int32_t* __restrict__ offsets,
                                                                       const double* __restrict__ val, const double* __restrict__ x,
                                                                       double* __restrict__ y)
{
    const int j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= jmax) return;
    double acc = y[j];
    for (int d = 0; d < ndiags; ++d)
    {
        const int64_t i = (int64_t)j - offsets[d];
        if (i >= 0 && i < nrow) acc = fma(val[(size_t)i * ndiags + d], x[i], acc);
    }
    y[j] = acc;
}

// the forward DIA product's column bound (kernels_misc.hip: dia_apply)
inline int dia_jmax(const spmv_mat* A) { return std::min(A->dia_col_bound > 0 ? A->dia_col_bound : std::min(A->nrow, A->ncol), A->ncol); }

int dia_transpose_apply(spmv_ctx* ctx, const spmv_mat* A, const transpose_state* st, const double* x, double* y)
{
    const int jmax = dia_jmax(A);
    if (A->nrow == 0 || A->k == 0 || jmax <= 0) return SPMV_OK;
    const dim3 grid((unsigned)ceil_div(jmax, kBlock));
    if (st->dia_rows == 0)
        hipLaunchKernelGGL(dia_transpose_general_kernel, grid, dim3(kBlock), 0, ctx->stream, A->nrow, jmax, A->k, A->a, A->v, x, y);
    else
    {
        const size_t lds  = sizeof(double) * (size_t)st->dia_rows * (kTrChunk + 2);
        const bool   wide = A->k % 2 == 0 && (((uintptr_t)A->v) & 15) == 0;
        if (wide)
            hipLaunchKernelGGL(dia_transpose_kernel<true>, grid, dim3(kBlock), lds, ctx->stream, A->nrow, jmax, A->k, A->a, st->dia_bounds,
                               A->v, x, y, st->dia_rows);
        else
            hipLaunchKernelGGL(dia_transpose_kernel<false>, grid, dim3(kBlock), lds, ctx->stream, A->nrow, jmax, A->k, A->a, st->dia_bounds,
                               A->v, x, y, st->dia_rows);
    }
    SPMV_HIP(hipGetLastError());
    return SPMV_OK;
}

// DIA set-up: the offsets read once, per chunk their bounds; the tiled kernel where every chunk spreads at most kTrSpread
int dia_transpose_setup(spmv_mat* A, transpose_state* st)
{
    if (A->k == 0) return SPMV_OK;
    std::vector<int32_t> off((size_t)A->k);
    SPMV_HIP(hipMemcpyAsync(off.data(), A->a, sizeof(int32_t) * off.size(), hipMemcpyDeviceToHost, A->ctx->stream));
    SPMV_HIP(hipStreamSynchronize(A->ctx->stream));
    const int            nchunks = (int)ceil_div(A->k, kTrChunk);
    std::vector<int32_t> b(2 * (size_t)nchunks);
    int64_t              widest = 0;
    for (int c = 0; c < nchunks; ++c)
    {
        const auto first = off.begin() + (size_t)c * kTrChunk, last = off.begin() + std::min<size_t>(off.size(), (size_t)(c + 1) * kTrChunk);
        b[2 * c]         = *std::min_element(first, last);
        b[2 * c + 1]     = *std::max_element(first, last);
        widest           = std::max<int64_t>(widest, (int64_t)b[2 * c + 1] - b[2 * c]);
    }
    if (widest > kTrSpread) return SPMV_OK;  // (the general kernel)
    SPMV_HIP(hipMalloc(&st->dia_bounds, sizeof(int32_t) * b.size()));
    st->bytes += (int64_t)(sizeof(int32_t) * b.size());
    SPMV_HIP(hipMemcpyAsync(st->dia_bounds, b.data(), sizeof(int32_t) * b.size(), hipMemcpyHostToDevice, A->ctx->stream));
    SPMV_HIP(hipStreamSynchronize(A->ctx->stream));
    st->dia_chunks = nchunks;
    st->dia_rows   = kBlock + (int)widest;
    return SPMV_OK;
}

// An internal handle of `format` over borrowed arrays; its kernel is what "transpose_kernel" asks for (spmv_mat_set_kernel), or
// chosen by the format's own AUTO.  No plan reaches it: the transposed state is not part of plans (a fresh handle has no node, and
// a context's plan is armed only while a public entry point creates a handle).
int make_companion(spmv_mat* A, int32_t format, int32_t nrow, int32_t ncol, int64_t nnz, const int32_t* a, const int32_t* b,
                   const double* v, spmv_mat** out)
{
    spmv_mat* m = new (std::nothrow) spmv_mat();
    if (!m) SPMV_FAIL(SPMV_ERR_ALLOC, "out of host memory");
    m->ctx           = A->ctx;
    m->format        = format;
    m->nrow          = nrow;
    m->ncol          = ncol;
    m->nnz           = nnz;
    m->a             = a;
    m->b             = b;
    m->v             = v;
    m->owned         = false;
    m->pb_trial      = A->pb_trial;
    m->kernel_forced = A->tr_kernel_req != SPMV_CSR_AUTO;  // (the analysis selects nothing; spmv_mat_set_kernel builds what is asked)
    int rc = format == SPMV_FMT_CSR ? csr_analyse(m) : (format == SPMV_FMT_CSC ? csc_analyse(m) : coo_analyse(m));
    if (rc == SPMV_OK && A->tr_kernel_req != SPMV_CSR_AUTO) rc = spmv_mat_set_kernel(m, A->tr_kernel_req, 0);
    if (rc != SPMV_OK)
    {
        (void)hipStreamSynchronize(A->ctx->stream);
        mat_free(m);
        return rc;
    }
    *out = m;
    return SPMV_OK;
}

int transpose_build(spmv_mat* A, transpose_state* st)
{
    switch (A->format)
    {
        case SPMV_FMT_CSR: return make_companion(A, SPMV_FMT_CSC, A->ncol, A->nrow, A->nnz, A->a, A->b, A->v, &st->comp);
        case SPMV_FMT_CSC: return make_companion(A, SPMV_FMT_CSR, A->ncol, A->nrow, A->nnz, A->a, A->b, A->v, &st->comp);
        case SPMV_FMT_COO: return make_companion(A, SPMV_FMT_COO, A->ncol, A->nrow, A->nnz, A->b, A->a, A->v, &st->comp);
        case SPMV_FMT_ELL:
        {
            const int64_t total = (int64_t)A->nrow * A->k;
            if (total > 0)
            {
                if (hipMalloc(&st->slot_rows, sizeof(int32_t) * (size_t)total) != hipSuccess)
                {
                    (void)hipGetLastError();
                    SPMV_FAIL(SPMV_ERR_ALLOC, "spmv_mat_transpose_setup: no device memory for the rows of %lld ELL slots", (long long)total);
                }
                st->bytes += (int64_t)sizeof(int32_t) * total;
                const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(kMaxGrid, ceil_div(total, kBlock)));
                hipLaunchKernelGGL(ell_slot_rows_kernel, dim3(grid), dim3(kBlock), 0, A->ctx->stream, A->nrow, total, st->slot_rows);
                SPMV_HIP(hipGetLastError());
            }
            return make_companion(A, SPMV_FMT_COO, A->ncol, A->nrow, total, A->b, st->slot_rows, A->v, &st->comp);
        }
        case SPMV_FMT_DIA: return dia_transpose_setup(A, st);
        case SPMV_FMT_BSR:
            // a BSR handle of A^T with arrays of its own (convert_bsr.hip), run by the forward kernel; unlike the borrowed companions
            // above it is real memory of the handle's: counted in A's device_bytes until transpose_free
            SPMV_TRY(bsr_transpose(A->ctx, A, &st->comp));
            st->counted_in_owner = st->comp->device_bytes;
            A->device_bytes += st->counted_in_owner;
            return SPMV_OK;
        case SPMV_FMT_CSR_F32:
            // a format-6 handle of A^T with arrays of its own (convert_f32.hip: widened, transposed on the device, packed again; the two
            // fp64 intermediates are gone when it returns), run by the forward kernel; counted in A's device_bytes like a BSR companion
            SPMV_TRY(f32_transpose(A->ctx, A, &st->comp));
            st->counted_in_owner = st->comp->device_bytes;
            A->device_bytes += st->counted_in_owner;
            return SPMV_OK;
        default: SPMV_FAIL(SPMV_ERR_INVALID, "spmv_mat_transpose_setup: unknown format %d", A->format);
    }
}

// a CSR handle that gave up col_ind / values (panel_keep_csr = 0) has no arrays left to read the other way round
inline bool released_csr(const spmv_mat* A) { return A->format == SPMV_FMT_CSR && A->nnz > 0 && (!A->b || !A->v); }

// Every check is made before the device is touched, so that they hold (and are tested) on a machine without one.
int check_transpose_args(const char* fn, spmv_ctx* ctx, const spmv_mat* A, const spmv_vec* x, spmv_vec* y)
{
    SPMV_REQUIRE(ctx && A && x && y, "%s: null argument", fn);
    SPMV_REQUIRE(x->n == A->nrow, "%s: x has %lld entries, matrix (shard) has %d rows", fn, (long long)x->n, A->nrow);
    SPMV_REQUIRE(y->n == A->ncol, "%s: y has %lld entries, matrix has %d columns", fn, (long long)y->n, A->ncol);
    SPMV_REQUIRE(x->n == 0 || y->n == 0 || x->d + x->n <= y->d || y->d + y->n <= x->d, "%s: x and y must not overlap", fn);
    SPMV_REQUIRE(!released_csr(A), "%s: this handle gave up its CSR arrays (panel_keep_csr = 0)", fn);
    return SPMV_OK;
}

}  // namespace

// (these two are called by the least-squares loop as well: solver_cgls.hip)
int transpose_setup(spmv_mat* A)
{
    SPMV_REQUIRE(!released_csr(A), "spmv_mat_transpose_setup: this handle gave up its CSR arrays (panel_keep_csr = 0)");
    if (A->tr) return SPMV_OK;
    SPMV_HIP(hipSetDevice(A->ctx->device));
    transpose_state* st = new (std::nothrow) transpose_state();
    if (!st) SPMV_FAIL(SPMV_ERR_ALLOC, "out of host memory");
    A->tr  = st;  // (transpose_free takes back whatever a failed build left)
    int rc = transpose_build(A, st);
    if (rc == SPMV_OK && hipStreamSynchronize(A->ctx->stream) != hipSuccess)
    {
        set_error("spmv_mat_transpose_setup: %s", hipGetErrorString(hipGetLastError()));
        rc = SPMV_ERR_HIP;
    }
    if (rc != SPMV_OK) transpose_free(A);
    return rc;
}

int transpose_apply(spmv_ctx* ctx, const spmv_mat* A, const double* x, double* y)
{
    const transpose_state* st = A->tr;
    if (A->format == SPMV_FMT_DIA) return dia_transpose_apply(ctx, A, st, x, y);
    return st->comp ? mat_apply_ex(ctx, st->comp, x, y) : SPMV_OK;
}

void transpose_free(spmv_mat* A)
{
    transpose_state* st = A->tr;
    if (!st) return;
    if (st->comp || st->slot_rows || st->dia_bounds) (void)hipStreamSynchronize(A->ctx->stream);
    if (st->comp) mat_free(st->comp);  // (its own layouts and copies; A's arrays it only borrowed - a BSR companion owns its own)
    A->device_bytes -= st->counted_in_owner;
    if (st->slot_rows) (void)hipFree(st->slot_rows);
    if (st->dia_bounds) (void)hipFree(st->dia_bounds);
    delete st;
    A->tr = nullptr;
}

int transpose_set_kernel(spmv_mat* A, int64_t kernel)
{
    const bool csr_companion = A->format == SPMV_FMT_CSC;
    if (A->format == SPMV_FMT_DIA)
        SPMV_REQUIRE(kernel == SPMV_CSR_AUTO || kernel == SPMV_CSR_VECTOR, "transpose_kernel: a DIA handle has one transposed kernel: AUTO (0) or VECTOR (1)");
    else if (A->format == SPMV_FMT_BSR)
        SPMV_REQUIRE(kernel == SPMV_CSR_AUTO || kernel == SPMV_CSR_VECTOR, "transpose_kernel: the BSR handle of A^T has one kernel: AUTO (0) or VECTOR (1)");
    else if (A->format == SPMV_FMT_CSR_F32)
        SPMV_REQUIRE(kernel == SPMV_CSR_AUTO || kernel == SPMV_CSR_VECTOR, "transpose_kernel: the format 6 handle of A^T has one kernel: AUTO (0) or VECTOR (1)");
    else if (csr_companion)
        SPMV_REQUIRE(kernel >= SPMV_CSR_AUTO && kernel <= SPMV_CSR_ELL, "transpose_kernel: a CSR kernel id (0 .. 8) for the CSR companion of a CSC handle");
    else
        SPMV_REQUIRE(kernel == SPMV_CSR_AUTO || kernel == SPMV_CSR_VECTOR || kernel == SPMV_CSR_PANEL,
                     "transpose_kernel: the companion (CSC or COO) takes AUTO (0), VECTOR (1: its own kernel) or PANEL (4: the row-grouped copy)");
    if (A->tr_kernel_req != (int32_t)kernel) transpose_free(A);  // (built under another request: the next set-up builds it anew)
    A->tr_kernel_req = (int32_t)kernel;
    return SPMV_OK;
}

bool transpose_get_param(const spmv_mat* A, const char* name, int64_t* value)
{
    const transpose_state* st = A->tr;
    if (!strcmp(name, "transpose_ready"))
        *value = st ? 1 : 0;
    else if (!strcmp(name, "transpose_bytes"))
        *value = st ? st->bytes + (st->comp ? st->comp->device_bytes : 0) : 0;
    else if (!strcmp(name, "transpose_kernel"))
    {
        if (!st)
            *value = A->tr_kernel_req;
        else if (A->format == SPMV_FMT_DIA)
            *value = SPMV_CSR_VECTOR;  // (the format's own transposed kernel)
        else
            *value = st->comp ? st->comp->kernel : A->tr_kernel_req;
    }
    else if (!strcmp(name, "transpose_rowgrouped_kernel"))  // the CSR kernel of the companion's row-grouped copy, where it runs from one
        *value = st && st->comp && runs_from_rowgrouped(st->comp) ? st->comp->rowgrouped->kernel : 0;
    else
        return false;
    return true;
}
}  // namespace spmv

using namespace spmv;

extern "C" {
int spmv_mat_transpose_setup(spmv_mat* A)
{
    SPMV_REQUIRE(A, "spmv_mat_transpose_setup: null matrix");
    return transpose_setup(A);
}

int spmv_apply_transpose(spmv_ctx* ctx, const spmv_mat* A, const spmv_vec* x, spmv_vec* y)
{
    SPMV_TRY(check_transpose_args("spmv_apply_transpose", ctx, A, x, y));
    SPMV_TRY(transpose_setup(const_cast<spmv_mat*>(A)));  // (once; the transposed state is no part of the forward one)
    SPMV_HIP(hipSetDevice(ctx->device));
    return transpose_apply(ctx, A, x->d, y->d);
}

int spmv_apply_transpose_timed(spmv_ctx* ctx, const spmv_mat* A, const spmv_vec* x, spmv_vec* y, int32_t reps, double* ms_per_apply)
{
    SPMV_TRY(check_transpose_args("spmv_apply_transpose_timed", ctx, A, x, y));
    SPMV_REQUIRE(reps > 0 && ms_per_apply, "spmv_apply_transpose_timed: reps=%d", reps);
    SPMV_TRY(transpose_setup(const_cast<spmv_mat*>(A)));  // outside the timed region
    SPMV_HIP(hipSetDevice(ctx->device));
    float ms = 0.f;
    SPMV_TRY(time_launches(ctx, reps, [&] { return transpose_apply(ctx, A, x->d, y->d); }, &ms));
    *ms_per_apply = ms;
    return SPMV_OK;
}
}  // extern "C"
