// abi.hip — the extern "C" entry points declared in include/spmv_abi.h.
//
// This file is glue: argument checking, handle life cycle, host<->device copies, and dispatch to the
// format kernels (kernels_*.hip), the conversions (convert.hip) and the generators (generate.hip).
// There is deliberately no CPU implementation of anything behind these entry points.
#include <algorithm>
#include <cmath>
#include <new>
#include <vector>

#include "common.hpp"
#include "sddmm_settings.hpp"
#include "solver_host.hpp"

namespace spmv
{
static thread_local char g_last_error[512] = "";

void set_error(const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_last_error, sizeof(g_last_error), fmt, ap);
    va_end(ap);
}

int ensure_scratch(spmv_ctx* ctx, size_t bytes)
{
    if (ctx->scratch_bytes >= bytes) return SPMV_OK;
    if (ctx->scratch)
    {
        SPMV_HIP(hipStreamSynchronize(ctx->stream));
        SPMV_HIP(hipFree(ctx->scratch));
        ctx->scratch       = nullptr;
        ctx->scratch_bytes = 0;
    }
    const size_t want = std::max<size_t>(bytes, 1 << 16);
    SPMV_HIP(hipMalloc(&ctx->scratch, want));
    ctx->scratch_bytes = want;
    return SPMV_OK;
}

// a handle over arrays that are not its own (spmv_*_wrap_device; mat_alloc goes on from here)
static int wrap(spmv_ctx* ctx, int32_t format, int32_t nrow, int32_t ncol, int64_t nnz, int32_t k, const int32_t* a,
                const int32_t* b, const double* v, spmv_mat** out)
{
    spmv_mat* m = new (std::nothrow) spmv_mat();
    if (!m) SPMV_FAIL(SPMV_ERR_ALLOC, "out of host memory");
    m->ctx    = ctx;
    m->format = format;
    m->nrow   = nrow;
    m->ncol   = ncol;
    m->nnz    = nnz;
    m->k      = k;
    m->a      = a;
    m->b      = b;
    m->v      = v;
    m->owned  = false;
    *out      = m;
    return SPMV_OK;
}

int mat_alloc(spmv_ctx* ctx, int32_t format, int32_t nrow, int32_t ncol, int64_t nnz, int32_t k, size_t a_count,
              size_t b_count, size_t v_count, spmv_mat** out)
{
    spmv_mat* m = nullptr;
    SPMV_TRY(wrap(ctx, format, nrow, ncol, nnz, k, nullptr, nullptr, nullptr, &m));
    void *a = nullptr, *b = nullptr, *v = nullptr;
    hipError_t e = hipSuccess;
    // a zero-length array still gets a valid (tiny) allocation so that kernels never see nullptr
    if (e == hipSuccess) e = hipMalloc(&a, std::max<size_t>(a_count, 1) * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc(&b, std::max<size_t>(b_count, 1) * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc(&v, std::max<size_t>(v_count, 1) * sizeof(double));
    if (e != hipSuccess)
    {
        if (a) (void)hipFree(a);
        if (b) (void)hipFree(b);
        if (v) (void)hipFree(v);
        delete m;
        SPMV_FAIL(SPMV_ERR_ALLOC, "device allocation of %zu+%zu int32 and %zu fp64 failed: %s", a_count, b_count,
                  v_count, hipGetErrorString(e));
    }
    m->a            = (const int32_t*)a;
    m->b            = (const int32_t*)b;
    m->v            = (const double*)v;
    m->owned        = true;
    m->device_bytes = (int64_t)((a_count + b_count) * sizeof(int32_t) + v_count * sizeof(double));
    *out            = m;
    return SPMV_OK;
}

void mat_free(spmv_mat* m)
{
    if (!m) return;
    transpose_free(m);  // (the companion borrows the arrays freed below)
    trsv_free(m);
    if (m->owned)
    {
        if (m->a) (void)hipFree(const_cast<int32_t*>(m->a));
        if (m->b) (void)hipFree(const_cast<int32_t*>(m->b));
        if (m->v) (void)hipFree(const_cast<double*>(m->v));
    }
    if (m->f32_ent) (void)hipFree(m->f32_ent);
    if (m->win_lo) (void)hipFree(m->win_lo);
    if (m->win_span) (void)hipFree(m->win_span);
    ell_layouts_free(m);
    csr_layouts_free(m, kCsrAllLayouts);
    for (const precond_row& P : kPreconds)  // (in id order)
        if (P.free) P.free(m);
    if (m->rowgrouped) mat_free(m->rowgrouped);
    coo_free_bins(m);
    delete m;
}

static int use_device(const spmv_ctx* ctx)
{
    SPMV_HIP(hipSetDevice(ctx->device));
    return SPMV_OK;
}

static int upload(void* dst, const void* src, size_t bytes, spmv_ctx* ctx)
{
    if (bytes == 0) return SPMV_OK;
    SPMV_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    SPMV_HIP(hipStreamSynchronize(ctx->stream));  // pageable host memory: the caller may free it on return
    return SPMV_OK;
}

// the host arrays of a new handle into its a / b / v (a count of 0 skips one); the handle is freed on failure
static int upload_arrays(spmv_mat* m, const int32_t* a, size_t a_count, const int32_t* b, size_t b_count, const double* v, size_t v_count)
{
    int rc = upload(const_cast<int32_t*>(m->a), a, sizeof(int32_t) * a_count, m->ctx);
    if (rc == SPMV_OK) rc = upload(const_cast<int32_t*>(m->b), b, sizeof(int32_t) * b_count, m->ctx);
    if (rc == SPMV_OK) rc = upload(const_cast<double*>(m->v), v, sizeof(double) * v_count, m->ctx);
    if (rc != SPMV_OK) mat_free(m);
    return rc;
}

// spmv_ctx_set_plan: the handle a public entry point is about to create takes the context's plan (plan.hip: plan_take_armed, at
// the handle's analysis); whatever the entry point does, the flag is down again when it returns
struct plan_arm
{
    spmv_ctx* c;
    explicit plan_arm(spmv_ctx* ctx) : c(ctx)
    {
        if (c && !c->plan_blob.empty()) c->plan_armed = true;
    }
    ~plan_arm()
    {
        if (c) c->plan_armed = false;
    }
};

static int finish(spmv_mat* m, spmv_mat** out)
{
    // The analysis and layout builders index by row and column (histograms in LDS, scatter cursors): a malformed
    // matrix must be refused before they run — an out-of-bounds access on the GPU can take the whole node down.
    int rc = mat_validate(m);
    if (rc == SPMV_OK && m->format == SPMV_FMT_CSR) rc = csr_analyse(m);
    if (rc == SPMV_OK && m->format == SPMV_FMT_COO) rc = coo_analyse(m);
    if (rc == SPMV_OK && m->format == SPMV_FMT_CSC) rc = csc_analyse(m);
    if (rc == SPMV_OK && m->format == SPMV_FMT_ELL) rc = ell_analyse(m);
    if (rc == SPMV_OK && m->format == SPMV_FMT_BSR) rc = bsr_analyse(m);
    if (rc == SPMV_OK && m->format == SPMV_FMT_CSR_F32) rc = csr_f32_analyse(m);
    if (rc != SPMV_OK)
    {
        mat_free(m);
        return rc;
    }
    *out = m;
    return SPMV_OK;
}
}  // namespace spmv

using namespace spmv;

extern "C" {

int         spmv_abi_version(void) { return SPMV_ABI_VERSION; }
const char* spmv_last_error(void) { return g_last_error; }

int spmv_device_count(int* count)
{
    SPMV_REQUIRE(count, "count is null");
    int        n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess)
    {
        *count = 0;
        SPMV_FAIL(SPMV_ERR_NO_DEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e));
    }
    *count = n;
    return SPMV_OK;
}

static void xcd_probe(spmv_ctx* ctx);
static bool host_stores_reach_kernels(spmv_ctx* ctx);
static int ctx_create_common(int device, void* borrowed_stream, bool borrow, spmv_ctx** out)
{
    SPMV_REQUIRE(out, "out is null");
    *out  = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        SPMV_FAIL(SPMV_ERR_NO_DEVICE, "no HIP device is visible; libspmv_hip has no CPU fallback");
    if (device < 0 || device >= n) SPMV_FAIL(SPMV_ERR_NO_DEVICE, "device %d out of range (%d visible)", device, n);
    SPMV_HIP(hipSetDevice(device));
    spmv_ctx* ctx = new (std::nothrow) spmv_ctx();
    if (!ctx) SPMV_FAIL(SPMV_ERR_ALLOC, "out of host memory");
    ctx->device = device;
    if (borrow)
    {
        ctx->stream      = (hipStream_t)borrowed_stream;
        ctx->owns_stream = false;
    }
    else
    {
        hipError_t e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
        if (e != hipSuccess)
        {
            delete ctx;
            SPMV_FAIL(SPMV_ERR_HIP, "hipStreamCreate: %s", hipGetErrorString(e));
        }
        ctx->owns_stream = true;
    }
    hipError_t e = hipEventCreate(&ctx->ev_begin);
    if (e == hipSuccess) e = hipEventCreate(&ctx->ev_end);
    if (e == hipSuccess) e = hipHostMalloc((void**)&ctx->host_pinned, 64, hipHostMallocDefault);
    if (e == hipSuccess) e = hipMalloc((void**)&ctx->dev_scalars, sizeof(double) * kDotDoubles);
    if (e != hipSuccess)
    {
        spmv_ctx_destroy(ctx);
        SPMV_FAIL(SPMV_ERR_HIP, "context setup: %s", hipGetErrorString(e));
    }
    xcd_probe(ctx);  // one small launch: do workgroups b and b + 8 share an XCD on this device? (see below)
    {
        int large = 0;
        if (hipDeviceGetAttribute(&large, hipDeviceAttributeIsLargeBar, device) == hipSuccess && large)
        {
            unsigned* reg = nullptr;
            if (hipDeviceGetAttribute((int*)&reg, hipDeviceAttributeHdpMemFlushCntl, device) == hipSuccess) ctx->hdp_flush = reg;
            const char* off = getenv("SPMV_HOST_STORES");  // SPMV_HOST_STORES=0: never store into device memory from the CPU (A/B; read once per context)
            ctx->large_bar  = !(off && off[0] == '0');
            // ... and only where this context has SEEN it work: CPU stores into a device buffer, read by a kernel, twice (the second
            // round right after a kernel read the first contents - the case a stale cache line would get wrong)
            if (ctx->large_bar && !host_stores_reach_kernels(ctx)) ctx->large_bar = 0;
        }
        (void)hipGetLastError();
    }
    *out = ctx;
    return SPMV_OK;
}

// ---- where do the workgroups of a launch land? --------------------------------------------------------------------------------
// HIP promises nothing about workgroup -> XCD placement; what is OBSERVED on MI355X is round-robin dealing (workgroup b on XCD
// (b + c) % 8 for some c that changes from launch to launch).  coo_segscan_bins_kernel (workgroup w scans bin w % 8) and the
// panel kernel's per-XCD bookkeeping lean on "b and b + 8 share an XCD" for speed.  This probe checks it once per context:
// 2048 workgroups write the XCC_ID hardware register (bits 3:0 of hwreg 20 on gfx942 / gfx950); the host requires that equal
// labels b % 8 saw ONE id each and different labels different ids.
namespace
{
__global__ void xcd_probe_kernel(int* __restrict__ out)
{
    if (threadIdx.x == 0) out[blockIdx.x] = (int)__builtin_amdgcn_s_getreg((3 << 11) | (0 << 6) | 20);  // GETREG_IMMED(size - 1, offset, XCC_ID)
}
}  // namespace

static void xcd_probe(spmv_ctx* ctx)
{
    constexpr int kProbeBlocks = 2048;
    ctx->xcd_round_robin = -1;
    if (ensure_scratch(ctx, sizeof(int) * kProbeBlocks) != SPMV_OK) return;
    int* d = (int*)ctx->scratch;
    std::vector<int> h(kProbeBlocks, -1);
    hipLaunchKernelGGL(xcd_probe_kernel, dim3(kProbeBlocks), dim3(64), 0, ctx->stream, d);
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(h.data(), d, sizeof(int) * kProbeBlocks, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
        hipStreamSynchronize(ctx->stream) != hipSuccess)
    {
        (void)hipGetLastError();
        return;
    }
    int  id_of_label[8];
    bool ok = true;
    unsigned seen = 0;
    for (int b = 0; b < kProbeBlocks; ++b)
    {
        seen |= 1u << (h[b] & 15);
        if (b < 8)
            id_of_label[b] = h[b];
        else if (h[b] != id_of_label[b & 7])
            ok = false;
    }
    for (int a = 0; a < 8 && ok; ++a)
        for (int b = a + 1; b < 8; ++b)
            if (id_of_label[a] == id_of_label[b]) ok = false;
    ctx->xcds_seen       = __builtin_popcount(seen);
    ctx->xcd_round_robin = ok ? 1 : 0;
}

// ---- may the CPU store x straight into device memory? --------------------------------------------------------------------------
// spmv_apply_host writes a small x into its device buffer with memcpy where the device reports a large BAR.  The attribute says
// the memory is mapped; that a KERNEL sees such stores (write-combining buffers drained, HDP flushed, no stale line in L2) is
// checked here once per context before the path is switched on: 512 doubles stored by the CPU, summed by a kernel, twice with
// different contents.  A mismatch (or any error) leaves large_bar off and x goes through the pinned staging buffer instead.
namespace
{
__global__ void host_store_probe_kernel(const double* __restrict__ in, int n, double* __restrict__ out)
{
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 64) s += in[i];
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if (threadIdx.x == 0) *out = s;
}
}  // namespace

static bool host_stores_reach_kernels(spmv_ctx* ctx)
{
    constexpr int kN = 512;
    double* buf = nullptr;
    if (hipMalloc((void**)&buf, sizeof(double) * kN) != hipSuccess)
    {
        (void)hipGetLastError();
        return false;
    }
    bool   ok = true;
    double host[kN];
    for (int round = 0; round < 2 && ok; ++round)
    {
        double want = 0.0;
        for (int i = 0; i < kN; ++i)
        {
            host[i] = (double)((i * 7 + round * 13) % 32) + (round ? 0.5 : 0.25);  // (sums of these are exact in fp64 in any order)
            want += host[i];
        }
        memcpy(buf, host, sizeof(host));
        __sync_synchronize();
        if (ctx->hdp_flush) *ctx->hdp_flush = 1u;
        hipLaunchKernelGGL(host_store_probe_kernel, dim3(1), dim3(64), 0, ctx->stream, buf, kN, ctx->dev_scalars);
        double got = -1.0;
        if (hipGetLastError() != hipSuccess || hipMemcpyAsync(&got, ctx->dev_scalars, sizeof(double), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
            hipStreamSynchronize(ctx->stream) != hipSuccess)
        {
            (void)hipGetLastError();
            ok = false;
        }
        else
            ok = got == want;
    }
    (void)hipFree(buf);
    return ok;
}

int spmv_ctx_xcd_round_robin(spmv_ctx* ctx, int32_t* round_robin, int32_t* xcds_seen)
{
    SPMV_REQUIRE(ctx, "ctx is null");
    if (round_robin) *round_robin = ctx->xcd_round_robin;
    if (xcds_seen) *xcds_seen = ctx->xcds_seen;
    return SPMV_OK;
}

int spmv_ctx_get_param(const spmv_ctx* ctx, const char* name, int64_t* value)
{
    SPMV_REQUIRE(ctx && name && value, "spmv_ctx_get_param: null argument");
    if (!strcmp(name, "host_stores"))
        *value = ctx->large_bar ? 1 : 0;
    else if (!strcmp(name, "xcd_round_robin"))
        *value = ctx->xcd_round_robin;
    else if (!strcmp(name, "xcds_seen"))
        *value = ctx->xcds_seen;
    else if (!strcmp(name, "trial_arena_bytes"))
        *value = (int64_t)ctx->arena_bytes;
    else if (!strcmp(name, "cg_graph_replays"))
        *value = ctx->cg_graph_replays;
    else
        SPMV_FAIL(SPMV_ERR_INVALID, "unknown context parameter '%s'", name);
    return SPMV_OK;
}

int spmv_ctx_create(int device, spmv_ctx** out) { return ctx_create_common(device, nullptr, false, out); }
int spmv_ctx_create_on_stream(int device, void* hip_stream, spmv_ctx** out)
{
    return ctx_create_common(device, hip_stream, true, out);
}

int spmv_ctx_destroy(spmv_ctx* ctx)
{
    if (!ctx) return SPMV_OK;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    if (ctx->scratch) (void)hipFree(ctx->scratch);
    block_ops_free(ctx);
    if (ctx->arena) (void)hipFree(ctx->arena);
    if (ctx->stage_x) (void)hipFree(ctx->stage_x);
    if (ctx->stage_y) (void)hipFree(ctx->stage_y);
    if (ctx->stage_pinned) (void)hipHostFree(ctx->stage_pinned);
    if (ctx->host_pinned) (void)hipHostFree(ctx->host_pinned);
    if (ctx->dev_scalars) (void)hipFree(ctx->dev_scalars);
    if (ctx->ev_begin) (void)hipEventDestroy(ctx->ev_begin);
    if (ctx->ev_end) (void)hipEventDestroy(ctx->ev_end);
    if (ctx->owns_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
    return SPMV_OK;
}

int spmv_ctx_mem_info(spmv_ctx* ctx, int64_t* free_bytes, int64_t* total_bytes)
{
    SPMV_REQUIRE(ctx && free_bytes && total_bytes, "spmv_ctx_mem_info: null argument");
    SPMV_HIP(hipSetDevice(ctx->device));
    size_t f = 0, t = 0;
    SPMV_HIP(hipMemGetInfo(&f, &t));
    *free_bytes  = (int64_t)f;
    *total_bytes = (int64_t)t;
    return SPMV_OK;
}

int spmv_sync(spmv_ctx* ctx)
{
    SPMV_REQUIRE(ctx, "ctx is null");
    SPMV_HIP(hipStreamSynchronize(ctx->stream));
    return SPMV_OK;
}

int spmv_ctx_device(const spmv_ctx* ctx, int* device)
{
    SPMV_REQUIRE(ctx && device, "null argument");
    *device = ctx->device;
    return SPMV_OK;
}

// ---- vectors ----------------------------------------------------------------------------------------------
int spmv_vec_create(spmv_ctx* ctx, int64_t n, spmv_vec** out)
{
    SPMV_REQUIRE(ctx && out && n >= 0, "spmv_vec_create: bad argument");
    SPMV_TRY(use_device(ctx));
    spmv_vec* v = new (std::nothrow) spmv_vec();
    if (!v) SPMV_FAIL(SPMV_ERR_ALLOC, "out of host memory");
    hipError_t e = hipMalloc((void**)&v->d, std::max<int64_t>(n, 1) * sizeof(double));
    if (e != hipSuccess)
    {
        delete v;
        SPMV_FAIL(SPMV_ERR_ALLOC, "device allocation of %lld fp64 failed: %s", (long long)n, hipGetErrorString(e));
    }
    v->ctx   = ctx;
    v->n     = n;
    v->owned = true;
    *out     = v;
    return SPMV_OK;
}

int spmv_vec_wrap_device(spmv_ctx* ctx, int64_t n, double* device_ptr, spmv_vec** out)
{
    SPMV_REQUIRE(ctx && out && n >= 0 && (device_ptr || n == 0), "spmv_vec_wrap_device: bad argument");
    spmv_vec* v = new (std::nothrow) spmv_vec();
    if (!v) SPMV_FAIL(SPMV_ERR_ALLOC, "out of host memory");
    v->ctx   = ctx;
    v->n     = n;
    v->d     = device_ptr;
    v->owned = false;
    *out     = v;
    return SPMV_OK;
}

int spmv_vec_destroy(spmv_vec* v)
{
    if (!v) return SPMV_OK;
    if (v->owned && v->d)
    {
        (void)hipSetDevice(v->ctx->device);
        (void)hipFree(v->d);
    }
    delete v;
    return SPMV_OK;
}

int spmv_vec_size(const spmv_vec* v, int64_t* n)
{
    SPMV_REQUIRE(v && n, "null argument");
    *n = v->n;
    return SPMV_OK;
}

int spmv_vec_device_ptr(const spmv_vec* v, double** device_ptr)
{
    SPMV_REQUIRE(v && device_ptr, "null argument");
    *device_ptr = v->d;
    return SPMV_OK;
}

int spmv_vec_upload(spmv_vec* v, int64_t offset, int64_t n, const double* host)
{
    SPMV_REQUIRE(v && offset >= 0 && n >= 0 && offset + n <= v->n && (host || n == 0),
                 "spmv_vec_upload: range [%lld,+%lld) outside vector of %lld", (long long)offset, (long long)n,
                 v ? (long long)v->n : -1LL);
    SPMV_TRY(use_device(v->ctx));
    return upload(v->d + offset, host, (size_t)n * sizeof(double), v->ctx);
}

int spmv_vec_download(const spmv_vec* v, int64_t offset, int64_t n, double* host)
{
    SPMV_REQUIRE(v && offset >= 0 && n >= 0 && offset + n <= v->n && (host || n == 0),
                 "spmv_vec_download: range [%lld,+%lld) outside vector of %lld", (long long)offset, (long long)n,
                 v ? (long long)v->n : -1LL);
    if (n == 0) return SPMV_OK;
    SPMV_TRY(use_device(v->ctx));
    SPMV_HIP(hipMemcpyAsync(host, v->d + offset, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, v->ctx->stream));
    SPMV_HIP(hipStreamSynchronize(v->ctx->stream));
    return SPMV_OK;
}

int spmv_vec_fill(spmv_vec* v, double a)
{
    SPMV_REQUIRE(v, "null vector");
    SPMV_TRY(use_device(v->ctx));
    return vec_fill(v->ctx, v->d, v->n, a);
}

// ---- matrices ---------------------------------------------------------------------------------------------
int spmv_csr_upload(spmv_ctx* ctx, int32_t nrow, int32_t ncol, const int32_t* row_ptr, const int32_t* col_ind,
                    const double* values, spmv_mat** out)
{
    SPMV_REQUIRE(ctx && out && nrow >= 0 && ncol >= 0 && row_ptr, "spmv_csr_upload: bad argument");
    const int64_t nnz = (int64_t)row_ptr[nrow] - row_ptr[0];
    SPMV_REQUIRE(row_ptr[0] == 0 && nnz >= 0 && (nnz == 0 || (col_ind && values)),
                 "spmv_csr_upload: row_ptr[0]=%d, nnz=%lld", row_ptr[0], (long long)nnz);
    SPMV_TRY(use_device(ctx));
    plan_arm arm(ctx);
    spmv_mat* m = nullptr;
    SPMV_TRY(mat_alloc(ctx, SPMV_FMT_CSR, nrow, ncol, nnz, 0, (size_t)nrow + 1, (size_t)nnz, (size_t)nnz, &m));
    SPMV_TRY(upload_arrays(m, row_ptr, (size_t)nrow + 1, col_ind, (size_t)nnz, values, (size_t)nnz));
    return finish(m, out);
}

int spmv_csr_wrap_device(spmv_ctx* ctx, int32_t nrow, int32_t ncol, const int32_t* d_row_ptr, const int32_t* d_col_ind,
                         const double* d_values, spmv_mat** out)
{
    SPMV_REQUIRE(ctx && out && nrow >= 0 && ncol >= 0 && d_row_ptr, "spmv_csr_wrap_device: bad argument");
    SPMV_TRY(use_device(ctx));
    plan_arm arm(ctx);
    int32_t ends[2] = {0, 0};
    SPMV_HIP(hipMemcpyAsync(&ends[0], d_row_ptr, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    SPMV_HIP(hipMemcpyAsync(&ends[1], d_row_ptr + nrow, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    SPMV_HIP(hipStreamSynchronize(ctx->stream));
    SPMV_REQUIRE(ends[0] == 0 && ends[1] >= 0, "spmv_csr_wrap_device: row_ptr[0]=%d row_ptr[nrow]=%d", ends[0], ends[1]);
    spmv_mat* m = nullptr;
    SPMV_TRY(wrap(ctx, SPMV_FMT_CSR, nrow, ncol, ends[1], 0, d_row_ptr, d_col_ind, d_values, &m));
    return finish(m, out);
}

int spmv_csr_upload_shard(spmv_ctx* ctx, int64_t row_begin, int64_t row_end, int32_t ncol, const int64_t* row_ptr64,
                          const int32_t* col_ind, const double* values, spmv_mat** out)
{
    SPMV_REQUIRE(ctx && out && row_ptr64 && row_begin >= 0 && row_end >= row_begin && row_end - row_begin <= INT32_MAX,
                 "spmv_csr_upload_shard: bad row range");
    const int32_t nrow = (int32_t)(row_end - row_begin);
    const int64_t base = row_ptr64[row_begin];
    const int64_t nnz  = row_ptr64[row_end] - base;
    SPMV_REQUIRE(nnz >= 0 && nnz <= INT32_MAX, "spmv_csr_upload_shard: shard holds %lld entries (int32 offsets)",
                 (long long)nnz);
    SPMV_TRY(use_device(ctx));
    plan_arm arm(ctx);
    // rebase exactly like src/mat_vec.cpp:260-263
    std::vector<int32_t> sub((size_t)nrow + 1);
    for (int32_t j = 0; j <= nrow; ++j) sub[j] = (int32_t)(row_ptr64[row_begin + j] - base);
    spmv_mat* m = nullptr;
    SPMV_TRY(mat_alloc(ctx, SPMV_FMT_CSR, nrow, ncol, nnz, 0, (size_t)nrow + 1, (size_t)nnz, (size_t)nnz, &m));
    SPMV_TRY(upload_arrays(m, sub.data(), sub.size(), col_ind + base, (size_t)nnz, values + base, (size_t)nnz));
    m->row_begin = row_begin;
    return finish(m, out);
}

int spmv_coo_upload(spmv_ctx* ctx, int32_t nrow, int32_t ncol, int64_t nnz, const int32_t* row_ind,
                    const int32_t* col_ind, const double* values, spmv_mat** out)
{
    SPMV_REQUIRE(ctx && out && nrow >= 0 && ncol >= 0 && nnz >= 0 && (nnz == 0 || (row_ind && col_ind && values)),
                 "spmv_coo_upload: bad argument");
    SPMV_TRY(use_device(ctx));
    plan_arm arm(ctx);
    spmv_mat* m = nullptr;
    SPMV_TRY(mat_alloc(ctx, SPMV_FMT_COO, nrow, ncol, nnz, 0, (size_t)nnz, (size_t)nnz, (size_t)nnz, &m));
    SPMV_TRY(upload_arrays(m, row_ind, (size_t)nnz, col_ind, (size_t)nnz, values, (size_t)nnz));
    return finish(m, out);
}

int spmv_coo_wrap_device(spmv_ctx* ctx, int32_t nrow, int32_t ncol, int64_t nnz, const int32_t* d_row_ind,
                         const int32_t* d_col_ind, const double* d_values, spmv_mat** out)
{
    SPMV_REQUIRE(ctx && out && nrow >= 0 && ncol >= 0 && nnz >= 0, "spmv_coo_wrap_device: bad argument");
    SPMV_TRY(use_device(ctx));
    plan_arm arm(ctx);
    spmv_mat* m = nullptr;
    SPMV_TRY(wrap(ctx, SPMV_FMT_COO, nrow, ncol, nnz, 0, d_row_ind, d_col_ind, d_values, &m));
    return finish(m, out);
}

int spmv_ell_upload(spmv_ctx* ctx, int32_t nrow, int32_t ncol, int32_t k, int64_t nnz, const int32_t* col_ind,
                    const double* values, spmv_mat** out)
{
    SPMV_REQUIRE(ctx && out && nrow >= 0 && ncol >= 0 && k >= 0, "spmv_ell_upload: bad argument");
    const size_t total = (size_t)nrow * (size_t)k;
    SPMV_REQUIRE(total == 0 || (col_ind && values), "spmv_ell_upload: null arrays");
    SPMV_TRY(use_device(ctx));
    plan_arm arm(ctx);
    spmv_mat* m = nullptr;
    SPMV_TRY(mat_alloc(ctx, SPMV_FMT_ELL, nrow, ncol, nnz, k, 0, total, total, &m));
    SPMV_TRY(upload_arrays(m, nullptr, 0, col_ind, total, values, total));
    m->max_row_nnz = k;
    return finish(m, out);
}

int spmv_ell_wrap_device(spmv_ctx* ctx, int32_t nrow, int32_t ncol, int32_t k, int64_t nnz, const int32_t* d_col_ind,
                         const double* d_values, spmv_mat** out)
{
    SPMV_REQUIRE(ctx && out && nrow >= 0 && ncol >= 0 && k >= 0, "spmv_ell_wrap_device: bad argument");
    plan_arm arm(ctx);
    spmv_mat* m = nullptr;
    SPMV_TRY(wrap(ctx, SPMV_FMT_ELL, nrow, ncol, nnz, k, nullptr, d_col_ind, d_values, &m));
    m->max_row_nnz = k;
    return finish(m, out);
}

int spmv_csc_upload(spmv_ctx* ctx, int32_t nrow, int32_t ncol, const int32_t* col_ptr, const int32_t* row_ind,
                    const double* values, spmv_mat** out)
{
    SPMV_REQUIRE(ctx && out && nrow >= 0 && ncol >= 0 && col_ptr, "spmv_csc_upload: bad argument");
    const int64_t nnz = (int64_t)col_ptr[ncol];
    SPMV_REQUIRE(col_ptr[0] == 0 && nnz >= 0 && (nnz == 0 || (row_ind && values)), "spmv_csc_upload: bad col_ptr");
    SPMV_TRY(use_device(ctx));
    plan_arm arm(ctx);
    spmv_mat* m = nullptr;
    SPMV_TRY(mat_alloc(ctx, SPMV_FMT_CSC, nrow, ncol, nnz, 0, (size_t)ncol + 1, (size_t)nnz, (size_t)nnz, &m));
    SPMV_TRY(upload_arrays(m, col_ptr, (size_t)ncol + 1, row_ind, (size_t)nnz, values, (size_t)nnz));
    return finish(m, out);
}

int spmv_dia_upload(spmv_ctx* ctx, int32_t nrow, int32_t ncol, int32_t ndiags, const int32_t* offsets,
                    const double* values, spmv_mat** out)
{
    SPMV_REQUIRE(ctx && out && nrow >= 0 && ncol >= 0 && ndiags >= 0, "spmv_dia_upload: bad argument");
    const size_t total = (size_t)nrow * (size_t)ndiags;
    SPMV_REQUIRE(ndiags == 0 || offsets, "spmv_dia_upload: null offsets");
    SPMV_REQUIRE(total == 0 || values, "spmv_dia_upload: null values");
    SPMV_TRY(use_device(ctx));
    spmv_mat* m = nullptr;
    SPMV_TRY(mat_alloc(ctx, SPMV_FMT_DIA, nrow, ncol, 0, ndiags, (size_t)ndiags, 0, total, &m));
    if (ndiags > 0)
    {
        m->dia_off_known = true;
        m->dia_off_min   = *std::min_element(offsets, offsets + ndiags);
        m->dia_off_max   = *std::max_element(offsets, offsets + ndiags);
    }
    SPMV_TRY(upload_arrays(m, offsets, (size_t)ndiags, nullptr, 0, values, total));
    return finish(m, out);
}

// ---- block CSR: k holds bs, nnz the stored values (blocks * bs * bs) ------------------------------------------------------------
static int check_bsr_shape(const char* who, const spmv_ctx* ctx, const void* out, int32_t nrow, int32_t ncol, int32_t bs, const int32_t* brow_ptr)
{
    SPMV_REQUIRE(ctx && out && brow_ptr, "%s: null argument", who);
    SPMV_REQUIRE(nrow >= 0 && ncol >= 0 && nrow <= INT32_MAX - 64 && ncol <= INT32_MAX - 64, "%s: bad size %d x %d", who, nrow, ncol);
    return bsr_check_bs(bs, who);
}

int spmv_bsr_upload(spmv_ctx* ctx, int32_t nrow, int32_t ncol, int32_t bs, const int32_t* brow_ptr, const int32_t* bcol, const double* values,
                    spmv_mat** out)
{
    SPMV_TRY(check_bsr_shape("spmv_bsr_upload", ctx, out, nrow, ncol, bs, brow_ptr));
    const int64_t mb = ceil_div(nrow, bs), nnzb = (int64_t)brow_ptr[mb] - brow_ptr[0];
    SPMV_REQUIRE(brow_ptr[0] == 0 && nnzb >= 0 && (nnzb == 0 || (bcol && values)), "spmv_bsr_upload: brow_ptr[0]=%d, %lld blocks", brow_ptr[0], (long long)nnzb);
    SPMV_TRY(use_device(ctx));
    plan_arm  arm(ctx);
    spmv_mat* m = nullptr;
    SPMV_TRY(mat_alloc(ctx, SPMV_FMT_BSR, nrow, ncol, nnzb * bs * bs, bs, (size_t)mb + 1, (size_t)nnzb, (size_t)(nnzb * bs * bs), &m));
    SPMV_TRY(upload_arrays(m, brow_ptr, (size_t)mb + 1, bcol, (size_t)nnzb, values, (size_t)(nnzb * bs * bs)));
    return finish(m, out);
}

int spmv_bsr_wrap_device(spmv_ctx* ctx, int32_t nrow, int32_t ncol, int32_t bs, const int32_t* d_brow_ptr, const int32_t* d_bcol,
                         const double* d_values, spmv_mat** out)
{
    SPMV_TRY(check_bsr_shape("spmv_bsr_wrap_device", ctx, out, nrow, ncol, bs, d_brow_ptr));
    SPMV_TRY(use_device(ctx));
    plan_arm      arm(ctx);
    const int64_t mb      = ceil_div(nrow, bs);
    int32_t       ends[2] = {0, 0};
    SPMV_HIP(hipMemcpyAsync(&ends[0], d_brow_ptr, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    SPMV_HIP(hipMemcpyAsync(&ends[1], d_brow_ptr + mb, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    SPMV_HIP(hipStreamSynchronize(ctx->stream));
    SPMV_REQUIRE(ends[0] == 0 && ends[1] >= 0 && (ends[1] == 0 || (d_bcol && d_values)), "spmv_bsr_wrap_device: brow_ptr[0]=%d brow_ptr[mb]=%d", ends[0], ends[1]);
    spmv_mat* m = nullptr;
    SPMV_TRY(wrap(ctx, SPMV_FMT_BSR, nrow, ncol, (int64_t)ends[1] * bs * bs, bs, d_brow_ptr, d_bcol, d_values, &m));
    return finish(m, out);
}

int spmv_csr_to_bsr(spmv_ctx* ctx, const spmv_mat* csr, int32_t bs, spmv_mat** out_bsr)
{
    SPMV_REQUIRE(ctx && csr && out_bsr, "spmv_csr_to_bsr: null argument");
    SPMV_TRY(csr_to_bsr_check(ctx, csr, bs, "spmv_csr_to_bsr"));
    SPMV_TRY(use_device(ctx));
    plan_arm  arm(ctx);
    spmv_mat* m = nullptr;
    SPMV_TRY(csr_to_bsr(ctx, csr, bs, &m));
    return finish(m, out_bsr);  // validates and analyses like an uploaded handle (frees on failure)
}

int spmv_bsr_to_csr(spmv_ctx* ctx, const spmv_mat* bsr, int32_t drop_zeros, spmv_mat** out_csr)
{
    SPMV_REQUIRE(ctx && bsr && out_csr, "spmv_bsr_to_csr: null argument");
    SPMV_TRY(bsr_to_csr_check(ctx, bsr, "spmv_bsr_to_csr"));
    SPMV_TRY(use_device(ctx));
    plan_arm  arm(ctx);
    spmv_mat* m = nullptr;
    SPMV_TRY(bsr_to_csr(ctx, bsr, drop_zeros, &m));
    return finish(m, out_csr);
}

// ---- CSR with single-precision value storage (format 6): the handle keeps the row pointer and one stream of packed entries ---------
int spmv_csr_to_f32(spmv_ctx* ctx, const spmv_mat* csr, spmv_mat** out_f32)
{
    SPMV_REQUIRE(ctx && csr && out_f32, "spmv_csr_to_f32: null argument");
    SPMV_TRY(csr_to_f32_check(ctx, csr, "spmv_csr_to_f32"));
    SPMV_TRY(use_device(ctx));
    spmv_mat* m = nullptr;
    SPMV_TRY(csr_to_f32(ctx, csr, "spmv_csr_to_f32", &m));
    return finish(m, out_f32);  // validates and analyses like an uploaded handle (frees on failure)
}

int spmv_csr_f32_upload(spmv_ctx* ctx, int32_t nrow, int32_t ncol, const int32_t* row_ptr, const int32_t* col_ind, const float* values, spmv_mat** out)
{
    SPMV_REQUIRE(ctx && out && row_ptr, "spmv_csr_f32_upload: null argument");
    SPMV_REQUIRE(nrow >= 0 && ncol >= 0, "spmv_csr_f32_upload: bad size %d x %d", nrow, ncol);
    const int64_t nnz = (int64_t)row_ptr[nrow] - row_ptr[0];
    SPMV_REQUIRE(row_ptr[0] == 0 && nnz >= 0 && (nnz == 0 || (col_ind && values)), "spmv_csr_f32_upload: row_ptr[0]=%d, nnz=%lld", row_ptr[0], (long long)nnz);
    SPMV_TRY(use_device(ctx));
    spmv_mat* m = nullptr;
    SPMV_TRY(csr_f32_from_host(ctx, nrow, ncol, nnz, row_ptr, col_ind, values, &m));
    return finish(m, out);
}

int spmv_f32_to_csr(spmv_ctx* ctx, const spmv_mat* f32, spmv_mat** out_csr)
{
    SPMV_REQUIRE(ctx && f32 && out_csr, "spmv_f32_to_csr: null argument");
    SPMV_TRY(f32_to_csr_check(ctx, f32, "spmv_f32_to_csr"));
    SPMV_TRY(use_device(ctx));
    plan_arm  arm(ctx);
    spmv_mat* m = nullptr;
    SPMV_TRY(f32_to_csr(ctx, f32, "spmv_f32_to_csr", &m));
    return finish(m, out_csr);
}

int spmv_f32_info(const spmv_mat* f32, int64_t* inexact, int64_t* underflow, double* max_rel_err)
{
    SPMV_REQUIRE(f32, "spmv_f32_info: null matrix");
    if (f32->format != SPMV_FMT_CSR_F32) SPMV_FAIL(SPMV_ERR_UNSUPPORTED, "spmv_f32_info: the input must be a handle of format 6 (format %d)", f32->format);
    if (inexact) *inexact = f32->f32_inexact;
    if (underflow) *underflow = f32->f32_underflow;
    if (max_rel_err) *max_rel_err = f32->f32_max_rel;
    return SPMV_OK;
}

int spmv_mat_destroy(spmv_mat* m)
{
    if (!m) return SPMV_OK;
    (void)hipSetDevice(m->ctx->device);
    (void)hipStreamSynchronize(m->ctx->stream);
    mat_free(m);
    return SPMV_OK;
}

int spmv_mat_validate(const spmv_mat* m)
{
    SPMV_REQUIRE(m, "null matrix");
    SPMV_TRY(use_device(m->ctx));
    return mat_validate(m);
}

int spmv_mat_get_info(const spmv_mat* m, spmv_mat_info* info)
{
    SPMV_REQUIRE(m && info, "null argument");
    info->format        = m->format;
    info->nrow          = m->nrow;
    info->ncol          = m->ncol;
    info->ell_k         = m->k;
    info->nnz           = m->nnz;
    info->row_begin     = m->row_begin;
    info->max_row_nnz   = m->max_row_nnz;
    info->kernel        = m->kernel;
    info->lanes_per_row = m->lanes_per_row;
    info->sorted_rows   = m->sorted_rows;
    info->device_bytes  = m->device_bytes;
    return SPMV_OK;
}

int spmv_mat_set_kernel(spmv_mat* m, int32_t kernel, int32_t lanes_per_row)
{
    SPMV_REQUIRE(m, "null matrix");
    SPMV_REQUIRE(kernel >= SPMV_CSR_AUTO && kernel <= SPMV_CSR_ELL, "unknown kernel id %d", kernel);
    if (m->format == SPMV_FMT_BSR) return bsr_set_kernel(m, kernel, lanes_per_row);  // (its lanes per block row are multiples of bs * bs)
    if (m->format == SPMV_FMT_CSR_F32) return csr_f32_set_kernel(m, kernel, lanes_per_row);  // (one kernel; anything else: UNSUPPORTED)
    SPMV_REQUIRE(lanes_per_row == 0 || (lanes_per_row >= 1 && lanes_per_row <= 64 &&
                                        (lanes_per_row & (lanes_per_row - 1)) == 0),
                 "lanes_per_row must be 0 or a power of two in 1..64, got %d", lanes_per_row);
    if (lanes_per_row > 0) m->lanes_per_row = lanes_per_row;
    // COO, CSC, ELL: the format's own kernel or the row-grouped copy (rowgrouped.hip)
    if (m->format == SPMV_FMT_COO || m->format == SPMV_FMT_CSC || m->format == SPMV_FMT_ELL) return rowgrouped_set_kernel(m, kernel);
    if (m->format == SPMV_FMT_CSR && m->nnz > 0 && (!m->b || !m->v))
        SPMV_REQUIRE(csr_layout_built(m, kernel) || (kernel == SPMV_CSR_AUTO && kernel_reads_own_layout(m->kernel)),
                     "this handle gave up its CSR arrays (panel_keep_csr = 0): only the product it was built for is left");
    if (kernel == SPMV_CSR_AUTO)
    {
        m->kernel_forced = false;
        if (m->format == SPMV_FMT_CSR && m->b && m->v)
        {
            SPMV_HIP(hipSetDevice(m->ctx->device));
            return csr_select_kernel(m);  // the model and, where it pays, a trial of the candidates (select.hip); builds what it picks
        }
    }
    else
    {
        m->kernel         = kernel;
        m->kernel_forced  = true;
        m->split_auto_low = false;  // (a forced SPLIT takes "split_row_threshold" or its default, not what AUTO found)
    }
    if (m->format != SPMV_FMT_CSR)  // a DIA handle: it has one kernel, and no layout of a CSR kernel to free or build
    {
        SPMV_REQUIRE(m->kernel != SPMV_CSR_SEGSCAN, "kernel SEGSCAN (6) is a CSR kernel (a COO handle's VECTOR is the same scan)");
        SPMV_REQUIRE(m->kernel != SPMV_CSR_SPLIT, "kernel SPLIT (7) is a CSR kernel");
        SPMV_REQUIRE(m->kernel != SPMV_CSR_ELL, "kernel ELL (8) is a CSR kernel: the ELL copy of a CSR handle");
        return SPMV_OK;
    }
    // a built panel or two-phase layout is KEPT under another kernel (device_bytes and panel_bytes go on counting it); the other three go
    csr_layouts_free(m, ((1u << SPMV_CSR_SEGSCAN) | (1u << SPMV_CSR_SPLIT) | (1u << SPMV_CSR_ELL)) & ~(1u << m->kernel));
    SPMV_HIP(hipSetDevice(m->ctx->device));
    return csr_layout_build(m, m->kernel);  // (re)build with the current parameters
}

int spmv_mat_set_param(spmv_mat* m, const char* name, int64_t value)
{
    SPMV_REQUIRE(m && name, "null argument");
    if (int rc = SPMV_OK; ell_set_param(m, name, value, &rc)) return rc;  // "ell_tiled_values", "ell_dia_order"
    for (const precond_row& P : kPreconds)  // the preconditioners' own, each by its unit's hook; they take effect at the next set-up
        if (int rc = SPMV_OK; P.set_param && P.set_param(m, name, value, &rc)) return rc;
    if (!strcmp(name, "panel_rows"))
        m->pb_group_rows = (int32_t)value;
    else if (!strcmp(name, "panel_width"))
        m->pb_panel_width = (int32_t)value;
    else if (!strcmp(name, "panel_sort"))
        m->pb_sort = (int32_t)value;
    else if (!strcmp(name, "panel_unroll"))
        m->pb_unroll = (int32_t)value;
    else if (!strcmp(name, "panel_aos"))
        m->pb_aos = (int32_t)value;
    else if (!strcmp(name, "panel_pipe"))
        m->pb_pipe = (int32_t)value;
    else if (!strcmp(name, "panel_two_per_cu"))
        m->pb_two_per_cu = (int32_t)value;
    else if (!strcmp(name, "panel_rounds"))
    {
        SPMV_REQUIRE(value >= 0 && value <= 16, "panel_rounds must be 0 (automatic), 1 (the fewest groups) or a multiple up to 16, got %lld", (long long)value);
        m->pb_rounds_req = (int32_t)value;
    }
    else if (!strcmp(name, "split_row_threshold"))
    {
        // rows of this many entries and more are "long" under kernel SPLIT (0: the default); takes effect at the next spmv_mat_set_kernel
        SPMV_REQUIRE(value >= 0 && value <= INT32_MAX, "split_row_threshold must be 0 (default) or a row length, got %lld", (long long)value);
        m->split_threshold = (int32_t)value;
    }
    else if (!strcmp(name, "split_mode"))
    {
        // how kernel SPLIT runs its long rows: 1 chunks of 4096 entries over the handle's own arrays, 2 virtual rows of 64 entries in a
        // matrix of their own, 0 by their density (kernels_csr_split.hip); takes effect at the next spmv_mat_set_kernel
        SPMV_REQUIRE(value >= 0 && value <= 2, "split_mode must be 0 (by density), 1 (chunks) or 2 (virtual rows), got %lld", (long long)value);
        m->split_mode = (int32_t)value;
    }
    else if (!strcmp(name, "panel_keep_csr"))
    {
        // 0: release col_ind / values of a CSR handle whose product runs from the panel layout (which holds the same
        // entries re-ordered; row_ptr stays).  Memory goes from 2x to 1x the matrix; what needs the arrays afterwards
        // (download, another kernel, a re-build with other parameters, conversions, the Jacobi diagonal) is refused.
        SPMV_REQUIRE(value == 0 || (m->b && m->v) || m->nnz == 0, "panel_keep_csr: the arrays are gone already");
        if (value == 0 && m->b && m->v)
        {
            SPMV_REQUIRE(m->format == SPMV_FMT_CSR && m->owned && csr_layout_built(m, m->kernel),
                         "panel_keep_csr = 0 needs an owned CSR handle whose panel or two-phase layout or ELL copy is built");
            SPMV_HIP(hipSetDevice(m->ctx->device));
            SPMV_HIP(hipStreamSynchronize(m->ctx->stream));
            transpose_free(m);  // (its companion reads the arrays released here)
            // a two-phase handle first offers the gigabytes it is about to release to its product stream's piece search
            // (kernels_csr_twophase.hip: memory of another moment of the allocator's history, at no transient cost)
            bool keep_b = false, keep_v = false;
            if (m->kernel == SPMV_CSR_TWOPHASE) SPMV_TRY(csr_twophase_offer_csr_copy(m, &keep_b, &keep_v));
            if (!keep_b) (void)hipFree(const_cast<int32_t*>(m->b));
            if (!keep_v) (void)hipFree(const_cast<double*>(m->v));
            m->b = nullptr;
            m->v = nullptr;
            m->device_bytes -= m->nnz * 12;
        }
    }
    else if (!strcmp(name, "coo_column_bins"))
    {
        // COO, segmented scan: bins per XCD of the copy the scan runs over (1..8), 0 = no copy (the scan reads the handle's
        // own arrays in their order), -1 = as many as keep a slice of x inside an XCD's L2
        SPMV_REQUIRE(m->format == SPMV_FMT_COO && value >= -1 && value <= 8, "coo_column_bins: a COO handle and -1 .. 8");
        SPMV_HIP(hipSetDevice(m->ctx->device));
        SPMV_HIP(hipStreamSynchronize(m->ctx->stream));
        if (value == 0)
            coo_free_bins(m);
        else
            SPMV_TRY(coo_build_bins(m, value < 0 ? 0 : (int)value, /*only_if_worth=*/false));
    }
    else if (!strcmp(name, "dia_col_bound"))
    {
        SPMV_REQUIRE(m->format == SPMV_FMT_DIA && value >= 0 && value <= m->ncol, "dia_col_bound: a DIA handle and 0 <= bound <= ncol");
        m->dia_col_bound = (int32_t)value;
    }
    else if (!strcmp(name, "transpose_kernel"))  // the companion's kernel (transpose.hip); takes effect at the next set-up
        SPMV_TRY(transpose_set_kernel(m, value));
    else if (!strcmp(name, "panel_sync"))
        m->pb_sync = (int32_t)value;
    else if (!strcmp(name, "twophase_offer_csr_copy"))
        m->tp_offer_csr = value < 0 || value > 2 ? 1 : (int32_t)value;  // (2: tests - a carved piece is taken whatever the timings say)
    else if (!strcmp(name, "panel_trial"))
        m->pb_trial = (int32_t)value;
    else if (!strcmp(name, "twophase_panel_cols"))  // takes effect at the next spmv_mat_set_kernel(TWOPHASE)
        m->tp_pcols_req = (int32_t)value;
    else if (!strcmp(name, "twophase_placement_budget_mb"))
    {
        // memory (MB) the piece search of the two-phase layout may hold beyond the product stream while it runs; 0 = no
        // search; -1 = the default (SPMV_TP_PLACEMENT_BUDGET_MB or 8192).  Takes effect at the next spmv_mat_set_kernel(TWOPHASE)
        // that builds the layout.
        SPMV_REQUIRE(value >= -1 && value <= (1 << 20), "twophase_placement_budget_mb: -1 (default), 0 (no search) or megabytes");
        m->tp_place_budget_mb = (int32_t)value;
    }
    else if (!strcmp(name, "twophase_pool_alloc") || !strcmp(name, "twophase_pool_config"))  // experiments (tools/probe_twophase_pairs.py)
    {
        const char* e_exp = getenv("SPMV_EXPERIMENTS");
        SPMV_REQUIRE(e_exp && e_exp[0] == '1', "%s is an experiment: set SPMV_EXPERIMENTS=1", name);
        SPMV_HIP(hipSetDevice(m->ctx->device));
        if (!strcmp(name, "twophase_pool_alloc"))
            SPMV_TRY(csr_twophase_pool_alloc(m, (int)value));
        else
            SPMV_TRY(csr_twophase_pool_config(m, value));
    }
    else if (!strcmp(name, "twophase_choose_pieces"))  // run the piece search of a built two-phase layout (again) with the current budget
    {
        SPMV_HIP(hipSetDevice(m->ctx->device));
        SPMV_TRY(csr_twophase_choose_again(m));
    }
    else if (!strcmp(name, "twophase_rotate"))  // starting points of the expand phase's workgroups inside their panels: 256 (default), 0 = all at the start
    {
        SPMV_REQUIRE(value >= 0 && value <= 256, "twophase_rotate: 0 .. 256 starting points");
        m->tp_rotate = (int32_t)value;
    }
    else if (!strcmp(name, "twophase_only"))
    {
        // experiment (tools/tune_twophase.py): run phase A (1) or phase B (2) alone.  THE PRODUCT IS THEN WRONG, so the
        // switch exists only under SPMV_EXPERIMENTS=1 (read here, once, not on the product's path).
        const char* e_exp = getenv("SPMV_EXPERIMENTS");
        SPMV_REQUIRE(value == 0 || (e_exp && e_exp[0] == '1'), "twophase_only is an experiment: set SPMV_EXPERIMENTS=1");
        SPMV_REQUIRE(value >= 0 && value <= 2, "twophase_only: 0, 1 (phase A alone) or 2 (phase B alone)");
        m->tp_only = (int32_t)value;
    }
    else if (!strcmp(name, "twophase_realloc"))
    {
        // experiment (tools/probe_twophase_placement.py): move streams of the two-phase layout to fresh allocations, the
        // old ones freed only afterwards so that other memory is handed out.  Bits: 1 products, 2 values, 4 columns, 8 rows
        const char* e_exp = getenv("SPMV_EXPERIMENTS");
        SPMV_REQUIRE(e_exp && e_exp[0] == '1', "twophase_realloc is an experiment: set SPMV_EXPERIMENTS=1");
        SPMV_REQUIRE(m->tp_val && m->tp_padded > 0, "twophase_realloc: the two-phase layout is not built");
        SPMV_HIP(hipSetDevice(m->ctx->device));
        SPMV_HIP(hipStreamSynchronize(m->ctx->stream));
        auto move = [&](void** slot, size_t bytes) -> int {
            void* fresh = nullptr;
            if (hipMalloc(&fresh, bytes) != hipSuccess) SPMV_FAIL(SPMV_ERR_ALLOC, "twophase_realloc: out of device memory");
            if (const hipError_t e = hipMemcpy(fresh, *slot, bytes, hipMemcpyDeviceToDevice); e != hipSuccess)
            {
                (void)hipFree(fresh);
                SPMV_FAIL(SPMV_ERR_HIP, "twophase_realloc: copy failed: %s", hipGetErrorString(e));
            }
            (void)hipFree(*slot);
            *slot = fresh;
            return SPMV_OK;
        };
        const size_t np = (size_t)m->tp_padded;
        // (a pool of an experiment owns the pieces: replacing them here would leave the pool holding freed pointers)
        SPMV_REQUIRE(!((value & 1) && m->tp_pool), "twophase_realloc bit 1: this handle's pieces belong to a pool (twophase_pool_alloc)");
        if (value & 1)  // the product stream's pieces: fresh allocations (its contents need no copy: phase A rewrites all of it)
            for (int i = 0; i < m->tp_npieces; ++i)
            {
                double* fresh = nullptr;
                if (hipMalloc(&fresh, i + 1 < m->tp_npieces ? (size_t)1 << 30 : (size_t)m->tp_last_piece_bytes) != hipSuccess) SPMV_FAIL(SPMV_ERR_ALLOC, "twophase_realloc: out of device memory");
                (void)hipFree(m->tp_piece[i]);
                m->tp_piece[i] = fresh;
            }
        if (value & 2) SPMV_TRY(move((void**)&m->tp_val, sizeof(double) * np));
        if (value & 4) SPMV_TRY(move((void**)&m->tp_col, sizeof(uint16_t) * np));
        if (value & 8) SPMV_TRY(move((void**)&m->tp_row, sizeof(uint16_t) * np));
        if (value & 16) SPMV_TRY(move((void**)&m->tp_blk, sizeof(int32_t) * 2 * ((np + 15) / 16)));
    }
    else
        SPMV_FAIL(SPMV_ERR_INVALID, "unknown parameter '%s'", name);
    return SPMV_OK;
}

int spmv_mat_get_param(const spmv_mat* m, const char* name, int64_t* value)
{
    SPMV_REQUIRE(m && name && value, "null argument");
    for (const precond_row& P : kPreconds)  // the preconditioners' own: what each unit's hook lists
        if (P.get_param && P.get_param(m, name, value)) return SPMV_OK;
    if (spgemm_get_param(m, name, value)) return SPMV_OK;  // "spgemm_products", "spgemm_rows_lds", "spgemm_rows_sorted", "spgemm_lds_products", ...
    if (trsv_get_param(m, name, value)) return SPMV_OK;  // "trsv_ready", "trsv_bytes", "trsv_multi_launches", "trsv_multi_level_launches"
    if (transpose_get_param(m, name, value)) return SPMV_OK;  // "transpose_ready", "transpose_bytes", "transpose_kernel", ...
    if (!strcmp(name, "panel_keep_csr"))
        *value = (m->b && m->v) || m->nnz == 0 ? 1 : 0;
    else if (!strcmp(name, "device_bytes"))
        *value = m->device_bytes;
    else if (!strcmp(name, "coo_column_bins"))  // bins of the copy the segmented scan runs over (8 x bins per XCD), 0: none
        *value = m->cb_bins;
    else if (!strcmp(name, "coo_bins_padded"))
        *value = m->cb_padded;
    else if (!strcmp(name, "panel_rows"))
        *value = m->pb_built_rows;
    else if (!strcmp(name, "panel_width"))
        *value = m->pb_built_width;
    else if (!strcmp(name, "panel_sort"))
        *value = m->pb_built_sort;
    else if (!strcmp(name, "panel_groups"))
        *value = m->pb_ngroups;
    // (panel_unroll / panel_pipe / panel_sync echo a REQUEST, aliases applied; a launch runs panel_effective, equal on every documented value)
    else if (!strcmp(name, "panel_unroll"))
        *value = std::min(8, m->pb_unroll > 0 ? m->pb_unroll : (m->pb_unroll_tuned > 0 ? m->pb_unroll_tuned : 8));  // (16 runs 8 since round 4)
    else if (!strcmp(name, "panel_bytes"))
        *value = m->pb_bytes;
    else if (!strcmp(name, "panel_pipe"))
        *value = m->pb_pipe >= 0 ? m->pb_pipe : (m->pb_pipe_tuned > 0 ? m->pb_pipe_tuned : 1);
    else if (!strcmp(name, "panel_sync"))
        *value = (m->pb_sync >= 0 ? m->pb_sync : m->pb_sync_tuned) == 2 ? 3 : (m->pb_sync >= 0 ? m->pb_sync : m->pb_sync_tuned);  // (2, the split barrier, runs 3 since round 5)
    else if (!strcmp(name, "panel_layout"))  // layout in memory: 0 three arrays, 1 records, 3 packed 12-byte entries
        *value = m->pb_pack ? (m->pb_pair ? 4 : 3) : 0;
    else if (!strcmp(name, "twophase_panel_cols"))
        *value = m->tp_pcols;
    else if (!strcmp(name, "twophase_pieces_carved"))  // pieces of the product stream that lie inside the released CSR copy's allocations
    {
        *value = 0;
        for (int i = 0; i < m->tp_npieces; ++i) *value += m->tp_piece_carved[i] ? 1 : 0;
    }
    else if (!strcmp(name, "twophase_placements_timed"))
        *value = m->tp_place_seen;
    else if (!strcmp(name, "twophase_placement_spread"))  // time as built / time with the pieces the search kept, in 1/1000
        *value = m->tp_place_gain;
    else if (!strcmp(name, "twophase_padded"))
        *value = m->tp_padded;
    else if (!strcmp(name, "twophase_pieces"))  // 1 GB pieces the product stream consists of
        *value = m->tp_npieces;
    else if (!strcmp(name, "twophase_pieces_exchanged"))  // of them: exchanged for other pieces by the search
        *value = m->tp_pieces_exchanged;
    else if (!strcmp(name, "twophase_placement_budget_mb"))
        *value = m->tp_place_budget_mb;
    else if (!strcmp(name, "window_max_span"))
        *value = m->win_max_span;
    else if (!strcmp(name, "window_avg_span"))
        *value = (int64_t)m->win_avg_span;
    else if (!strcmp(name, "contiguous_permille"))
        *value = (int64_t)(m->contig_frac * 1000.0 + 0.5);
    else if (!strcmp(name, "rowgrouped_kernel"))
        *value = runs_from_rowgrouped(m) ? m->rowgrouped->kernel : 0;
    else if (!strcmp(name, "panel_rounds"))
        *value = m->pb_built_rounds;
    else if (!strcmp(name, "panel_rounds_us_one"))
        *value = (int64_t)(m->pb_rounds_us[0] + 0.5f);
    else if (!strcmp(name, "panel_rounds_us_more"))
        *value = (int64_t)(m->pb_rounds_us[1] + 0.5f);
    else if (!strcmp(name, "split_row_threshold"))
        *value = m->format == SPMV_FMT_CSR ? csr_split_threshold(m) : 0;
    else if (!strcmp(name, "split_long_rows"))
        *value = m->split_long_rows;
    else if (!strcmp(name, "split_mode"))
        *value = m->split_built_mode ? m->split_built_mode : m->split_mode;
    else if (!strcmp(name, "split_virtual_rows"))
        *value = m->split_vrows;
    else if (!strcmp(name, "split_long_kernel"))
        *value = m->split_long ? m->split_long->kernel : 0;
    else if (!strcmp(name, "split_long_entries"))
        *value = m->split_long_nnz;
    else if (!strcmp(name, "min_row_entries"))
        *value = m->min_row_nnz;
    else if (!strcmp(name, "adds_into_y_with_atomics"))  // 1: the product adds into y with device atomics (spmv_apply_host stages y in device memory)
        *value = adds_into_y_with_atomics(m) ? 1 : 0;
    else if (!strcmp(name, "split_inner_kernel"))
        *value = m->format == SPMV_FMT_CSR && m->kernel == SPMV_CSR_SPLIT && m->split_short ? m->split_short->kernel : 0;
    else if (!ell_get_param(m, name, value) && !select_get_param(m, name, value))  // "ell_*", "ell_copy_*"; "select_candidates", "select_rounds", "select_us_<name>"
        SPMV_FAIL(SPMV_ERR_INVALID, "unknown parameter '%s'", name);
    return SPMV_OK;
}

int spmv_mat_set_flags(spmv_mat* m, uint32_t flags)
{
    SPMV_REQUIRE(m, "null matrix");
    if (m->format == SPMV_FMT_CSR_F32 && flags)
        SPMV_FAIL(SPMV_ERR_UNSUPPORTED, "spmv_mat_set_flags: a handle of format 6 has one kernel and takes no tuning bits (flags = 0x%x)", flags);
    m->flags = flags;
    return SPMV_OK;
}

int spmv_mat_download(const spmv_mat* m, int32_t* a, int32_t* b, double* v)
{
    SPMV_REQUIRE(m, "null matrix");
    SPMV_TRY(use_device(m->ctx));
    size_t na = 0, nb = 0, nv = 0;
    switch (m->format)
    {
        case SPMV_FMT_CSR: na = (size_t)m->nrow + 1; nb = nv = (size_t)m->nnz; break;
        case SPMV_FMT_COO: na = nb = nv = (size_t)m->nnz; break;
        case SPMV_FMT_ELL: nb = nv = (size_t)m->nrow * (size_t)m->k; break;
        case SPMV_FMT_CSC: na = (size_t)m->ncol + 1; nb = nv = (size_t)m->nnz; break;
        case SPMV_FMT_DIA: na = (size_t)m->k; nv = (size_t)m->nrow * (size_t)m->k; break;
        case SPMV_FMT_BSR: na = (size_t)ceil_div(m->nrow, m->k) + 1; nb = (size_t)(m->nnz / (m->k * m->k)); nv = (size_t)m->nnz; break;
        case SPMV_FMT_CSR_F32:
        {
            // the row pointer as it is; the columns and the values - widened to double - out of the packed stream, through set-up memory
            const size_t nnz = (size_t)m->nnz;
            hipStream_t  s   = m->ctx->stream;
            if (a) SPMV_HIP(hipMemcpyAsync(a, m->a, ((size_t)m->nrow + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, s));
            void *   d_b = nullptr, *d_v = nullptr;
            int      rc  = SPMV_OK;
            if (nnz && b && hipMalloc(&d_b, nnz * sizeof(int32_t)) != hipSuccess) rc = SPMV_ERR_ALLOC;
            if (rc == SPMV_OK && nnz && v && hipMalloc(&d_v, nnz * sizeof(double)) != hipSuccess) rc = SPMV_ERR_ALLOC;
            if (rc == SPMV_ERR_ALLOC)
            {
                (void)hipGetLastError();
                set_error("spmv_mat_download: out of device memory for %zu widened entries of a format 6 handle", nnz);
            }
            if (rc == SPMV_OK && (d_b || d_v)) rc = f32_widen_arrays(m->ctx, m, (int32_t*)d_b, (double*)d_v);
            if (rc == SPMV_OK && d_b && hipMemcpyAsync(b, d_b, nnz * sizeof(int32_t), hipMemcpyDeviceToHost, s) != hipSuccess) rc = SPMV_ERR_HIP;
            if (rc == SPMV_OK && d_v && hipMemcpyAsync(v, d_v, nnz * sizeof(double), hipMemcpyDeviceToHost, s) != hipSuccess) rc = SPMV_ERR_HIP;
            if (hipStreamSynchronize(s) != hipSuccess && rc == SPMV_OK) rc = SPMV_ERR_HIP;
            if (rc == SPMV_ERR_HIP) set_error("spmv_mat_download: %s", hipGetErrorString(hipGetLastError()));
            if (d_b) (void)hipFree(d_b);
            if (d_v) (void)hipFree(d_v);
            return rc;
        }
        default: SPMV_FAIL(SPMV_ERR_INVALID, "unknown format %d", m->format);
    }
    SPMV_REQUIRE(!((b && nb && !m->b) || (v && nv && !m->v)), "spmv_mat_download: this handle gave up its arrays (panel_keep_csr = 0)");
    hipStream_t s = m->ctx->stream;
    if (a && na) SPMV_HIP(hipMemcpyAsync(a, m->a, na * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (b && nb) SPMV_HIP(hipMemcpyAsync(b, m->b, nb * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (v && nv) SPMV_HIP(hipMemcpyAsync(v, m->v, nv * sizeof(double), hipMemcpyDeviceToHost, s));
    SPMV_HIP(hipStreamSynchronize(s));
    return SPMV_OK;
}

int spmv_mat_device_ptrs(const spmv_mat* m, const int32_t** a, const int32_t** b, const double** v)
{
    SPMV_REQUIRE(m, "null matrix");
    if (m->format == SPMV_FMT_CSR_F32)
        SPMV_FAIL(SPMV_ERR_UNSUPPORTED, "spmv_mat_device_ptrs: a handle of format 6 holds one packed entry stream, no column and value arrays");
    if (a) *a = m->a;
    if (b) *b = m->b;
    if (v) *v = m->v;
    return SPMV_OK;
}

// ---- the hot path -----------------------------------------------------------------------------------------
static int check_apply_args(spmv_ctx* ctx, const spmv_mat* A, const spmv_vec* x, spmv_vec* y)
{
    SPMV_REQUIRE(ctx && A && x && y, "spmv_apply: null argument");
    SPMV_REQUIRE(x->n == A->ncol, "spmv_apply: x has %lld entries, matrix has %d columns", (long long)x->n, A->ncol);
    SPMV_REQUIRE(y->n == A->nrow, "spmv_apply: y has %lld entries, matrix (shard) has %d rows", (long long)y->n,
                 A->nrow);
    SPMV_REQUIRE(x->d != y->d || x->n == 0, "spmv_apply: x and y must not alias");
    return SPMV_OK;
}

int spmv_apply(spmv_ctx* ctx, const spmv_mat* A, const spmv_vec* x, spmv_vec* y)
{
    SPMV_TRY(check_apply_args(ctx, A, x, y));
    SPMV_TRY(use_device(ctx));
    return mat_apply_ex(ctx, A, x->d, y->d);
}

int spmv_apply_timed(spmv_ctx* ctx, const spmv_mat* A, const spmv_vec* x, spmv_vec* y, int32_t reps,
                     double* ms_per_apply)
{
    SPMV_TRY(check_apply_args(ctx, A, x, y));
    SPMV_REQUIRE(reps > 0 && ms_per_apply, "spmv_apply_timed: reps=%d", reps);
    SPMV_TRY(use_device(ctx));
    float ms = 0.f;
    SPMV_TRY(time_launches(ctx, reps, [&] { return mat_apply_ex(ctx, A, x->d, y->d); }, &ms));
    *ms_per_apply = ms;
    return SPMV_OK;
}

// ---- several vectors at once: Y += A*X, X and Y row-major (kernels_spmm.hip) --------------------------------
// Every check is made before the device is touched, so that they hold (and are tested) on a machine without one.
static int check_apply_multi_args(spmv_ctx* ctx, const spmv_mat* A, int32_t k, const spmv_vec* X, spmv_vec* Y)
{
    SPMV_REQUIRE(ctx && A && X && Y, "spmv_apply_multi: null argument");
    SPMV_REQUIRE(k >= 1 && k <= 64, "spmv_apply_multi: k = %d, must be in [1, 64]", k);
    SPMV_REQUIRE(X->n == (int64_t)A->ncol * k, "spmv_apply_multi: X has %lld entries, ncol * k = %d * %d", (long long)X->n,
                 A->ncol, k);
    SPMV_REQUIRE(Y->n == (int64_t)A->nrow * k, "spmv_apply_multi: Y has %lld entries, nrow * k = %d * %d", (long long)Y->n,
                 A->nrow, k);
    SPMV_REQUIRE(X->n == 0 || Y->n == 0 || X->d + X->n <= Y->d || Y->d + Y->n <= X->d,
                 "spmv_apply_multi: X and Y must not overlap");
    if (A->format != SPMV_FMT_CSR && A->format != SPMV_FMT_ELL)
        SPMV_FAIL(SPMV_ERR_UNSUPPORTED, "spmv_apply_multi: CSR and ELL handles only (format %d)", A->format);
    // the product reads the handle's own arrays: a CSR handle that released them (panel_keep_csr = 0) is refused here, on the host
    const int64_t entries = A->format == SPMV_FMT_CSR ? A->nnz : (int64_t)A->nrow * A->k;
    SPMV_REQUIRE(entries == 0 || (A->b && A->v),
                 "spmv_apply_multi: this handle gave up its CSR arrays (panel_keep_csr = 0)");
    return SPMV_OK;
}

int spmv_apply_multi(spmv_ctx* ctx, const spmv_mat* A, int32_t k, const spmv_vec* X, spmv_vec* Y, int32_t overwrite)
{
    SPMV_TRY(check_apply_multi_args(ctx, A, k, X, Y));
    SPMV_TRY(use_device(ctx));
    return spmm_apply(ctx, A, k, X->d, Y->d, overwrite != 0);
}

int spmv_apply_multi_timed(spmv_ctx* ctx, const spmv_mat* A, int32_t k, const spmv_vec* X, spmv_vec* Y, int32_t overwrite,
                           int32_t reps, double* ms_per_apply)
{
    SPMV_TRY(check_apply_multi_args(ctx, A, k, X, Y));
    SPMV_REQUIRE(reps > 0 && ms_per_apply, "spmv_apply_multi_timed: reps=%d", reps);
    SPMV_TRY(use_device(ctx));
    float ms = 0.f;
    SPMV_TRY(time_launches(ctx, reps, [&] { return spmm_apply(ctx, A, k, X->d, Y->d, overwrite != 0); }, &ms));
    *ms_per_apply = ms;
    return SPMV_OK;
}

// ---- dense products sampled on a CSR pattern: out = alpha * (U V^T)|pattern + beta * out (kernels_sddmm.hip) ------------------
// Every check is made before the device is touched, so that they hold (and are tested) on a machine without one.
static bool vec_overlap(const spmv_vec* p, const spmv_vec* q)
{
    return p->n > 0 && q->n > 0 && !(p->d + p->n <= q->d || q->d + q->n <= p->d);
}

static int check_sddmm_args(spmv_ctx* ctx, const spmv_mat* A, int32_t k, const spmv_vec* U, const spmv_vec* V, spmv_vec* out)
{
    SPMV_REQUIRE(ctx && A && U && V && out, "spmv_sddmm: null argument");
    SPMV_REQUIRE(k >= 1 && k <= kSddmmMaxK, "spmv_sddmm: k = %d, must be in [1, %d]", k, kSddmmMaxK);
    if (A->format != SPMV_FMT_CSR) SPMV_FAIL(SPMV_ERR_UNSUPPORTED, "spmv_sddmm: CSR patterns only (format %d)", A->format);
    SPMV_REQUIRE(U->n == (int64_t)A->nrow * k, "spmv_sddmm: U has %lld entries, nrow * k = %d * %d", (long long)U->n, A->nrow, k);
    SPMV_REQUIRE(V->n == (int64_t)A->ncol * k, "spmv_sddmm: V has %lld entries, ncol * k = %d * %d", (long long)V->n, A->ncol, k);
    SPMV_REQUIRE(out->n == A->nnz, "spmv_sddmm: out has %lld entries, the pattern %lld", (long long)out->n, (long long)A->nnz);
    SPMV_REQUIRE(!vec_overlap(out, U) && !vec_overlap(out, V), "spmv_sddmm: out must not overlap U or V");
    SPMV_REQUIRE(A->a && (A->nnz == 0 || A->b), "spmv_sddmm: this handle gave up its CSR arrays (panel_keep_csr = 0)");
    return SPMV_OK;
}

int spmv_sddmm(spmv_ctx* ctx, const spmv_mat* A, int32_t k, double alpha, const spmv_vec* U, const spmv_vec* V, double beta,
               spmv_vec* out)
{
    SPMV_TRY(check_sddmm_args(ctx, A, k, U, V, out));
    SPMV_TRY(use_device(ctx));
    return sddmm_apply(ctx, A, k, alpha, U->d, V->d, beta, out->d);
}

int spmv_sddmm_timed(spmv_ctx* ctx, const spmv_mat* A, int32_t k, double alpha, const spmv_vec* U, const spmv_vec* V, double beta,
                     spmv_vec* out, int32_t reps, double* ms_per_call)
{
    SPMV_TRY(check_sddmm_args(ctx, A, k, U, V, out));
    SPMV_REQUIRE(reps > 0 && ms_per_call, "spmv_sddmm_timed: reps=%d", reps);
    SPMV_TRY(use_device(ctx));
    float ms = 0.f;
    SPMV_TRY(time_launches(ctx, reps, [&] { return sddmm_apply(ctx, A, k, alpha, U->d, V->d, beta, out->d); }, &ms));
    *ms_per_call = ms;
    return SPMV_OK;
}

// a CSR handle over A's own row_ptr / col_ind and the vector's storage as its values: spmv_csr_wrap_device over pointers the engine
// already holds (a shard stays a shard); analysed like any wrapped handle
int spmv_csr_with_values(spmv_ctx* ctx, const spmv_mat* A, const spmv_vec* values, spmv_mat** out)
{
    SPMV_REQUIRE(ctx && A && values && out, "spmv_csr_with_values: null argument");
    SPMV_REQUIRE(A->format == SPMV_FMT_CSR && A->a && (A->nnz == 0 || A->b),
                 "spmv_csr_with_values: A is not a CSR handle with its arrays (format %d; panel_keep_csr = 0 released them?)", A->format);
    SPMV_REQUIRE(values->n == A->nnz, "spmv_csr_with_values: values has %lld entries, the pattern %lld", (long long)values->n,
                 (long long)A->nnz);
    SPMV_TRY(use_device(ctx));
    plan_arm arm(ctx);
    spmv_mat* m = nullptr;
    SPMV_TRY(wrap(ctx, SPMV_FMT_CSR, A->nrow, A->ncol, A->nnz, 0, A->a, A->b, values->d, &m));
    m->row_begin = A->row_begin;
    return finish(m, out);
}

// ---- the reference's own call shape: host vectors in, host vector out ---------------------------------------------------------
// CSRMatrixMatVector(A, x, y) and its siblings take HOST vectors on every call (include/mat_vec.h:7-11; main.cpp:56-59 calls
// them 50 times).  Behind that signature a product costs two hand-overs whatever the kernel does; for small matrices they ARE the
// cost (C1: kernel 3 us).  Rounds 1-4 paid three synchronous hipMemcpy of pageable memory per call (~17 us each: 67 us per C1
// product, 4.8 GFLOP/s against the reference's 5.6 on one CPU thread).  Here, for vectors up to 1 MB together (tools/probe_apply_host_sizes.py: beyond ~1.5 MB the copies' fixed cost is paid back by their higher rate): the host copies
// y into a pinned, device-mapped staging buffer (memcpy: 80 KB in 3 us) and stores x straight into a device buffer where the
// platform lets the CPU do that (large BAR: 80 KB in 2 us; elsewhere x goes through the staging buffer and one kernel pulls it
// over the host link), the product gathers x from device memory and updates y IN the staging buffer (kernels that add into y
// with device atomics - the COO scan, the CSC scatter - get y through a device buffer and two more launches instead), the
// host polls the stream (hipStreamQuery: no interrupt wake-up) and copies y out.  ONE launch, no hipMemcpy: what is left of a
// C1 product is the 12-17 us a kernel launch takes from doorbell to completion signal on this platform.  Larger vectors take asynchronous copies from / to the caller's memory
// (the PCIe time dominates there).  The caller's arrays are never registered or mapped: they may be freed or re-allocated
// between calls without a stale mapping being left behind.
static int grow(double** p, size_t* have, size_t want)
{
    if (*have >= want) return SPMV_OK;
    if (*p) SPMV_HIP(hipFree(*p));
    *p    = nullptr;
    *have = 0;
    const size_t n = std::max<size_t>(want + want / 4, 4096);
    if (hipMalloc(p, sizeof(double) * n) != hipSuccess)
    {
        (void)hipGetLastError();
        SPMV_FAIL(SPMV_ERR_ALLOC, "spmv_apply_host: no device memory for a staging vector of %zu entries", n);
    }
    *have = n;
    return SPMV_OK;
}

// The end of a staged call: hipStreamSynchronize.  Measured for an empty kernel (tools/probe_launch_floor.hip,
// profiles/r06_probe_launch_floor.txt): launch + hipStreamQuery spin (round 5) 16.9 us, launch + hipStreamSynchronize 10.5,
// launch + a word of pinned host memory the kernel writes and the host spins on 6.4.  The last one does not survive contact with a
// real call: the word has to come AFTER the product's stores, i.e. from a second launch (23.9 us per C1 call against 22.2 with
// the plain synchronize, same box, profiles/r06_dropin_small_products.txt) or from the product's own last workgroup behind
// system-wide fences of every lane (32 us).  So: the call HIP guarantees, and nothing to go wrong.
static int host_wait(spmv_ctx* ctx)
{
    SPMV_HIP(hipStreamSynchronize(ctx->stream));
    return SPMV_OK;
}

int spmv_apply_host(spmv_ctx* ctx, const spmv_mat* A, const double* x_host, double* y_host)
{
    SPMV_REQUIRE(ctx && A && (x_host || A->ncol == 0) && (y_host || A->nrow == 0), "spmv_apply_host: null argument");
    SPMV_REQUIRE(A->ctx == ctx, "spmv_apply_host: the matrix belongs to another context");
    SPMV_TRY(use_device(ctx));
    const size_t nx = (size_t)A->ncol, ny = (size_t)A->nrow;
    if (ny == 0) return SPMV_OK;
    // (No wait for the stream here: the staging buffers are touched by this function alone, and it returns only when its own
    // launches are done with them; work queued earlier by others runs before ours by stream order.  Growing a buffer waits.)
    if (ctx->stage_x_n < std::max<size_t>(nx, 1) || ctx->stage_y_n < ny) SPMV_HIP(hipStreamSynchronize(ctx->stream));
    SPMV_TRY(grow(&ctx->stage_x, &ctx->stage_x_n, std::max<size_t>(nx, 1)));
    SPMV_TRY(grow(&ctx->stage_y, &ctx->stage_y_n, ny));
    const double* dx = ctx->stage_x;
    double*       dy = ctx->stage_y;
    // (SPMV_HOST_STAGED_MB: the limit in megabytes, for tools/probe_apply_host_sizes.py; read per call, this is not a product's path
    // that anything is measured on)
    static const size_t kStagedLimit = [] {
        const char* e = getenv("SPMV_HOST_STAGED_MB");
        return ((size_t)(e && atoi(e) > 0 ? atoi(e) : 1) << 20) / sizeof(double);
    }();
    if (nx + ny <= kStagedLimit)
    {
        if (ctx->stage_pinned_n < nx + ny)
        {
            SPMV_HIP(hipStreamSynchronize(ctx->stream));
            if (ctx->stage_pinned) (void)hipHostFree(ctx->stage_pinned);
            ctx->stage_pinned     = nullptr;
            ctx->stage_pinned_dev = nullptr;
            ctx->stage_pinned_n   = 0;
            const size_t n        = std::max<size_t>(2 * (nx + ny), 32768);
            void*        dev      = nullptr;
            if (hipHostMalloc((void**)&ctx->stage_pinned, sizeof(double) * n, hipHostMallocMapped) != hipSuccess ||
                hipHostGetDevicePointer(&dev, ctx->stage_pinned, 0) != hipSuccess)
            {
                if (ctx->stage_pinned) (void)hipHostFree(ctx->stage_pinned);
                ctx->stage_pinned = nullptr;
                SPMV_FAIL(SPMV_ERR_ALLOC, "spmv_apply_host: no pinned host memory for %zu staged entries: %s", n, hipGetErrorString(hipGetLastError()));
            }
            ctx->stage_pinned_dev = (double*)dev;
            ctx->stage_pinned_n   = n;
        }
        double* hx = ctx->stage_pinned;
        double* hy = ctx->stage_pinned + nx;
        // Kernels that touch every y_i once with a plain read and a plain store (the row-parallel, LDS-window, scalar, panel and
        // two-phase CSR kernels, the ELL and DIA kernels, and handles running from a copy that runs one of those) update y IN
        // the staging buffer over the host link: two launches.  Kernels that add into y with device atomics (the COO scan, the
        // CSC scatter, CSR under SEGSCAN or SPLIT's chunks - whether the handle's own or its copy's: adds_into_y_with_atomics)
        // get y through a device buffer: fp64 atomics on host memory over the link are platform behaviour, not a HIP guarantee.
        // (experiment, tools/probe_apply_host_atomics.py: SPMV_EXPERIMENTS=1 SPMV_HOST_Y_IN_PLACE=1 keeps y in the staging buffer
        // whatever the kernel - to SEE what device atomics on mapped host memory do on a given box; never a product's path)
        static const bool kForceInPlace = [] {
            const char *e = getenv("SPMV_EXPERIMENTS"), *f = getenv("SPMV_HOST_Y_IN_PLACE");
            return e && e[0] == '1' && f && f[0] == '1';
        }();
        const bool y_in_place = kForceInPlace || !adds_into_y_with_atomics(A);
        // Round 6 (tools/probe_launch_floor.hip, tools/probe_small_host_calls.py; profiles/r06_dropin_small_products.txt):
        //   * the call ends in hipStreamSynchronize, not in a hipStreamQuery spin (host_wait above), and does not begin with one;
        //   * y NEED NOT TRAVEL TO THE DEVICE.  The CSR kernels that form a row's sum and add it to y in one step - row-parallel,
        //     panel, two-phase: y_i = y_i + sum_i, the reference's own shape (src/mat_vec.cpp:59-64: private sum, one +=) - write
        //     sum_i alone (their "overwrite" mode) and the host does y_host[i] += sum_i while it copies out: the same IEEE add,
        //     bit for bit what the kernel would have stored, one memcpy and one crossing of the host link less.  Kernels whose
        //     accumulator starts AT y_i (ELL, DIA, scalar CSR: the reference's order y0 + p0 + p1 + ...) keep y in place.
        const spmv_mat* K = A;  // the handle whose kernel runs
        while (runs_from_rowgrouped(K)) K = K->rowgrouped;
        const bool sum_then_add = y_in_place && !kForceInPlace && (K->format == SPMV_FMT_CSR || K->format == SPMV_FMT_CSR_F32) && K->nnz > 0 && writes_row_sums_in_one_launch(K);
        if (nx && !ctx->large_bar) memcpy(hx, x_host, sizeof(double) * nx);
        if (!sum_then_add) memcpy(hy, y_host, sizeof(double) * ny);
        // x: where the CPU can store into device memory (large BAR) it writes x into the device buffer itself - 80 KB in 2 us,
        // no launch (tools/probe_host_write_vram.hip: the next kernel sees the stores, also right after a kernel that read the
        // previous contents; the HDP flush register is written behind them as the platform prescribes for such stores; the
        // context checked it once for itself when it was created).  Elsewhere one kernel pulls x out of the staging buffer.
        const bool direct = ctx->large_bar != 0;
        if (direct && nx)
        {
            memcpy(ctx->stage_x, x_host, sizeof(double) * nx);
            __sync_synchronize();
            if (ctx->hdp_flush) *ctx->hdp_flush = 1u;
        }
        if (y_in_place)
        {
            dy = ctx->stage_pinned_dev + nx;
            if (!direct) SPMV_TRY(vec_copy2(ctx, ctx->stage_x, ctx->stage_pinned_dev, (int64_t)nx, nullptr, nullptr, 0));
            apply_extra ex;
            ex.overwrite = sum_then_add;
            SPMV_TRY(mat_apply_ex(ctx, A, dx, dy, ex));
        }
        else
        {
            SPMV_TRY(vec_copy2(ctx, ctx->stage_x, ctx->stage_pinned_dev, direct ? 0 : (int64_t)nx, ctx->stage_y, ctx->stage_pinned_dev + nx, (int64_t)ny));
            SPMV_TRY(mat_apply_ex(ctx, A, dx, dy));
            SPMV_TRY(vec_copy2(ctx, ctx->stage_pinned_dev + nx, ctx->stage_y, (int64_t)ny, nullptr, nullptr, 0));
        }
        SPMV_TRY(host_wait(ctx));
        if (sum_then_add)
            for (size_t i = 0; i < ny; ++i) y_host[i] += hy[i];
        else
            memcpy(y_host, hy, sizeof(double) * ny);
        return SPMV_OK;
    }
    if (nx) SPMV_HIP(hipMemcpyAsync(ctx->stage_x, x_host, sizeof(double) * nx, hipMemcpyHostToDevice, ctx->stream));
    SPMV_HIP(hipMemcpyAsync(ctx->stage_y, y_host, sizeof(double) * ny, hipMemcpyHostToDevice, ctx->stream));
    SPMV_TRY(mat_apply_ex(ctx, A, dx, dy));
    SPMV_HIP(hipMemcpyAsync(y_host, ctx->stage_y, sizeof(double) * ny, hipMemcpyDeviceToHost, ctx->stream));
    SPMV_HIP(hipStreamSynchronize(ctx->stream));
    return SPMV_OK;
}

// ---- BLAS-1 -----------------------------------------------------------------------------------------------
int spmv_dot(spmv_ctx* ctx, const spmv_vec* x, const spmv_vec* y, double* result)
{
    SPMV_REQUIRE(ctx && x && y && result, "spmv_dot: null argument");
    SPMV_REQUIRE(x->n == y->n, "spmv_dot: sizes %lld and %lld differ", (long long)x->n, (long long)y->n);
    SPMV_TRY(use_device(ctx));
    return vec_dot(ctx, x->d, y->d, x->n, result);
}

int spmv_axpby(spmv_ctx* ctx, double alpha, const spmv_vec* x, double beta, const spmv_vec* y, spmv_vec* w)
{
    SPMV_REQUIRE(ctx && x && y && w, "spmv_axpby: null argument");
    // the reference sizes the loop by w (src/vec_vec.cpp:33)
    SPMV_REQUIRE(x->n >= w->n && y->n >= w->n, "spmv_axpby: w has %lld entries, x %lld, y %lld", (long long)w->n,
                 (long long)x->n, (long long)y->n);
    SPMV_TRY(use_device(ctx));
    return vec_axpby(ctx, alpha, x->d, beta, y->d, w->d, w->n);
}

// ---- solver step (solver.hip) -----------------------------------------------------------------------------
int spmv_apply_dot(spmv_ctx* ctx, const spmv_mat* A, const spmv_vec* x, spmv_vec* y, int32_t overwrite, const spmv_vec* w,
                   double* dot)
{
    SPMV_TRY(check_apply_args(ctx, A, x, y));
    SPMV_REQUIRE(w && dot, "spmv_apply_dot: null argument");
    SPMV_REQUIRE(w->n == A->nrow, "spmv_apply_dot: w has %lld entries, matrix has %d rows", (long long)w->n, A->nrow);
    SPMV_REQUIRE(w->d != y->d || y->n == 0, "spmv_apply_dot: w and y must not alias");
    SPMV_TRY(use_device(ctx));
    double* out = ctx->dev_scalars;
    SPMV_HIP(hipMemsetAsync(out, 0, sizeof(double) * kDotDoubles, ctx->stream));
    apply_extra ex;
    ex.overwrite = overwrite != 0;
    ex.dot_w     = w->d;
    ex.dot_out   = out;
    SPMV_TRY(mat_apply_ex(ctx, A, x->d, y->d, ex));
    std::vector<double> slots(kDotDoubles);
    SPMV_HIP(hipMemcpyAsync(slots.data(), out, sizeof(double) * kDotDoubles, hipMemcpyDeviceToHost, ctx->stream));
    SPMV_HIP(hipStreamSynchronize(ctx->stream));
    double total = 0.0;
    for (int i = 0; i < kDotSlots; ++i) total += slots[(size_t)i * kDotStride];
    *dot = total;
    return SPMV_OK;
}

// The solves.  Every check is made before the device is touched, so that they hold (and are tested) on a machine without one;
// the checks they share are solver_host.hpp's, and what each solver's refusals depend on (k*Rules) stands beside the preconditioners'
// table (precond.hip).
int spmv_cg(spmv_ctx* ctx, const spmv_mat* A, const spmv_vec* b, spmv_vec* x, int32_t max_iter, double rel_tol,
            int32_t check_every, int32_t precond, int32_t* iters, double* rel_resid)
{
    SPMV_TRY(check_square_solve(kCgRules, ctx, A, b, x, max_iter, rel_tol, precond, iters, rel_resid));
    SPMV_TRY(check_preconditioner(kCgRules, A, precond));
    SPMV_TRY(use_device(ctx));
    return cg_solve(ctx, A, b->d, x->d, max_iter, rel_tol, check_every, precond, iters, rel_resid);
}

// k right-hand sides at once (solver_multi.hip)
int spmv_cg_multi(spmv_ctx* ctx, const spmv_mat* A, int32_t k, const spmv_vec* B, spmv_vec* X, int32_t max_iter, double rel_tol,
                  int32_t check_every, int32_t precond, int32_t* iters, double* rel_resid)
{
    SPMV_REQUIRE(ctx && A && B && X && iters && rel_resid, "spmv_cg_multi: null argument");
    SPMV_REQUIRE(k >= 1 && k <= 64, "spmv_cg_multi: k = %d, must be in [1, 64]", k);
    SPMV_REQUIRE(A->nrow == A->ncol, "spmv_cg_multi: the matrix is %d x %d, not square", A->nrow, A->ncol);
    SPMV_REQUIRE(B->n == (int64_t)A->nrow * k && X->n == (int64_t)A->nrow * k,
                 "spmv_cg_multi: B has %lld and X %lld entries, nrow * k = %d * %d", (long long)B->n, (long long)X->n, A->nrow, k);
    SPMV_REQUIRE(vectors_disjoint(B, X), "spmv_cg_multi: B and X must not overlap");
    SPMV_TRY(check_limits("spmv_cg_multi", max_iter, rel_tol));
    SPMV_TRY(check_known_preconditioner("spmv_cg_multi", precond));
    if (A->format != SPMV_FMT_CSR && A->format != SPMV_FMT_ELL)
        SPMV_FAIL(SPMV_ERR_UNSUPPORTED, "spmv_cg_multi: CSR and ELL handles only (format %d), as spmv_apply_multi", A->format);
    SPMV_TRY(check_preconditioner(kCgMultiRules, A, precond));
    // the product reads the handle's own arrays: a CSR handle that released them (panel_keep_csr = 0) is refused here, on the host
    const int64_t entries = A->format == SPMV_FMT_CSR ? A->nnz : (int64_t)A->nrow * A->k;
    SPMV_REQUIRE(entries == 0 || (A->b && A->v), "spmv_cg_multi: this handle gave up its CSR arrays (panel_keep_csr = 0)");
    SPMV_TRY(use_device(ctx));
    return cg_multi_solve(ctx, A, k, B->d, X->d, max_iter, rel_tol, check_every, precond, iters, rel_resid);
}

// least squares over A and A^T (solver_cgls.hip)
int spmv_cgls(spmv_ctx* ctx, const spmv_mat* A, const spmv_vec* b, spmv_vec* x, int32_t max_iter, double rel_tol, int32_t check_every,
              double damp, int32_t* iters, double* rel_normal_resid, double* rel_resid)
{
    SPMV_REQUIRE(ctx && A && b && x && iters && rel_normal_resid && rel_resid, "spmv_cgls: null argument");
    SPMV_REQUIRE(b->n == A->nrow, "spmv_cgls: b has %lld entries, the matrix (shard) %d rows", (long long)b->n, A->nrow);
    SPMV_REQUIRE(x->n == A->ncol, "spmv_cgls: x has %lld entries, the matrix %d columns", (long long)x->n, A->ncol);
    SPMV_REQUIRE(vectors_disjoint(b, x), "spmv_cgls: b and x must not overlap");
    SPMV_TRY(check_limits("spmv_cgls", max_iter, rel_tol));
    SPMV_REQUIRE(damp >= 0.0 && std::isfinite(damp), "spmv_cgls: damp=%g, must be finite and not negative", damp);
    // the transposed product reads the handle's own arrays the other way round: a CSR handle that released them is refused here
    SPMV_REQUIRE(!(A->format == SPMV_FMT_CSR && A->nnz > 0 && (!A->b || !A->v)),
                 "spmv_cgls: this handle gave up its CSR arrays (panel_keep_csr = 0)");
    SPMV_TRY(use_device(ctx));
    return cgls_solve(ctx, A, b->d, x->d, max_iter, rel_tol, check_every, damp, iters, rel_normal_resid, rel_resid);
}

// nonsymmetric square systems over two forward products (solver_bicgstab.hip)
int spmv_bicgstab(spmv_ctx* ctx, const spmv_mat* A, const spmv_vec* b, spmv_vec* x, int32_t max_iter, double rel_tol, int32_t check_every,
                  int32_t precond, int32_t* iters, double* rel_resid)
{
    SPMV_TRY(check_square_solve(kBicgstabRules, ctx, A, b, x, max_iter, rel_tol, precond, iters, rel_resid));
    SPMV_TRY(check_preconditioner(kBicgstabRules, A, precond));
    *iters     = 0;
    *rel_resid = 0.0;
    if (A->nrow == 0) return SPMV_OK;
    SPMV_TRY(use_device(ctx));
    return bicgstab_solve(ctx, A, b->d, x->d, max_iter, rel_tol, check_every, precond, iters, rel_resid);
}

// nonsymmetric square systems by restarted GMRES over one forward product per iteration (solver_gmres.hip)
int spmv_gmres(spmv_ctx* ctx, const spmv_mat* A, const spmv_vec* b, spmv_vec* x, int32_t restart, int32_t max_iter, double rel_tol,
               int32_t check_every, int32_t precond, int32_t* iters, double* rel_resid)
{
    SPMV_TRY(check_square_solve(kGmresRules, ctx, A, b, x, max_iter, rel_tol, precond, iters, rel_resid));
    SPMV_REQUIRE(restart >= 0 && restart <= 64, "spmv_gmres: restart=%d, must be 1 .. 64 (0: 30)", restart);
    SPMV_TRY(check_preconditioner(kGmresRules, A, precond));
    *iters     = 0;
    *rel_resid = 0.0;
    if (A->nrow == 0) return SPMV_OK;
    SPMV_TRY(use_device(ctx));
    return gmres_solve(ctx, A, b->d, x->d, restart == 0 ? 30 : restart, max_iter, rel_tol, check_every, precond, iters, rel_resid);
}

// symmetric indefinite systems with a shift over one forward product per iteration (solver_minres.hip)
int spmv_minres(spmv_ctx* ctx, const spmv_mat* A, const spmv_mat* P, const spmv_vec* b, spmv_vec* x, double shift, int32_t max_iter, double rel_tol,
                int32_t check_every, int32_t precond, int32_t* iters, double* rel_resid)
{
    SPMV_TRY(check_square_solve(kMinresRules, ctx, A, b, x, max_iter, rel_tol, precond, iters, rel_resid));
    SPMV_TRY(check_shift_and_precond_handle(kMinresRules, ctx, A, P, shift, precond));
    SPMV_TRY(check_preconditioner(kMinresRules, P ? P : A, precond));
    *iters     = 0;
    *rel_resid = 0.0;
    if (A->nrow == 0) return SPMV_OK;
    SPMV_TRY(use_device(ctx));
    return minres_solve(ctx, A, P, b->d, x->d, shift, max_iter, rel_tol, check_every, precond, iters, rel_resid);
}

// iterative refinement: the residual with A in fp64, the correction from spmv_cg or spmv_bicgstab on A_lo (solver_refine.hip)
int spmv_refine(spmv_ctx* ctx, const spmv_mat* A, const spmv_mat* A_lo, const spmv_vec* b, spmv_vec* x, int32_t solver, int32_t precond,
                int32_t max_outer, int32_t inner_max_iter, double inner_tol, double rel_tol, int32_t* outer, int32_t* inner_total, double* rel_resid)
{
    SPMV_TRY(check_refine(ctx, A, A_lo, b, x, solver, precond, max_outer, inner_max_iter, inner_tol, rel_tol, outer, inner_total, rel_resid));
    SPMV_TRY(check_preconditioner(solver == SPMV_REFINE_CG ? kCgRules : kBicgstabRules, A_lo, precond));  // (the inner solver's own refusals)
    *outer       = 0;
    *inner_total = 0;
    *rel_resid   = 0.0;
    if (A->nrow == 0) return SPMV_OK;
    SPMV_TRY(use_device(ctx));
    return refine_solve(ctx, A, A_lo, b->d, x->d, solver, precond, max_outer, inner_max_iter, inner_tol, rel_tol, outer, inner_total, rel_resid);
}

// blocks: G = U^T V and Out = S C (block_ops.hip)
int spmv_block_gram(spmv_ctx* ctx, int64_t n, int32_t p, const spmv_vec* U, int64_t ldu, int32_t q, const spmv_vec* V, int64_t ldv, double* G_host)
{
    SPMV_TRY(block_gram_check(ctx, n, p, U, ldu, q, V, ldv, G_host));
    if (n > 0) SPMV_TRY(use_device(ctx));
    return block_gram(ctx, n, p, U->d, ldu, q, V->d, ldv, G_host);
}

int spmv_block_combine(spmv_ctx* ctx, int64_t n, int32_t p, const spmv_vec* S, int64_t lds, int32_t q, const double* C_host, spmv_vec* Out, int64_t ldo)
{
    SPMV_TRY(block_combine_check(ctx, n, p, S, lds, q, C_host, Out, ldo));
    if (n == 0) return SPMV_OK;
    SPMV_TRY(use_device(ctx));
    return block_combine(ctx, n, p, S->d, lds, q, C_host, Out->d, ldo);
}

// extreme eigenpairs of a symmetric matrix by LOBPCG (solver_lobpcg.hip)
int spmv_lobpcg(spmv_ctx* ctx, const spmv_mat* A, int32_t k, int32_t nev, int32_t largest, spmv_vec* X, int32_t max_iter, double tol, int32_t precond,
                double* theta, double* resid, int32_t* iters)
{
    const solver_rules& S = kLobpcgRules;
    SPMV_REQUIRE(ctx && A && X && theta && resid && iters, "%s: null argument", S.who);
    SPMV_REQUIRE(A->nrow == A->ncol, "%s: %s is %d x %d, not square", S.who, S.matrix, A->nrow, A->ncol);
    SPMV_REQUIRE(k >= 1 && k <= SPMV_LOBPCG_MAX_K, "%s: k = %d vectors in the block, must be 1 .. %d", S.who, k, SPMV_LOBPCG_MAX_K);
    SPMV_REQUIRE(nev >= 1 && nev <= k, "%s: nev = %d wanted pairs, must be 1 .. k = %d", S.who, nev, k);
    SPMV_REQUIRE(A->nrow == 0 || A->nrow >= 3 * k, "%s: the matrix has %d rows, fewer than 3 k = %d: the basis [X P W] would not fit", S.who, A->nrow, 3 * k);
    SPMV_REQUIRE(X->n == (int64_t)A->nrow * k, "%s: X has %lld entries, nrow * k = %d * %d", S.who, (long long)X->n, A->nrow, k);
    SPMV_REQUIRE(max_iter >= 0 && tol >= 0.0, "%s: max_iter=%d tol=%g", S.who, max_iter, tol);
    SPMV_TRY(check_known_preconditioner(S.who, precond));
    SPMV_TRY(check_preconditioner(S, A, precond));
    *iters = 0;
    for (int j = 0; j < k; ++j) theta[j] = resid[j] = 0.0;
    if (A->nrow == 0) return SPMV_OK;
    SPMV_TRY(use_device(ctx));
    return lobpcg_solve(ctx, A, k, nev, largest != 0, X->d, max_iter, tol, precond, theta, resid, iters);
}

int spmv_symgs_setup(spmv_ctx* ctx, spmv_mat* A)
{
    SPMV_REQUIRE(ctx && A, "spmv_symgs_setup: null argument");
    SPMV_REQUIRE(A->ctx == ctx, "spmv_symgs_setup: the matrix belongs to another context");
    SPMV_TRY(use_device(ctx));
    return symgs_setup(A);
}

int spmv_symgs_order(spmv_ctx* ctx, const spmv_mat* A, int32_t* order)
{
    SPMV_REQUIRE(ctx && A && (order || A->nrow == 0), "spmv_symgs_order: null argument");
    SPMV_TRY(use_device(ctx));
    return symgs_sequence(A, order);
}

int spmv_symgs(spmv_ctx* ctx, spmv_mat* A, const spmv_vec* b, spmv_vec* x, int32_t sweeps)
{
    SPMV_REQUIRE(ctx && A && b && x, "spmv_symgs: null argument");
    SPMV_REQUIRE(A->ctx == ctx, "spmv_symgs: the matrix belongs to another context");
    SPMV_TRY(check_vector_lengths("spmv_symgs", A, "b", b, "x", x));
    SPMV_REQUIRE(b->d != x->d || x->n == 0, "spmv_symgs: b and x must not alias");
    SPMV_REQUIRE(sweeps >= 0, "spmv_symgs: sweeps = %d", sweeps);
    SPMV_TRY(use_device(ctx));
    SPMV_TRY(symgs_setup(A));  // first call: split, levels, schedule (synchronous); later calls: nothing
    for (int k = 0; k < sweeps; ++k) SPMV_TRY(symgs_sweep(ctx, A, b->d, x->d, /*zero_guess=*/false));
    return SPMV_OK;
}

// ILU(0) (ilu0.hip).  Every check is made before the device is touched, so that they hold (and are tested) on a machine without one.
int spmv_ilu0_setup(spmv_ctx* ctx, spmv_mat* A)
{
    SPMV_REQUIRE(ctx && A, "spmv_ilu0_setup: null argument");
    SPMV_REQUIRE(A->ctx == ctx, "spmv_ilu0_setup: the matrix belongs to another context");
    SPMV_TRY(ilu0_check_handle(A, "spmv_ilu0_setup"));
    if (A->nrow == 0) return SPMV_OK;
    SPMV_TRY(use_device(ctx));
    return ilu0_setup(A);
}

int spmv_ilu0_solve(spmv_ctx* ctx, const spmv_mat* A, const spmv_vec* r, spmv_vec* z)
{
    SPMV_REQUIRE(ctx && A && r && z, "spmv_ilu0_solve: null argument");
    SPMV_REQUIRE(A->ctx == ctx, "spmv_ilu0_solve: the matrix belongs to another context");
    SPMV_TRY(ilu0_check_handle(A, "spmv_ilu0_solve"));
    SPMV_TRY(check_vector_pair("spmv_ilu0_solve", A, "r", r, "z", z));
    if (A->nrow == 0) return SPMV_OK;
    SPMV_TRY(use_device(ctx));
    SPMV_TRY(ilu0_setup(const_cast<spmv_mat*>(A)));  // first call: order, symbolic, numeric (synchronous); later calls: nothing
    return ilu0_apply(ctx, A, r->d, z->d);
}

int spmv_ilu0_factors(spmv_ctx* ctx, const spmv_mat* A, double* values_host)
{
    SPMV_REQUIRE(ctx && A && (values_host || A->nnz == 0), "spmv_ilu0_factors: null argument");
    SPMV_REQUIRE(A->ctx == ctx, "spmv_ilu0_factors: the matrix belongs to another context");
    SPMV_TRY(ilu0_check_handle(A, "spmv_ilu0_factors"));
    if (A->nrow == 0) return SPMV_OK;
    SPMV_TRY(use_device(ctx));
    SPMV_TRY(ilu0_setup(const_cast<spmv_mat*>(A)));
    return ilu0_factor_values(A, values_host);
}

int spmv_ilu0_order(spmv_ctx* ctx, const spmv_mat* A, int32_t* order_host)
{
    SPMV_REQUIRE(ctx && A && (order_host || A->nrow == 0), "spmv_ilu0_order: null argument");
    SPMV_REQUIRE(A->ctx == ctx, "spmv_ilu0_order: the matrix belongs to another context");
    SPMV_TRY(ilu0_check_handle(A, "spmv_ilu0_order"));
    if (A->nrow == 0) return SPMV_OK;
    SPMV_TRY(use_device(ctx));
    SPMV_TRY(ilu0_setup(const_cast<spmv_mat*>(A)));
    return ilu0_sequence(A, order_host);
}

// Triangular solves with the handle's own triangles (sptrsv.hip).  Every check is made before the device is touched.
int spmv_trsv_setup(spmv_ctx* ctx, spmv_mat* A, uint32_t flags)
{
    SPMV_REQUIRE(ctx && A, "spmv_trsv_setup: null argument");
    SPMV_TRY(trsv_check_flags(flags, "spmv_trsv_setup"));
    SPMV_REQUIRE(A->ctx == ctx, "spmv_trsv_setup: the matrix belongs to another context");
    SPMV_TRY(trsv_check_handle(A, "spmv_trsv_setup"));
    if (A->nrow == 0) return SPMV_OK;
    SPMV_TRY(use_device(ctx));
    return trsv_setup(A, flags);
}

// b and x: the same vector, or apart
static int check_trsv_vectors(const char* who, int64_t want, const char* name_b, const spmv_vec* b, const char* name_x, const spmv_vec* x)
{
    SPMV_REQUIRE(b->n == want && x->n == want, "%s: %s has %lld and %s %lld entries, %lld expected", who, name_b, (long long)b->n, name_x,
                 (long long)x->n, (long long)want);
    SPMV_REQUIRE(b->d == x->d || vectors_disjoint(b, x), "%s: %s and %s overlap in part: they may be the same vector or lie apart", who, name_b,
                 name_x);
    return SPMV_OK;
}

int spmv_trsv_solve(spmv_ctx* ctx, const spmv_mat* A, uint32_t flags, const spmv_vec* b, spmv_vec* x)
{
    SPMV_REQUIRE(ctx && A && b && x, "spmv_trsv_solve: null argument");
    SPMV_TRY(trsv_check_flags(flags, "spmv_trsv_solve"));
    SPMV_REQUIRE(A->ctx == ctx, "spmv_trsv_solve: the matrix belongs to another context");
    SPMV_TRY(trsv_check_handle(A, "spmv_trsv_solve"));
    SPMV_TRY(check_trsv_vectors("spmv_trsv_solve", A->nrow, "b", b, "x", x));
    if (A->nrow == 0) return SPMV_OK;
    SPMV_TRY(use_device(ctx));
    SPMV_TRY(trsv_setup(const_cast<spmv_mat*>(A), flags));  // first call: the working copy and its analysis (synchronous); later calls: nothing
    return trsv_apply(ctx, A, flags, b->d, x->d);
}

int spmv_trsv_solve_multi(spmv_ctx* ctx, const spmv_mat* A, uint32_t flags, int32_t k, const spmv_vec* B, spmv_vec* X)
{
    SPMV_REQUIRE(ctx && A && B && X, "spmv_trsv_solve_multi: null argument");
    SPMV_TRY(trsv_check_flags(flags, "spmv_trsv_solve_multi"));
    SPMV_REQUIRE(k >= 1 && k <= 64, "spmv_trsv_solve_multi: k = %d, must be in [1, 64]", k);
    SPMV_REQUIRE(A->ctx == ctx, "spmv_trsv_solve_multi: the matrix belongs to another context");
    SPMV_TRY(trsv_check_handle(A, "spmv_trsv_solve_multi"));
    SPMV_TRY(check_trsv_vectors("spmv_trsv_solve_multi", (int64_t)A->nrow * k, "B", B, "X", X));
    if (A->nrow == 0) return SPMV_OK;
    SPMV_TRY(use_device(ctx));
    SPMV_TRY(trsv_setup(const_cast<spmv_mat*>(A), flags));
    return trsv_apply_multi(ctx, A, flags, k, B->d, X->d);
}

int spmv_trsv_info(const spmv_mat* A, uint32_t flags, int32_t* levels, int32_t* lanes, int32_t* launches, int64_t* bytes)
{
    SPMV_REQUIRE(A, "spmv_trsv_info: null argument");
    return trsv_info(A, flags, levels, lanes, launches, bytes);
}

// The Chebyshev polynomial preconditioner and the Lanczos spectrum estimate (chebyshev.hip).  Every check is made before the device is
// touched and reads the leading fields of the handle alone, so that they hold (and are tested) on a machine without one.
int spmv_chebyshev_coefficients(int32_t degree, double lmin, double lmax, double* c0, double* c1, double* c2)
{
    return cheby_coefficients(degree, lmin, lmax, c0, c1, c2);
}

int spmv_lanczos(spmv_ctx* ctx, const spmv_mat* A, int32_t scaled, int32_t steps, uint64_t seed, double* ritz_min, double* ritz_max,
                 double* alpha, double* beta, int32_t* steps_done)
{
    SPMV_REQUIRE(ctx && A && ritz_min && ritz_max && steps_done, "spmv_lanczos: null argument");
    SPMV_REQUIRE(steps >= 1 && steps <= 64, "spmv_lanczos: steps=%d, must be 1 .. 64", steps);
    SPMV_REQUIRE(A->nrow == A->ncol && A->row_begin == 0, "spmv_lanczos: needs the whole square matrix (%d x %d, first row %lld)", A->nrow, A->ncol,
                 (long long)A->row_begin);
    if (scaled) SPMV_TRY(cheby_check_scaled(A, "spmv_lanczos"));
    *ritz_min = *ritz_max = 0.0;
    *steps_done           = 0;
    if (A->nrow == 0) return SPMV_OK;
    SPMV_TRY(use_device(ctx));
    return cheby_lanczos(ctx, A, scaled, steps, seed, ritz_min, ritz_max, alpha, beta, steps_done);
}

int spmv_chebyshev_setup(spmv_ctx* ctx, spmv_mat* A, int32_t degree, int32_t scaled, double lmin, double lmax)
{
    SPMV_REQUIRE(ctx && A, "spmv_chebyshev_setup: null argument");
    SPMV_TRY(cheby_check_setup(A, degree, scaled, lmin, lmax, "spmv_chebyshev_setup"));
    SPMV_REQUIRE(A->ctx == ctx, "spmv_chebyshev_setup: the matrix belongs to another context");
    SPMV_TRY(use_device(ctx));
    return cheby_setup(ctx, A, degree, scaled, lmin, lmax);
}

int spmv_chebyshev_info(const spmv_mat* A, int32_t* degree, int32_t* scaled, double* lmin, double* lmax)
{
    SPMV_REQUIRE(A && degree && scaled && lmin && lmax, "spmv_chebyshev_info: null argument");
    return cheby_info(A, degree, scaled, lmin, lmax);
}

int spmv_chebyshev_solve(spmv_ctx* ctx, const spmv_mat* A, const spmv_vec* r, spmv_vec* z)
{
    SPMV_REQUIRE(ctx && A && r && z, "spmv_chebyshev_solve: null argument");
    SPMV_TRY(cheby_check_handle(A, "spmv_chebyshev_solve"));
    SPMV_TRY(check_vector_pair("spmv_chebyshev_solve", A, "r", r, "z", z));
    if (A->nrow == 0) return SPMV_OK;
    SPMV_TRY(use_device(ctx));
    return cheby_apply(ctx, A, r->d, z->d);
}

// Aggregation AMG (amg.hip).  Every check is made before the device is touched.
int spmv_amg_setup(spmv_ctx* ctx, spmv_mat* A, int32_t max_levels, int32_t coarse_max, int32_t smooth_degree, double strength, double overcorrection)
{
    SPMV_REQUIRE(ctx && A, "spmv_amg_setup: null argument");
    SPMV_TRY(amg_check_setup(A, max_levels, coarse_max, smooth_degree, strength, overcorrection, "spmv_amg_setup"));
    SPMV_REQUIRE(A->ctx == ctx, "spmv_amg_setup: the matrix belongs to another context");
    SPMV_TRY(use_device(ctx));
    return amg_setup(ctx, A, max_levels, coarse_max, smooth_degree, strength, overcorrection);
}

int spmv_amg_setup_smoothed(spmv_ctx* ctx, spmv_mat* A, int32_t max_levels, int32_t coarse_max, int32_t smooth_degree, double strength,
                            double overcorrection, double prolong_damping)
{
    const char* const who = "spmv_amg_setup_smoothed";
    SPMV_REQUIRE(ctx && A, "%s: null argument", who);
    SPMV_TRY(amg_check_setup_smoothed(A, max_levels, coarse_max, smooth_degree, strength, overcorrection, prolong_damping, who));
    SPMV_REQUIRE(A->ctx == ctx, "%s: the matrix belongs to another context", who);
    SPMV_TRY(use_device(ctx));
    return amg_setup_smoothed(ctx, A, max_levels, coarse_max, smooth_degree, strength, overcorrection, prolong_damping);
}

int spmv_amg_prolongator(spmv_ctx* ctx, const spmv_mat* A, int32_t level, int64_t* nnz, int32_t* row_ptr, int32_t* col, double* val)
{
    const char* const who = "spmv_amg_prolongator";
    SPMV_REQUIRE(ctx && A && nnz, "%s: null argument", who);
    SPMV_TRY(amg_check_handle(A, who));
    if (!A->amg) SPMV_FAIL(SPMV_ERR_INVALID, "%s: the handle was not set up (spmv_amg_setup_smoothed)", who);
    SPMV_TRY(use_device(ctx));
    return amg_prolongator_download(ctx, A, level, nnz, row_ptr, col, val);
}

int spmv_amg_transfer_timed(spmv_ctx* ctx, const spmv_mat* A, int32_t level, int32_t what, int32_t lanes, spmv_vec* v, int32_t reps, double* ms_per_call)
{
    const char* const who = "spmv_amg_transfer_timed";
    SPMV_REQUIRE(ctx && A && v && ms_per_call, "%s: null argument", who);
    SPMV_REQUIRE(reps > 0, "%s: reps=%d", who, reps);
    SPMV_TRY(amg_check_handle(A, who));
    SPMV_TRY(amg_check_transfer(A, level, what, lanes, v->n, who));
    SPMV_TRY(use_device(ctx));
    void* t = nullptr;
    if (hipMalloc(&t, sizeof(double) * (size_t)std::max<int64_t>(v->n, 1)) != hipSuccess)
    {
        (void)hipGetLastError();
        SPMV_FAIL(SPMV_ERR_ALLOC, "%s: out of device memory for a work vector of %lld entries", who, (long long)v->n);
    }
    float     ms = 0.f;
    const int rc = time_launches(ctx, reps, [&] { return amg_transfer_launch(ctx, A, level, what, lanes, v->d, (double*)t); }, &ms);
    (void)hipStreamSynchronize(ctx->stream);
    (void)hipFree(t);
    SPMV_TRY(rc);
    *ms_per_call = ms;
    return SPMV_OK;
}

int spmv_amg_info(const spmv_mat* A, int32_t* levels, int64_t* rows, int64_t* nnz)
{
    SPMV_REQUIRE(A && levels, "spmv_amg_info: null argument");
    return amg_info(A, levels, rows, nnz);
}

int spmv_amg_level(spmv_ctx* ctx, const spmv_mat* A, int32_t level, int32_t* agg_host, int32_t* row_ptr, int32_t* col, double* val)
{
    SPMV_REQUIRE(ctx && A, "spmv_amg_level: null argument");
    SPMV_TRY(amg_check_handle(A, "spmv_amg_level"));
    if (!A->amg) SPMV_FAIL(SPMV_ERR_INVALID, "spmv_amg_level: the handle was not set up (spmv_amg_setup)");
    SPMV_TRY(use_device(ctx));
    return amg_level_download(ctx, A, level, agg_host, row_ptr, col, val);
}

int spmv_amg_solve(spmv_ctx* ctx, const spmv_mat* A, const spmv_vec* r, spmv_vec* z)
{
    SPMV_REQUIRE(ctx && A && r && z, "spmv_amg_solve: null argument");
    SPMV_TRY(amg_check_handle(A, "spmv_amg_solve"));
    SPMV_TRY(check_vector_pair("spmv_amg_solve", A, "r", r, "z", z));
    if (!A->amg) SPMV_FAIL(SPMV_ERR_INVALID, "spmv_amg_solve: the handle was not set up (spmv_amg_setup)");
    if (A->nrow == 0) return SPMV_OK;
    SPMV_TRY(use_device(ctx));
    return amg_apply(ctx, A, r->d, z->d);
}

// FSAI (fsai.hip).  Every check is made before the device is touched and reads the leading fields of the handle alone.
int spmv_fsai_setup(spmv_ctx* ctx, spmv_mat* A, int32_t level)
{
    const char* const who = "spmv_fsai_setup";
    SPMV_REQUIRE(ctx && A, "%s: null argument", who);
    SPMV_TRY(fsai_check_level(level, who));
    SPMV_TRY(fsai_check_handle(A, who));
    SPMV_REQUIRE(A->ctx == ctx, "%s: the matrix belongs to another context", who);
    if (A->nrow > 0) SPMV_TRY(use_device(ctx));
    return fsai_setup(ctx, A, level);
}

int spmv_fsai_solve(spmv_ctx* ctx, const spmv_mat* A, const spmv_vec* r, spmv_vec* z)
{
    const char* const who = "spmv_fsai_solve";
    SPMV_REQUIRE(ctx && A && r && z, "%s: null argument", who);
    SPMV_TRY(fsai_check_handle(A, who));
    SPMV_REQUIRE(A->ctx == ctx, "%s: the matrix belongs to another context", who);
    SPMV_TRY(check_vector_pair(who, A, "r", r, "z", z));
    if (!A->fsai) SPMV_FAIL(SPMV_ERR_INVALID, "%s: the handle was not set up (spmv_fsai_setup)", who);
    if (A->nrow == 0) return SPMV_OK;
    SPMV_TRY(use_device(ctx));
    return fsai_apply(ctx, A, r->d, z->d);
}

int spmv_fsai_info(const spmv_mat* A, int32_t* level, int64_t* nnz, int32_t* max_row)
{
    SPMV_REQUIRE(A && level && nnz && max_row, "spmv_fsai_info: null argument");
    return fsai_info(A, level, nnz, max_row);
}

int spmv_fsai_factor(spmv_ctx* ctx, const spmv_mat* A, int64_t* nnz, int32_t* row_ptr, int32_t* col, double* val)
{
    const char* const who = "spmv_fsai_factor";
    SPMV_REQUIRE(ctx && A && nnz, "%s: null argument", who);
    SPMV_TRY(fsai_check_handle(A, who));
    SPMV_REQUIRE(A->ctx == ctx, "%s: the matrix belongs to another context", who);
    if (!A->fsai) SPMV_FAIL(SPMV_ERR_INVALID, "%s: the handle was not set up (spmv_fsai_setup)", who);
    if (A->nrow > 0) SPMV_TRY(use_device(ctx));
    return fsai_factor_download(ctx, A, nnz, row_ptr, col, val);
}

int spmv_chebyshev(spmv_ctx* ctx, spmv_mat* A, const spmv_vec* b, spmv_vec* x)
{
    SPMV_REQUIRE(ctx && A && b && x, "spmv_chebyshev: null argument");
    SPMV_TRY(cheby_check_handle(A, "spmv_chebyshev"));
    SPMV_TRY(check_vector_pair("spmv_chebyshev", A, "b", b, "x", x));
    if (A->nrow == 0) return SPMV_OK;
    SPMV_TRY(use_device(ctx));
    return cheby_smooth(ctx, A, b->d, x->d);
}

// ---- sparse products (spgemm.hip).  Every check but the two counts is made before the device is touched. ---
int spmv_spgemm(spmv_ctx* ctx, const spmv_mat* A, const spmv_mat* B, int32_t method, spmv_mat** out_C)
{
    SPMV_REQUIRE(ctx && A && B && out_C, "spmv_spgemm: null argument");
    SPMV_TRY(spgemm_check(ctx, A, B, method, "spmv_spgemm"));
    SPMV_TRY(use_device(ctx));
    return spgemm(ctx, A, B, method, out_C);
}

int spmv_csr_transpose(spmv_ctx* ctx, const spmv_mat* A, spmv_mat** out_At)
{
    SPMV_REQUIRE(ctx && A && out_At, "spmv_csr_transpose: null argument");
    SPMV_TRY(csr_transpose_check(ctx, A, "spmv_csr_transpose"));
    SPMV_TRY(use_device(ctx));
    return csr_transpose(ctx, A, out_At);
}

// ---- conversions ------------------------------------------------------------------------------------------
// a converted ELL handle gets the same analysis as an uploaded one (kernel choice, regrouped copy when it pays)
static int analyse_new_ell(spmv_mat** out)
{
    const int rc = ell_analyse(*out);
    if (rc != SPMV_OK)
    {
        mat_free(*out);
        *out = nullptr;
    }
    return rc;
}

int spmv_coo_to_csr(spmv_ctx* ctx, const spmv_mat* coo, spmv_mat** out_csr)
{
    SPMV_REQUIRE(ctx && coo && out_csr, "spmv_coo_to_csr: null argument");
    SPMV_TRY(use_device(ctx));
    plan_arm arm(ctx);
    return coo_to_csr(ctx, coo, out_csr);
}

int spmv_csr_to_ell(spmv_ctx* ctx, const spmv_mat* csr, spmv_mat** out_ell)
{
    SPMV_REQUIRE(ctx && csr && out_ell, "spmv_csr_to_ell: null argument");
    SPMV_TRY(use_device(ctx));
    plan_arm arm(ctx);
    SPMV_TRY(csr_to_ell(ctx, csr, out_ell));
    return analyse_new_ell(out_ell);
}

int spmv_csr_split_columns(spmv_ctx* ctx, const spmv_mat* csr, int32_t col_begin, int32_t col_end, spmv_mat** out_inside,
                           spmv_mat** out_outside)
{
    SPMV_REQUIRE(ctx && csr && out_inside && out_outside, "spmv_csr_split_columns: null argument");
    SPMV_TRY(use_device(ctx));
    spmv_mat *in = nullptr, *outm = nullptr;
    SPMV_TRY(csr_split_columns(ctx, csr, col_begin, col_end, &in, &outm));
    int rc = finish(in, out_inside);  // validates and analyses like an uploaded handle (frees on failure)
    if (rc != SPMV_OK)
    {
        mat_free(outm);
        return rc;
    }
    rc = finish(outm, out_outside);
    if (rc != SPMV_OK)
    {
        mat_free(*out_inside);
        *out_inside = nullptr;
    }
    return rc;
}

int spmv_coo_to_ell(spmv_ctx* ctx, const spmv_mat* coo, spmv_mat** out_ell)
{
    SPMV_REQUIRE(ctx && coo && out_ell, "spmv_coo_to_ell: null argument");
    SPMV_TRY(use_device(ctx));
    spmv_mat* csr = nullptr;
    SPMV_TRY(coo_to_csr(ctx, coo, &csr));
    int rc = csr_to_ell(ctx, csr, out_ell);
    mat_free(csr);
    plan_arm arm(ctx);  // (for the ELL handle: the intermediate CSR form above selected as usual)
    return rc == SPMV_OK ? analyse_new_ell(out_ell) : rc;
}

// ---- sharding ---------------------------------------------------------------------------------------------
int spmv_partition_rows(int64_t nrow, int32_t nparts, int32_t part, int64_t* row_begin, int64_t* row_end)
{
    SPMV_REQUIRE(nrow >= 0 && nparts > 0 && part >= 0 && part < nparts && row_begin && row_end,
                 "spmv_partition_rows: nrow=%lld nparts=%d part=%d", (long long)nrow, nparts, part);
    // src/mat_vec.cpp:233,245-246: rows_per_thread = nrow / nthreads, the last part takes the remainder
    const int64_t per = nrow / nparts;
    *row_begin        = (int64_t)part * per;
    *row_end          = (part == nparts - 1) ? nrow : *row_begin + per;
    return SPMV_OK;
}

int spmv_partition_rows_balanced(int64_t nrow, const int64_t* row_ptr64, int32_t nparts, int64_t* bounds)
{
    SPMV_REQUIRE(nrow >= 0 && row_ptr64 && nparts > 0 && bounds, "spmv_partition_rows_balanced: bad argument");
    const int64_t nnz = row_ptr64[nrow] - row_ptr64[0];
    bounds[0]         = 0;
    for (int32_t p = 1; p < nparts; ++p)
    {
        // the row boundary whose offset lies NEAREST to p / nparts of the entries (a row is never split; ties go to the later
        // boundary), kept monotonic
        const int64_t  target = row_ptr64[0] + (int64_t)(((__int128)nnz * p) / nparts);
        const int64_t* it     = std::lower_bound(row_ptr64, row_ptr64 + nrow + 1, target);
        int64_t        r      = it - row_ptr64;
        if (r > nrow) r = nrow;
        if (r > 0 && target - row_ptr64[r - 1] < row_ptr64[r] - target) --r;
        if (r < bounds[p - 1]) r = bounds[p - 1];
        bounds[p] = r;
    }
    bounds[nparts] = nrow;
    return SPMV_OK;
}

// bounds of a row partition of a device-resident handle (columns for CSC, which the reference shards by column)
int spmv_mat_partition_rows(const spmv_mat* m, int32_t nparts, int32_t balance_entries, int64_t* bounds)
{
    SPMV_REQUIRE(m && nparts > 0 && bounds, "spmv_mat_partition_rows: bad argument");
    if (m->format == SPMV_FMT_BSR && balance_entries)
        SPMV_FAIL(SPMV_ERR_UNSUPPORTED, "spmv_mat_partition_rows: a BSR handle is not sharded: no partition by entries (balance_entries = 1)");
    if (m->format == SPMV_FMT_CSR_F32 && balance_entries)
        SPMV_FAIL(SPMV_ERR_UNSUPPORTED, "spmv_mat_partition_rows: a handle of format 6 is not sharded: no partition by entries (balance_entries = 1)");
    const int64_t n = m->format == SPMV_FMT_CSC ? m->ncol : m->nrow;
    // padded formats store the same number of slots for every row: equal rows ARE equal work
    if (!balance_entries || m->format == SPMV_FMT_ELL || m->format == SPMV_FMT_DIA || n == 0)
    {
        for (int32_t p = 0; p < nparts; ++p)
        {
            int64_t b = 0, e = 0;
            SPMV_TRY(spmv_partition_rows(n, nparts, p, &b, &e));
            bounds[p]     = b;
            bounds[p + 1] = e;
        }
        return SPMV_OK;
    }
    std::vector<int64_t> rp64((size_t)n + 1);
    if (m->format == SPMV_FMT_COO)
        SPMV_TRY(coo_row_offsets(m, rp64.data()));
    else
    {
        SPMV_REQUIRE(m->a, "spmv_mat_partition_rows: the handle has no offset array");
        std::vector<int32_t> rp((size_t)n + 1);
        SPMV_HIP(hipSetDevice(m->ctx->device));
        SPMV_HIP(hipMemcpyAsync(rp.data(), m->a, sizeof(int32_t) * rp.size(), hipMemcpyDeviceToHost, m->ctx->stream));
        SPMV_HIP(hipStreamSynchronize(m->ctx->stream));
        for (size_t i = 0; i < rp.size(); ++i) rp64[i] = rp[i];
    }
    return spmv_partition_rows_balanced(n, rp64.data(), nparts, bounds);
}

int spmv_csr_extract_rows(spmv_ctx* dst_ctx, const spmv_mat* csr, int64_t row_begin, int64_t row_end, spmv_mat** out)
{
    SPMV_REQUIRE(dst_ctx && csr && out, "spmv_csr_extract_rows: null argument");
    int before = -1;
    if (hipGetDevice(&before) != hipSuccess) before = -1;
    spmv_mat* m  = nullptr;
    plan_arm  arm(dst_ctx);
    int       rc = csr_extract_rows(dst_ctx, csr, row_begin, row_end, &m);
    if (rc == SPMV_OK) rc = finish(m, out);  // validates and analyses like an uploaded shard (frees on failure)
    if (before >= 0) (void)hipSetDevice(before);
    return rc;
}

// ---- generators -------------------------------------------------------------------------------------------
int spmv_gen_csr_uniform(spmv_ctx* ctx, int64_t row_begin, int64_t row_end, int32_t ncol, int32_t k, int32_t band,
                         uint64_t seed, spmv_mat** out)
{
    SPMV_REQUIRE(ctx && out, "spmv_gen_csr_uniform: null argument");
    SPMV_TRY(use_device(ctx));
    plan_arm arm(ctx);
    return gen_csr_uniform(ctx, row_begin, row_end, ncol, k, band, seed, out);
}

int spmv_gen_ell_banded(spmv_ctx* ctx, int32_t nrow, int32_t ncol, int32_t k, uint64_t seed, spmv_mat** out)
{
    SPMV_REQUIRE(ctx && out, "spmv_gen_ell_banded: null argument");
    SPMV_TRY(use_device(ctx));
    plan_arm arm(ctx);
    SPMV_TRY(gen_ell_banded(ctx, nrow, ncol, k, seed, out));
    return analyse_new_ell(out);
}

int spmv_gen_dia_banded(spmv_ctx* ctx, int32_t nrow, int32_t k, uint64_t seed, spmv_mat** out)
{
    SPMV_REQUIRE(ctx && out, "spmv_gen_dia_banded: null argument");
    SPMV_TRY(use_device(ctx));
    return gen_dia_banded(ctx, nrow, k, seed, out);
}

int spmv_gen_coo_powerlaw(spmv_ctx* ctx, int32_t nrow, int32_t ncol, int32_t max_len, uint64_t seed, spmv_mat** out)
{
    SPMV_REQUIRE(ctx && out, "spmv_gen_coo_powerlaw: null argument");
    SPMV_TRY(use_device(ctx));
    plan_arm arm(ctx);
    return gen_coo_powerlaw(ctx, nrow, ncol, max_len, seed, false, out);
}

int spmv_gen_coo_powerlaw_sorted(spmv_ctx* ctx, int32_t nrow, int32_t ncol, int32_t max_len, uint64_t seed, spmv_mat** out)
{
    SPMV_REQUIRE(ctx && out, "spmv_gen_coo_powerlaw_sorted: null argument");
    SPMV_TRY(use_device(ctx));
    plan_arm arm(ctx);
    return gen_coo_powerlaw(ctx, nrow, ncol, max_len, seed, true, out);
}

int spmv_gen_vec_uniform(spmv_ctx* ctx, spmv_vec* v, int64_t index_offset, uint64_t seed)
{
    SPMV_REQUIRE(ctx && v, "spmv_gen_vec_uniform: null argument");
    SPMV_TRY(use_device(ctx));
    return gen_vec_uniform(ctx, v->d, v->n, index_offset, seed);
}

}  // extern "C"
