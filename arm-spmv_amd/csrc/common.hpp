// common.hpp — internal types shared by the translation units of libspmv_hip.so.
// Not part of the ABI (include/spmv_abi.h is).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <vector>

#include "ell_settings.hpp"
#include "spmv_abi.h"

namespace spmv
{
// ---- error plumbing -----------------------------------------------------------------------------
void set_error(const char* fmt, ...) __attribute__((format(printf, 1, 2)));

#define SPMV_FAIL(code, ...)            \
    do                                  \
    {                                   \
        ::spmv::set_error(__VA_ARGS__); \
        return (code);                  \
    } while (0)

#define SPMV_HIP(call)                                                                     \
    do                                                                                     \
    {                                                                                      \
        hipError_t e_ = (call);                                                            \
        if (e_ != hipSuccess)                                                              \
            SPMV_FAIL(SPMV_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), \
                      __FILE__, __LINE__);                                                 \
    } while (0)

#define SPMV_TRY(call)          \
    do                          \
    {                           \
        int rc_ = (call);       \
        if (rc_ != 0) return rc_; \
    } while (0)

#define SPMV_REQUIRE(cond, ...) \
    do                          \
    {                           \
        if (!(cond)) SPMV_FAIL(SPMV_ERR_INVALID, __VA_ARGS__); \
    } while (0)

// ---- chip constants (MI355X / gfx950) -------------------------------------------------------------
constexpr int kWave      = 64;   // wavefront width
constexpr int kBlock     = 256;  // default workgroup: 4 waves, one per SIMD
constexpr int kNumXcd    = 8;
constexpr int kNumCu     = 256;
constexpr int kMaxGrid   = kNumCu * 8;  // grid-stride cap for streaming kernels (8 blocks / CU)

static inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
// workgroups of a grid-stride kernel over n elements, one per thread: at least one, at most kMaxGrid
static inline int stream_grid(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>(kMaxGrid, ceil_div(n, kBlock))); }

// ---- counter-based PRNG shared by the device generators and their numpy twin ------------------------
// splitmix64 finaliser; stream keys are derived on the host, the device adds the element index.
__host__ __device__ static inline uint64_t splitmix64(uint64_t z)
{
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
enum : uint64_t
{
    kStreamCol = 1,
    kStreamVal = 2,
    kStreamVec = 3,
    kStreamLen = 4
};
static inline uint64_t stream_key(uint64_t seed, uint64_t stream)
{
    return splitmix64(seed ^ (0x9E3779B97F4A7C15ull * (stream + 1)));
}
__host__ __device__ static inline double u64_to_unit(uint64_t r)  // [0,1)
{
    return (double)(r >> 11) * 0x1.0p-53;
}
__host__ __device__ static inline double u64_to_sym(uint64_t r)  // [-1,1)
{
    return (double)(r >> 11) * 0x1.0p-52 - 1.0;
}
__host__ __device__ static inline uint32_t u64_to_range(uint64_t r, uint32_t n)  // [0,n)
{
    return (uint32_t)(((r >> 32) * (uint64_t)n) >> 32);
}
}  // namespace spmv

// ---- the opaque ABI types ---------------------------------------------------------------------------
struct spmv_ctx
{
    int         device      = 0;
    hipStream_t stream      = nullptr;
    bool        owns_stream = false;
    hipEvent_t  ev_begin    = nullptr;
    hipEvent_t  ev_end      = nullptr;
    // small persistent scratch (dot partials, flags); grown on demand outside hot loops
    void*  scratch       = nullptr;
    size_t scratch_bytes = 0;
    double* host_pinned  = nullptr;  // 64 B of pinned host memory for scalar results
    double* dev_scalars  = nullptr;  // one slotted accumulator (kDotDoubles) for scalar results; never re-allocated
    // Start-up probe (abi.hip: xcd_probe): are the workgroups of a launch dealt round-robin over 8 XCDs, so that workgroups b
    // and b + 8 share an XCD (and its L2) and b, b + 1, ..., b + 7 sit on 8 different ones?  1 yes / 0 no (a partitioned
    // device, another dispatch order) / -1 the probe could not run.  Layouts that lean on it for SPEED (the COO scan over one
    // column bin per XCD) are not built when it is not 1; nothing leans on it for correctness.
    int32_t xcd_round_robin = -1;
    int32_t xcds_seen       = 0;
    int64_t cg_graph_replays = 0;  // spmv_cg under SPMV_CG_GRAPH=1: launches of the captured four iterations so far (tests read it)
    // spmv_apply_host (abi.hip): the caller's HOST vectors staged through pinned, device-mapped host memory (small vectors: the
    // GPU copies them in and out itself, one stream, no hipMemcpy) and device buffers for x and y; grown on demand
    double* stage_pinned     = nullptr;  // host address
    double* stage_pinned_dev = nullptr;  // the same memory as the GPU sees it
    size_t  stage_pinned_n   = 0;        // doubles
    double* stage_x = nullptr;
    double* stage_y = nullptr;
    size_t  stage_x_n = 0, stage_y_n = 0;
    // spmv_ctx_set_plan: handles created on this context take this plan instead of selecting (plan.hip); `plan_armed` is set by
    // the public entry point that creates a handle and consumed by that handle's analysis (its children get theirs handed down)
    std::vector<unsigned char> plan_blob;
    bool                       plan_armed = false;
    // can the CPU store straight into device memory (large BAR: hipDeviceAttributeIsLargeBar)?  Then spmv_apply_host writes a
    // small x into its device buffer itself (80 KB in 2 us) instead of launching a kernel that pulls it over the host link;
    // hdp_flush: the HDP flush register (hipDeviceAttributeHdpMemFlushCntl), written after such stores
    int32_t            large_bar = 0;
    volatile unsigned* hdp_flush = nullptr;
    // the trial arena (select.hip): ONE allocation that the timing launches of AUTO carve their scratch vectors from, so that no
    // hipMalloc / hipFree falls between a candidate's build and its timing window; grown between trials, freed with the context
    void*  arena       = nullptr;
    size_t arena_bytes = 0;
    int    arena_users = 0;  // trials holding pointers into it (it is not re-allocated while > 0)
    // spmv_block_gram / spmv_block_combine (block_ops.hip): a ticket, the small matrix and the partial sums on the device (grown on
    // demand), the small matrix once more in pinned host memory, and the event behind the last copy out of it; freed with the context
    void*      block_dev       = nullptr;
    size_t     block_dev_bytes = 0;
    double*    block_pinned    = nullptr;
    hipEvent_t block_ev        = nullptr;
};

namespace spmv
{
struct symgs_plan;
struct ilu0_plan;
struct cheby_state;
struct amg_state;
struct fsai_state;
struct transpose_state;
struct trsv_state;
// ---- plans (plan.hip): the decisions a handle's set-up made - by model or by timing - as plain data ------------------------------
// One node per handle, children by index (the row-grouped copy of a COO / CSC / ELL handle or the short-row copy of a split,
// the long rows' matrix of a split in virtual-row mode, the ELL copy of a CSR handle).  32 four-byte fields, no pointers:
// the blob of spmv_mat_get_plan is a plan_header followed by nnodes plan_node, node 0 the handle itself.
struct plan_node
{
    int32_t  format, kernel, lanes_per_row;
    uint32_t flags;
    int32_t  pb_group_rows, pb_width, pb_sort, pb_aos, pb_unroll, pb_pipe, pb_sync, pb_two_per_cu, pb_rounds;
    int32_t  split_threshold, split_mode;
    int32_t  tp_pcols, tp_rotate;
    int32_t  ell_variant, ell_tiled;
    int32_t  coo_bins_per_xcd;
    int32_t  child_rowgrouped, child_long, child_ell;  // node indices, -1: none
    int32_t  reserved[9];
};
static_assert(sizeof(plan_node) == 128, "plan_node is 32 four-byte fields");
struct plan_header
{
    uint32_t magic, version, bytes, nnodes;
};
constexpr uint32_t kPlanMagic = 0x4e4c5053u;  // "SPLN"
constexpr uint32_t kPlanVersion = 1;
}

struct spmv_vec
{
    spmv_ctx* ctx   = nullptr;
    int64_t   n     = 0;
    double*   d     = nullptr;
    bool      owned = false;
};

struct spmv_mat
{
    spmv_ctx* ctx       = nullptr;
    int32_t   format    = 0;
    int32_t   nrow      = 0;
    int32_t   ncol      = 0;
    int32_t   k         = 0;  // ELL slots / DIA ndiags / BSR block size bs
    int64_t   nnz       = 0;
    int64_t   row_begin = 0;
    // a: row_ptr | row_ind | -       | col_ptr | offsets | block row_ptr | row_ptr
    // b: col_ind | col_ind | col_ind | row_ind | -       | block col_ind | -       (CSR | COO | ELL | CSC | DIA | BSR | CSR_F32: f32_ent below)
    const int32_t* a = nullptr;
    const int32_t* b = nullptr;
    const double*  v = nullptr;
    bool           owned        = false;
    int64_t        device_bytes = 0;

    // ---- analysis results (filled by analyse_*) ----
    bool    dia_off_known = false;  // DIA: smallest / largest diagonal offset (set where the offsets pass through the host)
    int32_t dia_off_min = 0, dia_off_max = 0;
    int32_t dia_col_bound = 0;  // DIA: columns >= this are skipped (0 = min(nrow, ncol)); row shards keep the global bound
    int32_t max_row_nnz   = 0;
    int32_t kernel        = SPMV_CSR_AUTO;
    int32_t lanes_per_row = 0;
    int32_t sorted_rows   = 0;
    bool    kernel_forced = false;
    uint32_t flags        = 0;  // SPMV_FLAG_* tuning bits

    // CSR LDS-window kernel: per row-block [lo, hi) column window
    int32_t  win_rows  = 0;        // rows per workgroup
    int32_t* win_lo    = nullptr;  // [nblocks] first column touched by the block
    int32_t* win_span  = nullptr;  // [nblocks] hi - lo
    int32_t  win_max_span = 0;

    double   win_avg_span = 0.0;   // mean over row blocks: how local the columns are
    double   contig_frac  = 0.0;   // CSR: fraction of the entries whose column is the previous entry's + 1 (dense blocks, bands)

    // AUTO selection by measurement (select.hip): candidates timed when the handle was analysed, microseconds per product
    // by slot (spmv::select_slot below); 0 = not timed
    int32_t  sel_candidates = 0;
    float    sel_us[10]     = {0};  // [spmv::kSelSlots]
    int32_t  sel_rounds     = 0;  // rounds the last trial went through until its minima stood still ("select_rounds")

    // CSR panel kernel (kernels_csr_panel.hip): entries re-ordered per row group by column panel / x line
    int32_t*  pb_col         = nullptr;  // [nnz] global column
    uint16_t* pb_row         = nullptr;  // [nnz] row inside its group
    double*   pb_val         = nullptr;  // [nnz]
    int32_t*  pb_gstart      = nullptr;  // [ngroups + 1] first row of every group (entry-balanced unless G was requested)
    int32_t   pb_group_rows  = 0;        // G (0 = choose)
    int32_t   pb_panel_width = 0;        // W (0 = default)
    int32_t   pb_sort        = 1;        // bucket tile entries by 128-byte line of x
    int32_t   pb_unroll      = 0;        // entries in flight per lane (0 = default)
    int32_t   pb_aos         = 4;        // layout: 4 = 12-byte packed entries, slices in interleaved pairs (falls back to 0), 3 = the same
                                         // without the pairing, 0 = three arrays (14 bytes)
    uint32_t* pb_pack        = nullptr;  // [nnz] layout 3: (column - slice base) << rowbits | local row
    int32_t*  pb_sbase       = nullptr;  // [slices] layout 3: line-aligned first column of every 1024-entry slice
    int32_t*  pb_soff        = nullptr;  // [ngroups + 1] layout 3: first slice of every group
    int32_t   pb_rowbits     = 0;
    bool      pb_pair        = false;    // layout 4: slices stored in interleaved pairs
    int32_t   pb_slices      = 0;        // layout 3: 1024-entry slices in all (padded entries / 1024)
    int32_t   pb_built_layout = -1;      // pb_aos the layout in memory was built for
    int32_t   pb_pipe        = -1;      // chunk pipeline: 0 off, 1 stream-first, 2 gather-first, -1 = 1 or 2 by trial
    int32_t   pb_pipe_tuned  = 0;       // the order found by trying (in effect while pb_pipe == -1; 0 = not tried: 1)
    int32_t   pb_tuned_key   = 0;        // what the build-time trial was made for (requested unroll / order / sync); 0 = not tried
    int32_t   pb_unroll_tuned = 0;       // chunk size found by trying (in effect while pb_unroll == 0)
    int64_t   pb_max_group_nnz = 0;      // entries of the fullest row group
    int32_t   pb_sync        = -1;       // keep a workgroup's wavefronts together: 0 no, 1 barrier per chunk, 2 priority to late ones,
                                         // 3 barrier between a chunk's loads and its LDS adds; -1 = by trial
    int32_t   pb_sync_tuned  = 0;        // what the trial found (in effect while pb_sync == -1)
    int32_t   pb_trial       = -1;       // timing launches when the layout is built: 1 yes, 0 no, -1 = SPMV_PANEL_TRIAL (default yes)
    int32_t   pb_two_per_cu  = 1;        // allow two workgroups per CU when the accumulators fit twice
    int32_t   pb_ngroups     = 0;
    int32_t   pb_rounds_req  = 0;        // groups for k rounds of 256 workgroups instead of the fewest the LDS cap allows (0: one round's worth unless
                                         // skewed rows make a finer cut worth a timing, 1: never)
    int32_t   pb_built_rounds = 0;       // what the layout in memory was cut for
    float     pb_rounds_us[2] = {0.f, 0.f};  // the timing that decided: the single round, the finer cut (microseconds per product; 0 = not timed)
    int32_t   pb_max_rows    = 0;        // rows of the fullest group (sizes the LDS accumulators)
    int32_t   pb_built_rows = 0, pb_built_width = 0, pb_built_sort = -1;  // parameters of the layout in memory
    int64_t   pb_bytes       = 0;

    // CSR two-phase kernel (kernels_csr_twophase.hip): entries in (column panel, row group) order
    double*   tp_val       = nullptr;  // [padded] (panel, group) order, runs padded to 16 entries
    uint16_t* tp_col       = nullptr;  // [padded] column - panel base, same order
    uint16_t* tp_row       = nullptr;  // [padded] row - group base, (group, panel) order; 0xFFFF = padding
    double*   tp_piece[4] = {};        // the stream between the two phases, (group, panel) order, in pieces of 2^26 pairs (1 GB)
    bool      tp_piece_carved[4] = {}; // the piece lies inside tp_parent[] (an allocation taken over from the released CSR copy), not its own
    void*     tp_parent[2] = {};       // allocations of the CSR copy (values, column indices) the product stream took over at panel_keep_csr = 0
    int32_t   tp_carve_taken = 0;      // bit k: the last search took allocation k of those on offer
    int32_t   tp_offer_csr = 1;        // panel_keep_csr = 0 offers the CSR copy's gigabytes to the piece search first (0: A/B, just release them)
    int32_t   tp_npieces   = 0;
    void*     tp_pool      = nullptr;  // experiments: a pool of pieces (kernels_csr_twophase.hip: tp_pool)
    int64_t   tp_last_piece_bytes = 0;  // the last piece: a whole one when the piece search ran, else what the stream needs of it
    int32_t*  tp_blk       = nullptr;  // [2 * ceil(padded / 16)] two table words per source line: source pair -> destination pair
    int32_t*  tp_panel_ptr = nullptr;  // [panels + 1]
    int32_t*  tp_group_ptr = nullptr;  // [groups + 1]
    int32_t*  tp_gstart    = nullptr;  // [groups + 1] first row of every group
    int32_t   tp_ngroups = 0, tp_panels = 0, tp_pcols = 0, tp_max_rows = 0;
    int32_t   tp_pcols_req = 0;  // requested panel width (0 = default)
    int32_t   tp_place_budget_mb = -1;          // memory the piece search may hold beyond the stream (-1: SPMV_TP_PLACEMENT_BUDGET_MB or 8192; 0: no search)
    int32_t   tp_pieces_exchanged = 0;               // pieces of the stream the search exchanged for others
    int32_t   tp_rotate = 256;                  // expand kernel: distinct starting points of the workgroups inside their panels (0 / 1: none)
    int32_t   tp_only = 0;                      // experiment (SPMV_EXPERIMENTS=1): 1 / 2 = run phase A / B alone - wrong results
    int32_t   tp_place_seen = 0, tp_place_gain = 0;  // placements of the product stream timed at build; slowest / kept, in 1/1000
    int64_t   tp_padded = 0;
    int64_t   tp_bytes   = 0;

    // CSR segmented-scan kernel (kernels_coo.hip: csr_segscan_build): the row of every entry
    int32_t* seg_row = nullptr;  // [nnz]
    bool     sel_no_segscan = false;  // the handle is the row-grouped copy of a COO handle: that handle's own kernel IS this scan

    // CSR handle of (nearly) equal rows: an ELL copy of it with a handle - and kernels, diagonal slots included - of its own
    // (kernels_ell.hip: csr_ell_copy_build; kernel SPMV_CSR_ELL); owned
    spmv_mat* ell_copy = nullptr;
    int32_t   min_row_nnz = 0;
    bool      sel_no_ell = false;  // the handle is itself somebody's copy whose source is an ELL handle
    bool      sel_no_rowgrouped = false;  // ELL: the handle is the ELL copy of a CSR handle (no row-grouped copy of the copy)

    // CSR long-row split (kernels_csr_split.hip): the long rows in chunks over the handle's own arrays, the others in `split_short`
    int32_t* split_chunks = nullptr;      // [3 * nchunks] row | first entry | end, per chunk of a long row
    int32_t  split_nchunks = 0;
    int32_t  split_threshold = 0;         // rows of this many entries and more are long (0: max(4096, longest / 16))
    int32_t  split_built_threshold = 0;   // what the split in memory was built with
    bool     split_auto_low = false;      // AUTO timed a threshold of 256 faster than the default on this handle (select.hip)
    int32_t  split_long_rows = 0;
    int64_t  split_long_nnz = 0;
    bool     sel_no_split = false;        // the handle is the short-row part of a split
    int32_t  split_mode = 0;              // how the long rows run: 1 chunks of the handle's own arrays, 2 virtual rows in a matrix of their own, 0 = by their density
    int32_t  split_built_mode = 0;         // the mode in effect (1 or 2)
    int32_t  split_built_for_mode = 0;     // the "split_mode" request the split in memory was built under
    spmv_mat* split_long = nullptr;       // mode 2: the virtual rows (a CSR handle with a kernel of its own); owned
    spmv_mat* split_short = nullptr;      // the copy without the long rows (a CSR handle with a kernel of its own); owned
    double*  split_yl = nullptr;          // mode 2: [split_vrows] the virtual rows' sums of one product
    int32_t* split_rows = nullptr;        // mode 2: [4 * long rows] row | first entry | virtual rows V | first virtual row
    int32_t  split_vrows = 0;

    // ELL whose slots are diagonals (kernels_ell.hip: ell_detect_diagonals): slot s holds column i + off[s] in the row
    // pairs whose bit is set; the product reads no column index there.  ell_diag = off[K] | xbase[K] | clusters
    // (kernels_ell.hip: stage_x_windows); mask[wavefront * K + s] = 64 row pairs
    int32_t* ell_diag      = nullptr;
    void*    ell_diag_mask = nullptr;
    int32_t  ell_diag_lds = 0;  // doubles of LDS the x stretches of a block take (0: none, x from global memory)
    int32_t  ell_variant  = 0;  // which of the format's own kernels runs (ell_settings.hpp: ell_variant_id; written by ell_use_variant and AUTO's trial)
    double*  ell_tval = nullptr;  // the values in tiles of 512 rows, (tile * k + slot) * 512 + row (ell_build_tiles); owned
    // ELL whose slots are diagonals, DIA-ORDER copy (kernels_ell.hip: ell_build_dia_order; ell_variant 3): the values once more
    // ROW-major, row * k + slot, multiplied by the DIA kernel (a workgroup streams one contiguous stretch and x goes through an
    // LDS window); rows in which any slot is not its diagonal are skipped there (ell_skip: a bit per row) and done by a side
    // kernel over the handle's own arrays (ell_nc_rows: their indices), in the same slot order: the same bits.  All owned.
    double*             ell_rval     = nullptr;
    unsigned long long* ell_skip     = nullptr;
    int32_t*            ell_nc_rows  = nullptr;
    int32_t             ell_nc_count = 0;
    int32_t             ell_off_min = 0, ell_off_max = 0;
    int32_t             ell_dia_order_req = -1;  // "ell_dia_order": -1 a candidate of the trial, 0 never, 1 built and used
    bool                ell_pad_marked = false;  // the ELL COPY of a CSR handle: padding slots carry a negative column and take no part in the sums (kernels_ell.hip: MASKED)

    // COO / CSC / ELL: the entries grouped by row, an internal CSR handle with a kernel of its own (rowgrouped.hip); owned
    spmv_mat* rowgrouped = nullptr;

    // COO: copy of the entries in column bins, one run of bins per XCD, for the segmented scan (kernels_coo.hip:
    // coo_build_bins); bins start on workgroup chunks, the padding carries row INT32_MAX
    int32_t* cb_row = nullptr;
    int32_t* cb_col = nullptr;
    double*  cb_val = nullptr;
    int32_t  cb_bins = 0;             // bins in all (a multiple of 8), 0: no copy
    int32_t  cb_region[8] = {0};      // first chunk of the XCD's bins
    int32_t  cb_chunks[8] = {0};      // chunks of the XCD's bins
    int64_t  cb_padded = 0;           // entries of the copy with its padding

    // a plan being applied (plan.hip): the node array and this handle's node in it; set only while spmv_mat_set_plan or the
    // analysis of a handle created under spmv_ctx_set_plan runs, handed down to the copies that are built meanwhile
    const spmv::plan_node* plan_base = nullptr;
    int32_t                plan_at   = -1;

    // symmetric Gauss-Seidel (symgs.hip): L / D / U copies, rows by level, launch schedule; built by symgs_setup
    struct spmv::symgs_plan* gs = nullptr;
    int32_t                  gs_order = 1;  // sweep order: 1 multicolour (default), 0 the matrix's own row order

    // ILU(0) (ilu0.hip): the factors L and U in sweep order, rows by level, launch schedules; built by ilu0_setup, no part of the
    // forward state (kernel, copies, plan) or of the transposed state
    struct spmv::ilu0_plan* ilu = nullptr;
    int32_t                 ilu_order = 1;  // "ilu0_order": 1 multicolour (default), 0 the matrix's own row order

    // triangular solves with the handle's own triangles (sptrsv.hip): a working copy, levels and schedules per (uplo, transpose) pair;
    // built by spmv_trsv_setup (or by the first solve), counted in device_bytes, no part of the forward state, of plans or of the
    // symgs, ILU(0) and transposed states
    struct spmv::trsv_state* trsv = nullptr;

    // the transposed product (transpose.hip): a companion handle of A^T over A's arrays, or the DIA transposed kernel's set-up;
    // built by spmv_mat_transpose_setup, no part of the forward state (kernel, copies, device_bytes, plan) - but for a BSR and a
    // format-6 handle, whose companions own their arrays and are counted in device_bytes
    struct spmv::transpose_state* tr            = nullptr;
    int32_t                       tr_kernel_req = SPMV_CSR_AUTO;  // "transpose_kernel": handed to spmv_mat_set_kernel on the companion

    // the Chebyshev polynomial preconditioner (chebyshev.hip): degree, bounds, coefficient table, 1 / a_ii and three work vectors; built
    // by spmv_chebyshev_setup (or by the first solve with SPMV_PRECOND_CHEBYSHEV), no part of the forward state, of plans or of trials
    struct spmv::cheby_state* cheby = nullptr;
    int32_t                   cheby_degree        = 4;   // "cheby_degree": what a solver's own set-up takes
    int32_t                   cheby_ratio         = 30;  // "cheby_ratio": lmin = lmax / ratio where lmin is estimated
    int32_t                   cheby_lanczos_steps = 0;   // "cheby_lanczos_steps": > 0: 1.05 ritz_max of that many steps competes with the row bound

    // aggregation AMG (amg.hip): aggregates, member lists, the coarse handles with their smoothers, the coarsest inverse and the levels'
    // vectors; built by spmv_amg_setup (or by the first solve with SPMV_PRECOND_AMG), no part of the forward state, of plans, of trials,
    // of copies or of the transposed state
    struct spmv::amg_state* amg              = nullptr;
    int32_t                 amg_level_kernel = 0;  // "amg_level_kernel": != 0 forces that CSR kernel id on every coarse handle of the next set-up

    // FSAI (fsai.hip): the factor G and G^T as CSR handles of their own and one work vector; built by spmv_fsai_setup (or by the first
    // solve with SPMV_PRECOND_FSAI), no part of the forward state, of plans, of trials, of copies, of device_bytes or of the transposed state
    struct spmv::fsai_state* fsai       = nullptr;
    int32_t                  fsai_level = 1;  // "fsai_level": the pattern of tril(A^level) that a solver's own set-up takes, 1 .. 3

    // a handle that spmv_spgemm made (spgemm.hip): what that product did ("spgemm_*"; 0 on every other handle)
    bool    spgemm_made = false;
    int64_t spgemm_products = 0, spgemm_rows_lds = 0, spgemm_rows_sorted = 0, spgemm_transient_bytes = 0;

    // single-precision value storage (SPMV_FMT_CSR_F32; kernels_csr_f32.hip, convert_f32.hip): `a` is the row pointer, b and v hold
    // nothing; the entries are ONE stream of packed words (csr_f32_settings.hpp: column | float bits << 32), owned, counted in
    // device_bytes.  What spmv_csr_to_f32's rounding did (zero on an uploaded handle): spmv_f32_info
    uint64_t* f32_ent       = nullptr;  // [max(nnz, 1)]
    int64_t   f32_inexact   = 0;        // values that changed
    int64_t   f32_underflow = 0;        // nonzero values that became zero or subnormal
    double    f32_max_rel   = 0.0;      // the largest relative change among the changed values that did not underflow
};

namespace spmv
{
// a launch holds fewer than 2^32 work-items: beyond that the grid wraps around without an error
inline bool launch_fits(int64_t items, int lanes_per_item) { return items * lanes_per_item < ((int64_t)1 << 32) - 4096; }
// a COO, CSC or ELL handle whose product runs from its row-grouped copy (reported as kernel PANEL)
inline bool runs_from_rowgrouped(const spmv_mat* m) { return m->format != SPMV_FMT_CSR && m->rowgrouped && m->kernel == SPMV_CSR_PANEL; }
// a CSR kernel that reads row_ptr and a layout of its own only, not col_ind / values (the panel and two-phase layouts, the ELL copy)
inline bool kernel_reads_own_layout(int32_t kernel) { return kernel == SPMV_CSR_PANEL || kernel == SPMV_CSR_TWOPHASE || kernel == SPMV_CSR_ELL; }
int ensure_scratch(spmv_ctx* ctx, size_t bytes);

// kernels_csr.hip
int csr_analyse(spmv_mat* m);
// the layouts of their own that five of the CSR kernels multiply from (panel, two-phase, segmented scan, long-row split, ELL copy)
int  csr_layout_build(spmv_mat* m, int32_t kernel);       // (re)builds `kernel`'s with the current parameters; VECTOR, LDSWIN, SCALAR: nothing
void csr_layouts_free(spmv_mat* m, uint32_t kernels);     // frees those of the kernels whose bit 1u << id is set
bool csr_layout_built(const spmv_mat* m, int32_t kernel);  // kernel_reads_own_layout(kernel) and that layout is in memory
constexpr uint32_t kCsrAllLayouts = ~0u;
void csr_choose_kernel(spmv_mat* m);  // the model's pick (no launches)
int  csr_ldswin_capacity();           // columns of x the LDS-window kernel's tile holds
bool csr_ldswin_fits(const spmv_mat* m);  // the widest block window of an analysed handle is known and the tile holds it: LDSWIN can launch
// select.hip: AUTO by measurement
bool select_trials_enabled(const spmv_mat* m);
// ms per launch of n launches between the context's two events (ev_begin / ev_end); a launch that fails ends it with that code
int  time_launches(spmv_ctx* ctx, int n, const std::function<int()>& launch, float* ms_per_launch);
int  csr_select_kernel(spmv_mat* m);
// zeroed x (ncol) and y (nrow) for timing launches; freed with the object
struct select_scratch
{
    double *x = nullptr, *y = nullptr;
    spmv_ctx* ctx        = nullptr;
    bool      from_arena = false;  // x / y lie in the context's trial arena (select.hip), not in allocations of their own
    int  alloc(spmv_ctx* ctx, int64_t ncol, int64_t nrow);
    void release();
    ~select_scratch() { release(); }
};
// candidates 0 .. n-1 timed in rounds until no minimum moves (select.hip); t[i] < 0: not timed yet
int  select_rounds(spmv_ctx* ctx, int n, const std::function<int(int)>& launch, float* t, int* rounds_run);
// ms per product of `launch`: 1 warm-up + 1 product, and 2 x 4 more (the minimum) unless that one was 3x behind best_so_far
int  select_time(spmv_ctx* ctx, const std::function<int()>& launch, float best_so_far, float* ms);
// The slots of spmv_mat::sel_us, microseconds per product of a candidate a trial timed ("select_us_<name>").  A CSR kernel's slot
// is its id, 1 (SPMV_CSR_VECTOR) .. 8 (SPMV_CSR_ELL); on a COO, CSC or ELL handle 1 is the format's own kernel and 4
// (SPMV_CSR_PANEL) the row-grouped copy.  The others:
enum select_slot : int
{
    kSelSplitLow = 0,  // "split_low": CSR, kernel SPLIT with rows of 256 entries and more split off (timed from 8M entries on)
    kSelVariant1 = 6,  // "variant1": ELL one row per lane; COO the scan over column bins (a CSR handle's "segscan")
    kSelVariant2 = 7,  // "variant2": ELL two rows per lane reading every column (a CSR handle's "split")
    kSelDiaOrder = 9,  // "dia_order": ELL, the DIA-order copy of the values
    kSelSlots    = 10
};
static_assert(sizeof(spmv_mat::sel_us) / sizeof(float) == kSelSlots, "sel_us holds one figure per slot");
bool select_get_param(const spmv_mat* m, const char* name, int64_t* value);  // "select_*" through the one table from name to slot; false: not one of them
void select_note(spmv_mat* m, int slot, float ms);  // records a timed candidate (sel_us[slot], sel_candidates)
void select_reset(spmv_mat* m);
constexpr int64_t kSelectMinNnz = (int64_t)64 << 10;  // below: every kernel takes a launch latency, nothing to choose
constexpr int64_t kSelectMaxNnz = (int64_t)8 << 20;   // CSR above: the model's pick unless a statistic casts doubt on it
// kernels_csr_panel.hip
int  csr_panel_build(spmv_mat* m);
int  panel_choose_pace(spmv_mat* m);
void csr_panel_free(spmv_mat* m);
int  csr_panel_apply(spmv_ctx* ctx, const spmv_mat* A, const double* x, double* y);
// kernels_csr_twophase.hip
int  csr_twophase_build(spmv_mat* m);
void csr_twophase_free(spmv_mat* m);
bool csr_twophase_worth(const spmv_mat* m);
int  csr_twophase_choose_again(spmv_mat* m);
int  csr_twophase_offer_csr_copy(spmv_mat* m, bool* keep_b, bool* keep_v);
int  csr_twophase_pool_alloc(spmv_mat* m, int extra);
int  csr_twophase_pool_config(spmv_mat* m, int64_t code);


// A sum that thousands of wavefronts add into is kept as kDotSlots partial sums on different 128-byte lines (an
// atomic on ONE word costs ~12 ns each at the L2, serialised: 8192 of them are 100 us); readers add the slots up.
constexpr int kDotSlots   = 32;
constexpr int kDotStride  = 16;                       // doubles between slots: one 128-byte line each
constexpr int kDotDoubles = kDotSlots * kDotStride;   // size of one slotted accumulator

// what a solver step wants on top of y += A*x (solver.hip)
struct apply_extra
{
    bool          overwrite = false;    // y = A*x instead of y += A*x
    const double* dot_w     = nullptr;  // if set: accumulate sum_i dot_w[i] * y_new[i] into dot_out
    double*       dot_out   = nullptr;  // slotted accumulator on the device (kDotDoubles doubles)
};
int  csr_panel_apply_ex(spmv_ctx* ctx, const spmv_mat* A, const double* x, double* y, const apply_extra& ex);
int  csr_twophase_apply_ex(spmv_ctx* ctx, const spmv_mat* A, const double* x, double* y, const apply_extra& ex);
// kernels_csr.hip: the product dispatch.  mat_apply_ex is the one function that decides which kernel a forward product of a
// handle (any format) runs; csr_apply is its CSR half (the trials time candidates through it)
int  mat_apply_ex(spmv_ctx* ctx, const spmv_mat* A, const double* x, double* y, const apply_extra& ex = apply_extra{});
int  csr_apply(spmv_ctx* ctx, const spmv_mat* A, const double* x, double* y, const apply_extra& ex = apply_extra{});
bool writes_row_sums_in_one_launch(const spmv_mat* A);  // the product can store sum_i instead of y_i + sum_i at no extra launch
bool adds_into_y_with_atomics(const spmv_mat* A);       // global_atomic_add_f64 on y, by the kernel (of the handle or its copies) that runs
// The solves' drivers.  Each is entered from its ABI entry (abi.hip) behind the argument checks and use_device, zeroes its
// outputs, returns at an empty system, and shares its host side - the workspace that owns its device memory, the preconditioner's
// set-up and application, the looks at its scalars - with the others through solver_host.hpp.
// Which driver takes which preconditioner is written down once, beside the preconditioners' table (precond.hip: kPreconds, k*Rules).
// solver.hip: conjugate gradients for a symmetric positive definite A
int cg_solve(spmv_ctx* ctx, const spmv_mat* A, const double* b, double* x, int max_iter, double rel_tol, int check_every,
             int precond, int* iters, double* rel_resid);
int vec_dot_accumulate(spmv_ctx* ctx, const double* x, const double* y, int64_t n, double* device_out);
// solver_multi.hip: k independent solves A x_c = b_c in one loop, B and X row-major (n x k); iters and rel_resid: host arrays of k
int cg_multi_solve(spmv_ctx* ctx, const spmv_mat* A, int32_t k, const double* B, double* X, int max_iter, double rel_tol,
                   int check_every, int precond, int32_t* iters, double* rel_resid);
// solver_cgls.hip: CGLS for min ||b - A x||^2 + damp^2 ||x||^2 over the forward and the transposed product of any handle
int cgls_solve(spmv_ctx* ctx, const spmv_mat* A, const double* b, double* x, int max_iter, double rel_tol, int check_every,
               double damp, int* iters, double* rel_normal_resid, double* rel_resid);
// solver_bicgstab.hip: right-preconditioned BiCGSTAB for square A over two forward products of any handle
int bicgstab_solve(spmv_ctx* ctx, const spmv_mat* A, const double* b, double* x, int max_iter, double rel_tol, int check_every,
                   int precond, int* iters, double* rel_resid);
// solver_gmres.hip: right-preconditioned restarted GMRES(restart) for square A over one forward product of any handle per iteration
// (restart: 1 .. 64)
int gmres_solve(spmv_ctx* ctx, const spmv_mat* A, const double* b, double* x, int restart, int max_iter, double rel_tol, int check_every,
                int precond, int* iters, double* rel_resid);
// solver_minres.hip: preconditioned MINRES for (A - shift I) x = b, A square and symmetric, over one forward product of any handle per
// iteration; the preconditioner is P's (null: A's)
int minres_solve(spmv_ctx* ctx, const spmv_mat* A, const spmv_mat* P, const double* b, double* x, double shift, int max_iter, double rel_tol,
                 int check_every, int precond, int* iters, double* rel_resid);
// solver_lobpcg.hip: LOBPCG for the k smallest (largest) eigenpairs of a symmetric A over one forward product per active column and
// iteration (k: 1 .. 16); X: n x k, column-major, ld = n
int lobpcg_solve(spmv_ctx* ctx, const spmv_mat* A, int k, int nev, bool largest, double* X, int max_iter, double tol, int precond, double* theta,
                 double* resid, int* iters);
// block_ops.hip: G = U^T V and Out = S C for column-major blocks of up to kBlockMaxCols columns (the layout and the contracts: there)
constexpr int kBlockMaxCols = 96;
int    block_gram_check(const spmv_ctx* ctx, int64_t n, int p, const spmv_vec* U, int64_t ldu, int q, const spmv_vec* V, int64_t ldv, const double* G_host);
int    block_combine_check(const spmv_ctx* ctx, int64_t n, int p, const spmv_vec* S, int64_t lds, int q, const double* C_host, const spmv_vec* Out, int64_t ldo);
int    block_gram(spmv_ctx* ctx, int64_t n, int p, const double* U, int64_t ldu, int q, const double* V, int64_t ldv, double* G_host);      // synchronous
int    block_combine(spmv_ctx* ctx, int64_t n, int p, const double* S, int64_t lds, int q, const double* C_host, double* Out, int64_t ldo);  // asynchronous
size_t block_gram_part_doubles(int64_t n, int p, int q);  // the partial sums a launch on n rows stores
size_t block_gram_part_bound(int cols);                   // at least that for every n and every p, q <= cols
// the launches by themselves, on device memory of the caller's: G (p q doubles), part (block_gram_part_doubles), a ticket that is 0
// and is left 0; C (p q doubles) on the device.  Out may be any block whose row i lies in S's row i (the same ld, a whole number of
// columns apart), or lie apart from S
int  block_gram_launch(spmv_ctx* ctx, int64_t n, int p, const double* U, int64_t ldu, int q, const double* V, int64_t ldv, double* G, double* part,
                       uint32_t* ticket);
int  block_combine_launch(spmv_ctx* ctx, int64_t n, int p, const double* S, int64_t lds, int q, const double* C, double* Out, int64_t ldo);
void block_ops_free(spmv_ctx* ctx);
// kernels_ell.hip (what a product launches: ell_settings.hpp)
int ell_apply(spmv_ctx* ctx, const spmv_mat* A, const double* x, double* y);
int ell_analyse(spmv_mat* m);
int  ell_use_variant(spmv_mat* m, int variant, bool keep_requested_copy);  // switches the format's own kernel; builds / drops the DIA-order copy
int  ell_use_tiles(spmv_mat* m, bool on);  // builds / drops the copy of the values in tiles of 512 rows
int  ell_build_dia_order(spmv_mat* m, bool only_if_worth);  // the DIA-order copy of the values (ell_variant 3)
void ell_free_dia_order(spmv_mat* m);
void ell_layouts_free(spmv_mat* m);  // slot descriptors, mask, tiles, DIA-order copy
bool ell_set_param(spmv_mat* m, const char* name, int64_t value, int* rc);  // "ell_*"; false: not one of them
bool ell_get_param(const spmv_mat* m, const char* name, int64_t* value);    // "ell_*", "ell_copy_*"; false: not one of them
int ell_select_kernel(spmv_mat* m);                    // AUTO: the format's own variants and (where a candidate) the row-grouped copy, timed
int ell_rowgrouped_copy(spmv_mat* m, int32_t force_kernel, spmv_mat** out);  // the row-grouped copy's CSR handle (rowgrouped_build)
int  csr_ell_copy_build(spmv_mat* m);  // SPMV_CSR_ELL: the ELL copy of a CSR handle with (nearly) equal rows
void csr_ell_copy_free(spmv_mat* m);
bool csr_ell_copy_worth(const spmv_mat* m);
// kernels_coo.hip
int coo_analyse(spmv_mat* m);
int coo_select_kernel(spmv_mat* m);                    // AUTO: the segmented scan or the row-grouped copy (which picks its own kernel), timed
int  coo_build_bins(spmv_mat* m, int bins_per_xcd, bool only_if_worth);  // bins_per_xcd 0: as many as keep a slice of x inside an XCD's L2
void coo_free_bins(spmv_mat* m);
int coo_apply(spmv_ctx* ctx, const spmv_mat* A, const double* x, double* y);
int  csr_segscan_build(spmv_mat* m);  // SPMV_CSR_SEGSCAN: the row index per entry the scan runs over
void csr_segscan_free(spmv_mat* m);
int  csr_segscan_apply(spmv_ctx* ctx, const spmv_mat* A, const double* x, double* y);
// kernels_csr_split.hip
int  csr_split_build(spmv_mat* m);
void csr_split_free(spmv_mat* m);
int  csr_split_threshold(const spmv_mat* m);
int  csr_split_long_rows_apply(spmv_ctx* ctx, const spmv_mat* A, const double* x, double* y);
// kernels_spmm.hip: Y += A*X (Y = A*X) for k row-major vectors, CSR and ELL handles, over the handle's own arrays
int spmm_apply(spmv_ctx* ctx, const spmv_mat* A, int32_t k, const double* X, double* Y, bool overwrite);
// kernels_sddmm.hip: out = alpha * (U V^T sampled on A's CSR pattern) + beta * out; U nrow x k, V ncol x k row-major, out nnz entries
int sddmm_apply(spmv_ctx* ctx, const spmv_mat* A, int32_t k, double alpha, const double* U, const double* V, double beta, double* out);
// kernels_misc.hip (CSC, DIA, BLAS-1, fill)
int csc_apply(spmv_ctx* ctx, const spmv_mat* A, const double* x, double* y);
int csc_analyse(spmv_mat* m);
int csc_select_kernel(spmv_mat* m);                       // AUTO: the scatter or the row-grouped copy (which picks its own kernel), timed
int csc_rowgrouped_copy(spmv_mat* m, int32_t force_kernel, spmv_mat** out);  // the row-grouped copy's CSR handle (rowgrouped_build)
int dia_apply(spmv_ctx* ctx, const spmv_mat* A, const double* x, double* y);
int dia_rows_apply(spmv_ctx* ctx, int nrow, int jmax, int k, const int32_t* offsets, const double* values, const double* x, double* y, bool off_known,
                   int off_min, int off_max, uint32_t flags, const unsigned long long* skip_rows, int stride);
int vec_fill(spmv_ctx* ctx, double* d, int64_t n, double a);
int vec_copy2(spmv_ctx* ctx, double* dst0, const double* src0, int64_t n0, double* dst1, const double* src1, int64_t n1);  // two copies, one launch
int vec_dot(spmv_ctx* ctx, const double* x, const double* y, int64_t n, double* result);
int vec_axpby(spmv_ctx* ctx, double alpha, const double* x, double beta, const double* y, double* w,
              int64_t n);
// kernels_bsr.hip: block CSR (what a product launches: bsr_settings.hpp); nnz counts stored values, nnz / bs^2 blocks
int bsr_apply(spmv_ctx* ctx, const spmv_mat* A, const double* x, double* y);
int bsr_analyse(spmv_mat* m);
int bsr_set_kernel(spmv_mat* m, int32_t kernel, int32_t lanes);  // spmv_mat_set_kernel on a BSR handle
int bsr_apply_plan(spmv_mat* m);
// convert_bsr.hip: the conversions and the handle of A^T (each check on the host, before the device is touched)
int bsr_check_bs(int32_t bs, const char* who);
int csr_to_bsr_check(const spmv_ctx* ctx, const spmv_mat* csr, int32_t bs, const char* who);
int bsr_to_csr_check(const spmv_ctx* ctx, const spmv_mat* bsr, const char* who);
int csr_to_bsr(spmv_ctx* ctx, const spmv_mat* csr, int32_t bs, spmv_mat** out);             // synchronous; analysed by the caller
int bsr_to_csr(spmv_ctx* ctx, const spmv_mat* bsr, int32_t drop_zeros, spmv_mat** out);    // synchronous; analysed by the caller
int bsr_transpose(spmv_ctx* ctx, const spmv_mat* A, spmv_mat** out);                       // synchronous; analysed
// kernels_csr_f32.hip: CSR with single-precision value storage (what a product launches: csr_f32_settings.hpp)
int csr_f32_apply(spmv_ctx* ctx, const spmv_mat* A, const double* x, double* y, const apply_extra& ex = apply_extra{});
int csr_f32_analyse(spmv_mat* m);
int csr_f32_set_kernel(spmv_mat* m, int32_t kernel, int32_t lanes);  // spmv_mat_set_kernel on a format-6 handle
int csr_pick_lanes(double mean_row);                                 // kernels_csr.hip: the row-parallel kernels' lanes per row from the mean row length
// convert_f32.hip: the conversions and the handle of A^T (each check on the host, before the device is touched)
int csr_to_f32_check(const spmv_ctx* ctx, const spmv_mat* csr, const char* who);
int f32_to_csr_check(const spmv_ctx* ctx, const spmv_mat* f32, const char* who);
int csr_to_f32(spmv_ctx* ctx, const spmv_mat* csr, const char* who, spmv_mat** out);  // synchronous; analysed by the caller
int csr_f32_from_host(spmv_ctx* ctx, int32_t nrow, int32_t ncol, int64_t nnz, const int32_t* row_ptr, const int32_t* col, const float* val,
                      spmv_mat** out);                                                 // synchronous; analysed by the caller
int f32_to_csr(spmv_ctx* ctx, const spmv_mat* f32, const char* who, spmv_mat** out);  // synchronous; analysed by the caller
int f32_widen_arrays(spmv_ctx* ctx, const spmv_mat* f32, int32_t* d_col, double* d_val);  // asynchronous; either array may be null
int f32_transpose(spmv_ctx* ctx, const spmv_mat* A, spmv_mat** out);                  // synchronous; analysed
// solver_refine.hip: iterative refinement, the residual with A in fp64, the correction from a solver on A_lo
int refine_solve(spmv_ctx* ctx, const spmv_mat* A, const spmv_mat* A_lo, const double* b, double* x, int solver, int precond, int max_outer,
                 int inner_max_iter, double inner_tol, double rel_tol, int* outer, int* inner_total, double* rel_resid);
// validate.hip
int mat_validate(const spmv_mat* m);
// convert.hip
int exclusive_scan_i32(spmv_ctx* ctx, const int32_t* in, int32_t* out, int64_t n);
constexpr int32_t kCsrAutoNoSegscan = -1;  // coo_to_csr's force_kernel: AUTO among the kernels a COO handle does not have itself
int coo_to_csr(spmv_ctx* ctx, const spmv_mat* coo, spmv_mat** out, int32_t force_kernel = 0 /* SPMV_CSR_AUTO: select */);
// The preconditioners.  Their host side is reached through one table, a row per SPMV_PRECOND_* id (precond.hpp); the pieces their
// handle checks are built from are precond.hip's (`noun`: the unit's name in the message):
int  check_whole_square(const spmv_mat* m, const char* who, const char* noun);      // INVALID: not square, or a shard that starts behind row 0
int  check_csr_arrays(const spmv_mat* m, const char* who, const char* what_for);    // INVALID: arrays released; what_for: "" or ": no ... for ..."
int  check_whole_square_csr(const spmv_mat* m, const char* who, const char* noun);  // UNSUPPORTED: not CSR; then the two above
// symgs.hip
int  symgs_setup(spmv_mat* m);
void symgs_free(spmv_mat* m);
int  symgs_sweep(spmv_ctx* ctx, const spmv_mat* A, const double* b, double* x, bool zero_guess);
bool symgs_get_param(const spmv_mat* m, const char* name, int64_t* value);      // "symgs_*"; false: not one of them
bool symgs_set_param(spmv_mat* m, const char* name, int64_t value, int* rc);  // "symgs_order"; false: not that
int  symgs_sequence(const spmv_mat* m, int32_t* out);
// ilu0.hip: ILU(0) of a CSR handle in sweep order and its application z = U^-1 L^-1 r (SPMV_PRECOND_ILU0)
int  ilu0_check_handle(const spmv_mat* m, const char* who);  // on the host: UNSUPPORTED (not CSR) / INVALID (a shard, not square, arrays released)
int  ilu0_setup(spmv_mat* m);                                 // order, symbolic and numeric set-up (synchronous; once per handle and order)
void ilu0_free(spmv_mat* m);
int  ilu0_apply(spmv_ctx* ctx, const spmv_mat* A, const double* r, double* z);  // asynchronous; r and z must not overlap
int  ilu0_factor_values(const spmv_mat* m, double* out);      // aligned to the handle's own entries, to the host
int  ilu0_sequence(const spmv_mat* m, int32_t* out);
bool ilu0_get_param(const spmv_mat* m, const char* name, int64_t* value);      // "ilu0_*"; false: not one of them
bool ilu0_set_param(spmv_mat* m, const char* name, int64_t value, int* rc);  // "ilu0_order"; false: not that
// sptrsv.hip: x = op(T)^-1 b with the strictly lower / upper part of a CSR handle plus the diagonal (flags: SPMV_TRSV_*)
int  trsv_check_flags(uint32_t flags, const char* who);      // on the host: INVALID (unknown bits)
int  trsv_check_handle(const spmv_mat* m, const char* who);  // on the host: UNSUPPORTED (not CSR) / INVALID (a shard, not square, arrays released)
int  trsv_setup(spmv_mat* m, uint32_t flags);                // the working copy and its analysis (synchronous; once per handle, uplo and transpose)
void trsv_free(spmv_mat* m);
int  trsv_apply(spmv_ctx* ctx, const spmv_mat* A, uint32_t flags, const double* b, double* x);  // asynchronous; b may be x
int  trsv_apply_multi(spmv_ctx* ctx, const spmv_mat* A, uint32_t flags, int32_t k, const double* B, double* X);  // row-major n x k; B may be X
int  trsv_info(const spmv_mat* m, uint32_t flags, int32_t* levels, int32_t* lanes, int32_t* launches, int64_t* bytes);
bool trsv_get_param(const spmv_mat* m, const char* name, int64_t* value);  // "trsv_*"; false: not one of them
// chebyshev.hip: the Chebyshev polynomial preconditioner z = p_d(diag(s) A) diag(s) r (SPMV_PRECOND_CHEBYSHEV), and the Lanczos estimate
int  cheby_coefficients(int degree, double lmin, double lmax, double* c0, double* c1, double* c2);  // host only; c1, c2: degree entries
int  cheby_check_handle(const spmv_mat* m, const char* who);  // on the host: INVALID (not square, a shard that starts behind row 0)
int  cheby_check_scaled(const spmv_mat* m, const char* who);  // on the host: INVALID (the Jacobi scaling: not CSR, arrays released)
int  cheby_check_setup(const spmv_mat* m, int degree, int scaled, double lmin, double lmax, const char* who);  // on the host
int  cheby_setup(spmv_ctx* ctx, spmv_mat* m, int degree, int scaled, double lmin, double lmax);  // synchronous; replaces earlier state
void cheby_free(spmv_mat* m);
int  cheby_info(const spmv_mat* m, int32_t* degree, int32_t* scaled, double* lmin, double* lmax);
int  cheby_apply(spmv_ctx* ctx, const spmv_mat* A, const double* r, double* z);   // z = M^-1 r, asynchronous; r and z must not overlap
int  cheby_smooth(spmv_ctx* ctx, const spmv_mat* A, const double* b, double* x);  // x += M^-1 (b - A x), asynchronous
int  cheby_lanczos(spmv_ctx* ctx, const spmv_mat* A, int scaled, int steps, uint64_t seed, double* ritz_min, double* ritz_max, double* alpha,
                   double* beta, int32_t* steps_done);  // synchronous; alpha, beta: host arrays of `steps` entries or null
int  cheby_row_bound(spmv_ctx* ctx, const spmv_mat* m, const double* s, double* bound);  // max_i |s_i| sum_j |a_ij| of a CSR handle's arrays (s null: 1); synchronous
bool cheby_get_param(const spmv_mat* m, const char* name, int64_t* value);      // "cheby_*"; false: not one of them
bool cheby_set_param(spmv_mat* m, const char* name, int64_t value, int* rc);  // "cheby_*"; false: not one of them
// amg.hip: aggregation AMG, one V(1,1) cycle z = B r (SPMV_PRECOND_AMG)
int  amg_check_handle(const spmv_mat* m, const char* who);  // on the host: UNSUPPORTED (not CSR) / INVALID (a shard, not square, arrays released)
int  amg_check_setup(const spmv_mat* m, int max_levels, int coarse_max, int smooth_degree, double strength, double overcorrection, const char* who);
int  amg_setup(spmv_ctx* ctx, spmv_mat* m, int max_levels, int coarse_max, int smooth_degree, double strength, double overcorrection);  // synchronous; 0: the default
// smoothed aggregation: the prolongators P = (I - g D^-1 A^F) T and R = P^T as CSR handles of every level, A_c = R A P by spgemm
int  amg_check_setup_smoothed(const spmv_mat* m, int max_levels, int coarse_max, int smooth_degree, double strength, double overcorrection,
                              double prolong_damping, const char* who);
int  amg_setup_smoothed(spmv_ctx* ctx, spmv_mat* m, int max_levels, int coarse_max, int smooth_degree, double strength, double overcorrection,
                        double prolong_damping);  // synchronous; 0: the default
int  amg_check_transfer(const spmv_mat* m, int level, int what, int lanes, int64_t v_entries, const char* who);  // on the host
int  amg_transfer_launch(spmv_ctx* ctx, const spmv_mat* m, int level, int what, int lanes, double* v, double* t);  // one restriction / prolongation by itself; asynchronous
int  amg_prolongator_download(spmv_ctx* ctx, const spmv_mat* m, int level, int64_t* nnz, int32_t* row_ptr, int32_t* col, double* val);
void amg_free(spmv_mat* m);
int  amg_info(const spmv_mat* m, int32_t* levels, int64_t* rows, int64_t* nnz);
int  amg_level_download(spmv_ctx* ctx, const spmv_mat* m, int level, int32_t* agg_host, int32_t* row_ptr, int32_t* col, double* val);
int  amg_apply(spmv_ctx* ctx, const spmv_mat* A, const double* r, double* z);  // z = B r, asynchronous; r and z must not overlap
bool amg_get_param(const spmv_mat* m, const char* name, int64_t* value);      // "amg_*"; false: not one of them
bool amg_set_param(spmv_mat* m, const char* name, int64_t value, int* rc);  // "amg_level_kernel"; false: not that
// fsai.hip: the factorised sparse approximate inverse G A G^T ~ I of an SPD CSR handle, z = G^T (G r) (SPMV_PRECOND_FSAI)
int  fsai_check_handle(const spmv_mat* m, const char* who);  // on the host: UNSUPPORTED (not CSR) / INVALID (a shard, not square, arrays released)
int  fsai_check_level(int32_t level, const char* who);       // on the host: 0 .. 3
int  fsai_setup(spmv_ctx* ctx, spmv_mat* m, int32_t level);  // synchronous; 0: the handle's "fsai_level"; replaces earlier state
void fsai_free(spmv_mat* m);
int  fsai_apply(spmv_ctx* ctx, const spmv_mat* A, const double* r, double* z);  // asynchronous; r and z must not overlap
int  fsai_info(const spmv_mat* m, int32_t* level, int64_t* nnz, int32_t* max_row);
int  fsai_factor_download(spmv_ctx* ctx, const spmv_mat* m, int64_t* nnz, int32_t* row_ptr, int32_t* col, double* val);
bool fsai_get_param(const spmv_mat* m, const char* name, int64_t* value);      // "fsai_*"; false: not one of them
bool fsai_set_param(spmv_mat* m, const char* name, int64_t value, int* rc);  // "fsai_level"; false: not that
// spgemm.hip: C = A B and A^T as CSR handles of their own
int  spgemm_check(const spmv_ctx* ctx, const spmv_mat* A, const spmv_mat* B, int32_t method, const char* who);  // on the host: every refusal made before the device is touched
int  csr_transpose_check(const spmv_ctx* ctx, const spmv_mat* A, const char* who);                              // likewise
// (force_kernel != 0: the product's handle runs that CSR kernel id instead of selecting one, for a caller that builds it for itself)
int  spgemm(spmv_ctx* ctx, const spmv_mat* A, const spmv_mat* B, int32_t method, spmv_mat** out, int32_t force_kernel = 0);  // synchronous
int  csr_transpose(spmv_ctx* ctx, const spmv_mat* A, spmv_mat** out, int32_t force_kernel = 0);                              // synchronous
bool spgemm_get_param(const spmv_mat* m, const char* name, int64_t* value);  // "spgemm_*"; false: not one of them
// convert_sort.hip
int sort_ids_by_key(spmv_ctx* ctx, const int32_t* keys, int64_t n, int bits, int32_t* out_ids);
int coo_place_by_stable_sort(spmv_ctx* ctx, int64_t nnz, int32_t nrow, const int32_t* row, const int32_t* col, const double* val,
                             int32_t* out_col, double* out_val);
int csr_to_ell(spmv_ctx* ctx, const spmv_mat* csr, spmv_mat** out, bool pad_own_column = false);
int csr_split_columns(spmv_ctx* ctx, const spmv_mat* csr, int32_t c0, int32_t c1, spmv_mat** out_in, spmv_mat** out_out);
int csr_extract_rows(spmv_ctx* dst, const spmv_mat* csr, int64_t r0, int64_t r1, spmv_mat** out);
int coo_row_offsets(const spmv_mat* coo, int64_t* row_ptr64 /* host, nrow + 1 */);
int reduce_max_i32(spmv_ctx* ctx, const int32_t* in, int64_t n, int32_t* result);
// generate.hip
int gen_csr_uniform(spmv_ctx* ctx, int64_t row_begin, int64_t row_end, int32_t ncol, int32_t k,
                    int32_t band, uint64_t seed, spmv_mat** out);
int gen_ell_banded(spmv_ctx* ctx, int32_t nrow, int32_t ncol, int32_t k, uint64_t seed,
                   spmv_mat** out);
int gen_dia_banded(spmv_ctx* ctx, int32_t nrow, int32_t k, uint64_t seed, spmv_mat** out);
int gen_coo_powerlaw(spmv_ctx* ctx, int32_t nrow, int32_t ncol, int32_t max_len, uint64_t seed, bool sorted_by_length,
                     spmv_mat** out);
int gen_vec_uniform(spmv_ctx* ctx, double* d, int64_t n, int64_t index_offset, uint64_t seed);

// plan.hip
inline const plan_node* plan_of(const spmv_mat* m) { return m->plan_base && m->plan_at >= 0 ? m->plan_base + m->plan_at : nullptr; }
enum plan_child { kPlanChildRowgrouped, kPlanChildLong, kPlanChildEll };
inline void plan_hand_down(const spmv_mat* parent, spmv_mat* child, plan_child which)
{
    const plan_node* p = plan_of(parent);
    if (!p) return;
    const int32_t at = which == kPlanChildRowgrouped ? p->child_rowgrouped : (which == kPlanChildLong ? p->child_long : p->child_ell);
    child->plan_base = at >= 0 ? parent->plan_base : nullptr;
    child->plan_at   = at;
}
// a handle under analysis applies its plan: the node handed down to it, else the context's armed plan (if its format is the
// plan's).  true: the plan decided, *rc says how; false: no plan, or a context's plan that does not fit this matrix (the handle selects)
bool plan_analyse(spmv_mat* m, int* rc);
void plan_clear(spmv_mat* m);
int  csr_apply_plan(spmv_mat* m);    // select.hip
void plan_reset_requests(spmv_mat* m);  // the parameters a plan sets explicitly, back to "choose" (a plan that did not fit)
int  ell_apply_plan(spmv_mat* m);    // kernels_ell.hip
int  coo_apply_plan(spmv_mat* m);    // kernels_coo.hip
int  csc_apply_plan(spmv_mat* m);    // kernels_misc.hip
// rowgrouped.hip: the row-grouped copy of a COO, CSC or ELL handle
void rowgrouped_drop(spmv_mat* m);
void release_unread_csr_arrays(spmv_mat* csr);  // a CSR handle whose kernel reads only its own layout gives col_ind / values back
int  rowgrouped_build(spmv_mat* m, int32_t force_kernel);  // reuse, size limit, drop, produce, release, adopt
int  rowgrouped_select(spmv_mat* m, int (*trial)(spmv_mat* m, const select_scratch& sv, bool model_copy, float* t_copy, float* t_own));  // COO, CSC AUTO
int  rowgrouped_set_kernel(spmv_mat* m, int32_t kernel);  // spmv_mat_set_kernel on a COO, CSC or ELL handle
// transpose.hip: the transposed product's state
int  transpose_setup(spmv_mat* A);                                       // builds it once (synchronous); no part of the forward state
int  transpose_apply(spmv_ctx* ctx, const spmv_mat* A, const double* x, double* y);  // y += A^T x; the state must be set up
void transpose_free(spmv_mat* A);                                        // drops it (A's arrays are only borrowed)
int  transpose_set_kernel(spmv_mat* A, int64_t kernel);                  // "transpose_kernel"
bool transpose_get_param(const spmv_mat* A, const char* name, int64_t* value);  // "transpose_*"; false: not one of them
// abi.hip helpers used by the other units
int  mat_alloc(spmv_ctx* ctx, int32_t format, int32_t nrow, int32_t ncol, int64_t nnz, int32_t k,
               size_t a_count, size_t b_count, size_t v_count, spmv_mat** out);
void mat_free(spmv_mat* m);
}  // namespace spmv
