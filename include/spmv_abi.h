/*
 * spmv_abi.h — the drop-in boundary of the MI355X SpMV engine (libspmv_hip.so).
 *
 * Plain C ABI: opaque handles, raw pointers, sizes.  No C++ types, no torch types.  Everything
 * the reference's hot path does (`y += A*x` for its storage formats, the format conversions, the
 * BLAS-1 helpers and the row-range sharding of its NUMA drivers) is reachable from here; the
 * C++ classes of the reference (include/matrix.h, include/vector.h, include/mat_vec.h in the
 * reference tree) are re-created as a thin source-compatible shim over this ABI in
 * include/arm_spmv_compat.hpp, so the reference's main.cpp recompiles unchanged.
 *
 * Conventions
 *   - every function returns 0 on success, a negative spmv_status otherwise; the message of the
 *     last failure on the calling thread is spmv_last_error().  (The reference has no error
 *     convention: ops return void, I/O failures printf + exit(1), src/data_io.cpp:53-75.)
 *   - values are fp64, indices int32 (as in the reference, include/matrix.h:9-16); counts that can
 *     exceed 2^31 across shards (nnz) are int64 in this ABI.
 *   - semantics are ACCUMULATING: spmv_apply computes y += A*x (src/mat_vec.cpp:39,64,91,116,142);
 *     the caller zeroes y (main.cpp:55,65,85).
 *   - host arrays passed to *_upload stay owned by the caller and may be freed on return; device
 *     pointers passed to *_wrap_device are borrowed and must outlive the handle.
 *   - work is queued on the context's HIP stream and is asynchronous; spmv_sync() waits.
 *   - threading: like the reference's entry points (synchronous, one caller), a context and the
 *     handles made from it are driven by ONE host thread at a time; different contexts (e.g. one
 *     per GPU) may be driven by different threads concurrently.  A matrix handle carries run-time
 *     state (scratch of the two-phase kernel, the pace guard of the panel kernel), so do not apply the
 *     same handle from two streams at once.
 *   - the library is HIP-only.  There is no CPU fallback: without a usable GPU spmv_ctx_create
 *     fails with SPMV_ERR_NO_DEVICE and nothing else can be called.
 */
#ifndef SPMV_ABI_H
#define SPMV_ABI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPMV_ABI_VERSION 1

typedef enum spmv_status
{
    SPMV_OK             = 0,
    SPMV_ERR_INVALID    = -1, /* bad argument (null handle, negative size, shape mismatch) */
    SPMV_ERR_NO_DEVICE  = -2, /* no HIP device / device index out of range */
    SPMV_ERR_HIP        = -3, /* a HIP runtime call failed (message has hipGetErrorString) */
    SPMV_ERR_ALLOC      = -4, /* device or host allocation failed */
    SPMV_ERR_UNSUPPORTED = -5 /* valid request the engine does not implement */
} spmv_status;

typedef enum spmv_format
{
    SPMV_FMT_COO = 0, /* include/matrix.h:7-25  (reference) */
    SPMV_FMT_CSR = 1, /* include/matrix.h:27-47 */
    SPMV_FMT_CSC = 2, /* include/matrix.h:49-68 */
    SPMV_FMT_ELL = 3, /* include/matrix.h:70-92, column-major: (row i, slot k) at i + k*nrow */
    SPMV_FMT_DIA = 4, /* include/matrix.h:117-138, row-major: (row i, diag d) at i*ndiags + d */
    SPMV_FMT_BSR = 5, /* block CSR, square blocks of bs x bs values, 2 <= bs <= 8 (no counterpart in the reference): spmv_bsr_upload */
    SPMV_FMT_CSR_F32 = 6 /* CSR whose values are stored as float, one packed 8-byte word per entry (no counterpart in the reference):
                            spmv_csr_to_f32, spmv_csr_f32_upload */
} spmv_format;

/* CSR kernel selection (spmv_mat_set_kernel).  AUTO (csrc/select.hip) is decided when the handle is
 * created - one-off, outside every timed region, like the reference's shard construction (src/mat_vec.cpp:240-268):
 *   the model   statistics of the matrix: fewer than 1.5M entries -> VECTOR (or LDSWIN for narrow bands; PANEL when a few hub
 *               rows dwarf the mean: they would serialise on one lane group); larger -> PANEL, or TWOPHASE when the sweeps of x
 *               the panel kernel would make (8 XCDs x rounds x 8 * ncol bytes) outweigh the 16 extra bytes per entry of the two
 *               phases, or VECTOR when the rows are long contiguous runs (dense blocks of 32 and more: x is read coalesced);
 *   the trial   handles of 64K to 8M entries - where a product takes microseconds and the candidates lie within a factor of a
 *               few - TIME their candidates (PANEL, VECTOR, LDSWIN where the windows fit, SCALAR for short even rows, the
 *               model's pick): 1 warm-up + 2 x 4 products each on zeroed scratch vectors (8 * (nrow + ncol) bytes, freed
 *               before the call returns), a candidate 3x behind after its first product is dropped at once, the fastest
 *               stays, layouts built for the others are freed.  Larger handles keep the model's pick without a launch, unless
 *               a statistic casts doubt on it: rows that are contiguous runs (then VECTOR and PANEL are timed), the model's
 *               TWOPHASE below 64M entries (PANEL is timed beside it).  At ANY size: a longest row with 1/128 of the entries
 *               adds SEGSCAN, rows 32x the mean (and >= 4096; from 8M entries on >= 1/512 of the entries) add SPLIT - from 8M
 *               entries on at two thresholds -, (nearly) equal rows with local columns add ELL (the kernels' own comments
 *               below).  The panel layout itself times a cut for more rounds of workgroups where skewed rows leave its
 *               busiest row group far above the mean ("panel_rounds").  COO and ELL handles time their own
 *               kernel(s) against a row-grouped CSR copy of themselves - which picks ITS kernel the same way - where that copy
 *               is a candidate (below).  "panel_trial" 0 / SPMV_PANEL_TRIAL=0: no timing launch anywhere, the model alone.
 *   what was timed is on record: spmv_mat_get_param "select_candidates", "select_us_vector" / "_ldswin" / "_scalar" / "_panel" /
 *   "_twophase" (microseconds per product, 0 = not timed; COO / ELL: "_vector" the format's own kernel, "_panel" the copy; ELL
 *   also "_variant1" one row per lane, "_variant2" two rows per lane reading every index), "rowgrouped_kernel" (the kernel the
 *   copy of a COO / ELL / CSC handle runs, 0 = no copy in use), "ell_variant", "contiguous_permille"; CSR handles also
 *   "select_us_segscan" / "_split" / "_split_low" / "_ell", "min_row_entries", for kernel ELL "ell_copy_slots",
 *   "ell_copy_diagonal_slots", "ell_copy_variant", and for kernel SPLIT "split_row_threshold" (get: in effect; set: 0 = default, read at the
 *   next spmv_mat_set_kernel), "split_mode" (likewise; get: the mode in effect), "split_long_rows", "split_long_entries",
 *   "split_inner_kernel" (what the short rows' copy runs), "split_long_kernel" / "split_virtual_rows" (mode 2).
 *   Audit on stencils, dense blocks, R-MAT graphs, rectangles, permutations, arrow and dense-row shapes, power laws, bands and meshes:
 *   tools/sweep_structures.py, tools/fuzz_medium.py, profiles/r05_sweep_structures_*, profiles/r05_fuzz_medium_sizes.txt.
 *
 * Order of the additions (all within the parity tolerance of 1e-10):
 *   SCALAR              the reference's own order (left to right inside a row): bit-identical to its fma flavour;
 *   VECTOR, LDSWIN      a fixed tree per row: deterministic, the same bits on every call;
 *   PANEL, TWOPHASE     products are added into per-row accumulators in LDS with ds_add_f64 in ARRIVAL order: two calls
 *                       on the same data may differ in the last bits (the reference's CSR loop is deterministic per row,
 *                       src/mat_vec.cpp:57-65; its COO and CSC loops are not: `omp atomic`, :36-39, :88-91).  Callers that
 *                       need run-to-run identical bits select VECTOR (spmv_mat_set_kernel(A, SPMV_CSR_VECTOR, 0));
 *   SEGSCAN             a fixed tree inside a wavefront's 512 entries; rows that cross into another wavefront's entries are joined by
 *                       atomic adds on y in arrival order (like the COO scan);
 *   ELL                 the reference's ELL order (slot after slot into the row's sum): deterministic;
 *   SPLIT               the long rows: mode 1 a fixed tree per chunk of 4096 entries, chunks joined by atomic adds in arrival order;
 *                       mode 2 as the virtual rows' kernel, then a fixed order over a row's partial sums; the other rows: as the
 *                       inner kernel. */
typedef enum spmv_csr_kernel
{
    SPMV_CSR_AUTO     = 0,
    SPMV_CSR_VECTOR   = 1, /* 2^k lanes per row, ds_swizzle/DPP segment reduction */
    SPMV_CSR_LDSWIN   = 2, /* row blocks whose x window is staged in LDS (banded matrices) */
    SPMV_CSR_SCALAR   = 3, /* one lane per row, strictly left-to-right (bitwise = oracle _fma) */
    SPMV_CSR_PANEL    = 4, /* row groups x column panels: x gathered from L2, y accumulated in LDS */
    SPMV_CSR_TWOPHASE = 5, /* x-stationary expand + y-stationary reduce (x far larger than the rows held: C5 shards) */
    SPMV_CSR_SEGSCAN  = 6, /* the entries in row order, 512 per wavefront whatever row they belong to, joined by a segmented scan
                              (the COO kernel over a row index per entry, 4 bytes per entry on top of the CSR arrays): a matrix whose
                              longest rows hold a large share of the entries - arrow shapes, a few dense rows - where every other CSR
                              kernel leaves that row to ONE wavefront or workgroup (1M entries in one row: 1.26 ms there, 0.045 here).
                              CSR handles only; AUTO times it where the longest row exceeds 1/128 of the entries */
    SPMV_CSR_SPLIT    = 7, /* the rows of "split_row_threshold" entries and more (default: a sixteenth of the longest row, at least
                              4096) leave the matrix; every other row goes into a copy without them, which picks its own kernel
                              ("split_inner_kernel"; the panel layout as a rule).  The long rows ("split_mode": 0 by their density):
                              1 = in chunks of 4096 entries over the handle's own arrays, one workgroup and one atomic add on y each
                              (dense rows: an entry per 2 columns); 2 = dealt out to virtual rows of 64 entries (entry j of a row to
                              virtual row j mod V) that form a CSR matrix with a handle and a kernel of its own ("split_long_kernel",
                              "split_virtual_rows"), its product summed per long row in a fixed order (long AND sparse rows: power
                              laws, graph hubs).  1M rows x 32 + one dense row: panel 1.26 ms, scan 0.47, split 0.11; 1M rows of
                              min(500000, 8/u) entries: panel 0.64, split 0.29.  CSR handles only; AUTO times it where the longest
                              row is >= 4096 and 32x the mean */
    SPMV_CSR_ELL      = 8  /* an ELL copy of the handle (column-major slots, padded to the longest row with value 0.0 and the row's own
                              last column; the copy's kernels leave that padding OUT of the sums - its slots are marked in the
                              copy's index stream - so the copy is the CSR matrix in non-finite arithmetic too) with the ELL kernels -
                              diagonal slots recognised, one or two rows per lane, the DIA-order copy, timed - for
                              matrices of (nearly) equal rows: stencils, bands, block diagonals (tridiagonal, 8M rows: panel 0.087
                              ms, this 0.056; a band of 33: 0.163 / 0.105).  12 bytes per slot on top of the CSR arrays.  CSR
                              handles only; AUTO times it where the padding stays below a quarter, no row is empty and the columns are local
                              (the x window of 256 rows within 2 MB, or all of x within 4 MB) */
} spmv_csr_kernel;

/* Tuning bits for spmv_mat_set_flags (speed only; results stay within the parity tolerance). */
#define SPMV_FLAG_DPP_REDUCE 1u /* CSR vector kernel: DPP row shifts instead of ds_swizzle for the <=16-lane steps */
#define SPMV_FLAG_XCD_REMAP  2u /* CSR vector kernel: each XCD walks one contiguous eighth of the rows */
#define SPMV_FLAG_ELL_READ_COLUMNS 8u /* ELL kernel: read the column indices even where the slots were found to be diagonals (A/B switch) */
#define SPMV_FLAG_DIA_GLOBAL_X 4u /* DIA kernel: read x from global memory even when the offsets lie in a band (A/B switch) */

typedef struct spmv_ctx spmv_ctx; /* one HIP device + one stream */
typedef struct spmv_vec spmv_vec; /* device-resident fp64 vector         (reference: class Vector) */
typedef struct spmv_mat spmv_mat; /* device-resident sparse matrix/shard (reference: XMatrix) */

typedef struct spmv_mat_info
{
    int32_t format;   /* spmv_format */
    int32_t nrow;     /* rows held by this handle (a shard holds its own rows only) */
    int32_t ncol;     /* columns = length of x (always global: x is a full replica, mat_vec.cpp:257) */
    int32_t ell_k;    /* ELL: slots per row (nonzeros_in_row); DIA: ndiags; BSR: the block size bs; else 0 */
    int64_t nnz;      /* stored nonzeros (ELL: true nnz given at creation, not nrow*k; BSR: stored values, blocks * bs * bs) */
    int64_t row_begin; /* first global row of this shard (0 for an unsharded matrix) */
    int32_t max_row_nnz; /* (BSR: the most blocks in a block row, times bs) */
    int32_t kernel;   /* CSR: the spmv_csr_kernel in effect.  COO / ELL / CSC: 1 = the format's own kernel (segmented scan / lanes
                         over rows / scatter over columns), 4 = the product runs from the handle's row-grouped CSR copy, whichever
                         kernel that copy runs (spmv_mat_get_param "rowgrouped_kernel") */
    int32_t lanes_per_row; /* CSR vector kernel: lanes cooperating on one row; BSR: lanes cooperating on one block row */
    int32_t sorted_rows;   /* COO: 1 if row indices are non-decreasing */
    int64_t device_bytes;  /* bytes of device memory owned by the handle */
} spmv_mat_info;

/* ---- library / context ---------------------------------------------------------------------- */
int         spmv_abi_version(void);
const char* spmv_last_error(void);
int         spmv_device_count(int* count);
/* Creates a context on `device` with its own non-blocking stream. */
int spmv_ctx_create(int device, spmv_ctx** out);
/* Same, but queues all work on a caller-owned hipStream_t (e.g. torch's current stream). */
int spmv_ctx_create_on_stream(int device, void* hip_stream, spmv_ctx** out);
int spmv_ctx_destroy(spmv_ctx* ctx);
int spmv_sync(spmv_ctx* ctx);
int spmv_ctx_device(const spmv_ctx* ctx, int* device);
/* The context's start-up probe of workgroup placement: *round_robin = 1 when the workgroups of a launch are dealt round-robin
 * over 8 XCDs (b and b + 8 share an XCD and its L2; read from the XCC_ID hardware register by 2048 workgroups when the context
 * was created), 0 when not (a partitioned device, another dispatch order), -1 when the probe could not run; *xcds_seen = distinct
 * XCD ids seen.  HIP promises no placement: layouts that lean on it for speed - the COO scan over one column bin per XCD
 * ("coo_column_bins") - are built only when it is 1 (otherwise the scan runs in place and the library says so once on stderr);
 * nothing leans on it for correctness.  Either pointer may be NULL. */
int spmv_ctx_xcd_round_robin(spmv_ctx* ctx, int32_t* round_robin, int32_t* xcds_seen);
/* What a context found out about its platform when it was created (read-only):
 *   "host_stores"      1 = spmv_apply_host stores a small x straight into device memory from the CPU (large BAR reported, a
 *                      self-check passed at creation - CPU stores summed by a kernel, twice - and SPMV_HOST_STORES is not 0)
 *   "xcd_round_robin", "xcds_seen"   as spmv_ctx_xcd_round_robin
 *   "trial_arena_bytes"  bytes of the arena that timing launches of AUTO take their scratch vectors from (0 until a trial ran)
 *   "cg_graph_replays"   launches of the captured four iterations by spmv_cg under SPMV_CG_GRAPH=1 so far (0: never replayed) */
int spmv_ctx_get_param(const spmv_ctx* ctx, const char* name, int64_t* value);
/* free and total device memory in bytes (sizing shards for 288 GB of HBM; checking that handles give memory back) */
int spmv_ctx_mem_info(spmv_ctx* ctx, int64_t* free_bytes, int64_t* total_bytes);

/* ---- vectors  (reference: include/vector.h:4-26 {int size; double* values}) --------------------- */
int spmv_vec_create(spmv_ctx* ctx, int64_t n, spmv_vec** out);
int spmv_vec_wrap_device(spmv_ctx* ctx, int64_t n, double* device_ptr, spmv_vec** out);
int spmv_vec_destroy(spmv_vec* v);
int spmv_vec_size(const spmv_vec* v, int64_t* n);
int spmv_vec_device_ptr(const spmv_vec* v, double** device_ptr);
/* copy host[0..n) -> v[offset..offset+n)  /  v[offset..offset+n) -> host[0..n); both synchronous */
int spmv_vec_upload(spmv_vec* v, int64_t offset, int64_t n, const double* host);
int spmv_vec_download(const spmv_vec* v, int64_t offset, int64_t n, double* host);
int spmv_vec_fill(spmv_vec* v, double a); /* Vector::Fill, src/vector.cpp:59-63 */
/* dst[dst_offset..+n) = src[src_offset..+n) between vectors of ANY two contexts (same GPU or peers over xGMI), queued on
 * the destination's stream behind the work already queued on the source's.  The sharded drivers assemble y with it
 * (the reference leaves the per-thread Y slices where they are, src/mat_vec.cpp:287-296; DIA copies them, :474-477). */
int spmv_vec_copy(spmv_vec* dst, int64_t dst_offset, const spmv_vec* src, int64_t src_offset, int64_t n);

/* ---- exchange between the contexts (GPUs) of ONE process -------------------------------------------------
 * Replaces the x replication of the reference's sharded drivers — memcpy(p[i].X, x.values, ...) per NUMA node,
 * src/mat_vec.cpp:257,266 — by an all-gather on the devices: participant i holds slice [offsets[i], offsets[i+1]) of x
 * in its own (full-length) vector; afterwards every participant's vector holds all of [0, offsets[n]).  Asynchronous:
 * ordered by events behind the work queued on the participants' streams, and the streams continue behind it.
 * Transport: RCCL (ncclCommInitAll; one in-place ncclAllGather when the slices are equal, else a group of broadcasts, one
 * per slice; loaded with dlopen and called through rccl.h's own prototypes; fresh communicators pass a self-check first) when
 * there are two or more participants, each with a GPU of its own, else — or with SPMV_COMM=peer — concurrent
 * hipMemcpyPeerAsync pulls, one stream per peer link.  SPMV_COMM=rccl: RCCL or SPMV_ERR_*, also with ONE participant (a
 * one-GPU box exercising the RCCL calls).  Participants may share a GPU (several shards on one device): then the copies
 * are device-to-device.  The calling thread's current HIP device is left as it was found.
 * (One process per GPU instead: arm-spmv_amd/dist.py does the same exchange through torch.distributed.) */
typedef struct spmv_comm spmv_comm;
int         spmv_comm_create(spmv_ctx* const* ctxs, int32_t n, spmv_comm** out);
void        spmv_comm_destroy(spmv_comm* comm);
const char* spmv_comm_backend(const spmv_comm* comm); /* "rccl" or "peer-copy" */
int         spmv_comm_allgather(spmv_comm* comm, spmv_vec* const* vecs, const int64_t* offsets /* n + 1 */);

/* ---- matrices ------------------------------------------------------------------------------ */
/* CSR (include/matrix.h:27-47).  nnz = row_ptr[nrow]. */
int spmv_csr_upload(spmv_ctx* ctx, int32_t nrow, int32_t ncol, const int32_t* row_ptr,
                    const int32_t* col_ind, const double* values, spmv_mat** out);
int spmv_csr_wrap_device(spmv_ctx* ctx, int32_t nrow, int32_t ncol, const int32_t* d_row_ptr,
                         const int32_t* d_col_ind, const double* d_values, spmv_mat** out);
/* One row-range shard [row_begin,row_end) of a host CSR matrix whose offsets may exceed int32:
 * row_ptr64 is the GLOBAL 64-bit offset array; the shard keeps a rebased int32 row_ptr and global
 * column indices, exactly as src/mat_vec.cpp:250-265 builds NumaNode4CSR. */
int spmv_csr_upload_shard(spmv_ctx* ctx, int64_t row_begin, int64_t row_end, int32_t ncol,
                          const int64_t* row_ptr64, const int32_t* col_ind, const double* values,
                          spmv_mat** out);
/* COO (include/matrix.h:7-25): file order, unsorted and duplicate entries allowed (summed). */
int spmv_coo_upload(spmv_ctx* ctx, int32_t nrow, int32_t ncol, int64_t nnz, const int32_t* row_ind,
                    const int32_t* col_ind, const double* values, spmv_mat** out);
int spmv_coo_wrap_device(spmv_ctx* ctx, int32_t nrow, int32_t ncol, int64_t nnz,
                         const int32_t* d_row_ind, const int32_t* d_col_ind, const double* d_values,
                         spmv_mat** out);
/* ELL (include/matrix.h:70-92): column-major nrow*k arrays, padding col 0 / val 0.0
 * (src/matrix.cpp:473-474).  nnz = true nonzero count (used for the flop count only). */
int spmv_ell_upload(spmv_ctx* ctx, int32_t nrow, int32_t ncol, int32_t k, int64_t nnz,
                    const int32_t* col_ind, const double* values, spmv_mat** out);
int spmv_ell_wrap_device(spmv_ctx* ctx, int32_t nrow, int32_t ncol, int32_t k, int64_t nnz,
                         const int32_t* d_col_ind, const double* d_values, spmv_mat** out);
/* CSC (include/matrix.h:49-68) and DIA (include/matrix.h:117-138). */
int spmv_csc_upload(spmv_ctx* ctx, int32_t nrow, int32_t ncol, const int32_t* col_ptr,
                    const int32_t* row_ind, const double* values, spmv_mat** out);
int spmv_dia_upload(spmv_ctx* ctx, int32_t nrow, int32_t ncol, int32_t ndiags,
                    const int32_t* offsets, const double* values, spmv_mat** out);

int spmv_mat_destroy(spmv_mat* m);
int spmv_mat_get_info(const spmv_mat* m, spmv_mat_info* info);
/* Structural check for untrusted input (the products themselves, like the reference's loops, never check an index):
 * every row/column index inside its range, offset arrays non-decreasing from 0 to the entry count.
 * SPMV_ERR_INVALID + message if not.  One pass over the index arrays; synchronous. */
int spmv_mat_validate(const spmv_mat* m);
/* Force a CSR kernel (and, for VECTOR, lanes_per_row in {1,2,4,...,64}; 0 = keep auto choice).
 * COO, CSC and ELL handles take AUTO, VECTOR (the format's own kernel: segmented scan / atomic scatter / one lane per row;
 * for ELL lanes_per_row 1 or 2 picks the one- or two-rows-per-lane variant; for a large COO handle whose x is beyond an
 * XCD's L2 the scan runs over a copy of the entries in column bins - "coo_column_bins" below) or PANEL (regroup by row now and
 * run the panel kernel on that copy).  AUTO for COO: the scan over the entries as they are against a copy grouped by row
 * (duplicates and the order inside a row kept) that picks its own CSR kernel - timed from 64K entries on, the copy by the
 * model from 1.5M on.  AUTO for ELL: its own variants timed from 64K slots on; the row-grouped copy (every slot, padding
 * included: the sums and the reference's 0.0 * x[0] stay) is a candidate where one lane per row cannot work - at most 65536
 * rows of 16 slots and more, or rows whose blocks of 256 span more than 16 columns per row (scattered) and whose slots are not
 * diagonals.  AUTO for CSC: the scatter over the columns (one atomic on y per entry) against the copy grouped by row, timed
 * from 64K entries on, the copy by the model from 1.5M on. */
int spmv_mat_set_kernel(spmv_mat* m, int32_t kernel, int32_t lanes_per_row);
int spmv_mat_set_flags(spmv_mat* m, uint32_t flags);
/* Named parameters.  None is needed in normal use: what is left at its default is chosen when the layout is built, by
 * timing a handful of launches (about 0.1 s for 320M entries; SPMV_PANEL_TRIAL=0 or "panel_trial" 0: no launches, the
 * choice that wins on scattered columns).  Panel-kernel parameters take effect with the next spmv_mat_set_kernel:
 *   "panel_rows"     rows per group (0 = choose, entry-balanced; at most 20000)
 *   "panel_rounds"   0 (default) = the fewest groups the cap of 20000 rows allows, a whole number of rounds of 256 workgroups; where
 *                    skewed rows leave the busiest CU more than 1.15x the mean, a cut for 2-4 rounds is timed against it (get:
 *                    "panel_rounds" what was built, "panel_rounds_us_one" / "_more" the timing); 1 = never, k = groups for k rounds
 *   "panel_width"    columns per panel (0 = 131072; at most 524288, rounded down to whole 128-byte lines of x)
 *   "panel_sort"     1 = bucket the entries of a panel by 128-byte line of x (default), 0 = leave unordered
 *   "panel_aos"      entry layout: 4 = 12-byte packed entries, slices of 1024 stored in interleaved pairs and read with 8- and
 *                    16-byte loads (default; falls back to 0 where padding would outweigh it), 3 = the same without the
 *                    pairing (4-/8-byte loads), 0 = three arrays (14 bytes)
 *   "panel_unroll"   chunk = unroll x 1024 entries: 2, 4 or 8 (0 = by trial; 16 existed through round 3 - every instance spilled
 *                    registers - and now runs 8)
 *   "panel_pipe"     order of a chunk's memory instructions: 0 = no pipelining, 1 = next chunk's stream first,
 *                    2 = this chunk's gathers first (-1 = by trial)
 *   "panel_sync"     how the 16 wavefronts of a workgroup are kept in the same chunk: 0 = not at all, 1 = workgroup barrier at
 *                    the top of every chunk, 3 = barrier between a chunk's loads and its LDS adds (-1 = by trial; DESIGN.md 4.2:
 *                    this is what keeps the workgroups of an XCD in step on scattered columns).  (2, a split barrier through an LDS
 *                    counter, was measured no better than 3 and runs 3 since round 5.)
 *                    Round 1's clock throttle and what hung on it - "panel_pace_ns", "panel_guard", "panel_stagger", the trace build
 *                    "panel_trace", the A/B switch "panel_legacy" - were deleted in round 5 with the kernel that carried them
 *                    inside its chunk loop (the headline's schedule had come to depend on that dead code: DESIGN.md 4.2).
 *   "panel_keep_csr" 0 = release col_ind / values of a CSR handle whose product runs from the panel or two-phase layout or from its ELL copy
 *                    (memory 2x -> 1x the matrix; download, other kernels, re-builds and conversions are then refused)
 *   "panel_trial"    1 / 0 = timing launches when the layout is built, yes / no (-1 = environment, default yes)
 *   "dia_col_bound"  DIA handles: columns >= this are skipped (row shards keep the bound of the whole matrix)
 *   "twophase_panel_cols"   two-phase CSR kernel: columns of x per panel (<= 20000, even); takes effect at the next
 *                    spmv_mat_set_kernel(SPMV_CSR_TWOPHASE)
 *   "twophase_placement_budget_mb", "twophase_choose_pieces"   two-phase CSR kernel, TRANSIENT MEMORY.  The stream of products
 *                    between the two phases (8 bytes per padded entry: 2.6 GB for 320M entries) lives in pieces of 1 GB,
 *                    and where those lie in the device's PHYSICAL memory decides a tenth of the product's time (DESIGN.md
 *                    4.7; nothing can be asked of the allocator).  When the layout is built - by spmv_mat_set_kernel(TWOPHASE),
 *                    or by the upload / generator calls when AUTO picks this kernel - the engine therefore allocates
 *                    budget / 1 GB more pieces than the stream needs, times configurations of pieces (3 products each,
 *                    ~0.3 s in all), keeps the fastest and FREES EVERY OTHER PIECE BEFORE THE CALL RETURNS.  While the call
 *                    runs it holds: the layout + budget (default 8192 MB, never more than a quarter of the free device
 *                    memory) + two scratch vectors (8 ncol + 8 nrow bytes).  Afterwards: the layout, its product stream
 *                    rounded up to whole gigabytes.  "twophase_placement_budget_mb": -1 = default (or the environment's
 *                    SPMV_TP_PLACEMENT_BUDGET_MB), 0 = no search and no timing launches ("panel_trial" 0 /
 *                    SPMV_PANEL_TRIAL=0 do the same), otherwise megabytes.  PRECEDENCE: a value >= 0 set on the handle wins
 *                    over the environment variable, which is consulted only while the handle's value is -1 (and only when a
 *                    layout is built or the search is run again, never on a product's path); "panel_trial" 0 /
 *                    SPMV_PANEL_TRIAL=0 override both (no search); it applies to the next build, or at once with
 *                    "twophase_choose_pieces" (any value): run the search again on the built layout.  Streams below 512 MB
 *                    are never searched.  The outcome is reported by spmv_mat_get_param (below); a timing launch that fails
 *                    is an error of the call, not a silent fallback.
 *                    Round 5: (a) a pool of more than 24 extra pieces is SAMPLED (every k-th piece, ~16 per slot): the classes of
 *                    physical memory come in runs of gigabytes to tens of gigabytes, so a 64 GB pool reaches as far with a
 *                    quarter of the timing launches; (b) "panel_keep_csr" 0 on a two-phase handle first offers the whole
 *                    gigabytes inside the col_ind / values arrays it is about to release to the search (no allocation, ~0.1 s):
 *                    an array that ends up under the stream stays with the layout, the pieces it replaced are freed
 *                    ("twophase_pieces_carved"; "twophase_offer_csr_copy" 0 switches the offer off).
 *   "twophase_rotate"   1 (default): workgroup b of the expand phase starts b / 256 of the way through its panels
 *   "twophase_only", "twophase_realloc", "twophase_pool_alloc", "twophase_pool_config"   experiments, refused unless
 *                    SPMV_EXPERIMENTS=1 is in the environment: run phase A (1) or B (2) alone - THE PRODUCT IS THEN WRONG -,
 *                    move streams of the built layout to fresh allocations (bits 1 products, 2 values, 4 columns, 8 rows,
 *                    16 table), hold a pool of pieces and put any of them under the product stream (10 bits per slot):
 *                    tools/tune_twophase.py, tools/probe_twophase_{moves,pairs,classes,rotate}.py
 *   "ell_tiled_values"  ELL handles whose slots were found to be diagonals, takes effect at once: 1 = keep a copy of the values
 *                    in tiles of 512 rows, (tile * k + slot) * 512 + row, and multiply from it - a workgroup then reads one
 *                    contiguous stretch instead of k stretches nrow * 8 bytes apart; same bits.  8 bytes per slot of device
 *                    memory for 1-7 % of the product's time (C3), so never made unasked.  0 = drop it.
 *   "coo_column_bins"   COO handles, takes effect at once: the segmented scan (kernel VECTOR) runs over a COPY of the entries in
 *                    8 x value column bins, the bins of one XCD after the other, so that each XCD gathers x from a slice that
 *                    stays in its L2 (kernels_coo.hip; C4: 0.76 ms against 1.81).  -1 = as many bins as keep a slice within
 *                    2 MB (what spmv_mat_set_kernel(VECTOR) does by itself when x is beyond 3 MB and the handle has >= 2M
 *                    entries), 0 = drop the copy: the scan reads the handle's own arrays in their order, 1..8 = bins per
 *                    XCD.  Costs 16 bytes per entry of device memory (+ up to 64 x 2048 entries of padding) and, while it is
 *                    built, 8 bytes per entry more.  Needs fewer than 2^31 - 131072 entries.  A row is spread over up to that
 *                    many runs, each ending in an atomic on y: results differ from the scan in place by rounding only.
 *   "symgs_order"    sweep order of spmv_symgs / SPMV_PRECOND_SYMGS: 1 multicolour (default), 0 the matrix's own row order
 *   "ilu0_order"     sweep order of the ILU(0) factorisation (spmv_ilu0_setup / SPMV_PRECOND_ILU0), with the same meaning and default
 *   "cheby_degree"   degree a solver's own set-up of SPMV_PRECOND_CHEBYSHEV takes (1 .. 64, default 4); "cheby_ratio": lmax / lmin where
 *                    lmin is estimated (2 .. 10^6, default 30); "cheby_lanczos_steps": 0 (default) .. 64, see spmv_chebyshev_setup
 *   "amg_level_kernel"   a CSR kernel id (1 .. 8) that the next spmv_amg_setup forces on every coarse handle; 0 (default): each selects.
 *                    An id that a coarse operator cannot run (LDSWIN: a block window wider than the tile) fails that set-up
 *                    (SPMV_ERR_UNSUPPORTED); no other kernel takes its place
 *   "fsai_level"     the pattern tril(A^level) that a solver's own set-up of SPMV_PRECOND_FSAI, and spmv_fsai_setup with level 0, take:
 *                    1 (default) .. 3
 *   "panel_two_per_cu"   0 = never two workgroups per CU (default 1: two when their accumulators fit the LDS twice) */
int spmv_mat_set_param(spmv_mat* m, const char* name, int64_t value);
/* What is in effect: "panel_rows", "panel_width", "panel_sort", "panel_groups", "panel_layout", "panel_unroll",
 * "panel_pipe", "panel_sync", "select_candidates" / "select_us_<kernel>" (what AUTO timed, microseconds per product; 0 = not timed),
 * "select_rounds" (rounds the last trial took until its candidates' minima stood still), "adds_into_y_with_atomics" (1: the product
 * adds into y with device atomics - the COO scan, the CSC scatter, CSR under SEGSCAN or SPLIT's chunks, or a copy that runs one of
 * those; spmv_apply_host then stages y in device memory),
 * "panel_bytes", "panel_keep_csr", "device_bytes", "window_max_span", "window_avg_span", "twophase_panel_cols",
 * "twophase_padded" (entries of the two-phase layout with its padding), "twophase_pieces" (1 GB pieces of its product stream),
 * "twophase_pieces_carved" (how many of them lie inside allocations taken over from the released CSR copy),
 * "ell_tiled_values" (1: the ELL product reads its values from the copy in tiles), "coo_column_bins" (bins of the copy the COO
 * segmented scan runs over, 0: none), "coo_bins_padded" (its entries with the padding),
 * "twophase_placement_budget_mb", "twophase_placements_timed" (configurations of pieces timed by the search, 0 = no search ran),
 * "twophase_placement_spread" (time as built / time kept in 1/1000, both re-timed in turn when the search is over; a
 * configuration that does not hold up there is dropped for the pieces as built, so never < 1000), "twophase_pieces_exchanged", "ell_diagonal_slots" (1: the slots of an ELL
 * handle were found to be diagonals and conforming rows read no column index), "symgs_order", "symgs_colours",
 * "symgs_levels_forward", "symgs_levels_backward", "symgs_launches", "symgs_bytes", "symgs_fused" (1: the colouring is proper and
 * the sweep takes one launch per colour), "ilu0_order", "ilu0_ready", "ilu0_colours", "ilu0_levels_forward", "ilu0_levels_backward",
 * "ilu0_launches" (per application), "ilu0_bytes", the "trsv_*" names listed at spmv_trsv_setup, the "cheby_*" names listed at spmv_chebyshev_setup, the "amg_*" names listed
 * at spmv_amg_setup, the "fsai_*" names listed at spmv_fsai_setup and the "spgemm_*" names listed at spmv_spgemm. */
int spmv_mat_get_param(const spmv_mat* m, const char* name, int64_t* value);
/* ---- plans: a handle's set-up decisions as plain data (plan.hip) ------------------------------------------------------------
 * AUTO is a measurement (spmv_mat_set_kernel above): which kernel a handle runs, in which layout, with which chunk size,
 * barrier placement, split threshold or ELL variant is found by timing candidates when the handle is created.  Consequences:
 * NON-DETERMINISM - two handles of one matrix, or two ranks holding statistically identical shards, may end on different
 * kernels (candidates within 2 % of each other swap places between two trials) and with them on different last bits of y (every
 * kernel stays within the parity tolerance; the order of a row's additions differs) and different step times - and set-up
 * time (C2: 0.2 s with the timing launches, 0.05 s without).  The reference builds its shards once, the same way every time
 * (src/mat_vec.cpp:240-268).  Three ways to get that back:
 *   - spmv_mat_set_kernel with an explicit kernel, or SPMV_PANEL_TRIAL=0 / "panel_trial" 0: the model alone, no launches;
 *   - a PLAN: spmv_mat_get_plan writes what a handle decided - for itself and for the copies it runs from - into a POD blob
 *     (16-byte header + 128 bytes per handle; pass buf = NULL to learn the size in *len); spmv_mat_set_plan builds exactly
 *     that kernel and layout on another handle of the same format, with NO timing launch;
 *   - spmv_ctx_set_plan: every handle of the plan's format created on the context afterwards (uploads, wraps, generators,
 *     conversions, spmv_csr_extract_rows) takes the plan instead of selecting; buf = NULL clears it.
 * A plan holds decisions, nothing about the matrix: row cuts, column panels and slot descriptors are derived again from the
 * handle's own arrays, so the plan of one shard fits a shard of another size (arm-spmv_amd/dist.py broadcasts rank 0's).  It
 * does not hold where a two-phase product stream lies in a device's physical memory: run "twophase_choose_pieces" afterwards
 * where that search is wanted.  A plan that does not fit the handle's matrix (an LDS window too wide, an ELL copy of a matrix
 * with an empty row) is an error of spmv_mat_set_plan; the handle then selects by itself.  Blobs are validated (magic, version,
 * sizes, ids, child indices) before anything is read from them. */
int spmv_mat_get_plan(const spmv_mat* m, void* buf, int64_t* len);
int spmv_mat_set_plan(spmv_mat* m, const void* buf, int64_t len);
int spmv_ctx_set_plan(spmv_ctx* ctx, const void* buf, int64_t len);
/* The checks spmv_mat_set_plan / spmv_ctx_set_plan run on a blob, by themselves (no device, no handle: a plan received from
 * another rank or read from a file can be looked at anywhere): SPMV_OK and the root's format, the root's kernel and the number
 * of nodes (any pointer may be NULL), or SPMV_ERR_INVALID with the reason in spmv_last_error(). */
int spmv_plan_check(const void* buf, int64_t len, int32_t* format, int32_t* kernel, int32_t* nodes);
/* Copy the arrays of a handle back to the host (any pointer may be NULL to skip it).
 *   CSR: a=row_ptr[nrow+1]  b=col_ind[nnz]      v=values[nnz]
 *   COO: a=row_ind[nnz]     b=col_ind[nnz]      v=values[nnz]
 *   ELL: a=NULL             b=col_ind[nrow*k]   v=values[nrow*k]
 *   CSC: a=col_ptr[ncol+1]  b=row_ind[nnz]      v=values[nnz]
 *   DIA: a=offsets[ndiags]  b=NULL              v=values[nrow*ndiags] */
int spmv_mat_download(const spmv_mat* m, int32_t* a, int32_t* b, double* v);
/* Device pointers of the same three arrays (borrowed; NULL where the format has none). */
int spmv_mat_device_ptrs(const spmv_mat* m, const int32_t** a, const int32_t** b, const double** v);

/* ---- the hot path: y += A*x  (include/mat_vec.h:7-11) ------------------------------------------ */
/* x must have ncol entries, y nrow entries (the shard's rows).  Asynchronous. */
int spmv_apply(spmv_ctx* ctx, const spmv_mat* A, const spmv_vec* x, spmv_vec* y);
/* `reps` back-to-back applications between two HIP events on the context's stream (the reference's
 * NUM_TEST loop, main.cpp:56-59).  Returns the mean milliseconds per application.  Synchronous. */
int spmv_apply_timed(spmv_ctx* ctx, const spmv_mat* A, const spmv_vec* x, spmv_vec* y, int32_t reps,
                     double* ms_per_apply);

/* ---- several vectors at once: Y += A*X  (not in the reference's API) ----------------------------------------------------------
 * Y += A*X (overwrite != 0: Y = A*X) for k vectors at once.  X holds ncol*k entries, Y nrow*k (the shard's rows), both ROW-MAJOR:
 * entry (j, c) of X at X[(int64)j*k + c] - a C-contiguous torch (ncol, k) tensor wrapped with spmv_vec_wrap_device is this layout.
 * 1 <= k <= 64.  CSR handles (uploaded, wrapped, shards) and ELL handles; COO / CSC / DIA: SPMV_ERR_UNSUPPORTED.  Asynchronous.
 * Every argument is checked before the device is touched: a null pointer, k out of range, X with other than ncol*k or Y with other
 * than nrow*k entries, X and Y overlapping, a CSR handle without its arrays (panel_keep_csr = 0): SPMV_ERR_INVALID.  Index arithmetic on X and Y is 64-bit (ncol*k passes 2^31 at 34M
 * columns and k = 64).
 * Order of the additions (the contract): column c of Y is BIT-IDENTICAL to the oracle's fma flavour on column c of X -
 *   CSR  a row's sum runs left to right from 0.0 with fma, then y += sum (y = sum with overwrite): the SCALAR kernel's order;
 *   ELL  the accumulator starts at y (0.0 with overwrite) and goes slot after slot; padding slots contribute 0.0 * X[pad col, c]
 *        (column 0 in the reference's layout) as spmv_apply on a true ELL handle does.
 *   So the product is deterministic, and k = 1 gives the bits of SPMV_CSR_SCALAR, which may differ in the last bits from what
 *   AUTO picked for spmv_apply on the same handle.
 * The product reads only the handle's own arrays (row_ptr / col_ind / values; ELL col_ind / values).  It deliberately ignores the
 * kernel AUTO or spmv_mat_set_kernel chose, the copies and layouts made for it (ELL copy, split, panel layout, row-grouped copy)
 * and the plan, and changes none of them: a handle's plan stays canonical whether or not it was used here.
 * Kernel (kernels_spmm.hip): a group of lanes owns one row and lane t one column of a tile of T = the next power of two >= k, at
 * most 16, columns; a larger k runs ceil(k / 16) column tiles, each re-reading the matrix (from the caches where it can).
 * SPMV_SPMM_LANES=32 or 64 (environment, read once per process at the first call; an A/B switch; other values are ignored) lets
 * one group cover up to that many columns instead.
 * A CSR handle that released its arrays (spmv_mat_set_param "panel_keep_csr" 0) has nothing this product can read: SPMV_ERR_INVALID.
 * Limitation: a row's entries form ONE chain of fmas per column, so a very long row runs on one lane group, in series: the arrow
 * matrix of 1M rows (one row of 1M entries) takes 90-98 ms per product at k = 1-32, against 0.02-0.66 ms for k spmv_apply calls
 * (DESIGN.md 9).  Splitting long rows would break the bit-identity. */
int spmv_apply_multi(spmv_ctx* ctx, const spmv_mat* A, int32_t k, const spmv_vec* X, spmv_vec* Y, int32_t overwrite);
/* `reps` back-to-back spmv_apply_multi between two HIP events on the context's stream; the mean milliseconds per product.
 * Synchronous. */
int spmv_apply_multi_timed(spmv_ctx* ctx, const spmv_mat* A, int32_t k, const spmv_vec* X, spmv_vec* Y, int32_t overwrite,
                           int32_t reps, double* ms_per_apply);

/* ---- dense products sampled on a CSR pattern (SDDMM), and a handle over their result ---------------------------------------------
 * spmv_sddmm:   out[e] = alpha * sum_{c < k} U[row(e), c] * V[col(e), c] + beta * out[e]   for every stored entry e of A.
 * A supplies the PATTERN only: its values are never read.  CSR handles (uploaded, wrapped, row shards: U then has the shard's rows);
 * every other format: SPMV_ERR_UNSUPPORTED, the message naming the format.  U holds nrow*k entries and V ncol*k, both ROW-MAJOR as
 * X and Y of spmv_apply_multi (a C-contiguous torch (n, k) tensor wraps directly); out holds info.nnz entries in the handle's CSR
 * entry order: out[row_ptr[i] + t] belongs to the t-th stored entry of row i.  1 <= k <= 64.  Index arithmetic on U and V is 64-bit.
 * beta == 0.0: out is NOT READ (NaN in it does not propagate); alpha == 0.0 has no special case.  U and V may be the same vector
 * (nrow == ncol).  nnz = 0, nrow = 0 or ncol = 0 succeed and launch nothing.  Asynchronous on the context's stream.
 * Every argument is checked on the host before the device is touched: a null pointer, k out of range, U, V or out of another
 * length, out overlapping U or V, a CSR handle that released its arrays (panel_keep_csr = 0): SPMV_ERR_INVALID with a message, out
 * untouched.
 * This is the adjoint of the products in the matrix values: for y = A x, dL/da_e = g[row(e)] * x[col(e)] (k = 1); for Y = A X,
 * dL/da_e = G[row(e), :] . X[col(e), :].
 * Order of the additions (the contract): every product U[i, c] * V[j, c] is rounded on its own (no fma).  With L the next power of
 * two >= k and p_c = 0.0 for k <= c < L, the L terms are summed as a balanced pairwise tree: p_c + p_(c xor 1), then the pair sums
 * at distance 2, 4, ..., L / 2 (k = 3: (p0 + p1) + (p2 + 0.0)).  Then out = alpha * s where beta == 0.0, else
 * fma(alpha, s, beta * out).  The order depends on k alone, never on the entry's position, its row's length or the launch: the call is
 * deterministic, and the same entries stored as one long row or as many short ones give the same bits.
 * The call reads row_ptr and col_ind of the handle only and changes nothing in it: plan, kernel, copies and device_bytes stay.
 * Kernel (kernels_sddmm.hip, sddmm_settings.hpp): work is divided by entries, not rows - a wavefront takes a run of 512 entries
 * wherever they lie and finds its rows by searching row_ptr, so one row of 1M entries is spread like any other 1M entries. */
int spmv_sddmm(spmv_ctx* ctx, const spmv_mat* A, int32_t k, double alpha, const spmv_vec* U, const spmv_vec* V, double beta,
               spmv_vec* out);
/* `reps` back-to-back spmv_sddmm between two HIP events on the context's stream; the mean milliseconds per call.  Synchronous. */
int spmv_sddmm_timed(spmv_ctx* ctx, const spmv_mat* A, int32_t k, double alpha, const spmv_vec* U, const spmv_vec* V, double beta,
                     spmv_vec* out, int32_t reps, double* ms_per_call);
/* A new CSR handle that BORROWS A's device row_ptr / col_ind and the storage of `values` as its values: spmv_csr_wrap_device over
 * pointers the engine already holds, so that an spmv_sddmm result becomes a matrix every product and solver accepts without a round
 * trip through the host.  A row shard gives a row shard.  The new handle is validated and analysed like any wrapped handle
 * (synchronous); A is not changed.  The caller keeps A and the vector alive for as long as the new handle lives, and destroys the
 * new handle with spmv_mat_destroy.  Refused (SPMV_ERR_INVALID): null arguments, `values` with other than nnz entries, A not a CSR
 * handle with its arrays. */
int spmv_csr_with_values(spmv_ctx* ctx, const spmv_mat* A, const spmv_vec* values, spmv_mat** out);

/* y += A^T x.  x has nrow entries (the shard's rows), y has ncol entries.  Asynchronous.  Every format: CSR (uploaded, wrapped,
 * shard), CSC and COO run on an internal companion handle that borrows A's arrays read the other way round (CSR -> CSC, CSC ->
 * CSR, COO -> COO with rows and columns swapped) and picks its own kernel; ELL runs as a COO companion that borrows col_ind and
 * values and owns one array of slot rows (padding slots take part, as in the forward product); DIA has a kernel of its own over
 * A's row-major values (outputs j < the forward product's column bound, diagonals in slot order from y_j).  A CSR row shard
 * gives its own contribution y[0..ncol) += A_p^T x_p (the caller sums over the shards).  Refused on the host, before any device
 * use: null arguments, wrong lengths, overlapping x and y, a CSR handle that released its arrays (panel_keep_csr = 0).
 * The transposed state never changes the handle's forward state: kernel, copies, device_bytes and plan stay as they were.
 * Parameters: "transpose_kernel" (set before the set-up; handed to spmv_mat_set_kernel on the companion; reads back the
 * companion's kernel), "transpose_bytes", "transpose_ready" and "transpose_rowgrouped_kernel" (read-only).  DESIGN.md 10. */
int spmv_apply_transpose(spmv_ctx* ctx, const spmv_mat* A, const spmv_vec* x, spmv_vec* y);
/* `reps` back-to-back spmv_apply_transpose between two HIP events; the set-up, if still due, runs before the first event.
 * Synchronous. */
int spmv_apply_transpose_timed(spmv_ctx* ctx, const spmv_mat* A, const spmv_vec* x, spmv_vec* y, int32_t reps, double* ms_per_apply);
/* Build the handle's transposed state now.  Synchronous and idempotent.  The first spmv_apply_transpose also runs it. */
int spmv_mat_transpose_setup(spmv_mat* A);

/* y_host += A * x_host with the caller's HOST vectors, synchronous - the reference's own call shape (include/mat_vec.h:7-11:
 * every CSRMatrixMatVector(A, x, y) hands over host arrays; main.cpp:56-59 does it 50 times), as ONE entry point so that the
 * hand-over can be done the cheapest way for its size.  Vectors of up to 1 MB together: x by CPU stores straight into device
 * memory where the platform has a large BAR and the context's self-check of such stores passed (SPMV_HOST_STORES=0: through a
 * pinned staging buffer and one more launch); y stays on the HOST where the kernel that runs forms a row's sum before it adds it
 * to y (row-parallel, panel and two-phase CSR: the kernel writes the sums into the pinned buffer, the host adds them to y while
 * it copies out - the same IEEE addition, bit for bit), is updated in place in the pinned buffer over the host link where the
 * accumulator starts at y_i (ELL, DIA, scalar and LDS-window CSR), and goes through a device buffer for the kernels that add
 * into y with atomics (spmv_mat_get_param "adds_into_y_with_atomics"; two more launches).  The call ends in hipStreamSynchronize.
 * Larger vectors: asynchronous copies.  x_host has ncol entries, y_host nrow.  The caller's arrays are neither registered nor
 * mapped (they may be freed or moved between calls).  C1 (10000 x 10000 x 16): 22 us per call, of which the kernel takes 3 - the
 * rest is one launch and its completion (10.5 us for an empty kernel on this platform), 80 KB each way and the runtime; never
 * part of a throughput figure: resident vectors (spmv_apply) are what the roofline numbers are measured with. */
int spmv_apply_host(spmv_ctx* ctx, const spmv_mat* A, const double* x_host, double* y_host);

/* ---- BLAS-1 (include/vec_vec.h:6-7) ---------------------------------------------------------- */
int spmv_dot(spmv_ctx* ctx, const spmv_vec* x, const spmv_vec* y, double* result); /* synchronous */
int spmv_axpby(spmv_ctx* ctx, double alpha, const spmv_vec* x, double beta, const spmv_vec* y,
               spmv_vec* w);

/* ---- the solver step around the product ------------------------------------ */
/* The reference ships vec_dot / vec_axpby (src/vec_vec.cpp) and `diagonal // for SymGS` fields
 * (include/matrix.h:36,81) for a Krylov loop it never calls; these two entry points are that loop,
 * device-resident.  Not present in the reference's API.
 *
 * spmv_apply_dot: y = A*x (overwrite != 0) or y += A*x, and *dot = sum_i w_i * y_i over the UPDATED y,
 *   computed in the product's own write-back where the kernel supports it (panel kernel), else by a
 *   pass behind it.  w has nrow entries and may be x itself (square A).  Synchronous (returns the scalar).
 * spmv_cg: conjugate gradients for symmetric positive definite A (square): solves A*x = b starting from
 *   the x passed in, until ||r|| <= rel_tol * ||b|| or max_iter iterations.  alpha/beta stay on the
 *   device; the host reads the residual every check_every iterations (>= 1).  *iters = iterations run,
 *   *rel_resid = ||r|| / ||b|| of the recurrence at the last check.  SPMV_ERR_INVALID if p.Ap <= 0.
 *   precond: spmv_precond (Jacobi uses the diagonal the reference's containers carry "for SymGS", matrix.h:36). */
int spmv_apply_dot(spmv_ctx* ctx, const spmv_mat* A, const spmv_vec* x, spmv_vec* y, int32_t overwrite,
                   const spmv_vec* w, double* dot);
enum spmv_precond
{
    SPMV_PRECOND_NONE   = 0,
    SPMV_PRECOND_JACOBI = 1, /* z = D^-1 r, D = diag(A) read from a CSR handle (zero diagonal: SPMV_ERR_INVALID) */
    SPMV_PRECOND_SYMGS  = 2, /* z = one symmetric Gauss-Seidel sweep on A z = r from z = 0 (spmv_symgs below; the handle is
                                set up on first use although it is passed as const) */
    SPMV_PRECOND_ILU0   = 3, /* z = U^-1 L^-1 r with the ILU(0) factors of a CSR handle (spmv_ilu0_setup below; set up on first use
                                in the same way).  spmv_cg, spmv_bicgstab and spmv_gmres; spmv_cg_multi: SPMV_ERR_UNSUPPORTED */
    SPMV_PRECOND_CHEBYSHEV = 4, /* z = p_d(diag(s) A) diag(s) r, a fixed Chebyshev polynomial applied through the handle's own forward
                                product (spmv_chebyshev_setup below).  A handle that was set up is used as it stands, any format; one
                                that was not is set up on first use with degree "cheby_degree" (4), Jacobi scaling and estimated
                                bounds, which needs a CSR handle with its arrays.  spmv_cg, spmv_bicgstab and spmv_gmres, with the
                                work vectors and arrangement of SPMV_PRECOND_ILU0; spmv_cg_multi: SPMV_ERR_UNSUPPORTED */
    SPMV_PRECOND_AMG = 5, /* z = B r, one V(1,1) cycle of aggregation AMG on a CSR handle (spmv_amg_setup below).  A handle that was set up
                            is used as it stands; one that was not is set up on first use with every default.  spmv_cg, spmv_bicgstab
                            and spmv_gmres, with the work vectors and arrangement of SPMV_PRECOND_ILU0; spmv_cg_multi:
                            SPMV_ERR_UNSUPPORTED */
    SPMV_PRECOND_FSAI = 6 /* z = G^T (G r), the factorised sparse approximate inverse of a symmetric positive definite CSR handle
                             (spmv_fsai_setup below): two forward products.  A handle that was set up is used as it stands; one that was
                             not is set up on first use at level "fsai_level" (1).  spmv_cg, spmv_bicgstab, spmv_gmres and spmv_lobpcg,
                             with the work vectors and arrangement of SPMV_PRECOND_ILU0; spmv_cg_multi: SPMV_ERR_UNSUPPORTED */
};
int spmv_cg(spmv_ctx* ctx, const spmv_mat* A, const spmv_vec* b, spmv_vec* x, int32_t max_iter,
            double rel_tol, int32_t check_every, int32_t precond, int32_t* iters, double* rel_resid);
/* spmv_cg_multi: k independent conjugate-gradient solves A x_c = b_c in one loop (solver_multi.hip).  B and X are
 *   ROW-MAJOR (nrow x k), as in spmv_apply_multi: entry (i, c) at [(int64)i*k + c].  X holds the starting vectors and receives the
 *   solutions.  iters and rel_resid are HOST arrays of k entries.  Synchronous.
 *   Columns are independent systems - this is not block CG: every column has its own alpha, beta, gamma and delta and follows the
 *   Chronopoulos-Gear recurrence of spmv_cg's two-launch iteration.  The product W = A U of an iteration runs
 *   through the spmv_apply_multi path with overwrite: the matrix is read once per iteration for all k systems, and column c of the
 *   product has the SCALAR order of additions, bit for bit, as that entry point promises.  Three launches per iteration.
 *   Handles: 1 <= k <= 64; CSR handles (uploaded, wrapped, shards that hold a square matrix) and ELL handles.  precond:
 *   SPMV_PRECOND_NONE, and SPMV_PRECOND_JACOBI on CSR (the diagonal as spmv_cg takes it, duplicates summed; a zero or missing
 *   diagonal entry: SPMV_ERR_INVALID).  SPMV_PRECOND_SYMGS, Jacobi on ELL and COO / CSC / DIA handles: SPMV_ERR_UNSUPPORTED.
 *   Stopping, per column: the host reads the k values of r.r every check_every iterations (>= 1) and after the last one; column
 *   c has converged when rr_c <= rel_tol^2 * bb_c and is then FROZEN by a flag on the device: later iterations leave its column of
 *   X and of every work vector untouched, bit for bit (it still rides through the product; converged columns are not compacted).
 *   iters[c] = the iteration count of the check that froze it, else the iterations run; rel_resid[c] = sqrt(rr_c / bb_c) at that
 *   check.  The call returns when every column is frozen or after max_iter iterations.
 *   A column with b_c = 0: iters[c] = 0, rel_resid[c] = 0, its column of X untouched (spmv_cg's rule at b.b = 0); its 0/0 reaches
 *   no other column and no status word.  A column whose r.r is at or below 1e-28 b_c.b_c passes quietly, as in spmv_cg.
 *   Breakdown: p.Ap <= 0 or r.M^-1 r <= 0 in a live column, or a non-finite b.b or r.r: SPMV_ERR_INVALID, and spmv_last_error()
 *   names the column; the other columns of X may then hold any iterate.
 *   Deterministic: no dot product is added up in arrival order (per-workgroup partial sums per column, added in a fixed order by
 *   the workgroup that finishes last), so two calls on the same data give the same bits - stronger than spmv_cg - and column c's
 *   result at fixed (nrow, k, c) depends on column c of B and X alone, not on what the other columns hold.
 *   Refused before any device use with SPMV_ERR_INVALID: null pointers, k out of range, a non-square matrix, B or X with other
 *   than nrow * k entries, B and X overlapping, max_iter < 0, rel_tol < 0, a CSR handle without its arrays (panel_keep_csr 0).
 *   Index arithmetic on the (nrow x k) blocks is 64-bit.  X and B need only be 8-byte aligned; where both are 16-byte aligned and
 *   k is even the vector kernels use 16-byte accesses.  The handle's forward state, copies and plan stay as they were.
 *   Device memory: four (Jacobi: five) work blocks of nrow * k doubles for the duration of the call. */
int spmv_cg_multi(spmv_ctx* ctx, const spmv_mat* A, int32_t k, const spmv_vec* B, spmv_vec* X, int32_t max_iter, double rel_tol,
                  int32_t check_every, int32_t precond, int32_t* iters, double* rel_resid);
/* spmv_cgls: least squares min ||b - A x||^2 + damp^2 ||x||^2 by CGLS, starting from the x passed in (solver_cgls.hip; DESIGN.md
 *   12).  b has nrow entries (a shard: its rows), x has ncol.  A is any handle spmv_apply and spmv_apply_transpose both accept: all
 *   five formats, uploaded, wrapped, or a shard, which is simply the rectangular matrix it holds.  Synchronous.
 *   The handle's transposed state is built on first use, although the handle is passed as const, as spmv_apply_transpose and
 *   SPMV_PRECOND_SYMGS build theirs; the forward state, copies, device_bytes and plan stay as they were.
 *   Recurrence:  r = b - A x;  s = A^T r - damp^2 x;  p = s;  gamma = s.s;  then per iteration  q = A p;  delta = q.q + damp^2 p.p;
 *   alpha = gamma / delta;  x += alpha p;  r -= alpha q;  s = A^T r - damp^2 x;  gamma' = s.s;  beta = gamma' / gamma;
 *   p = s + beta p;  gamma = gamma'.  Six launches per iteration (the two products and four vector kernels); alpha, beta, gamma and
 *   delta stay on the device; the host reads gamma, r.r and a status word every check_every iterations (>= 1) and after the last.
 *   Stopping: gamma <= rel_tol^2 * ||A^T b||^2 (the reference does not depend on x0; one more transposed product at the set-up), or
 *   max_iter iterations.  *iters = iterations run, *rel_normal_resid = sqrt(gamma / ||A^T b||^2) and *rel_resid = sqrt(r.r / b.b) at
 *   the last check (max_iter = 0: those of x0).  A^T b = 0, b = 0 among it: *iters = 0, both outputs 0, x untouched (spmv_cg's rule
 *   at b.b = 0).  An iteration whose gamma is at or below 1e-28 ||A^T b||^2 passes quietly, as in spmv_cg; gamma = 0 ends the solve.
 *   SPMV_ERR_INVALID with a message naming the quantity: a non-finite b.b, ||A^T b||^2, gamma or r.r, or delta <= 0 while gamma is
 *   above that floor.
 *   Refused before any device use with SPMV_ERR_INVALID: null pointers, b with other than nrow or x with other than ncol entries,
 *   b and x overlapping, max_iter < 0, rel_tol < 0, damp < 0 or not finite, a CSR handle without its arrays (panel_keep_csr 0).
 *   Deterministic dot products (per-workgroup partial sums added in a fixed order by the workgroup that finishes last): a solve is
 *   exactly as reproducible as the two products its handle runs.  x and b need only be 8-byte aligned; where they are 16-byte
 *   aligned the vector kernels use 16-byte accesses on them.  nrow = 0 or ncol = 0: SPMV_OK, *iters = 0, nothing is launched.
 *   Device memory: work vectors r, q (nrow) and p, s (ncol) and a small scalar block for the duration of the call. */
int spmv_cgls(spmv_ctx* ctx, const spmv_mat* A, const spmv_vec* b, spmv_vec* x, int32_t max_iter, double rel_tol,
              int32_t check_every, double damp, int32_t* iters, double* rel_normal_resid, double* rel_resid);
/* spmv_bicgstab: A x = b for a square A that need not be symmetric, by right-preconditioned BiCGSTAB, starting from the x passed in
 *   (solver_bicgstab.hip).  b and x have nrow entries.  A is any handle spmv_apply accepts: all five formats, uploaded,
 *   wrapped, or a shard that holds a square matrix.  Synchronous.  Both products of an iteration are forward ones and run the
 *   handle's own kernel; no transposed state is built, and the handle's kernel, copies, device_bytes and plan stay as they were.
 *   Recurrence:  r = b - A x;  rhat = r;  p = r;  rho = rhat.r;  then per iteration  phat = M^-1 p;  v = A phat;
 *   alpha = rho / rhat.v;  s = r - alpha v;  shat = M^-1 s;  t = A shat;  omega = t.s / t.t;  x += alpha phat + omega shat;
 *   r = s - omega t;  rho' = rhat.r;  beta = (rho' / rho) * (alpha / omega);  p = r + beta (p - omega v);  rho = rho'.
 *   precond: SPMV_PRECOND_NONE (M = I: phat and shat are p and s, no copies) or SPMV_PRECOND_JACOBI (M = diag(A) of a CSR handle,
 *   duplicates summed; a zero or missing diagonal entry: SPMV_ERR_INVALID).  The preconditioner is applied on the right, so r is
 *   the residual of A x = b itself.  SPMV_PRECOND_SYMGS and Jacobi on a non-CSR handle: SPMV_ERR_UNSUPPORTED (out of scope here).
 *   SPMV_PRECOND_ILU0 (M = L U of spmv_ilu0_setup; the handles that takes): phat and shat are two applications of spmv_ilu0_solve
 *   behind the plain direction and half-step kernels, 7 launches plus twice "ilu0_launches" per iteration, eight work vectors.
 *   Seven launches per iteration (the two products, two dot kernels, three vector kernels); alpha, omega, beta, rho and the dots
 *   stay on the device; the host reads r.r and a status word every check_every iterations (>= 1) and after the last one.
 *   Stopping: r.r <= rel_tol^2 * b.b on the recurrence's r, or max_iter iterations.  *iters = iterations run, *rel_resid =
 *   sqrt(r.r / b.b) at the last check.  b.b = 0: *iters = 0, *rel_resid = 0, x untouched (spmv_cg's rule).  r0.r0 = 0 or already
 *   within the tolerance, or max_iter = 0: no iteration, *rel_resid is that of x0.  An iteration that starts with r.r at or below
 *   1e-28 b.b passes quietly (x and the work vectors stay); r.r = 0 ends the solve.  t.t = 0 (s = 0: the half step landed):
 *   omega = 0, x += alpha phat, r = s.
 *   Breakdown - rho = 0, rhat.v = 0, or omega = 0 while r.r is above that floor, or a non-finite b.b, rho or r.r:
 *   SPMV_ERR_INVALID, and spmv_last_error() names the quantity and "at or before iteration k"; the kernel that detects it leaves x
 *   and r alone, so x holds an iterate of the recurrence.
 *   Refused before any device use with SPMV_ERR_INVALID: null pointers, nrow != ncol, b or x with other than nrow entries, b and x
 *   overlapping, max_iter < 0, rel_tol < 0, an unknown precond, Jacobi on a CSR handle without its arrays (panel_keep_csr 0; the
 *   plain solve takes such a handle).  nrow = 0: SPMV_OK, *iters = 0, nothing is launched.
 *   Deterministic dot products (per-workgroup partial sums added in a fixed order by the workgroup that finishes last): a solve is
 *   exactly as reproducible as the product its handle runs.  x and b need only be 8-byte aligned; where they are 16-byte aligned
 *   the vector kernels use 16-byte accesses on them.
 *   Device memory: six work vectors of nrow doubles (Jacobi: nine) and a small scalar block for the duration of the call, released
 *   on every path. */
int spmv_bicgstab(spmv_ctx* ctx, const spmv_mat* A, const spmv_vec* b, spmv_vec* x, int32_t max_iter, double rel_tol,
                  int32_t check_every, int32_t precond, int32_t* iters, double* rel_resid);
/* spmv_gmres: A x = b for a square A that need not be symmetric, by right-preconditioned restarted GMRES(restart), starting from the
 *   x passed in (solver_gmres.hip).  b and x have nrow entries.  A is any handle spmv_bicgstab takes: all five formats,
 *   uploaded, wrapped, or a shard that holds a square matrix.  Synchronous.  One forward product through the handle's own kernel and
 *   one preconditioner application per iteration (spmv_bicgstab: two of each); no transposed state is built, and the handle's kernel,
 *   copies, device_bytes and plan stay as they were.  It does not break down where BiCGSTAB does (the rotation [[0, 1], [-1, 0]]).
 *   restart = m: 1 .. 64; 0 means 30; anything else is SPMV_ERR_INVALID.
 *   Recurrence:  r = b - A x;  beta = ||r||;  v_0 = r / beta;  g = (beta, 0, ...);  then for column j = 0 .. m-1 of a cycle
 *   z = M^-1 v_j;  w = A z;  twice (classical Gram-Schmidt): c_i = v_i . w for i = 0..j, all against the same w, w -= sum_i c_i v_i,
 *   h_i += c_i;  h_{j+1} = ||w||;  v_{j+1} = w / h_{j+1};  the rotations 0..j-1 applied to h;  d = sqrt(h_j^2 + h_{j+1}^2);
 *   (cs_j, sn_j) = (h_j, h_{j+1}) / d;  h_j = d;  g_{j+1} = -sn_j g_j;  g_j = cs_j g_j.  The recurrence's residual is |g_{j+1}|.  A
 *   cycle ends at j = m, at a stop, at max_iter or when it landed:  y = R^-1 g;  x += M^-1 (sum_i y_i v_i);  and if the solve goes on,
 *   r = b - A x is computed again.
 *   precond: spmv_bicgstab's set with the same codes - SPMV_PRECOND_NONE (z is v_j, no copy), SPMV_PRECOND_JACOBI (M = diag(A) of a
 *   CSR handle, duplicates summed; a zero or missing diagonal entry: SPMV_ERR_INVALID), SPMV_PRECOND_ILU0 (M = L U of
 *   spmv_ilu0_setup; the handles that takes; one application per iteration and one at a cycle's end); SPMV_PRECOND_SYMGS and Jacobi
 *   on a non-CSR handle: SPMV_ERR_UNSUPPORTED.  The preconditioner is applied on the right, so r is the residual of A x = b itself.
 *   Six launches per iteration (the product, two dots kernels that take all j + 1 dots of a pass in one sweep, two updates, the
 *   normalisation; ILU(0): and "ilu0_launches"); R, cs, sn, g and y stay on the device; the host reads the residual, the column count
 *   and a status word every check_every iterations (>= 1), after the last one and behind every restart.
 *   Stopping: |g_{j+1}| <= rel_tol * ||b|| at a look; behind a restart the recomputed ||r|| is compared instead; or max_iter
 *   iterations.  *iters = iterations run, *rel_resid = that ratio at the last look.  max_iter = k with rel_tol = 0 runs exactly k
 *   iterations and leaves the GMRES iterate x_k, formed from the columns that stand, in x.  b.b = 0: *iters = 0, *rel_resid = 0, x
 *   untouched.  A start within the tolerance, or max_iter = 0: no iteration, *rel_resid is that of x0.  An iteration that starts with
 *   |g_j| at or below 1e-14 ||b|| passes quietly (its kernels write nothing: no vector is divided by a norm that is rounding noise;
 *   h_{j+1} = 0, the lucky breakdown, is such a case); the host ends the cycle at its next look with the columns that stand, and an
 *   exact 0 ends the solve.  Stagnation is no error: GMRES(1) on the rotation keeps |g| = ||b|| until max_iter and returns SPMV_OK.
 *   Breakdown - d = 0 (at or below 2^-44 times the norm of the new column) while the residual is above that floor: the Krylov space
 *   is exhausted and A is singular - or a non-finite b.b, beta, h or g: SPMV_ERR_INVALID, and spmv_last_error() names the quantity
 *   and "at or before iteration k"; x then holds the iterate of the last completed cycle.
 *   Refused before any device use with SPMV_ERR_INVALID: null pointers, nrow != ncol, b or x with other than nrow entries, b and x
 *   overlapping, restart outside 0 .. 64, max_iter < 0, rel_tol < 0, an unknown precond, Jacobi on a CSR handle without its arrays
 *   (panel_keep_csr 0; the plain solve takes such a handle).  nrow = 0: SPMV_OK, *iters = 0, nothing is launched.
 *   Deterministic dot products (per-workgroup partial sums per dot, added in a fixed order by the workgroup that finishes last): a
 *   solve is exactly as reproducible as the product its handle runs.  x and b need only be 8-byte aligned; where they are 16-byte
 *   aligned the vector kernels use 16-byte accesses on them.
 *   Device memory: restart + 2 work vectors of nrow doubles (ILU(0): + 3, Jacobi: + 4), the partial sums of restart + 2 quantities
 *   and a 36 KB block for the small problem for the duration of the call, released on every path; running out is SPMV_ERR_ALLOC with
 *   the size in the message. */
int spmv_gmres(spmv_ctx* ctx, const spmv_mat* A, const spmv_vec* b, spmv_vec* x, int32_t restart, int32_t max_iter, double rel_tol,
               int32_t check_every, int32_t precond, int32_t* iters, double* rel_resid);
/* spmv_minres: (A - shift I) x = b for a square SYMMETRIC A that need not be positive definite, by Paige and Saunders' preconditioned
 *   MINRES, starting from the x passed in (solver_minres.hip).  b and x have nrow entries.  A is any handle
 *   spmv_bicgstab takes: every format, uploaded, wrapped, or a shard that holds a square matrix; it is meant to be symmetric and nothing
 *   checks that.  Synchronous.  One forward product through the handle's own kernel and one preconditioner application per iteration,
 *   a three-term recurrence, no breakdown on a symmetric A, and a residual norm that never grows.  No transposed state is built, and the
 *   handle's kernel, copies, device_bytes and plan stay as they were.  The shift is applied behind the product, for every format: there
 *   is no handle of A - shift I.  Use: saddle-point systems, A - sigma I with sigma inside the spectrum, singular consistent systems.
 *   P: the handle the preconditioner `precond` is built from and kept in; NULL means A.  M must be symmetric positive definite, and one
 *   built from an indefinite A is not: pass blockdiag(K, I) for a saddle point, the unshifted operator for A - sigma I.  P is square, of
 *   A's size and in A's context; P given with SPMV_PRECOND_NONE is SPMV_ERR_INVALID.
 *   Recurrence:  r1 = b - (A - shift I) x;  y = M^-1 r1;  beta1 = sqrt(r1.y);  r2 = r1;  beta = beta1;  oldb = 0;  dbar = epsln = 0;
 *   phibar = beta1;  cs = -1;  sn = 0;  w = w2 = 0;  then per iteration  v = y / beta;  y = A v - shift v;  from the second one on
 *   y -= (beta / oldb) r1;  alfa = v.y;  y -= (alfa / beta) r2;  r1 = r2;  r2 = y;  y = M^-1 r2;  oldb = beta;  beta = sqrt(r2.y);
 *   oldeps = epsln;  delta = cs dbar + sn alfa;  gbar = sn dbar - cs alfa;  epsln = sn beta;  dbar = -cs beta;
 *   gamma = sqrt(gbar^2 + beta^2);  cs = gbar / gamma;  sn = beta / gamma;  phi = cs phibar;  phibar = sn phibar;  w1 = w2;  w2 = w;
 *   w = (v - oldeps w1 - delta w2) / gamma;  x += phi w.  phibar is ||r_k|| in the M^-1 norm (the 2-norm without a preconditioner).
 *   precond: SPMV_PRECOND_NONE, SPMV_PRECOND_JACOBI (the diagonal of P, a CSR handle with its arrays; a zero or missing entry:
 *   SPMV_ERR_INVALID, and so is a negative one, "the Jacobi preconditioner is not positive definite", at the set-up),
 *   SPMV_PRECOND_CHEBYSHEV, SPMV_PRECOND_AMG and SPMV_PRECOND_FSAI on the handles those take.  SPMV_PRECOND_SYMGS and SPMV_PRECOND_ILU0:
 *   SPMV_ERR_UNSUPPORTED (neither is a symmetric positive definite M).
 *   Four launches per iteration without a preconditioner and with Jacobi (the product; y and alfa; r2, r2.y and the rotation; w, x and
 *   the next v); a preconditioner applied by launches adds its own sequence and one dot kernel.  Every scalar stays on the device; the
 *   host reads phibar, the iteration count and a status word every check_every iterations (>= 1) and after the last one.
 *   Stopping: phibar <= rel_tol * beta_b at a look, beta_b = sqrt(b.M^-1 b) (||b|| without a preconditioner; one more application at
 *   the set-up, and no dependence on x0), or max_iter iterations.  *iters = iterations run, *rel_resid = phibar / beta_b at the last
 *   look.  max_iter = k with rel_tol = 0 runs exactly k iterations.  b = 0: *iters = 0, *rel_resid = 0, x untouched.  A start within the
 *   tolerance, or max_iter = 0: no iteration, *rel_resid is that of x0.  An iteration that starts with phibar at or below the floor
 *   1e-14 beta_b passes quietly (its kernels write nothing), and the host ends the solve at its next look; beta = 0 - the Krylov space
 *   is exhausted and the iterate exact - gives phibar = 0 and ends the solve with SPMV_OK.
 *   SPMV_ERR_INVALID through the status word, naming the quantity and "at or before iteration k": r.M^-1 r below zero beyond rounding,
 *   that is below -(4 * 1e-14 beta_b)^2, in the start or in an iteration - "preconditioner is not positive definite (r.M^-1 r = ...)"
 *   (between that and zero it counts as 0); a non-finite b.b, b.M^-1 b, beta1, alfa, beta or phibar.  The kernel that sees it leaves
 *   x alone, so x holds an iterate of the recurrence.
 *   Refused before any device use with SPMV_ERR_INVALID: null ctx, A, b, x, iters or rel_resid, nrow != ncol, b or x with other than
 *   nrow entries, b and x overlapping, max_iter < 0, rel_tol < 0, a shift that is not finite, an unknown precond, a P of another size
 *   or context, P with SPMV_PRECOND_NONE, Jacobi on a CSR handle without its arrays.  nrow = 0: SPMV_OK, *iters = 0, nothing launched.
 *   Deterministic dot products (per-workgroup partial sums added in a fixed order by the workgroup that finishes last): a solve is
 *   exactly as reproducible as the product its handle runs.  x and b need only be 8-byte aligned; where they are 16-byte aligned the
 *   vector kernels use 16-byte accesses on them.
 *   Device memory: six work vectors of nrow doubles (a preconditioner: seven, Jacobi: eight), the partial sums of three quantities
 *   and a small scalar block for the duration of the call, released on every path. */
int spmv_minres(spmv_ctx* ctx, const spmv_mat* A, const spmv_mat* P, const spmv_vec* b, spmv_vec* x, double shift, int32_t max_iter,
                double rel_tol, int32_t check_every, int32_t precond, int32_t* iters, double* rel_resid);
/* Iterative refinement (solver_refine.hip): fp64 answers from a solver that runs on a cheaper handle.  A (any square
 *   handle) defines the system; A_lo (any handle of the same shape in the same context - a SPMV_FMT_CSR_F32 copy of A is the intended
 *   use; A_lo == A is allowed) is what the inner solver multiplies by.  From the x passed in, per outer step:
 *     r = b - A x with A's forward product and ||r||, both in fp64 (the deterministic dot of the solvers);
 *     stop if ||r|| <= rel_tol ||b||, or after max_outer steps, or if ||r|| is not below the smallest residual seen so far - then x
 *     goes back to the iterate of that smallest residual; else
 *     solve A_lo d = r from d = 0 with `solver` (SPMV_REFINE_CG: spmv_cg, SPMV_REFINE_BICGSTAB: spmv_bicgstab) to inner_tol within
 *     inner_max_iter iterations, check_every = 1, `precond` handed to that solver on A_lo exactly as it takes it (its refusals are
 *     this call's, made before the device is touched); an inner solve that runs out of iterations is no error, its d is used; an
 *     inner breakdown returns the inner solver's error;  x += d.
 *   SPMV_OK in all three stopping cases.  *outer = the steps that solved and updated, *inner_total = the inner iterations of all
 *   of them, *rel_resid = ||b - A x|| / ||b|| of the x returned - always written.  b = 0: x is untouched, the counts and the
 *   residual are 0 (spmv_cg's rule).  nrow = 0: likewise.
 *   Refused with SPMV_ERR_INVALID before any device use: null pointers, A not square, A_lo of another shape or another context,
 *   b or x of the wrong length, b and x overlapping, negative max_outer / inner_max_iter / inner_tol / rel_tol, an unknown solver.
 *   Synchronous.  Device memory for the duration of the call: three work vectors of nrow doubles (r, d, and the best iterate) on
 *   top of the inner solver's own, released on every path.  The handles' forward state (kernel, copies, plan) is left as it was;
 *   a preconditioner's state is built in A_lo as the inner solver builds it. */
enum
{
    SPMV_REFINE_CG       = 0,
    SPMV_REFINE_BICGSTAB = 1
};
int spmv_refine(spmv_ctx* ctx, const spmv_mat* A, const spmv_mat* A_lo, const spmv_vec* b, spmv_vec* x, int32_t solver, int32_t precond,
                int32_t max_outer, int32_t inner_max_iter, double inner_tol, double rel_tol, int32_t* outer, int32_t* inner_total,
                double* rel_resid);
/* Blocks: the dense tall-skinny arithmetic of a block method (block_ops.hip).  A BLOCK is p columns of n doubles held
 *   column-major in one spmv_vec: column c starts at entry c * ld, ld >= n, and the vector holds at least (p - 1) * ld + n entries.
 *   Rows n .. ld - 1 of a column are padding: never read, never written.  1 <= p, q <= 96 (SPMV_BLOCK_MAX_COLS) in both calls; blocks
 *   need only be 8-byte aligned.
 * spmv_block_gram: G = U^T V, p x q, row-major, into host memory; one sweep over the rows, every column read once (U and V the same
 *   block - same start, same ld, p = q - is read once altogether).  Synchronous.  Deterministic: no double is added in arrival order;
 *   per-workgroup partial sums are added in buffer order by the workgroup that finishes last, the grid depends on n alone, and two calls
 *   on the same data give the same bits.  With U = V the result is exactly symmetric (both triangles take the same additions; fma is
 *   commutative in its factors).  n = 0: all zeros, nothing is launched.
 * spmv_block_combine: Out[i, :] = S[i, :] C for every row i, C p x q row-major in host memory, Out a block of q columns.  Asynchronous
 *   (C_host may be reused on return: it is copied to pinned memory of the context and reaches the device through the stream).
 *   Out[i][j] starts from 0.0 and takes fma(S[i][k], C[k][j], .) for k = 0 .. p - 1 in that order: a function of the row alone.  Out may be
 *   S itself - the same start and the same ld; a row is read completely before any of it is written - and must not overlap it otherwise.
 * Refused on the host before any device use with SPMV_ERR_INVALID: null pointers (G_host, C_host among them), p or q outside 1 .. 96,
 *   n < 0, an ld below n, a vector too short for its block, Out overlapping S other than exactly in place. */
#define SPMV_BLOCK_MAX_COLS 96
int spmv_block_gram(spmv_ctx* ctx, int64_t n, int32_t p, const spmv_vec* U, int64_t ldu, int32_t q, const spmv_vec* V, int64_t ldv,
                    double* G_host);
int spmv_block_combine(spmv_ctx* ctx, int64_t n, int32_t p, const spmv_vec* S, int64_t lds, int32_t q, const double* C_host, spmv_vec* Out,
                       int64_t ldo);
/* spmv_lobpcg: the nev smallest (largest != 0: largest) eigenvalues of a symmetric A and their vectors by LOBPCG, Knyazev's locally
 *   optimal block preconditioned conjugate gradients, with a block of k >= nev vectors (solver_lobpcg.hip).  Synchronous.
 *   A is any handle spmv_bicgstab takes (all five formats, square); it is meant to be symmetric and nothing checks that.
 *   1 <= nev <= k <= 16 (SPMV_LOBPCG_MAX_K) and nrow >= 3 k.  X: nrow * k entries, column-major with ld = nrow; it holds the start
 *   block (for example spmv_gen_vec_uniform over nrow * k entries) and receives the vectors.  precond: spmv_gmres's set with the same
 *   refusals, applied column by column; it must be symmetric positive definite for the method to make sense.
 *   Algorithm, with the thresholds as constants of solver_lobpcg.hip (and of its NumPy twin, tests/lobpcg_ref.py):
 *   ORTHONORMALISE(B): G = B^T B; d = diag(G)^-1/2; d G d = L L^T; a pivot (the diagonal entry before its square root) below a
 *   threshold is rank loss; B <- B d L^-T.  RAYLEIGH-RITZ: the symmetric problem of the Gram matrices, solved on the host by cyclic
 *   Jacobi rotations (small_dense.hpp; no LAPACK).
 *   Start: orthonormalise X (threshold 1e-6, kLobpcgRankPivot; rank loss: SPMV_ERR_INVALID, "start block"); AX by k forward products
 *   through the handle's own kernel; Rayleigh-Ritz on X^T A X; X and AX rotated by its vectors.
 *   Iteration: (1) R = AX - X diag(theta) and resid_j = ||R_j||, one fused deterministic launch; (2) the host looks: active = the
 *   columns with resid_j > tol, every iteration anew; no active column among the first nev, or max_iter iterations run: stop;
 *   (3) W = M^-1 R_active; W -= X (X^T W), twice; orthonormalise W (rank loss: the first column that depends on those before it is
 *   left out of this iteration, and so on; no column left: SPMV_ERR_INVALID, and X, theta, resid hold the last iterate); AW by one
 *   product per column of W; (4) P, where it exists, is orthonormalised and AP transformed alike; rank loss
 *   drops P for this iteration; (5) S = [X P W], AS = [AX AP AW]; GB = S^T S and GA = S^T AS (symmetrised); GB's smallest pivot below
 *   1e-4 (kLobpcgBasisPivot) with P in use: the step is redone without P; (6) the host solves GA c = theta GB c and takes the k
 *   lowest (largest: highest) values and their vectors C; (7) X <- S C, AX <- AS C, P <- S C0[:, active], AP <- AS C0[:, active],
 *   C0 = C with the rows of X cleared.  GB is always computed: nothing rests on the blocks being orthonormal to rounding.
 *   Outputs: theta[k] ascending (largest: descending); resid[j] = ||A x_j - theta_j x_j||_2 of the returned unit vectors, an absolute
 *   number (a caller who wants a relative one divides by a norm estimate such as the Chebyshev row bound); *iters = iterations run.
 *   max_iter = 0 returns the Rayleigh-Ritz of the start block.  Reaching max_iter unconverged is SPMV_OK: the residuals tell.  nrow = 0
 *   (then k = nev = 1 .. 16 and an empty X): SPMV_OK, *iters = 0, nothing is launched.  A non-finite theta or residual:
 *   SPMV_ERR_INVALID naming the quantity.
 *   Refused before any device use with SPMV_ERR_INVALID: null pointers, nrow != ncol, k outside 1 .. 16, nev outside 1 .. k,
 *   0 < nrow < 3 k, X with other than nrow * k entries, max_iter < 0, tol < 0 or NaN, an unknown precond, Jacobi on a CSR handle
 *   without its arrays; SPMV_PRECOND_SYMGS and Jacobi on a non-CSR handle: SPMV_ERR_UNSUPPORTED.
 *   The handle's kernel, copies, plan and device_bytes stay as they were (a preconditioner that is set up on first use stays in the
 *   handle, as in the other solvers).  Deterministic: every sum over the rows is a fixed chain per workgroup and the workgroups' sums
 *   are added in buffer order; a solve is exactly as reproducible as the product its handle runs.
 *   Device memory: seven blocks of nrow x k doubles (S = [X P W] and AS = [AX AP AW] of 3 k columns each, R of k; a column a padded
 *   vector apart), nrow more for Jacobi, and the partial sums (512 x 9 k^2 doubles: 2.4 MB at k = 8), for the duration of the call, released on every path.  Per iteration
 *   with a active columns and P in use: a preconditioner applications and a products, 1 residual launch, 6 Gram launches (X^T W
 *   twice, W^T W, P^T P, S^T S, S^T AS) and 7 combine launches (W twice, W, P, AP, S, AS); the host looks six times (the residual
 *   norms and five Gram results: S^T S and S^T AS are read together). */
#define SPMV_LOBPCG_MAX_K 16
int spmv_lobpcg(spmv_ctx* ctx, const spmv_mat* A, int32_t k, int32_t nev, int32_t largest, spmv_vec* X, int32_t max_iter, double tol,
                int32_t precond, double* theta, double* resid, int32_t* iters);
/* spmv_symgs: `sweeps` symmetric Gauss-Seidel sweeps on A*x = b, x updated in place: forward over the rows in sweep
 *   order with the newest x, then backward — the sweep the reference's `diagonal // for SymGS` fields were reserved
 *   for (include/matrix.h:36,81) and that it never wrote.  A: CSR handle holding the whole square matrix with a non-zero
 *   diagonal (duplicates of a diagonal entry are summed); symmetric or not.
 *   Sweep order (spmv_mat_set_param "symgs_order", before the first use or between uses):
 *     1 (default) multicolour: the greedy colouring in row order (colour(i) = smallest colour no coupled row j < i has),
 *       rows swept colour by colour, ascending row index inside a colour — rows of a colour are solved together, a
 *       sweep is a handful of launches (two colours, 6 launches for a 7-point Laplacian);
 *     0 the matrix's own row order i = 0..n-1, exactly — as parallel as the matrix allows (the rows are solved in
 *       dependency levels: ~480 levels, ~790 launches for a 7-point Laplacian on 160^3 points; a band matrix is sequential).
 *   spmv_symgs_order returns the sequence (order[k] = the k-th row of a forward sweep), so that a host implementation can
 *   repeat the sweep number by number.  Either way the result is exact for that order (only the sums inside a row are
 *   taken by several lanes).
 *   spmv_symgs_setup (also run by the first spmv_symgs / spmv_cg(SPMV_PRECOND_SYMGS) on the handle): colours the rows,
 *   splits A into L + D + U by sweep order on the device, finds the dependency levels of both parts and fixes a launch
 *   schedule; synchronous; kept in the handle (about the size of the matrix again).  A sweep is then t = b - U*x,
 *   (L+D)*x = t level by level, t = b - L*x, (D+U)*x = t level by level — asynchronous.  spmv_mat_get_param
 *   "symgs_colours" / "symgs_levels_forward" / "symgs_levels_backward" / "symgs_launches" (per sweep) / "symgs_bytes".
 *   SPMV_ERR_UNSUPPORTED if a dependency chain exceeds 2^18 rows. */
int spmv_symgs_setup(spmv_ctx* ctx, spmv_mat* A);
int spmv_symgs_order(spmv_ctx* ctx, const spmv_mat* A, int32_t* order /* host, nrow entries */);
int spmv_symgs(spmv_ctx* ctx, spmv_mat* A, const spmv_vec* b, spmv_vec* x, int32_t sweeps);
/* ILU(0): the incomplete LU factorisation without fill of a CSR handle, computed on the device, and z = U^-1 L^-1 r by two
 *   level-scheduled triangular solves (ilu0.hip).  A: a CSR handle that holds the whole square matrix and still has
 *   its arrays; symmetric or not; every row needs a stored diagonal entry.
 *   Definition.  pos[i] is the position of row i in the sweep order - spmv_mat_set_param "ilu0_order": 1 (default) the multicolour
 *   order of spmv_symgs (the same greedy colouring, colour by colour, ascending row index inside a colour), 0 the matrix's own row
 *   order.  The pattern P is the set of (i, j) with at least one stored entry; duplicates are summed first.  The factors are those
 *   of the IKJ elimination restricted to P, rows taken in sweep order:  for k in row i with pos[k] < pos[i], ascending pos[k]:
 *   l_ik = a_ik / u_kk;  for j in row k with pos[j] > pos[k] and (i, j) in P:  a_ij = fma(-l_ik, u_kj, a_ij);  then u_ij = a_ij for
 *   pos[j] >= pos[i].  L is unit lower triangular in sweep order, U upper triangular with the diagonal.  Every entry receives its
 *   subtractions in ascending pos[k]: two set-ups of one matrix give the same bits, and two applications the same z.
 *   spmv_ilu0_setup: order, symbolic set-up (a working copy with every row sorted by pos and split into L, D, U; dependency levels
 *   and launch schedules of both triangles) and the numeric factorisation, level by level.  Synchronous, idempotent; rebuilds when
 *   "ilu0_order" changed since.  A row without a diagonal entry, or a pivot that is zero or not finite: SPMV_ERR_INVALID - the
 *   message names the offending row with the smallest sweep position - and nothing is left in the handle.  SPMV_ERR_UNSUPPORTED
 *   if a dependency chain exceeds 2^18 rows.  Re-factorising after the values of a wrapped handle changed is not offered.
 *   spmv_ilu0_solve: z = U^-1 L^-1 r, asynchronous; vectors in the matrix's own numbering; r and z must not overlap.  Sets the
 *   handle up on first use although it is passed as const.  One launch per large level, one workgroup per run of small levels.
 *   spmv_ilu0_factors: the factor values aligned to the handle's own nnz entries, as an in-place csrilu0 would leave them: l_ik in
 *   the entries of L, u_ij in the diagonal and upper ones; of a set of duplicates the first stored one carries the value, the
 *   others hold 0.0.  spmv_ilu0_order: order[k] = the k-th row of the sweep (nrow entries).  Both set the handle up if need be.
 *   Refused on the host, before any device use: a handle that is not CSR (SPMV_ERR_UNSUPPORTED); a shard or a non-square matrix, a
 *   handle whose arrays were released (panel_keep_csr 0), null pointers, vectors of other than nrow entries, another context's
 *   handle (SPMV_ERR_INVALID).  nrow = 0: SPMV_OK, nothing is launched.
 *   The state lives in the handle (spmv_mat_get_param "ilu0_ready", "ilu0_colours", "ilu0_levels_forward", "ilu0_levels_backward",
 *   "ilu0_launches" per application, "ilu0_bytes", "ilu0_order"), is counted in device_bytes and freed with the handle; the forward
 *   kernel, the copies, the transposed state and the plan stay as they were. */
int spmv_ilu0_setup(spmv_ctx* ctx, spmv_mat* A);
int spmv_ilu0_solve(spmv_ctx* ctx, const spmv_mat* A, const spmv_vec* r, spmv_vec* z);
int spmv_ilu0_factors(spmv_ctx* ctx, const spmv_mat* A, double* values_host /* nnz entries */);
int spmv_ilu0_order(spmv_ctx* ctx, const spmv_mat* A, int32_t* order_host /* nrow entries */);

/* Sparse triangular solves with a matrix the caller supplies: x = op(T)^-1 b for one right-hand side or k of them, by level
 *   scheduling (sptrsv.hip).  A: a CSR handle that holds the whole square matrix and still has its arrays - a Cholesky,
 *   IC, ILUT or ILU(k) factor computed elsewhere, a triangular operator, or the combined LU array of spmv_ilu0_factors uploaded on
 *   A's own pattern.
 *   Definition.  flags selects T: SPMV_TRSV_LOWER the entries with column < row, SPMV_TRSV_UPPER those with column > row, plus the
 *   diagonal; entries of the other triangle are ignored, not refused.  Duplicates of the diagonal entry are summed; every other
 *   stored entry, duplicates and stored zeros included, is a term of its own; columns may be unsorted and the order inside a row is
 *   kept.  SPMV_TRSV_UNIT: the diagonal is 1 and stored diagonal entries are ignored.  SPMV_TRSV_TRANSPOSE: op(T) = T^T, solved
 *   from a transposed working copy whose rows hold their entries in ascending column index (duplicates in stored order).
 *   spmv_trsv_setup: a working copy of the selected triangle, its dependency levels, rows by level and the launch schedule
 *   (tri_levels.hpp, as spmv_ilu0_setup's triangles).  Synchronous, idempotent.  A handle holds one analysis per (uplo, transpose)
 *   pair, up to four; UNIT and non-UNIT solves share it.  Without UNIT: a diagonal entry that is missing, zero or not finite is
 *   SPMV_ERR_INVALID, the message names the smallest such row, and the call leaves nothing in the handle that was not there before
 *   (the same handle still solves with UNIT).  SPMV_ERR_UNSUPPORTED if a dependency chain exceeds 2^18 rows.  Re-analysis after the
 *   values of a wrapped handle changed is not offered.
 *   spmv_trsv_solve: x = op(T)^-1 b, asynchronous; sets the handle up on first use although it is passed as const.  b and x may be
 *   the SAME vector (a row reads b at its own index only, before it writes x there); otherwise they must not overlap.  1, 4 or 16
 *   lanes share a row (by the triangle's entries per row) and their partial sums meet in a fixed tree: two solves give the same bits.
 *   spmv_trsv_solve_multi: the same for k right-hand sides, 1 <= k <= 64, B and X row-major n x k (the layout of spmv_apply_multi),
 *   in the launches of ONE solve: a group of T lanes owns a row (T the next power of two >= min(k, 16)), lane t its column t of every
 *   tile of 16 columns.  Order contract: for every column a row's sum runs left to right over the working copy's entries from 0.0 with
 *   fma, then x = b - acc (UNIT) or (b - acc) / d.  Column c of a k-column solve is therefore bit-identical to a k = 1 solve of that
 *   column, for every k, and to spmv_trsv_solve wherever spmv_trsv_info reports 1 lane.  B and X may be the same vector.
 *   spmv_trsv_info: levels, lanes per row and launches per spmv_trsv_solve of the analysis `flags` selects, and its device bytes;
 *   any output may be null; SPMV_ERR_INVALID where that analysis is not there.
 *   Refused on the host, before any device use: a handle that is not CSR (SPMV_ERR_UNSUPPORTED); a shard or a non-square matrix, a
 *   handle whose arrays were released (panel_keep_csr 0), null pointers, unknown flag bits, vectors of other than nrow (nrow * k)
 *   entries, k outside 1 .. 64, vectors that overlap in part, another context's handle (SPMV_ERR_INVALID).  nrow = 0: SPMV_OK,
 *   nothing is launched.
 *   The state lives in the handle (spmv_mat_get_param "trsv_ready": bit (upper ? 1 : 0) | (transpose ? 2 : 0) of every analysis
 *   present; "trsv_bytes"; "trsv_multi_launches" and "trsv_multi_level_launches": the launches of the last spmv_trsv_solve_multi,
 *   all of them and those that were a level of their own), is counted in device_bytes and freed with the handle; the forward kernel,
 *   the copies, the plan and the symgs, ILU(0) and transposed states stay as they were. */
#define SPMV_TRSV_LOWER     0u
#define SPMV_TRSV_UPPER     1u
#define SPMV_TRSV_UNIT      2u /* the diagonal is 1; stored diagonal entries are ignored */
#define SPMV_TRSV_TRANSPOSE 4u /* solve with the transpose of the selected triangle */
int spmv_trsv_setup(spmv_ctx* ctx, spmv_mat* A, uint32_t flags);
int spmv_trsv_solve(spmv_ctx* ctx, const spmv_mat* A, uint32_t flags, const spmv_vec* b, spmv_vec* x);
int spmv_trsv_solve_multi(spmv_ctx* ctx, const spmv_mat* A, uint32_t flags, int32_t k, const spmv_vec* B, spmv_vec* X);
int spmv_trsv_info(const spmv_mat* A, uint32_t flags, int32_t* levels, int32_t* lanes, int32_t* launches, int64_t* bytes);

/* The Chebyshev polynomial preconditioner / smoother, and the Lanczos estimate of a symmetric handle's extreme eigenvalues
 * (chebyshev.hip).  A: a handle of any format that holds the whole square matrix (a shard that starts behind row 0:
 * SPMV_ERR_INVALID).
 *
 *   Definition.  degree d in 1 .. 64 (the products per application); s_i = 1 / a_ii where `scaled` (the diagonal as
 *   SPMV_PRECOND_JACOBI reads it from a CSR handle that still has its arrays, duplicates summed; a zero or missing entry:
 *   SPMV_ERR_INVALID), s_i = 1 otherwise; B = diag(s) A; 0 < lmin < lmax.  On the host, in double, every line one rounded operation:
 *       theta = (lmax + lmin) / 2;  delta = (lmax - lmin) / 2;  sigma = theta / delta;  rho_0 = 1 / sigma;  c0 = 1 / theta
 *       for k = 1..d:  rho_k = 1 / (2 sigma - rho_{k-1});  c1_k = rho_k rho_{k-1};  c2_k = 2 rho_k / delta
 *   (spmv_chebyshev_coefficients returns this table; it touches no device).  The application z = M^-1 r leaves r as it is:
 *       d = c0 (s .* r);  z = d;  t = r;      for k = 1..d:  w = A d;  t = t - w;  d = c1_k d + c2_k (s .* t);  z = z + d
 *   that is z = p_d(B) diag(s) r; the start and the d terms are d + 1 corrections of the Chebyshev iteration, so p_d has degree d
 *   and 1 - lambda p_d(lambda) = T_{d+1}((theta - lambda) / delta) / T_{d+1}(sigma): one application contracts the error of a
 *   symmetric system by at most 1 / T_{d+1}(sigma) where the bounds hold.  M^-1 is symmetric
 *   positive definite whenever A is and lmax is at or above B's largest eigenvalue: a legitimate preconditioner of spmv_cg.  An lmax
 *   that is too small shows as r.M^-1 r <= 0, which spmv_cg reports.  2 d + 1 launches per application ("cheby_launches"): one
 *   start, and per term the handle's forward product and ONE pass over the vectors; no dot product, no look by the host.
 *
 *   spmv_chebyshev_setup (synchronous; replaces earlier state).  lmax = 0: estimated.  A CSR handle that still has its arrays takes
 *   the row bound max_i |s_i| sum_j |a_ij| over every stored entry - the infinity norm of B, a RIGOROUS upper bound of every
 *   |lambda|.  Where spmv_mat_set_param "cheby_lanczos_steps" is above 0 (default 0) it also takes 1.05 times the largest Ritz value
 *   of that many steps of spmv_lanczos (seed 1) and keeps the smaller of the two, or the Lanczos value alone on a handle without CSR
 *   arrays.  A Ritz value is a LOWER estimate of the largest eigenvalue; the factor 1.05 (what Ifpack2 and hypre put on their
 *   power-method estimates) usually covers the difference and guarantees nothing.  Neither source: SPMV_ERR_UNSUPPORTED.
 *   lmin = 0: lmax / "cheby_ratio" (default 30, the smoother default of the same libraries; 2 .. 10^6).  SPMV_ERR_INVALID: a
 *   negative or non-finite bound, lmin >= lmax, degree outside 1 .. 64, a matrix that is not square or a shard that starts behind
 *   row 0, `scaled` on a handle that is not CSR with its arrays.  Explicit bounds with scaled = 0: any format.  nrow = 0: SPMV_OK.
 *   spmv_chebyshev_info: what the state holds; not set up: degree 0.
 *
 *   spmv_chebyshev_solve: z = M^-1 r, asynchronous; r and z must not overlap; the handle must be set up.
 *   spmv_chebyshev: x += M^-1 (b - A x), one smoothing step (one product more), asynchronous; b and x must not overlap.
 *
 *   spmv_lanczos (synchronous): `steps` (1 .. 64) steps of the Lanczos recurrence without reorthogonalisation on
 *   C = diag(sqrt s) A diag(sqrt s), which has B's spectrum (scaled: every a_ii > 0, else SPMV_ERR_INVALID; unscaled: A itself),
 *   from v_0 = spmv_gen_vec_uniform(seed) normalised.  One product and two launches per step, every sum deterministic, alpha and
 *   beta on the device until the end.  beta_{j+1} at or below 2^-44 max(|alpha|, beta) seen so far is an invariant subspace and
 *   ends the run quietly (steps_done < steps).  Returns the smallest and the largest eigenvalue of the steps_done x steps_done
 *   tridiagonal matrix (bisection on the Sturm count, to 2 ulp of the largest |value|) and, where asked for, alpha_j and
 *   beta_{j+1}, j = 0 .. steps_done - 1.  A is meant to be symmetric; nothing checks it.
 *
 *   The state lives in the handle (spmv_mat_get_param "cheby_ready", "cheby_degree", "cheby_bytes", "cheby_launches",
 *   "cheby_lanczos_steps", "cheby_ratio", "cheby_lmax_source": 0 the caller's, 1 the row bound, 2 Lanczos): degree, bounds, the
 *   table, s where scaled and three work vectors; it is counted in device_bytes and freed with the handle, and is no part of the
 *   forward state, of plans or of trials. */
int spmv_chebyshev_coefficients(int32_t degree, double lmin, double lmax, double* c0, double* c1 /* degree */, double* c2 /* degree */);
int spmv_lanczos(spmv_ctx* ctx, const spmv_mat* A, int32_t scaled, int32_t steps, uint64_t seed, double* ritz_min, double* ritz_max,
                 double* alpha /* steps entries or NULL */, double* beta /* steps entries or NULL */, int32_t* steps_done);
int spmv_chebyshev_setup(spmv_ctx* ctx, spmv_mat* A, int32_t degree, int32_t scaled, double lmin, double lmax);
int spmv_chebyshev_info(const spmv_mat* A, int32_t* degree, int32_t* scaled, double* lmin, double* lmax);
int spmv_chebyshev_solve(spmv_ctx* ctx, const spmv_mat* A, const spmv_vec* r, spmv_vec* z);
int spmv_chebyshev(spmv_ctx* ctx, spmv_mat* A, const spmv_vec* b, spmv_vec* x);

/* ---- aggregation algebraic multigrid (amg.hip) -----------------------------------------------------------------------
 * spmv_amg_setup builds a hierarchy on the device from a CSR handle (square, the whole matrix, arrays kept: the rules of
 *   spmv_ilu0_setup, checked on the host before any device use) and spmv_amg_solve applies one V(1,1) cycle z = B r.  Synchronous;
 *   replaces earlier state; a failed set-up leaves the earlier state.  An argument of 0 takes its default:
 *     max_levels 1 .. 32 (16);  coarse_max 1 .. 1024 (256);  smooth_degree 1 .. 64 (2);  strength theta, <= 0 (default): every stored
 *     off-diagonal entry is a neighbour, > 0: j is a neighbour of i iff a_ij^2 >= theta^2 |a_ii a_jj|;  overcorrection omega inside
 *     (0, 2) (1.5).  Anything else: SPMV_ERR_INVALID.
 *   The method.  Level 0 is the handle's arrays.  Every row needs a stored non-zero diagonal entry (duplicates summed), else
 *   SPMV_ERR_INVALID.  Rows are aggregated by a maximal independent set of distance 2 over the rows' own neighbour lists (nothing is
 *   symmetrised): the priority of row i is the pair (h(i), i) compared as unsigned numbers, h the 32-bit finaliser h ^= h >> 16;
 *   h *= 0x85ebca6b; h ^= h >> 13; h *= 0xc2b2ae35; h ^= h >> 16 of i; in a round every undecided row whose priority is the largest
 *   among the undecided rows within two steps becomes a root and the undecided rows within two steps of a root are removed, until no
 *   row is undecided.  Roots take ids in ascending row order; a row with roots among its neighbours joins the one of smallest id;
 *   every other row joins the smallest id among its neighbours as that pass left them.  The coarse operator is
 *   A_c[I, J] = sum of a_ij over all stored entries with agg(i) = I, agg(j) = J, added from 0.0 in ascending (I, J, entry) order: the
 *   result does not depend on the order of the launches.  Level l is the coarsest when n_l <= coarse_max, l + 1 == max_levels, or the
 *   next level would hold more than 0.8 n_l rows.  Every level is smoothed by the Chebyshev polynomial of spmv_chebyshev_setup(degree =
 *   smooth_degree, scaled, estimated bounds: the row bound, ratio 30); level 0's is the HANDLE'S OWN Chebyshev state, which
 *   spmv_amg_setup replaces as spmv_chebyshev_setup would.  A coarsest level of at most 1024 rows is inverted densely on the host (LU
 *   with partial pivoting in double; a pivot below 2^-44 of the largest entry: SPMV_ERR_INVALID, "singular coarsest operator") and
 *   applied by one launch; a larger one takes one Chebyshev application.  The cycle on level l with right-hand side b_l:
 *     x_l = M_l^-1 b_l;  b_{l+1}[I] = sum over i in I, ascending, of (b_l - A_l x_l)[i];  x_{l+1} = cycle(l + 1);
 *     x_l[i] += omega x_{l+1}[agg(i)];  x_l += M_l^-1 (b_l - A_l x_l)
 *   B is symmetric positive definite for a symmetric positive definite A and 0 < omega < 2, so spmv_cg may use it.  r is never
 *   written; r and z must not overlap; asynchronous, nothing is allocated or read back; results are deterministic.
 * spmv_amg_info: the number of levels and, where the pointers are not NULL, rows and entries per level (arrays of at least 32).
 * spmv_amg_level: to the host, the aggregate of every row of `level` (NULL, or an array of rows[level]; the coarsest level has none:
 *   SPMV_ERR_INVALID) and the operator of `level` as CSR (NULLs, or arrays of rows + 1, entries, entries).
 * spmv_amg_solve, spmv_amg_level and spmv_amg_info on a handle that was not set up: SPMV_ERR_INVALID.
 * spmv_mat_get_param: "amg_ready", "amg_levels", "amg_bytes" (counted in device_bytes), "amg_launches" (per application: 4 d + 7 a
 *   level and 1 or 2 d + 1 at the coarsest), "amg_mis_rounds" (summed over the levels), "amg_smoothed" (below).  spmv_mat_set_param "amg_level_kernel": a CSR
 *   kernel id forced on every coarse handle of the next set-up (0, the default: each selects its own).  A forced id that a coarse
 *   operator cannot run - the LDS-window kernel where a block of 256 rows spans more columns than its tile holds - fails the set-up
 *   with SPMV_ERR_UNSUPPORTED (the message names the level, the id, the window and the capacity), leaving the earlier state.  The
 *   hierarchy's bits do not depend on the id.  The application is bit-reproducible from call to call and from set-up to set-up under
 *   the six ids whose kernels store every y_i once (VECTOR, LDSWIN, SCALAR, PANEL, TWOPHASE, ELL; PANEL and TWOPHASE within what "Order
 *   of the additions" above says of their LDS sums) where level 0 runs one of them too; it is not promised to be under SEGSCAN and
 *   SPLIT (atomic adds on y in arrival order), nor under 0: every coarse handle then selects as any handle does, from 64K entries on
 *   by a timed trial that may pick any of the eight.  The state is freed with the handle and is no part of plans, trials, copies or
 *   the transposed state. */
int spmv_amg_setup(spmv_ctx* ctx, spmv_mat* A, int32_t max_levels, int32_t coarse_max, int32_t smooth_degree, double strength,
                   double overcorrection);
int spmv_amg_info(const spmv_mat* A, int32_t* levels, int64_t* rows /* levels, or NULL */, int64_t* nnz /* levels, or NULL */);
int spmv_amg_level(spmv_ctx* ctx, const spmv_mat* A, int32_t level, int32_t* agg_host /* rows[level], or NULL */, int32_t* row_ptr,
                   int32_t* col, double* val /* the operator of `level`, or NULLs */);
int spmv_amg_solve(spmv_ctx* ctx, const spmv_mat* A, const spmv_vec* r, spmv_vec* z);

/* ---- smoothed aggregation (amg.hip) -------------------------------------------------------------------------------------
 * spmv_amg_setup_smoothed builds the hierarchy of spmv_amg_setup with smoothed prolongators: the same rules, refusals, stop rules,
 *   aggregates and "a failed set-up leaves the earlier state"; an argument of 0 takes its default, which here is 1.0 for
 *   overcorrection (inside (0, 2)) and 4/3 for prolong_damping (inside (0, 2); NaN or outside: SPMV_ERR_INVALID on the host, before
 *   any device use).  It replaces whatever AMG state the handle holds; a later spmv_amg_setup replaces it with a plain one.
 *   The method, on level l with agg and the strength mask of spmv_amg_setup:
 *     A^F  theta <= 0: the level's own arrays.  theta > 0: row i holds, in stored order, every stored diagonal entry and every entry
 *          the mask calls a neighbour; a row with at least one weak off-diagonal entry ends on one more entry (i, i), the sum of its
 *          weak values from 0.0, left to right.
 *     d_i  the sum of the diagonal entries of row i of A^F in stored order; a zero d_i: SPMV_ERR_INVALID, the message names the level.
 *     lam  max_i |1 / d_i| sum_j |A^F_ij| over every stored entry (the row bound of spmv_chebyshev_setup; for theta <= 0 the lmax
 *          of the level's smoother).
 *     T    n x nc, one entry 1.0 at (i, agg(i)).
 *     P    AT = spmv_spgemm(A^F, T) (every row i holds column agg(i): the diagonal is stored); g = prolong_damping / lam on the host;
 *          c_i = g / d_i; P[i, J] = e - c_i AT[i, J] with e = 1.0 where J = agg(i) and 0.0 elsewhere: the product rounded once,
 *          then a plain subtraction, no fma.  P has AT's pattern (ascending columns; an entry that comes out 0.0 stays).
 *     R    spmv_csr_transpose(P);  A_{l+1} = spmv_spgemm(R, spmv_spgemm(A_l, P)) with the full A_l, selected or forced
 *          ("amg_level_kernel", the refused LDS window included) as the coarse operators of spmv_amg_setup are.
 *   spmv_spgemm defines every sum and the row bound is a maximum: the hierarchy is defined bit for bit.  The cycle is that of
 *   spmv_amg_setup with b_{l+1} = R (b_l - A_l x_l) and x_l += omega P x_{l+1}, each one launch (a group of 2^k lanes a row, the
 *   entries of a lane left to right, a fixed tree: no atomics, equal bits from call to call): "amg_launches" keeps its formula.  R
 *   is P^T exactly, so B stays symmetric positive definite for such an A.  P and R persist per level; T, A^F and A P are freed
 *   before the next level is built.  spmv_amg_solve and SPMV_PRECOND_AMG apply the state as it stands; spmv_amg_info and
 *   spmv_amg_level work unchanged (aggregates on every level but the coarsest).  Measured: about a third to half
 *   the iterations of the plain hierarchy on large Laplacians at the same cost of a cycle and 2 - 3 times the set-up and the
 *   state; on a large convection-dominated (first-order upwind) system the smoothed cycle did not converge where the plain one
 *   does - R = P^T smooths the restriction with A, not A^T - so spmv_amg_setup stays the one for those.
 * spmv_amg_prolongator: to the host, the entries of P of `level` in *nnz and, where the pointers are not NULL, P as CSR (arrays of
 *   rows[level] + 1, *nnz, *nnz: ask for nnz alone first).  A plain state, the coarsest level, a handle that was not set up:
 *   SPMV_ERR_INVALID.
 * spmv_mat_get_param: "amg_smoothed" (1 under a smoothed state, else 0); "amg_bytes" counts the P and R handles of every level (and
 *   no member lists: the restriction runs over R). */
int spmv_amg_setup_smoothed(spmv_ctx* ctx, spmv_mat* A, int32_t max_levels, int32_t coarse_max, int32_t smooth_degree, double strength,
                            double overcorrection, double prolong_damping);
int spmv_amg_prolongator(spmv_ctx* ctx, const spmv_mat* A, int32_t level, int64_t* nnz, int32_t* row_ptr, int32_t* col,
                         double* val /* P of `level`, or NULLs */);
/* spmv_amg_transfer_timed: for measurements (tools/bench_amg.py) - one transfer of `level` of a smoothed state by itself,
 *   `reps` times between two events, milliseconds per call.  v has rows[level] entries: the right-hand side b of a restriction (read;
 *   w and the result are the level's own vectors) or the x of a prolongation (added into).  what: the cycle's fused kernel
 *   (RESTRICT_FUSED, PROLONG_FUSED; lanes 0: the lanes the set-up chose, "amg_lanes_r<level>" / "amg_lanes_p<level>" of
 *   spmv_mat_get_param, else a power of two in 1 .. 64) or the same step as a vector pass and a product through the handle of R or P
 *   (RESTRICT_UNFUSED: t = b - w, then R t; PROLONG_UNFUSED: t = P x_c, then x += omega t).  A plain state, the coarsest level, a
 *   vector of another length: SPMV_ERR_INVALID on the host. */
enum
{
    SPMV_AMG_RESTRICT_FUSED   = 0,
    SPMV_AMG_RESTRICT_UNFUSED = 1,
    SPMV_AMG_PROLONG_FUSED    = 2,
    SPMV_AMG_PROLONG_UNFUSED  = 3
};
int spmv_amg_transfer_timed(spmv_ctx* ctx, const spmv_mat* A, int32_t level, int32_t what, int32_t lanes, spmv_vec* v, int32_t reps,
                            double* ms_per_call);

/* ---- FSAI: a factorised sparse approximate inverse applied by two products (fsai.hip) ---------------------------------
 * For a symmetric positive definite A, a sparse lower-triangular G with G A G^T ~ I (Kolotilina-Yeremin); the preconditioner is
 * z = G^T (G r).  Handles: those of spmv_ilu0_setup - a CSR handle (BSR and every other format: SPMV_ERR_UNSUPPORTED) holding the whole
 * square matrix, of this context, with its arrays (a shard, a rectangle, another context's handle, arrays released by
 * panel_keep_csr = 0: SPMV_ERR_INVALID) - checked on the host before any device use.  n = 0: SPMV_OK, nothing is launched.
 *
 *   Pattern.  S is the lower triangle, diagonal included, of the structural pattern of A^level, level 1, 2 or 3.  Every stored entry
 *   counts, zeros included.  Each row of S holds distinct columns in ascending order, and its last column is the row itself: a row
 *   without a stored diagonal entry is SPMV_ERR_INVALID naming the (smallest such) row.  Level 1 is tril(A) with duplicates merged;
 *   levels 2 and 3 come from spmv_spgemm's structural pattern (A A, then (A A) A) cut to the lower triangle on the device.
 *   Row i, with J = S_i and m = |J|.  M = A[J, J], of which only the LOWER triangle of A is read: entry (p, q), q <= p, is the sum of
 *   the stored entries (J_p, J_q) of row J_p of A, from 0.0, duplicates in stored order.  Symmetry is NOT checked, as in any Cholesky
 *   routine: the upper triangle of A is never looked at.  M = C C^T (right-looking: c_kk = sqrt(m_kk), c_pk = m_pk / c_kk, then
 *   m_pq = fma(-c_pk, c_qk, m_pq) for k < q <= p); row i of G is the solution g of C^T g = e_m, from the last unknown up
 *   (g_p = t_p / c_pp, then t_a = fma(-c_pa, g_p, t_a) for a < p), so g_ii = 1 / c_mm.  A pivot m_kk that is not finite or not
 *   positive is SPMV_ERR_INVALID: the message names the smallest such row, and nothing is left in the handle.
 *   Cap.  m <= 64.  A longer row is SPMV_ERR_UNSUPPORTED; the message names the first such row, its m and the cap, and the state of
 *   an earlier set-up stays in the handle (a missing diagonal entry or a bad pivot leave none).
 *   Application.  z = G^T (G r): G and G^T are two internal CSR handles, G^T built by the path of spmv_csr_transpose, each with its
 *   own AUTO kernel choice ("panel_trial" of A holds for both); two product launches that overwrite their outputs, one work vector
 *   of n.  Two set-ups give the same bits of G; two applications of one state give the same bits of z, and so do two states whose
 *   handles chose the same kernels (always, where the choice is the model's: below 65,536 entries, or under "panel_trial" 0).
 *
 * spmv_fsai_setup: synchronous; level 0 means the handle's "fsai_level"; anything outside 0 .. 3 is SPMV_ERR_INVALID on the host.
 *   Called again, it rebuilds.  spmv_fsai_solve: asynchronous; r and z overlapping, wrong lengths or a handle that was not set up:
 *   SPMV_ERR_INVALID on the host.  spmv_fsai_info: level, entries of G and the longest row of a state.  spmv_fsai_factor: to the host,
 *   the entries of G in *nnz and, where the pointers are not NULL, G as CSR (arrays of nrow + 1, *nnz, *nnz: ask for nnz alone first).
 * spmv_mat_get_param: "fsai_level" (what a solver's own set-up takes), "fsai_ready", "fsai_bytes" (both handles and the work vector;
 *   NOT counted in device_bytes), "fsai_max_row", and the wall time of the last set-up in microseconds by phase: "fsai_setup_us_pattern"
 *   (the sparse products, the cut, G's offsets and columns), "fsai_setup_us_rows" (the row kernel), "fsai_setup_us_handles" (the analysis
 *   of G, the transpose and its analysis).  The state is no part of the forward state, of plans, trials, copies or the
 *   transposed state, and is freed with the handle.
 * Not built here: thresholded or adaptive patterns, rows truncated at the cap, a two-factor variant for nonsymmetric matrices, FSAI as
 *   an AMG smoother, FSAI under spmv_cg_multi or the sharded solver (both possible, since the application is products only). */
#define SPMV_FSAI_MAX_ROW 64
int spmv_fsai_setup(spmv_ctx* ctx, spmv_mat* A, int32_t level);
int spmv_fsai_solve(spmv_ctx* ctx, const spmv_mat* A, const spmv_vec* r, spmv_vec* z);
int spmv_fsai_info(const spmv_mat* A, int32_t* level, int64_t* nnz, int32_t* max_row);
int spmv_fsai_factor(spmv_ctx* ctx, const spmv_mat* A, int64_t* nnz, int32_t* row_ptr, int32_t* col, double* val /* G, or NULLs */);

/* ---- sparse products on the device (spgemm.hip) ------------------------------------------------------------------------
 * spmv_spgemm: C = A B for two CSR handles of one context, A m x k and B k x n, both whole matrices (row_begin 0) that still hold
 *   their arrays.  The inputs may hold unsorted columns, duplicate entries and stored zeros.  Synchronous; *out_C is an owning CSR
 *   handle like any other: products, solvers, set-ups, spmv_mat_download, spmv_mat_validate, and an input of another spmv_spgemm.
 *   It selects its kernel as an uploaded handle does (a plan of the context is not applied to it).
 *   Pattern: C holds exactly one entry (i, j) for every pair that at least one stored a_ip and stored b_pj reach.  The pattern is
 *     structural: stored zeros and sums that cancel still give an entry.  Columns ascend strictly inside a row.
 *   Value: the scalar products of row i are taken in the order (position of the A entry in row i as stored, then position of the B
 *     entry in its row as stored).  Each is t = a * b, rounded once; c_ij is the sum of its t, from 0.0, left to right in that order,
 *     in plain additions - no fma, no atomics on doubles, nothing reassociated.  Every method and every run returns the same bytes.
 *   Empty: an empty row of A, or one that reaches only empty rows of B, is an empty row of C; nnz(C) = 0 is a valid result; m, k or
 *     n = 0 are allowed as spmv_csr_upload allows them.
 *   method: SPMV_SPGEMM_ROWS - a row of up to 2048 scalar products is expanded, sorted and added up in LDS by 16 lanes, a wavefront
 *     or a workgroup (by its number of products); longer rows go through SORT in one batch.  SPMV_SPGEMM_SORT - every row is
 *     expanded into global memory, ordered by two stable radix passes and added up run by run (40 bytes of transient memory per
 *     scalar product).  SPMV_SPGEMM_AUTO - ROWS.
 *   Refused on the host, before any device use: a null argument, a shard, released CSR arrays (panel_keep_csr = 0), a handle of
 *     another context, A->ncol != B->nrow, a method outside 0 .. 2 (SPMV_ERR_INVALID); a handle that is not CSR
 *     (SPMV_ERR_UNSUPPORTED).  After counting on the device: more than 2^31 - 1 entries in C, or more than 2^31 - 1 scalar products
 *     on the sort path, whose ids are int32 (SPMV_ERR_UNSUPPORTED; the message names the count).  A failure frees what it
 *     allocated and leaves *out_C untouched.
 *   spmv_mat_get_param on the result: "spgemm_products" (scalar products formed), "spgemm_rows_lds" / "spgemm_rows_sorted" (non-empty
 *     rows per path), "spgemm_lds_products" (the largest row, in scalar products, that the LDS path takes: 2048),
 *     "spgemm_transient_bytes" (device memory the call held beside C and the radix sort's own buffers).  0 on any other handle.
 * spmv_csr_transpose: the n x m CSR handle of A^T.  Row j holds the entries of column j of A in ascending row i; entries with equal
 *   (j, i) keep A's stored order; duplicates are kept, not summed; values are copied bit for bit.  Same refusals as above. */
enum
{
    SPMV_SPGEMM_AUTO = 0,
    SPMV_SPGEMM_ROWS = 1,
    SPMV_SPGEMM_SORT = 2
};
int spmv_spgemm(spmv_ctx* ctx, const spmv_mat* A, const spmv_mat* B, int32_t method, spmv_mat** out_C);
int spmv_csr_transpose(spmv_ctx* ctx, const spmv_mat* A, spmv_mat** out_At);

/* ---- reordering (reorder.hip) ------------------------------------------------------------------------------------------
 * A permutation is an object of a context: n, and order and inverse on the device (8 n bytes).  The convention is that of
 *   spmv_symgs_order: order[k] is the old index that takes new position k, and inverse[order[k]] = k.
 * spmv_perm_create: uploads order_host[n] and builds the inverse on the device.  Synchronous.  Anything that is not a permutation of
 *   0 .. n-1 is refused with SPMV_ERR_INVALID; the message names the smallest position k whose value is out of range or stands at an
 *   earlier position already.  n = 0 is valid (order_host may be NULL) and touches no device.
 * spmv_perm_rcm: the reverse Cuthill-McKee ordering of a square CSR handle (the whole matrix, arrays still held), computed on the
 *   device.  Synchronous; only order and inverse stay allocated when it returns.
 *   Graph: vertices 0 .. n-1; i ~ j for i != j if (i, j) or (j, i) is stored - the pattern of A + A^T.  Stored zeros count, duplicates
 *     count once, self-loops are ignored.  deg(i) is the number of distinct neighbours.
 *   Sequence cm: (1) all vertices of degree 0, in ascending index.  (2) While unnumbered vertices remain, a root r: the unnumbered
 *     vertex of smallest (deg, index), refined by George and Liu's rule - build the level structure of r over the unnumbered
 *     vertices, let c be the vertex of its last level with smallest (deg, index), build c's level structure; if it has more levels
 *     than r's, c becomes r and the rule is applied again, at most 8 times per component in all (kRcmRootRepeats of
 *     reorder_settings.hpp).  (3) r is numbered, then level by level: the next level is the set of unnumbered neighbours of the
 *     current one, ordered by (smallest position in cm among its neighbours in the current level, deg, index).  That is the queue
 *     algorithm (pop v, append its unnumbered neighbours in ascending (deg, index)).
 *   Result: order[k] = cm[n-1-k].  Every run returns the same integers; tests/rcm_ref.py is the NumPy twin.
 *   Refused on the host: a null argument, a shard, released CSR arrays, a handle of another context, a matrix that is not square
 *     (SPMV_ERR_INVALID); a handle that is not CSR (SPMV_ERR_UNSUPPORTED).  After counting on the device: more than 2^31 - 1 keys of
 *     the symmetrised adjacency, two per stored off-diagonal entry, whose ids are int32 (SPMV_ERR_UNSUPPORTED).
 * spmv_perm_download: order and / or inverse to the host (n entries each; NULL skips one).  Synchronous.
 * spmv_perm_info: "n"; and what spmv_perm_rcm did, 0 for a permutation made by spmv_perm_create: "rcm_isolated" (vertices of degree
 *   0), "rcm_components" (components with at least one edge), "rcm_levels" (levels of the numbering passes, the roots' included, summed
 *   over the components), "rcm_bfs" (level structures built, root searches included), "rcm_launches" (kernel launches, scans, sorts
 *   and device copies the call issued), "rcm_transient_bytes" (device memory the call held beside the permutation and the radix
 *   sort's own buffers).  An unknown name: SPMV_ERR_INVALID.
 * spmv_perm_destroy: waits for the context's stream and frees the permutation.  NULL is allowed.
 * spmv_csr_permute: B = P_r A P_c^T, B[k][l] = A[order_r[k]][order_c[l]], as an owning CSR handle like spmv_spgemm's result: it selects
 *   its kernel as an uploaded handle does (a plan of the context is not applied to it).  Synchronous.  Row k of B holds the entries
 *   of row order_r[k] of A with column j renamed inverse_c[j], in ascending new column; entries of equal new column keep A's stored
 *   order; duplicates are kept, not summed; values are copied bit for bit.  A NULL permutation is the identity (the columns of a row
 *   are still put in ascending order).  A may be rectangular: rows->n = nrow, cols->n = ncol.  Refused on the host: what
 *   spmv_csr_transpose refuses, a permutation of another size, a permutation of another context (SPMV_ERR_INVALID).
 * spmv_vec_permute: back = 0: dst[k] = src[order[k]] (a vector in the old numbering becomes one in the new numbering); back = 1:
 *   dst[order[k]] = src[k] (and back again).  One launch, asynchronous on the context's stream.  The values travel as 64-bit words:
 *   NaN payloads and -0.0 arrive as they left.  Refused on the host: a null argument, back outside 0 .. 1, a permutation or a
 *   vector of another context, src or dst of another length than the permutation, src and dst that overlap (SPMV_ERR_INVALID).  n = 0: nothing is
 *   launched.
 * spmv_csr_bandwidth: bandwidth = max |i - j| over the stored entries of a CSR handle (0 without entries), profile = the sum over the
 *   non-empty rows of max(0, i - min j).  One reduction kernel, synchronous.  Refusals as spmv_csr_transpose.
 * Solving in the new numbering: INTEGRATION.md ("Solving in another numbering"). */
typedef struct spmv_perm spmv_perm;
int spmv_perm_create(spmv_ctx* ctx, int64_t n, const int32_t* order_host, spmv_perm** out);
int spmv_perm_rcm(spmv_ctx* ctx, const spmv_mat* A, spmv_perm** out);
int spmv_perm_download(const spmv_perm* p, int32_t* order_host, int32_t* inverse_host);
int spmv_perm_info(const spmv_perm* p, const char* name, int64_t* value);
int spmv_perm_destroy(spmv_perm* p);
int spmv_csr_permute(spmv_ctx* ctx, const spmv_mat* A, const spmv_perm* rows, const spmv_perm* cols, spmv_mat** out_B);
int spmv_vec_permute(spmv_ctx* ctx, const spmv_perm* p, int32_t back, const spmv_vec* src, spmv_vec* dst);
int spmv_csr_bandwidth(spmv_ctx* ctx, const spmv_mat* A, int64_t* bandwidth, int64_t* profile);

/* ---- format conversion on the device (src/matrix.cpp:115-154, :450-500) -------------------------- */
/* Both keep the COO order of the entries inside each row (stable), like the reference's backward
 * scatter, so the result is identical to the reference's arrays, not merely equivalent. */
int spmv_coo_to_csr(spmv_ctx* ctx, const spmv_mat* coo, spmv_mat** out_csr);
int spmv_coo_to_ell(spmv_ctx* ctx, const spmv_mat* coo, spmv_mat** out_ell);
int spmv_csr_to_ell(spmv_ctx* ctx, const spmv_mat* csr, spmv_mat** out_ell);

/* ---- block CSR (BSR): csrc/kernels_bsr.hip, csrc/convert_bsr.hip ------------------------------------------------------------
 * Square blocks of bs x bs values, 2 <= bs <= 8 (any other bs: SPMV_ERR_UNSUPPORTED).  nrow and ncol are SCALAR dimensions and
 * need not be multiples of bs: there are mb = ceil(nrow / bs) block rows and nbc = ceil(ncol / bs) block columns.  Arrays (in
 * the order of spmv_mat_download / spmv_mat_device_ptrs): a = the block row pointer, mb + 1 entries from 0 to nnzb; b = the block
 * column of every block, nnzb entries < nbc; v = nnzb * bs * bs doubles, the blocks one after the other, row-major inside a
 * block.  Positions of a stored block outside nrow x ncol are ABSENT: they are never multiplied (whatever the caller left
 * there), x is never read at or beyond ncol and y never written at or beyond nrow.
 * spmv_mat_get_info: format 5, ell_k = bs, nnz = nnzb * bs * bs, max_row_nnz = the most blocks in a block row times bs,
 * kernel 1, lanes_per_row = the lanes a block row gets - bs * bs times a divisor of 64 / (bs * bs), chosen at creation from the
 * mean number of blocks per block row; spmv_mat_set_kernel takes AUTO (0: choose again) or VECTOR (1) with 0 or such a number.
 * The product y += A x (spmv_apply, _timed, _host, _dot and every solver under SPMV_PRECOND_NONE / _CHEBYSHEV) adds a scalar
 * row's sums in a fixed order without atomics: the same bits at every launch.  spmv_apply_transpose runs the same kernel on a
 * BSR handle of A^T that spmv_mat_transpose_setup builds on the device (blocks in stable order by block column, each block
 * transposed); that handle's memory is counted in device_bytes and freed with the handle.
 * Refused: spmv_apply_multi and spmv_cg_multi, spmv_mat_partition_rows(balance_entries = 1) (SPMV_ERR_UNSUPPORTED), and
 * every entry point that needs a CSR handle (ILU(0), SymGS, AMG, SpGEMM, the reorderings, the Jacobi preconditioner), as for
 * an ELL handle.  The way there is spmv_bsr_to_csr. */
int spmv_bsr_upload(spmv_ctx* ctx, int32_t nrow, int32_t ncol, int32_t bs, const int32_t* brow_ptr, const int32_t* bcol, const double* values,
                    spmv_mat** out);
int spmv_bsr_wrap_device(spmv_ctx* ctx, int32_t nrow, int32_t ncol, int32_t bs, const int32_t* d_brow_ptr, const int32_t* d_bcol,
                         const double* d_values, spmv_mat** out);
/* Both conversions run on the device, synchronously; the caller owns the result.
 * spmv_csr_to_bsr: any unsharded CSR handle with its arrays.  The blocks are those that hold an entry; block columns ascend
 *   inside a block row; a stored position is the sum of the CSR entries that fall on it, added in stored order from 0.0
 *   (duplicates are added, a single entry comes through unchanged), a position without an entry is 0.0.
 * spmv_bsr_to_csr: the stored positions inside nrow x ncol, columns ascending (blocks of one block row in stable order by
 *   block column); drop_zeros != 0 leaves out the values equal to 0.0.
 * For a CSR handle with ascending columns, no duplicates and no zero values, bsr_to_csr(csr_to_bsr(A, bs), 1) is A, array for
 * array.  Refused on the host: null arguments, a bs outside 2 .. 8, a handle of the wrong format (SPMV_ERR_UNSUPPORTED), a
 * shard, a handle of another context, a CSR handle without its arrays (SPMV_ERR_INVALID). */
int spmv_csr_to_bsr(spmv_ctx* ctx, const spmv_mat* csr, int32_t bs, spmv_mat** out_bsr);
int spmv_bsr_to_csr(spmv_ctx* ctx, const spmv_mat* bsr, int32_t drop_zeros, spmv_mat** out_csr);

/* ---- CSR with single-precision value storage (SPMV_FMT_CSR_F32 = 6): csrc/kernels_csr_f32.hip, csrc/convert_f32.hip -----------
 * A CSR matrix with an int32 row pointer (nnz < 2^31, as CSR) whose entries live in ONE packed stream: an 8-byte word per entry,
 * the column in the low 32 bits, the IEEE bits of the float value in the high 32.  The handle holds the row pointer and that
 * stream - no fp64 copy of the values, no separate column array: 8 bytes per entry against CSR's 12.  x is gathered, the sums
 * are accumulated and y is written in fp64.  device_bytes = 4 (nrow + 1) + 8 nnz.
 * The product y += A x (spmv_apply, _timed, _host, _dot, and every solver under SPMV_PRECOND_NONE or a Chebyshev state set up with
 * explicit bounds) runs csr_f32_kernel<lanes>: the arrangement AND the order of operations of the row-parallel CSR kernel.  THE
 * CONTRACT: a product of a format-6 handle returns the same bits as the product of the fp64 CSR handle that holds the widened
 * values, forced to SPMV_CSR_VECTOR at the same lanes_per_row with default flags.  No atomics touch y.
 * spmv_mat_get_info: format 6, kernel 1 (SPMV_CSR_VECTOR), lanes_per_row chosen from the mean row length, max_row_nnz.
 * spmv_mat_set_kernel: AUTO (0: choose the lanes again) or VECTOR (1) with 0 or a power of two <= 64; anything else
 * SPMV_ERR_UNSUPPORTED.  spmv_mat_validate: the CSR checks.  spmv_mat_download: a = the row pointer, b = the columns, v = the
 * values widened to double.  spmv_apply_transpose: spmv_mat_transpose_setup builds a format-6 handle of A^T once - the values
 * are widened into an fp64 CSR copy, the device transpose (spmv_csr_transpose) runs on it and the result is packed again; the
 * two fp64 intermediates (12 nnz bytes each, plus the transpose's own set-up memory) are TRANSIENT and freed before it
 * returns; the companion (4 (ncol + 1) + 8 nnz bytes) is counted in device_bytes and freed with the handle.
 * Refused with SPMV_ERR_UNSUPPORTED, the message naming format 6: spmv_apply_multi and spmv_cg_multi, spmv_mat_device_ptrs,
 * spmv_mat_set_flags with any bit set, spmv_mat_partition_rows(balance_entries = 1), spmv_mat_get_plan / spmv_mat_set_plan (a
 * format-6 handle has one kernel and no plan; spmv_plan_check refuses a node of format 6), and every entry point that needs a
 * CSR handle (ILU(0), SymGS, AMG, FSAI, SpGEMM, the reorderings, the Jacobi preconditioner).  The way there is spmv_f32_to_csr.
 * There is NO spmv_csr_f32_wrap_device: the packed stream is the handle's own layout, not one a caller holds.
 *
 * spmv_csr_to_f32: from an unsharded CSR handle of this context that still has its arrays.  ONE device pass rounds every value
 *   to nearest-even, packs the stream and gathers three statistics: the values that changed (inexact), the nonzero values that
 *   became zero or subnormal (underflow), and the largest relative change |float(v) - v| / |v| among the changed values that did
 *   not underflow.  Counts are integer atomics and the largest change is a maximum: the same bits after every call.  A value that
 *   rounds to +-inf, or is not finite to begin with, refuses the conversion with SPMV_ERR_INVALID (the message gives their number
 *   and the first row that holds one); no handle is returned.
 * spmv_csr_f32_upload: host arrays (row_ptr of nrow + 1 entries from 0, nnz columns, nnz floats), packed on the device; a value
 *   that is not finite is refused in the same way.
 * spmv_f32_to_csr: the fp64 CSR handle of the widened values (exact), analysed like an uploaded one.
 * spmv_f32_info: the three statistics of spmv_csr_to_f32; all zero for an uploaded handle (any pointer may be null).
 * Refused on the host before the device is touched: null arguments, a handle of the wrong format (SPMV_ERR_UNSUPPORTED), a
 * shard, a handle of another context, a CSR handle without its arrays (SPMV_ERR_INVALID). */
int spmv_csr_to_f32(spmv_ctx* ctx, const spmv_mat* csr, spmv_mat** out_f32);
int spmv_csr_f32_upload(spmv_ctx* ctx, int32_t nrow, int32_t ncol, const int32_t* row_ptr, const int32_t* col_ind, const float* values,
                        spmv_mat** out);
int spmv_f32_to_csr(spmv_ctx* ctx, const spmv_mat* f32, spmv_mat** out_csr);
int spmv_f32_info(const spmv_mat* f32, int64_t* inexact, int64_t* underflow, double* max_rel_err);

/* Split a CSR handle (a row shard) by column range, on the device: `inside` holds the entries with a column in
 * [col_begin, col_end), REBASED to 0 (it multiplies the caller's own slice of x: ncol = col_end - col_begin);
 * `outside` holds the others with their global columns.  A*x = inside*x[col_begin:col_end] + outside*x, rows and the
 * order inside each row kept.  For the sharded solver step: the inside product needs no exchange and can run while
 * the x all-gather is in flight (no counterpart in the reference).
 * Row bookkeeping: `outside` keeps the shard's row_begin.  `inside` reports row_begin = csr.row_begin - col_begin (see
 * spmv_mat_get_info): because its columns are rebased, local row i meets its own diagonal at column row_begin + i of
 * `inside` - the offset the Jacobi diagonal and the Gauss-Seidel sweep of the sharded solver use.  For the usual call
 * (col_begin = the shard's first row) that is 0: a square block starting at (0, 0).  It is NEGATIVE when col_begin lies
 * beyond the shard's first row (rows before col_begin have no diagonal inside the block). */
int spmv_csr_split_columns(spmv_ctx* ctx, const spmv_mat* csr, int32_t col_begin, int32_t col_end,
                           spmv_mat** out_inside, spmv_mat** out_outside);

/* ---- row-range sharding (src/mat_vec.cpp:233,245-246) ------------------------------------------- */
/* Equal rows per part, the last part takes the remainder.  Pure host arithmetic. */
int spmv_partition_rows(int64_t nrow, int32_t nparts, int32_t part, int64_t* row_begin,
                        int64_t* row_end);
/* Entry-balanced alternative ("an nnz-balanced split as an option for C4-like skew"): bounds[nparts+1],
 * bounds[p] = first row of part p; the boundary of part p is the row boundary whose offset lies nearest to p / nparts of the
 * entries (rows are never split, so a part can exceed its share by at most half its longest boundary row).  The reference
 * partitions by equal rows only (src/mat_vec.cpp:151,233): that stays the default of every driver; this is the option. */
int spmv_partition_rows_balanced(int64_t nrow, const int64_t* row_ptr64, int32_t nparts,
                                 int64_t* bounds);
/* The same for a DEVICE-RESIDENT handle: bounds[nparts+1] over its rows (over its COLUMNS for CSC, which the reference shards
 * by column, src/mat_vec.cpp:299-337).  balance_entries = 0: equal rows, the last part takes the remainder (the reference's
 * split); 1: by entries - CSR / CSC from the offset array, COO from a histogram of its row indices taken on the device (any
 * entry order); ELL and DIA store the same number of slots for every row, so equal rows are equal work and are what they
 * get either way.  Synchronous; the offsets cross to the host (4 bytes per row), the entries do not. */
int spmv_mat_partition_rows(const spmv_mat* m, int32_t nparts, int32_t balance_entries, int64_t* bounds);
/* Rows [row_begin, row_end) of a device-resident CSR handle (local row numbers of that handle) as a shard of their own on
 * dst_ctx - the same GPU or a peer over xGMI: rebased int32 row_ptr, global column indices (src/mat_vec.cpp:250-265), entries
 * copied device to device, analysed like an uploaded shard; its row_begin = the source's row_begin + row_begin.  With
 * spmv_mat_partition_rows this shards a matrix that was generated, converted or uploaded once without a second trip through
 * the host.  Synchronous.  The source must still hold its CSR arrays (panel_keep_csr = 1). */
int spmv_csr_extract_rows(spmv_ctx* dst_ctx, const spmv_mat* csr, int64_t row_begin, int64_t row_end, spmv_mat** out);

/* ---- synthetic inputs (counter-based splitmix64) ------------- */
/* CSR shard with exactly k entries in each of rows [row_begin,row_end) of a (nrow_global x ncol)
 * matrix.  band == 0: columns uniform over [0,ncol); band > 0: uniform in a window of `band`
 * columns centred on the diagonal (wrapping).  values U(-1,1). */
int spmv_gen_csr_uniform(spmv_ctx* ctx, int64_t row_begin, int64_t row_end, int32_t ncol, int32_t k,
                         int32_t band, uint64_t seed, spmv_mat** out);
/* ELL with k slots per row, circulant band col = (i + d - k/2) mod ncol, values U(-1,1). */
int spmv_gen_ell_banded(spmv_ctx* ctx, int32_t nrow, int32_t ncol, int32_t k, uint64_t seed,
                        spmv_mat** out);
/* Row-sorted COO with power-law row lengths min(max_len, floor(8/u)), u ~ U(0,1], uniform columns. */
/* DIA (row-major, reference layout) with k diagonals at offsets d - k/2, same value draws as spmv_gen_ell_banded. */
int spmv_gen_dia_banded(spmv_ctx* ctx, int32_t nrow, int32_t k, uint64_t seed, spmv_mat** out);
int spmv_gen_coo_powerlaw(spmv_ctx* ctx, int32_t nrow, int32_t ncol, int32_t max_len, uint64_t seed,
                          spmv_mat** out);
/* The same distribution of row lengths taken at its quantiles (u_i = (i + 1) / nrow) instead of drawn: the rows come SORTED BY
 * LENGTH, the longest first - every heavy row at one end, the positional skew an equal-rows partition handles worst (the first
 * of 8 equal-rows shards of N = 2M holds 43 % of the entries).  Columns and values as above. */
int spmv_gen_coo_powerlaw_sorted(spmv_ctx* ctx, int32_t nrow, int32_t ncol, int32_t max_len, uint64_t seed,
                                 spmv_mat** out);
/* v[i] = U(0,1) drawn from (seed, global index index_offset + i). */
int spmv_gen_vec_uniform(spmv_ctx* ctx, spmv_vec* v, int64_t index_offset, uint64_t seed);

#ifdef __cplusplus
}
#endif
#endif /* SPMV_ABI_H */
