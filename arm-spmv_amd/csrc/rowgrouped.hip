// rowgrouped.hip - the row-grouped copy of a COO, CSC or ELL handle (host code only).
//
// A handle in one of those formats can run from a copy of its entries grouped by row: an internal CSR handle that picks ITS
// kernel like any CSR handle (select.hip) - row-parallel, LDS window, panel, two-phase.  That is how the COO C4 workload runs in
// 0.26 ms against 0.75 for the segmented scan over column bins (a large COO handle with an x beyond L2 is gather-bound in entry
// order exactly like CSR: 13 % of roofline with the scan in place), and how scattered or ragged ELL beats its own kernels.  While it
// does, the handle reports kernel SPMV_CSR_PANEL (runs_from_rowgrouped) and its device_bytes include the copy's.  What each
// format does to produce the copy stays with the format (coo_to_csr, csc_rowgrouped_copy, ell_rowgrouped_copy); reusing,
// dropping and adopting a copy, and the part of AUTO and of spmv_mat_set_kernel the formats share, are here.
#include "common.hpp"

namespace spmv
{
void rowgrouped_drop(spmv_mat* m)
{
    if (!m->rowgrouped) return;
    (void)hipStreamSynchronize(m->ctx->stream);
    m->device_bytes -= m->rowgrouped->device_bytes;
    mat_free(m->rowgrouped);
    m->rowgrouped = nullptr;
    if (m->kernel == SPMV_CSR_PANEL) m->kernel = SPMV_CSR_VECTOR;
}

// An internal CSR handle (a row-grouped copy, a part of a long-row split) whose kernel reads only row_ptr and a layout of its own
// gives its col_ind / values back.  (Every such handle comes from mat_alloc: owned, and its arrays are allocated even when empty.)
void release_unread_csr_arrays(spmv_mat* csr)
{
    if (!kernel_reads_own_layout(csr->kernel) || !csr->owned || csr->nnz <= 0 || !csr->b || !csr->v) return;
    (void)hipFree(const_cast<int32_t*>(csr->b));
    (void)hipFree(const_cast<double*>(csr->v));
    csr->device_bytes -= csr->nnz * 12;
    csr->b = nullptr;
    csr->v = nullptr;
}

// force_kernel AUTO: the copy picks its kernel like any CSR handle (a COO handle's copy leaves out the segmented scan: the handle
// has that scan itself); another kernel id: that kernel is forced on the copy.  A copy that is there already and runs the wanted
// kernel (any, for AUTO) is kept.  A handle too large for the copy's int32 offsets, or empty, gets none (SPMV_OK).
int rowgrouped_build(spmv_mat* m, int32_t force_kernel)
{
    if (m->rowgrouped && (force_kernel == SPMV_CSR_AUTO || m->rowgrouped->kernel == force_kernel))
    {
        m->kernel = SPMV_CSR_PANEL;
        return SPMV_OK;
    }
    const int64_t entries = m->format == SPMV_FMT_ELL ? (int64_t)m->nrow * m->k : m->nnz;  // (ELL: every slot that says something)
    if (entries == 0 || entries > (int64_t)INT32_MAX - 65536 || (m->format == SPMV_FMT_CSC && !launch_fits(m->ncol, 8))) return SPMV_OK;
    rowgrouped_drop(m);
    spmv_mat* csr = nullptr;
    if (m->format == SPMV_FMT_COO)
        SPMV_TRY(coo_to_csr(m->ctx, m, &csr, force_kernel == SPMV_CSR_AUTO ? kCsrAutoNoSegscan : force_kernel));
    else if (m->format == SPMV_FMT_CSC)
        SPMV_TRY(csc_rowgrouped_copy(m, force_kernel, &csr));
    else
        SPMV_TRY(ell_rowgrouped_copy(m, force_kernel, &csr));
    release_unread_csr_arrays(csr);
    m->rowgrouped = csr;
    m->kernel     = SPMV_CSR_PANEL;  // reported as "runs from the row-grouped copy" (whichever CSR kernel that copy picked)
    m->device_bytes += csr->device_bytes;
    return SPMV_OK;
}

// AUTO for a COO or CSC handle, the part the two share: the format's own kernel (the segmented scan, the scatter over the columns)
// or the row-grouped copy.  Model: the copy from 1.5M entries on.  From kSelectMinNnz entries on (trials enabled) the copy is
// built first and `trial` times it against the format's own kernel (select.hip: no allocation between two timings), giving back
// the two best times; the copy stays where it is no slower than 2 % behind (the model's pick) or 2 % ahead (the other one).
int rowgrouped_select(spmv_mat* m, int (*trial)(spmv_mat* m, const select_scratch& sv, bool model_copy, float* t_copy, float* t_own))
{
    const bool     model_copy = m->nnz >= ((int64_t)3 << 19);
    select_scratch sv;
    if (!select_trials_enabled(m) || m->nnz < kSelectMinNnz || sv.alloc(m->ctx, m->ncol, m->nrow) != SPMV_OK)
        return model_copy ? rowgrouped_build(m, SPMV_CSR_AUTO) : SPMV_OK;
    int rc = rowgrouped_build(m, SPMV_CSR_AUTO);
    if (rc == SPMV_ERR_ALLOC && (m->format == SPMV_FMT_CSC || !model_copy))  // (COO: the error stands where the model wants the copy)
    {
        (void)hipGetLastError();
        rc = SPMV_OK;  // no memory for the copy: the format's own kernel runs
    }
    if (rc != SPMV_OK) return rc;
    float t_copy = 1e30f, t_own = 1e30f;
    SPMV_TRY(trial(m, sv, model_copy, &t_copy, &t_own));
    const bool keep_copy = m->rowgrouped && (model_copy ? t_copy <= t_own * 1.02f : t_copy < t_own * 0.98f);
    if (!keep_copy) rowgrouped_drop(m);
    m->kernel = m->rowgrouped ? SPMV_CSR_PANEL : SPMV_CSR_VECTOR;
    return SPMV_OK;
}

// spmv_mat_set_kernel on a COO, CSC or ELL handle: AUTO = the format's own kernel or the row-grouped copy, as selection finds;
// VECTOR = the format's own kernel (a copy stays allocated); PANEL = the copy with the panel kernel forced on it, built now
int rowgrouped_set_kernel(spmv_mat* m, int32_t kernel)
{
    const char* name = m->format == SPMV_FMT_COO ? "COO" : (m->format == SPMV_FMT_CSC ? "CSC" : "ELL");
    const char* own  = m->format == SPMV_FMT_COO ? "segmented scan" : (m->format == SPMV_FMT_CSC ? "scatter over the columns" : "one lane per row");
    SPMV_REQUIRE(kernel == SPMV_CSR_AUTO || kernel == SPMV_CSR_VECTOR || kernel == SPMV_CSR_PANEL, "%s handles take kernel AUTO (0), VECTOR (1: %s) or PANEL (4), got %d",
                 name, own, kernel);
    SPMV_HIP(hipSetDevice(m->ctx->device));
    m->kernel_forced = kernel != SPMV_CSR_AUTO;
    if (kernel == SPMV_CSR_VECTOR)
    {
        m->kernel = SPMV_CSR_VECTOR;
        if (m->format == SPMV_FMT_COO && !m->cb_bins)
        {
            // the scan runs over a copy of the entries in column bins when x is beyond an XCD's L2 ("coo_column_bins" = 0 drops it)
            const int rc = coo_build_bins(m, 0, /*only_if_worth=*/true);
            if (rc != SPMV_OK && rc != SPMV_ERR_ALLOC) return rc;  // (no room for the copy: the scan runs over the handle's own arrays)
            (void)hipGetLastError();
        }
        // lanes_per_row (spmv_mat_set_kernel) picks the variant of the format's own kernel; a DIA-order copy the trial had kept goes
        if (m->format == SPMV_FMT_ELL) SPMV_TRY(ell_use_variant(m, kEllTwoRows, /*keep_requested_copy=*/true));
        return SPMV_OK;
    }
    if (kernel == SPMV_CSR_AUTO)
        SPMV_TRY(m->format == SPMV_FMT_COO ? coo_select_kernel(m) : (m->format == SPMV_FMT_CSC ? csc_select_kernel(m) : ell_select_kernel(m)));
    else
        SPMV_TRY(rowgrouped_build(m, SPMV_CSR_PANEL));
    m->kernel = m->rowgrouped ? SPMV_CSR_PANEL : SPMV_CSR_VECTOR;
    if (m->format == SPMV_FMT_COO && m->kernel == SPMV_CSR_PANEL)
    {
        SPMV_HIP(hipStreamSynchronize(m->ctx->stream));
        coo_free_bins(m);  // (the scan's column bins: nobody multiplies from them now)
    }
    return SPMV_OK;
}
}  // namespace spmv
