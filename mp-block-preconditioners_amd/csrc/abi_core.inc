// The first section of the C ABI: version and last error, the kernel options and their setters, operator assembly,
// scan, SpGEMM and the refills, the row-block planner, diagonal / Gershgorin / extraction, SpMV, the Jacobi and
// Chebyshev steps, gather / scatter and the event helpers.
// Opens with device_flags, the zero / launch / read-back round trip that five of its entries share.
// Needs mpbp.hip's prelude, its assembly, SpGEMM, epilogue and SpMV kernels, and launchers.inc.
// A fragment of mpbp.hip, included there once and in order: not a self-contained header.

namespace {
// One round trip of device flags: `count` words of T zeroed on the device, launch(d) enqueues the kernels that set
// them, and they are copied to `out` once the stream has drained.  Always frees; a HIP error is reported as who's.
template <class T, class Launch>
int device_flags(const char* who, T* out, size_t count, hipStream_t st, Launch&& launch) {
    T* d = nullptr;
    hipError_t e = hipMalloc(&d, count * sizeof(T));
    if (e == hipSuccess) e = hipMemsetAsync(d, 0, count * sizeof(T), st);
    if (e == hipSuccess) {
        launch(d);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out, d, count * sizeof(T), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    (void)hipFree(d);
    return e == hipSuccess ? MPBP_OK : set_error(MPBP_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
}
}  // namespace

// ================================================================ C ABI ====
extern "C" {

const char* mpbp_version(void) { return "libmpbp 0.1 (gfx950)"; }

void mpbp_kernel_opts_default(mpbp_kernel_opts* out) {
    if (out) *out = KO();
}

int mpbp_kernel_opts_set_thread(const mpbp_kernel_opts* o, const mpbp_kernel_opts** prev) {
    if (int rc = check_opts(o, "kernel_opts_set_thread")) return rc;
    if (prev) *prev = t_opts;
    t_opts = o;
    return MPBP_OK;
}

// The process defaults, one entry point per field that has one (ranges: kOpts, mpbp.hip).  Four of them store on != 0.
int mpbp_set_march_rows(int32_t rows) { return set_default(offsetof(mpbp_kernel_opts, march_rows), rows); }
int mpbp_set_init_diag(int32_t mode) { return set_default(offsetof(mpbp_kernel_opts, init_diag), mode); }
int mpbp_set_f_pair(int32_t on) { return set_default(offsetof(mpbp_kernel_opts, f_pair), on); }
int mpbp_set_f_direct(int32_t on) { return set_default(offsetof(mpbp_kernel_opts, f_direct), on); }
int mpbp_set_gtg_drhs(int32_t on) { return set_default(offsetof(mpbp_kernel_opts, gtg_drhs), on); }
int mpbp_set_q13_sym(int32_t on) { return set_default(offsetof(mpbp_kernel_opts, q13_sym), on); }
int mpbp_set_f_tile(int32_t on) { return set_default(offsetof(mpbp_kernel_opts, f_tile), on); }
int mpbp_set_f_solve(int32_t on) { return set_default(offsetof(mpbp_kernel_opts, f_solve), on); }
int mpbp_set_mg_galerkin_mf(int32_t on) { return set_default(offsetof(mpbp_kernel_opts, mg_galerkin_mf), on); }
int mpbp_set_mg_galerkin_mf_p(int32_t on) { return set_default(offsetof(mpbp_kernel_opts, mg_galerkin_mf_p), on); }
int mpbp_set_mg_group_rows(int32_t rows) { return set_default(offsetof(mpbp_kernel_opts, mg_group_rows), rows); }
int mpbp_set_pg_direct(int32_t on) { return set_default(offsetof(mpbp_kernel_opts, pg_direct), on != 0); }
int mpbp_set_mg_svl(int32_t on) { return set_default(offsetof(mpbp_kernel_opts, mg_svl), on != 0); }
int mpbp_set_mg_mf_transfer(int32_t on) { return set_default(offsetof(mpbp_kernel_opts, mg_mf_transfer), on != 0); }
int mpbp_set_csr_table(int32_t on) { return set_default(offsetof(mpbp_kernel_opts, csr_table), on != 0); }
int mpbp_set_gtg_fused(int32_t on) {   // 256 / 512: on, with that many lanes per workgroup
    if (on != 256 && on != 512) return set_default(offsetof(mpbp_kernel_opts, gtg_fused), on);
    g_defaults.gtg_tpb = on;
    return set_default(offsetof(mpbp_kernel_opts, gtg_fused), 1);
}
const char* mpbp_last_error(void) { return g_err; }

int mpbp_stokes_theta(int32_t n, double* cell, double* uface, double* vface, void* stream) {
    if (n < 1 || !cell || !uface || !vface) return set_error(MPBP_ERR_ARG, "mpbp_stokes_theta: bad args");
    k_theta<<<grid_for((int64_t)n * n), kBlock, 0, as_stream(stream)>>>(n, cell, uface, vface);
    MPBP_HIP(hipGetLastError());
    return MPBP_OK;
}

int64_t mpbp_stokes_rows(int32_t n, int32_t op) {
    const int64_t N = (int64_t)n * n;
    switch (op) {
    case MPBP_OP_A: return 5 * N;
    case MPBP_OP_F: case MPBP_OP_G: return 4 * N;
    case MPBP_OP_D: case MPBP_OP_D_N: case MPBP_OP_D_S: return N;
    case MPBP_OP_L_N: case MPBP_OP_L_S: case MPBP_OP_G_N: case MPBP_OP_G_S:
    case MPBP_OP_XI_N: case MPBP_OP_XI_S: return 2 * N;
    default: return set_error(MPBP_ERR_ARG, "unknown operator %d", op);
    }
}

int64_t mpbp_stokes_cols(int32_t n, int32_t op) {
    const int64_t N = (int64_t)n * n;
    switch (op) {
    case MPBP_OP_A: return 5 * N;
    case MPBP_OP_F: case MPBP_OP_D: return 4 * N;
    case MPBP_OP_G: case MPBP_OP_G_N: case MPBP_OP_G_S: return N;
    case MPBP_OP_L_N: case MPBP_OP_L_S: case MPBP_OP_D_N: case MPBP_OP_D_S:
    case MPBP_OP_XI_N: case MPBP_OP_XI_S: return 2 * N;
    default: return set_error(MPBP_ERR_ARG, "unknown operator %d", op);
    }
}

static int make_stokes(const mpbp_stokes_params* prm, const double* cell, const double* uface,
                       const double* vface, StokesDev* P) {
    if (!prm || prm->n < 1 || !cell) return set_error(MPBP_ERR_ARG, "stokes: bad params");
    if ((int64_t)prm->n * prm->n * 5 > INT32_MAX) return set_error(MPBP_ERR_OVERFLOW, "stokes: n too large");
    *P = StokesDev{prm->n, prm->xi, prm->eta_n, prm->eta_s, prm->c, prm->d_u, prm->d_p, prm->d_div,
                   cell, uface, vface};
    return MPBP_OK;
}

int mpbp_stokes_count(const mpbp_stokes_params* prm, int32_t op, const double* cell,
                      int32_t* row_nnz, void* stream) {
    StokesDev P;
    int rc = make_stokes(prm, cell, nullptr, nullptr, &P);
    if (rc) return rc;
    const int64_t rows = mpbp_stokes_rows(prm->n, op);
    if (rows < 0) return (int)rows;
    k_stokes_count<<<grid_for(rows), kBlock, 0, as_stream(stream)>>>(P, op, rows, row_nnz);
    MPBP_HIP(hipGetLastError());
    return MPBP_OK;
}

int mpbp_stokes_fill(const mpbp_stokes_params* prm, int32_t op, const double* cell,
                     const double* uface, const double* vface, const int32_t* row_ptr,
                     int32_t* col_idx, double* val, void* stream) {
    StokesDev P;
    int rc = make_stokes(prm, cell, uface, vface, &P);
    if (rc) return rc;
    if ((op == MPBP_OP_A || op == MPBP_OP_F) && (!uface || !vface))
        return set_error(MPBP_ERR_ARG, "stokes fill: A/F need face tables");
    const int64_t rows = mpbp_stokes_rows(prm->n, op);
    if (rows < 0) return (int)rows;
    k_stokes_fill<<<grid_for(rows), kBlock, 0, as_stream(stream)>>>(P, op, rows, row_ptr, col_idx, val);
    MPBP_HIP(hipGetLastError());
    return MPBP_OK;
}

int mpbp_stokes_count_rows(const mpbp_stokes_params* prm, int32_t op, const double* cell, const int32_t* rows,
                           int32_t nrows, int32_t* row_nnz, void* stream) {
    StokesDev P;
    int rc = make_stokes(prm, cell, nullptr, nullptr, &P);
    if (rc) return rc;
    if (mpbp_stokes_rows(prm->n, op) < 0) return set_error(MPBP_ERR_ARG, "stokes count rows: unknown operator %d", op);
    if (nrows < 0 || (nrows > 0 && (!rows || !row_nnz))) return set_error(MPBP_ERR_ARG, "stokes count rows: bad args");
    if (nrows == 0) return MPBP_OK;
    k_stokes_count<<<grid_for(nrows), kBlock, 0, as_stream(stream)>>>(P, op, nrows, row_nnz, rows);
    MPBP_HIP(hipGetLastError());
    return MPBP_OK;
}

int mpbp_stokes_fill_rows(const mpbp_stokes_params* prm, int32_t op, const double* cell, const double* uface,
                          const double* vface, const int32_t* rows, int32_t nrows, const int32_t* row_ptr,
                          int32_t* col_idx, double* val, void* stream) {
    StokesDev P;
    int rc = make_stokes(prm, cell, uface, vface, &P);
    if (rc) return rc;
    if ((op == MPBP_OP_A || op == MPBP_OP_F) && (!uface || !vface))
        return set_error(MPBP_ERR_ARG, "stokes fill rows: A/F need face tables");
    if (mpbp_stokes_rows(prm->n, op) < 0) return set_error(MPBP_ERR_ARG, "stokes fill rows: unknown operator %d", op);
    if (nrows < 0 || (nrows > 0 && (!rows || !row_ptr))) return set_error(MPBP_ERR_ARG, "stokes fill rows: bad args");
    if (nrows == 0) return MPBP_OK;
    k_stokes_fill<<<grid_for(nrows), kBlock, 0, as_stream(stream)>>>(P, op, nrows, row_ptr, col_idx, val, rows);
    MPBP_HIP(hipGetLastError());
    return MPBP_OK;
}

int mpbp_exclusive_scan(const int32_t* row_nnz, int32_t* row_ptr, int64_t n, int64_t* total,
                        void* stream) {
    if (n < 0 || !row_ptr || (n > 0 && !row_nnz)) return set_error(MPBP_ERR_ARG, "scan: bad args");
    const int64_t ntiles = (n + kScanTile - 1) / kScanTile;
    long long* d_total = nullptr;   // [total, tile sums...]
    MPBP_HIP(hipMalloc(&d_total, sizeof(long long) * (size_t)(1 + ntiles)));
    hipStream_t st = as_stream(stream);
    if (ntiles > 0) k_scan_tiles<<<(unsigned)ntiles, 256, 0, st>>>(row_nnz, n, d_total + 1);
    k_scan_offsets<<<1, 256, 0, st>>>(d_total + 1, ntiles, row_ptr, n, d_total);
    if (ntiles > 0) k_scan_apply<<<(unsigned)ntiles, 256, 0, st>>>(row_nnz, n, d_total + 1, row_ptr);
    hipError_t e = hipGetLastError();
    long long h = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&h, d_total, sizeof(h), hipMemcpyDeviceToHost, as_stream(stream));
    if (e == hipSuccess) e = hipStreamSynchronize(as_stream(stream));
    (void)hipFree(d_total);
    if (e != hipSuccess) return set_error(MPBP_ERR_HIP, "scan: %s", hipGetErrorString(e));
    if (h > INT32_MAX) return set_error(MPBP_ERR_OVERFLOW, "scan: %lld entries exceed int32 row_ptr", h);
    if (total) *total = h;
    return MPBP_OK;
}

int mpbp_spgemm_count(const mpbp_csr* A, const mpbp_csr* B, int32_t* row_nnz, void* stream) {
    return spgemm_count<kSpgemmMaxW>(A, B, row_nnz, stream);
}
int mpbp_spgemm_fill(const mpbp_csr* A, const mpbp_csr* B, double alpha, const int32_t* row_ptr,
                     int32_t* col_idx, double* val, void* stream) {
    return spgemm_fill<kSpgemmMaxW>(A, B, alpha, row_ptr, col_idx, val, stream);
}
int mpbp_spgemm_count_wide(const mpbp_csr* A, const mpbp_csr* B, int32_t* row_nnz, void* stream) {
    return spgemm_count<kSpgemmWideW>(A, B, row_nnz, stream);
}
int mpbp_spgemm_fill_wide(const mpbp_csr* A, const mpbp_csr* B, double alpha, const int32_t* row_ptr,
                          int32_t* col_idx, double* val, void* stream) {
    return spgemm_fill<kSpgemmWideW>(A, B, alpha, row_ptr, col_idx, val, stream);
}

namespace {
inline RCsr to_rcsr(const mpbp_csr* A) { return RCsr{A->row_ptr, A->col_idx, A->val, A->nrows, A->ncols, A->nnz}; }

// launches k_refill<MODE> (wide: its two-entries-per-lane form) over C's rows, waits and turns the kernel's flags into
// a return code
int run_refill(const char* who, int mode, const mpbp_csr* X, const mpbp_csr* Y, const mpbp_csr* Z, double alpha_inner,
               double alpha_outer, const mpbp_csr* C, void* stream, bool wide = false) {
    if (C->nrows == 0) return MPBP_OK;
    hipStream_t st = as_stream(stream);
    int h[2] = {0, 0};
    const int rc = device_flags(who, h, 2, st, [&](int* d_err) {
        const unsigned grid = (unsigned)(((int64_t)C->nrows + kBlock / 64 - 1) / (kBlock / 64));
        double* cval = const_cast<double*>(C->val);   // the one array a refill writes
        const RCsr x = to_rcsr(X), y = to_rcsr(Y), z = Z ? to_rcsr(Z) : RCsr{nullptr, nullptr, nullptr, 0, 0, 0};
        if (wide && mode == kRefillPair) k_refill<kRefillPair, true><<<grid, kBlock, 0, st>>>(x, y, z, alpha_inner, alpha_outer, to_rcsr(C), cval, d_err);
        else if (wide && mode == kRefillLeft) k_refill<kRefillLeft, true><<<grid, kBlock, 0, st>>>(x, y, z, alpha_inner, alpha_outer, to_rcsr(C), cval, d_err);
        else if (wide) k_refill<kRefillRight, true><<<grid, kBlock, 0, st>>>(x, y, z, alpha_inner, alpha_outer, to_rcsr(C), cval, d_err);
        else if (mode == kRefillPair) k_refill<kRefillPair><<<grid, kBlock, 0, st>>>(x, y, z, alpha_inner, alpha_outer, to_rcsr(C), cval, d_err);
        else if (mode == kRefillLeft) k_refill<kRefillLeft><<<grid, kBlock, 0, st>>>(x, y, z, alpha_inner, alpha_outer, to_rcsr(C), cval, d_err);
        else k_refill<kRefillRight><<<grid, kBlock, 0, st>>>(x, y, z, alpha_inner, alpha_outer, to_rcsr(C), cval, d_err);
    });
    if (rc) return rc;
    if (h[0] & kRefillIndex) return set_error(MPBP_ERR_ARG, "%s: %d rows hold a row extent or column index out of range", who, h[1]);
    if (h[0] & kRefillWide)
        return set_error(MPBP_ERR_OVERFLOW, "%s: %d rows have an output row wider than %d", who, h[1], kSpgemmWideW);
    if (h[0] & kRefillLong)
        return set_error(MPBP_ERR_OVERFLOW, "%s: %d rows have an %s row wider than %d", who, h[1],
                         wide ? "inner" : "output or inner", kSpgemmMaxW);
    if (h[0] & kRefillMissing)
        return set_error(MPBP_ERR_PATTERN, "%s: %d rows of C lack a column their product holds", who, h[1]);
    return MPBP_OK;
}
}  // namespace

static int spgemm_refill(const char* who, bool wide, const mpbp_csr* A, const mpbp_csr* B, double alpha,
                         const mpbp_csr* C, void* stream) {
    int rc = check_csr(A);
    if (!rc) rc = check_csr(B);
    if (!rc) rc = check_csr(C);
    if (rc) return rc;
    if (A->ncols != B->nrows || C->nrows != A->nrows || C->ncols != B->ncols)
        return set_error(MPBP_ERR_ARG, "%s: shape mismatch", who);
    return run_refill(who, kRefillPair, A, B, nullptr, 1.0, alpha, C, stream, wide);
}
int mpbp_spgemm_refill(const mpbp_csr* A, const mpbp_csr* B, double alpha, const mpbp_csr* C, void* stream) {
    return spgemm_refill("spgemm_refill", false, A, B, alpha, C, stream);
}
int mpbp_spgemm_refill_wide(const mpbp_csr* A, const mpbp_csr* B, double alpha, const mpbp_csr* C, void* stream) {
    return spgemm_refill("spgemm_refill_wide", true, A, B, alpha, C, stream);
}

static int triple_refill(const char* who, bool wide, const mpbp_csr* X, const mpbp_csr* Y, const mpbp_csr* Z,
                         int32_t assoc, double alpha_inner, double alpha_outer, const mpbp_csr* C, void* stream) {
    int rc = check_csr(X);
    if (!rc) rc = check_csr(Y);
    if (!rc) rc = check_csr(Z);
    if (!rc) rc = check_csr(C);
    if (rc) return rc;
    if (assoc != MPBP_ASSOC_LEFT && assoc != MPBP_ASSOC_RIGHT)
        return set_error(MPBP_ERR_ARG, "%s: assoc must be MPBP_ASSOC_LEFT or MPBP_ASSOC_RIGHT", who);
    if (X->ncols != Y->nrows || Y->ncols != Z->nrows || C->nrows != X->nrows || C->ncols != Z->ncols)
        return set_error(MPBP_ERR_ARG, "%s: shape mismatch", who);
    return run_refill(who, assoc == MPBP_ASSOC_LEFT ? kRefillLeft : kRefillRight, X, Y, Z, alpha_inner, alpha_outer, C,
                      stream, wide);
}
int mpbp_triple_refill(const mpbp_csr* X, const mpbp_csr* Y, const mpbp_csr* Z, int32_t assoc, double alpha_inner,
                       double alpha_outer, const mpbp_csr* C, void* stream) {
    return triple_refill("triple_refill", false, X, Y, Z, assoc, alpha_inner, alpha_outer, C, stream);
}
int mpbp_triple_refill_wide(const mpbp_csr* X, const mpbp_csr* Y, const mpbp_csr* Z, int32_t assoc, double alpha_inner,
                            double alpha_outer, const mpbp_csr* C, void* stream) {
    return triple_refill("triple_refill_wide", true, X, Y, Z, assoc, alpha_inner, alpha_outer, C, stream);
}

int64_t mpbp_plan_row_blocks(const int32_t* row_ptr, int32_t row_begin, int32_t row_end,
                             int32_t* pairs, int64_t capacity) {
    if (!row_ptr || row_begin < 0 || row_end < row_begin) return set_error(MPBP_ERR_ARG, "plan: bad args");
    int64_t nb = 0;
    int32_t r = row_begin;
    while (r < row_end) {
        const int32_t s = r;
        int32_t e = r;
        while (e < row_end && e - s < kBlock && row_ptr[e + 1] - row_ptr[s] <= MPBP_BLOCK_NNZ) ++e;
        if (e == s) e = s + 1;   // one row longer than the LDS stage
        if (pairs && nb < capacity) {
            pairs[2 * nb] = s;
            pairs[2 * nb + 1] = e;
        }
        ++nb;
        r = e;
    }
    return nb;
}

int mpbp_csr_diag(const mpbp_csr* A, int32_t col_offset, double* diag, int32_t* missing, void* stream) {
    int rc = check_csr(A);
    if (rc) return rc;
    int h = 0;
    rc = device_flags("csr_diag", &h, 1, as_stream(stream), [&](int* d_miss) {
        k_csr_diag<<<grid_for(A->nrows), kBlock, 0, as_stream(stream)>>>(to_csr(A), A->nrows, col_offset,
                                                                      diag, d_miss);
    });
    if (rc) return rc;
    if (missing) *missing = h;
    return MPBP_OK;
}

int mpbp_gershgorin(const mpbp_csr* A, const double* diag, double* lmax, void* stream) {
    int rc = check_csr(A);
    if (rc) return rc;
    unsigned long long h = 0;
    rc = device_flags("gershgorin", &h, 1, as_stream(stream), [&](unsigned long long* d_out) {
        k_gershgorin<<<grid_for(A->nrows), kBlock, 0, as_stream(stream)>>>(to_csr(A), A->nrows, diag, d_out);
    });
    if (rc) return rc;
    double v;
    memcpy(&v, &h, sizeof(v));
    if (lmax) *lmax = v;
    return MPBP_OK;
}

int mpbp_csr_extract_count(const mpbp_csr* A, const int32_t* rows, int32_t nrows_local,
                           int32_t* row_nnz, void* stream) {
    int rc = check_csr(A);
    if (rc) return rc;
    if (nrows_local < 0 || (nrows_local && (!rows || !row_nnz))) return set_error(MPBP_ERR_ARG, "extract: bad args");
    if (nrows_local == 0) return MPBP_OK;
    k_extract_count<<<grid_for(nrows_local), kBlock, 0, as_stream(stream)>>>(to_csr(A), rows, nrows_local, row_nnz);
    MPBP_HIP(hipGetLastError());
    return MPBP_OK;
}

int mpbp_csr_extract_fill(const mpbp_csr* A, const int32_t* rows, int32_t nrows_local,
                          const int32_t* colmap, const int32_t* row_ptr_local, int32_t* col_local,
                          double* val_local, void* stream) {
    int rc = check_csr(A);
    if (rc) return rc;
    if (nrows_local == 0) return MPBP_OK;
    int h = 0;
    rc = device_flags("extract_fill", &h, 1, as_stream(stream), [&](int* d_bad) {
        k_extract_fill<<<grid_for(nrows_local), kBlock, 0, as_stream(stream)>>>(
            to_csr(A), rows, nrows_local, colmap, row_ptr_local, col_local, val_local, d_bad);
    });
    if (rc) return rc;
    if (h) return set_error(MPBP_ERR_PATTERN, "extract: %d entries reference columns outside the halo", h);
    return MPBP_OK;
}

int mpbp_spmv(const mpbp_csr* A, const mpbp_rowblocks* blocks, int32_t mode, const double* x,
              const double* z, double* y, void* stream) {
    int rc = check_csr(A);
    if (rc) return rc;
    if (!x || !y || (mode != MPBP_SPMV_STORE && !z)) return set_error(MPBP_ERR_ARG, "spmv: bad vectors");
    const hipStream_t st = as_stream(stream);
    switch (mode) {
    case MPBP_SPMV_STORE: return launch_rows(A, blocks, x, EpiStore{y}, st);
    case MPBP_SPMV_ADD: return launch_rows(A, blocks, x, EpiAdd{z, y}, st);
    case MPBP_SPMV_RESID: return launch_rows(A, blocks, x, EpiResid{z, y}, st);
    default: return set_error(MPBP_ERR_ARG, "spmv: unknown mode %d", mode);
    }
}

int mpbp_hbm_stream(const void* src, int64_t bytes, int32_t mode, double* dst, void* stream) {
    if (!src || !dst || bytes < 16 || (mode != 0 && mode != 1)) return set_error(MPBP_ERR_ARG, "hbm_stream: bad args");
    const hipStream_t st = as_stream(stream);
    if (mode == 0) {
        const int64_t n16 = bytes / 16;
        k_hbm_read<<<(unsigned)((n16 + 1023) / 1024), kBlock, 0, st>>>(reinterpret_cast<const f64x2*>(src), n16, dst);
    } else {
        const int64_t nwaves = bytes / (576 * 16);
        if (nwaves < 1) return set_error(MPBP_ERR_ARG, "hbm_stream: mode 1 needs >= 9 KiB");
        k_hbm_readwrite<<<(unsigned)((nwaves + 3) / 4), kBlock, 0, st>>>(reinterpret_cast<const f64x2*>(src), nwaves,
                                                                         dst);
    }
    MPBP_HIP(hipGetLastError());
    return MPBP_OK;
}

int mpbp_spmv_seg(const mpbp_csr* A, const mpbp_rowblocks* blocks, int32_t mode, const double* x,
                  const double* z, double* y, void* stream) {
    int rc = check_csr(A);
    if (rc) return rc;
    if (!x || !y || (mode != MPBP_SPMV_STORE && !z)) return set_error(MPBP_ERR_ARG, "spmv_seg: bad vectors");
    const hipStream_t st = as_stream(stream);
    switch (mode) {
    case MPBP_SPMV_STORE: return launch_rows_seg(A, blocks, x, EpiStore{y}, st);
    case MPBP_SPMV_ADD: return launch_rows_seg(A, blocks, x, EpiAdd{z, y}, st);
    case MPBP_SPMV_RESID: return launch_rows_seg(A, blocks, x, EpiResid{z, y}, st);
    default: return set_error(MPBP_ERR_ARG, "spmv_seg: unknown mode %d", mode);
    }
}

int mpbp_jacobi_init(int32_t nrows, const double* b, const double* diag, const double* sub,
                     double* x_out, void* stream) {
    if (nrows < 0 || (nrows && (!b || !diag || !x_out))) return set_error(MPBP_ERR_ARG, "jacobi_init: bad args");
    if (!nrows) return MPBP_OK;
    k_jacobi_init<<<grid_for(nrows), kBlock, 0, as_stream(stream)>>>(nrows, b, diag, sub, x_out);
    MPBP_HIP(hipGetLastError());
    return MPBP_OK;
}

int mpbp_jacobi_step(const mpbp_csr* A, const mpbp_rowblocks* blocks, const double* x_in,
                     const double* b, const double* diag, const double* sub, double* x_out,
                     void* stream) {
    int rc = check_csr(A);
    if (rc) return rc;
    if (!x_in || !b || !diag || !x_out || x_in == x_out) return set_error(MPBP_ERR_ARG, "jacobi_step: bad vectors");
    return launch_rows(A, blocks, x_in, EpiJacobi{x_in, b, diag, sub, x_out}, as_stream(stream));
}

int mpbp_cheb_init(int32_t nrows, const double* b, const double* diag, double c2, double* d,
                   const double* sub, double* x_out, void* stream) {
    if (nrows < 0 || (nrows && (!b || !diag || !d || !x_out))) return set_error(MPBP_ERR_ARG, "cheb_init: bad args");
    if (!nrows) return MPBP_OK;
    k_cheb_init<<<grid_for(nrows), kBlock, 0, as_stream(stream)>>>(nrows, b, diag, c2, d, sub, x_out);
    MPBP_HIP(hipGetLastError());
    return MPBP_OK;
}

static int cheb_step_impl(const mpbp_csr* A, const mpbp_rowblocks* blocks, const double* x_in,
                          const double* b, const double* diag, double c1, double c2, double* d,
                          const double* sub, double* x_out, void* stream, int store_d) {
    int rc = check_csr(A);
    if (rc) return rc;
    if (!x_in || !b || !diag || !d || !x_out || x_in == x_out) return set_error(MPBP_ERR_ARG, "cheb_step: bad vectors");
    return launch_rows(A, blocks, x_in, EpiCheb{x_in, b, diag, d, c1, c2, sub, x_out, store_d}, as_stream(stream));
}

int mpbp_cheb_step(const mpbp_csr* A, const mpbp_rowblocks* blocks, const double* x_in,
                   const double* b, const double* diag, double c1, double c2, double* d,
                   const double* sub, double* x_out, void* stream) {
    return cheb_step_impl(A, blocks, x_in, b, diag, c1, c2, d, sub, x_out, stream, 1);
}

int mpbp_cheb_coeffs(double lmin, double lmax, int32_t sweeps, double* c1, double* c2) {
    if (sweeps < 1 || !c1 || !c2 || !(lmax > lmin) || !(lmin >= 0.0))
        return set_error(MPBP_ERR_ARG, "cheb_coeffs: need sweeps >= 1 and lmax > lmin >= 0");
    cheb_coeffs(lmin, lmax, sweeps, c1, c2);
    return MPBP_OK;
}

int mpbp_gather(int32_t count, const int32_t* idx, const double* src, double* dst, void* stream) {
    if (count <= 0) return MPBP_OK;
    k_gather<<<grid_for(count), kBlock, 0, as_stream(stream)>>>(count, idx, src, dst);
    MPBP_HIP(hipGetLastError());
    return MPBP_OK;
}

int mpbp_scatter(int32_t count, const int32_t* idx, const double* src, double* dst, void* stream) {
    if (count <= 0) return MPBP_OK;
    k_scatter<<<grid_for(count), kBlock, 0, as_stream(stream)>>>(count, idx, src, dst);
    MPBP_HIP(hipGetLastError());
    return MPBP_OK;
}

int mpbp_event_create(void** ev) {
    hipEvent_t e;
    MPBP_HIP(hipEventCreate(&e));
    *ev = (void*)e;
    return MPBP_OK;
}

int mpbp_event_create_scoped(void** ev, int32_t device_scope) {
    hipEvent_t e;
    MPBP_HIP(hipEventCreateWithFlags(&e, device_scope ? hipEventReleaseToDevice : hipEventDefault));
    *ev = (void*)e;
    return MPBP_OK;
}

int mpbp_event_record(void* ev, void* stream) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    MPBP_HIP(hipStreamIsCapturing(as_stream(stream), &cs));
    if (cs == hipStreamCaptureStatusNone) MPBP_HIP(hipEventRecord((hipEvent_t)ev, as_stream(stream)));
    return MPBP_OK;
}

int mpbp_event_destroy(void* ev) {
    MPBP_HIP(hipEventDestroy((hipEvent_t)ev));
    return MPBP_OK;
}

int mpbp_event_elapsed_ms(void* start, void* stop, float* ms) {
    MPBP_HIP(hipEventElapsedTime(ms, (hipEvent_t)start, (hipEvent_t)stop));
    return MPBP_OK;
}

}  // extern "C"
