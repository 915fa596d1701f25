// C ABI, part 3: the multigrid entries (mg_fields, transfers, mpbp_mg_solve, acceleration coefficients) and
// mpbp_stokes_apply_part.  Needs mpbp.hip's MgFields and k_mg_transfer, launch_stokes_a (pg_stencil.inc),
// abi_stencil.inc, schur_ops.inc, mg_solve.inc and mg_accel.inc.
// A fragment of mpbp.hip, included there once and in order: not a self-contained header.

// ======================================================= multigrid (C ABI) ====
extern "C" {

static int mg_fields(int32_t n, int32_t nfields, const int32_t* kinds, MgFields* F) {
    if (n < 4 || (n & 1) || nfields < 1 || nfields > 8 || !kinds)
        return set_error(MPBP_ERR_ARG, "mg_transfer: need even n >= 4 and 1..8 fields");
    F->nfields = nfields;
    for (int f = 0; f < nfields; ++f) {
        F->ky[f] = kinds[2 * f];
        F->kx[f] = kinds[2 * f + 1];
        if ((F->ky[f] != MPBP_MG_CELL && F->ky[f] != MPBP_MG_NODE) || (F->kx[f] != MPBP_MG_CELL && F->kx[f] != MPBP_MG_NODE))
            return set_error(MPBP_ERR_ARG, "mg_transfer: field kinds must be MPBP_MG_CELL or MPBP_MG_NODE");
    }
    if ((int64_t)nfields * n * n > INT32_MAX) return set_error(MPBP_ERR_ARG, "mg_transfer: too many rows");
    return MPBP_OK;
}

static int64_t mg_rows(int32_t n, int32_t nfields, int32_t which) {
    const int64_t m = which == MPBP_MG_P ? n : n / 2;
    return (int64_t)nfields * m * m;
}

int mpbp_mg_transfer_count(int32_t n, int32_t nfields, const int32_t* kinds, int32_t which, int32_t* row_nnz,
                           void* stream) {
    MgFields F;
    const int rc = mg_fields(n, nfields, kinds, &F);
    if (rc) return rc;
    if (!row_nnz || (which != MPBP_MG_P && which != MPBP_MG_R)) return set_error(MPBP_ERR_ARG, "mg_transfer: bad args");
    const int64_t rows = mg_rows(n, nfields, which);
    k_mg_transfer<<<grid_for(rows), kBlock, 0, as_stream(stream)>>>(F, n, which, rows, nullptr, row_nnz, nullptr, nullptr);
    MPBP_HIP(hipGetLastError());
    return MPBP_OK;
}

int mpbp_mg_transfer_fill(int32_t n, int32_t nfields, const int32_t* kinds, int32_t which, const int32_t* row_ptr,
                          int32_t* col_idx, double* val, void* stream) {
    MgFields F;
    const int rc = mg_fields(n, nfields, kinds, &F);
    if (rc) return rc;
    if (!row_ptr || !col_idx || !val || (which != MPBP_MG_P && which != MPBP_MG_R))
        return set_error(MPBP_ERR_ARG, "mg_transfer: bad args");
    const int64_t rows = mg_rows(n, nfields, which);
    k_mg_transfer<<<grid_for(rows), kBlock, 0, as_stream(stream)>>>(F, n, which, rows, row_ptr, nullptr, col_idx, val);
    MPBP_HIP(hipGetLastError());
    return MPBP_OK;
}

int mpbp_mg_transfer_rows_count(int32_t n, int32_t nfields, const int32_t* kinds, int32_t which, const int32_t* rows,
                                int32_t nrows, int32_t* row_nnz, void* stream) {
    MgFields F;
    const int rc = mg_fields(n, nfields, kinds, &F);
    if (rc) return rc;
    if (nrows < 0 || (nrows && (!rows || !row_nnz)) || (which != MPBP_MG_P && which != MPBP_MG_R))
        return set_error(MPBP_ERR_ARG, "mg_transfer_rows: bad args");
    if (nrows == 0) return MPBP_OK;
    k_mg_transfer<<<grid_for(nrows), kBlock, 0, as_stream(stream)>>>(F, n, which, nrows, nullptr, row_nnz, nullptr,
                                                                     nullptr, rows);
    MPBP_HIP(hipGetLastError());
    return MPBP_OK;
}

int mpbp_mg_transfer_rows_fill(int32_t n, int32_t nfields, const int32_t* kinds, int32_t which, const int32_t* rows,
                               int32_t nrows, const int32_t* row_ptr, int32_t* col_idx, double* val, void* stream) {
    MgFields F;
    const int rc = mg_fields(n, nfields, kinds, &F);
    if (rc) return rc;
    if (nrows < 0 || (nrows && (!rows || !row_ptr || !col_idx || !val)) || (which != MPBP_MG_P && which != MPBP_MG_R))
        return set_error(MPBP_ERR_ARG, "mg_transfer_rows: bad args");
    if (nrows == 0) return MPBP_OK;
    k_mg_transfer<<<grid_for(nrows), kBlock, 0, as_stream(stream)>>>(F, n, which, nrows, row_ptr, nullptr, col_idx, val,
                                                                     rows);
    MPBP_HIP(hipGetLastError());
    return MPBP_OK;
}

// the any-size rule's arguments: n >= 5 of either parity (nc = n / 2 >= 2)
static int mg_fields_any(int32_t n, int32_t nfields, const int32_t* kinds, MgFields* F) {
    if (n < 5 || nfields < 1 || nfields > 8 || !kinds)
        return set_error(MPBP_ERR_ARG, "mg_transfer_any: need n >= 5 and 1..8 fields");
    F->nfields = nfields;
    for (int f = 0; f < nfields; ++f) {
        F->ky[f] = kinds[2 * f];
        F->kx[f] = kinds[2 * f + 1];
        if ((F->ky[f] != MPBP_MG_CELL && F->ky[f] != MPBP_MG_NODE) || (F->kx[f] != MPBP_MG_CELL && F->kx[f] != MPBP_MG_NODE))
            return set_error(MPBP_ERR_ARG, "mg_transfer_any: field kinds must be MPBP_MG_CELL or MPBP_MG_NODE");
    }
    if ((int64_t)nfields * n * n > INT32_MAX) return set_error(MPBP_ERR_ARG, "mg_transfer_any: too many rows");
    return MPBP_OK;
}

int mpbp_mg_transfer_any_count(int32_t n, int32_t nfields, const int32_t* kinds, int32_t which, int32_t* row_nnz,
                               void* stream) {
    MgFields F;
    const int rc = mg_fields_any(n, nfields, kinds, &F);
    if (rc) return rc;
    if (!row_nnz || (which != MPBP_MG_P && which != MPBP_MG_R)) return set_error(MPBP_ERR_ARG, "mg_transfer_any: bad args");
    const int64_t rows = mg_rows(n, nfields, which);
    k_mg_transfer_any<<<grid_for(rows), kBlock, 0, as_stream(stream)>>>(F, n, which, rows, nullptr, row_nnz, nullptr, nullptr);
    MPBP_HIP(hipGetLastError());
    return MPBP_OK;
}

int mpbp_mg_transfer_any_fill(int32_t n, int32_t nfields, const int32_t* kinds, int32_t which, const int32_t* row_ptr,
                              int32_t* col_idx, double* val, void* stream) {
    MgFields F;
    const int rc = mg_fields_any(n, nfields, kinds, &F);
    if (rc) return rc;
    if (!row_ptr || !col_idx || !val || (which != MPBP_MG_P && which != MPBP_MG_R))
        return set_error(MPBP_ERR_ARG, "mg_transfer_any: bad args");
    const int64_t rows = mg_rows(n, nfields, which);
    k_mg_transfer_any<<<grid_for(rows), kBlock, 0, as_stream(stream)>>>(F, n, which, rows, row_ptr, nullptr, col_idx, val);
    MPBP_HIP(hipGetLastError());
    return MPBP_OK;
}

int mpbp_mg_accel_coeffs(double rho, int32_t K, double* omega, double* mu) {
    if (K < 1 || K > 64 || !omega || !mu || !(rho > 0.0) || !(rho < 1.0))
        return set_error(MPBP_ERR_ARG, "mg_accel_coeffs: need 1 <= K <= 64 and 0 < rho < 1");
    mg_accel_coeffs(rho, K, omega, mu);
    return MPBP_OK;
}

int mpbp_mg_combine(int64_t n, const double* y, const double* xk, const double* xold, double omega, double mu,
                    const double* sub, double* out, void* stream) {
    return mg_combine(n, y, xk, xold, omega, mu, sub, out, as_stream(stream));
}

int mpbp_mg_solve(const mpbp_mg* mg, const double* b, const double* sub, double* x_out, void* stream) {
    if (!mg || !b || !x_out || mg->nlevels < 2 || !mg->levels) return set_error(MPBP_ERR_ARG, "mg_solve: bad args");
    if (int rc = check_opts(mg->opts, "mg_solve")) return rc;
    const OptsScope scope(mg->opts);
    const mpbp_mg_level& L = mg->levels[0];
    if (check_csr(&L.A)) return MPBP_ERR_ARG;
    if (mg->part_levels < 0 || mg->part_levels >= mg->nlevels || (mg->part_levels > 0 && (!mg->halo || !mg->gather)))
        return set_error(MPBP_ERR_ARG, "mg_solve: part_levels must be in [0, nlevels) with halo and gather callbacks");
    for (int l = 0; l < mg->nlevels; ++l) {
        const mpbp_mg_level& Q = mg->levels[l];
        if (!Q.x || !Q.t || !Q.r || !Q.d || !Q.b || !Q.diag)
            return set_error(MPBP_ERR_ARG, "mg_solve: level %d is missing work vectors", l);
        // (row-partitioned levels: the transfers' columns index the ghost layout, so only the row counts are checked)
        const bool part = l < mg->part_levels;
        if (l + 1 < mg->nlevels && (Q.P.nrows != Q.nrows ||
                                    (!part && (Q.R.nrows != mg->levels[l + 1].nrows || Q.P.ncols != mg->levels[l + 1].nrows ||
                                               Q.R.ncols != Q.nrows))))
            return set_error(MPBP_ERR_ARG, "mg_solve: transfer shapes of level %d do not match", l);
    }
    const MgFine f{mg_level_op(L), L.diag, L.x, L.t, L.r, L.d, mg->part_levels > 0 ? mg->halo : nullptr, mg->halo_ctx,
                   L.halo_kind};
    return mg_solve(mg, f, b, x_out, sub, as_stream(stream));
}

// The matrix-free system matrix on one rank's rows of the row partition (StokesADev<FS, true>).  Kept last in the
// file: its kernel instances follow every other kernel in the code object.
int mpbp_stokes_apply_part(const mpbp_stokes_params* prm, const double* cell, const double* uface,
                           const double* vface, const mpbp_row_part* part, int32_t mode, const double* x,
                           const double* z, double* y, void* stream) {
    if (!part || part->halo <= 0) return mpbp_stokes_apply(prm, cell, uface, vface, mode, x, z, y, stream);
    // mpbp_stokes_apply's refusals, then the partition's; every one before the first HIP call
    if (!prm || !cell || !uface || !vface)
        return set_error(MPBP_ERR_ARG, "stokes_apply: needs the parameters and the three thn tables");
    const bool fast = (mode & MPBP_SPMV_FAST) != 0;
    mode &= ~MPBP_SPMV_FAST;
    if (mode != MPBP_SPMV_STORE && mode != MPBP_SPMV_ADD && mode != MPBP_SPMV_RESID)
        return set_error(MPBP_ERR_ARG, "stokes_apply: unknown mode %d", mode);
    if (!x || !y || x == y || (mode != MPBP_SPMV_STORE && !z))
        return set_error(MPBP_ERR_ARG, "stokes_apply: bad vectors (x, y distinct and non-null; z for ADD / RESID)");
    if (prm->n < 3) return set_error(MPBP_ERR_ARG, "stokes_apply: needs n >= 3 (n = %d)", prm->n);
    if ((int64_t)prm->n * prm->n * 5 > INT32_MAX)
        return set_error(MPBP_ERR_OVERFLOW, "stokes_apply: n = %d too large (5 n^2 > INT32_MAX)", prm->n);
    // A's output is the owned rows alone: no ghost rows computed (which = 3, ext), no output ghost depth of its own
    if (part->which < 0 || part->which > 2 || part->ext != 0)
        return set_error(MPBP_ERR_ARG, "stokes_apply_part: which = %d, ext = %d (which must be 0, 1 or 2 and ext 0: "
                         "A's output has no ghost layout)", part->which, part->ext);
    if (part->rows < 1 || part->r0 < 0 || (int64_t)part->r0 + part->rows > prm->n || part->halo > part->rows)
        return set_error(MPBP_ERR_ARG, "stokes_apply_part: bad row partition (r0 = %d, rows = %d, halo = %d, n = %d)",
                         part->r0, part->rows, part->halo, prm->n);
    if (part->oh != 0 && part->oh != part->halo)
        return set_error(MPBP_ERR_ARG, "stokes_apply_part: oh = %d must be 0 or the halo depth %d", part->oh, part->halo);
    if (((int64_t)part->rows + 2 * (int64_t)part->halo) * prm->n * 5 > INT32_MAX)
        return set_error(MPBP_ERR_OVERFLOW, "stokes_apply_part: 5 (rows + 2 halo) n > INT32_MAX");
    FStencilDev P;
    int rc = make_fstencil(prm, cell, uface, vface, part, &P);
    if (rc) return rc;
    const hipStream_t st = as_stream(stream);
    switch (mode) {
    case MPBP_SPMV_STORE: return launch_stokes_a<true>(P, prm->d_p, prm->d_div, x, EpiStore{y}, st, fast);
    case MPBP_SPMV_ADD: return launch_stokes_a<true>(P, prm->d_p, prm->d_div, x, EpiAddLate{z, y}, st, fast);
    default: return launch_stokes_a<true>(P, prm->d_p, prm->d_div, x, EpiResidLate{z, y}, st, fast);
    }
}

}  // extern "C"
