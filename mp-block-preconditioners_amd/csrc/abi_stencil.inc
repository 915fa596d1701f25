// C ABI, part 2 (part 1 is abi_core.inc): SELL, the F stencil (make_fstencil), the
// pressure stencils (make_pgstencil) and mpbp_stokes_apply.  Needs mpbp.hip's epilogues and FStencilDev, launch_march
// and with_f_policy (f_solve_w.inc), PGDev, the D / G / Gt_G policies and launch_stokes_a (pg_stencil.inc) and
// launch_sell (launchers.inc).
// A fragment of mpbp.hip, included there once and in order: not a self-contained header.

// ============================================================== SELL ABI ====
extern "C" {

int64_t mpbp_sell_plan(const int32_t* row_ptr, const int32_t* ranges, int32_t nranges, int32_t* slices,
                       int64_t capacity, int64_t* pair_rows) {
    if (!row_ptr || nranges < 0 || (nranges && !ranges)) return set_error(MPBP_ERR_ARG, "sell_plan: bad args");
    int64_t ns = 0, pr = 0;
    for (int32_t q = 0; q < nranges; ++q) {
        const int32_t a = ranges[2 * q], b = ranges[2 * q + 1];
        if (a < 0 || b < a) return set_error(MPBP_ERR_ARG, "sell_plan: bad range");
        for (int32_t r0 = a; r0 < b; r0 += 64) {
            const int32_t rows = (b - r0) < 64 ? (b - r0) : 64;
            int32_t w = 0;
            for (int32_t r = r0; r < r0 + rows; ++r) {
                const int32_t len = row_ptr[r + 1] - row_ptr[r];
                if (len > 255) return set_error(MPBP_ERR_OVERFLOW, "sell_plan: row %d has %d > 255 entries", r, len);
                w = len > w ? len : w;
            }
            if (slices && ns < capacity) {
                slices[4 * ns] = r0;
                slices[4 * ns + 1] = rows;
                slices[4 * ns + 2] = w;
                slices[4 * ns + 3] = (int32_t)pr;
            }
            pr += (w + 1) / 2;
            if (pr > INT32_MAX) return set_error(MPBP_ERR_OVERFLOW, "sell_plan: too many pair rows");
            ++ns;
        }
    }
    if (pair_rows) *pair_rows = pr;
    return ns;
}

int mpbp_sell_fill(const mpbp_csr* A, const int32_t* slices, int32_t nslices, uint8_t* row_len, double* val,
                   int32_t* col, void* stream) {
    int rc = check_csr(A);
    if (rc) return rc;
    if (nslices <= 0) return MPBP_OK;
    if (!slices || !row_len || !val || !col) return set_error(MPBP_ERR_ARG, "sell_fill: bad args");
    k_sell_fill<<<grid_for((int64_t)nslices * 64), kBlock, 0, as_stream(stream)>>>(
        to_csr(A), reinterpret_cast<const int4*>(slices), nslices, row_len, val, col);
    MPBP_HIP(hipGetLastError());
    return MPBP_OK;
}

static int check_sell(const mpbp_sell* S) {
    if (!S || S->nslices < 0 || (S->nslices && (!S->slices || !S->row_len || !S->val || !S->col)))
        return set_error(MPBP_ERR_ARG, "invalid sell matrix");
    return MPBP_OK;
}

int mpbp_sell_spmv(const mpbp_sell* S, int32_t mode, const double* x, const double* z, double* y, void* stream) {
    int rc = check_sell(S);
    if (rc) return rc;
    if (!x || !y || (mode != MPBP_SPMV_STORE && !z)) return set_error(MPBP_ERR_ARG, "sell_spmv: bad vectors");
    const hipStream_t st = as_stream(stream);
    switch (mode) {
    case MPBP_SPMV_STORE: return launch_sell(S, x, EpiStore{y}, st);
    case MPBP_SPMV_ADD: return launch_sell(S, x, EpiAdd{z, y}, st);
    case MPBP_SPMV_RESID: return launch_sell(S, x, EpiResid{z, y}, st);
    default: return set_error(MPBP_ERR_ARG, "sell_spmv: unknown mode %d", mode);
    }
}

int mpbp_sell_jacobi_step(const mpbp_sell* S, const double* x_in, const double* b, const double* diag,
                          const double* sub, double* x_out, void* stream) {
    int rc = check_sell(S);
    if (rc) return rc;
    if (!x_in || !b || !diag || !x_out || x_in == x_out) return set_error(MPBP_ERR_ARG, "sell_jacobi_step: bad vectors");
    return launch_sell(S, x_in, EpiJacobi{x_in, b, diag, sub, x_out}, as_stream(stream));
}

static int sell_cheb_impl(const mpbp_sell* S, const double* x_in, const double* b, const double* diag, double c1,
                          double c2, double* d, const double* sub, double* x_out, void* stream, int store_d) {
    int rc = check_sell(S);
    if (rc) return rc;
    if (!x_in || !b || !diag || !d || !x_out || x_in == x_out) return set_error(MPBP_ERR_ARG, "sell_cheb_step: bad vectors");
    return launch_sell(S, x_in, EpiCheb{x_in, b, diag, d, c1, c2, sub, x_out, store_d}, as_stream(stream));
}

int mpbp_sell_cheb_step(const mpbp_sell* S, const double* x_in, const double* b, const double* diag, double c1,
                        double c2, double* d, const double* sub, double* x_out, void* stream) {
    return sell_cheb_impl(S, x_in, b, diag, c1, c2, d, sub, x_out, stream, 1);
}

static int make_fstencil(const mpbp_stokes_params* prm, const double* cell, const double* uface,
                         const double* vface, const mpbp_row_part* part, FStencilDev* P) {
    if (!prm || prm->n < 3 || !cell || !uface || !vface)
        return set_error(MPBP_ERR_ARG, "f_stencil: needs n >= 3 and the three thn tables");
    if ((int64_t)prm->n * prm->n * 5 > INT32_MAX) return set_error(MPBP_ERR_OVERFLOW, "f_stencil: n too large");
    const double dx = 1.0 / prm->n;
    int r0 = 0, L = prm->n, h = 0, which = 0, ext = 0, oh = 0;
    if (part && part->halo > 0) {
        r0 = part->r0; L = part->rows; h = part->halo; which = part->which;
        ext = which == 3 ? part->ext : 0;
        oh = part->oh > 0 ? part->oh : h;
        if (L < 1 || r0 < 0 || r0 + L > prm->n || which < 0 || which > 3 || ext < 0 || ext + 1 > h || ext > oh ||
            h > L || oh > L)
            return set_error(MPBP_ERR_ARG, "f_stencil: bad row partition");
    }
    *P = FStencilDev{prm->n, prm->xi, prm->eta_n, prm->eta_s, prm->c, prm->d_u, cell, uface, vface,
                     dx * dx, 1.0 / (dx * dx), -1.0 / (dx * dx), r0, L, h, which,
                     (prm->n & (prm->n - 1)) == 0 ? 1 : 0, ext, oh};
    if (P->pow2) {   // idx2 = n^2 exactly: eta * idx2 is an exact scaling (f_row's M bit 3)
        P->ce0 = prm->eta_n * P->idx2;
        P->ce1 = prm->eta_s * P->idx2;
    }
    return MPBP_OK;
}

}  // extern "C"

namespace {
template <class Epi>
int launch_fstencil(const FStencilDev& P, const double* x, Epi epi, hipStream_t st, bool fast = false) {
    return with_f_policy(P, fast, [&](const auto& Q) { return launch_march(Q, XPlain{x}, epi, KO().march_rows, st); });
}

}  // namespace

extern "C" {

int mpbp_f_stencil_spmv(const mpbp_stokes_params* prm, const double* cell, const double* uface,
                        const double* vface, const mpbp_row_part* part, int32_t mode, const double* x,
                        const double* z, double* y, void* stream) {
    FStencilDev P;
    int rc = make_fstencil(prm, cell, uface, vface, part, &P);
    if (rc) return rc;
    const bool fast = (mode & MPBP_SPMV_FAST) != 0;
    mode &= ~MPBP_SPMV_FAST;
    if (!x || !y || (mode != MPBP_SPMV_STORE && !z)) return set_error(MPBP_ERR_ARG, "f_stencil_spmv: bad vectors");
    const hipStream_t st = as_stream(stream);
    switch (mode) {
    case MPBP_SPMV_STORE: return launch_fstencil(P, x, EpiStore{y}, st, fast);
    case MPBP_SPMV_ADD: return launch_fstencil(P, x, EpiAdd{z, y}, st, fast);
    case MPBP_SPMV_RESID: return launch_fstencil(P, x, EpiResid{z, y}, st, fast);
    default: return set_error(MPBP_ERR_ARG, "f_stencil_spmv: unknown mode %d", mode);
    }
}

static int f_stencil_jacobi_impl(const mpbp_stokes_params* prm, const double* cell, const double* uface,
                                 const double* vface, const mpbp_row_part* part, const double* x_in,
                                 const double* b, const double* sub, double* x_out, void* stream, bool fast) {
    FStencilDev P;
    int rc = make_fstencil(prm, cell, uface, vface, part, &P);
    if (rc) return rc;
    if (!x_in || !b || !x_out || x_in == x_out) return set_error(MPBP_ERR_ARG, "f_stencil_jacobi_step: bad vectors");
    return launch_fstencil(P, x_in, EpiJacobi{x_in, b, nullptr, sub, x_out}, as_stream(stream), fast);
}

int mpbp_f_stencil_jacobi_step(const mpbp_stokes_params* prm, const double* cell, const double* uface,
                               const double* vface, const mpbp_row_part* part, const double* x_in,
                               const double* b, const double* sub, double* x_out, void* stream) {
    return f_stencil_jacobi_impl(prm, cell, uface, vface, part, x_in, b, sub, x_out, stream, false);
}

static int f_stencil_cheb_impl(const mpbp_stokes_params* prm, const double* cell, const double* uface,
                               const double* vface, const mpbp_row_part* part, const double* x_in,
                               const double* b, double c1, double c2, double* d, const double* sub,
                               double* x_out, void* stream, int store_d, bool fast = false) {
    FStencilDev P;
    int rc = make_fstencil(prm, cell, uface, vface, part, &P);
    if (rc) return rc;
    if (!x_in || !b || !d || !x_out || x_in == x_out) return set_error(MPBP_ERR_ARG, "f_stencil_cheb_step: bad vectors");
    return launch_fstencil(P, x_in, EpiCheb{x_in, b, nullptr, d, c1, c2, sub, x_out, store_d}, as_stream(stream),
                           fast);
}

int mpbp_f_stencil_cheb_step(const mpbp_stokes_params* prm, const double* cell, const double* uface,
                             const double* vface, const mpbp_row_part* part, const double* x_in,
                             const double* b, double c1, double c2, double* d, const double* sub,
                             double* x_out, void* stream) {
    return f_stencil_cheb_impl(prm, cell, uface, vface, part, x_in, b, c1, c2, d, sub, x_out, stream, 1);
}

static int make_pgstencil(const mpbp_stokes_params* prm, const double* cell, const mpbp_row_part* part, PGDev* P) {
    if (!prm || prm->n < 3 || !cell) return set_error(MPBP_ERR_ARG, "pg_stencil: needs n >= 3 and the cell thn table");
    if ((int64_t)prm->n * prm->n * 5 > INT32_MAX) return set_error(MPBP_ERR_OVERFLOW, "pg_stencil: n too large");
    const double dx = 1.0 / prm->n;   // as phase_D_row / phase_G_row evaluate 1.0 / dx, -1.0 / dx
    int r0 = 0, L = prm->n, h = 0, which = 0, ext = 0, oh = 0;
    if (part && part->halo > 0) {
        r0 = part->r0; L = part->rows; h = part->halo; which = part->which;
        ext = which == 3 ? part->ext : 0;
        oh = part->oh > 0 ? part->oh : h;
        if (L < 1 || r0 < 0 || r0 + L > prm->n || which < 0 || which > 3 || ext < 0 || ext + 1 > h || ext > oh ||
            h > L || oh > L)
            return set_error(MPBP_ERR_ARG, "pg_stencil: bad row partition");
    }
    *P = PGDev{prm->n, cell, prm->d_p, 1.0 / dx, -1.0 / dx, r0, L, h, which, ext, oh};
    P->unit = P->d_p == 1.0 && P->minv == -P->inv;
    return MPBP_OK;
}

}  // extern "C"

namespace {
template <class S>
int pg_spmv(const S& P, int32_t mode, const double* x, const double* z, double* y, hipStream_t st) {
    switch (mode) {
    case MPBP_SPMV_STORE: return launch_march(P, XPlain{x}, EpiStore{y}, pg_rows(), st);
    case MPBP_SPMV_ADD: return launch_march(P, XPlain{x}, EpiAdd{z, y}, pg_rows(), st);
    case MPBP_SPMV_RESID: return launch_march(P, XPlain{x}, EpiResid{z, y}, pg_rows(), st);
    default: return set_error(MPBP_ERR_ARG, "pg_stencil_spmv: unknown mode %d", mode);
    }
}
}  // namespace

extern "C" {

int mpbp_pg_stencil_spmv(const mpbp_stokes_params* prm, const double* cell, const mpbp_row_part* part, int32_t op,
                         int32_t mode, const double* x, const double* z, double* y, void* stream) {
    PGDev P;
    int rc = make_pgstencil(prm, cell, part, &P);
    if (rc) return rc;
    if (!x || !y || x == y || (mode != MPBP_SPMV_STORE && !z)) return set_error(MPBP_ERR_ARG, "pg_stencil_spmv: bad vectors");
    const hipStream_t st = as_stream(stream);
    switch (op) {
    case MPBP_PG_D: return pg_spmv(DStencilDev{P}, mode, x, z, y, st);
    case MPBP_PG_G: return pg_spmv(GStencilDev{P}, mode, x, z, y, st);
    case MPBP_PG_GTG: return pg_spmv(GtGStencilDev{P}, mode, x, z, y, st);
    default: return set_error(MPBP_ERR_ARG, "pg_stencil_spmv: unknown operator %d", op);
    }
}

int mpbp_stokes_apply(const mpbp_stokes_params* prm, const double* cell, const double* uface, const double* vface,
                      int32_t mode, const double* x, const double* z, double* y, void* stream) {
    // every refusal comes before the first HIP call
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
    FStencilDev P;
    int rc = make_fstencil(prm, cell, uface, vface, nullptr, &P);
    if (rc) return rc;
    const hipStream_t st = as_stream(stream);
    switch (mode) {
    case MPBP_SPMV_STORE: return launch_stokes_a<false>(P, prm->d_p, prm->d_div, x, EpiStore{y}, st, fast);
    case MPBP_SPMV_ADD: return launch_stokes_a<false>(P, prm->d_p, prm->d_div, x, EpiAddLate{z, y}, st, fast);
    default: return launch_stokes_a<false>(P, prm->d_p, prm->d_div, x, EpiResidLate{z, y}, st, fast);
    }
}

int mpbp_gtg_stencil_jacobi_step(const mpbp_stokes_params* prm, const double* cell, const mpbp_row_part* part,
                                 const double* x_in, const double* b, const double* sub, double* x_out,
                                 void* stream) {
    PGDev P;
    int rc = make_pgstencil(prm, cell, part, &P);
    if (rc) return rc;
    if (!x_in || !b || !x_out || x_in == x_out) return set_error(MPBP_ERR_ARG, "gtg_stencil_jacobi_step: bad vectors");
    return launch_march(GtGStencilDev{P}, XPlain{x_in}, EpiJacobi{x_in, b, nullptr, sub, x_out}, pg_rows(),
                        as_stream(stream));
}

// dzero: d is +0.0 (a restart: multigrid post-smoothing), read as such instead of loaded -- no memset launch
static int gtg_stencil_cheb_impl(const mpbp_stokes_params* prm, const double* cell, const mpbp_row_part* part,
                                 const double* x_in, const double* b, double c1, double c2, double* d,
                                 const double* sub, double* x_out, void* stream, int store_d, bool dzero = false) {
    PGDev P;
    int rc = make_pgstencil(prm, cell, part, &P);
    if (rc) return rc;
    if (!x_in || !b || !d || !x_out || x_in == x_out) return set_error(MPBP_ERR_ARG, "gtg_stencil_cheb_step: bad vectors");
    const EpiCheb e{x_in, b, nullptr, d, c1, c2, sub, x_out, store_d};
    if (dzero) return launch_march(GtGStencilDev{P}, XPlain{x_in}, EpiZeroD<EpiCheb>{e}, pg_rows(), as_stream(stream));
    return launch_march(GtGStencilDev{P}, XPlain{x_in}, e, pg_rows(), as_stream(stream));
}

int mpbp_gtg_stencil_cheb_step(const mpbp_stokes_params* prm, const double* cell, const mpbp_row_part* part,
                               const double* x_in, const double* b, double c1, double c2, double* d,
                               const double* sub, double* x_out, void* stream) {
    return gtg_stencil_cheb_impl(prm, cell, part, x_in, b, c1, c2, d, sub, x_out, stream, 1);
}

}  // extern "C"
