// Small kernels and the host launchers of the stored-matrix paths: k_sell_fill, k_jacobi_init / k_cheb_init,
// to_csr, launch_rows, launch_grp and the grp_* forms, k_grp_rr (small multigrid levels with their transfers folded
// in), the stencil-values-layout, segmented and SELL launchers, check_csr, cheb_coeffs and spgemm_count / spgemm_fill.
// Needs mpbp.hip's prelude and its SpGEMM, multigrid-transfer, epilogue and SpMV sections, and XPlain / XInit.
// A fragment of mpbp.hip, included there once and in order: not a self-contained header.

namespace {

// One thread per (slice, lane): copy the CSR row into its column-major slots.
__global__ void k_sell_fill(Csr A, const int4* slices, int nslices, uint8_t* rlen, double* val, int32_t* col) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int sidx = (int)(t >> 6), lane = (int)(t & 63);
    if (sidx >= nslices) return;
    const int4 sl = slices[sidx];
    if (lane >= sl.y) return;
    const int32_t r = sl.x + lane;
    const int32_t k0 = A.rp[r], len = A.rp[r + 1] - k0;
    rlen[r] = (uint8_t)len;
    for (int k = 0; k < len; ++k) {
        const size_t slot = ((size_t)sl.w + (k >> 1)) * 64 + lane;
        val[2 * slot + (k & 1)] = A.va[k0 + k];
        col[2 * slot + (k & 1)] = A.ci[k0 + k];
    }
}

__global__ void k_jacobi_init(int32_t n, const double* b, const double* diag, const double* sub,
                              double* xout) {
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const double x = b[r] / diag[r];
    xout[r] = sub ? sub[r] - x : x;
}

__global__ void k_cheb_init(int32_t n, const double* b, const double* diag, double c2, double* d,
                            const double* sub, double* xout) {
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const double z = b[r] / diag[r];
    const double dn = c2 * z;
    d[r] = dn;
    xout[r] = sub ? sub[r] - dn : dn;
}

inline Csr to_csr(const mpbp_csr* A) { return Csr{A->row_ptr, A->col_idx, A->val, A->ncols}; }

template <class Epi>
int launch_rows(const mpbp_csr* A, const mpbp_rowblocks* blk, const double* x, Epi epi, hipStream_t st) {
    if (!blk || blk->count <= 0) return MPBP_OK;
    k_csr_wave<Epi><<<blk->count, kBlock, 0, st>>>(to_csr(A), x, reinterpret_cast<const int2*>(blk->pairs),
                                                    blk->count, KO().csr_table ? blk->table : nullptr, epi);
    MPBP_HIP(hipGetLastError());
    return MPBP_OK;
}
// Small-level CSR products through k_csr_grp: lanes per row from the mean row length (2: <= 16 entries, 4: <= 32,
// 8: longer), so one chunk holds a multigrid coarse row (transfers 1-16 entries, Galerkin levels 20-46).
template <class Epi, class XS = XPlain>
int launch_grp(const mpbp_csr* A, const XS& xs, Epi epi, hipStream_t st) {
    if (A->nrows <= 0) return MPBP_OK;
    const int64_t avg = A->nnz / A->nrows;
    auto go = [&](auto gc) {
        constexpr int G = decltype(gc)::value;
        constexpr int rpb = kBlock / G;
        k_csr_grp<G, XS, Epi><<<(unsigned)((A->nrows + rpb - 1) / rpb), kBlock, 0, st>>>(to_csr(A), A->nrows, xs, epi);
        MPBP_HIP(hipGetLastError());
        return (int)MPBP_OK;
    };
    return avg <= 16 ? go(std::integral_constant<int, 2>{})
                     : avg <= 32 ? go(std::integral_constant<int, 4>{}) : go(std::integral_constant<int, 8>{});
}
inline bool use_grp(const mpbp_csr& A) { return KO().mg_group_rows > 0 && A.nrows > 0 && A.nrows <= KO().mg_group_rows && A.nnz > 0; }
int grp_spmv(const mpbp_csr* A, int32_t mode, const double* x, const double* z, double* y, hipStream_t st) {
    const XPlain xs{x};
    switch (mode) {
    case MPBP_SPMV_STORE: return launch_grp(A, xs, EpiStore{y}, st);
    case MPBP_SPMV_ADD: return launch_grp(A, xs, EpiAdd{z, y}, st);
    case MPBP_SPMV_RESID: return launch_grp(A, xs, EpiResid{z, y}, st);
    default: return set_error(MPBP_ERR_ARG, "grp_spmv: unknown mode %d", mode);
    }
}
int grp_cheb(const mpbp_csr* A, const double* xin, const double* b, const double* dg, double c1, double c2, double* d,
             const double* sub, double* xo, hipStream_t st, int store_d, bool dzero) {
    const EpiCheb e{xin, b, dg, d, c1, c2, sub, xo, store_d};
    const XPlain xs{xin};
    return dzero ? launch_grp(A, xs, EpiZeroD<EpiCheb>{e}, st) : launch_grp(A, xs, e, st);
}
// First sweep from x = 0: x0 = d0 = c2_0 b / diag folded in (no k_cheb_init launch, same bits).
int grp_cheb_first(const mpbp_csr* A, const double* b, const double* dg, double c2_0, double c1, double c2, double* d,
                   const double* sub, double* xo, hipStream_t st, int store_d) {
    EpiChebFirstGrp e;
    static_cast<EpiChebFirst&>(e) = EpiChebFirst{b, d, c1, c2, sub, xo, store_d};
    e.diag = dg;
    e.c2_0 = c2_0;
    return launch_grp(A, XInit{b, dg, c2_0}, e, st);
}

// ---- small multigrid levels with their transfers folded in (kernel option mg_fuse_small) ----
// b_c = R (b - A x) in one launch, one wave per coarse row I: four lanes per fine row of R's row (<= 4 x 4 of them)
// gather that row's CSR entries at once and the slot's first lane adds the products left to right from 0.0 (k_csr_grp's
// sum) and forms b_j - sum (EpiResid); the wave's first lane then adds R's products (yw xw) r_j in list order
// (k_mg_transfer_spmv's restriction).  The residual and restriction launches' operations, bit for bit, without r's
// store and reload.  A fine row shared by neighbouring coarse rows is recomputed by each (up to 4x), so it pays only
// where the two launches are latency-bound: coarse levels of <= kRrMaxCoarse rows (1024^2, mg:1, profiles/
// r06l_mg_apply_kernel_trace.md: 7.3 vs 5.0 + 4.9 us into 1024 coarse rows, 6.6 vs ~9.8 into 256; into 4096, 10.4 vs
// 5.1 + 4.9; into 16384, 32 vs 11 + 5).  Folding the prolongation into the first post-smoothing sweep's gathers
// (x + P x_c per gathered column: five loads instead of one) measured slower than its two launches at every level
// (10-31 vs 9-17 us) and is not kept.
constexpr int32_t kRrMaxCoarse = 1024;
constexpr int kRrL = 4, kRrJ = 12, kRrCap = kRrL * kRrJ;   // lanes per fine row, entries per lane and chunk
__device__ inline int sel4(const int* v, int i) { return i == 0 ? v[0] : i == 1 ? v[1] : i == 2 ? v[2] : v[3]; }
__global__ void __launch_bounds__(kBlock) k_grp_rr(Csr A, MgFields F, MgDiv dv, int32_t n, int32_t ncr,
                                                  const double* __restrict__ x, const double* __restrict__ b,
                                                  double* __restrict__ bc) {
    constexpr int WPB = kBlock / 64;
    __shared__ double prod[WPB * 16 * kRrCap];
    __shared__ double rs[WPB * 16];
    const int w = threadIdx.x / 64, lane = threadIdx.x % 64, s = lane / kRrL, k = lane % kRrL;
    const int32_t I = blockIdx.x * WPB + w;   // wave-uniform: a wave past the last coarse row leaves whole
    if (I >= ncr) return;
    MgRow R;
    mg_row(F, dv, n, MPBP_MG_R, I, R);
    const bool live = s < R.my * R.mx;
    const int a = live ? (s >= R.mx) + (s >= 2 * R.mx) + (s >= 3 * R.mx) : 0, c = s - a * R.mx;
    const int32_t j = live ? R.off + sel4(R.yi, a) * n + sel4(R.xi, c) : 0;
    const int32_t ks = A.rp[j], ke = live ? A.rp[j + 1] : ks;
    const double bj = (live && k == 0) ? b[j] : 0.0;
    double* pr = prod + (w * 16 + s) * kRrCap;
    double acc = 0.0;
    for (int32_t cb = ks; cb < ke; cb += kRrCap) {
        double v[kRrJ];
        int32_t ci[kRrJ];
#pragma unroll
        for (int u = 0; u < kRrJ; ++u) {
            const int32_t e = cb + k + kRrL * u;
            const bool in = e < ke;
            v[u] = in ? A.va[e] : 0.0;
            ci[u] = in ? A.ci[e] : 0;
        }
        double p[kRrJ];
#pragma unroll
        for (int u = 0; u < kRrJ; ++u) p[u] = v[u] * x[ci[u]];
        if (cb != ks) wave_lds_sync();   // the previous chunk's sums have read their slots
#pragma unroll
        for (int u = 0; u < kRrJ; ++u) pr[k + kRrL * u] = p[u];
        wave_lds_sync();
        if (k == 0) {
            const int32_t cnt = min(ke - cb, (int32_t)kRrCap);
            for (int32_t e = 0; e < cnt; ++e) acc += pr[e];
        }
    }
    if (live && k == 0) rs[w * 16 + s] = bj - acc;
    wave_lds_sync();
    if (lane == 0) {
        double r = 0.0;
#pragma unroll
        for (int ya = 0; ya < 4; ++ya)
#pragma unroll
            for (int xb = 0; xb < 4; ++xb)
                if (ya < R.my && xb < R.mx) r += (R.yw[ya] * R.xw[xb]) * rs[w * 16 + ya * R.mx + xb];
        bc[I] = r;
    }
}

// Products through the stencil-values layout (k_svl).
inline Svl to_svl(const mpbp_svl* V) {
    return Svl{V->nfields, V->m, V->reach, V->slots, V->delta, V->vals, V->edge_rows, V->n_edge};
}
int check_svl(const mpbp_svl* V, const mpbp_csr* A) {
    if (!V || !A || V->slots < 1 || V->nfields < 1 || V->nfields * V->slots > kSvMaxDelta || V->reach < 0 ||
        V->m < 2 * V->reach + 2 || (V->m & 1) || (V->reach & 1) || (int64_t)V->nfields * V->m * V->m != A->nrows ||
        (int64_t)V->slots * A->nrows > INT32_MAX || !V->delta || !V->vals ||
        V->n_edge < 0 || (V->n_edge && !V->edge_rows))
        return set_error(MPBP_ERR_ARG, "svl: layout does not match the operator");
    return MPBP_OK;
}
template <class Epi, class XS = XPlain>
int launch_svl(const mpbp_svl* V, const mpbp_csr* A, const XS& xs, Epi epi, hipStream_t st) {
    const int64_t w = V->m - 2 * V->reach;
    const int64_t per = (w / 2) * w;
    const int64_t threads = (((int64_t)V->n_edge * kSvEdgeG + kBlock - 1) / kBlock) * kBlock + V->nfields * per;
    if (threads <= 0) return MPBP_OK;
    k_svl<XS, Epi><<<(unsigned)((threads + kBlock - 1) / kBlock), kBlock, 0, st>>>(to_svl(V), to_csr(A), A->nrows, xs,
                                                                                    epi);
    MPBP_HIP(hipGetLastError());
    return MPBP_OK;
}
int svl_spmv(const mpbp_svl* V, const mpbp_csr* A, int32_t mode, const double* x, const double* z, double* y,
             hipStream_t st) {
    const XPlain xs{x};
    switch (mode) {
    case MPBP_SPMV_STORE: return launch_svl(V, A, xs, EpiStore{y}, st);
    case MPBP_SPMV_ADD: return launch_svl(V, A, xs, EpiAdd{z, y}, st);
    case MPBP_SPMV_RESID: return launch_svl(V, A, xs, EpiResid{z, y}, st);
    default: return set_error(MPBP_ERR_ARG, "svl_spmv: unknown mode %d", mode);
    }
}
int svl_cheb(const mpbp_svl* V, const mpbp_csr* A, const double* xin, const double* b, const double* dg, double c1,
             double c2, double* d, const double* sub, double* xo, hipStream_t st, int store_d, bool dzero) {
    const EpiCheb e{xin, b, dg, d, c1, c2, sub, xo, store_d};
    const XPlain xs{xin};
    return dzero ? launch_svl(V, A, xs, EpiZeroD<EpiCheb>{e}, st) : launch_svl(V, A, xs, e, st);
}
template <class Epi>
int launch_rows_seg(const mpbp_csr* A, const mpbp_rowblocks* blk, const double* x, Epi epi, hipStream_t st) {
    if (!blk || blk->count <= 0) return MPBP_OK;
    k_csr_seg<Epi><<<blk->count, kBlock, 0, st>>>(to_csr(A), x, reinterpret_cast<const int2*>(blk->pairs),
                                                   blk->count, epi);
    MPBP_HIP(hipGetLastError());
    return MPBP_OK;
}

template <class Epi>
int launch_sell(const mpbp_sell* S, const double* x, Epi epi, hipStream_t st) {
    if (!S || S->nslices <= 0) return MPBP_OK;
    const int slices_per_block = kBlock / 64;
    const int grid = (S->nslices + slices_per_block - 1) / slices_per_block;
    k_sell_rows<Epi><<<grid, kBlock, 0, st>>>(
        Sell{reinterpret_cast<const int4*>(S->slices), S->row_len, reinterpret_cast<const double2*>(S->val),
             reinterpret_cast<const int2*>(S->col)},
        x, S->nslices, epi);
    MPBP_HIP(hipGetLastError());
    return MPBP_OK;
}

int check_csr(const mpbp_csr* A) {
    if (!A || !A->row_ptr || A->nrows < 0) return set_error(MPBP_ERR_ARG, "invalid csr");
    if (A->nnz > 0 && (!A->col_idx || !A->val)) return set_error(MPBP_ERR_ARG, "csr without entries");
    return MPBP_OK;
}

// Chebyshev-Jacobi coefficients (Saad, Iterative Methods, Alg. 12.1 with diag(A)^-1 preconditioning).
void cheb_coeffs(double lmin, double lmax, int sweeps, double* c1, double* c2) {
    const double theta = (lmax + lmin) / 2.0;
    const double delta = (lmax - lmin) / 2.0;
    const double sigma = theta / delta;
    double rho = 1.0 / sigma;
    c1[0] = 0.0;
    c2[0] = 1.0 / theta;
    for (int s = 1; s < sweeps; ++s) {
        const double rho_new = 1.0 / (2.0 * sigma - rho);
        c1[s] = rho_new * rho;
        c2[s] = 2.0 * rho_new / delta;
        rho = rho_new;
    }
}

}  // namespace

// C = alpha A B's two passes with output rows up to W entries (mpbp_spgemm_count / _fill and their wide forms)
namespace {
template <int W>
int spgemm_count(const mpbp_csr* A, const mpbp_csr* B, int32_t* row_nnz, void* stream) {
    int rc = check_csr(A);
    if (!rc) rc = check_csr(B);
    if (rc) return rc;
    if (A->ncols != B->nrows) return set_error(MPBP_ERR_ARG, "spgemm: shape mismatch");
    int* d_over = nullptr;
    MPBP_HIP(hipMalloc(&d_over, sizeof(int)));
    hipError_t e = hipMemsetAsync(d_over, 0, sizeof(int), as_stream(stream));
    if (e == hipSuccess) {
        k_spgemm_count<W><<<grid_for(A->nrows), kBlock, 0, as_stream(stream)>>>(to_csr(A), to_csr(B), A->nrows,
                                                                             row_nnz, d_over);
        e = hipGetLastError();
    }
    int h = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&h, d_over, sizeof(int), hipMemcpyDeviceToHost, as_stream(stream));
    if (e == hipSuccess) e = hipStreamSynchronize(as_stream(stream));
    (void)hipFree(d_over);
    if (e != hipSuccess) return set_error(MPBP_ERR_HIP, "spgemm_count: %s", hipGetErrorString(e));
    if (h) return set_error(MPBP_ERR_OVERFLOW, "spgemm: %d rows wider than %d", h, W);
    return MPBP_OK;
}

template <int W>
int spgemm_fill(const mpbp_csr* A, const mpbp_csr* B, double alpha, const int32_t* row_ptr, int32_t* col_idx,
                double* val, void* stream) {
    int rc = check_csr(A);
    if (!rc) rc = check_csr(B);
    if (rc) return rc;
    k_spgemm_fill<W><<<grid_for(A->nrows), kBlock, 0, as_stream(stream)>>>(to_csr(A), to_csr(B), A->nrows, alpha,
                                                                        row_ptr, col_idx, val);
    MPBP_HIP(hipGetLastError());
    return MPBP_OK;
}
}  // namespace
