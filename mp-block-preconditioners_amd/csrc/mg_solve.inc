// The geometric multigrid inner solve (MPBP_INNER_MG): MgFine, the level operators and transfers (mg_fields,
// mg_transfer_mf), the dense coarsest level (k_dense_cm), mg_smooth, the fused level-0 launchers and mg_vcycle.
// Continues schur_ops.inc's namespace; needs it and what it names.
// A fragment of mpbp.hip, included there once and in order: not a self-contained header.
namespace {

// ---- geometric multigrid inner solve (MPBP_INNER_MG) ----
// The reference's own pointer for these inverses: "In IBAMR, we'd use Multigrid PC with Jacobi smoother"
// (solve.py:266, 274).  V-cycles over the levels of an mpbp_mg hierarchy (Galerkin coarse operators
// R A P, mpbp_mg_transfer_*): Chebyshev-Jacobi pre- and post-smoothing on each level, the coarsest level solved
// by its dense (pseudo-)inverse.  Every step is an existing apply-path kernel (SpMV epilogues, Chebyshev
// steps), so the cycle is graph-capturable and its operation order is the oracle's (oracle/mg_oracle.py).
// Level 0 can be any operator of the plan (matrix-free stencil, SELL or CSR: the same bits).
struct MgFine {
    OpPair op;               // level 0's operator (interior + boundary rows under a row partition)
    const double* diag;
    double *x, *t, *r, *d;   // two iterate buffers, residual, Chebyshev direction
    mpbp_halo_fn halo;       // level 0's ghost-row exchange (NULL: one GPU)
    void* hctx;
    int32_t kind;
};

int pair_spmv(const OpPair& o, int32_t mode, const double* x, const double* z, double* y, hipStream_t st) {
    const int rc = op_spmv(o.in, mode, x, z, y, st);
    return rc ? rc : op_spmv(o.bd, mode, x, z, y, st);
}
int pair_cheb(const OpPair& o, const double* xin, const double* b, const double* dg, double c1, double c2, double* d,
              const double* sub, double* xo, hipStream_t st, int store_d, bool dzero = false) {
    const int rc = op_cheb(o.in, xin, b, dg, c1, c2, d, sub, xo, st, store_d, dzero);
    return rc ? rc : op_cheb(o.bd, xin, b, dg, c1, c2, d, sub, xo, st, store_d, dzero);
}

OpRef mg_csr_op(const mpbp_csr& A, const mpbp_rowblocks& blk) {
    return OpRef{&A, &blk, nullptr, nullptr, false, 0, SOP_NONE};
}
// A level's operator: its SELL-64 copy when it has one (same bits), else the CSR form.
OpPair mg_level_op(const mpbp_mg_level& L) {
    const OpRef none{nullptr, nullptr, nullptr, nullptr, true, 0, SOP_NONE};
    if (use_grp(L.A)) return OpPair{OpRef{&L.A, &L.A_blocks, nullptr, nullptr, false, 0, SOP_NONE, 0, 1}, none};
    if (L.A_svl && KO().mg_svl)
        return OpPair{OpRef{&L.A, &L.A_blocks, nullptr, nullptr, false, 0, SOP_NONE, 0, 0, L.A_svl}, none};
    return OpPair{L.A_sell.nslices > 0 ? OpRef{&L.A, nullptr, &L.A_sell, nullptr, false, 0, SOP_NONE}
                                       : mg_csr_op(L.A, L.A_blocks), none};
}
// Ghost rows of a level-l vector (row-partitioned levels l < part_levels; level 0 through the caller's halo).
void mg_exchange(const mpbp_mg* m, int l, const MgFine& f, double* x, hipStream_t st) {
    if (l == 0) {
        if (f.halo) {
            f.halo(f.hctx, f.kind, x, MPBP_HALO_BEGIN, (void*)st);
            f.halo(f.hctx, f.kind, x, MPBP_HALO_END, (void*)st);
        }
        return;
    }
    if (l < m->part_levels && m->halo) {
        m->halo(m->halo_ctx, m->levels[l].halo_kind, x, MPBP_HALO_BEGIN, (void*)st);
        m->halo(m->halo_ctx, m->levels[l].halo_kind, x, MPBP_HALO_END, (void*)st);
    }
}
MgFields mg_fields(const mpbp_mg* m) {
    MgFields F{};
    F.nfields = m->tr_nfields;
    for (int f = 0; f < m->tr_nfields; ++f) {
        F.ky[f] = m->tr_ky[f];
        F.kx[f] = m->tr_kx[f];
    }
    return F;
}
inline MgDiv mg_div(int32_t nr) { return MgDiv{divu((uint32_t)nr * (uint32_t)nr), divu((uint32_t)nr)}; }
// Level l's restriction (which = MPBP_MG_R) or prolongation (MPBP_MG_P) matrix-free when the hierarchy names its
// field kinds and the level is whole-grid (not row-partitioned); 1: launched, 0: not applicable.
// Level l's size is tr_n0 >> l under either coarsening rule (floor halving).  An even level takes the 2:1 lists
// (k_mg_transfer_spmv), an odd one -- coarsen="any" hierarchies only -- the any-size lists (k_mg_transfer_any_spmv).
template <class Epi>
int mg_transfer_mf(const mpbp_mg* m, int l, int32_t which, int32_t nrows, const double* x, Epi epi, hipStream_t st) {
    const int32_t n = m->tr_n0 >> l, nr = which == MPBP_MG_P ? n : n / 2;
    if (n & 1)
        k_mg_transfer_any_spmv<Epi><<<grid_for(nrows), kBlock, 0, st>>>(mg_fields(m), mg_div(nr), n, which, nrows, x, epi);
    else
        k_mg_transfer_spmv<Epi><<<grid_for(nrows), kBlock, 0, st>>>(mg_fields(m), mg_div(nr), n, which, nrows, x, epi);
    MPBP_HIP(hipGetLastError());
    return MPBP_OK;
}
inline bool mg_level_even(const mpbp_mg* m, int l) { return ((m->tr_n0 >> l) & 1) == 0; }
inline bool use_mf_transfer(const mpbp_mg* m, int l) {
    const int32_t n = m->tr_n0 >> l;
    return KO().mg_mf_transfer && m->tr_nfields > 0 && m->tr_nfields <= 8 && l >= m->part_levels && n >= 4 &&
           (mg_level_even(m, l) || (n >= 5 && n <= kMgAnyMaxN));
}
// Kernel option mg_fuse_small (k_grp_rr): level l >= 1 of a hierarchy held whole on this GPU (one GPU, or a level every
// rank replicates), its operator on k_csr_grp rows, its transfers matrix-free with the level sizes the transfers imply,
// the coarse level at most kRrMaxCoarse rows.  An even level only: k_grp_rr builds the 2:1 restriction lists (<= 16 fine
// rows per coarse row).
bool mg_small_ok(const mpbp_mg* m, int l, const OpPair& o) {
    if (!KO().mg_fuse_small || l < 1 || l < m->part_levels || l + 1 >= m->nlevels || !o.in.grp || !o.in.csr ||
        o.in.gal || !o.bd.empty || !use_mf_transfer(m, l) || !mg_level_even(m, l))
        return false;
    const int64_t n = m->tr_n0 >> l, rows = (int64_t)m->tr_nfields * n * n;
    const mpbp_csr& A = *o.in.csr;
    return A.nrows == rows && A.ncols == rows && m->levels[l].nrows == rows && m->levels[l + 1].nrows == rows / 4 &&
           rows / 4 <= kRrMaxCoarse;
}
int launch_grp_rr(const mpbp_mg* m, int l, const mpbp_csr* A, const double* x, const double* b, double* bc,
                  hipStream_t st) {
    const int32_t n = m->tr_n0 >> l, ncr = m->tr_nfields * (n / 2) * (n / 2);
    constexpr int WPB = kBlock / 64;
    k_grp_rr<<<(unsigned)((ncr + WPB - 1) / WPB), kBlock, 0, st>>>(to_csr(A), mg_fields(m), mg_div(n / 2), n, ncr, x, b,
                                                                 bc);
    MPBP_HIP(hipGetLastError());
    return MPBP_OK;
}
int mg_transfer(const mpbp_csr& M, const mpbp_rowblocks& blk, const mpbp_sell& S, int32_t mode, const double* x,
                const double* z, double* y, hipStream_t st) {
    if (use_grp(M)) return grp_spmv(&M, mode, x, z, y, st);
    return S.nslices > 0 ? mpbp_sell_spmv(&S, mode, x, z, y, (void*)st) : mpbp_spmv(&M, &blk, mode, x, z, y, (void*)st);
}

// y = M b for the coarsest level's dense (pseudo-)inverse, column-major (Mt[j * m + i] = M[i][j]).  A workgroup
// owns kDR rows: its 1024 threads request a kDK-column slab of them at once (16 loads each, all in flight), form
// the slab's products with b in LDS, then one lane per row adds them over the columns in order from 0.0 -- the CSR
// row's order with every entry stored (bit-identical to the CSR form of the same inverse).
constexpr int kDR = 16, kDK = 1024, kDT = 1024;
__global__ void __launch_bounds__(kDT) k_dense_cm(int32_t m, const double* __restrict__ Mt,
                                                  const double* __restrict__ b, double* __restrict__ y) {
    __shared__ double tile[kDK * kDR];   // [column][row]
    __shared__ double bs[kDK];
    const int32_t r0 = blockIdx.x * kDR;
    const int t = threadIdx.x;
    double acc = 0.0;
    for (int32_t j0 = 0; j0 < m; j0 += kDK) {
        const int kc = min(kDK, m - j0);
        constexpr int U = kDK * kDR / kDT;
        double v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int e = t + kDT * u, c = e / kDR, row = r0 + e % kDR;
            v[u] = (c < kc && row < m) ? Mt[(size_t)(j0 + c) * m + row] : 0.0;
        }
        const double bv = t < kc ? b[j0 + t] : 0.0;
        bs[t] = bv;
        __syncthreads();
        // the slab's products M[row][col] * b[col] formed by all 1024 threads at once, so the summing lanes' loop is
        // LDS reads and dependent adds only (22 -> ~6 us for the 1024-row coarsest F level)
#pragma unroll
        for (int u = 0; u < U; ++u) tile[t + kDT * u] = v[u] * bs[(t + kDT * u) / kDR];
        __syncthreads();
        if (t < kDR) {   // 32 LDS reads in flight ahead of each run of dependent adds (same order)
            int c = 0;
            for (; c + 32 <= kc; c += 32) {
                double q[32];
#pragma unroll
                for (int u = 0; u < 32; ++u) q[u] = tile[(c + u) * kDR + t];
#pragma unroll
                for (int u = 0; u < 32; ++u) acc += q[u];
            }
            for (; c < kc; ++c) acc += tile[c * kDR + t];
        }
        __syncthreads();
    }
    if (t < kDR && r0 + t < m) y[r0 + t] = acc;
}

// The same product in tolerance mode (kernel option mg_coarse_tree): a workgroup owns kDR rows and every thread sums the
// products of its 16 columns of one row in registers as it loads them (no LDS round trip per product); the row's 64
// partial sums are then added pairwise in LDS.  One memory round trip and a 6-deep tree instead of the ordered row sum's
// m dependent additions (~1e-16 relative from the exact mode's k_dense_cm, which keeps the CSR row's bits).
__global__ void __launch_bounds__(kDT) k_dense_tree(int32_t m, const double* __restrict__ Mt,
                                                   const double* __restrict__ b, double* __restrict__ y) {
    constexpr int CPT = kDK * kDR / kDT;   // 16 columns per thread and slab
    constexpr int NP = kDT / kDR;          // 64 partial sums per row
    __shared__ double part[kDR * NP];
    const int32_t r0 = blockIdx.x * kDR;
    const int t = threadIdx.x, row = r0 + t % kDR, k = t / kDR;   // thread t: row t % 16, columns k + 64 u
    double acc = 0.0;
    for (int32_t j0 = 0; j0 < m; j0 += kDK) {
        double v[CPT], bv[CPT];
#pragma unroll
        for (int u = 0; u < CPT; ++u) {
            const int32_t c = j0 + k + NP * u;
            const bool in = c < m && row < m;
            v[u] = in ? Mt[(size_t)c * m + row] : 0.0;   // (lanes of a wave: 16 rows x 4 columns, 128-byte runs)
            bv[u] = c < m ? b[c] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < CPT; ++u) acc += v[u] * bv[u];
    }
    part[(t % kDR) * NP + k] = acc;
    __syncthreads();
#pragma unroll
    for (int w = NP / 2; w >= 1; w >>= 1) {   // rows' partials pairwise: t < 16 w lanes, row t % 16
        if (t < kDR * w) part[(t % kDR) * NP + t / kDR] += part[(t % kDR) * NP + t / kDR + w];
        __syncthreads();
    }
    if (t < kDR && r0 + t < m) y[r0 + t] = part[t * NP];
}

// K Chebyshev-Jacobi sweeps on [lmin, lmax].  zero: from x = 0 (the first sweep is the init pass: d = x =
// c2[0] b / diag), else from the iterate in *cur (d starts at 0).  The last sweep writes `dst` (or the free
// ping-pong buffer when dst is NULL), as sub - x when sub is set; *cur points at the result on return.  xch(x)
// refreshes x's ghost rows before every sweep that reads them (a no-op on one GPU).
// The last two sweeps of a tolerance-mode F Chebyshev solve may run as one fused launch (k_march2 / k_ftile).
bool f_pair_ok(const mpbp_schur_plan* p) { return p->f_numerics == MPBP_NUMERICS_FAST && KO().f_pair && p->f_stencil; }

template <class Xch>
int mg_smooth(const OpPair& op, int32_t nrows, const double* diag, double lmin, double lmax, int K, bool zero,
              const double* b, double** cur, double* alt, double* d, double* dst, const double* sub, hipStream_t st,
              Xch&& xch, int s0 = 0, double* spare = nullptr) {
    double c1[64] = {}, c2[64] = {};
    if (K < 1 || K > 64) return set_error(MPBP_ERR_ARG, "mg: smoothing sweeps must be in [1, 64]");
    cheb_coeffs(lmin, lmax, K, c1, c2);
    const OpRef& o = op.in;
    double* x = *cur;
    double* other = alt;
    // spare (a restart only): the iterate given in *cur is kept -- where the ping-pong would write back into it, the
    // sweep writes `spare` instead
    double* const keep = spare ? *cur : nullptr;
    auto recycle = [&](double* v) { return v == keep ? spare : v; };
    int s = s0;   // s0 > 0: sweeps 0 .. s0 - 1 already ran from *cur's predecessor (d holds their direction)
    if (s0 && (zero || s0 >= K)) return set_error(MPBP_ERR_ARG, "mg: a smoothing resumed at sweep %d of %d", s0, K);
    if (zero && K >= 2 && op.bd.empty && o.stencil && !o.stencil->halo && o.which == 0 &&
        (o.sop == SOP_F || o.sop == SOP_GTG)) {
        // whole-grid stencil level (level 0 of the Schur apply's hierarchies): the first sweep stages
        // x0 = d0 = c2[0] b / diag itself (op_first_sweep, as the Chebyshev inner solve): no init launch, same bits
        double* out1 = K == 2 ? (dst ? dst : other) : other;
        const int rc = op_first_sweep(o, true, b, diag, c2[0], c1[1], c2[1], d, K == 2 ? sub : nullptr, out1, st,
                                      K == 2 ? 0 : 1);
        if (rc) return rc;
        other = x;
        x = out1;
        s = 2;
    } else if (zero && K >= 2 && op.bd.empty && o.grp && o.csr->ncols == nrows) {
        // grouped small level: the first sweep gathers x0 = c2[0] b / diag itself (no init launch, same bits; on the
        // large stencil-values levels the division per gathered entry costs more than the init launch: 110 vs 97 us).
        // Not on a row-partitioned level: its columns reach ghost rows, whose x0 only the exchange after an init
        // pass provides (b and diag hold the owned rows alone)
        double* out1 = K == 2 ? (dst ? dst : other) : other;
        const int rc = grp_cheb_first(o.csr, b, diag, c2[0], c1[1], c2[1], d, K == 2 ? sub : nullptr, out1, st,
                                      K == 2 ? 0 : 1);
        if (rc) return rc;
        other = x;
        x = out1;
        s = 2;
    } else if (zero && K >= 2 && op.bd.empty && o.gal && KO().mg_fuse_l0 && gal_fused_ok(*o.gal) &&
               o.gal->m->part_levels <= 1) {
        // matrix-free level 1 (k_gal1 / k_gal1p): the first sweep stages x0 = c2[0] b / diag itself (XInit) and its
        // epilogue takes the row's own x0 as iterate and direction -- no init launch, k_cheb_init's bits.  Not on a
        // row-partitioned level 1 (b and diag hold the owned rows; the ghosts' x0 comes from the init and exchange)
        double* out1 = K == 2 ? (dst ? dst : other) : other;
        EpiChebFirstGrp e;
        static_cast<EpiChebFirst&>(e) = EpiChebFirst{b, d, c1[1], c2[1], K == 2 ? sub : nullptr, out1, K == 2 ? 0 : 1};
        e.diag = diag;
        e.c2_0 = c2[0];
        bool done = false;
        const int rc = gal_fused(*o.gal, XInit{b, diag, c2[0]}, e, st, &done);
        if (rc) return rc;
        if (!done) return set_error(MPBP_ERR_ARG, "mg: the fused level-1 first sweep did not launch");
        other = x;
        x = out1;
        s = 2;
    } else if (zero) {
        double* out0 = K == 1 ? (dst ? dst : other) : x;
        int rc = op_init(o, nrows, true, b, diag, c2[0], d, K == 1 ? sub : nullptr, out0, st);
        if (rc) return rc;
        if (K == 1) {
            *cur = out0;
            return MPBP_OK;
        }
        s = 1;
    }
    // tolerance-mode F level 0 on one GPU: the last two sweeps as one tiled launch (k_ftile); a restart of two sweeps
    // reads d as +0.0 there, so it needs no memset either
    const bool tpair = K - s >= 2 && o.stencil && o.sop == SOP_F && op.bd.empty && !o.stencil->halo && o.which == 0 &&
                       f_pair_ok(o.stencil) && KO().f_tile && ftile_ok(o.stencil->f_prm.n);
    // restart from the iterate in *cur: d = 0 -- read as +0.0 by the grouped kernel's first sweep, else zeroed
    bool dzero = !zero && !s0 && (((op.in.grp || op.in.svl || op.in.gal || (o.stencil && o.sop == SOP_GTG)) && op.bd.empty) ||
                           (tpair && s == K - 2));
    if (!zero && !dzero && !s0) MPBP_HIP(hipMemsetAsync(d, 0, sizeof(double) * (size_t)nrows, st));
    for (; s < K; ++s) {
        if (tpair && s == K - 2) {
            double* out = dst ? dst : other;
            FStencilDev P;
            const mpbp_schur_plan* p = o.stencil;
            int rc = make_fstencil(&p->f_prm, p->f_cell, p->f_uface, p->f_vface, nullptr, &P);
            if (rc) return rc;
            FTile a{x, d, b, sub, out, nullptr, c1[s], c2[s], c1[s + 1], c2[s + 1]};
            a.dzero = dzero ? 1 : 0;
            rc = launch_ftile<false>(P, a, st);
            if (rc) return rc;
            other = recycle(x);
            x = out;
            break;
        }
        const bool last = s == K - 1;
        double* nxt = (last && dst) ? dst : other;
        xch(x);
        const int rc = pair_cheb(op, x, b, diag, c1[s], c2[s], d, last ? sub : nullptr, nxt, st, last ? 0 : 1, dzero);
        dzero = false;
        if (rc) return rc;
        other = recycle(x);
        x = nxt;
    }
    *cur = x;
    return MPBP_OK;
}

// Level 1 as R_0 (F (P_0 x)): tolerance-mode F (or Gt_G) stencil level 0, level 1 smoothed.  mg_galerkin_mf 1: the three
// launches (one GPU, matrix-free level-0 transfers); 2 (default): the one-launch form where the grid allows it
// (gal_fused_ok: even n >= 72), else the stored Galerkin level -- on one GPU and under a row partition alike (level 0's
// interior / boundary rows and its halo; level 1 replicated whole or its owned rows), so both run the same level 1.
bool mg_gal_ok(const mpbp_mg* m, const MgFine& f) {
    const OpRef& o = f.op.in;
    if (m->smoother != MPBP_MG_SMOOTH_POINT) return false;   // a coupled level 1 is the stored Galerkin level
    if (!KO().mg_galerkin_mf || !o.stencil || !(o.sop == SOP_F || (o.sop == SOP_GTG && KO().mg_galerkin_mf_p)) ||
        o.stencil->f_numerics != MPBP_NUMERICS_FAST || m->nlevels <= 2 || !f.r || !f.d)
        return false;
    const MgGal g{m, o, f.r, f.d};
    if (m->part_levels == 0)
        return o.which == 0 && f.op.bd.empty && !f.halo && !o.stencil->halo && use_mf_transfer(m, 0) &&
               mg_level_even(m, 0) && (KO().mg_galerkin_mf == 1 || gal_fused_ok(g));
    return f.halo && o.stencil->halo && m->tr_nfields > 0 && m->tr_n0 == o.stencil->f_prm.n && gal_fused_ok(g);
}

// Level 0's descent as ONE k_fpre launch (pre-smoothing V(2, .) from x = 0, residual, restriction): tolerance-mode
// matrix-free F on one GPU, the whole grid, the F hierarchy's MAC transfers matrix-free, a grid the tile's staging
// wraps onto at most once (kernel option mg_fuse_l0).
bool fpre_ok(const mpbp_mg* m, const MgFine& f) {
    const OpRef& o = f.op.in;
    if (m->smoother != MPBP_MG_SMOOTH_POINT) return false;   // the fused descent smooths with point Jacobi
    if (!KO().mg_fuse_l0 || !o.stencil || o.sop != SOP_F || o.which != 0 || !f.op.bd.empty || f.halo || o.stencil->halo)
        return false;
    const mpbp_schur_plan* p = o.stencil;
    if (p->f_numerics != MPBP_NUMERICS_FAST || !p->f_stencil || m->part_levels > 0 || !use_mf_transfer(m, 0) ||
        m->tr_nfields != 4)
        return false;
    for (int fl = 0; fl < 4; ++fl)
        if (m->tr_ky[fl] != ((fl & 1) ? MPBP_MG_NODE : MPBP_MG_CELL) || m->tr_kx[fl] != ((fl & 1) ? MPBP_MG_CELL : MPBP_MG_NODE))
            return false;
    const int n = p->f_prm.n;
    return (n & 1) == 0 && m->tr_n0 == n && fsolve_ok_n<3>(n);
}
int launch_fpre(const mpbp_schur_plan* p, const double* b, double lmin, double lmax, double* x_out, double* bc,
                hipStream_t st) {
    FStencilDev Pd;
    const int rc = make_fstencil(&p->f_prm, p->f_cell, p->f_uface, p->f_vface, nullptr, &Pd);
    if (rc) return rc;
    const FStencilFast P{Pd};
    if (P.h != 0 || P.which != 0 || !fsolve_ok_n<3>(P.n) || (P.n & 1) || !b || !x_out || !bc)
        return set_error(MPBP_ERR_ARG, "fpre: one GPU, whole even grid n >= 72");
    double c1[2] = {}, c2[2] = {};
    cheb_coeffs(lmin, lmax, 2, c1, c2);
    const int64_t tiles = (int64_t)((P.n + kFTW - 1) / kFTW) * ((P.n + kFTH - 1) / kFTH);
    k_fpre<<<(unsigned)tiles, 256, 0, st>>>(P, FPre{b, x_out, bc, c2[0], c1[1], c2[1]});
    MPBP_HIP(hipGetLastError());
    return MPBP_OK;
}

// The pressure hierarchy's level 0 the same way (k_gtg_level0): matrix-free Gt_G on one GPU, the whole grid, its
// cell-centred transfers matrix-free, a grid the staging wraps onto at most once (kernel option mg_fuse_l0).
bool gpre_ok(const mpbp_mg* m, const MgFine& f) {
    const OpRef& o = f.op.in;
    if (m->smoother != MPBP_MG_SMOOTH_POINT) return false;
    if (!KO().mg_fuse_l0 || !o.stencil || o.sop != SOP_GTG || o.which != 0 || !f.op.bd.empty || f.halo || o.stencil->halo)
        return false;
    const mpbp_schur_plan* p = o.stencil;
    if (!p->pg_stencil || m->part_levels > 0 || !use_mf_transfer(m, 0) || m->tr_nfields != 1 ||
        m->tr_ky[0] != MPBP_MG_CELL || m->tr_kx[0] != MPBP_MG_CELL)
        return false;
    const int n = p->f_prm.n;
    return (n & 1) == 0 && m->tr_n0 == n && n >= kGTW + kGTH + 6;
}
// pre: x0, sweep 1 (x_out), r = b - A x1, b_c = R_0 r; post: x = x_in + P_0 x_c, two sweeps from d = 0 (x_out, or
// sub - x when sub is set)
int launch_gtg_level0(bool pre, const mpbp_schur_plan* p, const double* b, const double* diag, const double* xin,
                      const double* xc, const double* sub, double lmin, double lmax, double* x_out, double* bc,
                      hipStream_t st) {
    PGDev Pg;
    const int rc = make_pgstencil(&p->f_prm, p->f_cell, nullptr, &Pg);
    if (rc) return rc;
    const GtGStencilDev S{Pg};
    if (S.n < kGTW + kGTH + 6 || (S.n & 1) || !b || !x_out || (pre && (!diag || !bc)) || (!pre && (!xin || !xc)))
        return set_error(MPBP_ERR_ARG, "gtg_level0: one GPU, whole even grid n >= 78, vectors");
    double c1[2] = {}, c2[2] = {};
    cheb_coeffs(lmin, lmax, 2, c1, c2);
    ChebK ck{};
    if (pre) {
        ck.c2[0] = c2[0];
        ck.c1[1] = c1[1];
        ck.c2[1] = c2[1];
    } else {   // the post-smoothing's sweeps s = 0, 1 as levels 1, 2
        ck.c1[1] = c1[0];
        ck.c2[1] = c2[0];
        ck.c1[2] = c1[1];
        ck.c2[2] = c2[1];
    }
    const int64_t tiles = (int64_t)((S.n + kGTW - 1) / kGTW) * ((S.n + kGTH - 1) / kGTH);
    if (pre) k_gtg_level0<true, false><<<(unsigned)tiles, 512, 0, st>>>(S, b, diag, nullptr, nullptr, nullptr, ck, x_out, bc);
    else if (sub) k_gtg_level0<false, true><<<(unsigned)tiles, 512, 0, st>>>(S, b, nullptr, xin, xc, sub, ck, x_out, nullptr);
    else k_gtg_level0<false, false><<<(unsigned)tiles, 512, 0, st>>>(S, b, nullptr, xin, xc, nullptr, ck, x_out, nullptr);
    MPBP_HIP(hipGetLastError());
    return MPBP_OK;
}

// One V-cycle on level l for A_l x = b.  Level 0 uses `fine` (operator and buffers); coarser levels their
// mpbp_mg_level.  *res receives the result's buffer (dst when given).  Row partition (m->part_levels > 0): levels
// l < part_levels hold owned rows (vectors read by an operator carry ghost rows, refreshed by mg_exchange); the
// restriction into level part_levels writes the rank's rows of that level into its r buffer, which is all-gathered
// into its (whole-grid) b, and every coarser level runs replicated on each rank -- the same operators and
// operands as on one GPU, so the same bits.
int mg_vcycle(const mpbp_mg* m, int l, const MgFine& fine, const double* b, bool zero, double* xin, double* dst,
              const double* sub, double** res, hipStream_t st) {
    const mpbp_mg_level& L = m->levels[l];
    const bool top = l == 0;
    // the phase-coupled smoother (mg_coupled.inc): residual + k_cpl_update per sweep, none of the fused launches below
    // (mg_gal_ok, fpre_ok and gpre_ok refuse it; k_grp_rr, residual + restriction only, and the transfers stay)
    const bool cpl = m->smoother == MPBP_MG_SMOOTH_COUPLED;
    OpPair o = top ? fine.op : mg_level_op(L);
    MgGal gal{m, fine.op.in, fine.r, fine.d};   // (fine.r, fine.d: dead while level 1 runs)
    if (l == 1 && mg_gal_ok(m, fine)) {
        o.in = OpRef{nullptr, nullptr, nullptr, nullptr, false, 0, SOP_NONE};
        o.in.gal = &gal;
        o.bd = OpRef{nullptr, nullptr, nullptr, nullptr, true, 0, SOP_NONE};
    }
    const double* diag = top ? fine.diag : L.diag;
    double* bx = top ? fine.x : L.x;
    double* bt = top ? fine.t : L.t;
    double* alt = xin == bx ? bt : bx;
    double* r = top ? fine.r : L.r;
    double* d = top ? fine.d : L.d;
    double* cur = xin;
    auto xch = [&](double* v) { mg_exchange(m, l, fine, v, st); };
    const mpbp_mg_level& C = m->levels[l + 1];
    const bool gather = m->part_levels > 0 && l + 1 == m->part_levels;
    const bool small = mg_small_ok(m, l, o);   // (never a gathering level: l >= part_levels)
    int rc = MPBP_OK;
    if (top && zero && L.pre == 2 && fpre_ok(m, fine)) {
        // x0, sweep 1, r = b - A x and b_c = R r in one launch; x1 where the smoothing would leave it (the free buffer)
        cur = alt;
        rc = launch_fpre(o.in.stencil, b, L.lmin, L.lmax, cur, C.b, st);
        if (rc) return rc;
        alt = cur == bx ? bt : bx;
    } else if (top && zero && L.pre == 2 && gpre_ok(m, fine)) {   // the same for the pressure hierarchy
        cur = alt;
        rc = launch_gtg_level0(true, o.in.stencil, b, diag, nullptr, nullptr, nullptr, L.lmin, L.lmax, cur, C.b, st);
        if (rc) return rc;
        alt = cur == bx ? bt : bx;
    } else {
        // an initial guess outside the level's two iterate buffers (the accelerated solve's x_k) is only read: the
        // pre-smoothing then ping-pongs between bx and bt, and everything after it works on those two
        double* spare = (!zero && xin != bx && xin != bt) ? bt : nullptr;
        rc = cpl ? mg_smooth_cpl(o, L.nrows, L.cpl_p, L.cpl_q, L.lmin, L.lmax, L.pre, zero, b, &cur, alt, r, d, nullptr,
                                 nullptr, st, xch, spare, top && m->cpl_fuse)
                 : mg_smooth(o, L.nrows, diag, L.lmin, L.lmax, L.pre, zero, b, &cur, alt, d, nullptr, nullptr, st, xch, 0,
                             spare);
        if (rc) return rc;
        alt = cur == bx ? bt : bx;
        if (small) {   // r = b - A x and b_c = R r in one launch (k_grp_rr)
            rc = launch_grp_rr(m, l, o.in.csr, cur, b, C.b, st);
        } else {       // r = b - A x ; b_c = R r
            xch(cur);
            rc = pair_spmv(o, MPBP_SPMV_RESID, cur, b, r, st);
            if (rc) return rc;
            if (l < m->part_levels) xch(r);
            rc = use_mf_transfer(m, l) ? mg_transfer_mf(m, l, MPBP_MG_R, L.R.nrows, r, EpiStore{gather ? C.r : C.b}, st)
                                       : mg_transfer(L.R, L.R_blocks, L.R_sell, MPBP_SPMV_STORE, r, nullptr,
                                                     gather ? C.r : C.b, st);
        }
        if (rc) return rc;
    }
    if (gather) {
        if (!m->gather) return set_error(MPBP_ERR_ARG, "mg: a partitioned hierarchy needs its gather callback");
        m->gather(m->halo_ctx, m->gather_kind, C.r, C.b, (void*)st);
    }
    double* xc = C.x;
    if (l + 1 == m->nlevels - 1) {
        if (m->coarse_dense) {
            // tolerance-mode hierarchies (the fine operator a fast-numerics stencil plan): the tree-summed product
            const bool tree = KO().mg_coarse_tree && fine.op.in.stencil &&
                              fine.op.in.stencil->f_numerics == MPBP_NUMERICS_FAST;
            if (tree) k_dense_tree<<<grid_for(C.nrows, kDR), kDT, 0, st>>>(C.nrows, m->coarse_dense, C.b, xc);
            else k_dense_cm<<<grid_for(C.nrows, kDR), kDT, 0, st>>>(C.nrows, m->coarse_dense, C.b, xc);
            MPBP_HIP(hipGetLastError());
        } else {
            rc = mpbp_spmv(&m->coarse_inv, &m->coarse_inv_blocks, MPBP_SPMV_STORE, C.b, nullptr, xc, (void*)st);
        }
    } else {
        rc = mg_vcycle(m, l + 1, fine, C.b, true, C.x, nullptr, nullptr, &xc, st);
    }
    if (rc) return rc;
    // x += P x_c (row-wise in place), then post-smoothing from x
    mg_exchange(m, l + 1, fine, xc, st);
    if (top && L.post == 2 && gpre_ok(m, fine)) {   // x + P_0 x_c and the two post-smoothing sweeps in one launch
        double* out = dst ? dst : alt;
        rc = launch_gtg_level0(false, o.in.stencil, b, nullptr, cur, xc, sub, L.lmin, L.lmax, out, nullptr, st);
        if (rc) return rc;
        *res = out;
        return MPBP_OK;
    }
    if (top && L.post == 2 && fpre_ok(m, fine) && f_pair_ok(o.in.stencil) && KO().f_tile && ftile_ok(o.in.stencil->f_prm.n)) {
        // the prolongation folded into the post-smoothing pair's staging (k_ftile<PRO>: x + P_0 x_c per staged cell,
        // the prolongation launch's operations), the restart's direction read as +0.0 -- mg_smooth's tile pair
        double c1[2] = {}, c2[2] = {};
        cheb_coeffs(L.lmin, L.lmax, 2, c1, c2);
        double* out = dst ? dst : alt;
        const mpbp_schur_plan* p = o.in.stencil;
        FStencilDev P;
        rc = make_fstencil(&p->f_prm, p->f_cell, p->f_uface, p->f_vface, nullptr, &P);
        if (rc) return rc;
        FTile a{cur, d, b, sub, out, nullptr, c1[0], c2[0], c1[1], c2[1]};
        a.dzero = 1;
        a.xc = xc;
        rc = launch_ftile<false>(P, a, st);
        if (rc) return rc;
        *res = out;
        return MPBP_OK;
    }
    if (o.in.gal && L.post >= 1 && L.post <= 64 && gal_pro_ok(*o.in.gal)) {
        // level 1 (matrix-free F): x + P_1 x_c staged by the first post-smoothing sweep (k_gal1<PRO>), the remaining
        // sweeps as mg_smooth's
        double c1[64] = {}, c2[64] = {};
        cheb_coeffs(L.lmin, L.lmax, L.post, c1, c2);
        const bool last = L.post == 1;
        double* x1 = last && dst ? dst : alt;
        const EpiCheb e{cur, b, diag, d, c1[0], c2[0], last ? sub : nullptr, x1, last ? 0 : 1};
        rc = gal_pro(*o.in.gal, cur, xc, EpiZeroD<EpiCheb>{e}, st);
        if (rc) return rc;
        if (!last) rc = mg_smooth(o, L.nrows, diag, L.lmin, L.lmax, L.post, false, b, &x1, cur, d, dst, sub, st, xch, 1);
        if (rc) return rc;
        *res = x1;
        return MPBP_OK;
    }
    rc = use_mf_transfer(m, l) ? mg_transfer_mf(m, l, MPBP_MG_P, L.P.nrows, xc, EpiAdd{cur, cur}, st)
                               : mg_transfer(L.P, L.P_blocks, L.P_sell, MPBP_SPMV_ADD, xc, cur, cur, st);
    if (rc) return rc;
    rc = cpl ? mg_smooth_cpl(o, L.nrows, L.cpl_p, L.cpl_q, L.lmin, L.lmax, L.post, false, b, &cur, alt, r, d, dst, sub,
                             st, xch, nullptr, top && m->cpl_fuse)
             : mg_smooth(o, L.nrows, diag, L.lmin, L.lmax, L.post, false, b, &cur, alt, d, dst, sub, st, xch);
    if (rc) return rc;
    *res = cur;
    return MPBP_OK;
}

}  // namespace
