// The Schur apply's operators: Ctx, OpRef / OpPair, MgGal, op_spmv / op_init / op_first_sweep / op_cheb /
// op_jacobi and two_phase.  Opens the namespace that schur_inner.inc closes.  Needs mpbp.hip's kernels, the kernel
// fragments and launchers.inc, the C entries of abi_core.inc (mpbp_spmv, mpbp_cheb_init, ...) and abi_stencil.inc.
// A fragment of mpbp.hip, included there once and in order: not a self-contained header.

// ======================================================= Schur apply ====
namespace {

struct Ctx {
    const mpbp_schur_plan* p;
    hipStream_t st;
};

// Profiling events are recorded only on eager (uncaptured) launches: a capturing stream skips them.
hipError_t record_event(hipEvent_t ev, hipStream_t st) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    hipError_t e = hipStreamIsCapturing(st, &cs);
    if (e != hipSuccess) return e;
    return cs == hipStreamCaptureStatusNone ? hipEventRecord(ev, st) : hipSuccess;
}

// One operator of the apply, restricted to interior or boundary rows, in CSR or SELL form.
enum StencilOp { SOP_NONE = 0, SOP_F, SOP_D, SOP_G, SOP_GTG };

struct OpRef {
    const mpbp_csr* csr;
    const mpbp_rowblocks* blk;
    const mpbp_sell* sell;
    const mpbp_schur_plan* stencil;   // rows recomputed from the plan's thn tables (sop says which operator)
    bool empty;
    int32_t which;                    // stencil rows: 0 all, 1 interior, 2 boundary, 3 owned + ext ghost rows
    int32_t sop;
    int32_t ext = 0;                  // which = 3
    int32_t grp = 0;                  // CSR rows through k_csr_grp (multigrid small levels)
    const mpbp_svl* svl = nullptr;    // stencil-values layout of csr (multigrid large levels)
    const struct MgGal* gal = nullptr;   // level 1 of an F hierarchy applied as R0 (F (P0 x)) (tolerance mode)
};

// Level 1 of the F hierarchy without its Galerkin matrix (tolerance mode): A_1 x = R_0 (F (P_0 x)) -- the same operator
// as the stored product (mg_oracle's R A P) in exact arithmetic -- from the matrix-free transfers and the tolerance-mode
// F sweep of level 0, through two fine-size temporaries (level 0's residual and direction buffers, dead while level 1
// runs).  Per application: x_c and the thn read, two fine vectors written and read once, the level-1 epilogue operands;
// ~115 MB at 1024^2 instead of streaming the 40-entry coarse rows' values (386 MB).
struct MgGal {
    const mpbp_mg* m;
    OpRef fine;     // level 0's whole-grid F stencil
    double* t0;     // fine-size temporaries
    double* t1;
};

// F and D read velocity vectors (f_part), G and Gt_G pressure vectors (p_part); D writes a pressure vector
// and G a velocity one (output ghost depth oh).
inline mpbp_row_part stencil_part(const OpRef& o) {
    const mpbp_schur_plan* p = o.stencil;
    mpbp_row_part q = (o.sop == SOP_F || o.sop == SOP_D) ? p->f_part : p->p_part;
    q.which = q.halo > 0 ? o.which : 0;
    q.ext = q.which == 3 ? o.ext : 0;
    q.oh = o.sop == SOP_D ? p->p_part.halo : o.sop == SOP_G ? p->f_part.halo : 0;
    return q;
}

template <class Epi>
int mg_transfer_mf(const mpbp_mg* m, int l, int32_t which, int32_t nrows, const double* x, Epi epi, hipStream_t st);
int op_spmv(const OpRef& o, int32_t mode, const double* x, const double* z, double* y, hipStream_t st);
// t1 = F (P_0 x): the first two stages of a matrix-free Galerkin level-1 product
int gal_fp(const MgGal& g, const double* x, hipStream_t st) {
    const int rc = mg_transfer_mf(g.m, 0, MPBP_MG_P, g.m->levels[0].P.nrows, x, EpiStore{g.t0}, st);
    return rc ? rc : op_spmv(g.fine, MPBP_SPMV_STORE, g.t0, nullptr, g.t1, st);
}
template <class Epi>
int gal_r(const MgGal& g, Epi epi, hipStream_t st) {
    return mg_transfer_mf(g.m, 0, MPBP_MG_R, g.m->levels[0].R.nrows, g.t1, epi, st);
}

// The whole level-1 product as one k_gal1 launch (KO().mg_galerkin_mf == 2): four fields, a grid the staged windows wrap once.
// gal_fused_ok: whether gal_fused takes the one-launch form for this level (else the caller runs the three launches)
// Under a row partition (g.m->part_levels > 0) level 1 is either the whole replicated level (part_levels == 1: the
// one-GPU launch on every rank) or row-partitioned (> 1: the PART launch over the owned coarse rows, its x read with
// >= 2 ghost rows each side -- the windows' reach).
bool gal_part(const MgGal& g, G1Part* q) {
    *q = G1Part{};
    if (g.m->part_levels <= 1) return true;
    const mpbp_mg_level& L1 = g.m->levels[1];
    const int nc = g.fine.stencil->f_prm.n / 2, nf = g.fine.sop == SOP_GTG ? 1 : 4;
    if (L1.nrows == nf * nc * nc && L1.part_r0 == 0) return true;   // one rank: its owned rows are the whole level
    if (nc <= 0 || L1.nrows % (nf * nc) || L1.part_h < 2 || L1.part_r0 < 0) return false;
    q->r0 = L1.part_r0;
    q->L = L1.nrows / (nf * nc);
    q->h = L1.part_h;
    return q->L >= q->h && q->r0 + q->L <= nc;
}
bool gal_fused_ok(const MgGal& g) {
    const mpbp_schur_plan* p = g.fine.stencil;
    if (KO().mg_galerkin_mf != 2 || p->f_prm.n < 2 * kG1CW || (p->f_prm.n & 1)) return false;
    G1Part q;
    if (!gal_part(g, &q)) return false;
    if (g.fine.sop == SOP_GTG) return g.m->tr_nfields == 1 && g.m->tr_ky[0] == MPBP_MG_CELL && g.m->tr_kx[0] == MPBP_MG_CELL;
    return g.m->tr_nfields == 4;
}
template <class Epi, class XS = XPlain>
int gal_fused(const MgGal& g, XS x, Epi epi, hipStream_t st, bool* done) {
    *done = false;
    const mpbp_schur_plan* p = g.fine.stencil;
    if (!gal_fused_ok(g)) return MPBP_OK;
    G1Part q;
    gal_part(g, &q);
    const bool part = q.L > 0;
    if (g.fine.sop == SOP_GTG) {   // the pressure hierarchy: one field, cell-centred (mg.FIELDS_PRESSURE)
        PGDev Pg;
        const int rc = make_pgstencil(&p->f_prm, p->f_cell, nullptr, &Pg);
        if (rc) return rc;
        const int nc = p->f_prm.n / 2;
        const int64_t tiles = (int64_t)((nc + kG1W - 1) / kG1W) * (((part ? q.L : nc) + kG1PH2 - 1) / kG1PH2);
        if (part) k_gal1p<Epi, XS, true><<<(unsigned)tiles, 256, 0, st>>>(GtGStencilDev{Pg}, x, epi, q);
        else k_gal1p<Epi, XS><<<(unsigned)tiles, 256, 0, st>>>(GtGStencilDev{Pg}, x, epi, q);
        MPBP_HIP(hipGetLastError());
        *done = true;
        return MPBP_OK;
    }
    FStencilDev Pd;
    const int rc = make_fstencil(&p->f_prm, p->f_cell, p->f_uface, p->f_vface, nullptr, &Pd);
    if (rc) return rc;
    MgFields F{};
    F.nfields = 4;
    for (int f = 0; f < 4; ++f) {
        F.ky[f] = g.m->tr_ky[f];
        F.kx[f] = g.m->tr_kx[f];
    }
    const int nc = p->f_prm.n / 2;
    const int64_t tiles = (int64_t)((nc + kGFW - 1) / kGFW) * (((part ? q.L : nc) + kGFH - 1) / kGFH);
    bool mac = true;   // the F hierarchy's MAC kinds (mg.FIELDS_VELOCITY)
    for (int f = 0; f < 4; ++f)
        mac = mac && F.ky[f] == ((f & 1) ? MPBP_MG_NODE : MPBP_MG_CELL) && F.kx[f] == ((f & 1) ? MPBP_MG_CELL : MPBP_MG_NODE);
    if (part && !mac) return set_error(MPBP_ERR_ARG, "mg: a row-partitioned matrix-free level 1 needs the MAC kinds");
    if (part) k_gal1<Epi, true, XS, true><<<(unsigned)tiles, 256, 0, st>>>(FStencilFast{Pd}, F, x, epi, q);
    else if (mac) k_gal1<Epi, true, XS><<<(unsigned)tiles, 256, 0, st>>>(FStencilFast{Pd}, F, x, epi, q);
    else k_gal1<Epi, false, XS><<<(unsigned)tiles, 256, 0, st>>>(FStencilFast{Pd}, F, x, epi, q);
    MPBP_HIP(hipGetLastError());
    *done = true;
    return MPBP_OK;
}

MgFields mg_fields(const mpbp_mg* m);
// The post-smoothing's first sweep on a matrix-free level 1 with level 2's correction folded in (k_gal1<PRO>,
// k_gal1p<PRO>): x = x_in + P_1 x_c staged, then the sweep from d = 0 -- the prolongation launch and that sweep's
// operations.  One GPU (or a replicated level 1), the F hierarchy's MAC kinds, the one-launch form.
bool gal_pro_ok(const MgGal& g) {
    G1Part q;
    if (!gal_fused_ok(g) || !gal_part(g, &q) || q.L || g.m->nlevels < 3 || !KO().mg_fuse_l0) return false;
    const int nf = g.fine.sop == SOP_GTG ? 1 : 4;   // (gal_fused_ok: the pressure hierarchy's one cell-centred field)
    if (nf == 4)
        for (int f = 0; f < 4; ++f)
            if (g.m->tr_ky[f] != ((f & 1) ? MPBP_MG_NODE : MPBP_MG_CELL) ||
                g.m->tr_kx[f] != ((f & 1) ? MPBP_MG_CELL : MPBP_MG_NODE))
                return false;
    const int n = g.fine.stencil->f_prm.n, n2 = n / 4;
    return n % 4 == 0 && n2 >= kG1QW && g.m->levels[2].nrows == nf * n2 * n2;
}
int gal_pro(const MgGal& g, const double* x, const double* xc, const EpiZeroD<EpiCheb>& epi, hipStream_t st) {
    const mpbp_schur_plan* p = g.fine.stencil;
    const int nc = p->f_prm.n / 2;
    if (g.fine.sop == SOP_GTG) {
        PGDev Pg;
        const int rc = make_pgstencil(&p->f_prm, p->f_cell, nullptr, &Pg);
        if (rc) return rc;
        const int64_t tiles = (int64_t)((nc + kG1W - 1) / kG1W) * ((nc + kG1PH2 - 1) / kG1PH2);
        k_gal1p<EpiZeroD<EpiCheb>, XPlain, false, true><<<(unsigned)tiles, 256, 0, st>>>(GtGStencilDev{Pg}, XPlain{x},
                                                                                         epi, G1Part{}, xc);
        MPBP_HIP(hipGetLastError());
        return MPBP_OK;
    }
    FStencilDev Pd;
    const int rc = make_fstencil(&p->f_prm, p->f_cell, p->f_uface, p->f_vface, nullptr, &Pd);
    if (rc) return rc;
    const int64_t tiles = (int64_t)((nc + kGFW - 1) / kGFW) * ((nc + kGFH - 1) / kGFH);
    k_gal1<EpiZeroD<EpiCheb>, true, XPlain, false, true><<<(unsigned)tiles, 256, 0, st>>>(
        FStencilFast{Pd}, mg_fields(g.m), XPlain{x}, epi, G1Part{}, xc);
    MPBP_HIP(hipGetLastError());
    return MPBP_OK;
}

int op_spmv(const OpRef& o, int32_t mode, const double* x, const double* z, double* y, hipStream_t st) {
    if (o.empty) return MPBP_OK;
    if (o.gal) {
        bool done = false;
        int rf = MPBP_OK;
        switch (mode) {
        case MPBP_SPMV_STORE: rf = gal_fused(*o.gal, XPlain{x}, EpiStore{y}, st, &done); break;
        case MPBP_SPMV_ADD: rf = gal_fused(*o.gal, XPlain{x}, EpiAdd{z, y}, st, &done); break;
        case MPBP_SPMV_RESID: rf = gal_fused(*o.gal, XPlain{x}, EpiResid{z, y}, st, &done); break;
        default: break;
        }
        if (rf || done) return rf;
        const int rc = gal_fp(*o.gal, x, st);
        if (rc) return rc;
        switch (mode) {
        case MPBP_SPMV_STORE: return gal_r(*o.gal, EpiStore{y}, st);
        case MPBP_SPMV_ADD: return gal_r(*o.gal, EpiAdd{z, y}, st);
        case MPBP_SPMV_RESID: return gal_r(*o.gal, EpiResid{z, y}, st);
        default: return set_error(MPBP_ERR_ARG, "galerkin spmv: unknown mode %d", mode);
        }
    }
    if (o.stencil) {
        const mpbp_schur_plan* p = o.stencil;
        const mpbp_row_part q = stencil_part(o);
        if (o.sop == SOP_F)
            return mpbp_f_stencil_spmv(&p->f_prm, p->f_cell, p->f_uface, p->f_vface, &q,
                                       mode | (p->f_numerics == MPBP_NUMERICS_FAST ? MPBP_SPMV_FAST : 0), x, z, y,
                                       (void*)st);
        const int32_t op = o.sop == SOP_D ? MPBP_PG_D : o.sop == SOP_G ? MPBP_PG_G : MPBP_PG_GTG;
        return mpbp_pg_stencil_spmv(&p->f_prm, p->f_cell, &q, op, mode, x, z, y, (void*)st);
    }
    if (o.grp) return grp_spmv(o.csr, mode, x, z, y, st);
    if (o.svl) return svl_spmv(o.svl, o.csr, mode, x, z, y, st);
    return o.sell ? mpbp_sell_spmv(o.sell, mode, x, z, y, (void*)st)
                  : mpbp_spmv(o.csr, o.blk, mode, x, z, y, (void*)st);
}
int op_jacobi(const OpRef& o, const double* xin, const double* b, const double* dg, const double* sub, double* xo,
              hipStream_t st) {
    if (o.empty) return MPBP_OK;
    if (o.stencil) {
        const mpbp_schur_plan* p = o.stencil;
        const mpbp_row_part q = stencil_part(o);
        if (o.sop == SOP_F)
            return f_stencil_jacobi_impl(&p->f_prm, p->f_cell, p->f_uface, p->f_vface, &q, xin, b, sub, xo, (void*)st,
                                         p->f_numerics == MPBP_NUMERICS_FAST);
        return mpbp_gtg_stencil_jacobi_step(&p->f_prm, p->f_cell, &q, xin, b, sub, xo, (void*)st);
    }
    return o.sell ? mpbp_sell_jacobi_step(o.sell, xin, b, dg, sub, xo, (void*)st)
                  : mpbp_jacobi_step(o.csr, o.blk, xin, b, dg, sub, xo, (void*)st);
}
int op_cheb(const OpRef& o, const double* xin, const double* b, const double* dg, double c1, double c2, double* d,
            const double* sub, double* xo, hipStream_t st, int store_d, bool dzero = false) {
    if (o.empty) return MPBP_OK;
    if (o.gal) {
        // (dzero: a restart's first sweep reads d as +0.0 -- no memset of the direction)
        auto run = [&](const auto& epi) {
            bool done = false;
            const int rf = gal_fused(*o.gal, XPlain{xin}, epi, st, &done);
            if (rf || done) return rf;
            const int rc = gal_fp(*o.gal, xin, st);
            return rc ? rc : gal_r(*o.gal, epi, st);
        };
        const EpiCheb e{xin, b, dg, d, c1, c2, sub, xo, store_d};
        return dzero ? run(EpiZeroD<EpiCheb>{e}) : run(e);
    }
    if (o.grp) return grp_cheb(o.csr, xin, b, dg, c1, c2, d, sub, xo, st, store_d, dzero);
    if (o.svl) return svl_cheb(o.svl, o.csr, xin, b, dg, c1, c2, d, sub, xo, st, store_d, dzero);
    if (dzero && !(o.stencil && o.sop == SOP_GTG))
        return set_error(MPBP_ERR_ARG, "cheb: a zero direction needs the grouped / stencil-values / Gt_G stencil path");
    if (o.stencil) {
        const mpbp_schur_plan* p = o.stencil;
        const mpbp_row_part q = stencil_part(o);
        if (o.sop == SOP_F)
            return f_stencil_cheb_impl(&p->f_prm, p->f_cell, p->f_uface, p->f_vface, &q, xin, b, c1, c2, d, sub,
                                       xo, (void*)st, store_d, p->f_numerics == MPBP_NUMERICS_FAST);
        return gtg_stencil_cheb_impl(&p->f_prm, p->f_cell, &q, xin, b, c1, c2, d, sub, xo, (void*)st, store_d, dzero);
    }
    return o.sell ? sell_cheb_impl(o.sell, xin, b, dg, c1, c2, d, sub, xo, (void*)st, store_d)
                  : cheb_step_impl(o.csr, o.blk, xin, b, dg, c1, c2, d, sub, xo, (void*)st, store_d);
}

struct OpPair {
    OpRef in, bd;
};

// x0 (= d0 for Chebyshev) of an inner solve from x = 0 over `nrows` owned rows: the tolerance-mode F operator on a row
// partition's owned rows takes the fast reciprocal diagonals (k_f_fast_init, the one-GPU fast first sweep's bits);
// every other operator the stored diagonal (k_cheb_init / k_jacobi_init: c2 (b / diag)).
int op_init(const OpRef& o, int32_t nrows, bool cheb, const double* b, const double* diag, double c2, double* d,
            const double* sub, double* xo, hipStream_t st) {
    const mpbp_schur_plan* p = o.stencil;
    if (p && o.sop == SOP_F && p->f_numerics == MPBP_NUMERICS_FAST && o.which != 3) {
        mpbp_row_part q = stencil_part(o);   // (the interior / boundary split of the sweeps: the init covers every owned row)
        q.which = 0;
        q.ext = 0;
        FStencilDev Pd;
        const int rc = make_fstencil(&p->f_prm, p->f_cell, p->f_uface, p->f_vface, &q, &Pd);
        if (rc) return rc;
        const FStencilFast P{Pd};
        if ((int64_t)4 * P.L * P.n != nrows) return set_error(MPBP_ERR_ARG, "f fast init: %d rows, not the owned ones", nrows);
        const int grid = grid_for((int64_t)P.L * P.n);
        if (cheb) k_f_fast_init<true><<<grid, 256, 0, st>>>(P, b, c2, d, sub, xo);
        else k_f_fast_init<false><<<grid, 256, 0, st>>>(P, b, 1.0, nullptr, sub, xo);
        MPBP_HIP(hipGetLastError());
        return MPBP_OK;
    }
    return cheb ? mpbp_cheb_init(nrows, b, diag, c2, d, sub, xo, (void*)st)
                : mpbp_jacobi_init(nrows, b, diag, sub, xo, (void*)st);
}

// The first sweep of an inner solve can fold in the init pass (x0 = d0 = c2[0] b / diag, recomputed
// from b and diag wherever the sweep stages x) when the operator is a whole-grid marching stencil.
bool can_fuse_init(const OpPair& op) {
    const OpRef& o = op.in;
    return o.stencil && !o.stencil->halo && !o.empty && op.bd.empty && o.which == 0 &&
           (o.sop == SOP_GTG || o.sop == SOP_F);
}

int op_first_sweep(const OpRef& o, bool cheb, const double* b, const double* diag, double c2_0, double c1, double c2,
                   double* d, const double* sub, double* xo, hipStream_t st, int store_d) {
    const mpbp_schur_plan* p = o.stencil;
    const XInit xs{b, diag, cheb ? c2_0 : 1.0};
    const mpbp_row_part q = stencil_part(o);   // one GPU: no partition; CA schedule: owned + ext ghost rows
    if (o.sop == SOP_F) {
        FStencilDev P;
        const int rc = make_fstencil(&p->f_prm, p->f_cell, p->f_uface, p->f_vface, &q, &P);
        if (rc) return rc;
        const bool fast = p->f_numerics == MPBP_NUMERICS_FAST;
        if (fast && cheb && KO().f_tile && q.halo == 0 && o.which == 0 && ftile_ok(P.n))   // x0, sweep 1 on 2D tiles
            return launch_ftile<true>(P, FTile{nullptr, nullptr, b, sub, xo, store_d ? d : nullptr, 0.0, c2_0, c1, c2},
                                      st);
        if (KO().init_diag == 0)
            return with_f_policy(P, fast, [&](const auto& Q) {
                return cheb ? launch_march(Q, xs, EpiChebFirst{b, d, c1, c2, sub, xo, store_d}, KO().march_rows, st)
                            : launch_march(Q, xs, EpiJacobi{nullptr, b, nullptr, sub, xo}, KO().march_rows, st);
            });
        return with_f_policy(P, fast, [&](const auto& Q) {
            return cheb ? launch_march_init(Q, b, xs.c2, EpiChebFirst{b, d, c1, c2, sub, xo, store_d}, KO().march_rows, st)
                        : launch_march_init(Q, b, xs.c2, EpiJacobi{nullptr, b, nullptr, sub, xo}, KO().march_rows, st);
        });
    }
    PGDev P;
    const int rc = make_pgstencil(&p->f_prm, p->f_cell, &q, &P);
    if (rc) return rc;
    // Gt_G: the staged diagonal is streamed (8 B per row; rebuilding it from thn measured slower, 21.6 vs 16.1 us
    // at 1024^2: the sweep is latency-bound and the rebuild lengthens its staging)
    const GtGStencilDev S{P};
    return cheb ? launch_march(S, xs, EpiChebFirst{b, d, c1, c2, sub, xo, store_d}, pg_rows(), st)
                : launch_march(S, xs, EpiJacobi{nullptr, b, nullptr, sub, xo}, pg_rows(), st);
}

OpPair make_op(const mpbp_schur_plan* p, const mpbp_csr& A, const mpbp_rowblocks& bi, const mpbp_rowblocks& bb,
               const mpbp_sell& si, const mpbp_sell& sb) {
    if (p->use_sell)
        return OpPair{OpRef{&A, nullptr, &si, nullptr, false, 0, SOP_NONE},
                      OpRef{&A, nullptr, &sb, nullptr, false, 0, SOP_NONE}};
    return OpPair{OpRef{&A, &bi, nullptr, nullptr, false, 0, SOP_NONE}, OpRef{&A, &bb, nullptr, nullptr, false, 0, SOP_NONE}};
}

// Stencil operator: interior + boundary rows under a row partition, else all rows in one launch.
OpPair make_stencil_op(const mpbp_schur_plan* p, int32_t sop, bool partitioned) {
    if (partitioned)
        return OpPair{OpRef{nullptr, nullptr, nullptr, p, false, 1, sop}, OpRef{nullptr, nullptr, nullptr, p, false, 2, sop}};
    return OpPair{OpRef{nullptr, nullptr, nullptr, p, false, 0, sop}, OpRef{nullptr, nullptr, nullptr, nullptr, true, 0, SOP_NONE}};
}

// Launch one sweep over interior rows, then (after the halo is complete) boundary rows.
template <class Fn>
int two_phase(const Ctx& c, int32_t kind, const double* x_ext, const OpPair& op, Fn&& launch) {
    const mpbp_schur_plan* p = c.p;
    if (p->halo && p->halo_first) {   // exchange first, then every row (stencils: one whole-partition launch)
        p->halo(p->halo_ctx, kind, const_cast<double*>(x_ext), MPBP_HALO_BEGIN, (void*)c.st);
        p->halo(p->halo_ctx, kind, const_cast<double*>(x_ext), MPBP_HALO_END, (void*)c.st);
        const int rc = launch(op.in);
        return rc ? rc : launch(op.bd);
    }
    if (p->halo) p->halo(p->halo_ctx, kind, const_cast<double*>(x_ext), MPBP_HALO_BEGIN, (void*)c.st);
    int rc = launch(op.in);
    if (rc) return rc;
    if (p->halo) p->halo(p->halo_ctx, kind, const_cast<double*>(x_ext), MPBP_HALO_END, (void*)c.st);
    return launch(op.bd);
}

// Tolerance mode on a row partition: Gt_F_G x_a from the diamond's upper half over the rank's row block (k_q13p; the
// plan's q13 then holds grid rows p_part.r0 - 2 .. r0 + rows - 1, mpbp_q13_build_rows), x_a's ghost rows complete.
bool q13p_ok(const mpbp_schur_plan* p) {
    return p->q13 && p->halo && KO().q13_sym && p->f_numerics == MPBP_NUMERICS_FAST && p->q13_n >= 5 &&
           p->p_part.halo >= 2 && p->p_part.rows >= 1 && p->np == p->p_part.rows * p->q13_n;
}
template <class Epi>
int launch_q13p(const mpbp_schur_plan* p, const double* x_ext, Epi epi, hipStream_t st) {
    const int32_t n = p->q13_n, L = p->p_part.rows;
    k_q13p<Epi><<<grid_for((int64_t)L * n), kBlock, 0, st>>>(n, p->p_part.r0, L, p->p_part.halo, p->q13, x_ext, epi);
    MPBP_HIP(hipGetLastError());
    return MPBP_OK;
}

}  // namespace
