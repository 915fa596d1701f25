// The pressure side's fused launches (d_rhs_x0, launch_gtg_solve_t, gtg_fused_ok, gtg_solve_fused), closing the
// namespace schur_ops.inc opened; their C entry mpbp_gtg_stencil_cheb_solve; then the Schur apply's inner solves
// (f_pair, inner_solve, f_solve_gx).  Needs schur_ops.inc, k_gtg_solve (gtg_solve.inc) and the F launchers
// (f_tile.inc, f_solve_w.inc).
// A fragment of mpbp.hip, included there once and in order: not a self-contained header.
namespace {

// rhs = D Finv_v + v_p with the first Gt_G sweep's x0 = c2 (rhs / diag_P) written beside it (one GPU, matrix-free D).
int d_rhs_x0(const mpbp_schur_plan* p, const double* Y, const double* v_p, double* rhs, double c2, double* x0,
             hipStream_t st) {
    PGDev P;
    const int rc = make_pgstencil(&p->f_prm, p->f_cell, nullptr, &P);
    if (rc) return rc;
    return launch_march(DStencilDev{P}, XPlain{Y}, EpiAddX0{v_p, rhs, p->diag_P, c2, x0}, pg_rows(), st);
}

// x = Gt_G^-1 b by the plan's Chebyshev inner solve in one k_gtg_solve launch (one GPU, matrix-free Gt_G, 2..6 sweeps).
template <int H, int GW, int GH>
int launch_gtg_solve_g(const GtGStencilDev& S, const double* b, const double* diag, const ChebK& ck, double* out,
                       hipStream_t st, GtgD dv) {
    const bool part = S.h != 0;
    // every staged cell of a tile (tile + H + 1 each side) must wrap onto the grid at most once (the staging's periodic
    // fold subtracts n once): refuse smaller grids here, whatever the caller checked (gtg_fused_ok) -- one bound for
    // both tiles (the 64 x 8 tile's, the larger), so the tile option never changes which grids the fused solve takes
    constexpr int kMin = kGTW + kGTH + 2 * H;
    static_assert(GW + GH + 2 * H <= kMin, "the documented bound covers this tile");
    if (S.n < kMin)
        return set_error(MPBP_ERR_ARG, "gtg_solve: a %d-sweep fused solve needs n >= %d (n = %d)", H + 1, kMin, S.n);
    const int rows = part ? S.L + 2 * S.ext : S.n;
    const int64_t tiles = (int64_t)((S.n + GW - 1) / GW) * ((rows + GH - 1) / GH);
    const bool db = dv.Y != nullptr;
    if (db && part) return set_error(MPBP_ERR_ARG, "gtg_solve: the fused D right-hand side is one-GPU only");
    // 512 lanes own rings 1 .. H - 1 one cell each (GtgTile::rings(H - 1) <= 512 cells)
    if constexpr (GtgTile<H, GW, GH>::rings(H - 1) <= 512) {
        if (KO().gtg_tpb == 512) {
            if (db) k_gtg_solve<H, false, 512, true, GW, GH><<<(unsigned)tiles, 512, 0, st>>>(S, b, diag, ck, out, dv);
            else if (part)
                k_gtg_solve<H, true, 512, false, GW, GH><<<(unsigned)tiles, 512, 0, st>>>(S, b, diag, ck, out, dv);
            else k_gtg_solve<H, false, 512, false, GW, GH><<<(unsigned)tiles, 512, 0, st>>>(S, b, diag, ck, out, dv);
            MPBP_HIP(hipGetLastError());
            return MPBP_OK;
        }
    }
    {
        if (db) k_gtg_solve<H, false, 256, true, GW, GH><<<(unsigned)tiles, 256, 0, st>>>(S, b, diag, ck, out, dv);
        else if (part) k_gtg_solve<H, true, 256, false, GW, GH><<<(unsigned)tiles, 256, 0, st>>>(S, b, diag, ck, out, dv);
        else k_gtg_solve<H, false, 256, false, GW, GH><<<(unsigned)tiles, 256, 0, st>>>(S, b, diag, ck, out, dv);
    }
    MPBP_HIP(hipGetLastError());
    return MPBP_OK;
}
// kernel option gtg_solve_tile: 32 x 16 tiles (1) -- shorter halo rings, fewer staged and halo cells per output, as
// k_fsolve_w -- or the 64 x 8 tile (0); every cell's operations are the same, so are the bits
template <int H>
int launch_gtg_solve_t(const GtGStencilDev& S, const double* b, const double* diag, const ChebK& ck, double* out,
                       hipStream_t st, GtgD dv = GtgD{}) {
    return KO().gtg_solve_tile ? launch_gtg_solve_g<H, 32, 16>(S, b, diag, ck, out, st, dv)
                               : launch_gtg_solve_g<H, kGTW, kGTH>(S, b, diag, ck, out, st, dv);
}
// The tile's staged cells must wrap onto the grid at most once each way (P.wrap), so n >= a tile plus its halos.
// part: under a row partition (the CA schedule's solves), else one GPU.
bool gtg_fused_ok(const mpbp_schur_plan* p, bool part = false) {
    const mpbp_inner_solver& in = p->inner_P;
    return KO().gtg_fused && p->pg_stencil && (p->halo != nullptr) == part && in.kind == MPBP_INNER_CHEBYSHEV &&
           in.sweeps >= 2 && in.sweeps <= 6 && in.lmax > in.lmin && in.lmin >= 0.0 &&
           p->f_prm.n >= kGTW + kGTH + 2 * (in.sweeps - 1);
}
// part: the CA schedule's owned + ext ghost rows (b and diag in the pressure ghost layout), else one GPU.
// dv.Y set (one GPU): b is not read; rhs = D dv.Y + dv.vp is built inside (k_gtg_solve<DB>).
int gtg_solve_fused(const mpbp_schur_plan* p, const double* b, double* out, hipStream_t st,
                    const mpbp_row_part* part = nullptr, const double* diag = nullptr, GtgD dv = GtgD{}) {
    PGDev P;
    const int rc = make_pgstencil(&p->f_prm, p->f_cell, part, &P);
    if (rc) return rc;
    const int K = p->inner_P.sweeps;
    if (part && (P.which != 3 || P.h < P.ext + K - 1 || P.oh < P.ext || !diag))
        return set_error(MPBP_ERR_ARG, "gtg_solve_fused: owned + ext rows need b ext + K - 1 deep and the ext diagonal");
    if (!part) diag = p->diag_P;
    ChebK ck{};
    double c1[64] = {}, c2[64] = {};
    cheb_coeffs(p->inner_P.lmin, p->inner_P.lmax, K, c1, c2);
    for (int s = 0; s < K; ++s) {
        ck.c1[s] = c1[s];
        ck.c2[s] = c2[s];
    }
    const GtGStencilDev S{P};
    switch (K - 1) {
    case 1: return launch_gtg_solve_t<1>(S, b, diag, ck, out, st, dv);
    case 2: return launch_gtg_solve_t<2>(S, b, diag, ck, out, st, dv);
    case 3: return launch_gtg_solve_t<3>(S, b, diag, ck, out, st, dv);
    case 4: return launch_gtg_solve_t<4>(S, b, diag, ck, out, st, dv);
    case 5: return launch_gtg_solve_t<5>(S, b, diag, ck, out, st, dv);
    default: return set_error(MPBP_ERR_ARG, "gtg_solve_fused: 2..6 sweeps");
    }
}

}  // namespace

extern "C" int mpbp_gtg_stencil_cheb_solve(const mpbp_stokes_params* prm, const double* cell, const double* b,
                                           const double* diag, double lmin, double lmax, int32_t sweeps,
                                           double* x_out, void* stream) {
    if (!prm || !cell || !b || !diag || !x_out || b == x_out || sweeps < 2 || sweeps > 6 || !(lmax > lmin) ||
        !(lmin >= 0.0))
        return set_error(MPBP_ERR_ARG, "gtg_stencil_cheb_solve: bad args (2..6 sweeps, 0 <= lmin < lmax)");
    PGDev P;
    const int rc = make_pgstencil(prm, cell, nullptr, &P);
    if (rc) return rc;
    ChebK ck{};
    double c1[64] = {}, c2[64] = {};
    cheb_coeffs(lmin, lmax, sweeps, c1, c2);
    for (int s = 0; s < sweeps; ++s) {
        ck.c1[s] = c1[s];
        ck.c2[s] = c2[s];
    }
    const GtGStencilDev S{P};
    const hipStream_t st = as_stream(stream);
    switch (sweeps - 1) {
    case 1: return launch_gtg_solve_t<1>(S, b, diag, ck, x_out, st);
    case 2: return launch_gtg_solve_t<2>(S, b, diag, ck, x_out, st);
    case 3: return launch_gtg_solve_t<3>(S, b, diag, ck, x_out, st);
    case 4: return launch_gtg_solve_t<4>(S, b, diag, ck, x_out, st);
    default: return launch_gtg_solve_t<5>(S, b, diag, ck, x_out, st);
    }
}

namespace {
// The first sweep of a Gt_G Chebyshev solve staging a precomputed x0 = d0 (one GPU, matrix-free Gt_G).
int gtg_first_sweep_x0(const mpbp_schur_plan* p, const double* x0, const double* b, double c1, double c2, double* d,
                       const double* sub, double* xo, int store_d, hipStream_t st) {
    PGDev P;
    const int rc = make_pgstencil(&p->f_prm, p->f_cell, nullptr, &P);
    if (rc) return rc;
    return launch_march(GtGStencilDev{P}, XPlain{x0}, EpiChebFirst{b, d, c1, c2, sub, xo, store_d}, pg_rows(), st);
}

// The last two sweeps of a tolerance-mode F Chebyshev solve fused (k_march2): one GPU whole grid, or (ext >= 0) the CA
// schedule's owned + ext ghost rows.
template <class BS = BNone>
int f_pair(const mpbp_schur_plan* p, int ext, const double* x_in, const double* b, double* dir, double c1a, double c2a,
           double c1b, double c2b, const double* sub, double* x_out, hipStream_t st, const BS& bs = BS{}) {
    FStencilDev P;
    int rc;
    if (ext >= 0) {
        OpRef o{nullptr, nullptr, nullptr, p, false, 3, SOP_F};
        o.ext = ext;
        const mpbp_row_part q = stencil_part(o);
        rc = make_fstencil(&p->f_prm, p->f_cell, p->f_uface, p->f_vface, &q, &P);
    } else {
        rc = make_fstencil(&p->f_prm, p->f_cell, p->f_uface, p->f_vface, nullptr, &P);
    }
    if (rc) return rc;
    if (ext < 0 && KO().f_tile && ftile_ok(P.n))   // one GPU: the pair on 2D tiles
        return launch_ftile<false>(P, FTile{x_in, dir, b, sub, x_out, nullptr, c1a, c2a, c1b, c2b}, st, bs);
    return launch_march2(P, Fused2{x_in, dir, b, sub, x_out, nullptr, c1a, c2a, c1b, c2b}, st, bs);
}

// x = M^-1 b by `inner` sweeps from x0 = 0 (solve.py:251/254 F_inv / Gt_G_factorization roles).
// The final iterate goes to dst (sub - iterate when sub != NULL); ping/pong hold the others.  x0_pre (Gt_G,
// Chebyshev, fusable first sweep): the first iterate c2[0] b / diag already computed by b's producer.
// fn() bracketed by the plan's profiling events (mpbp_schur_plan.prof_events) when asked and not capturing.
template <class Fn>
int profiled(const mpbp_schur_plan* p, bool profile, hipStream_t st, Fn&& fn) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    const bool rec = profile && p->prof_events && p->prof_count && *p->prof_count < p->prof_capacity &&
                     hipStreamIsCapturing(st, &cs) == hipSuccess && cs == hipStreamCaptureStatusNone;
    if (rec) MPBP_HIP(record_event((hipEvent_t)p->prof_events[2 * *p->prof_count], st));
    const int rc = fn();
    if (rc) return rc;
    if (rec) {
        MPBP_HIP(record_event((hipEvent_t)p->prof_events[2 * *p->prof_count + 1], st));
        ++*p->prof_count;
    }
    return MPBP_OK;
}

int inner_solve(const Ctx& c, int32_t kind, const OpPair& op, const double* diag, const mpbp_inner_solver& in,
                int32_t nrows, const double* b, double* dst, const double* sub, double* ping, double* pong,
                double* dir, bool profile, const double* x0_pre = nullptr) {
    if (in.kind == MPBP_INNER_MG) {   // one GPU: V-cycles whose level 0 is this operator
        const mpbp_mg* m = kind == MPBP_VEC_VELOCITY ? c.p->mg_F : c.p->mg_P;
        if (!m)
            return set_error(MPBP_ERR_ARG, "schur_apply: a multigrid inner solve needs plan.mg_%s",
                             kind == MPBP_VEC_VELOCITY ? "F" : "P");
        if ((c.p->halo != nullptr) != (m->part_levels > 0))
            return set_error(MPBP_ERR_ARG, "schur_apply: a %s apply needs a %s multigrid hierarchy",
                             c.p->halo ? "row-partitioned" : "one-GPU", c.p->halo ? "row-partitioned" : "whole-grid");
        if (m->levels[0].nrows != nrows) return set_error(MPBP_ERR_ARG, "schur_apply: mg level 0 size mismatch");
        const MgFine f{op, diag, ping, pong, m->levels[0].r, dir, c.p->halo, c.p->halo_ctx, kind};
        return mg_solve(m, f, b, dst, sub, c.st);
    }
    const int K = in.sweeps;
    double c1[64] = {}, c2[64] = {};   // zeros for Jacobi (never read uninitialised)
    if (K < 1 || K > 64) return set_error(MPBP_ERR_ARG, "inner sweeps must be in [1, 64]");
    const bool cheb = in.kind == MPBP_INNER_CHEBYSHEV;
    if (cheb) {
        if (!(in.lmax > in.lmin) || !(in.lmin >= 0.0)) return set_error(MPBP_ERR_ARG, "bad Chebyshev interval");
        cheb_coeffs(in.lmin, in.lmax, K, c1, c2);
    } else if (in.kind != MPBP_INNER_JACOBI) {
        return set_error(MPBP_ERR_ARG, "unknown inner solver %d", in.kind);
    }
    // tolerance-mode F on one GPU: the whole solve as one launch
    if (cheb && f_pair_ok(c.p) && KO().f_solve && op.in.stencil && op.in.sop == SOP_F && op.bd.empty && op.in.which == 0 &&
        !c.p->halo && fsolve_ok(K, c.p->f_prm.n)) {
        FStencilDev P;
        int rc = make_fstencil(&c.p->f_prm, c.p->f_cell, c.p->f_uface, c.p->f_vface, nullptr, &P);
        if (rc) return rc;
        return profiled(c.p, profile, c.st, [&] { return launch_fsolve(P, K, c1, c2, b, sub, dst, c.st); });
    }
    double* cur = (K == 1) ? dst : ping;
    int s = 1, rc = MPBP_OK;
    if (K >= 2 && can_fuse_init(op)) {   // sweep 1 recomputes x0 = d0 from b and diag: no init pass
        double* nxt = K == 2 ? dst : pong;
        rc = (x0_pre && cheb && op.in.sop == SOP_GTG)
                 ? gtg_first_sweep_x0(c.p, x0_pre, b, c1[1], c2[1], dir, K == 2 ? sub : nullptr, nxt, K == 2 ? 0 : 1,
                                      c.st)
                 : op_first_sweep(op.in, cheb, b, diag, c2[0], c1[1], c2[1], dir, K == 2 ? sub : nullptr, nxt, c.st,
                                  K == 2 ? 0 : 1);
        if (rc) return rc;
        cur = nxt;
        s = 2;
    } else {
        const double* s0 = (K == 1) ? sub : nullptr;
        rc = op_init(op.in, nrows, cheb, b, diag, c2[0], dir, s0, cur, c.st);
        if (rc) return rc;
    }
    // tolerance-mode F on one GPU: the last two sweeps as one fused launch
    const bool pair_ok = cheb && f_pair_ok(c.p) && op.in.stencil && op.in.sop == SOP_F && op.bd.empty &&
                         op.in.which == 0 && !c.p->halo;
    while (s < K) {
        const bool pair = pair_ok && s == K - 2;
        const bool last = s == K - 1 || pair;
        double* nxt = last ? dst : (cur == ping ? pong : ping);
        const double* sb = last ? sub : nullptr;
        const mpbp_schur_plan* p = c.p;
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        const bool rec = profile && p->prof_events && p->prof_count && *p->prof_count < p->prof_capacity &&
                         hipStreamIsCapturing(c.st, &cs) == hipSuccess && cs == hipStreamCaptureStatusNone;
        if (rec) MPBP_HIP(record_event((hipEvent_t)p->prof_events[2 * *p->prof_count], c.st));
        if (pair)
            rc = f_pair(p, -1, cur, b, dir, c1[s], c2[s], c1[s + 1], c2[s + 1], sb, nxt, c.st);
        else
            rc = two_phase(c, kind, cur, op, [&](const OpRef& o) {
                return cheb ? op_cheb(o, cur, b, diag, c1[s], c2[s], dir, sb, nxt, c.st, last ? 0 : 1)
                            : op_jacobi(o, cur, b, diag, sb, nxt, c.st);
            });
        if (rc) return rc;
        if (rec) {
            MPBP_HIP(record_event((hipEvent_t)p->prof_events[2 * *p->prof_count + 1], c.st));
            ++*p->prof_count;
        }
        cur = nxt;
        s += pair ? 2 : 1;
    }
    return MPBP_OK;
}

// u = Finv_v - F^-1 (G x_p) (solve.py:273-276) with the second F solve's right-hand side W = G x_p recomputed
// inside each of its sweeps from x_p (GxB) instead of a G launch writing W: one GPU, matrix-free F and G,
// Chebyshev with K >= 2 sweeps.  Each row performs the IEEE operations of G's row followed by inner_solve's
// sweep (bit-identical), and the solve reads one pressure field instead of W's four velocity fields.
int f_solve_gx(const Ctx& c, const double* xp, const mpbp_inner_solver& in, double* dst, const double* sub,
               double* ping, double* pong, double* dir, bool profile) {
    const mpbp_schur_plan* p = c.p;
    const int K = in.sweeps;
    if (in.kind != MPBP_INNER_CHEBYSHEV || K < 2 || K > 64 || !(in.lmax > in.lmin) || !(in.lmin >= 0.0))
        return set_error(MPBP_ERR_ARG, "schur_apply (fused G): needs a Chebyshev F solve of 2..64 sweeps");
    double c1[64] = {}, c2[64] = {};
    cheb_coeffs(in.lmin, in.lmax, K, c1, c2);
    FStencilDev P;
    int rc = make_fstencil(&p->f_prm, p->f_cell, p->f_uface, p->f_vface, nullptr, &P);
    if (rc) return rc;
    PGDev G;
    rc = make_pgstencil(&p->f_prm, p->f_cell, nullptr, &G);
    if (rc) return rc;
    const GxB bs{xp, G.d_p, G.inv, G.minv, G.n};
    if (f_pair_ok(p) && KO().f_solve && fsolve_ok(K, P.n))   // the whole solve as one launch
        return profiled(p, profile, c.st, [&] { return launch_fsolve(P, K, c1, c2, nullptr, sub, dst, c.st, bs); });
    double* cur = K == 2 ? dst : pong;
    if (p->f_numerics == MPBP_NUMERICS_FAST && KO().f_tile && ftile_ok(P.n))   // x0 and sweep 1 on 2D tiles
        rc = launch_ftile<true>(P, FTile{nullptr, nullptr, nullptr, K == 2 ? sub : nullptr, cur, K == 2 ? nullptr : dir,
                                         0.0, c2[0], c1[1], c2[1]}, c.st, bs);
    else
    rc = with_f_policy(P, p->f_numerics == MPBP_NUMERICS_FAST, [&](const auto& Q) {
        return launch_march_init(Q, nullptr, c2[0], EpiChebFirst{nullptr, dir, c1[1], c2[1], K == 2 ? sub : nullptr, cur,
                                                                 K == 2 ? 0 : 1}, KO().march_rows, c.st, bs);
    });
    if (rc) return rc;
    for (int s = 2; s < K;) {
        const bool pair = f_pair_ok(p) && s == K - 2;
        const bool last = s == K - 1 || pair;
        double* nxt = last ? dst : (cur == ping ? pong : ping);
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        const bool rec = profile && p->prof_events && p->prof_count && *p->prof_count < p->prof_capacity &&
                         hipStreamIsCapturing(c.st, &cs) == hipSuccess && cs == hipStreamCaptureStatusNone;
        if (rec) MPBP_HIP(record_event((hipEvent_t)p->prof_events[2 * *p->prof_count], c.st));
        if (pair)
            rc = f_pair(p, -1, cur, nullptr, dir, c1[s], c2[s], c1[s + 1], c2[s + 1], sub, nxt, c.st, bs);
        else
            rc = with_f_policy(P, p->f_numerics == MPBP_NUMERICS_FAST, [&](const auto& Q) {
                return launch_march(Q, XPlain{cur}, EpiCheb{cur, nullptr, nullptr, dir, c1[s], c2[s], last ? sub : nullptr,
                                                            nxt, last ? 0 : 1}, KO().march_rows, c.st, bs);
            });
        if (rc) return rc;
        if (rec) {
            MPBP_HIP(record_event((hipEvent_t)p->prof_events[2 * *p->prof_count + 1], c.st));
            ++*p->prof_count;
        }
        cur = nxt;
        s += pair ? 2 : 1;
    }
    return MPBP_OK;
}

// The upper block form's u = F^-1 (v_u - G x_p) (mpbp_schur_plan.form) as ONE whole-solve launch whose right-hand side
// is built per cell from v_u and x_p (GxR): no G launch, W never stored, the bits of the G launch in MPBP_SPMV_RESID
// mode followed by inner_solve.  One GPU, matrix-free F and G, fast numerics, Chebyshev F of 3 or 4 sweeps on a grid
// the launch takes (fsolve_ok); *taken says whether it ran -- otherwise nothing was launched and the caller runs the pair.
int f_solve_gr(const Ctx& c, const double* xp, const double* v_u, const mpbp_inner_solver& in, double* dst, bool profile,
               bool* taken) {
    const mpbp_schur_plan* p = c.p;
    const int K = in.sweeps;
    *taken = false;
    if (p->halo || !p->f_stencil || !p->pg_stencil || in.kind != MPBP_INNER_CHEBYSHEV || !(in.lmax > in.lmin) ||
        !(in.lmin >= 0.0) || !f_pair_ok(p) || !KO().f_solve || !fsolve_ok(K, p->f_prm.n))
        return MPBP_OK;
    double c1[64] = {}, c2[64] = {};
    cheb_coeffs(in.lmin, in.lmax, K, c1, c2);
    FStencilDev P;
    int rc = make_fstencil(&p->f_prm, p->f_cell, p->f_uface, p->f_vface, nullptr, &P);
    if (rc) return rc;
    PGDev G;
    rc = make_pgstencil(&p->f_prm, p->f_cell, nullptr, &G);
    if (rc) return rc;
    const GxR bs{{xp, G.d_p, G.inv, G.minv, G.n}, v_u};
    *taken = true;
    return profiled(p, profile, c.st, [&] { return launch_fsolve(P, K, c1, c2, nullptr, nullptr, dst, c.st, bs); });
}

}  // namespace
