// The communication-avoiding schedule of the row partition (ext_op, ca_inner_solve, schur_apply_ca) and
// mpbp_schur_apply.  Continues schur_inner.inc's namespace; needs it, q13.inc, schur_ops.inc and mg_accel.inc.
// A fragment of mpbp.hip, included there once and in order: not a self-contained header.
namespace {

// ---- communication-avoiding schedule (row partition) ----
// A stencil operator over the owned rows and `ext` ghost rows each side.
OpRef ext_op(const mpbp_schur_plan* p, int32_t sop, int ext) {
    OpRef o{nullptr, nullptr, nullptr, p, false, 3, sop};
    o.ext = ext;
    return o;
}

// Inner solve whose result is needed on the owned rows and d_out ghost rows each side: no exchange --
// sweep s (of S = K - 1) runs on d_out + S - s ghost rows, the fused first sweep stages x0 from b and the
// ghost-row diagonal d_out + S rows deep.  Same IEEE operations per row as the one-GPU solve.
int ca_inner_solve(const Ctx& c, int32_t sop, const double* b, const double* diag_ext, const mpbp_inner_solver& in,
                   int32_t n_init, double* dst, const double* sub, double* ping, double* pong, double* dir, int d_out,
                   bool profile) {
    const mpbp_schur_plan* p = c.p;
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
    if (K == 1) {   // x = x0 elementwise on every row the caller needs (n_init: owned, or the whole ext vector)
        if (n_init <= 0) return MPBP_OK;
        if (cheb) k_cheb_init<<<grid_for(n_init), kBlock, 0, c.st>>>(n_init, b, diag_ext, c2[0], dir, sub, dst);
        else k_jacobi_init<<<grid_for(n_init), kBlock, 0, c.st>>>(n_init, b, diag_ext, sub, dst);
        MPBP_HIP(hipGetLastError());
        return MPBP_OK;
    }
    // Gt_G: the whole Chebyshev solve as one tiled launch over the owned + d_out ghost rows (bit-identical)
    if (cheb && sop == SOP_GTG && !sub && gtg_fused_ok(p, true)) {
        const mpbp_row_part q = stencil_part(ext_op(p, SOP_GTG, d_out));
        if (q.halo >= d_out + K - 1) return gtg_solve_fused(p, b, dst, c.st, &q, diag_ext);
    }
    // tolerance-mode F: the whole solve as one tiled launch over the owned + d_out ghost rows
    if (cheb && sop == SOP_F && f_pair_ok(p) && KO().f_solve && fsolve_ok(K, p->f_prm.n)) {
        const mpbp_row_part q = stencil_part(ext_op(p, SOP_F, d_out));
        FStencilDev P;
        int rc = make_fstencil(&p->f_prm, p->f_cell, p->f_uface, p->f_vface, &q, &P);
        if (rc) return rc;
        if (P.h >= d_out + K - 1)
            return profiled(p, profile, c.st, [&] { return launch_fsolve(P, K, c1, c2, b, sub, dst, c.st); });
    }
    double* cur = K == 2 ? dst : pong;
    int rc = op_first_sweep(ext_op(p, sop, d_out + K - 2), cheb, b, diag_ext, c2[0], c1[1], c2[1], dir,
                            K == 2 ? sub : nullptr, cur, c.st, K == 2 ? 0 : 1);
    if (rc) return rc;
    for (int s = 2; s < K;) {
        const bool pair = cheb && sop == SOP_F && f_pair_ok(p) && s == K - 2;
        const bool last = s == K - 1 || pair;
        double* nxt = last ? dst : (cur == ping ? pong : ping);
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        const bool rec = profile && p->prof_events && p->prof_count && *p->prof_count < p->prof_capacity &&
                         hipStreamIsCapturing(c.st, &cs) == hipSuccess && cs == hipStreamCaptureStatusNone;
        if (rec) MPBP_HIP(record_event((hipEvent_t)p->prof_events[2 * *p->prof_count], c.st));
        const OpRef o = ext_op(p, sop, d_out + K - 1 - s);
        if (pair)   // level B on d_out ghost rows (the last sweep's), level A one deeper (sweep K-2's)
            rc = f_pair(p, d_out, cur, b, dir, c1[s], c2[s], c1[s + 1], c2[s + 1], sub, nxt, c.st);
        else
            rc = cheb ? op_cheb(o, cur, b, nullptr, c1[s], c2[s], dir, last ? sub : nullptr, nxt, c.st, last ? 0 : 1)
                      : op_jacobi(o, cur, b, nullptr, last ? sub : nullptr, nxt, c.st);
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

// The CA schedule's second F solve (owned rows) with W = G x_p recomputed inside its sweeps (GxB over x_p's ghost
// layout, which holds S_F + 1 ghost rows each side -- the G launch's d_W = S_F plus its one-row reach): no G launch
// and no W buffer; the same IEEE operations per row as ca_inner_solve after the G launch.
int ca_f_solve_gx(const Ctx& c, const double* xp, const mpbp_inner_solver& in, double* dst, const double* sub,
                  double* ping, double* pong, double* dir, bool profile) {
    const mpbp_schur_plan* p = c.p;
    const int K = in.sweeps;
    if (in.kind != MPBP_INNER_CHEBYSHEV || K < 2 || K > 64 || !(in.lmax > in.lmin) || !(in.lmin >= 0.0))
        return set_error(MPBP_ERR_ARG, "schur_apply (CA, fused G): needs a Chebyshev F solve of 2..64 sweeps");
    double c1[64] = {}, c2[64] = {};
    cheb_coeffs(in.lmin, in.lmax, K, c1, c2);
    PGDev G;
    int rc = make_pgstencil(&p->f_prm, p->f_cell, &p->p_part, &G);
    if (rc) return rc;
    const GxBPart bs{xp, G.d_p, G.inv, G.minv, G.n, G.L, G.h};
    auto fpol = [&](int ext, FStencilDev* P) {
        const mpbp_row_part q = stencil_part(ext_op(p, SOP_F, ext));
        return make_fstencil(&p->f_prm, p->f_cell, p->f_uface, p->f_vface, &q, P);
    };
    FStencilDev P;
    if (f_pair_ok(p) && KO().f_solve && fsolve_ok(K, p->f_prm.n) && bs.h >= K) {   // the whole solve as one launch
        if ((rc = fpol(0, &P))) return rc;
        if (P.h >= K - 1)
            return profiled(p, profile, c.st, [&] { return launch_fsolve(P, K, c1, c2, nullptr, sub, dst, c.st, bs); });
    }
    if ((rc = fpol(K - 2, &P))) return rc;
    double* cur = K == 2 ? dst : pong;
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
        if (pair) {
            rc = f_pair(p, 0, cur, nullptr, dir, c1[s], c2[s], c1[s + 1], c2[s + 1], sub, nxt, c.st, bs);
        } else {
            if ((rc = fpol(K - 1 - s, &P))) return rc;
            rc = with_f_policy(P, p->f_numerics == MPBP_NUMERICS_FAST, [&](const auto& Q) {
                return launch_march(Q, XPlain{cur}, EpiCheb{cur, nullptr, nullptr, dir, c1[s], c2[s], last ? sub : nullptr,
                                                            nxt, last ? 0 : 1}, KO().march_rows, c.st, bs);
            });
        }
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

// The exchange of one vector, complete before the next launch.
void ca_exchange(const Ctx& c, int32_t kind, double* x_ext) {
    c.p->halo(c.p->halo_ctx, kind, x_ext, MPBP_HALO_BEGIN, (void*)c.st);
    c.p->halo(c.p->halo_ctx, kind, x_ext, MPBP_HALO_END, (void*)c.st);
}

// solve.py:257-277 with 2 halo exchanges: v (velocity and pressure parts) before the first F solve, x_b
// before the second Gt_G solve; every other operator runs on the ghost rows its successors read.
int schur_apply_ca(const Ctx& c, const double* v, double* out) {
    const mpbp_schur_plan* p = c.p;
    const int SF = p->inner_F.sweeps - 1, SP = p->inner_P.sweeps - 1, q = p->ca_reach_q;
    const int d_xa = q, d_rhs = d_xa + SP, d_Y = d_rhs + 1, d_W = SF, d_xp = d_W + 1, d_xb = d_xp + SP;
    if (SF < 0 || SP < 0 || q < 1 || p->f_part.halo < d_Y + SF || p->p_part.halo < d_rhs || p->p_part.halo < d_xb ||
        p->p_part.halo < q || !p->wu_ext || !p->diag_F_ext || !p->diag_P_ext)
        return set_error(MPBP_ERR_ARG, "schur_apply (CA): halo depths %d/%d below the schedule's %d/%d, or ext "
                         "buffers missing", p->f_part.halo, p->p_part.halo, d_Y + SF, d_rhs > d_xb ? d_rhs : d_xb);
    double *Y = p->wu[0], *U0 = p->wu[1], *U1 = p->wu[2], *Ud = p->wu[3], *Vu = p->wu_ext;
    double *Prhs = p->wp[0], *Pxa = p->wp[1], *Pxb = p->wp[2], *Pxp = p->wp[3];
    double *P0 = p->wp[4], *P1 = p->wp[5], *Pd = p->wp[6];
    double* Vp = Pxb;   // v's pressure part lives in x_b's buffer until Gt_F_G overwrites it
    int rc;
    // v with its halo: velocity d_Y + S_F rows deep, pressure d_rhs rows deep (one exchange each)
    MPBP_HIP(hipMemcpyAsync(Vu, v, sizeof(double) * (size_t)p->nu, hipMemcpyDeviceToDevice, c.st));
    MPBP_HIP(hipMemcpyAsync(Vp, v + p->nu, sizeof(double) * (size_t)p->np, hipMemcpyDeviceToDevice, c.st));
    if (p->halo_pair) {
        p->halo_pair(p->halo_ctx, Vu, Vp, (void*)c.st);
    } else {
        ca_exchange(c, MPBP_VEC_VELOCITY, Vu);
        ca_exchange(c, MPBP_VEC_PRESSURE, Vp);
    }
    // 1. Finv_v on owned + d_Y ghost rows                                    solve.py:258
    rc = ca_inner_solve(c, SOP_F, Vu, p->diag_F_ext, p->inner_F, p->nu_ext, Y, nullptr, U0, U1, Ud, d_Y, true);
    if (rc) return rc;
    // 2. rhs = D Finv_v + v_p on owned + d_rhs ghost rows                      solve.py:259
    rc = op_spmv(ext_op(p, SOP_D, d_rhs), MPBP_SPMV_ADD, Y, Vp, Prhs, c.st);
    if (rc) return rc;
    // 3. x_a = Gt_G^-1 rhs on owned + q ghost rows                            solve.py:265
    rc = ca_inner_solve(c, SOP_GTG, Prhs, p->diag_P_ext, p->inner_P, p->np_ext, Pxa, nullptr, P0, P1, Pd, d_xa, false);
    if (rc) return rc;
    // 4. x_b = Gt_F_G x_a on the owned rows (its columns reach q ghost rows)  solve.py:267
    //    (tolerance mode: the diamond's upper half over the rank's row block, as k_q13<SYM> on one GPU)
    if (q13p_ok(p)) {
        rc = launch_q13p(p, Pxa, EpiStore{Pxb}, c.st);
    } else {
        const OpPair Q = make_op(p, p->GtFG, p->Q_int, p->Q_bnd, p->Qs_int, p->Qs_bnd);
        rc = op_spmv(Q.in, MPBP_SPMV_STORE, Pxa, nullptr, Pxb, c.st);
        if (!rc) rc = op_spmv(Q.bd, MPBP_SPMV_STORE, Pxa, nullptr, Pxb, c.st);
    }
    if (rc) return rc;
    ca_exchange(c, MPBP_VEC_PRESSURE, Pxb);
    // 5. x_p = Gt_G^-1 x_b on owned + d_xp ghost rows                         solve.py:271
    rc = ca_inner_solve(c, SOP_GTG, Pxb, p->diag_P_ext, p->inner_P, p->np_ext, Pxp, nullptr, P0, P1, Pd, d_xp, false);
    if (rc) return rc;
    MPBP_HIP(hipMemcpyAsync(out + p->nu, Pxp, sizeof(double) * (size_t)p->np, hipMemcpyDeviceToDevice, c.st));
    // 6.+7. fused: the second F solve recomputes G x_p in its sweeps (Chebyshev F)   solve.py:273-276
    if (p->fuse_g && p->inner_F.kind == MPBP_INNER_CHEBYSHEV && p->inner_F.sweeps >= 2)
        return ca_f_solve_gx(c, Pxp, p->inner_F, out, Y, U0, U1, Ud, true);
    // 6. G x_p on owned + d_W ghost rows (into v's velocity buffer)          solve.py:273
    rc = op_spmv(ext_op(p, SOP_G, d_W), MPBP_SPMV_STORE, Pxp, nullptr, Vu, c.st);
    if (rc) return rc;
    // 7. u = Finv_v - F^-1 (G x_p) on the owned rows                          solve.py:274-276
    return ca_inner_solve(c, SOP_F, Vu, p->diag_F_ext, p->inner_F, p->nu, out, Y, U0, U1, Ud, 0, true);
}

}  // namespace

// Multigrid level 1 of the plan's F (kind MPBP_VEC_VELOCITY) or Gt_G (MPBP_VEC_PRESSURE) hierarchy applied matrix-free
// as ONE fused launch (k_gal1 / k_gal1p: R_0 (A_0 (P_0 x))), y = op(A_1 x) with the modes of mpbp_spmv -- the kernel the
// tolerance-mode multigrid apply runs for its level-1 sweeps and residuals, exposed for timing (bench.py mg_apply).
extern "C" int mpbp_mg_level1_apply(const mpbp_schur_plan* p, int32_t kind, int32_t mode, const double* x,
                                    const double* z, double* y, void* stream) {
    if (!p || !x || !y || (mode != MPBP_SPMV_STORE && !z)) return set_error(MPBP_ERR_ARG, "mg_level1_apply: bad args");
    if (int rc = check_opts(p->opts, "mg_level1_apply")) return rc;
    const OptsScope scope(p->opts);
    const mpbp_mg* m = kind == MPBP_VEC_VELOCITY ? p->mg_F : kind == MPBP_VEC_PRESSURE ? p->mg_P : nullptr;
    if (!m || p->halo || p->f_numerics != MPBP_NUMERICS_FAST || KO().mg_galerkin_mf != 2)
        return set_error(MPBP_ERR_ARG, "mg_level1_apply: a one-GPU fast plan with that multigrid hierarchy, "
                                       "kernel option mg_galerkin_mf = 2");
    const int sop = kind == MPBP_VEC_VELOCITY ? SOP_F : SOP_GTG;
    if ((sop == SOP_F && !p->f_stencil) || (sop == SOP_GTG && (!p->pg_stencil || !KO().mg_galerkin_mf_p)))
        return set_error(MPBP_ERR_ARG, "mg_level1_apply: the level-0 operator is not matrix-free");
    const OpPair fine = make_stencil_op(p, sop, false);
    const MgGal g{m, fine.in, nullptr, nullptr};
    const hipStream_t st = as_stream(stream);
    bool done = false;
    int rc = MPBP_OK;
    switch (mode) {
    case MPBP_SPMV_STORE: rc = gal_fused(g, XPlain{x}, EpiStore{y}, st, &done); break;
    case MPBP_SPMV_ADD: rc = gal_fused(g, XPlain{x}, EpiAdd{z, y}, st, &done); break;
    case MPBP_SPMV_RESID: rc = gal_fused(g, XPlain{x}, EpiResid{z, y}, st, &done); break;
    default: return set_error(MPBP_ERR_ARG, "mg_level1_apply: unknown mode %d", mode);
    }
    if (rc) return rc;
    return done ? MPBP_OK : set_error(MPBP_ERR_ARG, "mg_level1_apply: the grid / transfer kinds do not take the fused kernel");
}

extern "C" int mpbp_schur_apply(const mpbp_schur_plan* p, const double* v, double* out, void* stream) {
    if (!p || !v || !out) return set_error(MPBP_ERR_ARG, "schur_apply: bad args");
    for (int i = 0; i < 4; ++i)
        if (!p->wu[i]) return set_error(MPBP_ERR_ARG, "schur_apply: missing velocity workspace");
    for (int i = 0; i < 7; ++i)
        if (!p->wp[i]) return set_error(MPBP_ERR_ARG, "schur_apply: missing pressure workspace");
    if (!p->wu_owned || !p->diag_F || !p->diag_P) return set_error(MPBP_ERR_ARG, "schur_apply: missing operands");
    const int32_t form = p->form;
    if (form != MPBP_FORM_FULL && form != MPBP_FORM_UPPER && form != MPBP_FORM_LOWER && form != MPBP_FORM_DIAGONAL)
        return set_error(MPBP_ERR_ARG, "schur_apply: unknown block form %d (MPBP_FORM_*)", form);
    if (form != MPBP_FORM_FULL && p->halo)
        return set_error(MPBP_ERR_ARG, "schur_apply: the upper, lower and diagonal block forms are one-GPU only");
    const bool f_first = form != MPBP_FORM_UPPER;                           // F^-1 v_u comes first ...
    const bool d_rhs = form == MPBP_FORM_FULL || form == MPBP_FORM_LOWER;   // ... and D of it joins the pressure rhs
    if (int rc = check_opts(p->opts, "schur_apply")) return rc;
    const OptsScope scope(p->opts);
    const Ctx c{p, as_stream(stream)};
    // the CA schedule needs every operator but Gt_F_G matrix-free on the marching kernel; otherwise the
    // per-sweep exchanges below (its deeper halos serve them as well)
    if (p->ca && p->halo && p->f_stencil && p->pg_stencil) return schur_apply_ca(c, v, out);
    if (p->f_stencil && p->halo && p->f_part.halo < 1)
        return set_error(MPBP_ERR_ARG, "schur_apply: a partitioned F stencil needs f_part");
    if (p->pg_stencil && p->halo && (p->p_part.halo < 1 || p->f_part.halo < 1))
        return set_error(MPBP_ERR_ARG, "schur_apply: partitioned D / G / Gt_G stencils need f_part and p_part");
    if ((p->f_stencil || p->pg_stencil) && !p->f_cell)
        return set_error(MPBP_ERR_ARG, "schur_apply: stencil operators need the thn tables");
    const bool part = p->halo != nullptr && !p->halo_first;   // stencils split interior / boundary rows
    const OpPair F = p->f_stencil ? make_stencil_op(p, SOP_F, part)
                                  : make_op(p, p->F, p->F_int, p->F_bnd, p->Fs_int, p->Fs_bnd);
    const OpPair D = p->pg_stencil ? make_stencil_op(p, SOP_D, part)
                                   : make_op(p, p->D, p->D_int, p->D_bnd, p->Ds_int, p->Ds_bnd);
    const OpPair G = p->pg_stencil ? make_stencil_op(p, SOP_G, part)
                                   : make_op(p, p->G, p->G_int, p->G_bnd, p->Gs_int, p->Gs_bnd);
    const OpPair P = p->pg_stencil ? make_stencil_op(p, SOP_GTG, part)
                                   : make_op(p, p->GtG, p->P_int, p->P_bnd, p->Ps_int, p->Ps_bnd);
    const OpPair Q = make_op(p, p->GtFG, p->Q_int, p->Q_bnd, p->Qs_int, p->Qs_bnd);
    const double* v_u = v;
    const double* v_p = v + p->nu;
    double* out_u = out;
    double* out_p = out + p->nu;
    // F^-1 v_u: the full form keeps it in Y for step 7; the lower and diagonal forms return it
    double *Y = form == MPBP_FORM_FULL ? p->wu[0] : out_u, *U0 = p->wu[1], *U1 = p->wu[2], *Ud = p->wu[3], *W = p->wu_owned;
    double *Prhs = p->wp[0], *Pxa = p->wp[1], *Pxb = p->wp[2], *Pxp = p->wp[3];
    double *P0 = p->wp[4], *P1 = p->wp[5], *Pd = p->wp[6];
    int rc;
    // one GPU, matrix-free D and Gt_G, Chebyshev Gt_G solves: b's producers (D, Gt_F_G) also write the first Gt_G
    // sweep's x0 = c2[0] b / diag into P0 (the solve's ping buffer, first overwritten by its second sweep)
    // ... unless each Gt_G solve runs as one fused launch (k_gtg_solve), which builds x0 itself
    const bool gfuse = gtg_fused_ok(p);
    const bool px0 = !gfuse && p->pg_stencil && !p->halo && p->inner_P.kind == MPBP_INNER_CHEBYSHEV &&
                     p->inner_P.sweeps >= 2 && p->inner_P.lmax > p->inner_P.lmin && p->inner_P.lmin >= 0.0 &&
                     p->inner_P.sweeps <= 64;
    double pc1[64] = {}, pc2[64] = {};
    if (px0) cheb_coeffs(p->inner_P.lmin, p->inner_P.lmax, p->inner_P.sweeps, pc1, pc2);
    // 1. Finv_v = F_inv @ v[:F.shape[1]]                                   solve.py:258
    if (f_first) {
        rc = inner_solve(c, MPBP_VEC_VELOCITY, F, p->diag_F, p->inner_F, p->nu, v_u, Y, nullptr, U0, U1, Ud, true);
        if (rc) return rc;
    }
    if (!d_rhs) {
        // upper and diagonal forms: 3. x_a = Gt_G^-1 v_p (no producer stages the solve's x0)
        rc = gfuse ? gtg_solve_fused(p, v_p, Pxa, c.st)
                   : inner_solve(c, MPBP_VEC_PRESSURE, P, p->diag_P, p->inner_P, p->np, v_p, Pxa, nullptr, P0, P1, Pd, false);
        if (rc) return rc;
    } else
    // 2.+3. fused: the first Gt_G solve builds rhs = D Finv_v + v_p itself          solve.py:259, 265
    if (gfuse && KO().gtg_drhs && p->pg_stencil && !px0) {
        rc = gtg_solve_fused(p, nullptr, Pxa, c.st, nullptr, nullptr, GtgD{Y, v_p});
        if (rc) return rc;
    } else {
    // 2. rhs_interim = D @ Finv_v + v[F.shape[1]:]                            solve.py:259
    if (px0)
        rc = d_rhs_x0(p, Y, v_p, Prhs, pc2[0], P0, c.st);
    else
        rc = two_phase(c, MPBP_VEC_VELOCITY, Y, D,
                       [&](const OpRef& o) { return op_spmv(o, MPBP_SPMV_ADD, Y, v_p, Prhs, c.st); });
    if (rc) return rc;
    // 3. x_a = Gt_G_factorization @ rhs_interim                             solve.py:265
    rc = gfuse ? gtg_solve_fused(p, Prhs, Pxa, c.st)
               : inner_solve(c, MPBP_VEC_PRESSURE, P, p->diag_P, p->inner_P, p->np, Prhs, Pxa, nullptr, P0, P1, Pd, false,
                             px0 ? P0 : nullptr);
    if (rc) return rc;
    }
    // 4. x_b = Gt_F_G @ x_a                                                solve.py:267
    //    (one GPU: the diamond layout when the plan has it)
    const bool qmf = qmf_ok(p);   // tolerance mode: the product as its factors, matrix-free (k_qmf)
    const bool qx0 = px0 && (p->q13 || qmf);
    if (qx0 && qmf)
        rc = launch_qmf(p, Pxa, EpiStoreX0{Pxb, p->diag_P, pc2[0], P0}, c.st);
    else if (qx0)
        rc = launch_q13(p->q13_n, p->q13, Pxa, EpiStoreX0{Pxb, p->diag_P, pc2[0], P0}, c.st,
                        KO().q13_sym && p->f_numerics == MPBP_NUMERICS_FAST);
    else if (qmf)
        rc = launch_qmf(p, Pxa, EpiStore{Pxb}, c.st);
    else if (p->q13 && !p->halo)   // tolerance mode: the symmetric product's upper half (k_q13<SYM>)
        rc = launch_q13(p->q13_n, p->q13, Pxa, EpiStore{Pxb}, c.st, KO().q13_sym && p->f_numerics == MPBP_NUMERICS_FAST);
    else if (q13p_ok(p)) {         // ... and on a row partition: x_a's ghost rows first, then the rank's rows
        ca_exchange(c, MPBP_VEC_PRESSURE, Pxa);
        rc = launch_q13p(p, Pxa, EpiStore{Pxb}, c.st);
    } else
        rc = two_phase(c, MPBP_VEC_PRESSURE, Pxa, Q,
                       [&](const OpRef& o) { return op_spmv(o, MPBP_SPMV_STORE, Pxa, nullptr, Pxb, c.st); });
    if (rc) return rc;
    // 5. x_p = Gt_G_factorization @ x_b                                    solve.py:271
    //    (one GPU: straight into the output, which G then reads; a partition needs x_p's ghost rows)
    if (!p->halo) Pxp = out_p;
    rc = gfuse ? gtg_solve_fused(p, Pxb, Pxp, c.st)
               : inner_solve(c, MPBP_VEC_PRESSURE, P, p->diag_P, p->inner_P, p->np, Pxb, Pxp, nullptr, P0, P1, Pd, false,
                             qx0 ? P0 : nullptr);
    if (rc) return rc;
    if (Pxp != out_p)
        MPBP_HIP(hipMemcpyAsync(out_p, Pxp, sizeof(double) * (size_t)p->np, hipMemcpyDeviceToDevice, c.st));
    if (form == MPBP_FORM_LOWER || form == MPBP_FORM_DIAGONAL) return MPBP_OK;   // u = F^-1 v_u is in place
    if (form == MPBP_FORM_UPPER) {
        // u = F^-1 (v_u - G x_p): one whole-solve launch that builds the right-hand side per cell (GxR), or
        if (p->fuse_g) {
            bool taken = false;
            rc = f_solve_gr(c, Pxp, v_u, p->inner_F, out_u, true, &taken);
            if (rc || taken) return rc;
        }
        // W = v_u - G x_p by the G operator, then the F solve
        rc = two_phase(c, MPBP_VEC_PRESSURE, Pxp, G,
                       [&](const OpRef& o) { return op_spmv(o, MPBP_SPMV_RESID, Pxp, v_u, W, c.st); });
        if (rc) return rc;
        return inner_solve(c, MPBP_VEC_VELOCITY, F, p->diag_F, p->inner_F, p->nu, W, out_u, nullptr, U0, U1, Ud, true);
    }
    // 6.+7. fused: the second F solve recomputes G x_p in its sweeps (one GPU, matrix-free F and G, Chebyshev F)
    if (p->fuse_g && !p->halo && p->f_stencil && p->pg_stencil && p->inner_F.kind == MPBP_INNER_CHEBYSHEV &&
        p->inner_F.sweeps >= 2)
        return f_solve_gx(c, Pxp, p->inner_F, out_u, Y, U0, U1, Ud, true);
    // 6. G_xp = G @ x_p                                                     solve.py:273
    rc = two_phase(c, MPBP_VEC_PRESSURE, Pxp, G,
                   [&](const OpRef& o) { return op_spmv(o, MPBP_SPMV_STORE, Pxp, nullptr, W, c.st); });
    if (rc) return rc;
    // 7. u = Finv_v - F_inv @ G_xp                                          solve.py:274-276
    return inner_solve(c, MPBP_VEC_VELOCITY, F, p->diag_F, p->inner_F, p->nu, W, out_u, Y, U0, U1, Ud, true);
}
