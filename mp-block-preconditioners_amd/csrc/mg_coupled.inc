// The phase-coupled multigrid smoother (mpbp_mg.smoother = MPBP_MG_SMOOTH_COUPLED): point-block Jacobi over the two
// phases.  Rows i and pi(i) = i +- nrows / 2 of a four-field velocity level are the network and solvent unknowns of one
// face; the smoother inverts their 2 x 2 block B_i = [[a, k], [k', a']] instead of the diagonal, so drag-dominated F
// (xi h^2 >> eta) keeps an O(1) smoothing interval.  Holds k_cpl_blocks and k_cpl_bound (setup), k_cpl_update (the
// sweep's second launch), EpiCplChebT (the sweep as one launch on the matrix-free F), their C entries and mg_smooth_cpl.  Needs mpbp.hip's prelude (Csr, f64x2, CellEpi, RcpOk),
// launchers.inc (to_csr, check_csr, cheb_coeffs), abi_core.inc's device_flags, abi_stencil.inc's make_fstencil /
// launch_fstencil and schur_ops.inc's OpPair / op_spmv.
// A fragment of mpbp.hip, included there once and in order: not a self-contained header.
namespace {

__device__ inline int32_t cpl_partner(int32_t i, int32_t H) { return i < H ? i + H : i - H; }

// Row i's line of B_i^-1: cpl_p = a' / det, cpl_q = (-k) / det with a = A[i,i], a' = A[pi,pi], k = A[i,pi], k' = A[pi,i]
// and det = a a' - k k' (an entry that is not stored reads as +0.0).  flags[0] counts the rows with a missing diagonal
// or a det that is not finite or not positive, flags[1] holds INT32_MAX - (the first of them).
__global__ void k_cpl_blocks(Csr A, int32_t nrows, double* cpl_p, double* cpl_q, unsigned* flags) {
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nrows) return;
    const int32_t pi = cpl_partner(i, nrows / 2);
    double a = 0.0, k = 0.0, a2 = 0.0, k2 = 0.0;
    bool fa = false, fa2 = false;
    for (int32_t e = A.rp[i]; e < A.rp[i + 1]; ++e) {
        const int32_t c = A.ci[e];
        if (c == i) { a = A.va[e]; fa = true; }
        if (c == pi) k = A.va[e];
    }
    for (int32_t e = A.rp[pi]; e < A.rp[pi + 1]; ++e) {
        const int32_t c = A.ci[e];
        if (c == pi) { a2 = A.va[e]; fa2 = true; }
        if (c == i) k2 = A.va[e];
    }
    const double det = a * a2 - k * k2;
    cpl_p[i] = a2 / det;
    cpl_q[i] = (-k) / det;
    if (!fa || !fa2 || !(det > 0.0) || !(det <= 1.7976931348623157e308)) {
        atomicAdd(&flags[0], 1u);
        atomicMax(&flags[1], (unsigned)(INT32_MAX - i));
    }
}

// max_i sum_c |p_i A[i,c] + q_i A[pi,c]| = ||B^-1 A||_inf: one row per lane, a two-pointer merge of rows i and pi(i)
// (columns ascending in both; out[1] counts the rows where they are not), an entry absent from one row contributing
// p (+0.0) resp. q (+0.0), the absolute values added left to right from 0.0; the maximum reduced as k_gershgorin's.
__global__ void k_cpl_bound(Csr A, int32_t nrows, const double* cpl_p, const double* cpl_q, unsigned long long* out) {
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    double s = 0.0;
    if (i < nrows) {
        const int32_t pi = cpl_partner(i, nrows / 2);
        const double p = cpl_p[i], q = cpl_q[i];
        int32_t e = A.rp[i], f = A.rp[pi];
        const int32_t e1 = A.rp[i + 1], f1 = A.rp[pi + 1];
        int32_t prev = -1;
        bool sorted = true;
        while (e < e1 || f < f1) {
            const int32_t ce = e < e1 ? A.ci[e] : INT32_MAX, cf = f < f1 ? A.ci[f] : INT32_MAX;
            const int32_t c = ce < cf ? ce : cf;
            const double v = ce == c ? A.va[e] : 0.0, w = cf == c ? A.va[f] : 0.0;
            s += fabs(p * v + q * w);
            e += ce == c;
            f += cf == c;
            sorted = sorted && c > prev;
            prev = c;
        }
        if (!sorted) atomicAdd(&out[1], 1ull);
    }
    // non-negative doubles order like their bit patterns (NaN: above every number, so a NaN bound is reported as one)
    for (int d = 32; d > 0; d >>= 1) {
        const double o = __shfl_xor(s, d, 64);
        s = o > s || o != o ? o : s;
    }
    if ((threadIdx.x & 63) == 0) atomicMax(&out[0], (unsigned long long)__double_as_longlong(s));
}

// The coupled sweep's update, after r = b - A x (the level's operator in MPBP_SPMV_RESID mode):
//   z_i = p_i r_i + q_i r_pi(i);  d_i = c1 d_i + c2 z_i;  x_i = x_i + d_i;  out_i = sub ? sub_i - x_i : x_i.
// xin NULL: the zero start, r is b and x0_i = d0_i = c2 z_i.  dzero: d is read as +0.0 (a restart's first sweep).
// store_d 0: d is not written (a solve's last sweep).
struct CplUpd {
    const double *p, *q, *r, *xin, *sub;
    double *d, *out;
    double c1, c2;
    int32_t H;   // nrows / 2
    int32_t dzero, store_d;
};
template <class T>
__device__ inline void cpl_update_row(const CplUpd& a, int64_t u, T r_own, T r_partner) {
    const T p = reinterpret_cast<const T*>(a.p)[u], q = reinterpret_cast<const T*>(a.q)[u];
    const T z = p * r_own + q * r_partner;
    T x, d;
    if (!a.xin) {
        d = a.c2 * z;
        x = d;
    } else {
        T dv = T(0.0);
        if (!a.dzero) dv = reinterpret_cast<const T*>(a.d)[u];
        d = a.c1 * dv + a.c2 * z;
        x = reinterpret_cast<const T*>(a.xin)[u] + d;
    }
    if (a.store_d) reinterpret_cast<T*>(a.d)[u] = d;
    reinterpret_cast<T*>(a.out)[u] = a.sub ? reinterpret_cast<const T*>(a.sub)[u] - x : x;
}
// One thread owns rows i and i + H (T = double), or i, i + 1 and their partners (T = f64x2: H even, every pointer
// 16-byte aligned), so r is read once.  The pointers carry no __restrict__: out may be xin; a lane reads before it writes.
template <class T>
__global__ void __launch_bounds__(kBlock) k_cpl_update(CplUpd a) {
    const int64_t nu = a.H / (int32_t)(sizeof(T) / sizeof(double));
    const int64_t u = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (u >= nu) return;
    const T r0 = reinterpret_cast<const T*>(a.r)[u], r1 = reinterpret_cast<const T*>(a.r)[u + nu];
    cpl_update_row<T>(a, u, r0, r1);
    cpl_update_row<T>(a, u + nu, r1, r0);
}

int launch_cpl_update(int32_t nrows, const double* cpl_p, const double* cpl_q, const double* r, const double* xin,
                      double c1, double c2, double* d, const double* sub, double* out, int store_d, bool dzero,
                      hipStream_t st) {
    if (nrows < 0 || (nrows & 3)) return set_error(MPBP_ERR_ARG, "cpl_update: nrows = %d is not a multiple of 4", nrows);
    if (nrows && (!cpl_p || !cpl_q || !r || !out || (!d && (store_d || (xin && !dzero)))))
        return set_error(MPBP_ERR_ARG, "cpl_update: needs the tables, r, out and d where it is read or stored");
    if (r == out || r == d) return set_error(MPBP_ERR_ARG, "cpl_update: r must not alias out or d (partner rows read it)");
    if (!nrows) return MPBP_OK;
    const CplUpd a{cpl_p, cpl_q, r, xin, sub, d, out, c1, c2, nrows / 2, dzero ? 1 : 0, store_d ? 1 : 0};
    const uintptr_t bits = (uintptr_t)cpl_p | (uintptr_t)cpl_q | (uintptr_t)r | (uintptr_t)xin | (uintptr_t)sub |
                           (uintptr_t)d | (uintptr_t)out;
    if ((bits & 15) == 0) k_cpl_update<f64x2><<<grid_for(nrows / 4), kBlock, 0, st>>>(a);
    else k_cpl_update<double><<<grid_for(nrows / 2), kBlock, 0, st>>>(a);
    MPBP_HIP(hipGetLastError());
    return MPBP_OK;
}

// The sweep as ONE launch on a matrix-free F level 0 (mpbp_mg.cpl_fuse): k_march / k_direct compute the four rows of a
// cell in one lane (fields 0..3 = u_n, v_n, u_s, v_s), so the partners (0, 2) and (1, 3) are lane-local.  This
// cell-wise epilogue (kCell, CellEpi) receives the four row sums -- row<EDGE>'s under the exact policy, so the bits are
// the two-launch form's; rows4's under the tolerance policy, whose reciprocal diagonals go unused -- forms
// r = b - sum as EpiResid does and performs k_cpl_update's operations.  MODE 0: a sweep that stores d; 1: a solve's last
// sweep (d not stored); 2: the last sweep writing sub - x.  DZ: d is read as +0.0 (a restart's first sweep).
template <int MODE, bool DZ>
struct EpiCplChebT {
    static constexpr bool kCell = true;
    const double *b, *cpl_p, *cpl_q;
    double* d;
    double c1, c2;
    const double* sub;
    double* xout;
    // b and d are requested ahead of the rows; the tables and sub once the four sums are known (as EpiChebT's kSubLate):
    // all four sums stay live until the cell is finished, and with the tables held through the rows as well the
    // marching instances spilled (16-124 B per lane at k_march's 4 waves per SIMD)
    struct P { double b, d; };
    __device__ P pre_lite(int32_t r) const { return {ld_stream(b + r), DZ ? 0.0 : ld_stream(d + r)}; }
    __device__ void cell(const int32_t* rw, const double* acc, const double* xv, const P* pe) const {
        double r[4], p[4], q[4], s[4];
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            p[o] = ld_stream(cpl_p + rw[o]);
            q[o] = ld_stream(cpl_q + rw[o]);
            s[o] = MODE == 2 ? ld_stream(sub + rw[o]) : 0.0;
            r[o] = pe[o].b - acc[o];
        }
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            const double z = p[o] * r[o] + q[o] * r[o ^ 2];
            const double dn = c1 * pe[o].d + c2 * z;
            if (MODE == 0) d[rw[o]] = dn;
            const double x = xv[o] + dn;
            xout[rw[o]] = MODE == 2 ? s[o] - x : x;
        }
    }
};
template <int M, bool Z> struct RcpOk<EpiCplChebT<M, Z>> : std::true_type {};

// Whether level 0's operator is the whole-grid matrix-free F on one GPU (the fused sweep's operator).
bool cpl_fuse_ok(const OpPair& op) {
    const OpRef& o = op.in;
    return o.stencil && o.sop == SOP_F && !o.empty && op.bd.empty && !o.stencil->halo && o.which == 0 &&
           o.stencil->f_stencil;
}
int launch_cpl_fused(const OpRef& o, const double* cpl_p, const double* cpl_q, const double* x, const double* b, double c1,
                     double c2, double* d, const double* sub, double* out, int store_d, bool dzero, hipStream_t st) {
    const mpbp_schur_plan* p = o.stencil;
    if (!x || !b || !d || !out || x == out || (sub && store_d))
        return set_error(MPBP_ERR_ARG, "cpl fused sweep: bad vectors (sub comes with a solve's last sweep)");
    FStencilDev P;
    const int rc = make_fstencil(&p->f_prm, p->f_cell, p->f_uface, p->f_vface, nullptr, &P);
    if (rc) return rc;
    const bool fast = p->f_numerics == MPBP_NUMERICS_FAST;
    auto go = [&](auto e) {
        e.b = b; e.cpl_p = cpl_p; e.cpl_q = cpl_q; e.d = d; e.c1 = c1; e.c2 = c2; e.sub = sub; e.xout = out;
        return launch_fstencil(P, x, e, st, fast);
    };
    const int mode = store_d ? 0 : (sub ? 2 : 1);
    if (dzero) return mode == 0 ? go(EpiCplChebT<0, true>{}) : mode == 1 ? go(EpiCplChebT<1, true>{}) : go(EpiCplChebT<2, true>{});
    return mode == 0 ? go(EpiCplChebT<0, false>{}) : mode == 1 ? go(EpiCplChebT<1, false>{}) : go(EpiCplChebT<2, false>{});
}

// mg_smooth for a coupled level: K sweeps on [lmin, lmax] of B^-1 A, each a residual launch (the level's operator, any
// form: the same bits) into `r` and k_cpl_update -- or, with `fuse` on a matrix-free F level 0, one launch_cpl_fused
// (the zero start stays k_cpl_update's init form).  zero / cur / alt / dst / sub / spare as mg_smooth; none of the
// point-Jacobi fusions applies.
template <class Xch>
int mg_smooth_cpl(const OpPair& op, int32_t nrows, const double* cpl_p, const double* cpl_q, double lmin, double lmax,
                  int K, bool zero, const double* b, double** cur, double* alt, double* r, double* d, double* dst,
                  const double* sub, hipStream_t st, Xch&& xch, double* spare = nullptr, bool fuse = false) {
    double c1[64] = {}, c2[64] = {};
    if (K < 1 || K > 64) return set_error(MPBP_ERR_ARG, "mg: smoothing sweeps must be in [1, 64]");
    if (!cpl_p || !cpl_q) return set_error(MPBP_ERR_ARG, "mg: a coupled level needs cpl_p and cpl_q");
    cheb_coeffs(lmin, lmax, K, c1, c2);
    double* x = *cur;
    double* other = alt;
    double* const keep = spare ? *cur : nullptr;   // mg_smooth's: a restart's iterate outside the two buffers is kept
    auto recycle = [&](double* v) { return v == keep ? spare : v; };
    int s = 0;
    if (zero) {
        double* out0 = K == 1 ? (dst ? dst : other) : x;
        const int rc = launch_cpl_update(nrows, cpl_p, cpl_q, b, nullptr, 0.0, c2[0], d, K == 1 ? sub : nullptr, out0,
                                         K == 1 ? 0 : 1, false, st);
        if (rc) return rc;
        if (K == 1) {
            *cur = out0;
            return MPBP_OK;
        }
        s = 1;
    }
    bool dzero = !zero;   // a restart: d = 0, read as +0.0 by its first sweep
    for (; s < K; ++s) {
        const bool last = s == K - 1;
        double* nxt = (last && dst) ? dst : other;
        xch(x);
        int rc = MPBP_OK;
        if (fuse && cpl_fuse_ok(op)) {
            rc = launch_cpl_fused(op.in, cpl_p, cpl_q, x, b, c1[s], c2[s], d, last ? sub : nullptr, nxt, last ? 0 : 1,
                                  dzero, st);
            if (rc) return rc;
            dzero = false;
            other = recycle(x);
            x = nxt;
            continue;
        }
        rc = op_spmv(op.in, MPBP_SPMV_RESID, x, b, r, st);
        if (!rc) rc = op_spmv(op.bd, MPBP_SPMV_RESID, x, b, r, st);
        if (!rc)
            rc = launch_cpl_update(nrows, cpl_p, cpl_q, r, x, c1[s], c2[s], d, last ? sub : nullptr, nxt, last ? 0 : 1,
                                   dzero, st);
        if (rc) return rc;
        dzero = false;
        other = recycle(x);
        x = nxt;
    }
    *cur = x;
    return MPBP_OK;
}

// mpbp_mg_solve's and the Schur apply's refusals of a coupled hierarchy, before anything is launched.
int mg_check_smoother(const mpbp_mg* m) {
    if (m->smoother == MPBP_MG_SMOOTH_POINT) return MPBP_OK;
    if (m->smoother != MPBP_MG_SMOOTH_COUPLED) return set_error(MPBP_ERR_ARG, "mg: unknown smoother %d", m->smoother);
    if (m->part_levels > 0)
        return set_error(MPBP_ERR_ARG, "mg: the coupled smoother is one GPU only (part_levels = %d)", m->part_levels);
    for (int l = 0; l + 1 < m->nlevels; ++l) {
        const mpbp_mg_level& L = m->levels[l];
        if (L.nrows & 3)
            return set_error(MPBP_ERR_ARG, "mg: the coupled smoother pairs rows i and i + nrows / 2 of four stacked "
                                           "fields: level %d has %d rows, not a multiple of 4", l, L.nrows);
        if (!L.cpl_p || !L.cpl_q)
            return set_error(MPBP_ERR_ARG, "mg: the coupled smoother needs level %d's cpl_p and cpl_q tables", l);
    }
    return MPBP_OK;
}

}  // namespace

extern "C" {

int mpbp_cpl_blocks(const mpbp_csr* A, double* cpl_p, double* cpl_q, void* stream) {
    int rc = check_csr(A);
    if (rc) return rc;
    if (A->nrows != A->ncols || (A->nrows & 3) || (A->nrows && (!cpl_p || !cpl_q)))
        return set_error(MPBP_ERR_ARG, "cpl_blocks: needs a square operator of 4 m rows and both tables");
    if (!A->nrows) return MPBP_OK;
    unsigned h[2] = {0, 0};
    rc = device_flags("cpl_blocks", h, 2, as_stream(stream), [&](unsigned* d_flags) {
        k_cpl_blocks<<<grid_for(A->nrows), kBlock, 0, as_stream(stream)>>>(to_csr(A), A->nrows, cpl_p, cpl_q, d_flags);
    });
    if (rc) return rc;
    if (h[0])
        return set_error(MPBP_ERR_PATTERN, "cpl_blocks: %u rows have no stored diagonal or a 2 x 2 phase block whose "
                                           "determinant is not finite and positive (first: row %d)", h[0],
                         INT32_MAX - (int32_t)h[1]);
    return MPBP_OK;
}

int mpbp_cpl_bound(const mpbp_csr* A, const double* cpl_p, const double* cpl_q, double* lmax, void* stream) {
    int rc = check_csr(A);
    if (rc) return rc;
    if (A->nrows != A->ncols || (A->nrows & 3) || !A->nrows || !cpl_p || !cpl_q || !lmax)
        return set_error(MPBP_ERR_ARG, "cpl_bound: needs a square operator of 4 m > 0 rows, both tables and lmax");
    unsigned long long h[2] = {0, 0};
    rc = device_flags("cpl_bound", h, 2, as_stream(stream), [&](unsigned long long* d_out) {
        k_cpl_bound<<<grid_for(A->nrows), kBlock, 0, as_stream(stream)>>>(to_csr(A), A->nrows, cpl_p, cpl_q, d_out);
    });
    if (rc) return rc;
    if (h[1])
        return set_error(MPBP_ERR_PATTERN, "cpl_bound: %llu rows (or their partners) do not hold their columns in "
                                           "ascending order", h[1]);
    double v;
    memcpy(&v, &h[0], sizeof(v));
    *lmax = v;
    return MPBP_OK;
}

int mpbp_cpl_update(int32_t nrows, const double* cpl_p, const double* cpl_q, const double* r, const double* x_in,
                    double c1, double c2, double* d, int32_t dzero, const double* sub, double* x_out, int32_t store_d,
                    void* stream) {
    return launch_cpl_update(nrows, cpl_p, cpl_q, r, x_in, c1, c2, d, sub, x_out, store_d, dzero != 0, as_stream(stream));
}

}  // extern "C"
