// The matrix-free pressure-side operators D, G and Gt_G (PGDev, DStencilDev, GStencilDev, GtGStencilDev) and the
// five-row A policy of the matrix-free Stokes operator (StokesADev, launch_stokes_a).
// Needs mpbp.hip's prelude (KO, MPBP_HIP) and kernel sections: the epilogues, the F stencil (FStencilDev, Wrap, add5,
// ext_row), the marching kernels with their launch geometry, and FStencilDevM and with_f_policy (f_solve_w.inc).
// A fragment of mpbp.hip, included there once and in order: not a self-contained header.

namespace {

// ------------------------------------------------------- matrix-free D, G, Gt_G ----
// The pressure-side operators rebuilt per row from the cell thn table: D (pressure rows, reading the 4
// velocity fields), G (velocity rows, reading pressure) and Gt_G = -(D G) (pressure rows), with the
// arithmetic of phase_D_row / phase_G_row (x d_p) / k_spgemm_fill (products accumulated in D's column
// order, then scaled by alpha = -1) and summed in CSR column order -- the assembled operators' results
// bit for bit.  Needs n >= 3 (distinct periodic neighbours).
struct PGDev {
    static constexpr bool kFast = false;
    int n;
    const double* cell;
    double d_p, inv, minv;   // d_p, 1.0 / dx, -1.0 / dx  (dx == dy; evaluated as the assembly does)
    // partition of the INPUT vector's grid rows, as FStencilDev (one GPU: r0 = 0, L = n, h = 0)
    int r0, L, h, which;
    int ext = 0;   // which = 3: ghost rows computed on each side
    int oh = 0;    // ghost depth of the output's layout (D: pressure, G: velocity, Gt_G: == h)
    int unit = 0;  // d_p == 1 and minv == -inv: Gt_G's eight products per phase are +-X^2 (GtGStencilDev::entries)
    __device__ int wrap(int a) const { return a < 0 ? a + n : (a >= n ? a - n : a); }
    template <int NFI>
    __device__ int32_t xrow_of(int f, int gr) const {
        if (h == 0) return (f * n + wrap(gr)) * n;
        return ext_row(NFI, f, gr - r0, L, h, n);
    }
    template <int NFO>
    __device__ int32_t out_of(int f, int lr, int gc) const {
        return (lr >= 0 && lr < L ? (f * L + lr) * n : ext_row(NFO, f, lr, L, oh, n)) + gc;
    }
};

// y = D x: pressure row (gr, gc) = sum over phases of the 4 velocity entries in column order.
struct DStencilDev : PGDev {
    struct Cell {};
    __device__ Cell cell_pre(int, int) const { return {}; }
    static constexpr int NF = 4, NOUT = 1;
    __device__ int32_t xrow(int f, int gr) const { return xrow_of<4>(f, gr); }
    __device__ int32_t out_row(int, int lr, int gc) const { return out_of<1>(0, lr, gc); }
    template <bool EDGE, class TA, class XA>
    __device__ double row(int, int gr, int gc, const TA& ta, const XA& xa, double* dg, const Cell&) const {
        const bool lastc = EDGE && gc == n - 1, lastr = EDGE && gr == n - 1;   // wrapped neighbour sorts first
        double acc = 0.0;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const double t0 = ta.T(p, gr, gc), tE = ta.T(p, gr, gc + 1), tW = ta.T(p, gr, gc - 1);
            const double tN = ta.T(p, gr - 1, gc), tS = ta.T(p, gr + 1, gc);
            const double uE = (inv * (0.5 * (t0 + tE))) * xa.X(2 * p, gr, gc + 1);
            const double uC = (minv * (0.5 * (t0 + tW))) * xa.X(2 * p, gr, gc);
            const double vC = (inv * (0.5 * (t0 + tN))) * xa.X(2 * p + 1, gr, gc);
            const double vS = (minv * (0.5 * (t0 + tS))) * xa.X(2 * p + 1, gr + 1, gc);
            acc += lastc ? uE : uC;
            acc += lastc ? uC : uE;
            acc += lastr ? vS : vC;
            acc += lastr ? vC : vS;
        }
        *dg = 0.0;
        return acc;
    }
};

// y = G x: velocity row o (u_n, v_n, u_s, v_s) at (gr, gc), two pressure entries in column order.
struct GStencilDev : PGDev {
    struct Cell {};
    __device__ Cell cell_pre(int, int) const { return {}; }
    static constexpr int NF = 1, NOUT = 4;
    __device__ int32_t xrow(int f, int gr) const { return xrow_of<1>(f, gr); }
    __device__ int32_t out_row(int f, int lr, int gc) const { return out_of<4>(f, lr, gc); }
    template <bool EDGE, class TA, class XA>
    __device__ double row(int o, int gr, int gc, const TA& ta, const XA& xa, double* dg, const Cell&) const {
        const int p = o >> 1;
        const double t0 = ta.T(p, gr, gc), xC = xa.X(0, gr, gc);
        double acc = 0.0;
        *dg = 0.0;
        if ((o & 1) == 0) {   // u row: entries p(gr, gc-1), p(gr, gc); the wrapped one sorts last
            const double gu = 0.5 * (t0 + ta.T(p, gr, gc - 1));
            const double uC = (d_p * (inv * gu)) * xC, uW = (d_p * (minv * gu)) * xa.X(0, gr, gc - 1);
            const bool wrapw = EDGE && gc == 0;
            acc += wrapw ? uC : uW;
            acc += wrapw ? uW : uC;
        } else {              // v row: entries p(gr-1, gc), p(gr, gc)
            const double gv = 0.5 * (t0 + ta.T(p, gr - 1, gc));
            const double vC = (d_p * (minv * gv)) * xC, vN = (d_p * (inv * gv)) * xa.X(0, gr - 1, gc);
            const bool wrapn = EDGE && gr == 0;
            acc += wrapn ? vC : vN;
            acc += wrapn ? vN : vC;
        }
        return acc;
    }
};

// y = A x, A = [[F, d_p G], [d_div D, 0]] (build_row's MPBP_OP_A; np.matmul(A, u_vec), apply.py:72): the five rows
// of a cell -- u_n, v_n, u_s, v_s and pressure -- from the five staged fields [u_n | v_n | u_s | v_s | p], one
// marching launch, nothing assembled.  FS is the F policy (FStencilDev, FStencilDevM<M>, FStencilFast) whose rows
// the velocity rows start from.  Exact numerics reproduce the assembled row's sequential sum: a velocity row is F's
// row sum with the two G products added to the SAME accumulator ((F-sum + g1) + g2: G's columns 4N + ... sort after
// all of F's), in GStencilDev::row's order; the pressure row is DStencilDev::row's eight products in its order,
// each entry d_div * (inv * avg) as the assembly forms it (phase_D_row's value scaled by d_div).  With FStencilFast
// the velocity rows start from the regrouped rows (rows4); the G products and the pressure row are the exact ones
// (explicit operations, the file is built without contraction), so pressure rows agree bit for bit in both modes.
// n >= 3.  PART = false: one GPU, whole-grid layouts.  PART = true: the rank's rows of a row partition (FS's r0, L, h,
// which = 0 / 1 / 2): x in the 5-field owned + ghost layout (ext_row), y and z the owned rows alone (A's product has
// no ghost rows); the thn tables, cell_pre, the column wrap and the EDGE test stay in global grid coordinates, so a
// row's operations and their order are the one-GPU instance's.
template <class FS, bool PART = false>
struct StokesADev : FS {
    double d_p, d_div, inv, minv;   // inv = 1.0 / dx, minv = -1.0 / dx as phase_D_row / phase_G_row evaluate them
    static constexpr int NF = 5, NOUT = 5;
    __device__ int32_t xrow(int f, int gr) const {
        if constexpr (PART) return ext_row(5, f, gr - this->r0, this->L, this->h, this->n);
        else return (f * this->n + this->wrap(gr)) * this->n;
    }
    __device__ int32_t out_row(int o, int lr, int gc) const {
        if constexpr (PART) return (o * this->L + lr) * this->n + gc;
        else return (o * this->n + lr) * this->n + gc;
    }
    // velocity row o's two G products added to acc: the wrapped neighbour sorts last
    template <bool EDGE, class TA, class XA>
    __device__ double add_g(double acc, int o, int gr, int gc, const TA& ta, const XA& xa) const {
        const int p = o >> 1;
        const double t0 = ta.T(p, gr, gc), xC = xa.X(4, gr, gc);
        if ((o & 1) == 0) {   // u row: entries p(gr, gc-1), p(gr, gc)
            const double gu = 0.5 * (t0 + ta.T(p, gr, gc - 1));
            const double uC = (d_p * (inv * gu)) * xC, uW = (d_p * (minv * gu)) * xa.X(4, gr, gc - 1);
            const bool wrapw = EDGE && gc == 0;
            acc += wrapw ? uC : uW;
            acc += wrapw ? uW : uC;
        } else {              // v row: entries p(gr-1, gc), p(gr, gc)
            const double gv = 0.5 * (t0 + ta.T(p, gr - 1, gc));
            const double vC = (d_p * (minv * gv)) * xC, vN = (d_p * (inv * gv)) * xa.X(4, gr - 1, gc);
            const bool wrapn = EDGE && gr == 0;
            acc += wrapn ? vC : vN;
            acc += wrapn ? vN : vC;
        }
        return acc;
    }
    // pressure row: phase n then phase s, the wrapped neighbour first
    template <bool EDGE, class TA, class XA>
    __device__ double p_row(int gr, int gc, const TA& ta, const XA& xa) const {
        const int n = this->n;
        const bool lastc = EDGE && gc == n - 1, lastr = EDGE && gr == n - 1;
        double acc = 0.0;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const double t0 = ta.T(p, gr, gc), tE = ta.T(p, gr, gc + 1), tW = ta.T(p, gr, gc - 1);
            const double tN = ta.T(p, gr - 1, gc), tS = ta.T(p, gr + 1, gc);
            const double uE = (d_div * (inv * (0.5 * (t0 + tE)))) * xa.X(2 * p, gr, gc + 1);
            const double uC = (d_div * (minv * (0.5 * (t0 + tW)))) * xa.X(2 * p, gr, gc);
            const double vC = (d_div * (inv * (0.5 * (t0 + tN)))) * xa.X(2 * p + 1, gr, gc);
            const double vS = (d_div * (minv * (0.5 * (t0 + tS)))) * xa.X(2 * p + 1, gr + 1, gc);
            acc += lastc ? uE : uC;
            acc += lastc ? uC : uE;
            acc += lastr ? vS : vC;
            acc += lastr ? vC : vS;
        }
        return acc;
    }
    template <bool EDGE, class TA, class XA>
    __device__ double row(int o, int gr, int gc, const TA& ta, const XA& xa, double* dg,
                          const typename FS::Cell& cl) const {
        if (o == 4) {
            *dg = 0.0;
            return p_row<EDGE>(gr, gc, ta, xa);
        }
        return add_g<EDGE>(FS::template row<EDGE>(o, gr, gc, ta, xa, dg, cl), o, gr, gc, ta, xa);
    }
    // tolerance mode (FS = FStencilFast): the five rows at once; no diagonal is handed over (rd unused by the
    // store / add / residual epilogues)
    template <class TA, class XA>
    __device__ void rows4(int gr, int gc, const TA& ta, const XA& xa, const typename FS::Cell& cl, double* acc,
                          double* rd) const {
        FS::template rows4<false>(gr, gc, ta, xa, cl, acc, rd);
#pragma unroll
        for (int o = 0; o < 4; ++o) acc[o] = add_g<true>(acc[o], o, gr, gc, ta, xa);
        acc[4] = p_row<true>(gr, gc, ta, xa);
#pragma unroll
        for (int o = 0; o < 5; ++o) rd[o] = 0.0;
    }
};

template <bool PART, class Epi>
int launch_stokes_a(const FStencilDev& P, double d_p, double d_div, const double* x, Epi epi, hipStream_t st,
                    bool fast) {
    const double dx = 1.0 / P.n;
    auto go = [&](const auto& Q) {
        using S = StokesADev<std::decay_t<decltype(Q)>, PART>;
        const S A{Q, d_p, d_div, 1.0 / dx, -1.0 / dx};
        const int64_t chunks = march_chunks(A, KO().march_rows, march_capacity<k_march<S, XPlain, Epi, BNone>>());
        if (chunks == 0) return (int)MPBP_OK;
        const int64_t strips = (A.n + kMB - 1) / kMB;
        k_march<S, XPlain, Epi, BNone><<<(unsigned)(chunks * strips), kMB, 0, st>>>(A, XPlain{x}, (int)chunks, epi, BNone{});
        MPBP_HIP(hipGetLastError());
        return (int)MPBP_OK;
    };
    if constexpr (std::is_same_v<Epi, EpiStore>) return with_f_policy(P, fast, go);
    // ADD / RESID: the M = 13 and M = 5 identity instances spilled (8 / 24 B per lane) beside the z operand; these
    // modes take the general exact rows there (the same bits: the identities only skip exactly known multiplies)
    if (fast) return go(FStencilFast{P});
    if (P.d_u == -1.0 && P.eta_s == 1.0 && P.eta_n == 1.0) return go(FStencilDevM<7>{P});
    return go(P);
}

// Gt_G = -(D G): row (gr, gc) has the five entries N, W, C, E, S (grid neighbours).  Each off-diagonal
// gets one product per phase; the diagonal gets four per phase, accumulated in D's column order.
struct GtGStencilDev : PGDev {
    struct Cell {};
    __device__ Cell cell_pre(int, int) const { return {}; }
    static constexpr int NF = 1, NOUT = 1;
    __device__ int32_t xrow(int f, int gr) const { return xrow_of<1>(f, gr); }
    __device__ int32_t out_row(int, int lr, int gc) const { return out_of<1>(0, lr, gc); }
    // e = {N, W, C, E, S}.  (vr, vc): the cell in the accessor's coordinates (it may lie up to a few cells
    // outside the grid in the fused solve); (gr, gc): the same cell wrapped onto the grid.
    template <class TA>
    __device__ void entries(int vr, int vc, int gr, int gc, const TA& ta, double* e) const {
        const bool lastc = gc == n - 1, lastr = gr == n - 1;
        double cN = 0.0, cW = 0.0, cC = 0.0, cE = 0.0, cS = 0.0;
        if (unit) {
            // d_p == 1 and minv == -inv: with X = inv * (0.5 * (t0 + t_nb)) per face, every D entry is +-X and
            // every G factor d_p * (+-inv * g) is +-X too (g is the same half sum), so the eight products below
            // are +-X^2 -- the same roundings (RN(-a b) = -RN(a b)), same bits, 12 multiplies per phase, not 28
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                const double t0 = ta.T(p, vr, vc), tE = ta.T(p, vr, vc + 1), tW = ta.T(p, vr, vc - 1);
                const double tN = ta.T(p, vr - 1, vc), tS = ta.T(p, vr + 1, vc);
                const double XW = inv * (0.5 * (t0 + tW)), XE = inv * (0.5 * (t0 + tE));
                const double XN = inv * (0.5 * (t0 + tN)), XS = inv * (0.5 * (t0 + tS));
                const double qW = XW * XW, qE = XE * XE, qN = XN * XN, qS = XS * XS;
                // uC_C = -qW, uC_W = qW, uE_E = qE, uE_C = -qE, vC_C = -qN, vC_N = qN, vS_S = qS, vS_C = -qS
                const double u1 = lastc ? -qE : -qW, u2 = lastc ? -qW : -qE;
                const double v1 = lastr ? -qS : -qN, v2 = lastr ? -qN : -qS;
                if (p == 0) {
                    cC = u1; cW = qW; cE = qE; cN = qN; cS = qS;
                } else {
                    cC += u1; cW += qW; cE += qE; cN += qN; cS += qS;
                }
                cC += u2;
                cC += v1;
                cC += v2;
            }
            e[0] = -1.0 * cN; e[1] = -1.0 * cW; e[2] = -1.0 * cC; e[3] = -1.0 * cE; e[4] = -1.0 * cS;
            return;
        }
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const double t0 = ta.T(p, vr, vc), tE = ta.T(p, vr, vc + 1), tW = ta.T(p, vr, vc - 1);
            const double tN = ta.T(p, vr - 1, vc), tS = ta.T(p, vr + 1, vc);
            // D row entries (phase_D_row)
            const double DuE = inv * (0.5 * (t0 + tE)), DuC = minv * (0.5 * (t0 + tW));
            const double DvC = inv * (0.5 * (t0 + tN)), DvS = minv * (0.5 * (t0 + tS));
            // G rows of the velocity unknowns u(gr,gc), u(gr,gc+1), v(gr,gc), v(gr+1,gc) (phase_G_row x d_p)
            const double gC = 0.5 * (t0 + tW), gE = 0.5 * (tE + t0);
            const double gN = 0.5 * (t0 + tN), gS = 0.5 * (tS + t0);
            const double uC_C = DuC * (d_p * (inv * gC)), uC_W = DuC * (d_p * (minv * gC));
            const double uE_E = DuE * (d_p * (inv * gE)), uE_C = DuE * (d_p * (minv * gE));
            const double vC_C = DvC * (d_p * (minv * gN)), vC_N = DvC * (d_p * (inv * gN));
            const double vS_S = DvS * (d_p * (minv * gS)), vS_C = DvS * (d_p * (inv * gS));
            const double u1 = lastc ? uE_C : uC_C, u2 = lastc ? uC_C : uE_C;
            const double v1 = lastr ? vS_C : vC_C, v2 = lastr ? vC_C : vS_C;
            if (p == 0) {   // first touch stores the product itself (k_spgemm_fill)
                cC = u1; cW = uC_W; cE = uE_E; cN = vC_N; cS = vS_S;
            } else {
                cC += u1; cW += uC_W; cE += uE_E; cN += vC_N; cS += vS_S;
            }
            cC += u2;
            cC += v1;
            cC += v2;
        }
        e[0] = -1.0 * cN; e[1] = -1.0 * cW; e[2] = -1.0 * cC; e[3] = -1.0 * cE; e[4] = -1.0 * cS;
    }
    // Gt_G x at a cell: the five entries summed in CSR column order (EDGE: sorted by wrapped column)
    template <bool EDGE, class TA, class XA>
    __device__ double apply_v(int vr, int vc, int gr, int gc, const TA& ta, const XA& xa, double* dg) const {
        double e[5];
        entries(vr, vc, gr, gc, ta, e);
        *dg = e[2];
        const double p[5] = {e[0] * xa.X(0, vr - 1, vc), e[1] * xa.X(0, vr, vc - 1), e[2] * xa.X(0, vr, vc),
                             e[3] * xa.X(0, vr, vc + 1), e[4] * xa.X(0, vr + 1, vc)};
        return add5<EDGE>(0.0, p, Wrap{gr == 0, gr == n - 1, gc == 0, gc == n - 1});
    }
    template <bool EDGE, class TA, class XA>
    __device__ double row(int, int gr, int gc, const TA& ta, const XA& xa, double* dg, const Cell&) const {
        return apply_v<EDGE>(gr, gc, gr, gc, ta, xa, dg);
    }
};

}  // namespace
