// Fused multigrid levels: the g1_* row helpers, level 1 of a tolerance-mode F hierarchy in one launch (k_gal1),
// its level 0 (pre-smoothing, residual and restriction in one launch) and the pressure hierarchy's level 1 (k_gal1p).
// Needs mpbp.hip's multigrid transfers (MgFields, mg_p1d_fast, mg_r1d_fast), epilogues, F stencil and XPlain,
// f_tile.inc's tile geometry, GtGStencilDev (pg_stencil.inc) and g1_rw's declaration (gtg_solve.inc).
// A fragment of mpbp.hip, included there once and in order: not a self-contained header.

namespace {

// ---- multigrid level 1 of a tolerance-mode F hierarchy in one launch (k_gal1) ----
// A_1 x = R_0 (F (P_0 x)) (MgGal) with the two fine-size intermediates kept in LDS: a workgroup owns a 16 x 8 tile of
// coarse cells (a 32 x 16 fine block; kGF* below), stages the coarse x of its four fields over the tile + 2 and thn
// over the fine block + 2, builds t0 = P_0 x on the fine block + 2 (36 x 20), t1 = F t0 on the fine block + 1 (34 x 18,
// the tolerance-mode rows), and R_0 t1 on its coarse rows, handing each to the level's epilogue.  Each value is built
// by the operations of the three launches it replaces (k_mg_transfer_spmv's 1D lists and product order,
// FStencilFast::rows4), so the result is bit-identical; HBM: x, thn and the epilogue operands once, no fine vector
// written or read.  (The 32 x 4 tile of kG1* above -- the level-0 fused kernels' coarse windows -- took 42 KB of LDS,
// three workgroups per CU: 33.1 vs 28.5 us per launch, profiles/r06s_ab_gal1_tile.txt.)
// a grid index to its slot in a staged window starting at virtual index `base` (the window is < the grid)
__device__ inline int g1_slot(int i, int base, int m) { int l = i - base; return l < 0 ? l + m : (l >= m ? l - m : l); }
// P_0's row at fine (gr, gc) of a field with compile-time kinds: k_mg_transfer_spmv's list order and products
// (S: the coarse window's row stride)
template <int KY, int KX, int S>
__device__ inline double g1_p(const double* xf, int gr, int gc, int nc, int rb, int cb) {
    int yi[2], xi[2];
    double yw[2], xw[2];
    const int my = mg_p1d_fast(KY, nc, gr, yi, yw), mx = mg_p1d_fast(KX, nc, gc, xi, xw);
    double acc = 0.0;
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        if (a >= my) break;
        const double* xr = xf + g1_slot(yi[a], rb, nc) * S;
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            if (b >= mx) break;
            acc += (yw[a] * xw[b]) * xr[g1_slot(xi[b], cb, nc)];
        }
    }
    return acc;
}
// R_0's row at coarse (cr, cc): 4 (cell) x 3 or 4 entries, compile-time counts (S: the fine window's row stride)
template <int KY, int KX, int S = kG1FW>
__device__ inline double g1_r(const double* tf, int cr, int cc, int n, int rb, int cb) {
    constexpr int MY = KY == MPBP_MG_CELL ? 4 : 3, MX = KX == MPBP_MG_CELL ? 4 : 3;
    int yi[4], xi[4];
    double yw[4], xw[4];
    mg_r1d_fast(KY, n, cr, yi, yw);
    mg_r1d_fast(KX, n, cc, xi, xw);
    double acc = 0.0;
#pragma unroll
    for (int a = 0; a < MY; ++a) {
        const double* tr1 = tf + g1_slot(yi[a], rb, n) * S;
#pragma unroll
        for (int b = 0; b < MX; ++b) acc += (yw[a] * xw[b]) * tr1[g1_slot(xi[b], cb, n)];
    }
    return acc;
}
// Interior tiles (no staged window wraps and no 1D list takes its periodic special case): P_0's and R_0's rows in
// window coordinates straight from the fine / coarse parity -- the same entries, weights, order and products as
// mg_p1d_fast / mg_r1d_fast give there, without their wrap tests, sorted-order selects and runtime weights.  A node
// kind's one-entry row (even fine index) takes a second entry of weight 0: its products are +-0 added to a sum that
// started from +0.0 (never -0.0), so the sum's bits are unchanged for finite x.  With t1 in t0's LDS (occupancy 2 -> 3
// workgroups per CU): k_gal1 45 -> 33 us, multigrid apply 1.610 -> 1.510 ms (A/B on one box, profiles/r05zd_ab.txt).
template <int K>
__device__ inline void g1_p1d_in(int r, int& lo, double& w0, double& w1) {
    const bool odd = r & 1;
    if constexpr (K == MPBP_MG_CELL) {   // even: c_{i-1} (1/4), c_i (3/4); odd: c_i (3/4), c_{i+1} (1/4)
        lo = (r >> 1) + (odd ? 1 : 0);
        w0 = odd ? 0.75 : 0.25;
        w1 = odd ? 0.25 : 0.75;
    } else {                             // even: c_i (1); odd: c_i, c_{i+1} (1/2 each)
        lo = (r >> 1) + 1;
        w0 = odd ? 0.5 : 1.0;
        w1 = odd ? 0.5 : 0.0;
    }
}
// P_0's row at window fine (r, c) of the block + 2 (the coarse window starts two coarse cells before the tile)
template <int KY, int KX, int S>
__device__ inline double g1_p_in(const double* xf, int r, int c) {
    int ry, cx;
    double y0, y1, x0, x1;
    g1_p1d_in<KY>(r, ry, y0, y1);
    g1_p1d_in<KX>(c, cx, x0, x1);
    const double* q = xf + ry * S + cx;
    double acc = 0.0;
    acc += (y0 * x0) * q[0];
    acc += (y0 * x1) * q[1];
    acc += (y1 * x0) * q[S];
    acc += (y1 * x1) * q[S + 1];
    return acc;
}
// R_0's row at tile coarse (lr, lc) over a fine window of row stride W whose slot OFF holds fine index 2 c0 - 1 (the
// tile's first coarse cell's first restriction entry): 2 lr + OFF + 0 .. 3 (cell) / 0 .. 2 (node)
template <int KY, int KX, int W, int OFF>
__device__ inline double g1_rw_in(const double* tf, int lr, int lc) {
    constexpr int MY = KY == MPBP_MG_CELL ? 4 : 3, MX = KX == MPBP_MG_CELL ? 4 : 3;
    constexpr double WC[4] = {0.25, 0.75, 0.75, 0.25}, WN[3] = {0.5, 1.0, 0.5};
    const double* q = tf + (2 * lr + OFF) * W + 2 * lc + OFF;
    double acc = 0.0;
#pragma unroll
    for (int a = 0; a < MY; ++a)
#pragma unroll
        for (int b = 0; b < MX; ++b)
            acc += ((KY == MPBP_MG_CELL ? WC[a] : WN[a]) * (KX == MPBP_MG_CELL ? WC[b] : WN[b])) * q[a * W + b];
    return acc;
}
// ... over t1's window (fine block + 1)
template <int KY, int KX, int S = kG1FW>
__device__ inline double g1_r_in(const double* tf, int lr, int lc) { return g1_rw_in<KY, KX, S, 0>(tf, lr, lc); }
// a tile whose transfers' windows neither wrap nor reach a 1D list's periodic special case (coarse tile of TH x TW
// cells at (cr0, cc0), windows two coarse cells beyond it)
__device__ inline bool g1_inner(int cr0, int cc0, int th, int tw, int nc) {
    return cr0 >= 2 && cr0 + th + 2 <= nc && cc0 >= 2 && cc0 + tw + 2 <= nc;
}
// Level 1 under a row partition (PART): this rank owns coarse rows [r0, r0 + L) of every field and its level-1 vectors
// hold them followed by h ghost rows above and below (ext_row's layout).  The tiles cover the owned rows only; every
// value is computed in global coordinates exactly as on one GPU (the same windows, lists and rows), so the rank's rows
// are the one-GPU launch's bits.
struct G1Part {
    int r0 = 0, L = 0, h = 0;
};
// level-1 x index of (field f, coarse row gr -- unwrapped, within two rows of the tile --, wrapped column c); window
// rows past the ghosts (a partial last tile's) are clamped: they feed only outputs the tile does not own
template <bool PART>
__device__ inline int32_t g1_xidx(const G1Part& q, int nf, int f, int gr, int c, int nc) {
    if constexpr (!PART) {
        (void)q; (void)nf;
        return (f * nc + (gr < 0 ? gr + nc : (gr >= nc ? gr - nc : gr))) * nc + c;
    } else {
        const int lr = min(max(gr - q.r0, -q.h), q.L + q.h - 1);
        return ext_row(nf, f, lr, q.L, q.h, nc) + c;
    }
}
// the level-1 row of an owned output (f, cr, cc)
template <bool PART>
__device__ inline int32_t g1_orow(const G1Part& q, int f, int cr, int cc, int nc) {
    return PART ? (f * q.L + cr - q.r0) * nc + cc : (f * nc + cr) * nc + cc;
}
// PRO (the post-smoothing's first sweep after level 2's correction): the staged x is x + P_1 x_c, level 2's window
// [cr0 / 2 - 2, cr0 / 2 + kGFQH - 2) x [cc0 / 2 - 2, cc0 / 2 + kGFQW - 2) staged first (k_ftile<PRO>'s scheme one level
// down: the same P rows in window coordinates, k_mg_transfer_spmv's lists and EpiAdd's sum), and the epilogue's iterate
// is the row's own staged value -- the prolongation launch folded in, bit-identical.
// k_gal1's own tile: 16 x 8 coarse cells (a 32 x 16 fine block) -- its windows and t0 take 36.5 KB of LDS, so four
// workgroups share a CU (the 32 x 4 tile's 42 KB held three), and F's rows on the block + 1 are 612 instead of 660
constexpr int kGFW = 16, kGFH = 8;
constexpr int kGFCW = kGFW + 4, kGFCH = kGFH + 4;               // coarse x: [c0 - 2, c0 + W + 2)
constexpr int kGFFW = 2 * kGFW + 2, kGFFH = 2 * kGFH + 2;       // t1: fine block + 1
constexpr int kGFPW = kGFFW + 2, kGFPH = kGFFH + 2;             // t0 and thn: fine block + 2
constexpr int kGFQW = kGFW / 2 + 4, kGFQH = kGFH / 2 + 4;       // PRO: level 2's window (row stride kGFQW)
constexpr int kG1QW = kG1W / 2 + 4;                             // (k_gal1p's level-2 window columns)
template <bool INNER, class Epi, bool MAC, class XS, bool PART, bool PRO>
__device__ __forceinline__ void gal1_run(const FStencilFast& P, const MgFields& tr, const XS& xin, const Epi& epi,
                                         double* xs, double* ts, double* t0, double* t1, int cr0, int cc0,
                                         const G1Part& q, const double* xc, double* xq);
// MAC: the F hierarchy's kinds (u: rows cell-, columns node-centred; v: the reverse) at compile time
// XS: the coarse x as staged -- XPlain (x itself) or XInit (x0 = c2_0 (b / diag): a pre-smoothing's first sweep with the
// init pass folded in, as the grouped small levels do; the epilogue then EpiChebFirstGrp)
template <class Epi, bool MAC = false, class XS = XPlain, bool PART = false, bool PRO = false>
__global__ void __launch_bounds__(256) MPBP_LDS_READS k_gal1(FStencilFast P, MgFields tr, XS xin, Epi epi, G1Part q,
                                                              const double* __restrict__ xc = nullptr) {
    constexpr int CN = kGFCW * kGFCH, PN = kGFPW * kGFPH, FN = kGFFW * kGFFH;
    static_assert(!PRO || (MAC && !PART), "the folded prolongation: MAC kinds, whole level");
    __shared__ double xs[4 * CN];
    __shared__ double ts[PN];
    __shared__ double t0[4 * PN];
    __shared__ double xq[PRO ? 4 * kGFQW * kGFQH : 1];
    double* t1 = t0;
    static_assert(FN <= PN, "t1 fits t0");
    const int nc = P.n >> 1;
    const int tx = (nc + kGFW - 1) / kGFW;
    const int bk = xcd_swizzle(blockIdx.x, gridDim.x);
    const int cr0 = (PART ? q.r0 : 0) + (bk / tx) * kGFH, cc0 = (bk % tx) * kGFW;     // the coarse tile
    if constexpr (MAC) {
        if (g1_inner(cr0, cc0, kGFH, kGFW, nc)) {
            gal1_run<true, Epi, MAC, XS, PART, PRO>(P, tr, xin, epi, xs, ts, t0, t1, cr0, cc0, q, xc, xq);
            return;
        }
    }
    gal1_run<false, Epi, MAC, XS, PART, PRO>(P, tr, xin, epi, xs, ts, t0, t1, cr0, cc0, q, xc, xq);
}
template <bool INNER, class Epi, bool MAC, class XS, bool PART, bool PRO>
__device__ __forceinline__ void gal1_run(const FStencilFast& P, const MgFields& tr, const XS& xin, const Epi& epi,
                                         double* xs, double* ts, double* t0, double* t1, int cr0, int cc0,
                                         const G1Part& q, const double* xc, double* xq) {
    constexpr int CN = kGFCW * kGFCH, PN = kGFPW * kGFPH, FN = kGFFW * kGFFH;
    const int n = P.n, nc = n >> 1;
    const int fr0 = 2 * cr0, fc0 = 2 * cc0;                      // its fine block
    const int tid = threadIdx.x;
    auto wrapc = [&](int a) { return a < 0 ? a + nc : (a >= nc ? a - nc : a); };
    // a grid index to its slot in a staged window starting at virtual index `base` (the window is < the grid)
    auto slot = [](int i, int base, int m) { int l = i - base; return l < 0 ? l + m : (l >= m ? l - m : l); };
    {   // stage the coarse x (4 fields) and thn, every load before the first LDS store
        constexpr int IX = (4 * CN + 255) / 256, IT = (PN + 255) / 256;
        typename XS::Raw vx[IX];
        double vt[IT];
#pragma unroll
        for (int it = 0; it < IX; ++it) {
            const int i = tid + it * 256;
            if (i < 4 * CN) {
                const int f = i / CN, j = i - f * CN, r = j / kGFCW, c = j - r * kGFCW;
                vx[it] = xin.load(g1_xidx<PART>(q, 4, f, cr0 - 2 + r, wrapc(cc0 - 2 + c), nc));
            }
        }
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int i = tid + it * 256;
            if (i < PN) {
                const int r = i / kGFPW, c = i - r * kGFPW;
                vt[it] = P.cell[P.wrap(fr0 - 2 + r) * n + P.wrap(fc0 - 2 + c)];
            }
        }
        const int n2 = nc >> 1;
        if constexpr (PRO) {   // level 2's window first: the staged x needs it
            auto wrap2 = [&](int a) { return a < 0 ? a + n2 : (a >= n2 ? a - n2 : a); };
            constexpr int QF = kGFQW * kGFQH, IQ = (4 * QF + 255) / 256;
            double vq[IQ];
#pragma unroll
            for (int it = 0; it < IQ; ++it) {
                const int i = tid + it * 256;
                if (i < 4 * QF) {
                    const int f = i / QF, j = i - f * QF, r = j / kGFQW, c = j - r * kGFQW;
                    vq[it] = xc[(f * n2 + wrap2((cr0 >> 1) - 2 + r)) * n2 + wrap2((cc0 >> 1) - 2 + c)];
                }
            }
#pragma unroll
            for (int it = 0; it < IQ; ++it) {
                const int i = tid + it * 256;
                if (i < 4 * QF) {
                    const int f = i / QF, j = i - f * QF, r = j / kGFQW, c = j - r * kGFQW;
                    xq[(f * kGFQH + r) * kGFQW + c] = vq[it];
                }
            }
            __syncthreads();
        }
        const bool inner2 = PRO && g1_inner(cr0 >> 1, cc0 >> 1, kGFH / 2, kGFW / 2, n2);
#pragma unroll
        for (int it = 0; it < IX; ++it) {
            const int i = tid + it * 256;
            if (i >= 4 * CN) continue;
            double v = xin.value(vx[it]);
            if constexpr (PRO) {   // x + P_1 x_c (EpiAdd: the row sum, then + x)
                const int f = i / CN, j = i - f * CN, r = j / kGFCW, c = j - r * kGFCW;
                const double* xf = xq + f * kGFQH * kGFQW;
                const int gr = wrapc(cr0 - 2 + r), gc = wrapc(cc0 - 2 + c), rb = (cr0 >> 1) - 2, cb = (cc0 >> 1) - 2;
                const double pc = inner2 ? ((f & 1) ? g1_p_in<MPBP_MG_NODE, MPBP_MG_CELL, kGFQW>(xf, r, c)
                                                    : g1_p_in<MPBP_MG_CELL, MPBP_MG_NODE, kGFQW>(xf, r, c))
                                         : ((f & 1) ? g1_p<MPBP_MG_NODE, MPBP_MG_CELL, kGFQW>(xf, gr, gc, n2, rb, cb)
                                                    : g1_p<MPBP_MG_CELL, MPBP_MG_NODE, kGFQW>(xf, gr, gc, n2, rb, cb));
                v = pc + v;
            }
            xs[i] = v;
        }
#pragma unroll
        for (int it = 0; it < IT; ++it)
            if (tid + it * 256 < PN) ts[tid + it * 256] = vt[it];
    }
    // the faces of this lane's t1 cells, loaded ahead (their latency behind the P_0 stage, not in the F stage)
    constexpr int IF = (FN + 255) / 256;
    double fu[IF], fv[IF];
#pragma unroll
    for (int it = 0; it < IF; ++it) {
        const int i = tid + it * 256;
        if (i < FN) {
            const int r = i / kGFFW, c = i - r * kGFFW;
            const int32_t k = P.wrap(fr0 - 1 + r) * n + P.wrap(fc0 - 1 + c);
            fu[it] = P.uface[k];
            fv[it] = P.vface[k];
        }
    }
    __syncthreads();
    // t0 = P_0 x on the fine block + 2
    for (int i = tid; i < PN; i += 256) {
        const int r = i / kGFPW, c = i - r * kGFPW;
        const int gr = P.wrap(fr0 - 2 + r), gc = P.wrap(fc0 - 2 + c);
        if constexpr (MAC && INNER) {
#pragma unroll
            for (int f = 0; f < 4; ++f)
                t0[f * PN + i] = (f & 1) ? g1_p_in<MPBP_MG_NODE, MPBP_MG_CELL, kGFCW>(xs + f * CN, r, c)
                                         : g1_p_in<MPBP_MG_CELL, MPBP_MG_NODE, kGFCW>(xs + f * CN, r, c);
            continue;
        }
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            if constexpr (MAC) {
                t0[f * PN + i] = (f & 1)
                    ? g1_p<MPBP_MG_NODE, MPBP_MG_CELL, kGFCW>(xs + f * CN, gr, gc, nc, cr0 - 2, cc0 - 2)
                    : g1_p<MPBP_MG_CELL, MPBP_MG_NODE, kGFCW>(xs + f * CN, gr, gc, nc, cr0 - 2, cc0 - 2);
                continue;
            }
            int yi[4], xi[4];
            double yw[4], xw[4];
            const int my = mg_p1d_fast(tr.ky[f], nc, gr, yi, yw), mx = mg_p1d_fast(tr.kx[f], nc, gc, xi, xw);
            double acc = 0.0;
            for (int a = 0; a < my; ++a) {
                const double* xr = xs + f * CN + slot(yi[a], cr0 - 2, nc) * kGFCW;
                for (int b = 0; b < mx; ++b) acc += (yw[a] * xw[b]) * xr[slot(xi[b], cc0 - 2, nc)];
            }
            t0[f * PN + i] = acc;
        }
    }
    __syncthreads();
    // t1 = F t0 on the fine block + 1
    {
        const TTileT<kGFPW> tt{ts, fr0 - 2, fc0 - 2};
        const XTileT<kGFPW, kGFPH> xt{t0, fr0 - 2, fc0 - 2};
        // t1 takes t0's LDS (63 -> 42 KB per workgroup: 3 resident per CU instead of 2): rows kept in registers until
        // every lane has read its t0 neighbours
        double tv[IF][4];
#pragma unroll
        for (int it = 0; it < IF; ++it) {
            const int i = tid + it * 256;
            if (i >= FN) break;
            const int r = i / kGFFW, c = i - r * kGFFW;
            double rd[4];
            P.template rows4<false>(fr0 - 1 + r, fc0 - 1 + c, tt, xt, FStencilDev::Cell{{fu[it], fv[it]}}, tv[it], rd);
        }
        __syncthreads();
#pragma unroll
        for (int it = 0; it < IF; ++it) {
            const int i = tid + it * 256;
            if (i >= FN) break;
#pragma unroll
            for (int f = 0; f < 4; ++f) t1[f * FN + i] = tv[it][f];
        }
    }
    __syncthreads();
    // R_0 t1 on the tile's coarse rows (4 fields x 128 cells), each to the epilogue
    if constexpr (MAC) {   // lane t: cell t & 127 of fields (t >> 7) and (t >> 7) + 2 -- one kind pair per wave
        const int cell = tid & (kGFW * kGFH - 1), fp = tid >> 7;
        const int cr = cr0 + cell / kGFW, cc = cc0 + cell % kGFW;
        if (cr < (PART ? q.r0 + q.L : nc) && cc < nc) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int f = fp + 2 * h;
                const int32_t row = g1_orow<PART>(q, f, cr, cc, nc);
                typename Epi::P pe;
                if constexpr (PRO) {   // the iterate is the staged x + P_1 x_c at the row
                    pe = epi.pre_lite(row);
                    set_x(pe, xs[f * CN + (cr - cr0 + 2) * kGFCW + (cc - cc0 + 2)]);
                    set_diag(pe, epi.diag[row]);
                } else {
                    pe = epi.pre(row);
                }
                double acc;
                if constexpr (INNER)
                    acc = fp ? g1_r_in<MPBP_MG_NODE, MPBP_MG_CELL, kGFFW>(t1 + f * FN, cr - cr0, cc - cc0)
                             : g1_r_in<MPBP_MG_CELL, MPBP_MG_NODE, kGFFW>(t1 + f * FN, cr - cr0, cc - cc0);
                else
                    acc = fp ? g1_r<MPBP_MG_NODE, MPBP_MG_CELL, kGFFW>(t1 + f * FN, cr, cc, n, fr0 - 1, fc0 - 1)
                             : g1_r<MPBP_MG_CELL, MPBP_MG_NODE, kGFFW>(t1 + f * FN, cr, cc, n, fr0 - 1, fc0 - 1);
                epi(row, acc, pe);
            }
        }
        return;
    }
    for (int j = tid; j < 4 * kGFW * kGFH; j += 256) {
        const int f = j / (kGFW * kGFH), cell = j - f * (kGFW * kGFH);
        const int cr = cr0 + cell / kGFW, cc = cc0 + cell % kGFW;
        if (cr >= (PART ? q.r0 + q.L : nc) || cc >= nc) continue;
        const int32_t row = g1_orow<PART>(q, f, cr, cc, nc);
        const typename Epi::P pe = epi.pre(row);
        int yi[4], xi[4];
        double yw[4], xw[4];
        const int my = mg_r1d_fast(tr.ky[f], n, cr, yi, yw), mx = mg_r1d_fast(tr.kx[f], n, cc, xi, xw);
        double acc = 0.0;
        for (int a = 0; a < my; ++a) {
            const double* tr1 = t1 + f * FN + slot(yi[a], fr0 - 1, n) * kGFFW;
            for (int b = 0; b < mx; ++b) acc += (yw[a] * xw[b]) * tr1[slot(xi[b], fc0 - 1, n)];
        }
        epi(row, acc, pe);
    }
}

// ---- multigrid level 0 of a tolerance-mode F hierarchy: pre-smoothing, residual and restriction in one launch ----
// k_fpre (the V-cycle's descent at level 0, V(2, .) from x = 0): on k_fsolve's 64 x 8 tiles with H = 3 levels -- x0 =
// c2_0 b / diag over the tile + 3, the Chebyshev sweep x1 over the tile + 2 (written out on the tile: the iterate the
// post-smoothing continues from), the residual r = b - F x1 over the tile + 1 (in LDS), then R_0 r on the tile's 32 x 4
// coarse cells into the coarse right-hand side.  Each value is built by the operations of the launches it replaces
// (k_ftile<INIT>'s x0 and sweep, the residual sweep's tolerance-mode rows and EpiResid, k_mg_transfer_spmv's restriction
// lists and product order): bit-identical to them.  HBM: b, thn and faces in, x1 and the coarse rhs out -- the residual
// is never written.
template <int KY, int KX, int W>
__device__ inline double g1_rw(const double* tf, int cr, int cc, int n, int rb, int cb) {
    constexpr int MY = KY == MPBP_MG_CELL ? 4 : 3, MX = KX == MPBP_MG_CELL ? 4 : 3;
    int yi[4], xi[4];
    double yw[4], xw[4];
    mg_r1d_fast(KY, n, cr, yi, yw);
    mg_r1d_fast(KX, n, cc, xi, xw);
    double acc = 0.0;
#pragma unroll
    for (int a = 0; a < MY; ++a) {
        const double* tr1 = tf + g1_slot(yi[a], rb, n) * W;
#pragma unroll
        for (int b = 0; b < MX; ++b) acc += (yw[a] * xw[b]) * tr1[g1_slot(xi[b], cb, n)];
    }
    return acc;
}
struct FPre {
    const double* b;   // the level's right-hand side
    double* x_out;     // x1 (the pre-smoothed iterate)
    double* bc;        // the coarse right-hand side R_0 (b - F x1)
    double c2_0, c1, c2;
};
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 8))) MPBP_LDS_READS
k_fpre(FStencilFast P, FPre a) {
    constexpr int H = 3;
    using T = FsTile<H>;
    // slots: the two tile cells (0, 1), rings 1 .. 3 (2 .. 4); ring 1 lives through the residual level, ring 2
    // through the sweep, ring 3 is x0 only -- state (d, 1 / diag) for slots 0 .. 3
    constexpr int NT = 2, NSL = H + 2, NS = H + 1;
    __shared__ double ts[T::TN];
    __shared__ double xa[4 * T::N], xb[4 * T::N];
    const int n = P.n, nn = n * n, nc = n >> 1, ncc = nc * nc;
    const int tx = (n + kFTW - 1) / kFTW;
    const int bk = xcd_swizzle(blockIdx.x, gridDim.x);
    const int r0 = (bk / tx) * kFTH, c0 = (bk % tx) * kFTW;
    const int rbt = r0 - H - 1, cbt = c0 - H - 1, rb = r0 - H, cb = c0 - H;
    const int tid = threadIdx.x;
    {
        constexpr int IT = (T::TN + 255) / 256;
        double v[IT];
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int i = tid + it * 256;
            if (i < T::TN) {
                const int sr = i / T::TW, sc = i - sr * T::TW;
                v[it] = P.cell[P.wrap(rbt + sr) * n + P.wrap(cbt + sc)];
            }
        }
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int i = tid + it * 256;
            if (i < T::TN) ts[i] = v[it];
        }
    }
    const int lr = tid >> 6, lc = tid & 63;
    int cr[NSL], cc[NSL], rr[NSL];
    bool own[NSL];
#pragma unroll
    for (int m = 0; m < NT; ++m) {
        cr[m] = r0 + lr + 4 * m; cc[m] = c0 + lc; own[m] = true; rr[m] = 0;
    }
#pragma unroll
    for (int r = 1; r <= H; ++r) {
        own[1 + r] = tid < 140 + 8 * r;
        rr[1 + r] = r;
        fs_ring_cell(r, own[1 + r] ? tid : 0, r0, c0, cr[1 + r], cc[1 + r]);
    }
    double fl[NSL][2], bl[NSL][4];
#pragma unroll
    for (int sl = 0; sl < NSL; ++sl) {
        if (!own[sl]) continue;
        const int gr = P.wrap(cr[sl]), gc = P.wrap(cc[sl]);
        const int32_t k = gr * n + gc;
        fl[sl][0] = P.uface[k];
        fl[sl][1] = P.vface[k];
#pragma unroll
        for (int f = 0; f < 4; ++f) bl[sl][f] = a.b[(f * n + gr) * n + gc];
    }
    __syncthreads();
    const TTileT<T::TW> tt{ts, rbt, cbt};
    double d[NS][4], rd[NS][4];
    // level 0: x0 = d0 = c2_0 b / diag over the tile + 3
#pragma unroll
    for (int sl = 0; sl < NSL; ++sl) {
        if (!own[sl]) continue;
        const int vr = cr[sl], vc = cc[sl];
        const FStencilDev::Stage sg{{fl[sl][0], fl[sl][1]}};
        double r4[4];
        P.rdiag4(vr, vc, tt, sg, r4);
        const int si = (vr - rb) * T::RW + (vc - cb);
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            const double x0 = a.c2_0 * bl[sl][f] * r4[f];
            xa[f * T::N + si] = x0;
            if (sl < NS) {
                d[sl][f] = x0;
                rd[sl][f] = r4[f];
            }
        }
    }
    __syncthreads();
    // level 1: the sweep over the tile + 2 (x1 into xb; the tile's cells also to memory)
    {
        const XTileT<T::RW, T::RH> xt{xa, rb, cb};
#pragma unroll
        for (int sl = 0; sl < NS; ++sl) {
            if (sl >= NT && (!own[sl] || rr[sl] > 2)) continue;
            const int vr = cr[sl], vc = cc[sl];
            double acc[4], rdx[4];
            P.template rows4<false>(vr, vc, tt, xt, FStencilDev::Cell{{fl[sl][0], fl[sl][1]}}, acc, rdx);
            const int si = (vr - rb) * T::RW + (vc - cb);
#pragma unroll
            for (int f = 0; f < 4; ++f) {
                const double z = (bl[sl][f] - acc[f]) * rd[sl][f];
                const double dn = a.c1 * d[sl][f] + a.c2 * z;
                const double x = xa[f * T::N + si] + dn;
                xb[f * T::N + si] = x;
                if (sl < NT && vr < n && vc < n) a.x_out[f * nn + vr * n + vc] = x;
            }
        }
    }
    __syncthreads();
    // level 2: r = b - F x1 over the tile + 1 (into xa)
    {
        const XTileT<T::RW, T::RH> xt{xb, rb, cb};
#pragma unroll
        for (int sl = 0; sl < NS; ++sl) {
            if (sl >= NT && (!own[sl] || rr[sl] > 1)) continue;
            const int vr = cr[sl], vc = cc[sl];
            double acc[4], rdx[4];
            P.template rows4<false>(vr, vc, tt, xt, FStencilDev::Cell{{fl[sl][0], fl[sl][1]}}, acc, rdx);
            const int si = (vr - rb) * T::RW + (vc - cb);
#pragma unroll
            for (int f = 0; f < 4; ++f) xa[f * T::N + si] = bl[sl][f] - acc[f];
        }
    }
    __syncthreads();
    // R_0 r on the tile's coarse rows (4 fields x 128 cells; the F hierarchy's MAC kinds): lane t, cell t & 127 of
    // fields (t >> 7) and (t >> 7) + 2
    const int cell = tid & (kG1W * kG1H - 1), fp = tid >> 7;
    const int crr = (r0 >> 1) + cell / kG1W, ccc = (c0 >> 1) + cell % kG1W;
    if (crr < nc && ccc < nc) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int f = fp + 2 * h;
            const bool inner = g1_inner(r0 >> 1, c0 >> 1, kFTH / 2, kFTW / 2, nc);   // (window coordinates, slot 2 =
                                                                                     // fine 2 c0 - 1: rb = r0 - 3)
            const int lr = crr - (r0 >> 1), lc = ccc - (c0 >> 1);
            const double acc =
                inner ? (fp ? g1_rw_in<MPBP_MG_NODE, MPBP_MG_CELL, T::RW, 2>(xa + f * T::N, lr, lc)
                            : g1_rw_in<MPBP_MG_CELL, MPBP_MG_NODE, T::RW, 2>(xa + f * T::N, lr, lc))
                      : (fp ? g1_rw<MPBP_MG_NODE, MPBP_MG_CELL, T::RW>(xa + f * T::N, crr, ccc, n, rb, cb)
                            : g1_rw<MPBP_MG_CELL, MPBP_MG_NODE, T::RW>(xa + f * T::N, crr, ccc, n, rb, cb));
            a.bc[f * ncc + crr * nc + ccc] = acc;
        }
    }
}

// The pressure hierarchy's level 1 the same way (tolerance mode): A_1 x = R_0 (Gt_G (P_0 x)) on a 32 x 8 coarse tile
// (a 64 x 16 fine block), one field, cell-centred both ways; Gt_G's rows by GtGStencilDev::entries and add5 (the
// matrix-free level-0 sweep's operations), the transfers' by k_mg_transfer_spmv's: bit-identical to the three launches.
constexpr int kG1PH2 = 8;                                     // coarse tile rows (pressure)
constexpr int kGPFH = 2 * kG1PH2 + 2, kGPPH = kGPFH + 2;       // fine t1 / t0 rows
// PRO: as k_gal1's (x + P_1 x_c staged, level 2's window of the 16 x 4 level-2 cells under the tile first)
constexpr int kG1PQH = kG1PH2 / 2 + 4;   // level-2 window rows (columns kG1QW, row stride kG1CW)
template <class Epi, class XS = XPlain, bool PART = false, bool PRO = false>
__global__ void __launch_bounds__(256) MPBP_LDS_READS k_gal1p(GtGStencilDev P, XS xin, Epi epi, G1Part q,
                                                               const double* __restrict__ xc = nullptr) {
    constexpr int CH = kG1PH2 + 4, CN = kG1CW * CH, PN = kG1PW * kGPPH, FN = kG1FW * kGPFH;
    __shared__ double xs[CN];
    __shared__ double ts[PN];
    __shared__ double t0[PN];
    __shared__ double xq[PRO ? kG1CW * kG1PQH : 1];
    static_assert(!PRO || !PART, "the folded prolongation: whole level");
    double* t1 = t0;   // (k_gal1's aliasing: 34.7 -> 25 KB per workgroup)
    static_assert(FN <= PN, "t1 fits t0");
    const int n = P.n, nc = n >> 1;
    const int tx = (nc + kG1W - 1) / kG1W;
    const int bk = xcd_swizzle(blockIdx.x, gridDim.x);
    const int cr0 = (PART ? q.r0 : 0) + (bk / tx) * kG1PH2, cc0 = (bk % tx) * kG1W;
    const int fr0 = 2 * cr0, fc0 = 2 * cc0;
    const int tid = threadIdx.x;
    auto wrapc = [&](int a) { return a < 0 ? a + nc : (a >= nc ? a - nc : a); };
    {
        constexpr int IX = (CN + 255) / 256, IT = (PN + 255) / 256;
        typename XS::Raw vx[IX];
        double vt[IT];
#pragma unroll
        for (int it = 0; it < IX; ++it) {
            const int i = tid + it * 256;
            if (i < CN) {
                const int r = i / kG1CW, c = i - r * kG1CW;
                vx[it] = xin.load(g1_xidx<PART>(q, 1, 0, cr0 - 2 + r, wrapc(cc0 - 2 + c), nc));
            }
        }
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int i = tid + it * 256;
            if (i < PN) {
                const int r = i / kG1PW, c = i - r * kG1PW;
                vt[it] = P.cell[P.wrap(fr0 - 2 + r) * n + P.wrap(fc0 - 2 + c)];
            }
        }
        const int n2 = nc >> 1;
        if constexpr (PRO) {   // level 2's window first
            auto wrap2 = [&](int a) { return a < 0 ? a + n2 : (a >= n2 ? a - n2 : a); };
            constexpr int QN = kG1QW * kG1PQH, IQ = (QN + 255) / 256;
            double vq[IQ];
#pragma unroll
            for (int it = 0; it < IQ; ++it) {
                const int i = tid + it * 256;
                if (i < QN) {
                    const int r = i / kG1QW, c = i - r * kG1QW;
                    vq[it] = xc[wrap2((cr0 >> 1) - 2 + r) * n2 + wrap2((cc0 >> 1) - 2 + c)];
                }
            }
#pragma unroll
            for (int it = 0; it < IQ; ++it) {
                const int i = tid + it * 256;
                if (i < QN) {
                    const int r = i / kG1QW, c = i - r * kG1QW;
                    xq[r * kG1CW + c] = vq[it];
                }
            }
            __syncthreads();
        }
        const bool inner2 = PRO && g1_inner(cr0 >> 1, cc0 >> 1, kG1PH2 / 2, kG1W / 2, n2);
#pragma unroll
        for (int it = 0; it < IX; ++it) {
            const int i = tid + it * 256;
            if (i >= CN) continue;
            double v = xin.value(vx[it]);
            if constexpr (PRO) {   // x + P_1 x_c (EpiAdd: the row sum, then + x)
                const int r = i / kG1CW, c = i - r * kG1CW;
                const double pc =
                    inner2 ? g1_p_in<MPBP_MG_CELL, MPBP_MG_CELL>(xq, r, c)
                           : g1_p<MPBP_MG_CELL, MPBP_MG_CELL>(xq, wrapc(cr0 - 2 + r), wrapc(cc0 - 2 + c), n2,
                                                              (cr0 >> 1) - 2, (cc0 >> 1) - 2);
                v = pc + v;
            }
            xs[i] = v;
        }
#pragma unroll
        for (int it = 0; it < IT; ++it)
            if (tid + it * 256 < PN) ts[tid + it * 256] = vt[it];
    }
    __syncthreads();
    const bool inner = g1_inner(cr0, cc0, kG1PH2, kG1W, nc);   // (k_gal1's g1_*_in)
    for (int i = tid; i < PN; i += 256) {   // t0 = P_0 x on the fine block + 2
        const int r = i / kG1PW, c = i - r * kG1PW;
        t0[i] = inner ? g1_p_in<MPBP_MG_CELL, MPBP_MG_CELL>(xs, r, c)
                      : g1_p<MPBP_MG_CELL, MPBP_MG_CELL>(xs, P.wrap(fr0 - 2 + r), P.wrap(fc0 - 2 + c), nc, cr0 - 2, cc0 - 2);
    }
    __syncthreads();
    {   // t1 = Gt_G t0 on the fine block + 1
        const TTileT<kG1PW> ta{ts, fr0 - 2, fc0 - 2};
        constexpr int IT1 = (FN + 255) / 256;
        double tv[IT1];
#pragma unroll
        for (int it = 0; it < IT1; ++it) {
            const int i0 = it * 256;
            const int i = i0 + tid;
            const bool live = i < FN;
            const int ii = live ? i : 0;
            const int r = ii / kG1FW, c = ii - r * kG1FW;
            const int vr = fr0 - 1 + r, vc = fc0 - 1 + c, gr = P.wrap(vr), gc = P.wrap(vc);
            const bool edge = __builtin_amdgcn_readfirstlane(__any(live && (gr == 0 || gr == n - 1 || gc == 0 ||
                                                                            gc == n - 1))) != 0;
            if (!live) continue;
            double e[5];
            P.entries(vr, vc, gr, gc, ta, e);
            const int si = (r + 1) * kG1PW + (c + 1);
            const double pr[5] = {e[0] * t0[si - kG1PW], e[1] * t0[si - 1], e[2] * t0[si], e[3] * t0[si + 1],
                                  e[4] * t0[si + kG1PW]};
            const Wrap wr{gr == 0, gr == n - 1, gc == 0, gc == n - 1};
            tv[it] = edge ? add5<true>(0.0, pr, wr) : add5<false>(0.0, pr, wr);
        }
        __syncthreads();
#pragma unroll
        for (int it = 0; it < IT1; ++it)
            if (it * 256 + tid < FN) t1[it * 256 + tid] = tv[it];
    }
    __syncthreads();
    {   // R_0 t1 on the tile's 256 coarse rows, each to the epilogue
        const int cr = cr0 + tid / kG1W, cc = cc0 + tid % kG1W;
        if (cr < (PART ? q.r0 + q.L : nc) && cc < nc) {
            const int32_t row = g1_orow<PART>(q, 0, cr, cc, nc);
            typename Epi::P pe;
            if constexpr (PRO) {   // the iterate is the staged x + P_1 x_c at the row
                pe = epi.pre_lite(row);
                set_x(pe, xs[(cr - cr0 + 2) * kG1CW + (cc - cc0 + 2)]);
                set_diag(pe, epi.diag[row]);
            } else {
                pe = epi.pre(row);
            }
            epi(row, inner ? g1_r_in<MPBP_MG_CELL, MPBP_MG_CELL>(t1, cr - cr0, cc - cc0)
                           : g1_r<MPBP_MG_CELL, MPBP_MG_CELL>(t1, cr, cc, n, fr0 - 1, fc0 - 1), pe);
        }
    }
}

}  // namespace
