// One Gt_G Chebyshev solve in one launch (k_gtg_solve) and the pressure hierarchy's multigrid level 0, descent and
// ascent in one launch each.
// Needs mpbp.hip's xcd_swizzle and the F stencil's edge order, f_tile.inc's geometry (kFTW, kFTH, TTileT,
// fs_ring_cell, the g1_* declarations), fs_ring_cell_t (f_solve_w.inc) and GtGStencilDev (pg_stencil.inc).
// A fragment of mpbp.hip, included there once and in order: not a self-contained header.

namespace {

// ---- one Gt_G Chebyshev solve in one launch (k_gtg_solve) ----
// The pressure solves x = Gt_G^-1 b of the apply (solve.py:265, 271) as K Chebyshev-Jacobi sweeps from x0 = 0, fused:
// a workgroup owns a TW x TH tile of cells and stages b and thn over the tile plus a halo of H = K - 1 cells, and
// x0 = d0 = c2_0 (b / diag) there from the stored diagonal (level 0).  Level l = 1 .. H recomputes the tile with halo
// H - l from level l - 1 (LDS ping-pong), the last writing the tile.  As in k_fsolve every cell has one owning lane for
// all its levels (the lane's two tile cells, and cell t of each halo ring r = 1 .. H - 1), which builds the cell's five
// entries once (GtGStencilDev::entries, from the staged thn) and keeps them, b and d in registers: a level reads only
// the five x values of the stencil from LDS.  Each row is GtGStencilDev::apply_v's IEEE operations (the entries', the
// products', add5's column order) and each update the Chebyshev epilogue's (EpiChebFirst at level 1, EpiCheb after):
// bit-identical to the K - 1 sweeps of the per-sweep path, for one launch and one pass over b instead of K - 1 passes
// over x, d, b.
constexpr int kGTW = kFTW, kGTH = kFTH;   // the 64 x 8 tile and ring numbering of k_fsolve (fs_ring_cell)
struct ChebK {
    double c1[8], c2[8];   // sweep s's coefficients (c2[0]: the initial iterate's)
};
template <int H, int GW = kGTW, int GH = kGTH>
struct GtgTile {   // a GW x GH tile of cells with H halo levels
    static constexpr int RW = GW + 2 * H, RH = GH + 2 * H, N = RW * RH;
    static constexpr int ring(int r) { return 2 * GW + 2 * GH - 4 + 8 * r; }   // cells of halo ring r
    static constexpr int rings(int h) { return h < 1 ? 0 : ring(h) + rings(h - 1); }
};
template <int H>
struct TTile {   // thn of the staged tile; (r, c) in the tile's virtual grid coordinates
    const double* t;
    int rb, cb;
    __device__ double T(int sph, int r, int c) const {
        const double v = t[(r - rb) * GtgTile<H>::RW + (c - cb)];
        return sph ? 1.0 - v : v;
    }
};

// PART: the tiles cover a row partition's owned rows and P.ext ghost rows each side (the CA schedule); b and diag in
// its ghost layout (depth P.h >= P.ext + H; deeper rows, read only for cells no output depends on, clamped), out in
// the output layout (depth P.oh).
// TPB = 512: one tile cell and at most one ring cell per lane (rings 1 .. H - 1 numbered across the workgroup), so a
// level's critical path is half as long and the smaller register state lets more waves share the CU.
// DB (one GPU): the right-hand side is rhs = D Y + v_p (solve.py:259), built at every staged cell with
// DStencilDev::row's operations and EpiAdd's sum from thn staged one cell wider and Y (the four velocity fields) from
// memory: the D launch, and rhs's write and re-read, disappear.
struct GtgD {
    const double* Y;    // Finv_v: u_n, v_n, u_s, v_s
    const double* vp;   // v's pressure part
};
template <int H, bool PART, int TPB, bool DB, int GW = kGTW, int GH = kGTH>
__global__ void __launch_bounds__(TPB) MPBP_LDS_READS k_gtg_solve(GtGStencilDev P, const double* __restrict__ b,
                                                   const double* __restrict__ diag, ChebK ck, double* __restrict__ out,
                                                   GtgD dv) {
    using G = GtgTile<H, GW, GH>;
    constexpr int SW = DB ? G::RW + 2 : G::RW, TN = DB ? SW * (G::RH + 2) : G::N;   // staged thn
    constexpr int NM = GW * GH / TPB;                // tile cells per lane
    constexpr int NR = TPB == 256 ? H - 1 : 1;       // ring slots per lane (rings 1 .. H - 1)
    constexpr int NS = NM + NR;
    static_assert(NM * TPB == GW * GH && TPB % GW == 0, "whole tile rows per lane group");
    static_assert(TPB == 512 || G::ring(H - 1) <= 256, "256 lanes own one cell of each ring");
    static_assert(TPB == 256 || G::rings(H - 1) <= 512, "512 lanes own at most one ring cell each");
    __shared__ double ts[TN], bs[G::N], xa[G::N], xb[G::N];
    const int n = P.n;
    const int tx = (n + GW - 1) / GW;
    const int bk = xcd_swizzle(blockIdx.x, gridDim.x);
    const int lo = PART ? P.r0 - P.ext : 0, hi = PART ? P.r0 + P.L + P.ext : n;   // output rows [lo, hi)
    const int r0 = lo + (bk / tx) * GH, c0 = (bk % tx) * GW;
    const int rb = r0 - H, cb = c0 - H;   // virtual coordinates of staged cell 0
    const int tid = threadIdx.x;
    // level 0 over the whole staged region: thn, b, x0 = c2_0 (b / diag); every load issued before the first LDS store
    if constexpr (DB) {
        const int nn = n * n;
        {   // thn one cell wider than the staged region
            constexpr int IT = (TN + TPB - 1) / TPB;
            double tv[IT];
#pragma unroll
            for (int it = 0; it < IT; ++it) {
                const int i = tid + it * TPB;
                if (i < TN) {
                    const int rr = i / SW, cc = i - rr * SW;
                    tv[it] = P.cell[P.wrap(rb - 1 + rr) * n + P.wrap(cb - 1 + cc)];
                }
            }
#pragma unroll
            for (int it = 0; it < IT; ++it)
                if (tid + it * TPB < TN) ts[tid + it * TPB] = tv[it];
        }
        // every staged cell's Y, v_p and diagonal loaded ahead of the barrier: one memory latency, not one per cell
        constexpr int IY = (G::N + TPB - 1) / TPB;
        double yl[IY][8], vpl[IY], dgl[IY];
#pragma unroll
        for (int it = 0; it < IY; ++it) {
            const int i = tid + it * TPB;
            if (i >= G::N) break;
            const int rr = i / G::RW, cc = i - rr * G::RW;
            const int gr = P.wrap(rb + rr), gc = P.wrap(cb + cc);
            const int ge = gc == n - 1 ? 0 : gc + 1, gs = gr == n - 1 ? 0 : gr + 1;
            const int32_t k = gr * n + gc;
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                yl[it][4 * q + 0] = dv.Y[2 * q * nn + gr * n + ge];         // u at the east face
                yl[it][4 * q + 1] = dv.Y[2 * q * nn + k];                   // u at the cell's west face
                yl[it][4 * q + 2] = dv.Y[(2 * q + 1) * nn + k];             // v at its north face
                yl[it][4 * q + 3] = dv.Y[(2 * q + 1) * nn + gs * n + gc];   // v at the south face
            }
            vpl[it] = dv.vp[k];
            dgl[it] = diag[k];
        }
        __syncthreads();
        const TTileT<SW> tD{ts, rb - 1, cb - 1};
#pragma unroll
        for (int it = 0; it < IY; ++it) {
            const int i = tid + it * TPB;
            if (i >= G::N) break;
            const int rr = i / G::RW, cc = i - rr * G::RW;
            const int vr = rb + rr, vc = cb + cc, gr = P.wrap(vr), gc = P.wrap(vc);
            const double* yv = yl[it];
            const double vpk = vpl[it], dgk = dgl[it];
            const bool lastc = gc == n - 1, lastr = gr == n - 1;   // the wrapped neighbour sorts first (DStencilDev)
            double acc = 0.0;
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const double t0 = tD.T(q, vr, vc), tE = tD.T(q, vr, vc + 1), tWv = tD.T(q, vr, vc - 1);
                const double tN = tD.T(q, vr - 1, vc), tS = tD.T(q, vr + 1, vc);
                const double uE = (P.inv * (0.5 * (t0 + tE))) * yv[4 * q + 0];
                const double uC = (P.minv * (0.5 * (t0 + tWv))) * yv[4 * q + 1];
                const double vC = (P.inv * (0.5 * (t0 + tN))) * yv[4 * q + 2];
                const double vS = (P.minv * (0.5 * (t0 + tS))) * yv[4 * q + 3];
                acc += lastc ? uE : uC;
                acc += lastc ? uC : uE;
                acc += lastr ? vS : vC;
                acc += lastr ? vC : vS;
            }
            const double bvv = acc + vpk;   // EpiAdd
            bs[i] = bvv;
            xa[i] = ck.c2[0] * (bvv / dgk);
        }
    } else {
        constexpr int IT = (G::N + TPB - 1) / TPB;
        double bv[IT], tv[IT], dv_[IT];
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int i = tid + it * TPB;
            if (i < G::N) {
                const int rr = i / G::RW, cc = i - rr * G::RW;
                const int gr = P.wrap(rb + rr), gc = P.wrap(cb + cc);
                int32_t kb = gr * n + gc;
                if constexpr (PART) {
                    int lr = rb + rr - P.r0;
                    lr = lr < -P.h ? -P.h : (lr >= P.L + P.h ? P.L + P.h - 1 : lr);
                    kb = ext_row(1, 0, lr, P.L, P.h, n) + gc;
                }
                bv[it] = b[kb];
                tv[it] = P.cell[gr * n + gc];
                dv_[it] = diag[kb];
            }
        }
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int i = tid + it * TPB;
            if (i < G::N) {
                ts[i] = tv[it];
                bs[i] = bv[it];
                xa[i] = ck.c2[0] * (bv[it] / dv_[it]);
            }
        }
    }
    __syncthreads();
    // the owned cells (slot 0, 1: the tile's; slot 1 + r: ring r), their entries, b and d0 = x0
    const TTileT<SW> ta{ts, DB ? rb - 1 : rb, DB ? cb - 1 : cb};
    const int lr = tid / GW, lc = tid % GW;
    int cr[NS], cc[NS], si[NS], rr[NS];
    bool own[NS], edge[NS];
    double e[NS][5], bo[NS], d[NS];
#pragma unroll
    for (int m = 0; m < NM; ++m) {
        cr[m] = r0 + lr + (TPB / GW) * m; cc[m] = c0 + lc; own[m] = true; rr[m] = 0;
    }
    if constexpr (TPB == 256) {
#pragma unroll
        for (int r = 1; r < H; ++r) {
            own[NM + r - 1] = tid < G::ring(r);
            rr[NM + r - 1] = r;
            fs_ring_cell_t<GW, GH>(r, own[NM + r - 1] ? tid : 0, r0, c0, cr[NM + r - 1], cc[NM + r - 1]);
        }
    } else if constexpr (NR > 0) {
        int r = 0, j = tid;   // rings 1 .. H - 1 numbered ring 1 first: lane t owns cell t of that sequence
#pragma unroll
        for (int q = 1; q < H; ++q)
            if (r == 0) {
                if (j < G::ring(q)) r = q;
                else j -= G::ring(q);
            }
        own[NM] = r != 0;
        rr[NM] = r;
        fs_ring_cell_t<GW, GH>(r ? r : 1, r ? j : 0, r0, c0, cr[NM], cc[NM]);
    }
#pragma unroll
    for (int sl = 0; sl < NS; ++sl) {
        const int vr = cr[sl], vc = cc[sl], gr = P.wrap(vr), gc = P.wrap(vc);
        si[sl] = (vr - rb) * G::RW + (vc - cb);
        edge[sl] = __builtin_amdgcn_readfirstlane(__any(own[sl] && (gr == 0 || gr == n - 1 || gc == 0 ||
                                                                    gc == n - 1))) != 0;
        if (own[sl]) {
            P.entries(vr, vc, gr, gc, ta, e[sl]);
            bo[sl] = bs[si[sl]];
            d[sl] = xa[si[sl]];
        }
    }
    double* cur = xa;
    double* nxt = xb;
#pragma unroll
    for (int l = 1; l <= H; ++l) {
        if (l > 1) __syncthreads();
        const double c1 = ck.c1[l], c2 = ck.c2[l];
#pragma unroll
        for (int sl = 0; sl < NS; ++sl) {
            if (TPB == 256 && sl >= NM && sl - NM + 1 > H - l) continue;   // (compile time) ring sl - NM + 1 is done
            if (sl >= NM && (!own[sl] || rr[sl] > H - l)) continue;        // ring rr lives through level H - rr
            const int vr = cr[sl], vc = cc[sl];
            if (l == H && (vr >= hi || vc >= n)) continue;            // a tile past the last row / column
            const int i = si[sl];
            const double p[5] = {e[sl][0] * cur[i - G::RW], e[sl][1] * cur[i - 1], e[sl][2] * cur[i],
                                 e[sl][3] * cur[i + 1], e[sl][4] * cur[i + G::RW]};
            const int gr = P.wrap(vr), gc = P.wrap(vc);
            const Wrap wr{gr == 0, gr == n - 1, gc == 0, gc == n - 1};
            const double acc = edge[sl] ? add5<true>(0.0, p, wr) : add5<false>(0.0, p, wr);
            const double z = (bo[sl] - acc) / e[sl][2];
            const double dn = c1 * d[sl] + c2 * z;
            const double x = cur[i] + dn;
            if (l < H) {
                nxt[i] = x;
                d[sl] = dn;
            } else {
                out[PART ? P.out_row(0, vr - P.r0, vc) : vr * n + vc] = x;
            }
        }
        double* t = cur;
        cur = nxt;
        nxt = t;
    }
}


// ---- multigrid level 0 of the pressure hierarchy (matrix-free Gt_G): descent and ascent in one launch each ----
// k_gpre: x0 = c2_0 (b / diag) over the tile + 3, the Chebyshev sweep x1 over the tile + 2 (written on the tile), the
// residual r = b - Gt_G x1 over the tile + 1 (in LDS) and R_0 r on the tile's 32 x 4 coarse cells (cell-centred both
// ways).  k_gpost: x = x_in + P_0 x_c staged over the tile + 2, two Chebyshev sweeps from d = +0.0 (the restart of the
// post-smoothing), the last writing the tile (sub - x when sub is set).  k_gtg_solve's 512-lane layout (one tile cell
// and at most one ring cell per lane, the cell's five entries built once from thn), its rows and updates, the
// transfers' k_mg_transfer_spmv lists and orders, EpiResid's and EpiAdd's sums: bit-identical to the launches they
// replace (the first / plain / zero-direction sweeps, the residual, the restriction, the prolongation).
template <int KY, int KX, int W>
__device__ inline double g1_rw(const double* tf, int cr, int cc, int n, int rb, int cb);
template <bool PRE, bool SUB>
__global__ void __launch_bounds__(512) MPBP_LDS_READS
k_gtg_level0(GtGStencilDev P, const double* __restrict__ b, const double* __restrict__ diag, const double* __restrict__ xin,
             const double* __restrict__ xc, const double* __restrict__ sub, ChebK ck, double* __restrict__ x_out,
             double* __restrict__ bc) {
    constexpr int H = PRE ? 3 : 2;   // staged halo: the tile + H
    using G = GtgTile<H>;
    constexpr int CW = kGTW / 2 + 4, CH = kGTH / 2 + 4, CN = CW * CH;   // k_gpost's coarse window (k_gal1's geometry)
    static_assert(CW == kG1CW, "g1_p_in's window stride");
    __shared__ double ts[G::N], bs[G::N], xa[G::N], xb[G::N];
    __shared__ double cs[PRE ? 1 : CN];
    const int n = P.n, nc = n >> 1;
    const int tx = (n + kGTW - 1) / kGTW;
    const int bk = xcd_swizzle(blockIdx.x, gridDim.x);
    const int r0 = (bk / tx) * kGTH, c0 = (bk % tx) * kGTW;
    const int rb = r0 - H, cb = c0 - H;
    const int cr0 = r0 >> 1, cc0 = c0 >> 1;
    const int tid = threadIdx.x;
    auto wrapc = [&](int q) { return q < 0 ? q + nc : (q >= nc ? q - nc : q); };
    {
        constexpr int IT = (G::N + 511) / 512, IC = PRE ? 1 : (CN + 511) / 512;
        double bv[IT], tv[IT], wv[IT], cv[IC];
        if constexpr (!PRE) {
#pragma unroll
            for (int it = 0; it < IC; ++it) {
                const int i = tid + it * 512;
                if (i < CN) {
                    const int r = i / CW, c = i - r * CW;
                    cv[it] = xc[wrapc(cr0 - 2 + r) * nc + wrapc(cc0 - 2 + c)];
                }
            }
        }
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int i = tid + it * 512;
            if (i < G::N) {
                const int rr = i / G::RW, cc = i - rr * G::RW;
                const int32_t k = P.wrap(rb + rr) * n + P.wrap(cb + cc);
                bv[it] = b[k];
                tv[it] = P.cell[k];
                wv[it] = PRE ? diag[k] : xin[k];
            }
        }
        if constexpr (!PRE) {
#pragma unroll
            for (int it = 0; it < IC; ++it)
                if (tid + it * 512 < CN) cs[tid + it * 512] = cv[it];
            __syncthreads();
        }
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int i = tid + it * 512;
            if (i < G::N) {
                ts[i] = tv[it];
                bs[i] = bv[it];
                if constexpr (PRE) {
                    xa[i] = ck.c2[0] * (bv[it] / wv[it]);   // x0 (k_cheb_init's expression, XInit's)
                } else {                                     // x_in + P_0 x_c (the prolongation's sum)
                    const int rr = i / G::RW, cc = i - rr * G::RW;
                    const double pc = g1_inner(cr0, cc0, kGTH / 2, kGTW / 2, nc)
                                          ? g1_p_in<MPBP_MG_CELL, MPBP_MG_CELL>(cs, rr, cc)
                                          : g1_p<MPBP_MG_CELL, MPBP_MG_CELL>(cs, P.wrap(rb + rr), P.wrap(cb + cc), nc,
                                                                             cr0 - 2, cc0 - 2);
                    xa[i] = pc + wv[it];
                }
            }
        }
    }
    __syncthreads();
    const TTileT<G::RW> ta{ts, rb, cb};
    const int lr = tid >> 6, lc = tid & 63;
    // slot 0: the tile cell; slot 1: ring cell t of rings 1 .. H - 1 numbered ring 1 first
    int cr[2], cc[2], si[2], rr[2];
    bool own[2], edge[2];
    double e[2][5], bo[2], d[2];
    cr[0] = r0 + lr; cc[0] = c0 + lc; own[0] = true; rr[0] = 0;
    {
        int r = 0, j = tid;
#pragma unroll
        for (int q = 1; q < H; ++q)
            if (r == 0) {
                if (j < 140 + 8 * q) r = q;
                else j -= 140 + 8 * q;
            }
        own[1] = r != 0;
        rr[1] = r;
        fs_ring_cell(r ? r : 1, r ? j : 0, r0, c0, cr[1], cc[1]);
    }
#pragma unroll
    for (int sl = 0; sl < 2; ++sl) {
        const int vr = cr[sl], vc = cc[sl], gr = P.wrap(vr), gc = P.wrap(vc);
        si[sl] = (vr - rb) * G::RW + (vc - cb);
        edge[sl] = __builtin_amdgcn_readfirstlane(__any(own[sl] && (gr == 0 || gr == n - 1 || gc == 0 ||
                                                                    gc == n - 1))) != 0;
        if (own[sl]) {
            P.entries(vr, vc, gr, gc, ta, e[sl]);
            bo[sl] = bs[si[sl]];
            d[sl] = PRE ? xa[si[sl]] : 0.0;   // PRE: d0 = x0; post: the restart's +0.0
        }
    }
    double* cur = xa;
    double* nxt = xb;
    constexpr int L = PRE ? 2 : 2;   // PRE: the sweep, then the residual; post: two sweeps
#pragma unroll
    for (int l = 1; l <= L; ++l) {
        if (l > 1) __syncthreads();
        const double c1 = ck.c1[l], c2 = ck.c2[l];
#pragma unroll
        for (int sl = 0; sl < 2; ++sl) {
            // PRE: ring rr lives through level 3 - rr (the residual at level 2 covers the tile + 1); post: 2 - rr
            if (sl == 1 && (!own[1] || rr[1] > (PRE ? 3 : 2) - l)) continue;
            const int vr = cr[sl], vc = cc[sl];
            const int i = si[sl];
            const double p[5] = {e[sl][0] * cur[i - G::RW], e[sl][1] * cur[i - 1], e[sl][2] * cur[i],
                                 e[sl][3] * cur[i + 1], e[sl][4] * cur[i + G::RW]};
            const int gr = P.wrap(vr), gc = P.wrap(vc);
            const Wrap wr{gr == 0, gr == n - 1, gc == 0, gc == n - 1};
            const double acc = edge[sl] ? add5<true>(0.0, p, wr) : add5<false>(0.0, p, wr);
            if (PRE && l == 2) {   // the residual (EpiResid)
                nxt[i] = bo[sl] - acc;
                continue;
            }
            const double z = (bo[sl] - acc) / e[sl][2];
            const double dn = c1 * d[sl] + c2 * z;
            const double x = cur[i] + dn;
            nxt[i] = x;
            d[sl] = dn;
            const bool out = PRE ? (l == 1) : (l == L);
            if (sl == 0 && out && vr < n && vc < n) {
                const int32_t o = vr * n + vc;
                x_out[o] = (SUB && !PRE) ? sub[o] - x : x;
            }
        }
        double* t = cur;
        cur = nxt;
        nxt = t;
    }
    if constexpr (PRE) {   // R_0 r on the tile's coarse cells (cur holds r over the tile + 1)
        __syncthreads();
        constexpr int CTW = kGTW / 2, CTH = kGTH / 2;   // the tile's coarse cells
        if (tid < CTW * CTH) {
            const int crr = cr0 + tid / CTW, ccc = cc0 + tid % CTW;
            if (crr < nc && ccc < nc)
                bc[crr * nc + ccc] = g1_inner(cr0, cc0, CTH, CTW, nc)
                                         ? g1_rw_in<MPBP_MG_CELL, MPBP_MG_CELL, G::RW, 2>(cur, crr - cr0, ccc - cc0)
                                         : g1_rw<MPBP_MG_CELL, MPBP_MG_CELL, G::RW>(cur, crr, ccc, n, rb, cb);
        }
    }
}

}  // namespace
