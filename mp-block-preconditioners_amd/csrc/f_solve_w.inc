// k_fsolve on 32 x 16 tiles with the halo rings dealt out over the waves (k_fsolve_w, FsGeom), its gate and
// launcher, launch_fsolve, the launchers of the marching kernels (launch_march, launch_march2, launch_march_init),
// FStencilDev::row, FStencilDevM and with_f_policy / with_f_identities.
// Needs mpbp.hip's prelude and kernel sections (epilogues, F stencil, marching kernels and their launch geometry) and
// f_tile.inc (FsTile, FSolve, k_fsolve and its launcher).
// A fragment of mpbp.hip, included there once and in order: not a self-contained header.

namespace {

// ---- k_fsolve on narrower tiles with the halo rings spread evenly over the waves (kernel option f_solve_tile) ----
// The same whole-solve launch as k_fsolve, the same operations per cell and level (bit-identical), on a TW x TH tile
// (32 x 16: 10 % fewer cell-levels than 64 x 8 -- 2 680 instead of 2 968 per 512 outputs at H = 3 -- because the
// halo rings are shorter).  A level's time is set by the wave with the most owned cells it updates, so ring r's cells
// are dealt out in four equal contiguous runs, one per wave: rings 1 .. H - 1 share one slot (lanes 0 .. 51 of every
// wave at 32 x 16, H = 3), ring H (x0 only) a second.  Per wave and level: x0 on 4 cells (k_fsolve 64 x 8: 5), then
// 3, 3, 2 stencil cells (4, 3, 2), and three cells' state in registers instead of four.  The level-invariant part of
// the rows is computed once: the node averages K(r, c) into an LDS table (FStencilFast::coeffs' kc / ks / ke are
// K(r, c), K(r + 1, c), K(r, c + 1), the same sums in the same order), and each owned cell keeps its XI couplings and
// identity weights in registers (in place of its two face values), so a level reads 6 coefficients instead of 8
// thn values and skips ~27 of the row's ~115 fp64 operations.  Level 0 reads the table too (one more barrier, no node
// average computed twice); thn, x_p and the table are staged by wave-uniform rows, and an owned cell's global and LDS
// indices all derive from one wrapped (row, column) pair and one tile-relative (dr, dc) pair.  (An in-place variant -- one x image, a second barrier
// per level, 34 KB of LDS for three workgroups per CU -- spilled ~700 B per lane at the 168-VGPR cap and ran 4.5x
// slower: removed.)
template <int TW, int TH, int H>
struct FsGeom {
    static constexpr int RW = TW + 2 * H, RH = TH + 2 * H, N = RW * RH;   // x levels: the tile + H
    static constexpr int TSW = RW + 2, TSH = RH + 2, TSN = TSW * TSH;     // thn: the tile + H + 1
    static constexpr int NT = TW * TH / 256;                             // tile cells per lane
    static constexpr int ring(int r) { return 2 * TW + 2 * TH + 8 * r - 4; }
    static constexpr int q(int r) { return ring(r) / 4; }               // ring r's cells per wave
    static constexpr int qa() {                                          // slot A: rings 1 .. H - 1, per wave
        int s = 0;
        for (int r = 1; r < H; ++r) s += q(r);
        return s;
    }
};
template <int TW, int TH>
__device__ inline void fs_ring_cell_t(int r, int j, int r0, int c0, int& vr, int& vc) {
    const int w = TW + 2 * r;
    if (j < 2 * w) {
        vr = j < w ? r0 - r : r0 + TH - 1 + r;
        vc = c0 - r + (j < w ? j : j - w);
    } else {
        const int k = j - 2 * w;
        vr = r0 - r + 1 + (k >> 1);
        vc = (k & 1) ? c0 + TW - 1 + r : c0 - r;
    }
}
// the same cell of ring r (a constant where it is called) as offsets from the corner of the tile + h
template <int TW, int TH>
__device__ inline void fs_ring_rel(int r, int j, int h, int& dr, int& dc) {
    const int w = TW + 2 * r, k = j - 2 * w;
    const bool top = j < w, row = j < 2 * w;
    dr = h + (row ? (top ? -r : TH - 1 + r) : 1 - r + (k >> 1));
    dc = h + (row ? (top ? j : j - w) - r : ((k & 1) ? TW - 1 + r : -r));
}
// base[off / 8] with base wave-uniform and off a 32-bit byte offset: the scalar-base form of the global access
template <class V>
__device__ inline V* at_off(V* base, uint32_t off) { return (V*)((const char*)base + off); }
__device__ inline double ld_off(const double* base, uint32_t off) { return *at_off(base, off); }
template <int W>
struct TRelT {   // staged thn around one cell: t points at it, W columns per staged row
    const double* t;
    __device__ double T(int sph, int r, int c) const {
        const double v = t[r * W + c];
        return sph ? 1.0 - v : v;
    }
};
template <int W, int N>
struct XRelT {   // 4 fields ([4][N], W columns per row) around one cell: x points at its field-0 entry
    const double* x;
    __device__ double X(int f, int r, int c) const { return x[f * N + r * W + c]; }
};
template <int TW, int TH, int H, bool SUB, bool PART, class BS>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 8))) MPBP_LDS_READS
k_fsolve_w(FStencilFast P, FSolve a, BS bs) {
    using T = FsGeom<TW, TH, H>;
    static_assert(TW * TH == 256 * T::NT && TW % 32 == 0, "whole rows of 32 lanes, NT cells per lane");
    static_assert((2 * TW + 2 * TH - 4) % 4 == 0, "every ring splits into four equal runs");
    static_assert(T::qa() <= 64 && T::q(H) <= 64, "one ring slot for rings 1 .. H - 1 and one for ring H");
    constexpr int NT = T::NT;
    constexpr int NSL = NT + 2;   // owned cells per lane: NT tile cells, slot A (rings 1 .. H - 1), slot B (ring H)
    constexpr int NS = NT + 1;    // ... with updates after x0 (ring H only needs x0)
    constexpr int PW = T::RW + 1, PH = T::RH + 1, PN = PW * PH;   // BS: x_p over the tile + H, + its west / north neighbours
    // node averages K(r, c) of the tile + H, + 1 row / column: ks / ke of every level-0 cell, ring H included
    constexpr int KW = T::RW + 1, KN = KW * (T::RH + 1);
    static_assert(T::TSW <= 64 && PW == KW, "a staged row is one wave's lanes; x_p's window and the K table share indices");
    __shared__ double ts[T::TSN];
    __shared__ double kt[KN];
    __shared__ double xa[4 * T::N], xb[4 * T::N];
    __shared__ double ps[BS::on ? PN : 1];
    const int n = P.n, nn = n * n;
    const int tx = (n + TW - 1) / TW;
    const int bk = xcd_swizzle(blockIdx.x, gridDim.x);
    const int lo = PART ? P.r0 - P.ext : 0, hi = PART ? P.r0 + P.L + P.ext : n;   // output rows [lo, hi)
    const int r0 = lo + (bk / tx) * TH, c0 = (bk % tx) * TW;
    const int rbt = r0 - H - 1, cbt = c0 - H - 1, rb = r0 - H, cb = c0 - H;
    const int tid = threadIdx.x;
    auto in_row = [&](int vr, int h) {
        if constexpr (PART) {
            const int lr = vr - P.r0;
            return lr < -h ? -h : (lr >= P.L + h ? P.L + h - 1 : lr);
        } else {
            return P.wrap(vr);
        }
    };
    // Staging by rows: wave w takes staged rows w, w + 4, ..., lane l column l.  A row's wrapped global base is
    // scalar work, the wrapped column is the lane's own for every row (x_p's window starts at the same (rbt, cbt)), and
    // an iteration is one load or one LDS store at an immediate offset from the lane's base.
    const int lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6) & 3;
    const uint32_t gcs = 8u * (uint32_t)P.wrap(cbt + (lane < T::TSW ? lane : 0));   // (byte offsets: n n 8 < 2^32)
    if (lane < T::TSW) {
        constexpr int IT = (T::TSH + 3) / 4;
        double v[IT];
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int sr = wv + 4 * it;
            if (sr < T::TSH) v[it] = ld_off(P.cell + P.wrap(rbt + sr) * n, gcs);
        }
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int sr = wv + 4 * it;
            if (sr < T::TSH) ts[sr * T::TSW + lane] = v[it];
        }
    }
    if constexpr (BS::on) {
        if (lane < PW) {
            constexpr int IT = (PH + 3) / 4;
            double v[IT];
#pragma unroll
            for (int it = 0; it < IT; ++it) {
                const int sr = wv + 4 * it;
                if (sr < PH) {
                    const int pr = in_row(rbt + sr, PART ? bs.h : 0);
                    v[it] = ld_off(bs.xp + (PART ? ext_row(1, 0, pr, P.L, bs.h, n) : pr * n), gcs);
                }
            }
#pragma unroll
            for (int it = 0; it < IT; ++it) {
                const int sr = wv + 4 * it;
                if (sr < PH) ps[sr * PW + lane] = v[it];
            }
        }
    }
    // owned cells at (dr, dc) from the corner (rb, cb) of the tile + H: one LDS index per cell, neighbours at
    // immediate offsets (xi: the x levels, xi + dr: the K table and x_p, xi + 2 dr + TSW + 1: thn)
    int dr[NSL], dc[NSL];
#pragma unroll
    for (int m = 0; m < NT; ++m) {   // tile cell m: row (tid / TW) + m (256 / TW), column tid % TW
        dr[m] = H + tid / TW + m * (256 / TW); dc[m] = H + tid % TW;
    }
    // slot A: rings 1 .. H - 1 in consecutive lane ranges (the ring is the range's: compile time); slot B: ring H
    int rA = 0;   // slot A's ring, 0: none
    dr[NT] = H; dc[NT] = H;
    {
        int base = 0;
#pragma unroll
        for (int q = 1; q < H; ++q) {
            if (lane >= base && lane < base + T::q(q)) {
                fs_ring_rel<TW, TH>(q, wv * T::q(q) + lane - base, H, dr[NT], dc[NT]);
                rA = q;
            }
            base += T::q(q);
        }
    }
    const bool ownB = lane < T::q(H);
    fs_ring_rel<TW, TH>(H, ownB ? wv * T::q(H) + lane : 0, H, dr[NT + 1], dc[NT + 1]);
    auto own = [&](int sl) { return sl < NT || (sl == NT ? rA != 0 : ownB); };
    // one wrapped (gr, gc) and k = gr n + gc per cell: faces, b, sub and the output (a tile cell inside the grid is
    // its own wrapped cell) index from it: a 32-bit byte offset from the field's base (n n 8 < 2^32)
    constexpr bool LB = !BS::on || BS::resid;   // b (BNone) or z (GxR) loaded per owned cell
    static_assert(!(BS::resid && (PART || SUB)), "GxR: one GPU, no sub");
    double fl[NSL][2], bl[LB ? NSL : 1][4];
    uint32_t kg[NSL];
    bool ww[NSL], wn[NSL], outok[NT];
#pragma unroll
    for (int sl = 0; sl < NSL; ++sl) {
        if (!own(sl)) continue;
        const int vr = rb + dr[sl], vc = cb + dc[sl];
        // (a tile cell's column is never negative, nor its row on the whole grid)
        const int gr = !PART && sl < NT ? (vr >= n ? vr - n : vr) : P.wrap(vr);
        const int gc = sl < NT ? (vc >= n ? vc - n : vc) : P.wrap(vc);
        kg[sl] = 8u * (uint32_t)(gr * n + gc);
        ww[sl] = gc == 0;
        wn[sl] = gr == 0;
        if (sl < NT) outok[sl < NT ? sl : 0] = vr < hi && vc < n;   // else a tile past the last row / column
        fl[sl][0] = ld_off(P.uface, kg[sl]);
        fl[sl][1] = ld_off(P.vface, kg[sl]);
        if constexpr (BS::resid) {
#pragma unroll
            for (int f = 0; f < 4; ++f) bl[sl][f] = ld_off(bs.z + (size_t)f * nn, kg[sl]);
        } else if constexpr (!BS::on) {
            if constexpr (PART) {
                const int br = in_row(vr, P.h);
#pragma unroll
                for (int f = 0; f < 4; ++f) bl[sl][f] = a.b[ext_row(4, f, br, P.L, P.h, n) + gc];
            } else {
#pragma unroll
                for (int f = 0; f < 4; ++f) bl[sl][f] = ld_off(a.b + (size_t)f * nn, kg[sl]);
            }
        }
    }
    __syncthreads();
    // the node averages every level reads (FStencilFast::coeffs' kc of cell (r, c), ks of (r - 1, c), ke of (r, c - 1):
    // the same sum in the same order), computed once, by rows as the staging; level 0 reads them too
    if (lane < KW) {
        constexpr int IK = (T::RH + 1 + 3) / 4;
#pragma unroll
        for (int it = 0; it < IK; ++it) {
            const int kr = wv + 4 * it;
            if (kr < T::RH + 1) {
                const double* t = ts + kr * T::TSW + lane;   // thn(rb + kr - 1, cb + lane - 1)
                kt[kr * KW + lane] = 0.25 * ((t[0] + t[1]) + (t[T::TSW] + t[T::TSW + 1]));
            }
        }
    }
    __syncthreads();
    // per owned cell: d, its reciprocal diagonals, b, and the level-invariant row terms (XI couplings xu / xv, weights)
    double d[NS][4], rd[NS][4], bv[NS][4], kx[NS][2];
    typename FStencilFast::W4 wt[NS];
    // level 0: x0 = d0 = c2_0 b / diag over the tile + H
#pragma unroll
    for (int sl = 0; sl < NSL; ++sl) {
        if (!own(sl)) continue;
        const int si = dr[sl] * T::RW + dc[sl], ki = si + dr[sl];
        const double* t = ts + (ki + dr[sl] + T::TSW + 1);   // thn at the cell
        const FStencilDev::Cell cl{{fl[sl][0], fl[sl][1]}};
        const double tw = t[-1], tc = t[0], tn = t[-T::TSW];
        const typename FStencilFast::Co k = P.coeffs_k(tw, tc, tn, tw + tc, kt[ki], kt[ki + KW], kt[ki + 1]);
        const typename FStencilFast::W4 w = P.weights(cl);
        double b4[4], r4[4];
        P.rdiag4_co(k, w, r4);
        if constexpr (BS::on) {
            const int pi = ki + PW + 1;
            const typename BS::Q q{ps[pi], ps[pi - 1], ps[pi - PW]};
#pragma unroll
            for (int f = 0; f < 4; ++f) {
                b4[f] = bs.b_at(f, 0, 0, ww[sl], wn[sl], TRelT<T::TSW>{t}, q);
                if constexpr (BS::resid) b4[f] = bl[sl][f] - b4[f];   // z - (G x_p), EpiResid's subtraction
            }
        } else {
#pragma unroll
            for (int f = 0; f < 4; ++f) b4[f] = bl[sl][f];
        }
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            const double x0 = a.c2_0 * b4[f] * r4[f];
            xa[f * T::N + si] = x0;
            if (sl < NS) {
                d[sl][f] = x0;
                rd[sl][f] = r4[f];
                bv[sl][f] = b4[f];
            }
        }
        if (sl < NS) {
            kx[sl][0] = k.xu;
            kx[sl][1] = k.xv;
            wt[sl] = w;
        }
    }
    double* cur = xa;
    double* nxt = xb;
    double sv[NT][4];
#pragma unroll
    for (int l = 1; l <= H; ++l) {
        __syncthreads();
        const double c1 = a.c1[l - 1], c2 = a.c2[l - 1];
        // tile cell m's entry of field f in the output's layout (the row partition keeps its layout's own addressing)
        auto out_at = [&](auto* v, int m, int f) {
            if constexpr (PART) return v + P.out_row(f, rb + dr[m] - P.r0, cb + dc[m]);
            else return at_off(v + (size_t)f * nn, kg[m]);
        };
        if constexpr (SUB) {
            if (l == H) {
#pragma unroll
                for (int m = 0; m < NT; ++m) {
                    if (!outok[m]) continue;
#pragma unroll
                    for (int f = 0; f < 4; ++f) sv[m][f] = *out_at(a.sub, m, f);
                }
            }
        }
#pragma unroll
        for (int sl = 0; sl < NS; ++sl) {
            if (sl >= NT && (l == H || rA == 0 || rA > H - l)) continue;   // ring r lives through level H - r
            if (l == H && !outok[sl < NT ? sl : 0]) continue;
            const int si = dr[sl] * T::RW + dc[sl], ki = si + dr[sl];
            const double* t = ts + (ki + dr[sl] + T::TSW + 1);
            typename FStencilFast::Co k;
            k.w = t[-1];
            k.c = t[0];
            k.nn = t[-T::TSW];
            k.kc = kt[ki];
            k.ks = kt[ki + KW];
            k.ke = kt[ki + 1];
            k.xu = kx[sl][0];
            k.xv = kx[sl][1];
            double acc[4];
            P.rows4_co(0, 0, k, wt[sl], XRelT<T::RW, T::N>{cur + si}, acc);
#pragma unroll
            for (int f = 0; f < 4; ++f) {
                const double z = (bv[sl][f] - acc[f]) * rd[sl][f];
                const double dn = c1 * d[sl][f] + c2 * z;
                if (l < H) {
                    nxt[f * T::N + si] = cur[f * T::N + si] + dn;
                    d[sl][f] = dn;
                } else {
                    const double x = cur[f * T::N + si] + dn;
                    if constexpr (SUB) *out_at(a.x_out, sl < NT ? sl : 0, f) = sv[sl < NT ? sl : 0][f] - x;
                    else *out_at(a.x_out, sl < NT ? sl : 0, f) = x;
                }
            }
        }
        double* t = cur;
        cur = nxt;
        nxt = t;
    }
}
// Grids the narrow tile's staged thn (tile + H + 1 each side) wraps onto at most once.
template <int TW, int TH, int H>
inline bool fsolve_w_ok_n(int n) { return n >= FsGeom<TW, TH, H>::TSW && n >= FsGeom<TW, TH, H>::TSH; }
template <int H, bool PART, class BS>
int launch_fsolve_w(const FStencilFast& P, const FSolve& a, hipStream_t st, const BS& bs) {
    constexpr int TW = 32, TH = 16;
    const int rows = PART ? P.L + 2 * P.ext : P.n;
    const int64_t tiles = (int64_t)((P.n + TW - 1) / TW) * ((rows + TH - 1) / TH);
    if constexpr (BS::resid) {   // GxR: the upper block form's solve, never subtracted from anything
        if (a.sub) return set_error(MPBP_ERR_ARG, "fsolve: the z - G x_p right-hand side takes no sub");
        k_fsolve_w<TW, TH, H, false, PART, BS><<<(unsigned)tiles, 256, 0, st>>>(P, a, bs);
    } else {
    if (a.sub) k_fsolve_w<TW, TH, H, true, PART, BS><<<(unsigned)tiles, 256, 0, st>>>(P, a, bs);
    else k_fsolve_w<TW, TH, H, false, PART, BS><<<(unsigned)tiles, 256, 0, st>>>(P, a, bs);
    }
    MPBP_HIP(hipGetLastError());
    return MPBP_OK;
}

// K = 3 or 4 Chebyshev updates (x0 and H = K - 1 stencil sweeps); columns wrap at most once per tile.
inline bool fsolve_ok(int K, int n) { return (K == 3 && fsolve_ok_n<2>(n)) || (K == 4 && fsolve_ok_n<3>(n)); }
// One GPU, whole grid (P.h == 0), or a row partition's owned rows + P.ext ghost rows (P.which == 3), b's ghost depth
// P.h >= P.ext + H (+ 1 for x_p's with GxBPart).
template <class BS = BNone>
int launch_fsolve(const FStencilDev& Pd, int K, const double* c1, const double* c2, const double* b, const double* sub,
                  double* x_out, hipStream_t st, const BS& bs = BS{}) {
    const FStencilFast P{Pd};
    const bool part = P.h != 0;
    int xp_h = 0;   // x_p's ghost depth (GxBPart)
    if constexpr (BS::on) {
        if (BS::part != part) return set_error(MPBP_ERR_ARG, "fsolve: G x_p's layout does not match F's");
        if constexpr (BS::part) xp_h = bs.h;
    }
    if (!fsolve_ok(K, P.n) || (!part && P.which != 0) ||
        (part && (P.which != 3 || P.h < P.ext + K - 1 || P.oh < P.ext || (BS::on && xp_h < P.ext + K))))
        return set_error(MPBP_ERR_ARG, "fsolve: one GPU whole grid, or owned + ext rows with b ext + K - 1 deep");
    if (!x_out || (!BS::on && !b) || x_out == b) return set_error(MPBP_ERR_ARG, "fsolve: bad vectors");
    if constexpr (BS::resid) {
        if (!bs.z || bs.z == x_out || part) return set_error(MPBP_ERR_ARG, "fsolve: z - G x_p needs z apart from x, one GPU");
    }
    FSolve a{b, sub, x_out, c2[0], {}, {}};
    for (int l = 1; l < K; ++l) {
        a.c1[l - 1] = c1[l];
        a.c2[l - 1] = c2[l];
    }
    constexpr bool bpart = BS::on && BS::part;   // GxBPart launches only the partitioned kernel, GxB the other
    if (KO().f_solve_tile) {   // 32 x 16 tiles, rings spread over the waves, level-invariant terms cached
        if (!(K == 3 ? fsolve_w_ok_n<32, 16, 2>(P.n) : fsolve_w_ok_n<32, 16, 3>(P.n)))
            return set_error(MPBP_ERR_ARG, "fsolve: grid smaller than the 32 x 16 tile's staging");
        if constexpr (BS::on) {
            return K == 3 ? launch_fsolve_w<2, bpart>(P, a, st, bs) : launch_fsolve_w<3, bpart>(P, a, st, bs);
        } else {
            if (part) return K == 3 ? launch_fsolve_w<2, true>(P, a, st, bs) : launch_fsolve_w<3, true>(P, a, st, bs);
            return K == 3 ? launch_fsolve_w<2, false>(P, a, st, bs) : launch_fsolve_w<3, false>(P, a, st, bs);
        }
    }
    if constexpr (BS::on) {
        return K == 3 ? launch_fsolve_t<2, bpart>(P, a, st, bs) : launch_fsolve_t<3, bpart>(P, a, st, bs);
    } else {
        if (part) return K == 3 ? launch_fsolve_t<2, true>(P, a, st, bs) : launch_fsolve_t<3, true>(P, a, st, bs);
        return K == 3 ? launch_fsolve_t<2, false>(P, a, st, bs) : launch_fsolve_t<3, false>(P, a, st, bs);
    }
}

// Sweeps s, s+1 of an F Chebyshev solve fused (k_march2, tolerance mode) over the rows P.which selects (0: the whole
// grid, 3: owned + ext ghost rows; level A then covers ext + 1).  d_in may be d_out only when the pair does not store
// its direction (SD false): level A reads d_in on its neighbours' rows and columns.
template <bool SUB, bool SD, class BS>
int launch_march2_t(const FStencilFast& P, const Fused2& a, hipStream_t st, const BS& bs) {
    const int64_t chunks = march_chunks(P, KO().march_rows, march_capacity<k_march2<SUB, SD, BS>>());
    if (chunks == 0) return MPBP_OK;
    const int64_t strips = (P.n + kMB - 1) / kMB;
    k_march2<SUB, SD, BS><<<(unsigned)(chunks * strips), kMB, 0, st>>>(P, a, (int)chunks, bs);
    MPBP_HIP(hipGetLastError());
    return MPBP_OK;
}
template <class BS = BNone>
int launch_march2(const FStencilDev& Pd, const Fused2& a, hipStream_t st, const BS& bs = BS{}) {
    const FStencilFast P{Pd};
    if (P.which == 1 || P.which == 2) return set_error(MPBP_ERR_ARG, "march2: interior / boundary row splits unsupported");
    if (!a.x_in || !a.d_in || !a.x_out || a.x_in == a.x_out || (!BS::on && !a.b) || (a.d_out && a.d_out == a.d_in))
        return set_error(MPBP_ERR_ARG, "march2: bad vectors");
    const bool sub = a.sub != nullptr, sd = a.d_out != nullptr;
    return sub ? (sd ? launch_march2_t<true, true>(P, a, st, bs) : launch_march2_t<true, false>(P, a, st, bs))
               : (sd ? launch_march2_t<false, true>(P, a, st, bs) : launch_march2_t<false, false>(P, a, st, bs));
}

// The first inner sweep with x0 = c2 b / diag staged and diag rebuilt from thn (k_march_init).  BS = GxB: b is
// W = G x_p recomputed per point (the second F solve of the apply).
template <class S, class Epi, class BS = BNone>
int launch_march_init(const S& P, const double* b, double c2, Epi epi, int rows_per_block, hipStream_t st,
                      const BS& bs = BS{}) {
    auto go = [&](const auto& e) {
        using E = std::decay_t<decltype(e)>;
        const int64_t chunks = march_chunks(P, rows_per_block, march_capacity<k_march_init<S, E, BS>>());
        if (chunks == 0) return (int)MPBP_OK;
        const int64_t strips = (P.n + kMB - 1) / kMB;
        k_march_init<S, E, BS><<<(unsigned)(chunks * strips), kMB, 0, st>>>(P, b, c2, (int)chunks, e, bs);
        MPBP_HIP(hipGetLastError());
        return (int)MPBP_OK;
    };
    if constexpr (BS::on) return with_fixed_epi_bx<S::kFast>(epi, go);
    else return with_fixed_epi<S::kFast>(epi, go);
}

template <class S, class XS, class Epi, class BS = BNone>
int launch_march(const S& P, const XS& xs, Epi epi, int rows_per_block, hipStream_t st, const BS& bs = BS{}) {
    auto go = [&](const auto& e) { return launch_march_fixed(P, xs, e, rows_per_block, st, bs); };
    if constexpr (BS::on) return with_fixed_epi_bx<S::kFast>(epi, go);
    else return with_fixed_epi<S::kFast>(epi, go);
}

// F row of field f at a cell (k_march policy).
template <bool EDGE, class TA, class XA>
__device__ inline double FStencilDev::row(int f, int gr, int gc, const TA& ta, const XA& xa, double* fd,
                                          const Cell& cl) const {
    return f_row<EDGE>(*this, f, gr, gc, ta, xa, fd, cl.face);
}

// The F policy with the parameter identities of f_row's M compiled in (the reference's own parameters,
// d_u = -1 and eta_s = 1, solve.py:292-297 / apply.py:33-35): fewer fp64 multiplies per row, same bits.
template <int M>
struct FStencilDevM : FStencilDev {
    template <bool EDGE, class TA, class XA>
    __device__ double row(int f, int gr, int gc, const TA& ta, const XA& xa, double* fd, const Cell& cl) const {
        return f_row<EDGE, TA, XA, false, M>(*this, f, gr, gc, ta, xa, fd, cl.face);
    }
    template <class TA>
    __device__ double stage_diag(int f, int gr, int gc, const TA& ta, const Stage& s) const {
        return f_stage_diag<M>(*this, f, gr, gc, ta, s);
    }
};

// Calls fn with the F policy the plan's numerics select: the tolerance-mode rows (fast) or the bit-exact rows
// specialised for P's parameter identities.
template <class Fn>
int with_f_identities(const FStencilDev& P, Fn&& fn);
template <class Fn>
int with_f_policy(const FStencilDev& P, bool fast, Fn&& fn) {
    if (fast) return fn(FStencilFast{P});
    return with_f_identities(P, fn);
}

// Calls fn with the F policy specialised for P's parameters (M = 0: none apply).
template <class Fn>
int with_f_identities(const FStencilDev& P, Fn&& fn) {
    if (P.d_u == -1.0 && P.eta_s == 1.0) {
        if (P.eta_n != 1.0 && P.pow2 && P.ce0 != 0.0 && __builtin_isfinite(P.ce0)) return fn(FStencilDevM<13>{P});
        return P.eta_n == 1.0 ? fn(FStencilDevM<7>{P}) : fn(FStencilDevM<5>{P});
    }
    return fn(P);
}

}  // namespace
